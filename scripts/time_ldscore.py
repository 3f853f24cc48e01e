"""Time the LD scores (`ldscore_packed`) and the per-sample counts of `jx gstats` on one GPU, on the LD panel of
`scripts/time_ldprune.py` synthesised in HBM.

    python scripts/time_ldscore.py [--n 20000] [--m 200000] [--reps 3] [--missing 0.0] [--out profiles/ldscore_time.json]

Windows: `100` and `1000` variants, `100kb`.  Per window: the score launches over all row ranges (`jxg_ld_score_p32`: memset, the
two forms, the reduce; ms, median of --reps after one warm-up, device events), the wall time of the window-bounds host call
(`jx_ldsc_window_bounds`) and of the whole call (median of --reps warm calls; it includes the P32 re-tiling of the payload, the
row counts and the copy of the scores), the 32 x 32 blocks computed by form and the share of their pairs that lie in a window.
In the same run `jxg_ld_band_mask_p32` is timed over the band of the same one-sided reach (band_end = the window's end): the
score kernel computes the band two-sided, about twice those blocks, so the figure to read is score / (2 x mask).  Then the
sample-count kernel (`jxg_sample_counts_p32`): ms and the bytes it must read (m x tiles x 32) as a fraction of 6.29 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402
from time_ldprune import HBM_BPS, I8_PEAK, ld_panel_gpu  # noqa: E402


def _events(fn, reps):
    """Median device time (ms) of fn() over `reps` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def _score_blocks(start, end, hasmiss):
    """32 x 32 blocks the score kernel computes, by form, and the pairs of a window among their pairs."""
    m = len(start)
    edges = np.arange(0, m, 32)
    jb0 = np.minimum.reduceat(start, edges) // 32
    jb1 = (np.maximum.reduceat(end, edges) - 1) // 32
    blk_miss = np.maximum.reduceat(hasmiss.astype(np.int64), edges) > 0
    cum = np.concatenate([[0], np.cumsum(blk_miss)])
    six = 0
    for b in range(len(edges)):
        six += int(jb1[b] - jb0[b] + 1) if blk_miss[b] else int(cum[jb1[b] + 1] - cum[jb0[b]])
    total = int((jb1 - jb0 + 1).sum())
    return total - six, six, int((end - start - 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--missing", type=float, default=0.0, help="missing-call rate on every second row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldscore_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    packed, pos = ld_panel_gpu(n, m, 42, dev, a.missing)
    torch.cuda.synchronize()
    rec = {"n": n, "m": m, "missing": a.missing, "windows": []}
    chrom = np.zeros(m, dtype=np.int32)
    panel = jx._panel(packed, n)
    counts = panel.counts().astype(np.int64)
    mean, std, maf, hasmiss = jx._ld_row_stats(counts, n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    mean_t, std_t, miss_t = up(mean), up(std), up(hasmiss.astype(np.uint8))
    self_t = up((((n - counts[:, 0]) > 1) & (maf > 0.0)).astype(np.float64))
    npad = panel.nt * 128
    for name, kind, value in (("100", "variants", 100), ("1000", "variants", 1000), ("100kb", "bp", 100000)):
        code, w_int, w_cm = jx._ldsc_parse_window(kind, value)
        tb = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _order, _off, start, end = jx._ldsc_window_bounds(chrom, pos, None, code, w_int, w_cm)
            tb.append(time.perf_counter() - t0)
        ranges = jx._ldsc_ranges(start, end, jx.LDSC_PARTIAL_BUDGET_BYTES)
        start_t, end_t = up(start.astype(np.int32)), up(end.astype(np.int32))
        part_t = torch.empty(max((r1 - r0) * npb for r0, r1, npb in ranges), dtype=torch.float64, device=dev)
        score_t = torch.empty(m, dtype=torch.float64, device=dev)

        def score():
            for r0, r1, npb in ranges:
                check(lib().jxg_ld_score_p32(_ptr(panel.p32), m, n, None, m, r0, r1, _ptr(start_t), _ptr(end_t), _ptr(mean_t),
                                             _ptr(std_t), _ptr(miss_t), _ptr(self_t), npb, _ptr(part_t), _ptr(score_t), _stream()))
        score_ms = _events(score, a.reps)
        # the mask kernel of the parent code over the band of the same one-sided reach
        idx = np.arange(m, dtype=np.int64)
        wpr = max(1, (int((end - idx - 1).max()) + 31) // 32)
        rows_cap = max(32, min(jx.LD_MASK_BUDGET_BYTES // (4 * wpr), 1 << 20))
        band_t = up(end.astype(np.int32))
        mask_t = torch.empty(min(rows_cap, m) * wpr, dtype=torch.int32, device=dev)

        def mask():
            for r0 in range(0, m, rows_cap):
                check(lib().jxg_ld_band_mask_p32(_ptr(panel.p32), m, n, None, m, r0, min(m, r0 + rows_cap), _ptr(band_t),
                                                 _ptr(mean_t), _ptr(std_t), _ptr(miss_t), 0.2, wpr, _ptr(mask_t), _stream()))
        mask_ms = _events(mask, a.reps)
        whole = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            _m, ldsc = jx.ldscore_packed(packed, n, chrom, pos, None, kind, value)
            whole.append(time.perf_counter() - t0)
        clean, six, useful = _score_blocks(start, end, hasmiss)
        ops = 2.0 * 1024 * npad * (clean + 6 * six)
        r = {"window": name, "ranges": len(ranges), "partials_per_row": max(npb for *_x, npb in ranges),
             "partial_bytes": int(sum((r1 - r0) * npb * 8 for r0, r1, npb in ranges)), "mean_M": round(float((end - start).mean()), 1),
             "mean_ldsc": round(float(ldsc.mean()), 3), "score_ms": round(score_ms, 2), "mask_ms_same_reach": round(mask_ms, 2),
             "score_over_twice_mask": round(score_ms / (2.0 * mask_ms), 3), "bounds_s": round(float(np.median(tb)), 4),
             "whole_call_s": round(float(np.median(whole[1:])), 3), "blocks_clean": clean, "blocks_six": six,
             "useful_pair_share": round(useful / (1024.0 * max(clean + six, 1)), 3),
             "int8_fraction": round(ops / (score_ms * 1e-3) / I8_PEAK, 4)}
        print(json.dumps(r), flush=True)
        rec["windows"].append(r)
    out_t = torch.empty((2, n), dtype=torch.int32, device=dev)
    ms = _events(lambda: check(lib().jxg_sample_counts_p32(_ptr(panel.p32), m, n, _ptr(out_t), _stream())), max(a.reps, 5))
    nbytes = float(m) * panel.nt * 32
    rec["sample_counts"] = {"kernel_ms": round(ms, 3), "bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_BPS, 4),
                            "snp_chunk": int(lib().jxg_sample_counts_chunk()),
                            "workgroups": int(-(-m // lib().jxg_sample_counts_chunk())) * panel.nt}
    print(json.dumps(rec["sample_counts"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
