"""Time LD pruning (`bed_packed_ld_prune_maf_priority`) on one GPU: the band-mask kernel (`jxg_ld_band_mask_p32`), the host greedy
(`jx_ld_prune_greedy`) and the whole call, on a panel synthesised in HBM.

    python scripts/time_ldprune.py [--n 20000] [--m 200000] [--reps 3] [--missing 0.0] [--out profiles/ldprune_time.json]

The panel has LD: blocks of 8 SNPs, each SNP a copy of the one before with 10 % of the haplotype entries redrawn, positions
cumulative sums of integers in [1, 2000) on one chromosome (independent SNPs would prune nothing and keep the greedy in its
longest scans).  Parameter sets: `50 5 0.2`, `500 50 0.2`, `500kb 50 0.2`.  Per set: the kernel over all SNP ranges (ms, median
of --reps after one warm-up, device events, mask copies excluded), the wall time of the host greedy and of the whole call
(median of --reps warm calls; the whole call includes the P32 re-tiling of the payload and the row counts, also timed on their
own, the mask copies and the greedy), the 32 x 32 blocks the kernel computed by form, the share of their pairs that lie in
the band (useful work), the int8 operation rate (2 operations per sample, pair and product of the blocks computed) as a fraction
of the 5.0 POP/s dense int8 peak, and the payload bytes the waves asked for (each wave streams its 64 rows once over the
samples; a row is asked for by every block that holds it, the L2 serves the repeats) as a fraction of 6.29 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402

HBM_BPS = 6.29e12
I8_PEAK = 5.0e15


def ld_panel_gpu(n, m, seed, dev, missing_rate=0.0):
    """(m, ceil(n / 4)) uint8 payload in HBM of the LD panel above, and its positions."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    bps = (n + 3) // 4
    mb = (m + 7) // 8                                         # blocks of 8 SNPs
    out = torch.empty((mb * 8, bps), dtype=torch.uint8, device=dev)
    chunk = max(1, (1 << 26) // max(n, 1))                    # blocks per pass
    for c0 in range(0, mb, chunk):
        nb = min(chunk, mb - c0)
        p = 0.05 + 0.45 * torch.rand((nb, 1, 1), generator=gen, device=dev)
        hap = torch.rand((nb, 2, n), generator=gen, device=dev) < p
        view = out[c0 * 8:(c0 + nb) * 8].view(nb, 8, bps)
        for k in range(8):
            if k:
                redraw = torch.rand((nb, 2, n), generator=gen, device=dev) < 0.1
                hap = torch.where(redraw, torch.rand((nb, 2, n), generator=gen, device=dev) < p, hap)
            d = hap[:, 0].to(torch.uint8) + hap[:, 1].to(torch.uint8)
            c = torch.where(d == 0, 0, d + 1).to(torch.uint8)
            if missing_rate > 0 and k % 2:
                c = torch.where(torch.rand((nb, n), generator=gen, device=dev) < missing_rate, torch.ones_like(c), c)
            c4 = torch.nn.functional.pad(c, (0, bps * 4 - n)).view(nb, bps, 4)
            view[:, k] = c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)
    out = out[:m].contiguous() if mb * 8 != m else out
    pos = np.cumsum(np.random.default_rng(seed).integers(1, 2000, size=m)).astype(np.int64)
    return out, pos


def _blocks(ranges, band_end, hasmiss):
    """32 x 32 blocks the kernel computes over the ranges, by form, and the pairs of the band among their pairs."""
    m = len(band_end)
    clean = six = useful = 0
    for a, _ws1, r1, wpr in ranges:
        for i0 in range(a, r1, 32):
            i1 = min(i0 + 32, r1)
            be = min(int(band_end[i0:i1].max()), m)
            mi = bool(hasmiss[i0:i1].any())
            for x in range(wpr + 1):
                j0 = i0 + 32 * x
                if j0 >= be or j0 >= m:
                    break
                if mi or bool(hasmiss[j0:j0 + 32].any()):
                    six += 1
                else:
                    clean += 1
            idx = np.arange(i0, i1)
            useful += int(np.minimum(band_end[i0:i1], idx + 1 + 32 * wpr).sum() - (idx + 1).sum())
    return clean, six, useful


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--missing", type=float, default=0.0, help="missing-call rate on every second row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldprune_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    t0 = time.perf_counter()
    packed, pos = ld_panel_gpu(n, m, 42, dev, a.missing)
    torch.cuda.synchronize()
    rec = {"n": n, "m": m, "missing": a.missing, "synth_s": round(time.perf_counter() - t0, 2), "sets": []}
    chrom = np.zeros(m, dtype=np.int32)
    t0 = time.perf_counter()
    panel = jx._panel(packed, n)
    counts = panel.counts()
    torch.cuda.synchronize()
    rec["panel_s"] = round(time.perf_counter() - t0, 3)
    mean, std, _maf, hasmiss = jx._ld_row_stats(counts, n)
    mean_t, std_t = torch.from_numpy(mean).to(dev), torch.from_numpy(std).to(dev)
    miss_t = torch.from_numpy(hasmiss.astype(np.uint8)).to(dev)
    npad = panel.nt * 128
    for name, wbp, wv, step in (("50 5 0.2", None, 50, 5), ("500 50 0.2", None, 500, 50), ("500kb 50 0.2", 500000, None, 50)):
        _order, _off, win_end, band_end = jx._ld_window_ends(chrom, pos, wbp, wv, step)
        ranges = jx._ld_ranges(win_end, band_end, jx.LD_MASK_BUDGET_BYTES)
        band_t = torch.from_numpy(band_end.astype(np.int32)).to(dev)
        mask_t = torch.empty(max((r1 - s) * w for s, _e, r1, w in ranges), dtype=torch.int32, device=dev)

        def kernel():
            for s, _e, r1, w in ranges:
                check(lib().jxg_ld_band_mask_p32(_ptr(panel.p32), m, n, None, m, s, r1, _ptr(band_t), _ptr(mean_t), _ptr(std_t),
                                                 _ptr(miss_t), 0.2, w, _ptr(mask_t), _stream()))
        kernel()
        torch.cuda.synchronize()
        ks = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernel()
            e1.record()
            e1.synchronize()
            ks.append(e0.elapsed_time(e1))
        whole, greedy, keep = [], [], None
        for _ in range(a.reps + 1):
            t = {}
            t0 = time.perf_counter()
            keep = jx.bed_packed_ld_prune_maf_priority(packed, n, chrom, pos, window_bp=wbp, window_variants=wv, step_variants=step,
                                                       r2_threshold=0.2, timings=t)
            whole.append(time.perf_counter() - t0)
            greedy.append(t["greedy_s"])
        clean, six, useful = _blocks(ranges, band_end, hasmiss)
        k_ms = float(np.median(ks))
        ops = 2.0 * 1024 * npad * (clean + 6 * six)
        asked = 64.0 * panel.nt * 32 * (clean + six)
        r = {"set": name, "ranges": len(ranges), "mask_words_per_row": max(w for *_x, w in ranges), "kept": int(keep.sum()),
             "kernel_ms": round(k_ms, 2), "greedy_s": round(float(np.median(greedy[1:])), 3),
             "whole_call_s": round(float(np.median(whole[1:])), 3), "blocks_clean": clean, "blocks_six": six,
             "useful_pair_share": round(useful / (1024.0 * max(clean + six, 1)), 3),
             "int8_fraction": round(ops / (k_ms * 1e-3) / I8_PEAK, 4), "payload_bytes_asked": asked,
             "payload_unique_bytes": float(m) * panel.nt * 32,
             "hbm_fraction_asked": round(asked / (k_ms * 1e-3) / HBM_BPS, 4)}
        print(json.dumps(r), flush=True)
        rec["sets"].append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
