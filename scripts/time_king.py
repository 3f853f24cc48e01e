"""Time KING (`jx grm -king`; csrc/k_king.hip) on one GPU, on the LD panel of `scripts/time_ldprune.py` synthesised in HBM.

    python scripts/time_king.py [--n 20000] [--m 200000] [--reps 5] [--warmup 2] [--threshold 0.05] [--out profiles/king_time.json]

In one process, each after --warmup untimed runs and as median / min / max over --reps runs:
  * the fused launch `jxg_king_related_p32` (device events around the counter's memset and the kernel) in each tile shape
    (JXGPU_KING_TILE = 128, 64) and in the shape the library picks by itself;
  * the whole `king_unrelated_set_packed` call (host clock; it includes the P32 re-tiling of the payload, the launch, the copy and
    sort of the pair table, the graph and the host prune);
  * the int8 GRM Gram of the same panel (`jxg_grm_accumulate` over every row: the count Gram of csrc/k_grm_i8.hip, device events).
The figure to read is fused / Gram: the fused kernel issues five MFMA passes per k-step where the Gram issues one.  Nothing is
asserted."""
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
from janusx_amd import pipeline, stats as st  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402
from time_ldprune import I8_PEAK, ld_panel_gpu  # noqa: E402


def _spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)), "runs": len(values)}


def _events(fn, warmup, reps):
    """Device time (ms) of fn() over `reps` runs after `warmup` untimed ones."""
    for _ in range(warmup):
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
    return _spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "king_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    packed, _pos = ld_panel_gpu(n, m, 42, dev, 0.0)
    torch.cuda.synchronize()
    panel = jx._panel(packed, n)
    rec = {"n": n, "m": m, "threshold": a.threshold, "reps": a.reps, "warmup": a.warmup}

    cap = 4 * n + 65536
    bi, bj, b0 = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
    bk = torch.empty(cap, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def fused():
        check(lib().jxg_king_related_p32(_ptr(panel.p32), panel.m, n, a.threshold, cap, _ptr(bi), _ptr(bj), _ptr(b0), _ptr(bk),
                                         _ptr(count), _stream()))

    mfma_ops = 5 * 2.0 * m * (n * (n + 1.0) / 2.0)            # five passes over the lower triangle, 2 operations per product
    for tile in ("128", "64", None):
        if tile is None:
            os.environ.pop("JXGPU_KING_TILE", None)
        else:
            os.environ["JXGPU_KING_TILE"] = tile
        t = _events(fused, a.warmup, a.reps)
        t["rows"] = int(count.item())
        t["share_of_int8_peak"] = mfma_ops / (t["median"] * 1e-3) / I8_PEAK
        rec["fused_ms_tile_" + (tile or "default")] = t
        print(f"fused launch, tile {tile or 'default'}: median {t['median']:.2f} ms (min {t['min']:.2f}, max {t['max']:.2f}, {a.reps} runs), "
              f"{t['rows']} rows, {100 * t['share_of_int8_peak']:.1f} % of the int8 peak over its five passes", flush=True)

    whole = []
    for r in range(a.warmup + a.reps):
        timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept, removed, edges, sites = jx.king_unrelated_set_packed(packed, n, a.threshold, timings=timings)
        dt = time.perf_counter() - t0
        if r >= a.warmup:
            whole.append(dt * 1e3)
    rec["unrelated_set_ms"] = _spread(whole)
    rec["unrelated_set"] = {"kept": int(kept.shape[0]), "removed": int(removed.shape[0]), "edges": int(edges), "sites": int(sites),
                            "launches": int(timings["launches"]), "pairs_s": timings["pairs_s"], "prune_s": timings["prune_s"]}
    print(f"king_unrelated_set_packed: median {rec['unrelated_set_ms']['median']:.1f} ms (min {rec['unrelated_set_ms']['min']:.1f}, max "
          f"{rec['unrelated_set_ms']['max']:.1f}); edges {edges}, kept {len(kept)}, removed {len(removed)}, launches {timings['launches']}",
          flush=True)

    keep, mean_g, scale, flip, _var = st.stream_grm_row_prepare(panel.counts(), n, 1, 0.0, 1.0, 0.0)
    rows = np.nonzero(keep)[0]
    lut = st.grm_lut_from_mean_scale(mean_g[rows], scale[rows], flip[rows])
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    lut_t = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(dev)
    acc = torch.zeros((panel.npad, panel.npad), dtype=torch.float64, device=dev)

    def gram():
        check(lib().jxg_grm_accumulate(_ptr(panel.p32), panel.m, panel.n, _ptr(rows_t), _ptr(lut_t), len(rows), _ptr(acc), 0, 0, _stream()))

    g = _events(gram, a.warmup, a.reps)
    g["rows"] = int(len(rows))
    rec["grm_accumulate_ms"] = g
    rec["fused_over_gram"] = rec["fused_ms_tile_default"]["median"] / g["median"]
    print(f"jxg_grm_accumulate over {len(rows)} rows: median {g['median']:.2f} ms (min {g['min']:.2f}, max {g['max']:.2f}); "
          f"fused / Gram = {rec['fused_over_gram']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
