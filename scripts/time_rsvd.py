"""Time the randomized-SVD products (`jxg_packed_mm_cols` Z Q, `jxg_packed_tmm_cols` Z' W) and `jx pca -rsvd` end to end on one
GPU at the BASELINE configs[4] shape (n = 200 000 x m = 1 000 000, panel synthesised in HBM by bench.py's generator).

    python scripts/time_rsvd.py [--n 200000] [--m 1000000] [--reps 5] [--out profiles/rsvd_time.json]

Per product: ms (median of --reps after one warm-up), payload bytes / time as a fraction of the measured 6.29 TB/s HBM read rate,
and the int8 MFMA operations issued (16x16x64: 32 768 ops each) as a fraction of the ~5.0 POPS dense int8 peak (2 x the
~2.5 PF BF16 rate).  End to end: `_admx_rsvd` (the function `jx pca -rsvd` calls) at -dim 10, power 3, tol 0.1, on the payload
already in HBM (BED staging excluded)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth_panel_gpu  # noqa: E402
from janusx_amd import janusx as jxrs  # noqa: E402
from janusx_amd import pipeline as pl  # noqa: E402
from janusx_amd.bed import Bim  # noqa: E402

HBM_BPS = 6.29e12
I8_PEAK = 5.0e15


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _mfma_ops(units_out, k_len, kp):
    nt = 1 if kp <= 4 else (2 if kp <= 8 else (4 if kp <= 16 else 8))
    ncb = (kp + 4 * nt - 1) // (4 * nt)
    n_mfma = ((units_out + 15) // 16) * ((k_len + 127) // 128) * 2 * 2 * nt * ncb   # 2 K halves x 2 planes x NT tiles
    return n_mfma * 16 * 16 * 64 * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rsvd_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    packed, _dos = synth_panel_gpu(a.n, a.m, 42, dev)
    torch.cuda.synchronize()
    rec = {"n": a.n, "m": a.m, "synth_s": round(time.perf_counter() - t0, 2), "products": []}
    payload = a.m * ((a.n + 127) // 128) * 32
    panel = pl.Panel(packed, a.n)
    c = panel.counts().astype(np.int64)
    nm = a.n - c[:, 0]
    p = (c[:, 1] + 2 * c[:, 2]) / (2.0 * np.maximum(nm, 1))
    flip = p > 0.5
    maf = np.where(flip, 1 - p, p).astype(np.float32)
    t0 = time.perf_counter()
    op = jxrs._RsvdOperator(panel, None, jxrs._rsvd_row_design(maf, flip))
    torch.cuda.synchronize()
    rec["t32_transpose_s"] = round(time.perf_counter() - t0, 3)
    for kp in (16, 32):
        q = torch.randn((a.n, kp), dtype=torch.float64, device=dev)
        w = torch.randn((a.m, kp), dtype=torch.float64, device=dev)
        for name, fn, ops in (("ZQ", lambda: op.zq(q), _mfma_ops(a.m, a.n, kp)),
                              ("ZtW", lambda: op.ztw(w), _mfma_ops(a.n, a.m, kp))):
            s = _time(fn, a.reps)
            r = {"product": name, "kp": kp, "ms": round(s * 1e3, 2), "hbm_fraction": round(payload / s / HBM_BPS, 3),
                 "i8_mfma_fraction": round(ops / s / I8_PEAK, 3)}
            print(json.dumps(r), flush=True)
            rec["products"].append(r)
        del q, w
    del op, panel
    torch.cuda.empty_cache()
    bim = Bim(["1"] * a.m, [f"rs{j}" for j in range(a.m)], list(range(1, a.m + 1)), ["A"] * a.m, ["G"] * a.m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev, _vec, tv, rounds = jxrs._admx_rsvd(None, 10, 42, 3, 0.1, False, 0.02, 0.05, payload=(packed, a.n, bim))
    torch.cuda.synchronize()
    rec["pca_rsvd_dim10"] = {"s": round(time.perf_counter() - t0, 3), "power_rounds": rounds,
                             "eigvals": [float(x) for x in ev[:10]], "total_variance": tv}
    print(json.dumps(rec["pca_rsvd_dim10"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
