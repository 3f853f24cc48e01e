"""Time the multi-trait LM scan (`jx gwas -lm -trait-level`; csrc/k_lm_traits.hip) on one GPU, on the LD panel of
`scripts/time_ldprune.py` synthesised in HBM.

    python scripts/time_lm_traits.py [--n 20000] [--m 200000] [--traits 16 256 1024] [--reps 3] [--warmup 1] [--missing 0.01]
                                     [--out profiles/lm_traits_time.json]

In one process, per trait count T, each after --warmup untimed runs and as median / min / max over --reps runs (device events
unless stated):
  * the operand preparation `jxg_lmt_prepare` of the T residualised trait columns;
  * the product launches `jxg_lmt_sums_p32` of those columns over every kept row (in row blocks of the pipeline's scratch
    budget), with the share of the int8 peak counted as 2 m n C planes (planes = 4; the missing-call operand doubles the issued
    products and is not counted);
  * the statistics kernel `jxg_lmt_stats` on one row block, dense form and hits form (pmax = 1e-6);
  * the whole `pipeline.scan_rows_lm_traits` call with pmax = 1e-6 (host clock: QR, residualisation, upload, planes, products,
    statistics, hit copy and sort);
and once, next to those, 16 consecutive `pipeline.scan_rows_lm` calls on the same rows (host clock around all 16, synchronised):
the only way to run many traits without this route.  Nothing is asserted."""
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
from janusx_amd import lm2, pipeline, stats as st  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _LmtOperand, _ptr, _stream  # noqa: E402
from time_ldprune import I8_PEAK, ld_panel_gpu  # noqa: E402


def _spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)), "runs": len(values)}


def _events(fn, warmup, reps):
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


def _host(fn, warmup, reps):
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return _spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--traits", type=int, nargs="+", default=[16, 256, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_traits_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    packed, _pos = ld_panel_gpu(n, m, 42, dev, a.missing)
    torch.cuda.synchronize()
    panel = jx._panel(packed, n)
    del packed
    counts = panel.counts()
    keep, af, _miss = st.gwas_scan_row_stats(counts, n, 0.02, 0.05, 1.0)
    rows = np.nonzero(keep)[0].astype(np.int32)
    mk = len(rows)
    rng = np.random.default_rng(7)
    x = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 3))], axis=1)
    rec = {"n": n, "m": m, "rows": mk, "missing": a.missing, "design_columns": 4, "reps": a.reps, "warmup": a.warmup, "by_traits": {}}
    print(f"panel n={n} m={m}, {mk} rows kept, {a.missing:.2%} missing calls", flush=True)

    # the single-trait scan, 16 calls in a row
    ys = rng.normal(size=(16, n))

    def sixteen():
        for t in range(16):
            pipeline.scan_rows_lm(panel, rows, af[rows], x, ys[t])

    s16 = _host(sixteen, a.warmup, a.reps)
    rec["scan_rows_lm_16_calls_ms"] = s16
    per_trait = s16["median"] / 16.0
    rec["scan_rows_lm_per_trait_ms"] = per_trait
    print(f"16 x scan_rows_lm: median {s16['median']:.1f} ms (min {s16['min']:.1f}, max {s16['max']:.1f}) = {per_trait:.2f} ms per trait",
          flush=True)

    q = lm2.qr_basis(x)
    rank = q.shape[1]
    rows_t = torch.from_numpy(rows).to(dev)
    mean_g = np.clip(np.float32(2.0) * af[rows].astype(np.float32), np.float32(0.0), np.float32(2.0))
    mean_t = torch.from_numpy(mean_g).to(dev)
    flip_t = torch.zeros(mk, dtype=torch.uint8, device=dev)
    d_t = torch.from_numpy(pipeline.lm_traits_row_d(counts[rows], n, mean_g, np.zeros(mk, dtype=bool))).to(dev)
    for T in a.traits:
        Y = rng.normal(size=(T, n))
        R = Y - (q @ (q.T @ Y.T)).T
        r_dev = torch.from_numpy(R).to(dev)
        rss0_t = torch.from_numpy(np.einsum("tn,tn->t", R, R)).to(dev)
        out = {}
        out["prepare_ms"] = _events(lambda: _LmtOperand(r_dev, n, panel.npad, dev), a.warmup, a.reps)
        op = _LmtOperand(r_dev, n, panel.npad, dev)
        op_q = _LmtOperand(q.T, n, panel.npad, dev)
        br = max(128, min(pipeline.LMT_SCRATCH_BYTES // (8 * (rank + T)), 1 << 22) // 128 * 128)
        br = min(br, mk)
        gy = torch.empty((br, T), dtype=torch.float64, device=dev)
        qg = torch.empty((br, rank), dtype=torch.float64, device=dev)

        def sums(o, dst, r0, nr):
            check(lib().jxg_lmt_sums_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, mean_t[r0:].data_ptr(),
                                         flip_t[r0:].data_ptr(), _ptr(o.planes), _ptr(o.scale), _ptr(o.colsum), o.ncols, _ptr(dst),
                                         dst.shape[1], _stream()))

        def products():
            for r0 in range(0, mk, br):
                sums(op, gy, r0, min(br, mk - r0))

        pt = _events(products, a.warmup, a.reps)
        pt["ops_2mnC_planes"] = 2.0 * mk * n * T * 4
        pt["share_of_int8_peak"] = pt["ops_2mnC_planes"] / (pt["median"] * 1e-3) / I8_PEAK
        pt["block_rows"] = br
        out["products_ms"] = pt
        sums(op_q, qg, 0, br)
        dense = torch.empty((T, br, 4), dtype=torch.float64, device=dev)
        cap = 1 << 20
        h_t, h_r = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        h_v = torch.empty((cap, 4), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)

        def stats(hits):
            count.zero_()
            check(lib().jxg_lmt_stats(_ptr(qg), None, rank, rank, _ptr(gy), T, T, _ptr(d_t), br, _ptr(rss0_t), n,
                                      None if hits else _ptr(dense), br * 4, 1e-6, cap, 0, 0, _ptr(h_t) if hits else None,
                                      _ptr(h_r) if hits else None, _ptr(h_v) if hits else None, _ptr(count) if hits else None,
                                      _stream()))

        out["stats_dense_ms"] = _events(lambda: stats(False), a.warmup, a.reps)
        out["stats_hits_ms"] = _events(lambda: stats(True), a.warmup, a.reps)
        out["stats_rows"] = br
        del dense, h_t, h_r, h_v, gy, qg, op, op_q, r_dev
        found = {}

        def whole():
            found["hits"] = len(pipeline.scan_rows_lm_traits(panel, rows, af[rows], x, Y, pmax=1e-6).trait)

        out["whole_call_pmax_1e-6_ms"] = _host(whole, a.warmup, a.reps)
        out["hits"] = found["hits"]
        out["single_trait_route_ms"] = per_trait * T
        rec["by_traits"][str(T)] = out
        print(f"T={T}: prepare {out['prepare_ms']['median']:.2f} ms; products {pt['median']:.1f} ms "
              f"({100 * pt['share_of_int8_peak']:.1f} % of the int8 peak, blocks of {br} rows); statistics of {br} rows dense "
              f"{out['stats_dense_ms']['median']:.2f} ms, hits {out['stats_hits_ms']['median']:.2f} ms; whole call "
              f"{out['whole_call_pmax_1e-6_ms']['median']:.1f} ms ({found['hits']} hits) against {per_trait * T:.1f} ms "
              f"= {T} x the single-trait scan", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
