"""Time the FarmCPU raw route (`jx gwas -farmcpu`; csrc/k_farmcpu.hip, janusx_amd/farmcpu.py) on one GPU, on the LD panel of
`scripts/time_ldprune.py` synthesised in HBM.

    python scripts/time_farmcpu.py [--n 20000] [--m 200000] [--q0 6 22 70] [--reps 3] [--warmup 1] [--missing 0.01]
                                   [--out profiles/farmcpu_time.json]

In one process, per design width q0 = 4 base columns + pseudo-QTN columns (decoded markers), each after --warmup untimed runs and
as median / min / max over --reps runs (device events unless stated):
  * the plane preparation `jxg_lmt_prepare` of [Q | r_y] and of what the digits of Q leave;
  * the product launches `jxg_lmt_sums_p32` of both operands over every kept row, in the pipeline's row blocks;
  * the statistics kernel `jxg_farmcpu_fem_stats` over every kept row;
  * the whole `pipeline.scan_rows_farmcpu_fem` call (host clock: basis, pseudo-inverse, upload, planes, products, statistics,
    the per-slot p);
  * `pipeline.scan_rows_lm` on the same design (host clock): the fixed-effect scan this build had before, as the yardstick;
and once: the REM step (`farmcpu.best_rem_lead_set`, the full 3 x nbin grid at the automatic QTN bound; host clock, with the
device decode of the leads timed apart) on the prior of the q0 = 22 scan, and a whole `janusx.farmcpu_packed` call on a
phenotype with planted effects (host clock, with its iteration count).  Nothing is asserted."""
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

from janusx_amd import farmcpu as fc  # noqa: E402
from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd import pipeline, stats as st  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _LmtOperand, _ptr, _stream  # noqa: E402
from time_ldprune import ld_panel_gpu  # noqa: E402
from time_lm_traits import _events, _host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--q0", type=int, nargs="+", default=[6, 22, 70])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "farmcpu_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    packed, pos = ld_panel_gpu(n, m, 42, dev, a.missing)
    torch.cuda.synchronize()
    panel = jx._panel(packed, n)
    counts = panel.counts()
    keep, af, _miss = st.gwas_scan_row_stats(counts, n, 0.02, 0.05, 1.0)
    rows = np.nonzero(keep)[0].astype(np.int32)
    mk = len(rows)
    flip = np.zeros(mk, dtype=bool)
    afr = af[rows]
    rng = np.random.default_rng(7)
    x_base = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 3))], axis=1)
    q_base = x_base.shape[1]
    causal = np.linspace(0, mk - 1, 12).astype(np.int64)[1:-1]
    gc = fc.decode_rows(panel, rows[causal], afr[causal], flip[causal])
    y = gc @ rng.normal(scale=0.25, size=gc.shape[1]) + rng.normal(size=n)
    rec = {"n": n, "m": m, "rows": mk, "missing": a.missing, "base_columns": q_base, "reps": a.reps, "warmup": a.warmup,
           "by_q0": {}}
    print(f"panel n={n} m={m}, {mk} rows kept, {a.missing:.2%} missing calls", flush=True)
    rows_t = torch.from_numpy(rows).to(dev)
    miss_v = pipeline.farmcpu_missing_value(afr)
    mean_t = torch.from_numpy(miss_v).to(dev)
    flip_t = torch.zeros(mk, dtype=torch.uint8, device=dev)
    ss_t = torch.from_numpy(pipeline.lm_traits_row_d(counts[rows], n, miss_v, flip)).to(dev)
    priors = {}
    for q0 in a.q0:
        kq = q0 - q_base
        qtn = np.linspace(0, mk - 1, kq + 2).astype(np.int64)[1:-1] if kq > 0 else np.zeros(0, dtype=np.int64)
        x = np.ascontiguousarray(np.hstack([x_base, fc.decode_rows(panel, rows[qtn], afr[qtn], flip[qtn])])) if kq else x_base
        des = fc.design_operands(x, q_base, y)
        rank = des.q.shape[1]
        cols = np.vstack([des.q.T, des.r_y[None, :]])
        out = {"k_qtn": kq, "rank": rank}

        def prepare():
            hi = _LmtOperand(cols, n, panel.npad, dev, keep_rem=True)
            return hi, _LmtOperand(hi.rem[:rank], n, panel.npad, dev)

        out["prepare_ms"] = _events(prepare, a.warmup, a.reps)
        op_hi, op_lo = prepare()
        hi = torch.empty((mk, rank + 1), dtype=torch.float64, device=dev)
        lo = torch.empty((mk, rank + 1), dtype=torch.float64, device=dev)
        br = max(128, min(pipeline.LMT_SCRATCH_BYTES // (8 * (2 * rank + 1)), 1 << 22) // 128 * 128)

        def products():
            for r0 in range(0, mk, br):
                nr = min(br, mk - r0)
                for op, dst in ((op_hi, hi), (op_lo, lo)):
                    check(lib().jxg_lmt_sums_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, mean_t[r0:].data_ptr(),
                                                 flip_t[r0:].data_ptr(), _ptr(op.planes), _ptr(op.scale), _ptr(op.colsum), op.ncols,
                                                 dst[r0:].data_ptr(), dst.shape[1], _stream()))

        out["products_ms"] = _events(products, a.warmup, a.reps)
        w_t = torch.from_numpy(des.w).to(dev) if kq else None
        bgb_t = torch.from_numpy(np.ascontiguousarray(des.bg_beta[q_base:])).to(dev) if kq else None
        dixx_t = torch.from_numpy(np.diag(des.ixx)[q_base:].copy()).to(dev) if kq else None
        res = torch.empty((mk, 3), dtype=torch.float64, device=dev)
        maxbits = torch.zeros(max(kq, 1), dtype=torch.int64, device=dev)

        def stats():
            check(lib().jxg_farmcpu_fem_stats(_ptr(hi), _ptr(lo), rank + 1, rank, hi[:, rank:].data_ptr(), rank + 1, _ptr(ss_t), mk,
                                              des.bg_rss, des.df, _ptr(w_t), rank, kq, _ptr(bgb_t), _ptr(dixx_t), _ptr(res),
                                              _ptr(maxbits), _stream()))

        out["stats_ms"] = _events(stats, a.warmup, a.reps)
        del hi, lo, op_hi, op_lo
        got = {}

        def whole():
            got["fem"] = pipeline.scan_rows_farmcpu_fem(panel, rows, afr, flip, x, q_base, y)

        out["scan_rows_farmcpu_fem_ms"] = _host(whole, a.warmup, a.reps)
        out["scan_rows_lm_ms"] = _host(lambda: pipeline.scan_rows_lm(panel, rows, afr, x, y), a.warmup, a.reps)
        priors[q0] = (x, fc.fix_zero_pvalues(got["fem"].p.cpu().numpy().copy()))
        rec["by_q0"][str(q0)] = out
        print(f"q0={q0}: prepare {out['prepare_ms']['median']:.2f} ms; products {out['products_ms']['median']:.1f} ms; statistics "
              f"{out['stats_ms']['median']:.2f} ms; scan_rows_farmcpu_fem {out['scan_rows_farmcpu_fem_ms']['median']:.1f} ms against "
              f"scan_rows_lm {out['scan_rows_lm_ms']['median']:.1f} ms", flush=True)

    # the REM step on the prior of a middle design
    q_rem = 22 if 22 in priors else a.q0[len(a.q0) // 2]
    x, prior = priors[q_rem]
    chrom = [str(1 + int(5 * i // mk)) for i in range(mk)]
    posr = np.asarray(pos)[rows] if pos is not None and len(pos) == m else np.arange(mk) * 3000
    gpos = fc.global_positions(chrom, posr)
    qb = fc.qtn_bound_auto(n)
    nbins, szb = fc.nbin_values(qb, 5), list(fc.DEFAULT_SZBIN)
    spent = {"decode": 0.0}

    def decode(idx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = fc.decode_rows(panel, rows[idx], afr[idx], flip[idx])
        spent["decode"] += time.perf_counter() - t0
        return d

    t0 = time.perf_counter()
    best, combos = fc.best_rem_lead_set(y, x, prior, gpos, szb, nbins, decode)
    rem = time.perf_counter() - t0
    rec["rem_step"] = {"q0": q_rem, "qtn_bound": qb, "combos": len(combos), "largest_lead_set": max(len(c[3]) for c in combos),
                       "total_ms": rem * 1e3, "device_decode_ms": spent["decode"] * 1e3, "winner": [combos[best][0], combos[best][1]]}
    print(f"REM step at q0={q_rem}: {len(combos)} combos up to {qb} leads: {rem * 1e3:.0f} ms, of which the device decode "
          f"{spent['decode'] * 1e3:.0f} ms", flush=True)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = jx.farmcpu_packed(y, x_base[:, 1:], packed, n, flip, afr, chrom, list(posr), row_indices=rows)
    whole_s = time.perf_counter() - t0
    rec["farmcpu_packed"] = {"seconds": whole_s, "iterations": len(res.trace), "qtn": len(res.qtn), "stage1_s": res.stage1_secs,
                             "stage2_s": res.stage2_secs}
    print(f"farmcpu_packed: {whole_s:.1f} s, {len(res.trace)} iterations, {len(res.qtn)} QTNs (search {res.stage1_secs:.1f} s, final "
          f"scan {res.stage2_secs:.2f} s)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
