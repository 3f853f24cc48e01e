"""Time the ADMIXTURE / FastPop passes (`jxg_admx_em_step` = EM pass + finalise, `jxg_admx_loglik`) and one whole `fit_k` on one
GPU, panels synthesised in HBM by bench.py's generator.

    python scripts/time_admx.py [--reps 3] [--skip-c4] [--out profiles/admx_time.json]

Shapes: BASELINE configs[4] (n = 200 000 x m = 1 000 000) at K = 4, 10, 16 and configs[2] (n = 20 000 x m = 200 000) at K = 8;
then `AdmxBedTrainingSession.fit_k` at configs[2], K = 8, with the CLI's settings (rsvd + ALS + Adam-EM, 500-iteration cap) on
the payload already in HBM (BED staging excluded).  Per pass: ms (median of --reps after one warm-up, device events), the
payload bytes read, the f32 operations of the arithmetic (rec: 2K per genotype; A, B, T: 6K per genotype; ll: 2K per genotype),
the payload rate as a fraction of 6.29 TB/s and the operation rate as a fraction of the 157 TF f32 peak.  The split between the
EM pass and the finalise kernels comes from `rocprofv3 --kernel-trace --stats` (profiles/admx_kernel_stats.csv)."""
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
from janusx_amd.bed import Bim  # noqa: E402

HBM_BPS = 6.29e12
F32_PEAK = 157e12


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _shape(n, m, ks, reps, rec, fit=False):
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    packed, _dos = synth_panel_gpu(n, m, 42, dev)
    torch.cuda.synchronize()
    bim = Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * m, ["G"] * m)
    sess = jxrs.AdmxBedTrainingSession(None, False, 0.02, 0.05, 0, payload=(packed, n, bim))
    del packed
    torch.cuda.synchronize()
    setup = round(time.perf_counter() - t0, 2)
    eng = sess._eng
    mk, payload = sess.n_snps, sess.n_snps * ((n + 127) // 128) * 32
    for k in ks:
        g = torch.Generator(device="cpu").manual_seed(k)
        p = torch.rand((mk, k), generator=g).clamp(0.05, 0.95).to(dev)
        q = torch.rand((n, k), generator=g) + 0.05
        q = (q / q.sum(1, keepdim=True)).to(dev)
        mom = tuple(torch.zeros_like(x) for x in (p, p, q, q))
        geno = float(mk) * n
        em = _time(lambda: eng.adam_step(p, q, mom, 0.005, 0.8, 0.88, 1e-8, 1.0, 1.0), reps)
        ll = _time(lambda: eng.loglik(p, q), reps)
        r = {"n": n, "m_kept": mk, "k": k, "work_bytes": int(eng.work.numel()),
             "em_iter_ms": round(em, 2), "em_bytes": payload, "em_flop": 8 * k * geno,
             "em_hbm_fraction": round(payload / (em * 1e-3) / HBM_BPS, 4),
             "em_f32_fraction": round(8 * k * geno / (em * 1e-3) / F32_PEAK, 4),
             "loglik_ms": round(ll, 2), "loglik_flop": 2 * k * geno,
             "loglik_f32_fraction": round(2 * k * geno / (ll * 1e-3) / F32_PEAK, 4)}
        print(json.dumps(r), flush=True)
        rec["passes"].append(r)
        del p, q, mom
    if fit:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = []
        p, q, ll, it, init_ll, als = sess._fit(8, 42, "adam-em", 5, 1e-5, 1000, 1e-5, 0.005, 0.8, 0.88, 1e-8, 500, 5, 0.5,
                                               1e-6, trace=tr)
        torch.cuda.synchronize()
        rec["fit_k8"] = {"n": n, "m_kept": mk, "s": round(time.perf_counter() - t0, 3), "setup_s": setup, "adam_iter": it,
                         "als_iter": als, "ll_final": ll, "init_ll": init_ll, "checks": len(tr)}
        print(json.dumps(rec["fit_k8"]), flush=True)
    del sess, eng
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-c4", action="store_true", help="configs[2] only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admx_time.json"))
    a = ap.parse_args()
    rec = {"passes": []}
    _shape(20000, 200000, (8,), a.reps, rec, fit=True)
    if not a.skip_c4:
        _shape(200000, 1000000, (4, 10, 16), a.reps, rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
