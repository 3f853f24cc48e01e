"""Time the cross-validation passes of `jx adamixture -cverror` (csrc/k_admx_cv.hip) on one GPU, on a panel synthesised in HBM by
bench.py's generator.

    python scripts/time_admx_cv.py [--n 20000] [--m 200000] [--k 8] [--folds 5] [--reps 5] [--warmup 2] [--skip-cv]
                                   [--out profiles/admx_cv_time.json]

In one process, each after --warmup untimed runs and as median / min / max over --reps runs (device events):
  * the three new launches: `jxg_admx_cv_fold_counts`, `jxg_admx_cv_fold_image` (fold 0) and `jxg_admx_cv_holdout_nll` (fold 0, K);
  * beside them, on the same panel: one Adam-EM pass (`jxg_admx_em_step`), `jxg_admx_loglik` and `jxg_admx_called`;
then a whole `admx_evaluate_cverror` at K with the CLI's settings (host clock; --skip-cv leaves it out).
Every pass is reported as bytes moved per second: the payload of the kept rows read once (the image pass writes it once more).
Nothing is asserted."""
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
from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.bed import Bim  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402


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
    return {"median": float(np.median(out)), "min": float(np.min(out)), "max": float(np.max(out)), "runs": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-cv", action="store_true", help="the launches only, no whole admx_evaluate_cverror")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admx_cv_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m, k, folds = a.n, a.m, a.k, a.folds
    packed, _dos = synth_panel_gpu(n, m, 42, dev)
    bim = Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * m, ["G"] * m)
    sess = jx.AdmxBedTrainingSession(None, False, 0.02, 0.05, 0, payload=(packed, n, bim))
    del packed
    torch.cuda.synchronize()
    eng = sess._eng
    mk = sess.n_snps
    payload = mk * ((n + 127) // 128) * 32
    rec = {"n": n, "m_kept": mk, "k": k, "folds": folds, "reps": a.reps, "warmup": a.warmup, "payload_bytes": payload}

    g = torch.Generator(device="cpu").manual_seed(k)
    p = torch.rand((mk, k), generator=g).clamp(0.05, 0.95).to(dev)
    q = torch.rand((n, k), generator=g) + 0.05
    q = (q / q.sum(1, keepdim=True)).to(dev)
    mom = tuple(torch.zeros_like(x) for x in (p, p, q, q))
    seed = jx._admx_cv_seed(a.seed)
    counts = torch.empty(folds, dtype=torch.int64, device=dev)
    fb = sess.make_cv_fold_backend(0, folds, a.seed)
    image, stats = fb._panel.p32, torch.empty((mk, 3), dtype=torch.int32, device=dev)
    image_args = (_ptr(eng.panel.p32), eng.panel.m, n, _ptr(eng.rows_t), mk)
    eng._ensure_work(k)

    passes = [
        ("cv_fold_counts", payload, lambda: check(lib().jxg_admx_cv_fold_counts(*image_args, folds, seed, _ptr(counts), _stream()))),
        ("cv_fold_image", 2 * payload, lambda: check(lib().jxg_admx_cv_fold_image(*image_args, _ptr(eng.flip_t), folds, seed, 0,
                                                                                 _ptr(image), _ptr(stats), _stream()))),
        ("cv_holdout_nll", payload, lambda: fb._holdout(p, q)),
        ("em_step", payload, lambda: eng.adam_step(p, q, mom, 0.005, 0.8, 0.88, 1e-8, 1.0, 1.0)),
        ("loglik", payload, lambda: eng.loglik(p, q)),
        ("called", payload, lambda: check(lib().jxg_admx_called(*image_args, _ptr(eng.work), int(eng.work.numel()), _ptr(eng.qb),
                                                                _stream()))),
    ]
    for name, nbytes, fn in passes:
        t = _events(fn, a.warmup, a.reps)
        t["bytes"] = nbytes
        t["tb_per_s"] = nbytes / (t["median"] * 1e-3) / 1e12
        rec[name] = t
        print(f"{name}: median {t['median']:.3f} ms (min {t['min']:.3f}, max {t['max']:.3f}, {a.reps} runs), "
              f"{nbytes / 1e9:.2f} GB moved, {t['tb_per_s']:.3f} TB/s", flush=True)
    rec["fold_counts"] = counts.cpu().numpy().tolist()
    fb.close()
    del fb, image, stats, mom

    if not a.skip_cv:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cv = jx.admx_evaluate_cverror(sess, k, folds, a.seed)
        torch.cuda.synchronize()
        rec["evaluate_cverror"] = {"s": time.perf_counter() - t0, "cverror": cv["cverror"], "cverror_se": cv["cverror_se"],
                                   "fold_mean_nll": cv["fold_mean_nll"].tolist()}
        print(f"admx_evaluate_cverror K={k}, {folds} folds: {rec['evaluate_cverror']['s']:.2f} s, CVerror {cv['cverror']:.6f} "
              f"(SE {cv['cverror_se']:.6f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
