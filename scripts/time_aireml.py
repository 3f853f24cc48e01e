"""Time the blocks of multi-kernel AI-REML (`jx reml`; csrc/k_potrf.hip, `pipeline.MultiKernelReml`) on one GPU at one size.

    python scripts/time_aireml.py --n 5000 [--q 2] [--reps 3] [--warmup 1] [--out profiles/aireml_time_n5000.json]

One size per process (run it once per size, each under its own time limit).  Kernels synthesised in HBM: K1 = G G' / m of centred
binomial genotypes (m = n markers), K2 = Z Z' of a one-hot factor with n / 12 levels, further kernels Wishart; X = [1 | N(0, 1)], p = 2.
After --warmup untimed runs, median / min / max over --reps runs of a host clock around work that ends in a device synchronise:
  * combine: V = sum theta_j K_j + theta_e I (`jxg_reml_combine_f64`), with the bytes it moves ((q + 1) / 2 matrices read and written:
    lower triangle only) over the time;
  * factor: `jxg_dpotrf_lower_f64`, as ms and as the fraction of the 78.6 TFLOP/s f64 matrix peak that n^3 / 3 flops in that time is;
  * `torch.linalg.cholesky` of the same matrix, the library comparison;
  * solve with p + 1 columns and with n columns (`jxg_dpotrs_lower_f64`; 2 n^2 nrhs flops);
  * one `profile` (combine + factor + two solves + host algebra) and one `ai_step`, exact and with 12 probes, at a theta whose
    factor is already there (the loop's situation: `profile` of the same theta precedes it).
Nothing is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from janusx_amd import pipeline  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _stream  # noqa: E402

F64_PEAK = 78.6e12


def timed(fn, warmup, reps, before=None):
    out = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--q", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, q = a.n, a.q
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    ks = torch.empty((q, n, n), dtype=torch.float64, device=dev)
    frq = torch.rand(n, generator=gen, device=dev) * 0.4 + 0.1
    g = (torch.rand((n, n), generator=gen, device=dev) < frq).double() + (torch.rand((n, n), generator=gen, device=dev) < frq).double()
    g -= g.mean(dim=0, keepdim=True)
    ks[0] = g @ g.T / float(n)
    for j in range(1, q):
        if j == 1:
            codes = torch.randint(0, max(4, n // 12), (n,), generator=gen, device=dev)
            ks[j] = (codes[:, None] == codes[None, :]).double()
        else:
            g = torch.randn((n, n + 8), generator=gen, device=dev, dtype=torch.float64)
            ks[j] = g @ g.T
            ks[j] /= ks[j].diagonal().mean()
    del g
    truth = np.array([0.5, 0.3, 0.4][:q] + [0.3]) if q <= 3 else np.full(q + 1, 0.3)
    v = torch.eye(n, dtype=torch.float64, device=dev) * truth[q]
    for j in range(q):
        v += ks[j] * truth[j]
    rng = np.random.default_rng(7)
    x = np.column_stack([np.ones(n), rng.standard_normal(n)])
    noise = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    y = x @ np.array([1.0, 0.5]) + (torch.linalg.cholesky(v) @ noise).cpu().numpy()
    fit = pipeline.MultiKernelReml(ks, x, y)
    p = fit.p
    theta = truth * 1.1
    res = {"n": n, "q": q, "p": p, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    th = np.ascontiguousarray(theta)
    res["combine"] = timed(lambda: check(lib().jxg_reml_combine_f64(fit.ks.data_ptr(), q, n, th.ctypes.data, fit.v.data_ptr(), _stream())),
                           a.warmup, a.reps)
    res["combine"]["gb_per_s"] = (q + 1) * 0.5 * n * n * 8 / (res["combine"]["median_ms"] * 1e-3) / 1e9
    info = C.c_int(0)

    def combine():
        check(lib().jxg_reml_combine_f64(fit.ks.data_ptr(), q, n, th.ctypes.data, fit.v.data_ptr(), _stream()))

    res["factor"] = timed(lambda: check(lib().jxg_dpotrf_lower_f64(fit.v.data_ptr(), n, n, C.addressof(info), _stream())),
                          a.warmup, a.reps, before=combine)
    assert info.value == 0
    res["factor"]["fraction_of_f64_peak"] = (n ** 3 / 3.0) / (res["factor"]["median_ms"] * 1e-3) / F64_PEAK
    vsym = torch.empty((n, n), dtype=torch.float64, device=dev)

    def full_v():
        combine()
        vsym.copy_(torch.tril(fit.v.T) + torch.tril(fit.v.T, -1).T)      # the whole symmetric matrix for the library routine

    full_v()
    res["torch_cholesky"] = timed(lambda: torch.linalg.cholesky(vsym), a.warmup, a.reps)
    res["torch_cholesky"]["fraction_of_f64_peak"] = (n ** 3 / 3.0) / (res["torch_cholesky"]["median_ms"] * 1e-3) / F64_PEAK
    combine()
    check(lib().jxg_dpotrf_lower_f64(fit.v.data_ptr(), n, n, C.addressof(info), _stream()))
    ref_l = torch.linalg.cholesky(vsym)
    res["factor_vs_torch_max_rel"] = float((torch.tril(fit.v.T) - ref_l).abs().max() / ref_l.abs().max())
    del ref_l, vsym
    for name, nrhs in (("solve_p1", p + 1), ("solve_n", n)):
        b = torch.randn((nrhs, n), generator=gen, device=dev, dtype=torch.float64)
        res[name] = timed(lambda: check(lib().jxg_dpotrs_lower_f64(fit.v.data_ptr(), n, n, b.data_ptr(), nrhs, n, _stream())),
                          a.warmup, a.reps)
        res[name]["nrhs"] = nrhs
        res[name]["fraction_of_f64_peak"] = (2.0 * n * n * nrhs) / (res[name]["median_ms"] * 1e-3) / F64_PEAK
        del b
    k = [0]

    def fresh_theta():
        k[0] += 1
        return theta * (1.0 + 1e-3 * k[0])

    res["profile"] = timed(lambda: fit.profile(fresh_theta()), a.warmup, a.reps)
    probes = np.where(rng.random((12, n)) < 0.5, -1.0, 1.0)
    cur = [None]

    def prep():
        cur[0] = fresh_theta()
        fit.profile(cur[0])

    res["ai_step_exact"] = timed(lambda: fit.ai_step(cur[0], None), a.warmup, a.reps, before=prep)
    res["ai_step_probes12"] = timed(lambda: fit.ai_step(cur[0], probes), a.warmup, a.reps, before=prep)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
