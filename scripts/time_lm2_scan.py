"""Timing of the SNP-by-covariate interaction scan (`lm2_moments_kernel` + `lm2_stats_kernel`, csrc/k_lm2.hip) on a resident
synthetic panel (GPU box): the moment kernel and the algebra kernel alone (device events around `jxg_lm2_scan_p32` stage 1 / 2),
the whole `pipeline.scan_rows_lm2`, and as yardsticks `pipeline.scan_rows_lm` on the same rows with the same X, and with a
design of as many columns as the moment kernel has weight columns (the plain f64-FMA form of the same sums: `lm_dots_kernel`,
four columns per pass over the genotypes).
python scripts/time_lm2_scan.py [n] [m] [q_base] [k] [json out]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                   # noqa: E402
from janusx_amd import janusx as jx            # noqa: E402
from janusx_amd import lm2                     # noqa: E402
from janusx_amd import pipeline as pl          # noqa: E402
from janusx_amd import stats as st             # noqa: E402
from janusx_amd._lib import check, lib         # noqa: E402

F64_MATRIX_PEAK = 78.6e12                      # README: v_mfma_f64 peak of the MI355X, FLOP/s
REPS = 5


def _events(fn):
    """Median device time of fn() over REPS runs after one warm-up, in seconds."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), float(min(times)), float(max(times))


def _wall(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
    q_base = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    k = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    out_json = sys.argv[5] if len(sys.argv) > 5 else None
    dev = torch.device("cuda", 0)
    packed, dos = bench.synth_panel_gpu(n, m, 11, dev, missing_rate=0.01)
    y = bench.make_phenotype(dos, n, 7, dev)
    del dos
    rng = np.random.default_rng(1)
    x = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, q_base - 1))], axis=1)
    cov = rng.standard_normal((n, k)) + np.linspace(0.0, 10.0, k)[None, :]
    panel = pl.Panel(packed, n)
    keep, af, _miss = st.gwas_scan_row_stats(panel.counts(), n, 0.02, 0.05, 1.0)
    rows = np.nonzero(keep)[0]
    mk = len(rows)

    # the two kernels alone, on the operands scan_rows_lm2 builds
    q, r_y, rss0 = lm2.qr_projection(x, y)
    img, nblk, nblk_v = lm2.weight_image(*lm2.weight_columns(q, r_y, cov))
    img_t = torch.from_numpy(img).to(dev)
    rows_t = torch.from_numpy(rows.astype(np.int32)).to(dev)
    lut_t = torch.from_numpy(jx._raw_additive_lut(af[rows], np.zeros(len(rows), dtype=bool), True)).to(dev)
    sums = torch.empty((mk, nblk * 16), dtype=torch.float64, device=dev)
    out = torch.empty((mk, 4 * (1 + k) + 4), dtype=torch.float64, device=dev)
    flag = torch.zeros(mk, dtype=torch.int32, device=dev)
    df = n - (q_base + 1 + k)

    def stage(s):
        check(lib().jxg_lm2_scan_p32(panel.p32.data_ptr(), panel.m, n, rows_t.data_ptr(), mk, lut_t.data_ptr(), img_t.data_ptr(),
                                     nblk, nblk_v, int(q.shape[1]), k, rss0, df, sums.data_ptr(), out.data_ptr(), flag.data_ptr(),
                                     s, torch.cuda.current_stream().cuda_stream))

    t_mom = _events(lambda: stage(1))
    t_alg = _events(lambda: stage(2))
    t_lm2 = _wall(lambda: pl.scan_rows_lm2(panel, rows, af[rows], x, cov, y))
    t_lm = _wall(lambda: pl.scan_rows_lm(panel, rows, af[rows], x, y))
    ncols = (int(q.shape[1]) + 1) * (k + 1) + (k + 1) * (k + 2) // 2
    xw = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, ncols - 2))], axis=1)      # ncols - 1 design columns + r_y
    t_fma = _wall(lambda: pl.scan_rows_lm(panel, rows, af[rows], xw, y))
    flop = 2.0 * mk * panel.nt * 128 * nblk * 16
    res = {
        "n": n, "rows": mk, "q_base": q_base, "k": k, "weight_columns": ncols, "weight_blocks": nblk, "reps": REPS,
        "moments_ms": [t * 1e3 for t in t_mom], "algebra_ms": [t * 1e3 for t in t_alg],
        "scan_rows_lm2_ms": [t * 1e3 for t in t_lm2], "scan_rows_lm_ms": [t * 1e3 for t in t_lm],
        "scan_rows_lm_as_many_columns_ms": [t * 1e3 for t in t_fma],
        "moments_msnps_per_s": mk / t_mom[0] / 1e6, "scan_rows_lm2_msnps_per_s": mk / t_lm2[0] / 1e6,
        "scan_rows_lm_msnps_per_s": mk / t_lm[0] / 1e6, "lm2_over_lm_time": t_lm2[0] / t_lm[0],
        "moments_matrix_flop": flop, "moments_share_of_f64_matrix_peak": flop / t_mom[0] / F64_MATRIX_PEAK,
        "moments_packed_stream_gbs": mk * panel.nt * 32 / t_mom[0] / 1e9, "flagged_rows": int(flag.sum().item()),
    }
    print(f"n={n} rows={mk} q_base={q_base} k={k}: {ncols} weight columns in {nblk} blocks (median, min, max of {REPS})")
    print(f"  moment kernel   {t_mom[0] * 1e3:8.2f} ms ({t_mom[1] * 1e3:.2f} .. {t_mom[2] * 1e3:.2f})  {res['moments_msnps_per_s']:.2f} M SNPs/s, "
          f"{flop / t_mom[0] / 1e12:.2f} TFLOP/s on the matrix pipe = {100 * res['moments_share_of_f64_matrix_peak']:.1f} % of "
          f"{F64_MATRIX_PEAK / 1e12:.1f}, packed stream {res['moments_packed_stream_gbs']:.0f} GB/s")
    print(f"  algebra kernel  {t_alg[0] * 1e3:8.2f} ms ({t_alg[1] * 1e3:.2f} .. {t_alg[2] * 1e3:.2f})")
    print(f"  scan_rows_lm2   {t_lm2[0] * 1e3:8.2f} ms ({t_lm2[1] * 1e3:.2f} .. {t_lm2[2] * 1e3:.2f})  {res['scan_rows_lm2_msnps_per_s']:.2f} M SNPs/s")
    print(f"  scan_rows_lm    {t_lm[0] * 1e3:8.2f} ms ({t_lm[1] * 1e3:.2f} .. {t_lm[2] * 1e3:.2f})  {res['scan_rows_lm_msnps_per_s']:.2f} M SNPs/s "
          f"(the same X); lm2 / lm = {res['lm2_over_lm_time']:.2f}")
    print(f"  scan_rows_lm with {ncols} columns of [X | r_y] (plain f64 FMA form of the sums) {t_fma[0] * 1e3:8.2f} ms "
          f"({t_fma[1] * 1e3:.2f} .. {t_fma[2] * 1e3:.2f})")
    if out_json:
        with open(out_json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
