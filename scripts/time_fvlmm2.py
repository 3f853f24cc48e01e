"""Time the SNP-pair interaction test (`jx fvlmm2`; csrc/k_fvlmm2.hip) on one GPU, on a synthetic panel in HBM.

    python scripts/time_fvlmm2.py [--n 20000] [--m 4096] [--pairs 8192] [--batch 4096] [--pcov 2] [--reps 3] [--warmup 1]
                                  [--out profiles/fvlmm2_time.json]

In one process, for the operators '*' and '&', on one batch of --batch pairs (device events, median / min / max over --reps runs after
--warmup untimed ones):
  * the combo kernel `jxg_fvlmm2_combo_p32` (g1, g2 and the combo row of every pair from the P32 image) against its byte model, the
    3 x batch x n x 4 bytes it writes;
  * the three rotations `jxg_rotate_dense_f32` (3 x batch x n x n x 2 flop on the f32 matrix pipes);
  * the joint kernel `jxg_fvlmm2_joint` on the rotated rows;
then one whole `fvlmm2_pairs_packed` call over --pairs pairs (host clock, tables and transfers included) and, for comparison, the
fixed-lambda scan of `jx gwas -fvlmm` (`pipeline.scan_rows`) over 3 x batch SNP rows of the same panel and null model: as many rows
rotated, on the int8 pipes there.  U^T is a random matrix scaled by 1 / sqrt(n): the times do not depend on its values.  Nothing is
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

from janusx_amd import fvlmm2 as f2  # noqa: E402
from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd import pipeline as pl  # noqa: E402
from janusx_amd import stats as st  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402
from time_king import _events  # noqa: E402
from time_ldprune import HBM_BPS, ld_panel_gpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--pcov", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fvlmm2_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m, nb, p = a.n, max(a.m, 3 * a.batch), a.batch, a.pcov
    packed, _pos = ld_panel_gpu(n, m, 42, dev, 0.01)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    ut = torch.randn((n, n), generator=gen, device=dev, dtype=torch.float32) / float(np.sqrt(n))
    s = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * 4.0
    xcov = torch.randn((n, p), generator=gen, device=dev, dtype=torch.float64)
    y = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    l10 = 0.0
    panel = jx._panel(packed, n)
    counts = panel.counts()
    maf = ((counts[:, 1] + 2.0 * counts[:, 2]) / (2.0 * np.maximum(n - counts[:, 0], 1))).astype(np.float32)
    flip = np.zeros(m, dtype=bool)
    lut_all = jx._raw_additive_lut(maf, flip, True)
    rng = np.random.default_rng(1)
    rec = {"n": n, "m": m, "batch": nb, "pairs": a.pairs, "p_cov": p, "reps": a.reps, "warmup": a.warmup}
    g = torch.empty((3, nb, n), dtype=torch.float32, device=dev)
    grot = torch.empty((3, nb, n), dtype=torch.float32, device=dev)
    cnt = torch.empty((nb, 3), dtype=torch.int32, device=dev)
    out = torch.empty((nb, 9), dtype=torch.float64, device=dev)
    for op in ("*", "&"):
        r1 = rng.integers(0, m, size=nb)
        r2 = (r1 + 1 + rng.integers(0, m - 1, size=nb)) % m
        tab, pos = f2.pair_tables(lut_all[r1], lut_all[r2], [op] * nb, np.zeros(nb, bool), np.zeros(nb, bool))
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
        t = [up(r1.astype(np.int32)), up(r2.astype(np.int32)), up(lut_all[r1]), up(lut_all[r2]), up(tab), up(pos.view(np.int32))]
        combo = _events(lambda: check(lib().jxg_fvlmm2_combo_p32(_ptr(panel.p32), panel.m, n, _ptr(t[0]), _ptr(t[1]), nb, _ptr(t[2]),
                                                                 _ptr(t[3]), _ptr(t[4]), _ptr(t[5]), _ptr(g[0]), _ptr(g[1]),
                                                                 _ptr(g[2]), n, _ptr(cnt), _stream())), a.warmup, a.reps)
        combo["share_of_hbm_peak"] = 3.0 * nb * n * 4.0 / (combo["median"] * 1e-3) / HBM_BPS

        def rotate():
            for k in range(3):
                check(lib().jxg_rotate_dense_f32(_ptr(g[k]), nb, n, _ptr(ut), _ptr(grot[k]), _stream()))
        rot = _events(rotate, a.warmup, a.reps)
        rot["tflops"] = 3.0 * 2.0 * nb * float(n) * n / (rot["median"] * 1e-3) / 1e12
        joint = _events(lambda: check(lib().jxg_fvlmm2_joint(_ptr(grot[0]), _ptr(grot[1]), _ptr(grot[2]), nb, n, n, _ptr(s),
                                                             _ptr(xcov), p, _ptr(y), 10.0 ** l10, _ptr(out), _stream())),
                        a.warmup, a.reps)
        joint["share_of_hbm_peak"] = 2.0 * 3.0 * nb * n * 4.0 / (joint["median"] * 1e-3) / HBM_BPS      # two passes over the rows
        rec[f"op_{'mul' if op == '*' else 'and'}"] = {"combo_ms": combo, "rotate3_ms": rot, "joint_ms": joint,
                                                      "nan_rows": int(torch.isnan(out[:, 0]).sum())}
        print(f"op {op}: combo {combo['median']:.3f} ms ({100 * combo['share_of_hbm_peak']:.1f} % of the HBM peak on its stores), three "
              f"rotations {rot['median']:.2f} ms ({rot['tflops']:.1f} Tflop/s f32), joint {joint['median']:.3f} ms "
              f"({100 * joint['share_of_hbm_peak']:.1f} % of the HBM peak over two passes)", flush=True)

        r1w = rng.integers(0, m, size=a.pairs)
        r2w = (r1w + 1 + rng.integers(0, m - 1, size=a.pairs)) % m
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = jx.fvlmm2_pairs_packed(packed, n, flip, maf, r1w, r2w, op, np.zeros(a.pairs, bool), np.zeros(a.pairs, bool), s, xcov, y, ut,
                                     l10, batch_size=nb)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
        rec[f"op_{'mul' if op == '*' else 'and'}"]["whole_call_s"] = whole
        rec[f"op_{'mul' if op == '*' else 'and'}"]["whole_call_pairs_per_s"] = a.pairs / whole
        print(f"op {op}: fvlmm2_pairs_packed over {a.pairs} pairs {whole:.3f} s ({a.pairs / whole:.0f} pairs/s; finite rows "
              f"{int(np.isfinite(res['p_combo']).sum())})", flush=True)
    del g, grot

    # the fixed-lambda scan of `jx gwas -fvlmm` over 3 x batch SNP rows: the same count of rotated rows
    sm = pl.SpectralModel.rotated(s, ut, xcov, y, dev)
    rows = np.arange(3 * nb)
    lut = st.scan_lut_from_counts(maf[rows], flip[rows], counts[rows], n)

    def scan():
        pl.scan_rows(panel, sm, rows, lut, "fvlmm", low=l10, high=l10 + 1.0, max_iter=0, tol=1e-2, init_log10_lbd=l10, block_rows=8192)
    if p >= 1:
        fv = _events(scan, a.warmup, a.reps)
        rec["fvlmm_scan_3x_rows_ms"] = fv
        print(f"-fvlmm scan of {3 * nb} SNP rows: {fv['median']:.2f} ms (min {fv['min']:.2f}, max {fv['max']:.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
