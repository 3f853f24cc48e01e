"""Time the exhaustive SNP-pair screen (`jx fvlmm2 -screen`; csrc/k_pairscreen.hip) on one GPU, on a synthetic panel in HBM.

    python scripts/time_fvlmm2_screen.py [--shapes 5000x20000,20000x20000] [--missing 0.01] [--p 1e-5] [--reps 3] [--warmup 1]
                                         [--out profiles/fvlmm2_screen_time.json]

Per shape n x m, in one process (device events, median / min / max over --reps runs after --warmup untimed ones):
  * the plane preparation `jxg_lmt_prepare` of the one column r;
  * the scan launch `jxg_pairscreen_scan_p32` over all m (m - 1) / 2 pairs and the 10 default variants at the chi^2_1 quantile
    of --p (the full form, 45 products a step: the only form built), with its int8 multiply-accumulates
    45 x 256 x 64 per tile and 64-sample step, and the share of the int8 peak they are;
  * the host sort of the hits the launch gave;
  * one whole `fvlmm2_screen_packed` call (host clock: re-tiling, planes, launch, download, sort);
  * next to them the six-sum launch of k_ld (`jxg_ld_sums_p32`) over a block of 4096 x m row pairs of the same rows, scaled to
    the pair count of the triangle (its stores, 24 B a pair, are part of that launch).
r is a standard normal vector: the hit count is that of a null scan.  Nothing is asserted."""
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
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _LmtOperand, _ptr, _stream  # noqa: E402
from time_king import _events  # noqa: E402
from time_ldprune import I8_PEAK, ld_panel_gpu  # noqa: E402


def _shape(n, m, a, dev):
    packed, _pos = ld_panel_gpu(n, m, 42, dev, a.missing)
    packed = packed[:m].contiguous()
    panel = jx._panel(packed, n)
    rng = np.random.default_rng(3)
    r = rng.normal(size=n)
    sigma2 = float(r @ r) / (n - 1)
    variants = f2.variant_array(f2.screen_variants())
    nv = int(variants.shape[0])
    t_min = f2.chi2_1_quantile(a.p)
    rec = {"n": n, "m": m, "missing": a.missing, "variants": nv, "t_min": t_min, "pairs": m * (m - 1) // 2}
    r_t = torch.from_numpy(r).to(dev).reshape(1, -1)
    prep = _events(lambda: _LmtOperand(r_t, n, panel.npad, dev), a.warmup, a.reps)
    op = _LmtOperand(r_t, n, panel.npad, dev)
    pstride, scale = int(op.planes.shape[1]) * int(op.planes.shape[2]), float(op.scale[0].item())
    cap = 1 << 22
    flip = torch.zeros(m, dtype=torch.uint8, device=dev)
    var_t = torch.from_numpy(variants).to(dev)
    hi, hj, hv, hn = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(4))
    ht = torch.empty(cap, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    scan = _events(lambda: check(lib().jxg_pairscreen_scan_p32(_ptr(panel.p32), m, n, None, m, _ptr(flip), None, None, 0, _ptr(op.planes),
                                                               pstride, scale, sigma2, _ptr(var_t), nv, t_min, cap, _ptr(hi), _ptr(hj),
                                                               _ptr(hv), _ptr(hn), _ptr(ht), _ptr(counts), _stream())), a.warmup, a.reps)
    nb = (m + 15) // 16
    macs = float(nb * (nb + 1) // 2) * panel.nt * 2 * 45 * 256 * 64
    scan["int8_macs"] = macs
    scan["share_of_int8_peak"] = 2.0 * macs / (scan["median"] * 1e-3) / I8_PEAK
    hits, screened = (int(v) for v in counts.cpu().numpy())
    rec.update(prepare_ms=prep, scan_full_ms=scan, scan_clean_ms=None, hits=hits, pairs_screened=screened)
    k = min(hits, cap)
    cols = [x[:k].cpu().numpy() for x in (hv, hj, hi)] + [-ht[:k].cpu().numpy()]
    t0 = time.perf_counter()
    np.lexsort(cols)
    rec["host_sort_s"] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = jx.fvlmm2_screen_packed(packed, n, np.zeros(m, bool), r, sigma2, variants, t_min)
    torch.cuda.synchronize()
    rec["whole_call_s"] = time.perf_counter() - t0
    assert res["hits_total"] == hits
    # the six-sum launch of k_ld over a block of the same rows
    bi = min(4096, m)
    sums = torch.empty((6, bi, m), dtype=torch.int32, device=dev)
    ld = _events(lambda: check(lib().jxg_ld_sums_p32(_ptr(panel.p32), m, n, None, m, 0, bi, 0, m, _ptr(sums), _stream())), a.warmup, a.reps)
    ld["block_pairs"] = bi * m
    ld["scaled_to_triangle_ms"] = ld["median"] * rec["pairs"] / float(bi * m)
    rec["ld_six_sums_ms"] = ld
    print(f"n={n} m={m}: planes {prep['median']:.3f} ms, scan (full form) {scan['median']:.1f} ms (min {scan['min']:.1f}, max "
          f"{scan['max']:.1f}; {macs:.3g} int8 MACs, {100 * scan['share_of_int8_peak']:.1f} % of the int8 peak), hits {hits} of "
          f"{screened} pairs x {nv}, host sort {rec['host_sort_s'] * 1e3:.2f} ms, whole call {rec['whole_call_s']:.3f} s; k_ld six sums "
          f"over {bi} x {m} pairs {ld['median']:.1f} ms = {ld['scaled_to_triangle_ms']:.1f} ms per triangle", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x20000,20000x20000")
    ap.add_argument("--missing", type=float, default=0.01)
    ap.add_argument("--p", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fvlmm2_screen_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"reps": a.reps, "warmup": a.warmup, "shapes": []}
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.lower().split("x"))
        out["shapes"].append(_shape(n, m, a, dev))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
