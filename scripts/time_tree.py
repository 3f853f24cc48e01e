"""Time the neighbour-joining tree (`jx tree -nj`; csrc/k_tree.hip) on one GPU, on the LD panel of `scripts/time_ldprune.py`
synthesised in HBM.

    python scripts/time_tree.py [--n 20000] [--m 200000] [--reps 3] [--warmup 1] [--out profiles/tree_time.json]

In one process:
  * the count launch `jxg_tree_counts_p32` (two MFMA passes per k-step, n x n) next to `jxg_king_counts_p32` over the same n x n
    block of the same image (eight passes), device events, median / min / max over --reps runs after --warmup untimed ones; the
    figure to read is tree / KING;
  * one whole `nj_newick_from_packed` call (host clock) with its stages: the counts with the P32 re-tiling, the download of the two
    count matrices, the host JC69 transform (the `ln`), the upload of the distance matrix, the NJ loop (device events), the branch
    lengths and the Newick text;
  * the NJ loop against its byte model: step with k active nodes reads k^2 doubles for the row sums and k^2 / 2 for the argmin,
    1.5 k^2 8 B, about 4 n^3 B in all; the achieved share of the HBM peak, and the time per step (three launches) next to it.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from janusx_amd import janusx as jx  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402
from time_king import _events  # noqa: E402
from time_ldprune import HBM_BPS, I8_PEAK, ld_panel_gpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m = a.n, a.m
    packed, _pos = ld_panel_gpu(n, m, 42, dev, 0.0)
    torch.cuda.synchronize()
    rec = {"n": n, "m": m, "reps": a.reps, "warmup": a.warmup}

    panel = jx._panel(packed, n)
    valid = torch.empty((n, n), dtype=torch.int32, device=dev)
    mism = torch.empty((n, n), dtype=torch.int32, device=dev)
    t = _events(lambda: check(lib().jxg_tree_counts_p32(_ptr(panel.p32), panel.m, n, 0, 0, _ptr(valid), _ptr(mism), _stream())),
                a.warmup, a.reps)
    t["share_of_int8_peak"] = 2 * 2.0 * m * float(n) * n / (t["median"] * 1e-3) / I8_PEAK
    rec["tree_counts_ms"] = t
    del valid, mism
    six = torch.empty((6, n, n), dtype=torch.int32, device=dev)
    k = _events(lambda: check(lib().jxg_king_counts_p32(_ptr(panel.p32), panel.m, n, 0, n, 0, n, _ptr(six), _stream())),
                a.warmup, a.reps)
    k["share_of_int8_peak"] = 8 * 2.0 * m * float(n) * n / (k["median"] * 1e-3) / I8_PEAK
    rec["king_counts_ms"] = k
    rec["tree_over_king"] = t["median"] / k["median"]
    del six, panel
    print(f"count launch: tree {t['median']:.2f} ms (min {t['min']:.2f}, max {t['max']:.2f}; {100 * t['share_of_int8_peak']:.1f} % of the "
          f"int8 peak over two passes), KING counts {k['median']:.2f} ms (min {k['min']:.2f}, max {k['max']:.2f}; eight passes), "
          f"tree / KING = {rec['tree_over_king']:.3f}", flush=True)

    timings = {}
    names = [f"s{i}" for i in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    text = jx.nj_newick_from_packed(packed, n, names, timings=timings)
    whole = time.perf_counter() - t0
    model_bytes = 1.5 * 8.0 * float(np.sum(np.arange(3, n + 1, dtype=np.float64) ** 2))
    loop_s = timings["nj_loop_ms"] * 1e-3
    host_ln = timings["download_s"] + timings["jc69_s"] + timings["upload_s"]
    rec["whole_call_s"] = whole
    rec["stages_s"] = {key: float(v) for key, v in timings.items() if key.endswith("_s")}
    rec["nj_loop"] = {"ms": timings["nj_loop_ms"], "steps": n - 2, "us_per_step": 1e6 * loop_s / max(n - 2, 1), "model_bytes": model_bytes,
                      "model_gbs": model_bytes / loop_s / 1e9, "share_of_hbm_peak": model_bytes / loop_s / HBM_BPS}
    rec["host_ln_and_transfers_s"] = host_ln
    rec["host_ln_and_transfers_share_of_whole"] = host_ln / whole
    rec["newick_bytes"] = len(text)
    print(f"whole call {whole:.2f} s: counts {timings['counts_s']:.2f} s, download {timings['download_s']:.2f} s, JC69 on the host "
          f"{timings['jc69_s']:.2f} s, upload {timings['upload_s']:.2f} s, NJ loop {loop_s:.3f} s ({rec['nj_loop']['us_per_step']:.1f} us "
          f"per step of three launches; byte model {model_bytes / 1e9:.1f} GB -> {rec['nj_loop']['model_gbs']:.0f} GB/s, "
          f"{100 * rec['nj_loop']['share_of_hbm_peak']:.1f} % of the HBM peak), lengths and Newick {timings['render_s']:.2f} s; host ln and "
          f"the transfers {100 * host_ln / whole:.0f} % of the call", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
