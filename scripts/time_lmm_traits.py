"""Time the trait-level LMM route (`jx gwas -lmm -trait-level-lmm`; `lmm_traits_chain_kernel` in csrc/k_scan_fast.hip) on one GPU,
on a synthetic HWE panel generated in HBM with polygenic traits.

    python scripts/time_lmm_traits.py [--sizes 5000x50000 20000x200000] [--traits 1 4 16] [--chunk 10000] [--reps 2]
                                      [--old-max-launches 0] [--out profiles/lmm_traits_time.json]

Per size and trait count T, in one process:
  (a) the stages of `pipeline.run_traits_lmm`: eigh, rotation of [X | Y], the T null fits, the T table workspaces, the block
      rotations and the scans (device events around the blocks, host clock synchronised around the others), with chains of
      --chunk rows and without chains;
  (b) on ONE rotated block (the default block of the route: whole chains within pipeline.TRAITS_BLOCK_BYTES) one launch of the new
      kernel for all T traits with 4 / 8 / 16 waves per workgroup (`jxg_lmm_traits_chain_tab_nw`, median of --reps after one warm-up)
      against T launches of `jxg_lmm_scan_chain_tab` on the same block (one run);
  (c) the whole `run_traits_lmm` call (host clock) against T x `pipeline.run_trait`, which is what `-lmm` does without the switch,
      both with chains and both without.
Nothing is asserted."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import make_phenotype, synth_panel_gpu  # noqa: E402
from janusx_amd import pipeline, stats as st  # noqa: E402
from janusx_amd._lib import check, lib  # noqa: E402
from janusx_amd.pipeline import _ptr, _stream  # noqa: E402

LOW, HIGH, MAX_ITER, TOL = -5.0, 5.0, 50, 1e-2


def _host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stages(payload, n, k, Y, x, chain):
    """(a): `run_traits_lmm` stage by stage -> dict of ms."""
    out = {}
    out["eigh"], (s, ut64) = _host(lambda: pipeline.eigh_from_grm(k, 1e-6, None, f32_consumer=True))
    nt = len(Y)

    def rot_and_nulls():
        return pipeline.SpectralModel.for_traits(s, ut64, x, Y)

    # rotation of [X | Y] alone, then the whole constructor (rotation + T null fits and profiles): nulls = the difference
    dev = s.device
    ut32 = torch.empty((n, n), dtype=torch.float32, device=dev)
    check(lib().jxg_cast_f64_to_f32(_ptr(ut64), _ptr(ut32), n * n, _stream()))
    cols = np.concatenate([x, Y.T], axis=1)

    def rotate_xy():
        for c0 in range(0, cols.shape[1], 16):
            xy = torch.from_numpy(np.ascontiguousarray(cols[:, c0:c0 + 16])).to(dev)
            rot = torch.empty_like(xy)
            check(lib().jxg_rotate_xy(_ptr(ut32), n, _ptr(xy), int(xy.shape[1]), _ptr(rot), _stream()))

    out["rotate_xy"], _ = _host(rotate_xy)
    del ut32
    whole, models = _host(rot_and_nulls)
    out["nulls"] = max(whole - out["rotate_xy"], 0.0)
    del ut64
    panel = pipeline.Panel(payload, n)
    counts = panel.counts()
    keep, af, _miss = st.gwas_scan_row_stats(counts, n, 0.02, 0.05, 1.0)
    rows = np.nonzero(keep)[0]
    lut = st.scan_lut_from_counts(af[rows], np.zeros(len(rows), dtype=bool), counts[rows], n)
    init = np.array([math.log10(m.null.lbd) if m.null.lbd > 0 else float("nan") for m in models])
    co = pipeline.traits_chain_offsets(len(rows), chain, 1) if chain else None
    tm = pipeline.StageTimes()
    pipeline.scan_rows_lmm_traits(panel, models[0], rows, lut, models[0].y_rot, init, chain_off=co, times=tm)
    out.update({"tables": tm.t["tables"] * 1e3, "block_rotation": tm.t["rotate"] * 1e3, "scan": tm.t["scan"] * 1e3})
    out["rows"] = int(len(rows))
    out["lambda0"] = [float(m.null.lbd) for m in models]
    return out, (models, panel, rows, lut, init)


def kernel_vs_entry(models, panel, rows, lut, init, chain, reps, old_max=0):
    """(b): one block, new kernel (4 / 8 / 16 waves) against T launches of the one-wave-per-chain entry."""
    shared = models[0]
    n, p, nt, dev = shared.n, shared.p, len(models), panel.device
    br = min(len(rows), max(1, pipeline.TRAITS_BLOCK_BYTES // (4 * n) // chain) * chain)
    stage = pipeline.DenseRotation(panel, shared, rows[:br], lut[:br], br)
    grot = torch.empty((br, n), dtype=torch.float32, device=dev)
    stage.rotate(grot, 0, br)
    co = pipeline.traits_chain_offsets(br, chain, 1)
    loc = torch.from_numpy(co.astype(np.int32)).to(dev)
    nch = len(co) - 1
    nbytes = int(lib().jxg_lmm_tables_bytes(n, p, LOW, HIGH))
    stride = (nbytes + 15) // 16 * 16
    tables = torch.empty((nt, stride), dtype=torch.uint8, device=dev)
    for ti in range(nt):
        check(lib().jxg_lmm_tables_build(_ptr(shared.S), _ptr(shared.xcov), shared.y_rot[ti].data_ptr(), n, p, LOW, HIGH,
                                         tables[ti].data_ptr(), _stream()))
    out = torch.empty((nt, br, 3), dtype=torch.float64, device=dev)
    ev = torch.zeros((nt, br), dtype=torch.int32, device=dev)
    res = {"block_rows": int(br), "chains": int(nch)}

    def carry0():
        return torch.from_numpy(np.repeat(init[:, None], nch, axis=1).copy()).to(dev)

    for nw in (4, 8, 16):
        def new(nw=nw):
            carry = carry0()
            check(lib().jxg_lmm_traits_chain_tab_nw(_ptr(grot), br, n, _ptr(shared.S), _ptr(shared.xcov), p, LOW, HIGH, _ptr(tables),
                                                    stride, nt, TOL, MAX_ITER, _ptr(loc), nch, _ptr(carry), nch, _ptr(out), br,
                                                    _ptr(ev), nw, _stream()))
        if nw == 4:
            new(8)                 # one warm-up launch in all (first touch of the block and of the tables)
        ms = [_event_ms(new) for _ in range(reps)]
        res[f"new_nw{nw}_ms"] = float(np.median(ms))
    res["mean_evals"] = float(ev.to(torch.float64).mean().item())

    nold = nt if old_max <= 0 else min(nt, old_max)

    def old():
        carry = carry0()
        for ti in range(nold):
            check(lib().jxg_lmm_scan_chain_tab(_ptr(grot), br, n, _ptr(shared.S), _ptr(shared.xcov), p, LOW, HIGH,
                                               tables[ti].data_ptr(), TOL, MAX_ITER, _ptr(loc), nch, carry[ti].data_ptr(), 0, 0.0,
                                               out[ti].data_ptr(), ev[ti].data_ptr(), _stream()))
    ms_old = _event_ms(old)
    res["old_launches_run"] = nold                      # fewer than T (--old-max-launches): the time is scaled by T / run
    res["old_T_launches_ms"] = ms_old * nt / nold
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["5000x50000", "20000x200000"])
    ap.add_argument("--traits", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--chunk", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--old-max-launches", type=int, default=0,
                    help="(b): run at most this many of the T launches of the old entry and scale (0 = all T)")
    ap.add_argument("--skip-route", action="store_true", help="leave (c) out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmm_traits_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rec = {"chunk": a.chunk, "bounds": [LOW, HIGH], "max_iter": MAX_ITER, "tol": TOL, "sizes": {}}
    for size in a.sizes:
        n, m = (int(v) for v in size.lower().split("x"))
        payload, head = synth_panel_gpu(n, m, 42, dev, missing_rate=0.01)
        tmax = max(a.traits)
        Yall = np.stack([make_phenotype(head, n, 100 + t, dev) for t in range(tmax)])
        x = np.concatenate([np.ones((n, 1)), np.random.default_rng(7).normal(size=(n, 1))], axis=1)
        k, eff, _ = pipeline.build_grm(payload, n, 1, 0.02, 0.05)
        pipeline.eigh_from_grm(k, 1e-6, None, f32_consumer=True)          # warm-up of the solver's workspaces
        srec = rec["sizes"][size] = {}
        print(f"== n={n} m={m} eff_m={eff}", flush=True)
        for T in a.traits:
            Y = Yall[:T]
            r = srec[str(T)] = {}
            r["stages_chain"], state = stages(payload, n, k, Y, x, a.chunk)
            r["stages_nochain"], _ = stages(payload, n, k, Y, x, None)
            print(f"T={T} (a) chains: " + " ".join(f"{kk}={v:.1f}" for kk, v in r["stages_chain"].items() if kk not in ("lambda0", "rows")),
                  flush=True)
            print(f"T={T} (a) no chains: " + " ".join(f"{kk}={v:.1f}" for kk, v in r["stages_nochain"].items() if kk not in ("lambda0", "rows")),
                  flush=True)
            r["kernel"] = kernel_vs_entry(*state, a.chunk, a.reps, a.old_max_launches)
            print(f"T={T} (b) " + " ".join(f"{kk}={v:.1f}" if isinstance(v, float) else f"{kk}={v}" for kk, v in r["kernel"].items()),
                  flush=True)
            del state
            if a.skip_route:
                continue
            for tag, chain in (("chain", (a.chunk, 1)), ("nochain", None)):
                new_ms, _res = _host(lambda: pipeline.run_traits_lmm(payload, n, k, None, Y, x, warm_chain=chain))

                def today():
                    for t in range(T):
                        pipeline.run_trait(payload, n, k, None, Y[t], x, "lmm", warm_chain=chain)
                old_ms, _ = _host(today)
                r[f"route_{tag}"] = {"run_traits_lmm_ms": new_ms, "T_x_run_trait_ms": old_ms, "ratio": old_ms / new_ms}
                print(f"T={T} (c) {tag}: run_traits_lmm {new_ms:.0f} ms, {T} x run_trait {old_ms:.0f} ms, ratio {old_ms / new_ms:.2f}",
                      flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
                fh.write("\n")
        del payload, k
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
