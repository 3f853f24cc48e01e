"""GPU tests of `jx reml` (csrc/k_potrf.hip, `pipeline.MultiKernelReml`, `janusx.ai_reml_multi_f64`, `blup.BLUP`, the command)
against numpy and the f64 restatement of the reference (tests/aireml_ref.py).

Bounds (u = 2^-53): a residual ||L L' - A|| / ||A|| or ||A X - B|| / (||A|| ||X||) <= 8 n u (the textbook backward bound with a
small constant); a forward quantity <= 64 n u cond2(A) times its size (the 64 covers the two chained triangular solves).  Every
test prints the measured ratio to its bound (`pytest -s`); DESIGN.md section 3.23 records them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import aireml_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


def _lib():
    from janusx_amd._lib import check, lib
    return lib(), check


@functools.lru_cache(maxsize=None)
def _case(n, q, seed):
    return R.make_case(n, q, seed)


@functools.lru_cache(maxsize=None)
def _case_v(n):
    a = R.case_v(n, 11)
    return a, float(np.linalg.cond(a))


def _nb():
    return int(_lib()[0].jxg_potrf_block())


def _upload_lower(a, lda, rng):
    """Column-major device image (ld = lda) of the lower triangle of `a`; everything else (the strict upper triangle, the
    padding rows) is filled with sentinels the factorisation must neither read nor write.  -> (tensor (n, lda), host copy)."""
    torch = _torch()
    n = a.shape[0]
    img = rng.standard_normal((n, lda)) * 1e3            # img[c, r] = element (r, c)
    for c in range(n):
        img[c, c:n] = a[c:n, c]
    return torch.from_numpy(img.copy()).cuda(), img


def _potrf(t, n, lda):
    torch = _torch()
    lib, check = _lib()
    info = C.c_int(-7)
    check(lib.jxg_dpotrf_lower_f64(t.data_ptr(), n, lda, C.addressof(info), torch.cuda.current_stream().cuda_stream))
    return int(info.value)


def _sizes():
    nb = 64
    return sorted({1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, 127, 128, 129, 200, 577})


# ---- 1. factor and solve at the layout edges ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,pad", [(n, 0) for n in _sizes()] + [(129, 3), (200, 3)])
def test_factor_and_solve(n, pad):
    """n over the block size (NB - 1, NB, NB + 1, 2 NB + 1), the 128-wide dgemm tile (127, 128, 129), 200 and 577 (the second
    512-column outer block: the rank-512 trailing update); lda = n + 3 for two of them.  L against numpy.linalg.cholesky, the
    residual of the factor, the solves for nrhs in {1, 3, 65, n}, and the bytes outside the lower triangle before and after."""
    torch = _torch()
    lib, check = _lib()
    assert _nb() == 64
    a, cond = _case_v(n)
    lda = n + pad
    rng = np.random.default_rng(n)
    t, before = _upload_lower(a, lda, rng)
    assert _potrf(t, n, lda) == 0
    after = t.cpu().numpy()
    low = np.zeros((n, lda), dtype=bool)
    for c in range(n):
        low[c, c:n] = True
    assert np.array_equal(after[~low].view(np.uint64), before[~low].view(np.uint64)), "bytes outside the lower triangle changed"
    l_dev = np.tril(after[:, :n].T)
    l_ref = np.linalg.cholesky(a)
    na = np.linalg.norm(a)
    res = np.linalg.norm(l_dev @ l_dev.T - a) / na
    fwd = np.linalg.norm(l_dev - l_ref) / np.linalg.norm(l_ref)
    print(f"\nn={n} lda={lda} cond={cond:.3g}: factor residual / bound = {res / (8 * n * U):.3g}, forward / bound = "
          f"{fwd / (64 * n * U * cond):.3g}")
    assert res <= 8 * n * U
    assert fwd <= 64 * n * U * cond
    ld = C.c_double(0.0)
    check(lib.jxg_potrf_logdet_f64(t.data_ptr(), n, lda, C.addressof(ld), torch.cuda.current_stream().cuda_stream))
    ref_ld = 2.0 * float(np.sum(np.log(np.diag(l_ref))))
    assert abs(ld.value - ref_ld) <= 64 * n * U * cond * float(np.sum(np.abs(2.0 * np.log(np.diag(l_ref))))) + 4 * U
    for nrhs in sorted({1, 3, 65, n}):
        b = rng.standard_normal((n, nrhs))
        ldb = n + pad
        bimg = rng.standard_normal((nrhs, ldb))
        bimg[:, :n] = b.T
        bt = torch.from_numpy(bimg.copy()).cuda()
        check(lib.jxg_dpotrs_lower_f64(t.data_ptr(), n, lda, bt.data_ptr(), nrhs, ldb, torch.cuda.current_stream().cuda_stream))
        got = bt.cpu().numpy()
        assert np.array_equal(got[:, n:].view(np.uint64), bimg[:, n:].view(np.uint64)), "padding rows of B changed"
        x = got[:, :n].T
        x_ref = np.linalg.solve(a, b)
        sres = np.linalg.norm(a @ x - b) / (na * np.linalg.norm(x))
        sfwd = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
        print(f"  nrhs={nrhs}: solve residual / bound = {sres / (8 * n * U):.3g}, forward / bound = {sfwd / (64 * n * U * cond):.3g}")
        assert sres <= 8 * n * U
        assert sfwd <= 64 * n * U * cond


def test_combine_and_sym_dot():
    """V = theta_e I + sum theta_j K_j on the lower triangle, bit for bit in the reference's order of operations, and
    sum_ij a_ij b_ij from two lower triangles, twice with the same bits (fixed summation order)."""
    torch = _torch()
    lib, check = _lib()
    n, q = 300, 3
    ks, _x, _y, _th = _case(n, q, 5)
    theta = np.array([0.31, 0.07, 1.9, 0.45])
    kd = torch.from_numpy(ks.copy()).cuda()
    v = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    check(lib.jxg_reml_combine_f64(kd.data_ptr(), q, n, theta.ctypes.data, v.data_ptr(), st))
    want = np.eye(n) * theta[q]
    for j in range(q):
        want = want + ks[j] * theta[j]
    got = v.cpu().numpy().T
    il = np.tril_indices(n)
    assert np.array_equal(got[il].view(np.uint64), want[il].view(np.uint64))
    rng = np.random.default_rng(3)
    a = rng.standard_normal((n, n))
    a = a + a.T
    ad = torch.from_numpy(np.tril(a).T.copy()).cuda()            # only the lower triangle is there to be read
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    check(lib.jxg_sym_dot_f64(ad.data_ptr(), kd[0].data_ptr(), n, n, n, out.data_ptr(), st))
    check(lib.jxg_sym_dot_f64(ad.data_ptr(), kd[0].data_ptr(), n, n, n, out[1:].data_ptr(), st))
    o = out.cpu().numpy()
    assert o[0].tobytes() == o[1].tobytes()
    ref = float(np.sum(a * ks[0]))
    assert abs(o[0] - ref) <= 4 * n * n * U * float(np.sum(np.abs(a * ks[0])))      # a sum of n^2 products, any order


# ---- 2. failed pivots, without a fault ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,idx", [(150, 0), (150, 64), (150, 149), (577, 520)])
def test_failed_pivot_is_reported(n, idx):
    """One diagonal entry of an SPD matrix made negative: at 0, at NB (the first pivot of the second block), at n - 1, and in the
    second outer block.  h_info is the index + 1, the call returns 0, and a valid factorisation afterwards is correct.  This is a
    refusal path: the kernel never takes the square root of, or divides by, the bad pivot."""
    a, _cond = _case_v(n)
    bad = a.copy()
    bad[idx, idx] = -1.0
    rng = np.random.default_rng(idx)
    t, _img = _upload_lower(bad, n, rng)
    assert _potrf(t, n, n) == idx + 1
    t2, _img = _upload_lower(a, n, rng)
    assert _potrf(t2, n, n) == 0
    l_dev = np.tril(t2.cpu().numpy().T)
    assert np.linalg.norm(l_dev @ l_dev.T - a) / np.linalg.norm(a) <= 8 * n * U


@pytest.mark.parametrize("row,col,expect", [(70, 70, 71), (0, 0, 1), (100, 3, 101), (149, 66, 150)])
def test_nan_entry_is_reported(row, col, expect):
    """A NaN on the diagonal reports its column.  A NaN below the diagonal at (row, col) is entry (col, row) of the symmetric
    matrix as well; the factorisation reports the first pivot it reaches -- pivot `row`, LAPACK dpotrf's rule -- i.e. column
    `row`."""
    n = 150
    a, _cond = _case_v(n)
    bad = a.copy()
    bad[row, col] = float("nan")
    t, _img = _upload_lower(bad, n, np.random.default_rng(1))
    assert _potrf(t, n, n) == expect


# ---- 3. one step at fixed theta -----------------------------------------------------------------------------------------------------

def _theta_start(y, q):
    return np.full(q + 1, np.var(y, ddof=1) / (q + 1))


def _compare_step(n, q, seed, theta, probes):
    from janusx_amd import pipeline
    ks, x, y, _th = _case(n, q, seed)
    ref = R.MultiKernelRemlRef(ks, x, y)
    dev = pipeline.MultiKernelReml(ks, x, y)
    v = np.eye(n) * theta[q]
    for j in range(q):
        v = v + ks[j] * theta[j]
    bound = 64 * n * U * float(np.linalg.cond(v))
    r_reml, r_ml, pc = ref.profile(theta)
    d_reml, d_ml, dpc = dev.profile(theta)
    # size of the likelihood: the sum of the absolute terms it is made of (reml.rs:874-879)
    size_reml = 0.5 * ((n - x.shape[1]) * abs(np.log(pc["qval"])) + abs(pc["log_det_v"]) + abs(pc["log_det_xt"])) + abs(r_reml)
    ratios = {"reml": abs(d_reml - r_reml) / (bound * size_reml), "ml": abs(d_ml - r_ml) / (bound * size_reml),
              "alpha": np.linalg.norm(dpc["alpha"] - pc["alpha"]) / (bound * np.linalg.norm(pc["vinv_r"]))}
    detail = {}
    r_score, r_ai, r_delta = ref.ai_step(theta, probes, detail)
    d_score, d_ai, d_delta = dev.ai_step(theta, probes)
    m = q + 1
    size_s = np.array([0.5 * (abs(t1) + abs(t2) + abs(qd)) for t1, t2, qd in detail["terms"]])
    size_ai = np.array([[0.5 * np.linalg.norm(detail["ka"][a]) * np.linalg.norm(detail["pka"][b]) for b in range(m)] for a in range(m)])
    size_ai = np.maximum(size_ai, size_ai.T)
    ratios["score"] = float(np.max(np.abs(d_score - r_score) / (bound * size_s)))
    ratios["ai"] = float(np.max(np.abs(d_ai - r_ai) / (bound * size_ai)))
    # delta solves AI delta = score: to first order |d delta| <= ||AI^-1|| (|d score| + |d AI| |delta|)
    size_d = np.linalg.norm(np.linalg.inv(r_ai), 2) * (np.linalg.norm(size_s) + np.linalg.norm(size_ai, 2) * np.linalg.norm(r_delta))
    ratios["delta"] = float(np.linalg.norm(d_delta - r_delta) / (bound * size_d))
    print(f"\nn={n} q={q} probes={'exact' if probes is None else len(probes)} cond={np.linalg.cond(v):.3g}: error / bound "
          + ", ".join(f"{k}={val:.3g}" for k, val in ratios.items()))
    for k, val in ratios.items():
        assert val <= 1.0, (k, val)


@pytest.mark.parametrize("n,q,seed", [(65, 3, 3), (200, 2, 7)])
@pytest.mark.parametrize("at", ["truth", "start"])
@pytest.mark.parametrize("trace", ["exact", "probes"])
def test_one_step(n, q, seed, at, trace):
    """profile -> reml, ml and ai_step -> score, AI, delta at the truth and at the start value, with the exact trace and with a
    12-column +-1 probe matrix handed to both sides, within the forward bound times the size of each quantity."""
    _torch()
    _ks, _x, y, th = _case(n, q, seed)
    theta = th.copy() if at == "truth" else _theta_start(y, q)
    probes = None if trace == "exact" else np.where(np.random.default_rng(9).random((12, n)) < 0.5, -1.0, 1.0)
    _compare_step(n, q, seed, theta, probes)


@pytest.mark.parametrize("trace", ["exact", "probes"])
def test_one_step_past_the_768_switch(trace):
    """n = 769, q = 2: the first size on the other side of the reference's exact / Hutchinson switch (and of the 512-column outer
    block of the factorisation)."""
    _torch()
    n, q, seed = 769, 2, 6
    _ks, _x, _y, th = _case(n, q, seed)
    probes = None if trace == "exact" else np.where(np.random.default_rng(9).random((12, n)) < 0.5, -1.0, 1.0)
    _compare_step(n, q, seed, th.copy(), probes)


# ---- 4. whole fits, exact trace ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,seed", [(64, 2, 2), (131, 2, 4), (300, 3, 5)])
def test_whole_fit_exact(n, q, seed):
    """The restatement converges in 17 / 8 / 7 iterations on these with no halving.  Its margins (printed below): the stopping
    quantity rel_max of the last two iterations is 1.36e-6 -> 6.1e-7, 1.10e-6 -> 2.9e-8, 4.2e-6 -> 5.3e-7 against tol = 1e-6: none
    within 10 % of flipping, where the two sides differ by ~1e-10.  The acceptance test of the LAST iterations is a different
    matter on every design: the step is below 1e-6, the gain in reml below 1e-12, so reml_cand - reml_curr is rounding noise
    inside the test's own 1e-12 slack (margins 1.2e-12, 9.9e-13, 3.8e-12 here).  A flip there halves a step that is already
    below tol: it changes neither `converged` nor `used_iter`, and theta by less than tol.  No seed avoids this."""
    _torch()
    from janusx_amd import janusx as jx
    ks, x, y, _th = _case(n, q, seed)
    log = []
    r_theta, _r_ml, r_reml, r_it, r_conv = R.ai_reml_multi_f64(ks, x, y, trace_probes=0, log=log)
    print(f"\nn={n}: restatement iterations={r_it} halvings={sum(r['halvings'] for r in log)} "
          f"smallest accepted margin={min(r['margins'][-1] for r in log):.3g} last rel_max={[r['rel_max'] for r in log][-2:]}")
    theta, _ml, reml, it, conv = jx.ai_reml_multi_f64(ks, x, y, trace_probes=0)
    print(f"  device: iterations={it} max rel theta difference={np.max(np.abs(theta - r_theta) / r_theta):.3g} "
          f"reml difference={abs(reml - r_reml):.3g}")
    assert r_conv and conv
    assert it == r_it
    assert np.max(np.abs(theta - r_theta) / r_theta) <= 1e-5


@pytest.mark.parametrize("n,q,seed", [(63, 1, 1), (65, 3, 3)])
def test_whole_fit_with_halvings(n, q, seed):
    """(65, 3, 3) halves 20 times in the restatement (one component runs into min_var); (63, 1, 1) is the single-kernel case.
    `converged` on both sides and |reml difference| <= 1e-7: REML is stationary at the fixed point."""
    _torch()
    from janusx_amd import janusx as jx
    ks, x, y, _th = _case(n, q, seed)
    _r_theta, _r_ml, r_reml, _r_it, r_conv = R.ai_reml_multi_f64(ks, x, y, trace_probes=0)
    _theta, _ml, reml, _it, conv = jx.ai_reml_multi_f64(ks, x, y, trace_probes=0)
    print(f"\nn={n}: reml difference={abs(reml - r_reml):.3g}")
    assert r_conv and conv
    assert abs(reml - r_reml) <= 1e-7


# ---- 5. the probe route end to end ---------------------------------------------------------------------------------------------------

def test_probe_route_end_to_end():
    """n = 769, q = 2, default probes (8, seed 42).  The restatement, given the same probe matrix, stops in its third iteration
    with converged = False: all 24 candidates are rejected with margins between -1.2e-9 and -3e-10 (printed), hundreds of times
    the rounding noise of reml at this size (~1e-12), so the comparison of `converged` is not borderline."""
    _torch()
    from janusx_amd import janusx as jx
    from janusx_amd import pipeline
    n, q, seed = 769, 2, 6
    ks, x, y, _th = _case(n, q, seed)
    probes = jx._reml_probe_signs(n, 8, 42)
    log = []
    _r_theta, _r_ml, _r_reml, r_it, r_conv = R.ai_reml_multi_f64(ks, x, y, trace_probes=8, probes=probes, log=log)
    print(f"\nrestatement: iterations={r_it} converged={r_conv} last margins={[f'{m:.3g}' for m in log[-1]['margins'][-3:]]}")
    theta, ml, reml, it, conv = jx.ai_reml_multi_f64(ks, x, y)
    first = pipeline.MultiKernelReml(ks, x, y).profile(_theta_start(y, q))[0]
    print(f"device: iterations={it} converged={conv} reml={reml:.6f} first={first:.6f}")
    assert np.all(np.isfinite(theta)) and np.all(theta >= 1e-12) and np.isfinite(ml)
    assert reml >= first - 1e-12 * it
    assert conv == r_conv and it == r_it


# ---- 6. BLUP on the device ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def blup_case():
    return R.make_blup_case(300, 8)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def test_blup_aireml(blup_case):
    """Through AI-REML.  theta agrees within 1e-5 by the stopping rule (test_whole_fit_exact); beta, the effects and the fitted
    values are smooth in the variance ratios with a sensitivity of the order of cond2(V) ~ 10: 1e-4 of the largest entry."""
    _torch()
    from janusx_amd import blup
    y, xc, z, gs = blup_case
    r = R.blup_fit(y, X=xc, Z=z, G=gs)
    b = blup.BLUP(y, X=xc, Z=z, G=gs, progress=False)
    assert r.route == "aireml" and b.route == "aireml"
    got = {"var ratios": _rel(b.var / b.var[-1], r.var / r.var[-1]), "beta": _rel(b.beta, r.beta), "u": _rel(b.u, r.u),
           "g1": _rel(b.g_by_G[0], r.g_by_G[0]), "g2": _rel(b.g_by_G[1], r.g_by_G[1]), "fitted": _rel(b.fitted, r.fitted)}
    print("\nBLUP through AI-REML, relative differences: " + ", ".join(f"{k}={v:.3g}" for k, v in got.items()))
    assert got["var ratios"] <= 1e-5
    for k in ("beta", "u", "g1", "g2", "fitted"):
        assert got[k] <= 1e-4, (k, got[k])


def test_blup_fallback(blup_case):
    """maxiter = 1 leaves AI-REML unconverged, so L-BFGS-B runs (with the same maxiter, as in the reference).  Scale-free
    quantities only; the tolerance is measured: the restatement's own optimiser from theta0 and from theta0 (1 + 1e-3), ten times
    the largest difference those two host runs show in each quantity."""
    _torch()
    from janusx_amd import blup
    y, xc, z, gs = blup_case
    r0 = R.blup_fit(y, X=xc, Z=z, G=gs, maxiter=1)
    r1 = R.blup_fit(y, X=xc, Z=z, G=gs, maxiter=1, theta0_scale=1.0 + 1e-3)
    assert r0.route == "lbfgsb" and r1.route == "lbfgsb"
    b = blup.BLUP(y, X=xc, Z=z, G=gs, maxiter=1, progress=False)
    assert b.route == "lbfgsb"

    def quantities(f):
        return {"theta ratios": f.theta / f.theta[-1], "beta": f.beta, "u": f.u, "g1": f.g_by_G[0], "g2": f.g_by_G[1], "fitted": f.fitted}
    q0, q1, qb = quantities(r0), quantities(r1), quantities(b)
    for k in q0:
        spread, diff = _rel(q1[k], q0[k]), _rel(qb[k], q0[k])
        print(f"\nBLUP fallback {k}: host spread={spread:.3g} device difference={diff:.3g}")
        assert diff <= 10.0 * spread, (k, diff, spread)


# ---- 7. command -----------------------------------------------------------------------------------------------------------------------

def test_command(tmp_path):
    """120 usable samples of 123 records, two -k files whose id files are in another order, one -rc column: both tables exist, the
    vc lines reproduce BLUP.var, the ids are in phenotype order."""
    _torch()
    from janusx_amd import blup, cli
    n_all = 123
    ks, x, y, _th = R.make_case(n_all, 3, 12)
    rng = np.random.default_rng(4)
    ids = [f"s{i:03d}" for i in range(n_all)]
    block = [f"b{int(v)}" for v in rng.integers(0, 5, n_all)]
    ph = tmp_path / "pheno.tsv"
    lines = ["id\ty\tage\tblock"]
    for i in range(n_all):
        yv = "NA" if i == 5 else f"{y[i]:.8f}"
        lines.append(f"{ids[i]}\t{yv}\t{x[i, 1]:.8f}\t{'NA' if i == 17 else block[i]}")
    ph.write_text("\n".join(lines) + "\n")
    paths = []
    for j, kk in enumerate((ks[0], ks[2])):
        order = rng.permutation(n_all)
        if j == 1:
            order = order[order != 40]                      # sample 40 is missing from the second matrix
        pth = str(tmp_path / f"k{j}.npy")
        np.save(pth, kk[np.ix_(order, order)].astype(np.float32))
        with open(pth + ".id", "w") as fh:
            fh.write("".join(f"{ids[i]}\n" for i in order))
        paths.append(pth)
    out = str(tmp_path / "res" / "fit")
    assert cli.main(["reml", "-p", str(ph), "-n", "y", "-k", paths[0], "-k", paths[1], "-c", "age", "-rc", "block", "-o", out]) == 0
    keep = [i for i in range(n_all) if i not in (5, 17, 40)]
    assert len(keep) == 120
    vc = [ln.split("\t") for ln in open(out + ".reml.vc.tsv").read().splitlines()]
    bl = [ln.split("\t") for ln in open(out + ".reml.blup.tsv").read().splitlines()]
    assert vc[0] == ["trait", "n", "term", "theta", "var", "pve", "reml", "ml", "iters", "route"]
    assert [r[2] for r in vc[1:]] == ["rc:block", "k:k0.npy", "k:k1.npy", "residual"] and all(r[1] == "120" for r in vc[1:])
    assert bl[0] == ["id", "trait", "fixed", "rc:block", "k:k0.npy", "k:k1.npy", "residual"]
    assert [r[0] for r in bl[1:]] == [ids[i] for i in keep]
    sel = [ids[i] for i in keep]
    levels = sorted({block[i] for i in keep})
    z = np.zeros((120, len(levels)))
    z[np.arange(120), [levels.index(block[i]) for i in keep]] = 1.0
    gl = [np.asarray(cli._load_grm(p, sel), dtype=np.float64) for p in paths]
    yk = np.array([float(f"{y[i]:.8f}") for i in keep])
    xk = np.array([float(f"{x[i, 1]:.8f}") for i in keep])
    b = blup.BLUP(yk, X=xk.reshape(-1, 1), Z=[z], G=gl, progress=False)
    np.testing.assert_allclose([float(r[4]) for r in vc[1:]], b.var, rtol=1e-8)
    np.testing.assert_allclose([float(r[5]) for r in vc[1:]], b.var / b.var.sum(), rtol=1e-8)
    assert {r[9] for r in vc[1:]} == {b.route}
    tot = np.array([[float(v) for v in r[2:]] for r in bl[1:]])
    np.testing.assert_allclose(tot.sum(axis=1), yk, rtol=1e-7, atol=1e-7)          # fixed + effects + residual = y
