"""The divide and conquer of the eigensolver (csrc/k_stedc.hip, behind src/math/eigh.rs:1422-1528) as a stage of its own, on
tridiagonal matrices chosen by the test: jxg_stedc_f64 with no JXGPU_* variable set, i.e. the product's leaves (65 .. 128 rows of
the batched QL kernel, both halves of its lane vectors), its deflation, its merges and the column window of the top-level merge.

Designs, units and hard bars: tests/stedc_ref.py.  Sizes: 129 (leaves 64 + 65), 130 (65 + 65), 254 (127 + 127), 256 (128 + 128), 611
and 1023 keep every merge product on the f64 GEMM; 2100 (halves of 1050) is the smallest round size whose top merge can take the
sliced int8 product (toeplitz does, with K = n).

At the f64-only sizes every measured quantity must also stay within 16 x max(LAPACK's value for the same T, 8 eps): the own kernels
sum in another order (64-lane wave reductions, rsq + Newton rotations, MFMA accumulation), which is worth a small constant over
LAPACK and not a factor that grows with n.  WIDENED holds the designs whose factor is larger, with the term responsible.

The scaled cases (T times 2^-40, 2^-200, 2^+40) pin the normalisation at the entry of stedc_split: the deflation tolerance of a
merge presumes ||T|| ~ 1; before that normalisation 2^-40 tridiag(-1, 2, -1), n = 611, came back with a residual of
6.7e-6 ||T|| and eigenvalues off by 3.0e-5 ||T|| (docs/EXPERIMENTS.md E.6).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stedc_ref as R   # noqa: E402

gpu = pytest.mark.gpu

# design -> factor over LAPACK that replaces REL_FACTOR at the f64-only sizes, never past the hard bars (reason beside it)
WIDENED = {}


def _lib():
    from janusx_amd._lib import lib
    return lib()


def _stedc(d, e, lo=0, hi=0):
    """jxg_stedc_f64 on fresh device copies of (d, e): (eigenvalues, Z row-major) as numpy arrays"""
    import torch
    from janusx_amd._lib import check
    dev = torch.device("cuda:0")
    n = len(d)
    d_d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).to(dev)
    d_e = torch.from_numpy(np.ascontiguousarray(e, dtype=np.float64)).to(dev)
    rows = (hi - lo) if hi > lo else n
    d_z = torch.full((rows, n), float("nan"), dtype=torch.float64, device=dev)
    check(_lib().jxg_stedc_f64(d_d.data_ptr(), d_e.data_ptr(), n, d_z.data_ptr(), 0, lo, hi, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d_d.cpu().numpy(), d_z.cpu().numpy()


def _assert_solution(case, d, e, w, z, tag=""):
    """the assertions of a full solve; prints and returns (ev, orth, res)"""
    n = len(d)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(w)), R.case_id(case)
    assert np.all(np.diff(w) >= 0), R.case_id(case)
    got = R.measure(d, e, w, z, R.reference_eigenvalues(case))
    line = f"stedc {R.case_id(case)}{tag}: ev {got[0]:.2e} orth {got[1]:.2e} res {got[2]:.2e}"
    if n <= max(R.SIZES_F64):
        lap = R.lapack_measures(case)
        line += f" | LAPACK ev {lap[0]:.2e} orth {lap[1]:.2e} res {lap[2]:.2e}"
    print(line)
    for name, g, bar in zip(("ev", "orth", "res"), got, R.hard_bars(n)):
        assert g < bar, (R.case_id(case), name, g, bar)
    if n <= max(R.SIZES_F64):
        factor = WIDENED.get(case[0], R.REL_FACTOR)
        for name, g, l, bar in zip(("ev", "orth", "res"), got, lap, R.hard_bars(n)):
            assert g <= min(bar, factor * max(l, R.REL_FLOOR)), (R.case_id(case), name, g, l)
    return got


@functools.lru_cache(maxsize=None)
def _full(case):
    """the unwindowed solve of a case, shared by the tests that compare with it (never modified)"""
    d, e = R.matrix(case)
    w, z = _stedc(d, e)
    w.setflags(write=False)
    z.setflags(write=False)
    return w, z


WINDOW_CASES = [("wilkinson", (257,), 0), ("two_roots", (611,), 0), ("glued", (21, 100, 1e-8), 0), ("toeplitz", (R.SIZE_OZ,), 0)]
# the cases whose unwindowed, unscaled solve another test compares with: only these stay cached
_SHARED = set(WINDOW_CASES) | {(c[0], c[1], 0) for c in R.CASES if c[2] != 0}


def test_reference_meets_the_bars():
    """numpy.linalg.eigh (LAPACK dsyevd) on the dense T of every case stays inside the hard bars, and bisection agrees with the
    closed forms: the designs and the checking code are sound on a machine without a GPU.  Measured (numpy 2.2, scipy 1.15), worst
    over the unscaled cases: orth 5.3e-15, res 1.5e-15, ev 5.9e-17 sqrt(n): three orders inside the bars."""
    from scipy.linalg import eigvalsh_tridiagonal
    for case in R.CASES:
        n = len(R.matrix(case)[0])
        if case[2] != 0 and n > max(R.SIZES_F64):
            continue        # dsyevd of 2^k T runs at 257 and 611; the 2100-row designs run unscaled (a second per matrix)
        got = R.lapack_measures(case)
        for name, g, bar in zip(("ev", "orth", "res"), got, R.hard_bars(n)):
            assert g < bar, (R.case_id(case), name, g, bar)
    for name, closed in R.CLOSED_FORM.items():
        for n in R.SIZES_F64 + (R.SIZE_OZ,):
            d, e = R.DESIGNS[name](n)
            # bisection resolves an eigenvalue to a few eps ||T||: 8 eps
            assert np.max(np.abs(eigvalsh_tridiagonal(d, e, lapack_driver="stebz") - closed(n))) < R.REL_FLOOR * R.tnorm(d, e)


@gpu
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] == 0], ids=R.case_id)
def test_full_solve(case):
    """Eigenvalues ascending, Z finite, the three hard bars, and at n <= 1023 the bar relative to LAPACK."""
    assert _lib().jxg_oz_planes() == 6          # the header's 2e-12 orthogonality belongs to the 6-plane products
    d, e = R.matrix(case)
    w, z = _full(case) if case in _SHARED else _stedc(d, e)
    _assert_solution(case, d, e, w, z)


@gpu
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] != 0], ids=R.case_id)
def test_scaled_solve(case):
    """T times a power of two: the same bars relative to ||2^k T||.  stedc_split normalises T by the power of two that brings
    max(|d|, |e|) into [1, 2), so T and 2^k T enter the recursion as the same bits: the eigenvalues are exactly 2^k times those of
    the unscaled solve and the eigenvectors bit-identical -- a consequence of that form of the fix, asserted here."""
    assert _lib().jxg_oz_planes() == 6
    d, e = R.matrix(case)
    w, z = _stedc(d, e)
    _assert_solution(case, d, e, w, z)
    w0, z0 = _full((case[0], case[1], 0))
    assert np.array_equal(w, np.ldexp(w0, case[2])), R.case_id(case)
    assert np.array_equal(z, z0), R.case_id(case)


@gpu
def test_zero_matrix_is_the_identity_decomposition():
    """T = 0: eigenvalues 0, eigenvectors the identity (nothing to normalise by), with and without a window."""
    n = 130
    w, z = _stedc(np.zeros(n), np.zeros(n - 1))
    assert np.array_equal(w, np.zeros(n)) and np.array_equal(z, np.eye(n))
    w, z = _stedc(np.zeros(n), np.zeros(n - 1), 7, 70)
    assert np.array_equal(w, np.zeros(n)) and np.array_equal(z, np.eye(n)[7:70])


@gpu
@pytest.mark.parametrize("case", WINDOW_CASES, ids=R.case_id)
def test_column_windows(case):
    """The column window of the top-level merge (sel_lo / sel_hi of stedc_split, the multi-rank path's form) on one device: per
    world in {2, 3, 8} one call per rank on [n r / world, n (r + 1) / world), and one-column windows at ranks 0, n / 2 and n - 1.
    Every call's eigenvalues are bit-identical to the unwindowed call's; the rows of all ranks stacked in order pass the bars of a
    full solve; a windowed row agrees with the unwindowed row up to sign within the orthogonality bar wherever its eigenvalue lies
    more than 1e-6 ||T|| from its neighbours.  two_roots keeps two roots at the top merge: most windows hold deflated columns only."""
    assert _lib().jxg_oz_planes() == 6
    d, e = R.matrix(case)
    n = len(d)
    w0, z0 = _full(case)
    t = R.tnorm(d, e)
    gap = np.full(n, np.inf)
    gap[1:] = np.diff(w0)
    gap[:-1] = np.minimum(gap[:-1], np.diff(w0))
    isolated = gap > 1e-6 * t

    def rows_agree(z, lo, hi, tag):
        ref = z0[lo:hi]
        sign = np.where(np.sum(z * ref, axis=1) < 0, -1.0, 1.0)
        err = np.max(np.abs(z * sign[:, None] - ref), axis=1)
        iso = isolated[lo:hi]
        if iso.any():
            assert np.max(err[iso]) < R.ORTH_BAR, (R.case_id(case), tag, float(np.max(err[iso])))

    for world in (2, 3, 8):
        parts = []
        for r in range(world):
            lo, hi = n * r // world, n * (r + 1) // world
            w, z = _stedc(d, e, lo, hi)
            assert z.shape == (hi - lo, n) and np.all(np.isfinite(z))
            assert np.array_equal(w, w0), (R.case_id(case), world, r)
            rows_agree(z, lo, hi, (world, r))
            parts.append(z)
        zs = np.concatenate(parts, axis=0)
        n_small = n <= max(R.SIZES_F64)
        got = R.measure(d, e, w0, zs, R.reference_eigenvalues(case))
        print(f"stedc windows {R.case_id(case)} world {world}: ev {got[0]:.2e} orth {got[1]:.2e} res {got[2]:.2e}")
        for name, g, bar in zip(("ev", "orth", "res"), got, R.hard_bars(n)):
            assert g < bar, (R.case_id(case), world, name, g, bar)
        if n_small:
            factor = WIDENED.get(case[0], R.REL_FACTOR)
            for name, g, l in zip(("ev", "orth", "res"), got, R.lapack_measures(case)):
                assert g <= factor * max(l, R.REL_FLOOR), (R.case_id(case), world, name, g, l)
    for r in (0, n // 2, n - 1):
        w, z = _stedc(d, e, r, r + 1)
        assert z.shape == (1, n) and np.all(np.isfinite(z))
        assert np.array_equal(w, w0), (R.case_id(case), "column", r)
        assert abs(float(z[0] @ z[0]) - 1.0) < R.ORTH_BAR
        tz = z[0] * d
        tz[:-1] += z[0, 1:] * e
        tz[1:] += z[0, :-1] * e
        assert np.max(np.abs(tz - w0[r] * z[0])) < R.RES_BAR * t, (R.case_id(case), "column", r)
        rows_agree(z, r, r + 1, ("column", r))


def test_window_arguments_are_checked():
    """jxg_stedc_f64 refuses a window outside [0, n] and sizes below 4 before any GPU work."""
    from janusx_amd._lib import lib
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    for n, lo, hi in ((3, 0, 0), (8, -1, 4), (8, 5, 3), (8, 2, 9)):
        assert lib().jxg_stedc_f64(p, p, n, p, 0, lo, hi, None) != 0
        assert b"jxg_stedc_f64" in lib().jx_last_error()
    assert lib().jxg_stedc_f64(None, p, 8, p, 0, 0, 0, None) != 0


# ---------------------------------------------------------------- the product route: jxg_eigh_f64 on dense copies

def _eigh_dense(a):
    """jxg_eigh_f64 with nothing set: (eigenvalues, U' row-major)"""
    import torch
    from janusx_amd._lib import check
    dev = torch.device("cuda:0")
    n = a.shape[0]
    d_a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_w = torch.zeros(n, dtype=torch.float64, device=dev)
    check(_lib().jxg_eigh_f64(d_a.data_ptr(), n, 0.0, d_w.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return d_w.cpu().numpy(), d_a.cpu().numpy()


def _assert_product(case, d, e):
    """bars of test_eigh_two_stage_path_and_its_fallback with ||T|| as the scale: 1e-11 on all three"""
    w, z = _eigh_dense(R.dense(d, e))
    two_stage = _lib().jxg_last_kernel_ms(10) == 1.0
    assert np.all(np.isfinite(z)) and np.all(np.diff(w) >= 0)
    ev, orth, res = R.measure(d, e, w, z, R.reference_eigenvalues(case))
    print(f"eigh {R.case_id(case)}: ev {ev:.2e} orth {orth:.2e} res {res:.2e} (finished on the {'two' if two_stage else 'one'}-stage reduction)")
    assert ev < 1e-11 and orth < 1e-11 and res < 1e-11, (R.case_id(case), ev, orth, res)
    return two_stage


PRODUCT_2100 = [("wilkinson", (R.SIZE_OZ,), 0), ("glued", (21, 100, 1e-8), 0), ("toeplitz", (R.SIZE_OZ,), 0),
                ("toeplitz", (R.SIZE_OZ,), -40)]


@gpu
@pytest.mark.parametrize("case", PRODUCT_2100, ids=R.case_id)
def test_product_route_two_stage(case):
    """n = 2100 through jxg_eigh_f64 with nothing set: the two-stage reduction of a matrix that is tridiagonal already (every
    panel of the band reduction is [R; 0] and keeps the identity transformation), the own divide and conquer with its default
    leaves (n >= 2048), both back-transformations; no fallback to the one-stage reduction."""
    assert _lib().jxg_oz_planes() == 6
    d, e = R.matrix(case)
    assert _assert_product(case, d, e)


@gpu
@pytest.mark.parametrize("case", [("wilkinson", (611,), 0), ("toeplitz", (611,), 0), ("negative", (611,), 0),
                                  ("toeplitz", (611,), -40)], ids=R.case_id)
def test_product_route_one_stage(case):
    """n = 611 through jxg_eigh_f64 with nothing set: the one-stage sytrd, and rocSOLVER's dstedc (below 2048 rows), which gets T
    normalised like the own merges: without that 2^-40 tridiag(-1, 2, -1) came back with ev 2.5e-5, res 3.9e-6."""
    d, e = R.matrix(case)
    assert not _assert_product(case, d, e)


@gpu
@pytest.mark.parametrize("case", [("toeplitz", (200,), 0), ("toeplitz", (200,), -40), ("negative", (200,), -200),
                                  ("negative", (200,), 40)], ids=R.case_id)
def test_product_route_below_256_rows(case):
    """n = 200 through jxg_eigh_f64: rocSOLVER's dsyevd, which does not scale its input as LAPACK's does; the matrix goes in with
    max|a_ij| in [1, 2).  Without that: 2^-40 tridiag(-1, 2, -1) ev 1.1e-5, res 2.0e-6; 2^-200 x negative ev 5e-2, res 0.18."""
    d, e = R.matrix(case)
    assert not _assert_product(case, d, e)


@gpu
@pytest.mark.parametrize("case", [("toeplitz", (R.SIZE_OZ,), 0), ("negative", (611,), 0)], ids=R.case_id)
def test_reduction_passes_a_tridiagonal_matrix_through(case):
    """jxg_sy2st_f64 on the dense copy: no failure flag, and (d, |e|) come back as they went in within 1e-12 max|A| (the factor of
    test_device_reflectors_satisfy_the_contract) -- a tridiagonal input passes both reduction stages untouched but for signs.
    The block below the band of a tridiagonal matrix holds a single non-zero entry, e[j + 63] in its top right corner: an exactly
    rank-deficient panel, which the band reduction's CholeskyQR cannot factor (failure flag 15 before sb_chol_kernel learned to
    recognise a panel that is [R; 0] already and to leave it alone)."""
    import torch
    from janusx_amd._lib import check
    dev = torch.device("cuda:0")
    d, e = R.matrix(case)
    n = len(d)
    d_a = torch.from_numpy(R.dense(d, e)).to(dev)
    d_d = torch.zeros(n, dtype=torch.float64, device=dev)
    d_e = torch.zeros(n, dtype=torch.float64, device=dev)
    hf = (ctypes.c_int * 4)()
    check(_lib().jxg_sy2st_f64(d_a.data_ptr(), n, d_d.data_ptr(), d_e.data_ptr(), None, hf, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert list(hf)[:2] == [0, 0]
    amax = max(float(np.max(np.abs(d))), float(np.max(np.abs(e))))
    dd = float(np.max(np.abs(d_d.cpu().numpy() - d)))
    de = float(np.max(np.abs(np.abs(d_e.cpu().numpy()[: n - 1]) - np.abs(e))))
    print(f"sy2st {R.case_id(case)}: d {dd:.2e} |e| {de:.2e} (max|A| {amax:.2e})")
    assert dd <= 1e-12 * amax and de <= 1e-12 * amax
