"""`jx pca` and the randomized SVD of packed genotypes (`rsvd_packed_subset`, `admx_rsvd_stream_sample`, the two skinny
products `jxg_packed_mm_cols` / `jxg_packed_tmm_cols`) against float64 numpy restatements in this file."""

import numpy as np
import pytest

from janusx_amd import bed

pytestmark = pytest.mark.gpu

N, M = 2000, 20000


def _panel_dosage(n=N, m=M, miss=0.01, seed=7):
    """Four subpopulations with distinct allele frequencies (three leading eigenvalues clear of the bulk), `miss` missing."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 0.9, m)
    pops = np.clip(base[None, :] + rng.normal(0.0, 0.15, (4, m)), 0.05, 0.95)
    lab = np.arange(n) % 4
    g = rng.binomial(2, pops[lab].T).astype(np.int8)            # (m, n)
    if miss > 0:
        g[rng.random(g.shape) < miss] = -1
    return g


_CACHE = {}


def _data():
    if "g" not in _CACHE:
        g = _panel_dosage()
        _CACHE["g"] = g
        _CACHE["packed"] = bed.pack_dosage(g)
    return _CACHE["g"], _CACHE["packed"]


def _design(g):
    """Centred design of `packed_subset_row_stats` + `prepare_packed_block_centered_mean_scale_f32` (missing -> 0):
    -> Z (m, n) f64, maf f32, flip, varsum."""
    called = g >= 0
    nm = called.sum(1)
    alt = np.where(called, g, 0).sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(nm > 0, alt / (2.0 * np.maximum(nm, 1)), 0.0)
    flip = (nm > 0) & (p > 0.5)
    pm = np.where(flip, 1.0 - p, p)
    maf = pm.astype(np.float32)
    mean = (np.float32(2.0) * maf).astype(np.float64)
    gg = np.where(flip[:, None], 2.0 - g, g.astype(np.float64))
    z = np.where(called, gg - mean[:, None], 0.0)
    varsum = float(np.sum(np.where(nm > 0, 2.0 * pm * (1.0 - pm), 0.0)))
    return z, maf, flip, varsum


def _mgs(x):
    q = np.zeros_like(x)
    for j in range(x.shape[1]):
        v = x[:, j].copy()
        for i in range(j):
            v -= (q[:, i] @ v) * q[:, i]
        nrm = np.sqrt(v @ v)
        assert nrm > 1e-12
        q[:, j] = v / nrm
    return q


def _lu(x, eps=1e-10, ratio=1e-8):
    rows, cols = x.shape
    if rows < cols:
        return _mgs(x), False
    a = x.copy()
    piv = np.arange(rows)
    d = []
    for j in range(cols):
        pr = j + int(np.argmax(np.abs(a[j:, j])))
        if not abs(a[pr, j]) > eps:
            return _mgs(x), False
        if pr != j:
            a[[j, pr]] = a[[pr, j]]
            piv[[j, pr]] = piv[[pr, j]]
        d.append(abs(a[j, j]))
        a[j + 1:, j] /= a[j, j]
        a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j, j + 1:])
    if min(d) / max(d) < ratio:
        return _mgs(x), False
    lo = np.tril(a[:, :cols], -1)
    lo[np.arange(cols), np.arange(cols)] = 1.0
    q = np.empty_like(lo)
    q[piv] = lo
    return q / np.linalg.norm(q, axis=0)[None, :], True


def _rsvd_ref(z, varsum, k, seed, power, tol, mode, kp):
    """float64 restatement of rsvd.rs:1548-1661 (mode "lu") / adamixture.rs:3527-3720 (mode "svd") with the product's Omega."""
    from janusx_amd.janusx import rsvd_omega
    n = z.shape[1]
    k_eff = min(k, n, kp)
    y = z.T @ rsvd_omega(seed, z.shape[0], kp)
    q = _mgs(y) if mode == "lu" else np.linalg.svd(y, full_matrices=False)[0]
    sk = np.zeros(kp)
    alpha, q_is_qr, rounds = 0.0, True, 0
    for it in range(power):
        y = z.T @ (z @ q) - alpha * q
        if mode == "lu":
            if it + 1 >= power:
                q, q_is_qr = _mgs(y), True
            else:
                q, used = _lu(y)
                q_is_qr = not used
            s_y = np.sort(np.linalg.norm(y, axis=0))[::-1]
        else:
            u, s_y, _ = np.linalg.svd(y, full_matrices=False)
            q = u
        rounds = it + 1
        if it > 0:
            now = s_y[:k_eff] + alpha
            rel = np.abs(now - sk[:k_eff]) / np.maximum(now, 1e-12)
            sk[:k_eff] = now
            if rel.max() < tol:
                if mode == "lu" and not q_is_qr:
                    q, q_is_qr = _mgs(q), True
                break
        else:
            sk[:] = s_y + alpha
        if alpha < s_y[kp - 1]:
            alpha = 0.5 * (alpha + s_y[kp - 1])
    if mode == "lu" and not q_is_qr:
        q = _mgs(q)
    w = z @ q
    ev, v = np.linalg.eigh(w.T @ w)
    o = np.argsort(-ev)
    ev, v = np.maximum(ev[o], 1e-12), v[:, o]
    return ev[:k_eff] / varsum, q @ v[:, :k_eff], rounds


def _align(a, b):
    """b's columns sign-aligned to a's."""
    s = np.sign(np.sum(a * b, axis=0))
    s[s == 0] = 1.0
    return b * s[None, :]


def _exact(z, varsum, k):
    kk = z.T @ z / varsum
    ev, v = np.linalg.eigh(kk)
    return ev[::-1][:k], v[:, ::-1][:, :k], float(np.trace(kk))


# ---- the two skinny products against the bound their digit form gives ---------------------------------------------------------
#
# A column x of the dense block is written as xmax (q1/127 + q2/(127 254) + q3/(127 254^2) + q4/(127 254^3)) with the residual
# after four digits at most half a unit of the last one: |x / xmax - digits| <= RS_D.  Every integer plane sum is exact, so in
# exact arithmetic
#     |W[r][c] - (Z Q)[r][c]|  <= RS_D qmax_c sum_i |z_ri|
#     |Y[i][c] - (Z' W)[i][c]| <= RS_D (umax_c sum_r G_ri + vmax_c sum_r M_ri),     u = b W, v = a W
# (G the 0 / 1 / 2 dose plane of the stored code, M the missing plane).  What is left is float64 rounding: of the numpy reference
# (a sum of N products: N 2^-53 sum |terms|), of the kernel's merge of its exact sums (a dozen operations on terms no larger than
# the ones below) and, for Z' W, of the column constant sum_r a_r W_rc (N terms again), together under (N + 64) 2^-52 sum |terms|:
#     Z Q:  terms = |a_r| (sum_i |q_ic| + sum_i M_ri |q_ic|) + |b_r| sum_i G_ri |q_ic|
#     Z' W: terms = sum_r |v_rc| + sum_r G_ri |u_rc| + sum_r M_ri |v_rc|
# which dominate sum |z| |q| resp. sum |z| |w| of the reference.  A column whose entries are exact four-digit numbers of its
# maximum (`_exact_digit_block`) has no residual: there the bound is the rounding term alone.
RS_D = 0.5 / (127.0 * 254.0 ** 3)
RS_KP = [1, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]                   # both sides of every rs_nt step and of the 32-column pass


# The launch arithmetic of csrc/k_rsvd.hip restated: `rs_nt` (columns per pass / 4), the constexpr ST of `rs_main` (record tiles
# per LDS stage) and the slices / tps block of `jxg_packed_tmm_cols`.  The library exports none of them, so a change there has
# to be carried over here by hand; the shape assertions of the two edge tests then say which case lost its property.
def _rs_nt(kp):
    return 1 if kp <= 4 else 2 if kp <= 8 else 4 if kp <= 16 else 8


def _rs_st(kp, nv):
    """LDS stage length in record tiles (`rs_main`: ST) for Z Q (nv = 1) and Z' W (nv = 2)."""
    return min(8, max(1, 256 // (16 * _rs_nt(kp) * nv)))


def _rs_slices(n, nrows, kp):
    """-> (nst, slices, tps) of `jxg_packed_tmm_cols`."""
    cpp = 4 * _rs_nt(kp)
    ncb = (kp + cpp - 1) // cpp
    nst = (nrows + 127) // 128
    gx = (n + 255) // 256
    slices = max(1, min((1024 + gx * ncb - 1) // (gx * ncb), 64, nst))
    tps = min((nst + slices - 1) // slices, (1 << 23) // 128)
    return nst, (nst + tps - 1) // tps, tps


def _scales(kp):
    """Column scales over 300 decades, the two extremes in columns 0 and 2 (every block of three or more columns has both)."""
    order = [0, 31, 63] + [i for i in range(64) if i not in (0, 31, 63)]
    return (10.0 ** np.linspace(-150.0, 150.0, 64))[order][:kp]


def _gauss_block(rng, rows, kp):
    x = rng.standard_normal((rows, kp)) * _scales(kp)[None, :]
    if kp >= 3:
        x[:, 1] = 0.0                                             # a column of zeros between live columns
    return x


def _exact_digit_block(rng, rows, kp, top_row=0):
    """Columns x = s (q1/127 + q2/(127 254) + q3/(127 254^2) + q4/(127 254^3)) with integer digits in [-126, 126] and the
    entry of row `top_row` at digits (+-127, 0, 0, 0): the column maximum is exactly s and `rs_digits` recovers every digit."""
    dg = rng.integers(-126, 127, (rows, kp, 4)).astype(np.float64)
    dg[top_row] = 0.0
    dg[top_row, :, 0] = 127.0 * np.where(np.arange(kp) % 2 == 0, 1.0, -1.0)
    t = (((dg[..., 3] / 254.0 + dg[..., 2]) / 254.0 + dg[..., 1]) / 254.0 + dg[..., 0]) / 127.0
    x = t * _scales(kp)[None, :]
    if kp >= 3:
        x[:, 1] = 0.0
    return x


def _assert_within(err, bound, tag):
    ok = err <= bound                                             # False for a NaN error
    worst = float(np.max(err[~ok] / np.maximum(bound[~ok], np.finfo(np.float64).tiny))) if not ok.all() else 0.0
    assert ok.all(), (tag, "error / bound", worst)


class _Case:
    """One panel, row list and (a, b), with the float64 design z of the listed rows and their codes (for the planes G, M)."""

    def __init__(self, g, rows, ab):
        import torch
        from janusx_amd import janusx as jxrs
        from janusx_amd import pipeline as pl
        self.dev = torch.device("cuda", 0)
        self.n, self.nrows, self.ab = g.shape[1], len(rows), ab
        self.gr = np.ascontiguousarray(g[rows])
        self._gm = None
        self.z = np.where(self.gr >= 0, ab[:, :1] + ab[:, 1:] * np.maximum(self.gr, 0), 0.0)
        panel = pl.Panel(torch.from_numpy(bed.pack_dosage(g)).to(self.dev), self.n)
        self.op = jxrs._RsvdOperator(panel, np.asarray(rows, dtype=np.int32), ab)

    def _planes(self):
        """G and M as float64: kept for a small case, rebuilt per check for a large one (2 x 168 MB at 70 000 x 300)."""
        if self._gm is not None:
            return self._gm
        gm = np.maximum(self.gr, 0).astype(np.float64), (self.gr < 0).astype(np.float64)
        if self.gr.size <= 1 << 22:
            self._gm = gm
        return gm

    def check_zq(self, q, exact, tag):
        import torch
        qt = torch.from_numpy(np.ascontiguousarray(q)).to(self.dev)
        w = self.op.zq(qt)
        assert torch.equal(w, self.op.zq(qt)), tag                # two runs, the same bits
        gp, mp = self._planes()
        aq = np.abs(q)
        a, b = np.abs(self.ab[:, :1]), np.abs(self.ab[:, 1:])
        bound = (self.n + 64) * 2.0 ** -52 * (a * (aq.sum(0)[None, :] + mp @ aq) + b * (gp @ aq))
        if not exact:
            bound = bound + RS_D * aq.max(0)[None, :] * np.abs(self.z).sum(1)[:, None]
        _assert_within(np.abs(w.cpu().numpy() - self.z @ q), bound, tag)

    def check_ztw(self, w, exact, tag):
        import torch
        wt = torch.from_numpy(np.ascontiguousarray(w)).to(self.dev)
        y = self.op.ztw(wt)
        assert torch.equal(y, self.op.ztw(wt)), tag               # the fixed-order merge of the slices
        gp, mp = self._planes()
        u, v = np.abs(w * self.ab[:, 1:]), np.abs(w * self.ab[:, :1])
        bound = (self.nrows + 64) * 2.0 ** -52 * (v.sum(0)[None, :] + gp.T @ u + mp.T @ v)
        if not exact:
            bound = bound + RS_D * (u.max(0)[None, :] * gp.sum(0)[:, None] + v.max(0)[None, :] * mp.sum(0)[:, None])
        _assert_within(np.abs(y.cpu().numpy() - self.z.T @ w), bound, tag)


def _edge_dosage(n, m, seed):
    """2 % missing; row 5 monomorphic, row 6 all missing, sample 3 all missing (where the panel has them)."""
    g = _panel_dosage(n, m, 0.02, seed=seed)
    if m > 6:
        g[5] = 0
        g[6] = -1
    if n > 3:
        g[:, 3] = -1
    return g


def _descending_rows(m, nrows):
    """The lowest `nrows` of m rows in descending order (m_total != nrows; rows 5 and 6 are listed from 7 rows on)."""
    assert nrows < m
    return np.arange(nrows - 1, -1, -1)


def _real_case(n, m, nrows, seed):
    """The GRM method-1 design (a = -2 maf, b = 1; a = 2 - 2 maf, b = -1 on a flipped row; a = 0 on rows 5 and 6)."""
    from janusx_amd.janusx import _rsvd_row_design
    g = _edge_dosage(n, m, seed)
    _z, maf, flip, _ = _design(g)
    rows = _descending_rows(m, nrows)
    case = _Case(g, rows, _rsvd_row_design(maf[rows], flip[rows]))
    assert np.array_equal(case.z, _z[rows])                       # the design restated in `_design`, not the one under test
    return case


def _synthetic_case(n, m, nrows, seed):
    """A synthetic (a, b): a = +-0.8125 or 0, b = +-1.  With an exact-digit W both images of Z' W, u = b W and v = a W, are
    then exact-digit columns (v_rc = a_r w_rc is the kernel's own product; its maximum sits on row 0, where a != 0)."""
    g = _edge_dosage(n, m, seed)
    rng = np.random.default_rng(seed + 1)
    ab = np.empty((nrows, 2))
    ab[:, 1] = np.where(rng.random(nrows) < 0.3, -1.0, 1.0)
    ab[:, 0] = 0.8125 * np.where(rng.random(nrows) < 0.5, -1.0, 1.0)
    if nrows >= 4:
        ab[1::7, 0] = 0.0                                         # a = 0 rows
    return _Case(g, _descending_rows(m, nrows), ab)


def test_products_match_numpy_for_several_widths():
    """The shape this test has always had (n = 700, 777 of 900 rows in random order), held to the digit bound."""
    from janusx_amd.janusx import _rsvd_row_design
    rng = np.random.default_rng(3)
    n, m = 700, 900
    g = _panel_dosage(n, m, 0.02, seed=11)
    g[5] = 0
    g[6] = -1                                                     # monomorphic and all-missing rows
    _z, maf, flip, _ = _design(g)
    rows = rng.permutation(m)[:777].astype(np.int32)
    case = _Case(g, rows, _rsvd_row_design(maf[rows], flip[rows]))
    assert np.array_equal(case.z, _z[rows])                       # the design restated in `_design`, not the one under test
    for kp in (1, 5, 16, 33, 64):
        case.check_zq(rng.standard_normal((n, kp)) * np.logspace(0, 3, kp)[None, :], False, ("zq", kp))
        case.check_ztw(rng.standard_normal((len(rows), kp)), False, ("ztw", kp))


@pytest.mark.parametrize("n,m,nrows", [(130, 300, 257), (5000, 1100, 1000), (20000, 700, 600)])
def test_products_hold_the_digit_bound_and_exact_digit_columns(n, m, nrows):
    """Gaussian columns over 300 decades to the four-digit bound, exact-digit columns to float64 rounding alone."""
    rng = np.random.default_rng(n)
    real, syn = _real_case(n, m, nrows, 21), _synthetic_case(n, m, nrows, 22)
    for kp in (3, 16, 40):
        real.check_zq(_gauss_block(rng, n, kp), False, ("zq gauss", kp))
        real.check_ztw(_gauss_block(rng, nrows, kp), False, ("ztw gauss", kp))
        real.check_zq(_exact_digit_block(rng, n, kp, top_row=n - 1), True, ("zq exact", kp))
        syn.check_zq(_exact_digit_block(rng, n, kp), True, ("zq exact, synthetic ab", kp))
        syn.check_ztw(_exact_digit_block(rng, nrows, kp), True, ("ztw exact", kp))
        syn.check_ztw(_gauss_block(rng, nrows, kp), False, ("ztw gauss, synthetic ab", kp))


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases (host planes, P32 / T32 images) live for this module only."""
    yield
    _CASES.clear()


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


@pytest.mark.parametrize("kp", RS_KP)
def test_zq_through_its_stage_edges(kp):
    """Z Q at sample counts below, at and above one tile, and at 11 tiles: two or more LDS stages with a ragged last one for
    every stage length, a last tile of 21 samples."""
    st = _rs_st(kp, 1)
    assert st == {1: 8, 2: 8, 4: 4, 8: 2}[_rs_nt(kp)]
    for n in (100, 128, 129, 1301):
        tiles = (n + 127) // 128
        if n == 1301:
            assert tiles == 11 and tiles > st and tiles % st != 0 and n % 128 == 21 and n % 16 != 0
        real = _cached(("zq real", n), lambda: _real_case(n, 400, 333, 31))
        syn = _cached(("zq syn", n), lambda: _synthetic_case(n, 400, 333, 32))
        rng = np.random.default_rng(1000 * n + kp)
        real.check_zq(_gauss_block(rng, n, kp), False, ("gauss", n, kp))
        real.check_zq(_exact_digit_block(rng, n, kp, top_row=n - 1), True, ("exact", n, kp))
        syn.check_zq(_exact_digit_block(rng, n, kp), True, ("exact, synthetic ab", n, kp))


@pytest.mark.parametrize("kp", RS_KP)
def test_ztw_through_its_slice_edges(kp):
    """Z' W with one slice (1, 127, 128 rows), two slices of one tile (129 rows) and 70 000 rows x 300 samples: 61 slices of
    9 tiles, longer than the longest LDS stage, the last slice of 7."""
    n = 300
    st = _rs_st(kp, 2)
    assert st == {1: 8, 2: 4, 4: 2, 8: 1}[_rs_nt(kp)]
    for nrows in (1, 127, 128, 129, 70000):
        nst, slices, tps = _rs_slices(n, nrows, kp)
        if nrows <= 128:
            assert (nst, slices, tps) == (1, 1, 1)
        elif nrows == 129:
            assert (nst, slices, tps) == (2, 2, 1)
        else:
            assert (nst, slices, tps) == (547, 61, 9) and tps > st and nst - (slices - 1) * tps == 7
        real = _cached(("ztw real", nrows), lambda: _real_case(n, nrows + 13, nrows, 41))
        syn = _cached(("ztw syn", nrows), lambda: _synthetic_case(n, nrows + 13, nrows, 42))
        rng = np.random.default_rng(1000 * nrows + kp)
        real.check_ztw(_gauss_block(rng, nrows, kp), False, ("gauss", nrows, kp))
        syn.check_ztw(_exact_digit_block(rng, nrows, kp), True, ("exact", nrows, kp))
        syn.check_ztw(_gauss_block(rng, nrows, kp), False, ("gauss, synthetic ab", nrows, kp))


def test_rsvd_packed_subset_parity_with_restatement():
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    z, maf, flip, varsum = _design(g)
    ev, vec, maf_o, flip_o, rounds = jxrs._rsvd_packed_subset(packed, N, 5, None, 42, 5, 0.1)
    np.testing.assert_array_equal(maf_o, maf)
    np.testing.assert_array_equal(flip_o, flip)
    rev, rvec, rr = _rsvd_ref(z, varsum, 5, 42, 5, np.float32(0.1), "lu", 20)
    assert rounds == rr
    assert np.max(np.abs(ev - rev) / rev) < 1e-5
    assert np.abs(_align(rvec, vec) - rvec).max() < 1e-4


def test_admx_rsvd_parity_with_restatement(tmp_path):
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    g = g.copy()
    g[:50] = np.where(g[:50] >= 0, 0, g[:50])                     # rare rows that the maf filter drops
    prefix = str(tmp_path / "p")
    m = g.shape[0]
    bim = bed.Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * (m - 7) + ["AT"] * 7, ["G"] * m)
    bed.write_bed(prefix, bed.pack_dosage(g), [f"s{i}" for i in range(N)], bim)
    ev, vec, tv, rounds = jxrs._admx_rsvd(prefix, 4, 42, 5, 0.1, True, 0.02, 0.05)
    called = g >= 0
    miss = 1.0 - called.mean(1)
    alt = np.where(called, g, 0).sum(1) / (2.0 * np.maximum(called.sum(1), 1))
    keep = (np.minimum(alt, 1 - alt) >= 0.02) & (miss <= 0.05)
    keep[m - 7:] = False
    z, _maf, _flip, _ = _design(g[keep])
    f = _maf.astype(np.float64)
    varsum = float(np.sum(2.0 * f * (1.0 - f)))
    rev, rvec, rr = _rsvd_ref(z, varsum, 4, 42, 5, np.float32(0.1), "svd", 12)
    assert rounds == rr
    assert np.max(np.abs(ev - rev) / rev) < 1e-5
    assert np.abs(_align(rvec, vec) - rvec).max() < 1e-4
    assert abs(tv - float(np.sum(z * z)) / varsum) < 1e-9 * tv


def test_converged_accuracy_and_defaults():
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    z, _maf, _flip, varsum = _design(g)
    eev, evec, _tr = _exact(z, varsum, 5)
    ev, vec, *_ = jxrs.rsvd_packed_subset(packed, N, 5, seed=42, power=30, tol=1e-7)
    # components 4 and 5 sit in the bulk (1.62, 1.61: not separated); the shift alpha of the method moves towards the tail of the
    # spectrum, where the centring null vector (eigenvalue 0) competes with the bulk edge, so only the three separated
    # components converge to the exact eigenpairs -- the restatement above (same control flow) reaches the same values
    assert np.max(np.abs(ev[:3] - eev[:3]) / eev[:3]) < 1e-5
    cos = np.abs(np.sum(vec.astype(np.float64) * evec, axis=0)) / np.linalg.norm(vec.astype(np.float64), axis=0)
    assert np.all(cos[:3] >= 1 - 1e-6), cos
    ev3, vec3, *_ = jxrs.rsvd_packed_subset(packed, N, 3, seed=42, power=3, tol=0.1)
    qa = np.linalg.qr(vec3.astype(np.float64))[0]
    sv = np.linalg.svd(qa.T @ evec[:, :3], compute_uv=False)
    assert sv.min() >= 0.999, sv
    assert np.max(np.abs(ev3 - eev[:3]) / eev[:3]) < 0.01


def test_invariances():
    import torch
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    a = jxrs.rsvd_packed_subset(packed, N, 5)
    b = jxrs.rsvd_packed_subset(packed, N, 5)
    c = jxrs.rsvd_packed_subset(torch.from_numpy(packed).cuda(), N, 5)
    for x, y in ((a, b), (a, c)):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    idx = np.random.default_rng(5).permutation(N)[:1500]
    s1 = jxrs.rsvd_packed_subset(packed, N, 4, sample_indices=idx)
    s2 = jxrs.rsvd_packed_subset(bed.pack_dosage(g[:, idx]), len(idx), 4)
    for u, v in zip(s1, s2):
        np.testing.assert_array_equal(u, v)
    gf = g.copy()
    rows = np.arange(0, M, 97)
    gf[rows] = np.where(gf[rows] >= 0, 2 - gf[rows], -1)
    # converged runs: a row with p = 0.5 exactly keeps flip = False either way, so its sign (and the start block's product) changes
    a = jxrs.rsvd_packed_subset(packed, N, 3, power=30, tol=1e-7)
    f = jxrs.rsvd_packed_subset(bed.pack_dosage(gf), N, 3, power=30, tol=1e-7)
    assert np.max(np.abs(f[0] - a[0]) / a[0]) < 1e-6
    assert np.abs(_align(a[1], f[1]) - a[1]).max() < 1e-6


def test_edge_cases():
    from janusx_amd import janusx as jxrs
    g = _panel_dosage(40, 15, 0.01, seed=2)
    ev, vec, _maf, _flip = jxrs.rsvd_packed_subset(bed.pack_dosage(g), 40, 60)      # k >= n, kp capped by m
    assert vec.shape == (40, 15) and ev.shape == (15,)
    z, _m, _f, varsum = _design(g)
    eev = np.linalg.eigvalsh(z.T @ z / varsum)[::-1]
    assert np.max(np.abs(ev[:10] - eev[:10]) / eev[:10]) < 1e-5
    g = _panel_dosage(300, 400, 0.01, seed=4)
    g[3] = 2
    g[4] = -1                                                                      # monomorphic and all-missing rows
    ev, vec, maf, flip = jxrs.rsvd_packed_subset(bed.pack_dosage(g), 300, 3, power=30, tol=1e-7)
    assert maf[3] == 0.0 and flip[3] and maf[4] == 0.0 and not flip[4]
    z, _m, _f, varsum = _design(g)
    eev = np.linalg.eigvalsh(z.T @ z / varsum)[::-1]
    assert np.max(np.abs(ev - eev[:3]) / eev[:3]) < 1e-5


def _write_panel(tmp_path):
    g, packed = _data()
    prefix = str(tmp_path / "cohort")
    bim = bed.Bim(["1"] * M, [f"rs{j}" for j in range(M)], list(range(1, M + 1)), ["A"] * M, ["G"] * M)
    bed.write_bed(prefix, packed, [f"s{i}" for i in range(N)], bim)
    called = g >= 0
    alt = np.where(called, g, 0).sum(1) / (2.0 * np.maximum(called.sum(1), 1))
    keep = (np.minimum(alt, 1 - alt) >= 0.02) & (1.0 - called.mean(1) <= 0.05)
    z, _maf, _flip, varsum = _design(g[keep])
    return prefix, z, varsum


def _read_vec(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows])


def test_cli_pca_routes(tmp_path):
    from janusx_amd import cli
    prefix, z, varsum = _write_panel(tmp_path)
    kk = z.T @ z / varsum
    eev, evec = np.linalg.eigh(kk)
    eev, evec = eev[::-1], evec[:, ::-1]
    out = str(tmp_path / "a")
    assert cli.main(["pca", "-bfile", prefix, "-o", out]) == 0
    ids, vec = _read_vec(out + ".eigenvec")
    assert ids == [f"s{i}" for i in range(N)] and vec.shape == (N, 3)
    lines = open(out + ".eigenvec").read().splitlines()
    assert all(len(f.split(".")[1]) == 6 for f in lines[0].split("\t")[1:])
    tab = np.loadtxt(out + ".eigenval")
    assert tab.shape == (N, 2)
    top = slice(0, 3)
    assert np.max(np.abs(tab[top, 0] - eev[top]) / eev[top]) < 1e-6
    np.testing.assert_allclose(tab[:, 1], tab[:, 0] / tab[:, 0].sum(), atol=2e-8)
    assert np.abs(_align(evec[:, top], vec) - evec[:, top]).max() <= 2e-6
    # -k on the GRM written by `jx grm`
    gout = str(tmp_path / "g")
    assert cli.main(["grm", "-bfile", prefix, "-o", gout]) == 0
    out2 = str(tmp_path / "b")
    assert cli.main(["pca", "-k", gout, "-o", out2]) == 0
    _, vec2 = _read_vec(out2 + ".eigenvec")
    assert np.abs(_align(vec, vec2) - vec).max() <= 2e-6
    tab2 = np.loadtxt(out2 + ".eigenval")
    assert np.max(np.abs(tab2[top, 0] - tab[top, 0]) / tab[top, 0]) < 1e-6
    assert cli.main(["pca", "-k", gout + ".cGRM.npy", "-o", out2]) == 0
    # -rsvd: k_eff rows, ratio over trace(K)
    out3 = str(tmp_path / "c")
    assert cli.main(["pca", "-bfile", prefix, "-rsvd", "3", "0.1", "-dim", "5", "-o", out3]) == 0
    t3 = np.loadtxt(out3 + ".eigenval")
    assert t3.shape == (5, 2)
    np.testing.assert_allclose(t3[:, 1], t3[:, 0] / np.trace(kk), rtol=1e-5, atol=1e-8)
    _, v3 = _read_vec(out3 + ".eigenvec")
    assert v3.shape == (N, 5)


def test_lu_rounds_hold_no_n_by_n_object():
    """The LU normalisation works on the n x kp block alone: at n = 60 000 a dense permutation (or any n x n object) would take
    28.8 GB of device memory."""
    import torch
    from janusx_amd import janusx as jxrs
    n = 60000
    g = _panel_dosage(n, 1500, 0.01, seed=9)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev, vec, _maf, _flip, rounds = jxrs._rsvd_packed_subset(bed.pack_dosage(g), n, 3, None, 42, 5, 1e-7)
    torch.cuda.synchronize()
    assert rounds >= 2 and vec.shape == (n, 3) and np.all(ev > 0)          # rounds before the last normalise by LU
    assert torch.cuda.max_memory_allocated() - base < (1 << 30)
