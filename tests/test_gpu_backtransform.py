"""The two back-transformations of the two-stage eigensolver as stages of their own (csrc/k_sbback.hip: C <- Q2 C, csrc/k_ormtr.hip:
C <- Q1 C; the last stages behind src/math/eigh.rs:1422-1528), every kernel form at sizes of a few hundred rows.

The stage entries jxg_sbback_apply_f64 / jxg_ormtr_apply_f64 take the reflectors from the caller, so they are made on the CPU
(Q2: scripts/proto_twostage.py `sb2st` on a random band matrix; Q1: random vectors) and no reduction runs first.  Which Q2 kernel
the product launches depends on n and the CU count; here the form, the units per slab and the groups per launch are arguments.

Reference: every Householder reflector applied on its own, last generated first, in numpy.longdouble, rounded to f64 at the end;
once per n on one random n x n matrix C (a case with ncols < n takes the leading columns: columns are independent).
Bar: for every column j  max|got_j - ref_j| <= 1e-12 ||C_j||_2 -- the project's bar for unit-norm eigenvectors after both stages at
these sizes (test_eigh_panel_and_tail_boundaries).  The grouped compact-WY application in f64 lies 4e-16 .. 5e-16 from this
reference (proto_twostage.apply_q2, g = 32, b = 64, n = 131 .. 700), so a correct kernel has three orders of magnitude of room
and a wrong tile, slab edge or group boundary misses the bar by twelve.
C sits in the middle of a larger buffer; the sentinel columns in front of and behind it must come back bit-unchanged.  Memory
the contracts call meaningless is NaN: v2 off the supports (the product's v2 is a scratch lease nobody clears), A on and above
the implicit unit entries and right of the last reflector, tau behind the last reflector.

Largest error / bar measured on an MI355X (256 CUs), over all cases of this file:
    Q2  three waves per unit 4.0e-16   one wave per unit 5.3e-16   two groups per pass 5.3e-16   balanced 5.3e-16
    Q1  6.5e-16
(in units of ||C_j||_2: the bar is 1e-12).  The bar stays where it is.
"""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12
GUARD = 3                      # sentinel columns on either side of C
FORMS = {"reg": 0, "solo": 1, "pair": 2, "bal": 3}
NU_RANGE = {"reg": range(1, 6), "solo": range(4, 12), "pair": range(4, 8), "bal": range(4, 8)}
LD = np.longdouble
_WORST = {}                    # form name -> largest error / ||C_j|| seen (printed; `pytest -s` shows it)


def _proto():
    spec = importlib.util.spec_from_file_location("proto_twostage", os.path.join(ROOT, "scripts", "proto_twostage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lib():
    from janusx_amd._lib import lib
    return lib()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _sb():
    return int(_lib().jxg_eigh_bandwidth())


def _steps_of_sweep(n, s):
    """supports of the reflectors of sweep s: [(k, first row, rows)]"""
    sb, out, k = _sb(), [], 0
    if s >= n - 2:
        return out
    while s + 1 + k * sb < n:
        r = s + 1 + k * sb
        out.append((k, r, min(sb, n - r)))
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def _c_matrix(n):
    """the random C of size n, as (column, row): row j of the array is column j of the column-major matrix"""
    return np.random.default_rng(1000 + n).standard_normal((n, n))


def _apply_q2_ref(n, v2, tau2, c_cols):
    """(column, row) array <- Q2 C, reflector by reflector in long double: the last generated first"""
    c = c_cols.astype(LD)
    for s in range(n - 3, -1, -1):
        for k, r, ln in reversed(_steps_of_sweep(n, s)):
            tau = LD(tau2[s, k])
            if tau == 0:
                continue
            v = v2[s, r:r + ln].astype(LD)
            sub = c[:, r:r + ln]
            sub -= np.multiply.outer(tau * (sub @ v), v)
    return c


@functools.lru_cache(maxsize=None)
def _q2_case(n):
    """reflectors of the bulge chasing of a random symmetric band matrix in the kernels' layout, and the reference"""
    import torch
    sb, ks = _sb(), int(_lib().jxg_sb2st_steps(n))
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n))
    a = np.tril(np.triu(a + a.T, -sb), sb)
    _, refl = _proto().sb2st(a, sb)
    v2 = np.full((n, n), np.nan)               # v2[s, row] = element row + s n; NaN off the supports
    tau2 = np.zeros((n, ks))                   # zero where no step exists (the product clears it)
    for s in range(n - 2):
        for k, r, ln in _steps_of_sweep(n, s):
            r0, v, tau = refl[(s, k)]
            assert r0 == r and len(v) == ln
            v2[s, r:r + ln] = v
            tau2[s, k] = tau
    assert len(refl) == sum(len(_steps_of_sweep(n, s)) for s in range(n - 2))
    c = _c_matrix(n)
    ref = _apply_q2_ref(n, v2, tau2, c).astype(np.float64)
    dev = torch.device("cuda:0")
    return {"n": n, "ks": ks, "v2": v2, "tau2": tau2, "c": c, "ref": ref, "cnorm": np.linalg.norm(c, axis=1),
            "d_v2": torch.from_numpy(v2).to(dev), "d_tau2": torch.from_numpy(tau2).to(dev)}


def _guarded(c_cols):
    """device buffer [GUARD sentinel columns | C | GUARD sentinel columns] and the sentinels' bits"""
    import torch
    ncols, n = c_cols.shape
    buf = np.empty((ncols + 2 * GUARD, n))
    sent = np.random.default_rng(7).standard_normal((2 * GUARD, n)) + 3.0
    buf[:GUARD] = sent[:GUARD]
    buf[GUARD + ncols:] = sent[GUARD:]
    buf[GUARD:GUARD + ncols] = c_cols
    return torch.from_numpy(buf).to("cuda:0"), sent


def _finish(d_buf, sent, ncols):
    import torch
    torch.cuda.synchronize()
    out = d_buf.cpu().numpy()
    assert np.array_equal(out[:GUARD].view(np.int64), sent[:GUARD].view(np.int64)), "columns in front of C were written"
    assert np.array_equal(out[GUARD + ncols:].view(np.int64), sent[GUARD:].view(np.int64)), "columns behind C were written"
    return out[GUARD:GUARD + ncols]


def _run_q2(case, ncols, form, nu, gpl=0, d_tau2=None):
    from janusx_amd._lib import check
    n = case["n"]
    d_buf, sent = _guarded(case["c"][:ncols])
    info = (ctypes.c_int * 4)()
    d_t = case["d_tau2"] if d_tau2 is None else d_tau2
    check(_lib().jxg_sbback_apply_f64(case["d_v2"].data_ptr(), d_t.data_ptr(), n, d_buf.data_ptr() + GUARD * n * 8, ncols, form, nu,
                                      gpl, info, _stream()))
    return _finish(d_buf, sent, ncols), list(info)


def _err(got, ref, cnorm):
    """largest over the columns of max|got_j - ref_j| / ||C_j||_2 (NaN counts as infinite)"""
    d = np.abs(got - ref).max(axis=1) / cnorm[:got.shape[0]]
    return float(np.where(np.isnan(d), np.inf, d).max())


def _check(tag, name, got, ref, cnorm):
    e = _err(got, ref[:got.shape[0]], cnorm)
    _WORST[name] = max(_WORST.get(name, 0.0), e)
    print(f"{tag}: err/||C_j|| = {e:.2e}")
    assert e <= BAR, f"{tag}: {e:.3e} > {BAR:g}"
    return e


def _slabs(units, nu):
    return -(-units // nu)


def _feasible(units, nu):
    """what jxg_sbback_apply_f64 accepts: no slab of the even deal holds fewer than nu - 1 units"""
    return units >= 1 and units // _slabs(units, nu) >= nu - 1


def _widest(units, nu):
    return -(-units // _slabs(units, nu))


def _full(units, nu):
    """... and at least one slab holds all nu units of the instantiation"""
    return _feasible(units, nu) and _widest(units, nu) == nu


def _instantiation_columns(nu):
    """n and the column counts for `nu` units per slab: n itself (when the even deal of its units gives slabs of nu or nu - 1; with
    10 units per slab neither 21 nor 44 units do, 40 do), one exact multiple of 16, and a last unit of 1, 4, 5, 13 and 15 columns"""
    n = next((m for m in (321, 700) if _full(-(-m // 16), nu)), 700)
    cols = []
    if _full(-(-n // 16), nu):
        cols.append(n)
    cols.append(16 * max(u for u in range(1, n // 16 + 1) if _full(u, nu)))
    for w in (1, 4, 5, 13, 15):
        cols.append(max(16 * (u - 1) + w for u in range(1, -(-n // 16) + 1) if _full(u, nu) and 16 * (u - 1) + w <= n))
    return n, list(dict.fromkeys(cols))        # (n = 321 is itself a last unit of one column)


INSTANTIATIONS = [(f, nu) for f in ("reg", "solo", "pair", "bal") for nu in NU_RANGE[f]]


@pytest.mark.gpu
@pytest.mark.parametrize("form,nu", INSTANTIATIONS, ids=[f"{f}{nu}" for f, nu in INSTANTIATIONS])
def test_q2_every_instantiation(form, nu):
    """All 21 template instantiations behind sbback_apply_q2 -- sbback_apply_reg_kernel<1..5>, sbback_apply_solo_kernel<4..11>,
    sbback_apply_pair_kernel<4..7>, sbback_apply_bal_kernel<64|80|96|112> -- at n = 321 (21 units) or n = 700 (44 units), with all
    columns, whole units only, and a ragged last unit of 1, 4, 5, 13 and 15 columns."""
    n, cols = _instantiation_columns(nu)
    case = _q2_case(n)
    assert len(cols) >= 6 and (n in cols or nu == 10)
    for ncols in cols:
        got, info = _run_q2(case, ncols, FORMS[form], nu)
        units = -(-ncols // 16)
        assert info == [FORMS[form], nu, _slabs(units, nu), 1], (ncols, info)
        _check(f"Q2 {form}<{nu}> n={n} ncols={ncols}", form, got, case["ref"], case["cnorm"])


@pytest.mark.gpu
@pytest.mark.parametrize("nu,pos", [(5, 5), (6, 5), (6, 6), (7, 6), (7, 7)])
def test_q2_balanced_four_column_waves(nu, pos):
    """Balanced form, five units per slab and more: the units beyond the fourth of a slab belong to the four-column waves (wave 4 + i
    owns the columns 4 i .. 4 i + 3 of each).  The column count ends inside unit `pos` of the last slab at 1, 4, 5, 8, 9 and 16
    columns of that unit: a wave of that unit is empty, partly filled or full."""
    n = 321
    case = _q2_case(n)
    units = max(u for u in range(1, n // 16 + 1) if _feasible(u, nu) and _widest(u, nu) == pos)
    for w in (1, 4, 5, 8, 9, 16):
        ncols = 16 * (units - 1) + w
        got, info = _run_q2(case, ncols, FORMS["bal"], nu)
        assert info == [3, nu, _slabs(units, nu), 1], info
        _check(f"Q2 bal<{nu}> n={n} last slab ends in unit {pos} at {w} columns (ncols={ncols})", "bal", got, case["ref"], case["cnorm"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [131, 194, 258])
def test_q2_size_edges(n):
    """The smallest two-stage size (131: five groups, a last step of two rows), 194 (six groups, a last step of one row) and 258
    (last steps of one and of 64 rows); odd n pads a row pair of the slab layout.  reg 1..5, the other forms with 4 and 5 units."""
    case = _q2_case(n)
    units = -(-n // 16)
    for form in ("reg", "solo", "pair", "bal"):
        for nu in (NU_RANGE[form] if form == "reg" else (4, 5)):
            assert _feasible(units, nu)
            got, info = _run_q2(case, n, FORMS[form], nu)
            assert info == [FORMS[form], nu, _slabs(units, nu), 1], info
            _check(f"Q2 {form}<{nu}> n={n}", form, got, case["ref"], case["cnorm"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [131, 194])
@pytest.mark.parametrize("form,nu", [("reg", 2), ("reg", 5), ("pair", 4), ("pair", 5), ("bal", 4), ("bal", 5)])
def test_q2_launch_boundaries(n, form, nu):
    """Launches of one and of three groups against one launch (n = 131: five groups, n = 194: six).  A pass of the
    two-groups-per-pass kernels then ends on a single group at a launch edge.  Every block does the same arithmetic on the same
    rows wherever the launch edges fall (blocks that change places work on disjoint rows), so the bits are those of one launch."""
    case = _q2_case(n)
    ngroups = (n - 2 + 31) // 32
    one, info = _run_q2(case, n, FORMS[form], nu)
    assert info[3] == 1
    _check(f"Q2 {form}<{nu}> n={n} one launch", form, one, case["ref"], case["cnorm"])
    for gpl in (1, 3):
        got, info = _run_q2(case, n, FORMS[form], nu, gpl=gpl)
        assert info[3] == -(-ngroups // gpl), info
        _check(f"Q2 {form}<{nu}> n={n} groups per launch {gpl}", form, got, case["ref"], case["cnorm"])
        assert np.array_equal(got.view(np.int64), one.view(np.int64)), f"{gpl} groups per launch differ from one launch"


@pytest.mark.gpu
def test_q2_product_plan():
    """form = -1 is the product's own plan: at n = 700 (44 units, far below three units per CU) the three-waves form with
    ceil(units / CUs) units per slab, in one launch."""
    import torch
    n = 700
    case = _q2_case(n)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    units = -(-n // 16)
    assert units <= 2 * cus
    nu = max(-(-units // cus), 1)
    got, info = _run_q2(case, n, -1, 0)
    assert info == [0, nu, _slabs(units, nu), 1], info
    _check(f"Q2 product plan n={n}", "reg", got, case["ref"], case["cnorm"])


@pytest.mark.gpu
def test_q2_refuses_what_the_plans_cannot_produce():
    """units per slab without a kernel, a slab with fewer than nu - 1 units, n below the smallest two-stage size: an error before
    any launch (C untouched)."""
    case = _q2_case(131)
    n = 131
    for form, nu, ncols in ((0, 0, n), (0, 6, n), (1, 3, n), (1, 12, n), (2, 8, n), (3, 8, n), (4, 4, n), (1, 7, n), (0, 3, 0), (0, 3, n + 1)):
        d_buf, sent = _guarded(case["c"][:max(min(ncols, n), 1)])
        rc = _lib().jxg_sbback_apply_f64(case["d_v2"].data_ptr(), case["d_tau2"].data_ptr(), n, d_buf.data_ptr() + GUARD * n * 8, ncols,
                                         form, nu, 0, None, _stream())
        assert rc != 0, (form, nu, ncols)
        got = _finish(d_buf, sent, max(min(ncols, n), 1))
        assert np.array_equal(got, case["c"][:got.shape[0]])
    d_buf, sent = _guarded(case["c"][:4, :130].copy())
    assert _lib().jxg_sbback_apply_f64(case["d_v2"].data_ptr(), case["d_tau2"].data_ptr(), 130, d_buf.data_ptr() + GUARD * 130 * 8, 4, 0, 1, 0,
                                       None, _stream()) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one_group", "all"])
def test_q2_degenerate_reflectors(which):
    """tau = 0 for one whole group of sweeps (every step of the sweeps 32 .. 63), and for all of them (what a diagonal input
    gives): identity reflectors, whatever their vectors hold."""
    import torch
    n = 321
    case = _q2_case(n)
    tau2 = case["tau2"].copy()
    if which == "all":
        tau2[:] = 0.0
        ref = case["c"]
    else:
        tau2[32:64] = 0.0
        ref = _apply_q2_ref(n, case["v2"], tau2, case["c"]).astype(np.float64)
    d_tau2 = torch.from_numpy(tau2).to("cuda:0")
    for form, nu in ((-1, 0), (0, 3), (1, 4), (2, 5), (3, 6)):
        got, info = _run_q2(case, n, form, nu, d_tau2=d_tau2)
        name = [k for k, v in FORMS.items() if v == info[0]][0]
        _check(f"Q2 {name}<{info[1]}> n={n} tau = 0 for {which}", name, got, ref, case["cnorm"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [321, 700])
def test_q2_lockstep_units_give_the_bits_of_staggered_units(n, monkeypatch):
    """JXGPU_QB_SKIP=64 (read per call): the lockstep three-waves form does the same operations in the same order per unit as the
    staggered one -- the small sibling of test_q2_staggered_units_equal_lockstep."""
    case = _q2_case(n)
    units = -(-n // 16)
    for nu in NU_RANGE["reg"]:
        assert _feasible(units, nu)
        monkeypatch.delenv("JXGPU_QB_SKIP", raising=False)
        stag, _ = _run_q2(case, n, 0, nu)
        monkeypatch.setenv("JXGPU_QB_SKIP", "64")
        lock, _ = _run_q2(case, n, 0, nu)
        monkeypatch.delenv("JXGPU_QB_SKIP", raising=False)
        _check(f"Q2 reg<{nu}> n={n} lockstep", "reg", lock, case["ref"], case["cnorm"])
        assert np.array_equal(stag.view(np.int64), lock.view(np.int64)), nu


# ---- Q1 ---------------------------------------------------------------------------------------------------------------------

def _apply_q1_ref(n, off, nref, a, tau, c_cols):
    """(column, row) array <- H_0 H_1 ... H_(nref-1) C in long double; a[j, row] = A(row, j)"""
    c = c_cols.astype(LD)
    for j in range(nref - 1, -1, -1):
        t = LD(tau[j])
        if t == 0:
            continue
        v = np.concatenate(([1.0], a[j, j + off + 1:])).astype(LD)
        sub = c[:, j + off:]
        sub -= np.multiply.outer(t * (sub @ v), v)
    return c


@functools.lru_cache(maxsize=None)
def _q1_case(n, off, nref):
    import torch
    rng = np.random.default_rng(100 * n + off)
    a = np.full((n, n), np.nan)                # a[j, row]: NaN on and above the unit entries and right of the last reflector
    tau = np.full(n, np.nan)
    for j in range(nref):
        v = rng.standard_normal(n - j - off - 1)
        a[j, j + off + 1:] = v
        tau[j] = 2.0 / (1.0 + v @ v)
    for j in {0, 5, nref // 2, min(64, nref - 1), nref - 1}:
        tau[j] = 0.0                           # identity reflectors (their vectors stay)
    c = _c_matrix(n)
    ref = _apply_q1_ref(n, off, nref, a, tau, c).astype(np.float64)
    return {"n": n, "c": c, "ref": ref, "cnorm": np.linalg.norm(c, axis=1), "d_a": torch.from_numpy(a).to("cuda:0"),
            "d_tau": torch.from_numpy(tau).to("cuda:0")}


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [None, "64", "256"])
@pytest.mark.parametrize("n,off,nref", [(700, 64, 635), (700, 1, 699), (258, 64, 193), (131, 64, 66)])
def test_q1_random_reflectors(n, off, nref, nb, monkeypatch):
    """ormtr_lower_off as the eigensolver calls it (off = 64: behind the band reduction; off = 1: behind the one-stage
    tridiagonalisation) with JXGPU_ORMTR_NB unset / 64 / 256 (read per call) -- at n = 700: one block; ten blocks with a ragged last
    one of 59; blocks of 256, 256 and 123; the triangular inverse at one, two and three levels -- and 1, 5, 17, 127, 129 and n
    columns."""
    from janusx_amd._lib import check
    case = _q1_case(n, off, nref)
    if nb is None:
        monkeypatch.delenv("JXGPU_ORMTR_NB", raising=False)
    else:
        monkeypatch.setenv("JXGPU_ORMTR_NB", nb)
    for ncols in (1, 5, 17, 127, 129, n):
        d_buf, sent = _guarded(case["c"][:ncols])
        check(_lib().jxg_ormtr_apply_f64(case["d_a"].data_ptr(), case["d_tau"].data_ptr(), n, off, nref, d_buf.data_ptr() + GUARD * n * 8,
                                         ncols, _stream()))
        got = _finish(d_buf, sent, ncols)
        _check(f"Q1 n={n} off={off} nref={nref} nb={nb} ncols={ncols}", "q1", got, case["ref"], case["cnorm"])


# ---- the device's own reflectors ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [131, 258, 700])
def test_device_reflectors_satisfy_the_contract(n):
    """The reflectors the two reduction stages write are the ones the layout above describes: with Q1 and Q2 formed from them
    reflector by reflector (long double, on the identity; rounded to f64 for the products), Q1' A Q1 is the band matrix stage 1
    hands to stage 2, Q2' B Q2 is the tridiagonal matrix, both within 1e-12 max|A| (the factor
    test_bulge_chasing_position_owned_equals_sweep_owned applies to T's spectrum), and Q2 leaves the first coordinate alone."""
    import torch
    from janusx_amd._lib import check
    sb, ks = _sb(), int(_lib().jxg_sb2st_steps(n))
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    z = torch.randn((n, 2 * n), generator=g, device=dev, dtype=torch.float64)
    a = z @ z.T / (2 * n)
    a = 0.5 * (a + a.T)
    a.diagonal().add_(1e-6)
    w = a.clone()
    d = torch.zeros(n, device=dev, dtype=torch.float64)
    e = torch.zeros(n, device=dev, dtype=torch.float64)
    ab = torch.zeros((n, 2 * sb), device=dev, dtype=torch.float64)
    tau = torch.zeros(n, device=dev, dtype=torch.float64)
    v2 = torch.zeros((n, n), device=dev, dtype=torch.float64)
    tau2 = torch.full((n, ks), float("nan"), device=dev, dtype=torch.float64)
    hf = (ctypes.c_int * 4)()
    check(_lib().jxg_sy2st_reflectors_f64(w.data_ptr(), n, d.data_ptr(), e.data_ptr(), ab.data_ptr(), hf, tau.data_ptr(), v2.data_ptr(),
                                          tau2.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert list(hf)[:2] == [0, 0]
    a_h, w_h, ab_h = a.cpu().numpy(), w.cpu().numpy(), ab.cpu().numpy()
    amax = np.abs(a_h).max()
    eye = np.eye(n)
    # stage 1: nref = n - SB - 1 reflectors, unit entry SB rows below the diagonal (w_h[j, row] = A(row, j) after the reduction)
    q1 = _apply_q1_ref(n, sb, n - sb - 1, w_h, tau.cpu().numpy(), eye).astype(np.float64).T        # (row, column)
    band = np.zeros((n, n))
    for dd in range(sb + 1):                    # ab[d + j ldab] = B[j + d, j]
        band += np.diag(ab_h[:n - dd, dd], -dd)
    band = band + np.tril(band, -1).T
    e1 = np.abs(q1.T @ a_h @ q1 - band).max()
    print(f"n={n}: max|Q1' A Q1 - B| = {e1:.2e} max|A| = {amax:.2e}")
    assert e1 <= 1e-12 * amax
    # stage 2
    v2_h, tau2_h = v2.cpu().numpy(), tau2.cpu().numpy()
    for s in range(n):                          # zero where no step exists
        assert np.all(tau2_h[s, len(_steps_of_sweep(n, s)):] == 0.0), s
    q2 = _apply_q2_ref(n, v2_h, tau2_h, eye).astype(np.float64).T
    d_h, e_h = d.cpu().numpy(), e.cpu().numpy()[:n - 1]
    tri = np.diag(d_h) + np.diag(e_h, 1) + np.diag(e_h, -1)
    e2 = np.abs(q2.T @ band @ q2 - tri).max()
    print(f"n={n}: max|Q2' B Q2 - T| = {e2:.2e}")
    assert e2 <= 1e-12 * amax
    assert np.array_equal(q2[:, 0], eye[:, 0])
