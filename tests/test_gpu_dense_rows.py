"""The dense-chunk mirrors on the dense-row stage of `pipeline` (`DenseRowsRotation`, `scan_dense_rows`, `scan_rows_lm_dense`):
their tables, bit for bit, against a restatement of what these entry points did before they were routed through the stage --
per block of 4096 rows an upload, `jxg_rotate_dense_f32` where there is a U^T, then ONE scan call -- written out below with
`jxg_*` calls on torch tensors.  n = 131 samples (two 128-column tiles of the f32 rotation, the last one 3 wide; odd row strides),
m = 4096 + 37 rows, so the 4096-row block seam is crossed: row 5 is all zero (the invalid row), rows 4095 and 4096 hold the same
values, one on each side of the seam.  Three covariate columns, and seven (the p + 1 > 4 form of the tables) for the exact and the
fixed-lambda scan.  The null-model helpers are compared with a direct launch of their `jxg_*` function."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from janusx_amd import janusx as jx  # noqa: E402

N, M, BLOCK = 131, 4096 + 37, 4096
LOW, HIGH, MAX_ITER, TOL, L10 = -5.0, 5.0, 50, 1e-2, 0.3
SEAM = ((0, BLOCK), (BLOCK, M))


class _Case:
    pass


@pytest.fixture(scope="module")
def case():
    """Synthetic eigenbasis (QR of a seeded normal matrix, seeded positive spectrum): no eigendecomposition needed."""
    import torch
    c = _Case()
    c.dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rng = np.random.default_rng(131)
    u = np.linalg.qr(rng.standard_normal((N, N)))[0]
    c.ut = np.ascontiguousarray(u.T, dtype=np.float32)
    c.s = np.sort(rng.gamma(2.0, 0.5, N)) + 1e-3
    c.y_raw = u @ (np.sqrt(c.s) * rng.standard_normal(N)) + rng.standard_normal(N)
    c.x_raw = {p: np.concatenate([np.ones((N, 1)), rng.standard_normal((N, p - 1))], axis=1) for p in (3, 7)}
    ut64 = c.ut.astype(np.float64)
    c.y = ut64 @ c.y_raw
    c.x = {p: np.ascontiguousarray(ut64 @ x) for p, x in c.x_raw.items()}
    g = rng.binomial(2, rng.uniform(0.05, 0.5, size=(M, 1)), size=(M, N)).astype(np.float32)
    g -= g.mean(axis=1, keepdims=True)
    g[5] = 0.0
    g[BLOCK] = g[BLOCK - 1]
    c.g = np.ascontiguousarray(g)
    c.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(c.dev)       # noqa: E731
    c.d_s, c.d_y, c.d_ut = c.t(c.s), c.t(c.y), c.t(c.ut)
    c.d_x = {p: c.t(x) for p, x in c.x.items()}
    c.nullml = _direct_loglike(c, 3, L10)[0]
    return c


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _direct_loglike(c, p, log10_lbd):
    import torch
    from janusx_amd._lib import check, lib
    o = torch.empty(2, dtype=torch.float64, device=c.dev)
    check(lib().jxg_lmm_loglike_null(c.d_s.data_ptr(), c.d_x[p].data_ptr(), c.d_y.data_ptr(), N, p, log10_lbd, o.data_ptr(),
                                     _stream()))
    return [float(v) for v in o.cpu().numpy()]


def _restated(c, g, rotate, scan, cols, blocks):
    """What the parent's host-pointer entry points did: per block an upload, the f32 rotation where asked, one scan call."""
    import torch
    from janusx_amd._lib import check, lib
    out = torch.empty((len(g), cols), dtype=torch.float64, device=c.dev)
    for r0, r1 in blocks:
        gb = c.t(g[r0:r1])
        if rotate:
            rot = torch.empty_like(gb)
            check(lib().jxg_rotate_dense_f32(gb.data_ptr(), r1 - r0, N, c.d_ut.data_ptr(), rot.data_ptr(), _stream()))
            gb = rot
        scan(gb, r1 - r0, out[r0:])
    return out.cpu().numpy()


def _null_ptrs(c, p):
    return c.d_s.data_ptr(), c.d_x[p].data_ptr(), c.d_y.data_ptr()


def _lmm_scan(c, p, nullml, low=LOW, high=HIGH, fn="jxg_lmm_scan"):
    from janusx_amd._lib import check, lib
    s_p, x_p, y_p = _null_ptrs(c, p)

    def scan(gb, nr, out):
        check(getattr(lib(), fn)(gb.data_ptr(), nr, N, s_p, x_p, y_p, p, low, high, TOL, MAX_ITER, 0, 0.0,
                                 0 if nullml is None else 1, 0.0 if nullml is None else nullml, out.data_ptr(), None, _stream()))
    return scan


def _lmm2_scan(c, p, nullml):
    from janusx_amd._lib import check, lib
    s_p, x_p, y_p = _null_ptrs(c, p)

    def scan(gb, nr, out):
        check(lib().jxg_lmm2_scan(gb.data_ptr(), nr, N, s_p, x_p, y_p, p, LOW, HIGH, TOL, MAX_ITER, 0, 0.0, nullml, out.data_ptr(),
                                  _stream()))
    return scan


def _fv_state(c, p):
    """`jxg_fvlmm_prepare` at 10^L10 -> (w, py, wx on the device, chol(X'WX) on the host, (yPy, log det V, df))."""
    import torch
    from janusx_amd._lib import check, lib
    w, py = (torch.empty(N, dtype=torch.float32, device=c.dev) for _ in range(2))
    wx = torch.empty((N, p), dtype=torch.float32, device=c.dev)
    a, sc = np.zeros((p, p)), np.zeros(3)
    torch.cuda.synchronize()
    check(lib().jxg_fvlmm_prepare(*_null_ptrs(c, p), N, p, 10.0 ** L10, w.data_ptr(), py.data_ptr(), wx.data_ptr(), a.ctypes.data,
                                  sc.ctypes.data))
    return w, py, wx, a, sc


def _fv_scan(c, p, nullml):
    from janusx_amd._lib import check, lib
    w, py, wx, a, sc = _fv_state(c, p)
    d_a = c.t(a)

    def scan(gb, nr, out):
        check(lib().jxg_fvlmm_scan_dev(gb.data_ptr(), nr, N, p, w.data_ptr(), py.data_ptr(), wx.data_ptr(), d_a.data_ptr(),
                                       float(sc[0]), int(sc[2]), 0 if nullml is None else 1, 0.0 if nullml is None else nullml,
                                       float(sc[1]), out.data_ptr(), _stream()))
    return scan


def _lm_scan(c, p):
    import torch
    from janusx_amd._lib import check, lib
    x, y = c.x_raw[p], np.ascontiguousarray(c.y_raw)
    ixx = np.linalg.inv(x.T @ x)
    xr, yy = np.empty((N, p + 1)), np.zeros(1)
    check(lib().jx_lm_residualize(y.ctypes.data, x.ctypes.data, ixx.ctypes.data, N, p, xr.ctypes.data, yy.ctypes.data))
    d_xr, d_ixx = c.t(xr), c.t(ixx)

    def scan(gb, nr, out):
        work = torch.empty(nr * (p + 2), dtype=torch.float64, device=c.dev)
        check(lib().jxg_lm_scan_dense(gb.data_ptr(), nr, N, N, d_xr.data_ptr(), p, d_ixx.data_ptr(), float(yy[0]), work.data_ptr(),
                                      out.data_ptr(), _stream()))
    return scan, ixx


def _zero_plrt_of_nan_rows(t):
    t = t.copy()
    t[np.isnan(t[:, 2]), 3] = 0.0
    return t


# name -> (mirror call, (rotate, scan, columns) of its restatement, what the mirror does to the table behind it), each by p
def _mirrors(c):
    null = lambda p: (c.s, c.x[p], c.y)       # noqa: E731
    same = lambda t: t                        # noqa: E731
    nm = c.nullml
    return {
        "lmm_reml_chunk_f32": (lambda p: jx.lmm_reml_chunk_f32(*null(p), LOW, HIGH, c.g, MAX_ITER, TOL),
                               lambda p: (False, _lmm_scan(c, p, None), 3), same),
        "lmm_reml_chunk_f32+nullml": (lambda p: jx.lmm_reml_chunk_f32(*null(p), LOW, HIGH, c.g, MAX_ITER, TOL, nullml=nm),
                                      lambda p: (False, _lmm_scan(c, p, nm), 4), same),
        "lmm_reml_chunk_from_snp_f32": (lambda p: jx.lmm_reml_chunk_from_snp_f32(*null(p), LOW, HIGH, c.g, c.ut, MAX_ITER, TOL),
                                        lambda p: (True, _lmm_scan(c, p, None), 3), same),
        "lmm_reml_lmm2_chunk_from_snp_f32": (lambda p: jx.lmm_reml_lmm2_chunk_from_snp_f32(*null(p), LOW, HIGH, c.g, c.ut, nm,
                                                                                                 MAX_ITER, TOL),
                                             lambda p: (True, _lmm2_scan(c, p, nm), 6), same),
        "fvlmm_assoc_chunk_f32": (lambda p: jx.fvlmm_assoc_chunk_f32(*null(p), L10, c.g),
                                  lambda p: (False, _fv_scan(c, p, None), 3), same),
        "fvlmm_assoc_chunk_f32+nullml": (lambda p: jx.fvlmm_assoc_chunk_f32(*null(p), L10, c.g, nullml=nm),
                                         lambda p: (False, _fv_scan(c, p, nm), 4), same),
        "fvlmm_assoc_chunk_from_snp_f32": (lambda p: jx.fvlmm_assoc_chunk_from_snp_f32(*null(p), L10, c.g, c.ut),
                                           lambda p: (True, _fv_scan(c, p, None), 3), same),
        "lmm_assoc_chunk_f32+nullml": (lambda p: jx.lmm_assoc_chunk_f32(*null(p), L10, c.g, nullml=nm),
                                       lambda p: (False, _fv_scan(c, p, nm), 4), _zero_plrt_of_nan_rows),
        "fvlmm_assoc_chunk_with_cache_f32+nullml": (
            lambda p: jx.fvlmm_assoc_chunk_with_cache_f32(jx.fvlmm_assoc_prepare_cache_f32(*null(p), L10), c.g, nullml=nm),
            lambda p: (False, _fv_scan(c, p, nm), 4), same),
    }


MIRRORS = [(name, p) for name, ps in (
    ("lmm_reml_chunk_f32", (3, 7)), ("lmm_reml_chunk_f32+nullml", (3,)), ("lmm_reml_chunk_from_snp_f32", (3, 7)),
    ("lmm_reml_lmm2_chunk_from_snp_f32", (3,)), ("fvlmm_assoc_chunk_f32", (3, 7)), ("fvlmm_assoc_chunk_f32+nullml", (3,)),
    ("fvlmm_assoc_chunk_from_snp_f32", (3, 7)), ("lmm_assoc_chunk_f32+nullml", (3,)),
    ("fvlmm_assoc_chunk_with_cache_f32+nullml", (3,))) for p in ps]


@pytest.mark.parametrize("name,p", MIRRORS, ids=[f"{n}-p{p}" for n, p in MIRRORS])
def test_mirror_equals_the_per_block_restatement_across_the_seam(case, name, p):
    """The mirror's bytes are those of the per-block launches over [0, 4096) and [4096, 4133); the same table comes from ONE
    launch over all 4133 rows (the scans run one wave per SNP and the f32 rotation walks the full k for every output element
    whatever the row tile: blocking does not reach the bits)."""
    mirror, restatement, behind = _mirrors(case)[name]
    got = mirror(p)
    rotate, scan, cols = restatement(p)
    want = behind(_restated(case, case.g, rotate, scan, cols, SEAM))
    assert got.dtype == np.float64 and got.shape == (M, cols)
    assert got.tobytes() == want.tobytes()
    assert got[BLOCK - 1].tobytes() == got[BLOCK].tobytes()             # the witnesses on either side of the seam
    assert np.isnan(got[5, 0]) and np.isfinite(got[[4, 6], :3]).all()   # the all-zero row is the invalid one
    one = behind(_restated(case, case.g, rotate, scan, cols, ((0, M),)))
    assert one.tobytes() == want.tobytes()


def test_lm_block_assoc_across_the_seam(case):
    """`lm_block_assoc_f32` runs one block by default; the seam is reached through the pipeline function with block_rows = 4096."""
    from janusx_amd import pipeline
    scan, ixx = _lm_scan(case, 3)
    want = _restated(case, case.g, False, scan, 4, SEAM)
    got = jx.lm_block_assoc_f32(case.y_raw, case.x_raw[3], ixx, case.g)
    seamed = pipeline.scan_rows_lm_dense(case.g, case.x_raw[3], np.ascontiguousarray(case.y_raw), ixx, block_rows=BLOCK)
    assert got.dtype == np.float64 and got.shape == (M, 4) and np.isfinite(got[[4, 6]]).all()
    assert seamed.cpu().numpy().tobytes() == want.tobytes() == got.tobytes()
    assert got[BLOCK - 1].tobytes() == got[BLOCK].tobytes()
    assert _restated(case, case.g, False, scan, 4, ((0, M),)).tobytes() == want.tobytes()


@pytest.mark.parametrize("low,tabulated", [(-8.0, True), (-8.5, False)])
def test_wide_brent_bounds(case, low, tabulated):
    """The tables serve high - low <= 16 (CH_MAXSEG = 8 segments of width 2): [-8, 8] is the widest interval they take and the
    mirror's bytes are those of `jxg_lmm_scan`; [-8.5, 8] is wider, `jxg_lmm_tables_bytes` is 0 there and the mirror's bytes are
    those of a direct `jxg_lmm_scan_exact` launch."""
    from janusx_amd._lib import lib
    assert (int(lib().jxg_lmm_tables_bytes(N, 3, low, 8.0)) > 0) == tabulated
    g = case.g[:300]
    got = jx.lmm_reml_chunk_f32(case.s, case.x[3], case.y, low, 8.0, g, MAX_ITER, TOL)
    fn = "jxg_lmm_scan" if tabulated else "jxg_lmm_scan_exact"
    want = _restated(case, g, False, _lmm_scan(case, 3, None, low, 8.0, fn), 3, ((0, 300),))
    assert got.tobytes() == want.tobytes() and np.isfinite(got[[4, 6]]).all() and np.isnan(got[5, 0])


def test_block_diagonal_parts_do_not_depend_on_the_blocking(case):
    """`scan_rows_splmm_dense` over two diagonal blocks (64 + 67 samples, each with a permuted sample list): 300 rows in blocks
    of 128 (two full ones and a remainder) give the bytes of one block."""
    from janusx_amd import pipeline
    rng = np.random.default_rng(67)
    perm = rng.permutation(N)
    parts = []
    for off, nb in ((0, 64), (64, 67)):
        ub = np.linalg.qr(rng.standard_normal((nb, nb)))[0]
        parts.append((off, nb, case.t(ub.T.astype(np.float32)), case.t(perm[off:off + nb].astype(np.int64))))
    w, py, wx, a, sc = _fv_state(case, 3)
    fv_state = (w, py, wx, a, float(sc[0]))
    g = case.g[:300]
    one = pipeline.scan_rows_splmm_dense(g, parts, N, 3, fv_state, case.dev, block_rows=300).cpu().numpy()
    cut = pipeline.scan_rows_splmm_dense(g, parts, N, 3, fv_state, case.dev, block_rows=128).cpu().numpy()
    assert one.shape == (300, 3) and np.isfinite(one[[4, 6]]).all() and np.isnan(one[5, 0])
    assert cut.tobytes() == one.tobytes()


def test_null_model_helpers_equal_their_direct_launch(case, monkeypatch):
    import torch
    from janusx_amd._lib import check, lib
    s_p, x_p, y_p = _null_ptrs(case, 3)
    null = (case.s, case.x[3], case.y)
    o3 = torch.empty(3, dtype=torch.float64, device=case.dev)
    check(lib().jxg_lmm_reml_null(s_p, x_p, y_p, N, 3, LOW, HIGH, 50, 1e-3, o3.data_ptr(), _stream()))
    got = jx.lmm_reml_null_f32(*null, LOW, HIGH, 50, 1e-3)
    assert isinstance(got, tuple) and np.array(got).tobytes() == o3.cpu().numpy().tobytes()
    ml = jx.ml_loglike_null_f32(*null, L10)
    assert type(ml) is float and np.float64(ml).tobytes() == np.float64(_direct_loglike(case, 3, L10)[0]).tobytes()
    assert np.array(jx._loglike_null(*null, L10)).tobytes() == np.array(_direct_loglike(case, 3, L10)).tobytes()
    # the null ML that `lmm_reml_lmm2_assoc_bed_to_tsv_f32` fits when it is handed none: what it passes on to its scan
    o2 = torch.empty(2, dtype=torch.float64, device=case.dev)
    check(lib().jxg_lmm2_null_ml(s_p, x_p, y_p, N, 3, -4.0, 3.0, 30, 1e-2, 1, 0.5, o2.data_ptr(), _stream()))
    monkeypatch.setattr(jx, "_bed_scan_to_tsv", lambda *a, **kw: a[17])
    fitted = jx.lmm_reml_lmm2_assoc_bed_to_tsv_f32("<unused>", "<unused>", *null, case.ut, 0.02, 0.05, 1.0, low=-4.0, high=3.0,
                                                   max_iter=30, tol=1e-2, init_log10_lbd_ml=0.5)
    assert type(fitted) is float and np.float64(fitted).tobytes() == o2.cpu().numpy()[1].tobytes()


def test_design_rotation_equals_its_direct_launch(case):
    import torch
    from janusx_amd._lib import check, lib

    def direct(cols):
        d_in = case.t(cols)
        d_out = torch.empty_like(d_in)
        check(lib().jxg_rotate_xy(case.d_ut.data_ptr(), N, d_in.data_ptr(), cols.shape[1], d_out.data_ptr(), _stream()))
        return d_out.cpu().numpy()

    x, y = case.x_raw[3], case.y_raw
    want = direct(np.concatenate([x, y[:, None]], axis=1))
    ox, oy = jx.lmm_rotate_x_y_with_ut_f64(case.ut, x, y)
    assert ox.shape == (N, 3) and oy.shape == (N, 1) and ox.dtype == oy.dtype == np.float64
    assert ox.tobytes() == np.ascontiguousarray(want[:, :3]).tobytes() and oy.tobytes() == np.ascontiguousarray(want[:, 3:]).tobytes()
    y_only = jx.lmm_rotate_y_with_ut_f64(case.ut, y)                    # rotated beside one zero column
    want_y = direct(np.concatenate([np.zeros((N, 1)), y[:, None]], axis=1))[:, 1]
    assert y_only.shape == (N,) and y_only.tobytes() == np.ascontiguousarray(want_y).tobytes()


def test_plain_eigh_equals_the_three_composed_calls(case):
    """n = 40 is on the rocSOLVER side of the 256 switch; the matrix is not symmetric to the last bit, so the symmetrisation
    counts."""
    import torch
    from janusx_amd._lib import check, lib
    n = 40
    rng = np.random.default_rng(40)
    b = rng.standard_normal((n, n))
    a = b @ b.T / n + 1e-9 * rng.standard_normal((n, n))
    d_a = case.t(a.copy())
    d_w = torch.empty(n, dtype=torch.float64, device=case.dev)
    d_u = torch.empty_like(d_a)
    check(lib().jxg_symmetrize_f64(d_a.data_ptr(), n, _stream()))
    check(lib().jxg_eigh_f64(d_a.data_ptr(), n, 1e-6, d_w.data_ptr(), _stream()))
    check(lib().jxg_transpose_f64(d_a.data_ptr(), d_u.data_ptr(), n, _stream()))
    res = jx.rust_eigh_from_array_f64(a, diag_shift=1e-6)
    assert res[0].tobytes() == d_w.cpu().numpy().tobytes() and res[1].tobytes() == d_u.cpu().numpy().tobytes()
    assert res[3] == "rocsolver_dsyevd" and res[4] == n and np.all(np.diff(res[0]) >= 0)
    values_only = jx.rust_eigh_from_array_f64(a, jobz="N", diag_shift=1e-6)
    assert values_only[1] is None and values_only[0].tobytes() == res[0].tobytes()
