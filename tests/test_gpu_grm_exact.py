"""GPU tests of the GRM kernels that are exact by construction (csrc/k_grm.hip, k_grm_i8.hip, k_grm_fp4.hip, k_grm_miss.hip;
`jxg_packed_dot` of k_gblup.hip) against a plain numpy restatement, bit for bit.

Everything is compared exactly, on DYADIC designs.  The value LUT is `stats.grm_lut_from_mean_scale(mean_g, scale, flip)` with
mean_g in {0, 1/8, .., 16/8}, scale in {1, 0.5} and any flip: every design value z is a multiple of 1/16 with |z| <= 2 (0 at a
missing call and at a padding sample), every product a multiple of 1/256 with |z z'| <= 4.  Hence Z Z' is representable in f64
whatever the order of summation; every f32 chunk sum of the fp16 split kernel is exact (8192 SNPs x 4 x 256 units = 2^23 < 2^24,
hi = half(z) exact, lo = 0); the i32 / f32 count sums, the affine terms r = C (b s) and B = sum b^2 (multiples of 1/8 and 1/64)
and the sparse correction's table values d (b + s c + d / 2) (multiples of 1/512) are exact too; f64 atomics of exact terms commute.
The device accumulator therefore has the bits of numpy's `Z.T @ Z`, and the tests use `np.array_equal` / `torch.equal`.  Each
reference also forms the Gram in int64 from rint(16 Z) and asserts that both agree: a design that is not dyadic fails there, loudly.

Rows classify by their LUT (grm_classify_kernel): scale 1 without a missing call among the selected samples -> flag 1 (clean int8
Gram); scale 1 with missing calls -> flag 2 (c* = 2 p, a multiple of 1/8 inside [0, 2]); scale 0.5 -> flag 0 (fp16 split kernel).
The exact prefix is (flag 1 + flag 2 rows) & ~63, the rest of them join the split kernel.

ONE form is not exact by construction: the dense missing-call form adds four scaled int8 Grams with the weights
(1 - 1/31 - 1/961, 1/31, 1/961, 1/961 - 1/31) / 3136.  With c* a multiple of 1/8 its digits are exact (P1 = 7 j, P2 = P3 = 0), all
quantisation noise vanishes and what is left is the digit algebra and the weights in f64: a few ulp per entry, bounded at
1e-12 max|K| (the bar of test_grm_count_gram_on_the_fp4_pipes for the same kind of sum), the diagonal included.

The accumulator is pre-filled with multiples of 1/4; every entry outside the lower tiles of the form under test must keep its
pre-fill.  Shapes: the smallest at which each path can go wrong -- n around a byte, a dword, the 128- and the 256-tile edge, odd
and even numbers of 128-tiles; row counts around the 64-row boundary of the exact prefix and the half BK = 128 step of the
256-tile kernels; one case at n = 9733, the smallest size at which the 256-tile forms are the natural dispatch."""
import functools

import numpy as np
import pytest
import torch

from janusx_amd import bed, pipeline, stats
from janusx_amd._lib import check, lib

pytestmark = pytest.mark.gpu

DENSE_TOL = 1e-12                 # of max|K_ref|: the dense missing-call form (see the module docstring), nothing else
SPARSE = {"JXGPU_GRM_MISS_MAX": "1", "JXGPU_GRM_MISS_DENSE_MIN": "1"}
DENSE = {"JXGPU_GRM_MISS_DENSE_MIN": "0", "JXGPU_GRM_MISS_DENSE_ROWS": "1"}
GRM_SWITCHES = ("JXGPU_GRM_I8_TILE", "JXGPU_GRM_FP4", "JXGPU_GRM_MISS", "JXGPU_GRM_MISS_MAX", "JXGPU_GRM_MISS_DENSE_MIN",
                "JXGPU_GRM_MISS_DENSE_ROWS", "JXGPU_GRM_MISS_DIGITS")


def _env(monkeypatch, settings):
    """exactly `settings` of the per-call GRM switches, every other one unset"""
    for k in GRM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in settings.items():
        assert k in GRM_SWITCHES
        monkeypatch.setenv(k, v)


# ---- designs and the numpy reference --------------------------------------------------------------------------------------------

def _codes(packed, n):
    """(m, ceil(n / 4)) PLINK payload -> (m, n) two-bit codes"""
    sh = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((packed[:, :, None] >> sh) & 3).reshape(packed.shape[0], -1)[:, :n]


def _design(n, kinds, seed, rate=0.0, lone=0):
    """Payload and LUT of len(kinds) rows over n samples.  kinds[r]: 1 = scale 1 without missing calls, 2 = scale 1 with missing
    calls at `rate` (at least one; exactly one in the first `lone` such rows; samples 0 and n - 1 BOTH missing in the next one),
    0 = scale 0.5 with missing calls at `rate`.  30 % of the rows are flipped.  The first and the last sample carry no zero count
    (1, 2, 1, .. and 2, 1, 2, ..): with n = 2, or in a row panel that holds one real sample, EVERY row then moves an entry, and a
    kernel that drops any single row is caught at those sizes too."""
    kinds = np.asarray(kinds, dtype=np.int64)
    m = len(kinds)
    rng = np.random.default_rng(seed)
    _, g = bed.synth_panel_numpy(n, m, seed=seed)
    g = g.copy()
    g[:, 0] = 1 + np.arange(m) % 2
    g[:, n - 1] = 2 - np.arange(m) % 2
    miss = (rng.random((m, n)) < rate) & (kinds != 1)[:, None]
    two = np.nonzero(kinds == 2)[0]
    for t, r in enumerate(two):
        if t < lone:
            miss[r] = False
        if not miss[r].any():
            miss[r, rng.integers(n)] = True
    if len(two) > lone:
        miss[two[lone], 0] = miss[two[lone], n - 1] = True
    g[miss] = -9
    mean_g = rng.integers(0, 17, size=m) / 8.0
    scale = np.where(kinds == 0, 0.5, 1.0)
    flip = rng.random(m) < 0.3
    return bed.pack_dosage(g), stats.grm_lut_from_mean_scale(mean_g, scale, flip)


def _mixed_kinds(m, seed, p=(0.25, 0.45, 0.30)):
    """flag-0, flag-1 and flag-2 rows interleaved at random"""
    return np.random.default_rng(seed).choice(3, size=m, p=p)


def _ref(codes, lut):
    """codes (mk, n) of the listed rows, lut (mk, 4) -> K = Z' Z in f64, checked against the int64 Gram of 16 Z"""
    z = np.take_along_axis(np.asarray(lut, dtype=np.float64), codes.astype(np.int64), axis=1)
    zi = np.rint(16.0 * z).astype(np.int64)
    assert np.array_equal(zi, 16.0 * z) and int(np.abs(zi).max()) <= 32, "the design is not dyadic"
    k = z.T @ z
    zt = np.ascontiguousarray(zi.T)                 # numpy's integer matmul is several times faster on contiguous rows
    assert np.array_equal(256.0 * k, zt @ zt.T), "the f64 reference is not exact"
    return k


def _n_exact(codes, lut):
    """rows of either affine kind / clean ones / missing calls of the affine rows, from the LUT and the codes of the listed rows"""
    affine = np.asarray(lut)[:, 2] - np.minimum(np.asarray(lut)[:, 0], np.asarray(lut)[:, 3]) == 1.0
    nmiss = (codes == 1).sum(axis=1)
    return int(affine.sum()), int((affine & (nmiss == 0)).sum()), int(nmiss[affine].sum())


def _share(n_rows_i8, mk):
    return np.float32((n_rows_i8 & ~63) / mk)


# ---- the device side ------------------------------------------------------------------------------------------------------------

def _prefill(row0, nrows, ld):
    """multiples of 1/4 that differ from entry to entry: rows [row0, row0 + nrows) of the (ld, ld) accumulator"""
    i = torch.arange(row0, row0 + nrows, device="cuda", dtype=torch.float64)[:, None]
    j = torch.arange(ld, device="cuda", dtype=torch.float64)[None, :]
    return ((7.0 * i + 3.0 * j) % 64.0) / 4.0 - 8.0


def _panel(packed, n, idx=None):
    return pipeline.Panel(torch.from_numpy(np.ascontiguousarray(packed)).cuda(), n, idx)


def _accumulate(p, rows, lut, acc, kchunk=0, precision=0, tiles=None):
    rows_t = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    lut_t = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    args = (p.p32.data_ptr(), p.m, p.n, None if rows_t is None else rows_t.data_ptr(), lut_t.data_ptr(), len(lut),
            acc.data_ptr(), int(kchunk), int(precision))
    if tiles is None:
        check(lib().jxg_grm_accumulate(*args, st))
    else:
        check(lib().jxg_grm_accumulate_rows(*args, int(tiles[0]), int(tiles[1]), st))
    torch.cuda.synchronize()
    return acc


def _compare(acc, acc0, k, n, tile, row0=0, tol=None):
    """acc, acc0: rows [row0, row0 + nr) of the accumulator after / before.  Lower triangle of the real samples == acc0 + K (bit for
    bit, or within tol max|K| where the form is the dense one); every entry outside the lower `tile` x `tile` tiles untouched."""
    a, a0 = acc.cpu().numpy(), acc0.cpu().numpy()
    nr, ld = a.shape
    i = row0 + np.arange(nr)[:, None]
    j = np.arange(ld)[None, :]
    outside = (i // tile) < (j // tile)
    assert np.array_equal(a[outside], a0[outside]), "an entry outside the lower tiles changed"
    real = max(0, min(n, row0 + nr) - row0)
    low = np.broadcast_to(j[:, :n] <= i[:real], (real, n))
    got, want = a[:real, :n][low], (a0[:real, :n] + k[row0:row0 + real, :n])[low]
    if tol is None:
        assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))
        return 0.0
    dev = float(np.abs(got - want).max()) / float(np.abs(k).max())
    print(f"dense form: max |acc - ref| / max|K| = {dev:.3e}")
    assert dev <= tol, dev
    diag = np.arange(row0, row0 + real)
    ddev = float(np.abs(a[diag - row0, diag] - a0[diag - row0, diag] - k[diag, diag]).max()) / float(np.abs(k).max())
    assert ddev <= tol, ddev
    return dev


def _run(p, rows, lut, k, tile, **kw):
    acc0 = _prefill(0, p.npad, p.npad)
    tol = kw.pop("tol", None)
    acc = _accumulate(p, rows, lut, acc0.clone(), **kw)
    return _compare(acc, acc0, k, p.n, tile, tol=tol)


# ---- 1. clean rows: both int8 tile shapes and the fp4 form -----------------------------------------------------------------------

CLEAN_FORMS = {"i8-128": ({"JXGPU_GRM_I8_TILE": "128"}, 128), "i8-256": ({"JXGPU_GRM_I8_TILE": "256"}, 256),
               "fp4-256": ({"JXGPU_GRM_I8_TILE": "256", "JXGPU_GRM_FP4": "1"}, 256)}
CLEAN_NS = [2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 385, 513, 641]
CLEAN_ES = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320]
# every n at E = 129 (prefix 128 + one row on the split kernel) and E = 192 (a half BK = 128 step, no remainder); every E at n = 256
# (whole tiles) and n = 301 (ragged: a partial byte, nt128 = 3, a trailing half 256-tile)
CLEAN_CASES = sorted({(n, e) for n in CLEAN_NS for e in (129, 192)} | {(n, e) for n in (256, 301) for e in CLEAN_ES})


@functools.lru_cache(maxsize=None)
def _clean_case(n, e):
    packed, lut = _design(n, np.ones(e, dtype=np.int64), seed=1000 * n + e)
    return packed, lut, _ref(_codes(packed, n), lut)


@pytest.mark.parametrize("form", list(CLEAN_FORMS))
@pytest.mark.parametrize("n,e", CLEAN_CASES)
def test_clean_rows(monkeypatch, n, e, form):
    """E clean affine rows: E & ~63 on grm_i8_kernel<128> / <256> / grm_nib_kernel + grm_fp4_kernel with the affine terms of
    jxg_packed_dot and grm_sumsq_kernel, E & 63 on grm_f16x2_kernel<128,128,64,64,false>."""
    packed, lut, k = _clean_case(n, e)
    env, tile = CLEAN_FORMS[form]
    _env(monkeypatch, env)
    _run(_panel(packed, n), np.arange(e), lut, k, tile)
    assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(e, e)


# ---- 2. row lists ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _list_case():
    n, m = 301, 500
    packed, lut = _design(n, _mixed_kinds(m, 21), seed=22, rate=0.003, lone=3)
    return n, packed, lut, _codes(packed, n)


ROW_LISTS = {"descending": np.arange(449, 149, -1), "strided": np.arange(1, 500, 3),
             "duplicate": np.concatenate([np.arange(30, 230), [117, 401, 117]]), "null": None}


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("which", list(ROW_LISTS))
def test_row_lists_and_mixed_rows(monkeypatch, which, tile):
    """A descending, a strided and a duplicated row list into a payload of more rows than are listed, and rows = NULL: flag-1, flag-2
    and flag-0 rows interleaved at random, so the stable partition (classify / partition / gather) must keep every row's LUT, beta
    and correction table with its payload.  Few missing calls: the flag-2 rows take the sparse correction (the default dispatch)."""
    n, packed, lut_all, codes = _list_case()
    rows = ROW_LISTS[which]
    sel = np.arange(len(packed)) if rows is None else rows
    k = _ref(codes[sel], lut_all[sel])
    _env(monkeypatch, {"JXGPU_GRM_I8_TILE": str(tile)})
    _run(_panel(packed, n), rows, lut_all[sel], k, tile)
    n_aff, n_clean, n_miss = _n_exact(codes[sel], lut_all[sel])
    assert 0 < n_miss <= 0.012 * len(sel) * n and n_clean >= 64 and n_aff - n_clean >= 32 and n_aff < len(sel)
    assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(n_aff, len(sel))


# ---- 3. SNP-chunked launches -----------------------------------------------------------------------------------------------------

def test_int8_gram_chunks_over_grid_y(monkeypatch):
    """Few tiles and more than 4096 rows: n = 301, E = 4160 -> chunks of 2048, 2048 and 64 rows over blockIdx.y, f64 atomics; the
    affine terms ride on the first chunk only."""
    n, e = 301, 4160
    packed, lut = _design(n, np.ones(e, dtype=np.int64), seed=31)
    _env(monkeypatch, {})
    _run(_panel(packed, n), np.arange(e), lut, _ref(_codes(packed, n), lut), 128)
    assert np.float32(lib().jxg_last_kernel_ms(12)) == np.float32(1.0)


def test_split_kernel_chunks_over_grid_y(monkeypatch):
    """2112 general rows, few tiles: grm_f16x2_kernel<128,128,64,64,false> in atomic mode (chunks of 1024, 1024 and 64 rows)."""
    n, m = 301, 2112
    packed, lut = _design(n, np.zeros(m, dtype=np.int64), seed=32, rate=0.01)
    _env(monkeypatch, {})
    _run(_panel(packed, n), np.arange(m), lut, _ref(_codes(packed, n), lut), 128)
    assert lib().jxg_last_kernel_ms(12) == 0.0


def test_plain_launches_and_several_calls_into_one_accumulator(monkeypatch):
    """kchunk = 512 and at most 2048 rows per call: one plain read-modify-write launch of the split kernel per 512 rows, one of the
    int8 kernel; three calls into one accumulator, the affine terms added once per call."""
    n, per = 301, 1100
    kinds = np.concatenate([np.random.default_rng(33 + c).permutation(np.repeat([1, 0], [500, 600])) for c in range(3)])
    packed, lut = _design(n, kinds, seed=34, rate=0.01)
    k = _ref(_codes(packed, n), lut)
    _env(monkeypatch, {})
    p = _panel(packed, n)
    acc0 = _prefill(0, p.npad, p.npad)
    acc = acc0.clone()
    for c in range(3):
        rows = np.arange(c * per, (c + 1) * per)
        _accumulate(p, rows, lut[rows], acc, kchunk=512)
        assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(500, per)
    _compare(acc, acc0, k, n, 128)


# ---- 4. missing calls ------------------------------------------------------------------------------------------------------------

MISS_FORMS = {
    # name: (switches, precision, tile of the int8 kernels, rows on the int8 path: "all" affine ones / "clean" only / by the rate)
    "default": ({}, 0, 128, "rate"),
    "sparse": (SPARSE, 0, 128, "all"),
    "sparse-256": ({**SPARSE, "JXGPU_GRM_I8_TILE": "256"}, 0, 256, "all"),
    "general": ({"JXGPU_GRM_MISS": "0"}, 0, 128, "clean"),
    "precision2": ({}, 2, 128, "clean"),
    "dense3-128": ({**DENSE, "JXGPU_GRM_I8_TILE": "128"}, 0, 128, "all"),
    "dense3-256": ({**DENSE, "JXGPU_GRM_I8_TILE": "256"}, 0, 256, "all"),
    "dense2-128": ({**DENSE, "JXGPU_GRM_I8_TILE": "128", "JXGPU_GRM_MISS_DIGITS": "2"}, 0, 128, "all"),
    "dense2-256": ({**DENSE, "JXGPU_GRM_I8_TILE": "256", "JXGPU_GRM_MISS_DIGITS": "2"}, 0, 256, "all"),
}
# n = 130: the payload's padding samples carry the missing code; 257 / 641: nt128 = 3 / 6, the 256-tile byte-LUT kernel with and
# without a trailing half tile.  clean = False: no flag-1 row at all (the affine terms ride on the first byte-LUT launch)
MISS_CASES = [(130, 0.03, True), (130, 0.003, True), (257, 0.03, True), (641, 0.003, True), (641, 0.03, False), (257, 0.003, False)]


@functools.lru_cache(maxsize=None)
def _miss_case(n, rate, clean):
    kinds = np.repeat([1, 2, 0], [150, 170, 40] if clean else [0, 320, 40])
    kinds = np.random.default_rng(41).permutation(kinds)
    packed, lut = _design(n, kinds, seed=42 + n, rate=rate, lone=5)
    codes = _codes(packed, n)
    return packed, lut, codes, _ref(codes, lut)


@pytest.mark.parametrize("form", list(MISS_FORMS))
@pytest.mark.parametrize("n,rate,clean", MISS_CASES)
def test_rows_with_missing_calls(monkeypatch, n, rate, clean, form):
    """Rows with missing calls (a few with one missing sample alone, one with both samples of a pair missing) beside clean and general
    rows: the default dispatch, the sparse correction (gm_lists / gm_scan / gm_spmm / gm_merge), the split kernel (JXGPU_GRM_MISS=0,
    precision = 2: grm_demote_kernel) -- all bit for bit -- and the dense form (grm_i8_kernel<.., LUT = true> in both tile shapes,
    grm_elut_kernel, grm_diag_add_kernel) with three and two digits at DENSE_TOL."""
    packed, lut, codes, k = _miss_case(n, rate, clean)
    env, precision, tile, on_i8 = MISS_FORMS[form]
    _env(monkeypatch, env)
    dense = form.startswith("dense")
    # largest value seen on the MI355X over all cases: 2.1e-16, with three and with two digits (the second and third digits are 0)
    _run(_panel(packed, n), np.arange(len(lut)), lut, k, tile, precision=precision, tol=DENSE_TOL if dense else None)
    n_aff, n_clean, n_miss = _n_exact(codes, lut)
    assert n_clean == (150 if clean else 0) and n_aff == 320 and n_miss >= 170
    if on_i8 == "rate":                        # the documented rule of the default: sparse correction up to 1.2 % missing calls
        on_i8 = "all" if n_miss <= 0.012 * len(lut) * n else "clean"
        assert on_i8 == ("all" if rate < 0.01 else "clean")
    # padding samples (code 01 in the P32 image) must not flag a row: every clean row stays on the int8 path in every form
    assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(n_aff if on_i8 == "all" else n_clean, len(lut))


# ---- 5. row panels ---------------------------------------------------------------------------------------------------------------

PANELS = [(641, 0, 2), (641, 2, 6), (641, 2, 4), (641, 1, 3), (641, 3, 6), (641, 5, 6), (513, 4, 5), (513, 2, 5)]


@functools.lru_cache(maxsize=None)
def _panel_case(n):
    packed, lut = _design(n, _mixed_kinds(330, 51, p=(0.15, 0.65, 0.20)), seed=52 + n, rate=0.003, lone=2)
    codes = _codes(packed, n)
    return packed, lut, codes, _ref(codes, lut)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("tile_env", ["256", None])
@pytest.mark.parametrize("n,t0,t1", PANELS)
def test_row_panels(monkeypatch, n, t0, t1, tile_env, precision):
    """jxg_grm_accumulate_rows on a panel buffer of (t1 - t0) 128 rows whose row 0 is sample row 128 t0: even starts take 256-tiles
    when asked to (also with t1 == nt128 odd: a trailing half tile), odd starts fall back to 128-tiles; rows with missing calls go
    to the split kernel in panel mode."""
    packed, lut, codes, k = _panel_case(n)
    _env(monkeypatch, {} if tile_env is None else {"JXGPU_GRM_I8_TILE": tile_env})
    p = _panel(packed, n)
    big = tile_env == "256" and t0 % 2 == 0 and (t1 % 2 == 0 or t1 == p.nt)
    acc0 = _prefill(128 * t0, 128 * (t1 - t0), p.npad)
    acc = _accumulate(p, np.arange(len(lut)), lut, acc0.clone(), precision=precision, tiles=(t0, t1))
    _compare(acc, acc0, k, n, 256 if big else 128, row0=128 * t0)
    assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(_n_exact(codes, lut)[1], len(lut))


def test_row_panel_out_of_range_is_refused(monkeypatch):
    packed, lut, _, _ = _panel_case(513)
    _env(monkeypatch, {})
    p = _panel(packed, 513)
    for t0, t1 in ((0, p.nt + 1), (-1, 2), (3, 3)):
        acc0 = _prefill(0, p.npad, p.npad)
        acc = acc0.clone()
        with pytest.raises(RuntimeError, match="jxg_grm_accumulate_rows: tile row range out of bounds"):
            _accumulate(p, np.arange(len(lut)), lut, acc, tiles=(t0, t1))
        torch.cuda.synchronize()
        assert torch.equal(acc, acc0)


# ---- 6. natural dispatch of the 256-tile forms -----------------------------------------------------------------------------------

def test_natural_dispatch_of_the_256_tile_forms(monkeypatch):
    """n = 9733: nt128 = 77, 780 tiles of 256 with a trailing half tile -- the smallest size at which launch_grm_i8 and
    launch_grm_i8_lut take the 256-tile kernels on their own.  m = 256 clean rows and rows with missing calls.  With nothing set the
    rows with missing calls take the sparse correction: bit for bit.  With the dense-form switches (and nothing else) they take
    grm_i8_kernel<256, .., LUT = true>, the one form that is not exact by construction: DENSE_TOL.  The reference is formed on the
    device: torch's f64 matmul of the decoded Z is exact for the same reason as numpy's, and an int64 Gram of 16 Z checks it."""
    n, m = 9733, 256
    packed, lut = _design(n, np.random.default_rng(61).permutation(np.repeat([1, 2], [140, 116])), seed=62, rate=0.003, lone=3)
    dev = torch.device("cuda")
    pt = torch.from_numpy(packed).to(dev)
    sh = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)
    codes = ((pt[:, :, None] >> sh) & 3).reshape(m, -1)[:, :n].to(torch.int64)
    z = torch.gather(torch.from_numpy(lut.astype(np.float64)).to(dev), 1, codes)
    zi = torch.round(16.0 * z).to(torch.int64)
    assert torch.equal(zi.to(torch.float64), 16.0 * z) and int(zi.abs().max()) <= 32
    k = z.T @ z
    ki = torch.zeros((n, n), dtype=torch.int64, device=dev)
    for r in range(m):
        ki += zi[r][:, None] * zi[r][None, :]
    assert torch.equal(256.0 * k, ki.to(torch.float64)), "the f64 reference is not exact"
    del ki, z, zi
    n_miss = int((codes == 1).sum())
    assert 0 < n_miss <= 0.012 * m * n
    del codes
    low = torch.tril(torch.ones((n, n), dtype=torch.bool, device=dev))
    p = pipeline.Panel(pt, n)
    ti = torch.arange(p.npad, device=dev) // 256
    outside = ti[:, None] < ti[None, :]
    kmax = float(k.abs().max())
    for env in ({}, DENSE):
        _env(monkeypatch, env)
        acc0 = _prefill(0, p.npad, p.npad)
        acc = _accumulate(p, np.arange(m), lut, acc0.clone())
        assert np.float32(lib().jxg_last_kernel_ms(12)) == np.float32(1.0)
        assert torch.equal(acc[outside], acc0[outside]), "an entry outside the lower 256-tiles changed"
        got = acc[:n, :n] - acc0[:n, :n]               # exact: multiples of 1/4 taken off multiples of 1/256 (dense: a few ulp)
        if not env:
            assert torch.equal(got[low], k[low])
        else:
            dev_max = float((got - k)[low].abs().max()) / kmax
            print(f"dense form, 256-tiles: max |acc - ref| / max|K| = {dev_max:.3e}")
            assert dev_max <= DENSE_TOL, dev_max          # largest value seen on the MI355X: 1.8e-16
        del acc, acc0, got


# ---- 7. a sample subset and junk pad bits ----------------------------------------------------------------------------------------

def test_sample_subset(monkeypatch):
    """Panel(pt, n, idx) with an unsorted list of 201 of 333 samples: the reference decodes the same samples in the same order."""
    n_src, m = 333, 300
    idx = np.random.default_rng(71).permutation(n_src)[:201]
    assert not np.array_equal(idx, np.sort(idx))
    packed, lut = _design(n_src, _mixed_kinds(m, 72), seed=73, rate=0.003, lone=2)
    codes = _codes(packed, n_src)[:, idx]
    _env(monkeypatch, {})
    p = _panel(packed, n_src, idx)
    assert p.n == 201
    _run(p, np.arange(m), lut, _ref(codes, lut), 128)
    assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(_n_exact(codes, lut)[0], m)


@pytest.mark.parametrize("n", [130, 301])
def test_junk_pad_bits_of_the_payload(monkeypatch, n):
    """The unused bits of the last byte of every SNP (n % 4 != 0) set to 11: the same acc[:n, :n] as with the clean payload."""
    m = 200
    packed, lut = _design(n, _mixed_kinds(m, 74), seed=75 + n, rate=0.003, lone=2)
    junk = packed.copy()
    junk[:, -1] |= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)
    assert np.array_equal(_codes(junk, n), _codes(packed, n)) and not np.array_equal(junk, packed)
    codes = _codes(packed, n)
    k = _ref(codes, lut)
    _env(monkeypatch, {})
    outs = []
    for pay in (packed, junk):
        p = _panel(pay, n)
        acc0 = _prefill(0, p.npad, p.npad)
        acc = _accumulate(p, np.arange(m), lut, acc0.clone())
        _compare(acc, acc0, k, n, 128)
        assert np.float32(lib().jxg_last_kernel_ms(12)) == _share(_n_exact(codes, lut)[0], m)
        outs.append(acc[:n, :n].clone())
    assert torch.equal(outs[0], outs[1])


# ---- 8. jxg_grm_finalize ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [129, 257])
def test_finalize_is_exact(n):
    """inv_scale = 2^-7: K == acc 2^-7 exactly on the lower triangle, mirrored bit for bit; the f32 output is the rounded f64 one.
    The upper triangle of the accumulator holds other numbers: nothing of it may reach K."""
    npad = lib().jxg_num_tiles(n) * 128
    rng = np.random.default_rng(81 + n)
    a = rng.integers(-2 ** 30, 2 ** 30, size=(npad, npad)).astype(np.float64) / 256.0
    acc = torch.from_numpy(a).cuda()
    want = np.tril(a[:n, :n]) * 2.0 ** -7
    want = want + np.tril(want, -1).T
    k64 = pipeline.grm_finalize(acc, n, 2.0 ** 7, dtype=torch.float64).cpu().numpy()
    k32 = pipeline.grm_finalize(acc, n, 2.0 ** 7, dtype=torch.float32).cpu().numpy()
    assert np.array_equal(k64, want) and np.array_equal(k64, k64.T)
    assert k32.dtype == np.float32 and np.array_equal(k32, want.astype(np.float32)) and np.array_equal(k32, k32.T)
