"""The two MFMA shapes of the DMA form of the int8 rotation (csrc/k_rotate_i8.hip, `rotate_i8_dma_kernel<MODE, SHAPE>`:
JXGPU_ROT_I8_MFMA = 16 | 32, read per call) inside one process through the C-ABI entries, at the smallest sizes the kernel takes.

Both shapes sum the same exact i32 plane sums and share one epilogue expression, so they are compared byte for byte; both are also
compared with a numpy reference built from the planes `jxg_ut_quant3` returned: exact integer sums `c . q_p` of the counts decoded
from the packed rows on the host, the f64 combination with `umax`, the epilogue in f32.  The bar of that comparison is one f32 unit
in the last place of the larger of the epilogue's two terms (the library is compiled without contraction, the bar allows it).

`jxg_rotate_packed16x_q` takes any n (no lower limit), so the sizes are small: n = 130 / 256 / 300 (padded 256 / 256 / 384: two
and three 128-sample steps; at n = 130 the second column tile keeps two live columns and six of the eight column-tile workgroups of
a row tile leave at once, at n = 300 the third column tile is masked from column 44 on, at n = 256 nothing is masked)
and 37 / 275 / 700 rows (one ragged row tile, 256 + 19, three tiles).  The entry wants its two position lists to cover `nrows`; the
int8 kernel itself only walks the list it is given, so the block is passed with nrows = len(sel) and the positions of `sel` index a
LARGER block (rows / LUTs / offsets / out): the rows of that block that `sel` leaves out must keep the sentinel `out` was filled with."""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SHAPES = [(n, r) for n in (130, 256, 300) for r in (37, 275, 700)]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _codes(packed, n):
    """(m, n) two-bit codes of the packed rows (sample s: bits 2 (s & 3) of byte s >> 2)."""
    sh = (2 * (np.arange(n) & 3)).astype(np.uint8)
    return (packed[:, np.arange(n) >> 2] >> sh[None, :]) & 3


def _plane_sums(operand, qn):
    """exact sums operand (R, n) . qn[p] (npad, n)^T as int64 (every |sum| < 2^53: the f64 product is exact)"""
    a = operand.astype(np.float64)
    return np.stack([np.rint(a @ qn[p].T.astype(np.float64)).astype(np.int64) for p in range(3)])


def _combine(acc, umax):
    um = umax.astype(np.float64)
    w1, w2, w3 = um / 127.0, um / (127.0 * 254.0), um / (127.0 * 254.0 * 254.0)
    return ((acc[0] * w1[None, :] + acc[1] * w2[None, :]) + acc[2] * w3[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(n, nsel, missing):
    """Inputs on the device and the numpy reference of one shape, built once and shared by the tests (never modified)."""
    import torch
    from janusx_amd import bed, pipeline as pl, stats as st
    from janusx_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    block = nsel + 23                                   # rows of the block; `sel` leaves 23 of them out
    m = 2 * block + 5
    packed, _ = bed.synth_panel_numpy(n, m, seed=1000 * n + nsel, missing_rate=missing)
    panel = pl.Panel(torch.from_numpy(packed).to(dev), n, None)
    rng = np.random.default_rng(n + 7 * nsel)
    rows = np.sort(rng.choice(m, size=block, replace=False)).astype(np.int32)[::-1].copy()      # not contiguous, descending
    assert np.any(np.diff(rows) != -1)
    counts = panel.counts()
    _, af, _ = st.gwas_scan_row_stats(counts, n, 0.0, 1.0, 1.0)
    flip = (np.arange(block) % 3) == 1
    lut = st.scan_lut_from_counts(af[rows], flip, counts[rows], n)
    rows_t = torch.from_numpy(rows).to(dev)
    lut_t = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(n + nsel)
    ut = torch.randn((n, n), generator=g, device=dev, dtype=torch.float32) / np.sqrt(n)
    npad = lib().jxg_num_tiles(n) * 128
    q = torch.empty((3, npad, npad), dtype=torch.int8, device=dev)
    umax = torch.empty(npad, dtype=torch.float32, device=dev)
    usum = torch.empty(npad, dtype=torch.float32, device=dev)
    check(lib().jxg_ut_quant3(ut.data_ptr(), n, q.data_ptr(), umax.data_ptr(), None))
    check(lib().jxg_ut_rowsum(ut.data_ptr(), n, usum.data_ptr(), None))
    lut16 = torch.empty((block, 16), dtype=torch.uint8, device=dev)
    rowoff = torch.empty(block, dtype=torch.float32, device=dev)
    rowmiss = torch.zeros(block, dtype=torch.float32, device=dev)
    check(lib().jxg_lut_split_rows_m(panel.p32.data_ptr(), panel.m, n, rows_t.data_ptr(), lut_t.data_ptr(), block, lut16.data_ptr(),
                                     rowoff.data_ptr(), rowmiss.data_ptr(), 1 << 30 if missing > 0 else 0, None))
    torch.cuda.synchronize()
    rowoff_h, rowmiss_h = rowoff.cpu().numpy(), rowmiss.cpu().numpy()
    assert not np.isnan(rowoff_h).any(), "every row of the block must keep the exact path"
    sel = rng.permutation(block)[:nsel].astype(np.int32)                                       # strict subset, not ascending
    assert len(sel) < block and np.any(np.diff(sel) < 0)
    selm = sel[rowmiss_h[sel] != 0].copy()

    # ---- numpy reference of the rows in `sel` -------------------------------------------------------------------------------
    qh = q.cpu().numpy()
    pos = np.arange(16)
    smp = ((pos & 3) << 2) | (pos >> 2)                                  # byte `pos` of a 16-sample group holds sample `smp`
    perm = (np.arange(npad) & ~15) + smp[np.arange(npad) & 15]
    assert not qh[:, n:, :].any() and not qh[:, :, perm >= n].any()       # columns / samples beyond n are zero padding
    qn = np.empty_like(qh)
    qn[:, :, perm] = qh                                                   # planes in sample order
    qn = qn[:, :n, :n]
    codes = _codes(packed[rows[sel]], n)
    cnt = np.where(codes == 2, 1, np.where(codes == 3, 2, 0))            # second-allele counts, 0 at a missing call (code 01)
    um, us = umax.cpu().numpy()[:n], usum.cpu().numpy()[:n]
    flipped = lut16.cpu().numpy().view(np.uint16)[:, 0] != 0
    assert np.array_equal(flipped, flip)
    v0 = _combine(_plane_sums(cnt, qn), um)
    off = (rowoff_h + np.where(flipped, np.float32(2.0), np.float32(0.0)).astype(np.float32))[sel].astype(np.float32)
    sgn = np.where(flipped, np.float32(-1.0), np.float32(1.0))[sel]
    t1 = off[:, None].astype(np.float64) * us[None, :].astype(np.float64)
    t2 = (sgn[:, None] * v0).astype(np.float64)
    ref0 = (t1 + t2).astype(np.float32)
    tol0 = np.spacing(np.maximum(np.abs(t1), np.abs(t2)).astype(np.float32))
    ve = _combine(_plane_sums((codes == 1).astype(np.int64), qn), um)    # indicator of the missing calls
    return dict(n=n, block=block, dev=dev, panel=panel, rows_t=rows_t, lut16=lut16, rowoff=rowoff, rowmiss=rowmiss, usum=usum, q=q,
                umax=umax, sel=sel, sel_t=torch.from_numpy(sel).to(dev), selm=selm, selm_t=torch.from_numpy(selm).to(dev),
                ref0=ref0, tol0=tol0, ve=ve, d=rowmiss_h[sel])


def _rotate(c, form, missing_term=False):
    """out (block, n) f32 on the host after the MODE 0 launch; with missing_term also after the MODE 1 launch behind it"""
    import torch
    from janusx_amd._lib import check, lib
    out = torch.full((c["block"], c["n"]), SENTINEL, dtype=torch.float32, device=c["dev"])
    p, nsel = c["panel"], len(c["sel"])
    with _env(JXGPU_ROT_I8_MFMA=form, JXGPU_ROT_I8_DMA=None):
        check(lib().jxg_rotate_packed16x_q(p.p32.data_ptr(), p.m, c["n"], c["rows_t"].data_ptr(), nsel, c["lut16"].data_ptr(),
                                           c["rowoff"].data_ptr(), c["usum"].data_ptr(), None, None, 10, c["q"].data_ptr(),
                                           c["umax"].data_ptr(), c["sel_t"].data_ptr(), nsel, None, 0, out.data_ptr(), None))
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        if not missing_term:
            return first
        check(lib().jxg_rotate_missing_dense(p.p32.data_ptr(), p.m, c["n"], c["rows_t"].data_ptr(), c["selm_t"].data_ptr(),
                                             len(c["selm"]), c["rowmiss"].data_ptr(), c["q"].data_ptr(), c["umax"].data_ptr(),
                                             out.data_ptr(), c["n"], None))
        torch.cuda.synchronize()
    return first, out.cpu().numpy()


def _check_sentinel(c, out):
    rest = np.setdiff1d(np.arange(c["block"]), c["sel"])
    assert len(rest) == c["block"] - len(c["sel"]) > 0
    assert np.all(out[rest] == np.float32(SENTINEL)), "a row outside `sel` was written"
    assert np.all(out[c["sel"]] != np.float32(SENTINEL))


def _check_ref(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    worst = float(np.max(err / tol))
    print(f"{what}: largest |gpu - numpy| = {worst:.3f} units in the last place of the larger term")
    assert np.all(err <= tol), (what, worst)


@pytest.mark.parametrize("n,nsel", SHAPES)
def test_both_mfma_shapes_give_the_same_bits(n, nsel):
    c = _case(n, nsel, 0.0)
    o16, o32 = _rotate(c, "16"), _rotate(c, "32")
    _check_sentinel(c, o16)
    _check_sentinel(c, o32)
    assert o16.tobytes() == o32.tobytes()
    assert float(np.abs(o16[c["sel"]]).max()) > 0.1


@pytest.mark.parametrize("form", ["16", "32"])
@pytest.mark.parametrize("n,nsel", SHAPES)
def test_rotation_against_integer_plane_sums(n, nsel, form):
    c = _case(n, nsel, 0.0)
    out = _rotate(c, form)
    _check_sentinel(c, out)
    _check_ref(out[c["sel"]], c["ref0"], c["tol0"], f"n={n} rows={nsel} shape={form}")


def test_missing_call_term_on_both_mfma_shapes():
    """MODE 1: 2 % missing calls and the split limit 1 << 30, so every row keeps the exact path; the rotation, then the
    missing-call term of the rows that have one:  out += d_r (e_r U)  with the indicator of the missing calls as the operand."""
    c = _case(300, 275, 0.02)
    assert len(c["selm"]) > 0.5 * len(c["sel"]), "most rows must carry a missing-call term"
    res = {form: _rotate(c, form, missing_term=True) for form in ("16", "32")}
    assert res["16"][0].tobytes() == res["32"][0].tobytes()
    assert res["16"][1].tobytes() == res["32"][1].tobytes()
    for form, (first, last) in res.items():
        _check_sentinel(c, last)
        _check_ref(first[c["sel"]], c["ref0"], c["tol0"], f"rotation, shape={form}")
        # the term is added to what the rotation wrote: fmaf(d_r, (float)(e_r U), out)
        prev = first[c["sel"]].astype(np.float64)
        t1 = c["d"][:, None].astype(np.float64) * c["ve"].astype(np.float64)
        has = c["d"] != 0
        ref = np.where(has[:, None], (t1 + prev).astype(np.float32), first[c["sel"]])
        tol = np.spacing(np.maximum(np.abs(t1), np.abs(prev)).astype(np.float32))
        _check_ref(last[c["sel"]], ref, tol, f"missing-call term, shape={form}")
        changed = np.any(last[c["sel"]] != first[c["sel"]], axis=1)
        assert changed[has].any() and not changed[~has].any()
