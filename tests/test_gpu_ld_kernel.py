"""GPU tests of csrc/k_ld.hip below the greedy: the whole band mask of `jxg_ld_band_mask_p32` against the numpy restatement bit for
bit (the host greedy reads only a quarter of the set bits), r^2 to the last bit through thresholds one ulp apart, the six sums of
`jxg_ld_sums_p32` at the sample-count edges, through a row list and in an image beyond 4 GiB, and the LD-block matrix in several
strips.  Every comparison of masks and sums is equality: the sums are integers and the f64 expressions are the reference's in
its order.  Every mask buffer lies between guard words that are checked after every call -- no sanitizer runs on the device, so
this is the out-of-bounds check -- and every mask call runs twice with identical results (the words are built by atomic ORs).

Conditions on the inputs are asserted on the host next to each comparison and their values printed (run with -s): the two
formulas both decide set bits wherever the panel has rows of both kinds, the share of set bits is neither 0 nor 1, pairs without
a value lie inside the band, and no band pair of the restatement lies within 1e-9 (relative) of the threshold."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import janusx as jx
from janusx_amd._lib import lib
from janusx_amd.pipeline import _ptr, _stream

from test_ld_host import (PARAM_SETS, LdRef, band_block_forms, band_form_meetings, band_hits, band_margin,     # noqa: E402
                          band_pair_forms, band_r2, band_value_kinds, describe_band_diff, ld_panel, pack_band_bits,
                          ref_ld_matrix, ref_row_stats_from_counts, ref_six_sums, ref_six_sums_chunked, sparse_missing_panel,
                          valueless_panel)

pytestmark = pytest.mark.gpu

M = 4000
GUARD = 1024                      # guard words on either side of a mask buffer
PATTERN = 0x5A5AA5A5              # fits an int32


# ---- helpers -----------------------------------------------------------------------------------------------------------------

class Dev:
    """A panel in HBM with its row statistics, for direct calls of the two LD entry points."""

    def __init__(self, g=None, packed=None, n=None, own_image=False):
        """`g`: dosages (m, n), or `packed`: a payload (host array, or a device tensor used in place) with its `n`.  `own_image`:
        the P32 image and the row counts are made here on the host and not by the library (see `HostImage`)."""
        self.n = int(g.shape[1] if n is None else n)
        if own_image:
            self.panel = HostImage(g)
        else:
            self.panel = jx._panel(bed.pack_dosage(g) if packed is None else packed, self.n)
        self.mean, self.std, self.maf, self.hasmiss = jx._ld_row_stats(self.panel.counts(), self.n)
        self.dev = self.panel.device

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)


class HostImage:
    """The P32 image of dosages (m, n), n a multiple of 128, laid out on the host: tile t holds the 32 payload bytes t of every
    row, row after row (csrc/k_pack.hip).  It stands in for `pipeline.Panel` where the library's own re-tiling refuses: its grid
    takes at most 65 535 tiles (8 388 480 samples), half of what k_ld.hip documents as its limit."""

    def __init__(self, g):
        self.m, self.n = (int(v) for v in g.shape)
        assert self.n % 128 == 0
        self.nt = self.n // 128
        with ThreadPoolExecutor(8) as pool:                                    # row by row: the packer's temporaries stay small
            payload = np.concatenate(list(pool.map(lambda r: bed.pack_dosage(g[r:r + 1]), range(self.m))), axis=0)
            counts = list(pool.map(lambda r: ((g[r] < 0).sum(), (g[r] == 1).sum(), (g[r] == 2).sum()), range(self.m)))
        assert payload.shape == (self.m, 32 * self.nt)
        self.p32 = torch.from_numpy(np.ascontiguousarray(payload.reshape(self.m, self.nt, 32).transpose(1, 0, 2))).cuda()
        self.device = self.p32.device
        self._counts = np.array(counts, dtype=np.int32)                        # (missing, het, hom_alt)

    def counts(self):
        return self._counts


def device_band_mask(d, rows, r0, r1, band_end, wpr, threshold, expect=0):
    """`jxg_ld_band_mask_p32` called directly on the rows [r0, r1) of the row list `rows` (None: the panel's rows in order) ->
    (r1 - r0, wpr) uint32.  The mask lies between GUARD words of a fixed pattern, which must be unchanged after the call; the
    call runs twice, into fresh buffers, and both masks must be identical."""
    nrows = d.panel.m if rows is None else len(rows)
    sel = np.arange(nrows) if rows is None else np.asarray(rows, dtype=np.int64)
    rows_t = None if rows is None else d.up(sel.astype(np.int32))
    mean_t, std_t, miss_t = d.up(d.mean[sel]), d.up(d.std[sel]), d.up(d.hasmiss[sel].astype(np.uint8))
    band_t = d.up(np.asarray(band_end).astype(np.int32))
    assert len(band_end) == nrows
    words = max(r1 - r0, 0) * wpr
    out = []
    for _ in range(2):
        buf = torch.full((GUARD + words + GUARD,), PATTERN, dtype=torch.int32, device=d.dev)
        st = lib().jxg_ld_band_mask_p32(_ptr(d.panel.p32), d.panel.m, d.n, _ptr(rows_t), nrows, int(r0), int(r1), _ptr(band_t),
                                        _ptr(mean_t), _ptr(std_t), _ptr(miss_t), float(threshold), int(wpr),
                                        buf.data_ptr() + 4 * GUARD, _stream())
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert st == expect, (st, lib().jx_last_error())
        assert (host[:GUARD] == PATTERN).all(), f"guard words before the mask changed: {np.nonzero(host[:GUARD] != PATTERN)[0][:8]}"
        assert (host[GUARD + words:] == PATTERN).all(), \
            f"guard words after the mask changed: {np.nonzero(host[GUARD + words:] != PATTERN)[0][:8]}"
        out.append(host[GUARD:GUARD + words].view(np.uint32).reshape(max(r1 - r0, 0), wpr).copy())
    assert np.array_equal(out[0], out[1]), "two runs of the same call gave different masks"
    return out[0]


def device_sums(d, rows, i0, i1, j0, j1):
    return jx._ld_sums(d.panel, i0, i1, j0, j1, rows=rows)


class Tally:
    """Set bits by formula, pairs without a value and the closest pair to the threshold over the cases of one test."""

    def __init__(self):
        self.pairs = self.set = self.nan = 0
        self.by = {"clean": 0, "pairwise": 0}
        self.margin = np.inf

    def add(self, r2, inband, clean, hits, thresh):
        self.pairs += int(inband.sum())
        self.set += int(hits.sum())
        self.nan += int((inband & np.isnan(r2)).sum())
        self.by["clean"] += int((hits & clean).sum())
        self.by["pairwise"] += int((hits & ~clean).sum())
        self.margin = min(self.margin, band_margin(r2, thresh))

    def __str__(self):
        return (f"{self.pairs} band pairs, {self.set} set bits (clean {self.by['clean']}, pairwise {self.by['pairwise']}), "
                f"{self.nan} pairs without a value, closest pair to the threshold {self.margin:.3e} (relative)")

    def check(self, both_formulas=True):
        assert 0 < self.set < self.pairs, str(self)
        assert self.by["clean"] > 0 and (not both_formulas or self.by["pairwise"] > 0), str(self)
        assert self.margin > 1e-9, str(self)


def compare_band(d, g_ref, rows, band_end, r0, r1, wpr, threshold, label, tally=None, r2_full=None):
    """One direct band-mask call against the restatement.  `g_ref`: an LdRef of the panel's dosages at this threshold.  `r2_full`:
    the restatement (r2, inband, clean) of the whole list at a width >= wpr, when the caller has it already."""
    nrows = d.panel.m if rows is None else len(rows)
    order = np.arange(nrows) if rows is None else np.asarray(rows, dtype=np.int64)
    if r2_full is None:
        r2, inband, clean = band_r2(g_ref, order, band_end, r0, r1, wpr)
    else:
        r2, inband, clean = (a[r0:r1, :32 * wpr] for a in r2_full)
    hits = band_hits(r2, g_ref.thresh)
    want = pack_band_bits(hits)
    got = device_band_mask(d, rows, r0, r1, band_end, wpr, threshold)
    if tally is not None:
        tally.add(r2, inband, clean, hits, g_ref.thresh)
    if not np.array_equal(got, want):
        forms = band_block_forms(d.hasmiss[order], band_end, nrows, r0, r1, wpr)
        raise AssertionError(f"{label}: " + describe_band_diff(got, want, r2, clean, r0, band_pair_forms(forms, r0, r1 - r0, wpr)))
    return got


def _panel_g(name):
    if name == "sparse":
        return sparse_missing_panel(M)
    return ld_panel(601 if name == "missing" else 600, M, 11 if name == "missing" else 7, name == "missing")


@pytest.fixture(scope="module")
def devs():
    cache = {}

    def get(name):
        if name not in cache:
            g, pos = _panel_g(name)
            cache[name] = (g, pos, Dev(g))
        return cache[name]
    return get


# ---- 1. the whole band mask ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["complete", "missing", "sparse"])
@pytest.mark.parametrize("params", PARAM_SETS)
def test_production_bands_bit_for_bit(devs, name, params):
    """The bands `_ld_window_ends` / `_ld_ranges` make, whole, under the default budget (one range) and under a small one (at
    least 8 ranges); a row that two ranges share gets the same bits from both."""
    g, pos, d = devs(name)
    wbp, wv, step, thr = params
    order, _off, win_end, band_end = jx._ld_window_ends(np.zeros(M, dtype=np.int32), pos, wbp, wv, step)
    assert np.array_equal(order, np.arange(M))
    ref = LdRef(g, thr)
    full = band_r2(ref, order, band_end)
    wpr_all = full[0].shape[1] // 32
    tally = Tally()
    for budget in (jx.LD_MASK_BUDGET_BYTES, 330 * 4 * wpr_all):
        ranges = jx._ld_ranges(win_end, band_end, budget)
        assert len(ranges) == 1 if budget == jx.LD_MASK_BUDGET_BYTES else len(ranges) >= 8, len(ranges)
        seen = {}
        for a, _ws1, r1, wpr in ranges:
            got = compare_band(d, ref, None, band_end, a, r1, wpr, thr, f"{name} {params} range [{a}, {r1}) wpr {wpr}",
                               tally if len(ranges) == 1 else None, full)
            for i in range(a, r1):
                if i in seen:
                    w = min(wpr, len(seen[i]))
                    assert np.array_equal(got[i - a, :w], seen[i][:w]) and not got[i - a, w:].any() and not seen[i][w:].any(), i
                seen[i] = got[i - a]
    print(f"{name} {params}: {tally}")
    tally.check(both_formulas=name != "complete")
    if name == "sparse":
        forms = band_block_forms(d.hasmiss, band_end, M, 0, M, wpr_all)
        both, complete_in_six, _ = band_form_meetings(band_hits(full[0], ref.thresh), full[2], band_pair_forms(forms, 0, M, wpr_all))
        print(f"  mask words fed by both launch forms {both}, set bits of complete pairs in six-form blocks {complete_in_six}")
        assert both > 0 and complete_in_six > 0
        # the same rows through an explicit row list
        compare_band(d, ref, np.arange(M), band_end, 0, M, wpr_all, thr, f"sparse {params} with a row list", None, full)


def test_pairs_without_a_value_inside_the_band():
    g, pos, _kinds = valueless_panel()
    m = g.shape[0]
    d = Dev(g)
    for wbp, wv, step, thr in ((None, 50, 5, 0.2), (30000, None, 3, 0.3)):
        order, _off, _we, band_end = jx._ld_window_ends(np.zeros(m, dtype=np.int32), pos, wbp, wv, step)
        ref = LdRef(g, thr)
        full = band_r2(ref, order, band_end)
        k = band_value_kinds(ref, order, *full)
        tally = Tally()
        compare_band(d, ref, None, band_end, 0, m, full[0].shape[1] // 32, thr, f"valueless {(wbp, wv, step, thr)}", tally, full)
        print(f"valueless {(wbp, wv, step, thr)}: {k}; {tally}")
        assert k["nan"] > 0 and k["n_le_1"] > 0 and k["zero_variance"] > 0 and k["std_floor"] > 0 and k["r2_one"] >= 4
        assert k["r2_one_clean"] >= 2
        tally.check()


def _hand_band(rng, nrows, w):
    """Non-monotone band ends, drawn per row between i + 1 and min(nrows, i + 1 + 32 w), with rows that have no pair and rows
    that reach nrows exactly."""
    idx = np.arange(nrows)
    hi = np.minimum(nrows, idx + 1 + 32 * w)
    be = idx + 1 + (rng.random(nrows) * (hi - idx)).astype(np.int64)          # in [i + 1, hi]
    be = np.minimum(be, hi)
    be[rng.random(nrows) < 0.1] = 0
    be = np.maximum(be, idx + 1)                                            # a tenth of the rows: no pair
    reach = (rng.random(nrows) < 0.1) & (hi == nrows)
    be[reach] = nrows
    if nrows >= 2:
        be[0] = hi[0]                                                       # the widest row the width admits
    return be


@pytest.mark.parametrize("nrows", [1, 2, 31, 32, 33, 63, 64, 65, 1003, 1400])
def test_hand_made_bands(devs, nrows):
    """The kernel must not depend on how the host makes `band_end`: non-monotone ends up to 40 words wide (11 workgroups in x,
    j-blocks that end early), the true `wpr`, a smaller one (the cap min(band_end, i + 1 + 32 wpr) must hold: nothing past the
    mask row, guards intact) and 1; row ranges that start off a 32-row boundary, of 1 / 31 / 32 / 33 rows, up to nrows, and
    empty."""
    g, _pos, _ = devs("missing")
    g = g[:nrows].copy()
    if nrows > 40:
        g[nrows // 2] = g[nrows // 2 - 1]                                    # an r2 of 1 far from the diagonal's neighbours
    d = Dev(g)
    thr = 0.01                # unlinked rows of n = 601 have r2 of the order 1 / n: both outcomes occur at every distance
    ref = LdRef(g, thr)
    rng = np.random.default_rng(100 + nrows)
    tally = Tally()
    for w in (40, 3):
        be = _hand_band(rng, nrows, w)
        need = max(1, (int(np.max(be - np.arange(nrows) - 1)) + 31) // 32)
        assert need == w or nrows < 1400                                      # 1400 rows: the widest row fills 40 words
        starts = sorted({0, min(5, nrows - 1), min(37, nrows - 1), max(nrows - 33, 0), nrows - 1})
        ranges = {(0, nrows), (nrows, nrows), (min(5, nrows), min(5, nrows))}
        for r0 in starts:
            for ln in (1, 31, 32, 33):
                ranges.add((r0, min(r0 + ln, nrows)))
            ranges.add((r0, nrows))
        for wpr in sorted({need, w, max(1, need // 3), 1}):                  # w > need: a mask wider than any band
            full = band_r2(ref, np.arange(nrows), be, 0, nrows, wpr)
            for r0, r1 in sorted(ranges):
                got = compare_band(d, ref, None, be, r0, r1, wpr, thr, f"nrows {nrows} width {w} wpr {wpr} rows [{r0}, {r1})",
                                   tally if (r0, r1) == (0, nrows) else None, full)
                assert got.shape == (r1 - r0, wpr)
    print(f"hand-made bands, nrows {nrows}: {tally}")
    if nrows >= 31:
        tally.check()
    else:
        assert tally.margin > 1e-9


def test_row_lists(devs):
    """The image read through a row list: a permutation, a descending list, a list with repeated records and a short list into
    a panel with many more rows."""
    g, _pos, d = devs("missing")
    rng = np.random.default_rng(21)
    near = np.arange(700)
    near[::2] = near[::2][rng.permutation(350)]                              # half of the rows stay beside an LD neighbour
    lists = {"permutation": near, "descending": np.arange(1500, 800, -1),
             "repeated records": np.sort(rng.integers(0, 300, size=700)),
             "short list into a long panel": np.sort(rng.permutation(M)[:200])}
    lists["short list into a long panel"][[0, -1]] = [0, M - 1]
    thr = 0.005               # unlinked rows of n = 601 have r2 of the order 1 / n: set bits at every distance
    ref = LdRef(g, thr)
    for label, rows in lists.items():
        nrows = len(rows)
        be = _hand_band(rng, nrows, 6)
        tally = Tally()
        for r0, r1, wpr in ((0, nrows, 6), (41, nrows - 7, 2)):
            compare_band(d, ref, rows, be, r0, r1, wpr, thr, f"{label} rows [{r0}, {r1}) wpr {wpr}", tally)
        print(f"row list, {label}: {tally}")
        tally.check()
        for blk in ((0, nrows, 0, nrows), (13, 14, 5, nrows), (nrows - 35, nrows, 31, 32)):
            got = device_sums(d, rows, *blk)
            assert np.array_equal(got, ref_six_sums(g, rows[blk[0]:blk[1]], rows[blk[2]:blk[3]])), (label, blk)


# ---- 2. r^2 to the last bit ------------------------------------------------------------------------------------------------------

def _threshold_for(v):
    """A threshold t with t * (1 + 1e-12) == v in the double product the library forms, or None."""
    c = v / (1.0 + 1e-12)
    cands = [c]
    for _ in range(4):
        cands = [np.nextafter(cands[0], 0.0)] + cands + [np.nextafter(cands[-1], 2.0)]
    for t in cands:
        if float(t) * (1.0 + 1e-12) == v:
            return float(t)
    return None


def test_r2_to_the_last_bit():
    """The mask is the only view of the device's r^2.  For the restatement's value v of a pair, a threshold whose product with
    (1 + 1e-12) is exactly v must leave the pair's bit 0 (a device value one ulp high sets it) and one whose product is the
    double below v must set it (a device value one ulp low leaves it 0); both times the whole mask equals the restatement's."""
    g, _ = ld_panel(601, 64, 31)
    rng = np.random.default_rng(32)
    holed = rng.permutation(64)[:16]
    sub = g[holed]
    sub[rng.random(sub.shape) < 0.02] = -9
    g[holed] = sub
    full_rows = np.setdiff1d(np.arange(64), holed)
    g[full_rows[1]] = g[full_rows[0]]                                        # one pair of identical complete rows
    twin = (int(min(full_rows[0], full_rows[1])), int(max(full_rows[0], full_rows[1])))
    d = Dev(g)
    assert d.hasmiss.sum() == 16
    be = np.full(64, 64)
    order = np.arange(64)
    r2, inband, clean = band_r2(LdRef(g, 0.5), order, be, 0, 64, 2)
    chosen = [(twin[0], twin[1] - twin[0] - 1)]
    for is_clean in (True, False):
        sel = np.argwhere(inband & np.isfinite(r2) & (clean == is_clean) & (r2 > 0) & (r2 < 1))
        vals = r2[sel[:, 0], sel[:, 1]]
        by_value = np.argsort(vals)
        assert vals[by_value[0]] < 1e-3
        # up to 30 values spread evenly in log r2 from the smallest to the largest below 1
        targets = np.exp(np.linspace(np.log(max(vals[by_value[0]], 1e-7)), np.log(vals[by_value[-1]]), 30))
        picks = sorted({int(by_value[min(np.searchsorted(vals[by_value], t), len(vals) - 1)]) for t in targets}
                       | {int(by_value[0]), int(by_value[-1])})
        assert len(picks) >= 16, len(picks)
        chosen += [tuple(int(k) for k in sel[p]) for p in picks]
    done = {True: 0, False: 0}
    skipped = 0
    for row, o in chosen:
        v = float(r2[row, o])
        t0, t1 = _threshold_for(v), _threshold_for(float(np.nextafter(v, 0.0)))
        if t0 is None or t1 is None:
            skipped += 1
            continue
        for t, bit in ((t0, 0), (t1, 1)):
            ref = LdRef(g, t)
            assert ref.thresh == (v if bit == 0 else float(np.nextafter(v, 0.0)))
            got = compare_band(d, ref, None, be, 0, 64, 2, t, f"pair ({row}, {row + 1 + o}) r2 {v!r} threshold {t!r}")
            assert (int(got[row, o >> 5]) >> (o & 31)) & 1 == bit, (row, o, v, t, bit)
        done[bool(clean[row, o])] += 1
    print(f"last bit: {done[True]} clean and {done[False]} pairwise pairs at thresholds one ulp apart, {skipped} of {len(chosen)} "
          f"skipped (no threshold with that product), r2 from {min(r2[r, o] for r, o in chosen):.3e} to "
          f"{max(r2[r, o] for r, o in chosen)!r}")
    assert 10 * skipped <= len(chosen)
    assert done[True] >= 16 and done[False] >= 16


# ---- 3. the six sums at the sample edges -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_six_sums_small_n(n):
    """One tile, and n at and around the MFMA step (64) and the tile (128): all four codes, a row with every call missing, a row
    of 2s, samples missing in every row at the tail (pad samples must add nothing); rectangles ragged on both sides."""
    rng = np.random.default_rng(500 + n)
    m = 70
    g = rng.integers(-1, 3, size=(m, n)).astype(np.int8)
    g[g < 0] = -9
    if n > 2:
        g[:, n - max(1, n // 9):] = -9
    g[11] = -9
    g[12] = 2
    g[13] = 1
    g[14] = 0
    d = Dev(g)
    for blk in ((0, m, 0, m), (3, 4, 0, m), (0, m, 5, 6), (1, 34, 33, m), (37, m, 0, 33), (31, 65, 30, 63), (69, 70, 69, 70)):
        got = device_sums(d, None, *blk)
        want = ref_six_sums(g, np.arange(blk[0], blk[1]), np.arange(blk[2], blk[3]))
        assert got.dtype == np.int32 and got.shape == want.shape
        for p, name in enumerate(("D", "N", "S_i", "S_j", "Q_i", "Q_j")):
            assert np.array_equal(got[p], want[p]), (name, n, blk)
    # the band mask at these sample counts (n - 1 = 0 and 1 in the clean formula's denominator)
    be = np.full(m, m)
    for thr in (0.05, 0.5):
        compare_band(d, LdRef(g, thr), None, be, 0, m, 3, thr, f"n {n} threshold {thr}")


def _long_panel(n, seed, chunk=1 << 20):
    """33 rows of n samples: two rows of 2s, then an LD chain (each row copies the one before and redraws a tenth of it), every
    third row of the chain with 2 % missing calls.  Drawn in sample chunks, each from its own stream, by a few threads."""
    g = np.empty((33, n), dtype=np.int8)

    def fill(c0):
        w = min(chunk, n - c0)
        rng = np.random.default_rng([seed, c0])
        out = g[:, c0:c0 + w]
        out[:2] = 2
        prev = rng.integers(0, 3, size=w, dtype=np.int8)
        for r in range(2, 33):
            if r > 2:
                redraw = rng.integers(0, 10, size=w, dtype=np.int8) == 0
                prev = np.where(redraw, rng.integers(0, 3, size=w, dtype=np.int8), prev)
            out[r] = prev
            if r % 3 == 0:
                out[r][rng.integers(0, 50, size=w, dtype=np.int8) == 0] = -9
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(fill, range(0, n, chunk)))
    g[1, ::1000] = -9
    return g


def test_six_sums_and_mask_at_the_largest_n():
    """n = 2^24, the documented limit: D and Q reach 2^26 on rows of 2s, and the mask's f64 products (n mean mean, S S, Q N) are
    near 2^50.  The reference sums are float64 products of chunks of 2^20 samples, exact, added in int64.  The image is laid out
    by the test: the library's re-tiling refuses this n ("jxg_repack_p32: grid too large", 131 072 tiles for a grid of 65 535),
    so through `jx._panel` the LD entry points are reachable up to 8 388 480 samples only."""
    n = 1 << 24
    g = _long_panel(n, 77)
    d = Dev(g, own_image=True)
    want = ref_six_sums_chunked(g)
    assert want[0, 0, 0] == 1 << 26 and want[4, 0, 0] == 1 << 26 and want.max() == 1 << 26
    got = device_sums(d, None, 0, 33, 0, 33)
    for p, name in enumerate(("D", "N", "S_i", "S_j", "Q_i", "Q_j")):
        assert np.array_equal(got[p], want[p]), (name, np.argwhere(got[p] != want[p])[:4])
    assert np.array_equal(device_sums(d, None, 32, 33, 1, 33), want[:, 32:33, 1:33])
    idx = np.arange(33)
    st = ref_row_stats_from_counts(want[1, idx, idx], want[2, idx, idx], want[4, idx, idx], n)
    assert np.array_equal(st["mean"], d.mean) and np.array_equal(st["std"], d.std) and np.array_equal(st["has_missing"], d.hasmiss)
    be = np.full(33, 33)
    for thr in (0.2, 0.6):
        ref = LdRef(g, thr, st=st, sums=want)
        tally = Tally()
        compare_band(d, ref, None, be, 0, 33, 1, thr, f"n 2^24 threshold {thr}", tally)
        print(f"n = 2^24, threshold {thr}: {tally}")
        tally.check()


def test_image_beyond_4_gib():
    """An image of more than 4 GiB (2.2 million records of 64 tiles): the tile stride times the tile index passes 2^32.  The
    payload is drawn on the device; about 70 rows, the first and the last record among them, are compared through a row list."""
    m, n = 2_200_000, 8192
    bps = n // 4
    need = 2 * m * bps + (1 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need >> 20} MiB of free HBM for the payload and its image, {free >> 20} MiB are free")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    payload = torch.randint(0, 256, (m, bps), dtype=torch.uint8, device="cuda", generator=gen)
    rng = np.random.default_rng(6)
    rows = np.unique(np.concatenate([[0, 1, m - 2, m - 1], rng.integers(0, m, size=66)])).astype(np.int64)
    rows = rows[rng.permutation(len(rows))]
    raw = payload[torch.from_numpy(rows).cuda()].cpu().numpy()
    codes = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(len(rows), n)
    # a uniform payload has missing calls (code 01) in every row: half of the chosen rows get 00 there, so both formulas decide
    whole = rng.random(len(rows)) < 0.5
    codes[whole] = np.where(codes[whole] == 1, 0, codes[whole])
    g = np.array([0, -9, 1, 2], dtype=np.int8)[codes]
    payload[torch.from_numpy(rows[whole]).cuda()] = torch.from_numpy(bed.pack_dosage(g[whole])).cuda()
    d = Dev(packed=payload, n=n)
    assert d.panel.p32.numel() > (1 << 32) and d.panel.nt == 64
    k = len(rows)
    got = device_sums(d, rows, 0, k, 0, k)
    want = ref_six_sums(g, np.arange(k), np.arange(k))
    for p, name in enumerate(("D", "N", "S_i", "S_j", "Q_i", "Q_j")):
        assert np.array_equal(got[p], want[p]), (name, np.argwhere(got[p] != want[p])[:4])
    # unlinked rows: r2 is of the order 1 / n, so a threshold there gives both outcomes
    thr = 1.0 / n
    ref = LdRef(g, thr)
    r2, inband, clean = band_r2(ref, np.arange(k), np.full(k, k), 0, k, 3)
    hits = band_hits(r2, ref.thresh)
    tally = Tally()
    tally.add(r2, inband, clean, hits, ref.thresh)
    print(f"image beyond 4 GiB: {tally}")
    tally.check()
    mask = device_band_mask(d, rows, 0, k, np.full(k, k), 3, thr)
    assert np.array_equal(mask, pack_band_bits(hits)), describe_band_diff(mask, pack_band_bits(hits), r2, clean, 0)


def test_refusals_that_need_a_device():
    """More than 2 097 120 rows in one range (65 535 i-blocks): refused, with buffers of the size the arguments claim (a row list
    that repeats a few records keeps the image small)."""
    g, _ = ld_panel(130, 64, 3)
    d = Dev(g)
    nrows = 2_097_121
    rows = (np.arange(nrows) % 64).astype(np.int64)
    be = np.minimum(np.arange(nrows) + 2, nrows)
    device_band_mask(d, rows, 0, nrows, be, 1, 0.2, expect=1)
    assert lib().jx_last_error().decode() == "jxg_ld_band_mask_p32: at most 2 097 120 rows per range"
    rows_t = d.up(rows.astype(np.int32))
    out = torch.zeros((6, nrows, 1), dtype=torch.int32, device=d.dev)
    st = lib().jxg_ld_sums_p32(_ptr(d.panel.p32), d.panel.m, d.n, _ptr(rows_t), nrows, 0, nrows, 0, 1, _ptr(out), _stream())
    torch.cuda.synchronize()
    assert st == 1 and lib().jx_last_error().decode() == "jxg_ld_sums_p32: at most 2 097 120 rows per block"
    assert not out.any()
    # one row fewer is served
    got = device_band_mask(d, rows, 0, nrows - 1, be, 1, 0.2)
    want = _numpy_rows(g, rows[:64 + 1], 0.2)
    assert np.array_equal(got[:64, 0], want)


def _numpy_rows(g, rows, thr):
    """Bit 0 of the mask rows of consecutive pairs (i, i + 1) of a row list."""
    ref = LdRef(g, thr)
    r2 = np.array([ref.r2_block(rows[i], rows[i + 1:i + 2])[0][0] for i in range(len(rows) - 1)])
    return band_hits(r2, ref.thresh).astype(np.uint32)


# ---- 4. the LD-block matrix in several strips ----------------------------------------------------------------------------------------

def test_ld_block_matrix_in_strips(devs, monkeypatch):
    g, _pos, _ = devs("missing")
    sub = g[1000:1301].copy()
    sub[7] = -9
    sub[8] = 1
    m, n = sub.shape
    packed = bed.pack_dosage(sub)
    one = jx.ld_r2_matrix_packed(packed, n)
    calls = []
    real = jx._ld_sums
    monkeypatch.setattr(jx, "_ld_sums", lambda *a, **k: (calls.append(a[1:5]), real(*a, **k))[1])
    monkeypatch.setattr(jx, "LD_MASK_BUDGET_BYTES", 24 * m * 64)
    strips = jx.ld_r2_matrix_packed(packed, n)
    assert [c[:2] for c in calls] == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 301)]
    assert np.array_equal(strips, one)                                # the same integer sums through the same f64 expression
    err = float(np.max(np.abs(strips.astype(np.float64) - ref_ld_matrix(sub))))
    print(f"ld_r2_matrix_packed in 5 strips of m = {m}: max abs error {err:.3e} (bar 2e-7)")
    assert err <= 2e-7
    monkeypatch.undo()
    calls.clear()
    monkeypatch.setattr(jx, "_ld_sums", lambda *a, **k: (calls.append(a[1:5]), real(*a, **k))[1])
    big = jx.ld_r2_matrix_packed(bed.pack_dosage(g), g.shape[1])
    assert len(calls) == 2 and calls[0][1] % 32 == 0 and calls[1][1] == M, calls
    err = float(np.max(np.abs(big.astype(np.float64) - ref_ld_matrix(g))))
    print(f"ld_r2_matrix_packed in 2 strips of m = {M}: max abs error {err:.3e} (bar 2e-7)")
    assert err <= 2e-7
