"""Host tests of the LD-pruning feature (`jx gformat -prune`), no GPU: the windows and the strict greedy of the host layer
(`jx_ld_window_ends`, `jx_ld_prune_greedy`) against a numpy restatement of the reference algorithm, the `-prune` argument parsers,
the argument errors of `bed_packed_ld_prune_maf_priority` and the `.bim` selection of `bed_ldblock_r2_rust`.

The restatement below (row statistics, the two pair formulas, the strict greedy, the LD-block matrix) is the one
`tests/test_gpu_ld.py` compares the device results with.  It is written from the reference's text (src/stats/ld.rs:270-402,
469-549, 1095-1198; src/math/ld.rs:817-834) in float64 / integer numpy and asks for pairs lazily, as the reference does: a pair's
r^2 is computed when the greedy first asks for it (in blocks of consecutive partners of the same row, each value being the
per-pair expression)."""
import os

import numpy as np
import pytest

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx


# ---- panel ---------------------------------------------------------------------------------------------------------------------

def ld_panel(n, m, seed, missing=False):
    """LD panel: SNPs in blocks of 8; the first SNP of a block draws two haplotype rows with frequency p ~ U(0.05, 0.5), each later
    one copies the previous SNP's haplotypes and redraws each entry (from the block's p) with probability 0.1; dosage = haplotype
    sum.  Positions: cumulative sums of integers in [1, 2000).  `missing`: 2 % missing calls (-9) on a random half of the rows.
    -> (dosage (m, n) int8, positions int64)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((m, n), dtype=np.int8)
    hap = None
    p = 0.0
    for i in range(m):
        if i % 8 == 0:
            p = rng.uniform(0.05, 0.5)
            hap = rng.random((2, n)) < p
        else:
            redraw = rng.random((2, n)) < 0.1
            hap = np.where(redraw, rng.random((2, n)) < p, hap)
        g[i] = hap[0].astype(np.int8) + hap[1].astype(np.int8)
    pos = np.cumsum(rng.integers(1, 2000, size=m)).astype(np.int64)
    if missing:
        rows = rng.permutation(m)[: m // 2]
        hole = rng.random((rows.size, n)) < 0.02
        sub = g[rows]
        sub[hole] = -9
        g[rows] = sub
    return g, pos


# ---- restatement ---------------------------------------------------------------------------------------------------------------

def ref_row_stats(g):
    """src/stats/ld.rs:469-543 -> dict of mean, std, maf (f64), has_missing, and the integer counts."""
    g = np.asarray(g)
    m, n = g.shape
    v = g >= 0
    g0 = np.where(v, g, 0).astype(np.int64)
    return ref_row_stats_from_counts(v.sum(axis=1).astype(np.int64), g0.sum(axis=1), (g0 * g0).sum(axis=1), n)


def ref_row_stats_from_counts(non_missing, alt_sum, sq_sum, n):
    """The float part of `ref_row_stats` from the integer row sums (called calls, sum g, sum g^2)."""
    m = len(non_missing)
    denom = float(max(n - 1, 1))
    mean, std, maf = np.zeros(m), np.full(m, 1e-6), np.zeros(m)
    for i in range(m):
        if non_missing[i] > 0:
            obs_n, sum_g, sum_g2 = float(non_missing[i]), float(alt_sum[i]), float(sq_sum[i])
            p = sum_g / (2.0 * obs_n)
            maf[i] = min(p, 1.0 - p)
            mean[i] = sum_g / obs_n
            ss = max(sum_g2 - (sum_g * sum_g / obs_n), 0.0)
            std[i] = np.sqrt(max(ss / denom, 1e-12))
    return dict(mean=mean, std=std, maf=maf, has_missing=non_missing < n, non_missing=non_missing, alt_sum=alt_sum, sq_sum=sq_sum)


def ref_six_sums(g, rows_i, rows_j):
    """D, N, S_i, S_j, Q_i, Q_j (int64, (len(rows_i), len(rows_j))) of row pairs.  The products run in float64 (BLAS): every
    partial sum is an integer <= 4 n < 2^53, so they are exact in any order of addition."""
    g = np.asarray(g)
    vi, vj = (g[rows_i] >= 0).astype(np.float64), (g[rows_j] >= 0).astype(np.float64)
    gi, gj = np.where(vi > 0, g[rows_i], 0).astype(np.float64), np.where(vj > 0, g[rows_j], 0).astype(np.float64)
    out = np.stack([gi @ gj.T, vi @ vj.T, gi @ vj.T, vi @ gj.T, (gi * gi) @ vj.T, vi @ (gj * gj).T])
    return np.rint(out).astype(np.int64)


def ref_six_sums_chunked(g, chunk=1 << 20, threads=8):
    """The six sums of all row pairs of a panel with many samples -> (6, m, m) int64: float64 matrix products over chunks of
    `chunk` samples (every entry of a chunk's product is an integer <= 4 chunk < 2^53, so the product is exact whatever order
    the BLAS adds in), added in int64.  One product per chunk, of the stacked planes (d; v; q) with their transpose, holds the
    six blocks; the chunks are shared among `threads` threads (numpy releases the lock in its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    g = np.asarray(g)
    m, n = g.shape
    blk = (slice(0, m), slice(m, 2 * m), slice(2 * m, 3 * m))                # d, v, q

    def one(c0):
        gc = g[:, c0:c0 + chunk]
        a = np.empty((3 * m, gc.shape[1]), dtype=np.float64)
        np.maximum(gc, 0, out=a[blk[0]], casting="unsafe")
        np.greater_equal(gc, 0, out=a[blk[1]], casting="unsafe")
        np.multiply(a[blk[0]], a[blk[0]], out=a[blk[2]])
        p = np.rint(a @ a.T).astype(np.int64)
        return np.stack([p[blk[x], blk[y]] for x, y in ((0, 0), (1, 1), (0, 1), (1, 0), (2, 1), (1, 2))])
    with ThreadPoolExecutor(threads) as pool:
        return sum(pool.map(one, range(0, n, chunk)), np.zeros((6, m, m), dtype=np.int64))


class LdRef:
    """The pair predicate "in LD" of the reference (src/stats/ld.rs:339-368) with its two formulas, asked lazily."""

    def __init__(self, g, r2_threshold, st=None, sums=None):
        """`st` / `sums`: row statistics and the (6, m, m) integer sums of all row pairs computed elsewhere (a panel too long to
        go through `ref_row_stats` / `ref_six_sums` in one piece)."""
        self.g = np.asarray(g)
        self.n = self.g.shape[1]
        self.st = ref_row_stats(self.g) if st is None else st
        self.sums = sums
        self.thresh = float(r2_threshold) * (1.0 + 1e-12)
        self.hits = {"clean": 0, "pairwise": 0}           # pairs in LD the greedy met, by the formula that decided them
        self.asked = 0
        self.min_margin = np.inf                          # smallest |r2 - thresh| / thresh over the pairs the greedy asked for
        self._cache = {}

    def r2_block(self, gi, gjs):
        """r^2 of row gi against the rows gjs (NaN where the reference has no value), and which pairs took the clean formula."""
        r2, is_clean = self.r2_rect(np.asarray([gi]), np.asarray(gjs))
        return r2[0], is_clean[0]

    def six_sums(self, gis, gjs):
        if self.sums is not None:
            return self.sums[:, np.asarray(gis)[:, None], np.asarray(gjs)[None, :]]
        return ref_six_sums(self.g, gis, gjs)

    def r2_rect(self, gis, gjs):
        """r^2 of every row of gis against every row of gjs, each value the per-pair expression (numpy's elementwise f64
        operations are the IEEE ones) -> ((len(gis), len(gjs)) f64 with NaN where the reference has no value, and which pairs
        took the clean formula)."""
        st, n = self.st, self.n
        gis, gjs = np.asarray(gis, dtype=np.int64), np.asarray(gjs, dtype=np.int64)
        d, nn, si, sj, si2, sj2 = self.six_sums(gis, gjs).astype(np.float64)
        denom = float(max(n - 1, 1))
        cov = d - (float(n) * st["mean"][gis])[:, None] * st["mean"][gjs][None, :]
        denom_corr = (denom * st["std"][gis])[:, None] * st["std"][gjs][None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            corr = np.where(denom_corr > 0.0, cov / denom_corr, 0.0)
            clean = corr * corr
            cov_num = d * nn - si * sj
            var_i = si2 * nn - si * si
            var_j = sj2 * nn - sj * sj
            den = var_i * var_j
            pw = (cov_num * cov_num) / den
        pw = np.where((nn > 1) & np.isfinite(den) & (den > 0.0) & np.isfinite(cov_num), pw, np.nan)
        is_clean = ~st["has_missing"][gis][:, None] & ~st["has_missing"][gjs][None, :]
        return np.where(is_clean, clean, pw), is_clean

    def in_ld(self, idx_list, li, lj):
        key = (id(idx_list), li)
        hit = self._cache.get(key)
        if hit is None or not (hit[0] <= lj < hit[0] + len(hit[1])):
            gjs = np.asarray(idx_list[lj:lj + 128])
            hit = (lj,) + self.r2_block(idx_list[li], gjs)
            self._cache[key] = hit
        r2, is_clean = hit[1][lj - hit[0]], hit[2][lj - hit[0]]
        self.asked += 1
        if np.isfinite(r2):
            self.min_margin = min(self.min_margin, abs(r2 - self.thresh) / self.thresh)
        ld = bool(np.isfinite(r2) and r2 > self.thresh)
        if ld:
            self.hits["clean" if is_clean else "pairwise"] += 1
        return ld


def ref_groups(chrom_codes):
    """Rows grouped by chromosome code, groups by first appearance (the outcome does not depend on their order)."""
    groups = {}
    for i, c in enumerate(np.asarray(chrom_codes).tolist()):
        groups.setdefault(c, []).append(i)
    return list(groups.values())


def ref_windows(idx_list, positions, window_bp, window_variants, step):
    """Windows [(block_start, end)] of one chromosome in local indices: src/stats/ld.rs:275-305, 397-400."""
    l = len(idx_list)
    out = []
    if l <= 1:
        return out
    pos = [int(positions[k]) for k in idx_list]
    pos_sorted = all(pos[k] >= pos[k - 1] for k in range(1, l))
    bp_end_ptr, block_start = 1, 0
    while block_start < l:
        if window_bp is not None:
            if pos_sorted:
                bp_end_ptr = max(bp_end_ptr, block_start + 1)
                target = pos[block_start] + window_bp
                while bp_end_ptr < l and pos[bp_end_ptr] <= target:
                    bp_end_ptr += 1
                end = bp_end_ptr
            else:
                e, p0 = block_start + 1, pos[block_start]
                while e < l:
                    if pos[e] - p0 <= window_bp:
                        e += 1
                    elif pos[e] > p0:
                        break
                    else:
                        e += 1
                end = e
        else:
            end = min(block_start + window_variants, l)
        out.append((block_start, end))
        if end >= l:
            break
        block_start += step
    return out


def ref_prune(in_ld, maf, chrom_codes, positions, window_bp, window_variants, step):
    """Strict greedy, src/stats/ld.rs:270-402 -> bool keep mask.  in_ld(idx_list, li, lj)."""
    m = len(maf)
    keep = np.ones(m, dtype=bool)
    eps = 1e-12
    for idx_list in ref_groups(chrom_codes):
        l = len(idx_list)
        dropped = [False] * l
        first_unchecked = [li + 1 for li in range(l)]
        for block_start, end in ref_windows(idx_list, positions, window_bp, window_variants, step):
            if end <= block_start + 1:
                continue
            while True:
                at_least_one_prune = False
                for li in range(block_start, end - 1):
                    if dropped[li]:
                        continue
                    scan_min = max(first_unchecked[li], block_start + 1)
                    if scan_min >= end:
                        first_unchecked[li] = end
                        continue
                    pruned_this_round = False
                    lj = scan_min
                    while lj < end:
                        if dropped[lj]:
                            lj += 1
                            continue
                        if in_ld(idx_list, li, lj):
                            at_least_one_prune = pruned_this_round = True
                            if maf[idx_list[li]] < (1.0 - eps) * maf[idx_list[lj]]:
                                dropped[li] = True
                            else:
                                dropped[lj] = True
                                nxt = lj + 1
                                while nxt < end and dropped[nxt]:
                                    nxt += 1
                                first_unchecked[li] = nxt
                            break
                        lj += 1
                    if not pruned_this_round and not dropped[li]:
                        first_unchecked[li] = end
                if not at_least_one_prune:
                    break
        for li in range(l):
            if dropped[li]:
                keep[idx_list[li]] = False
    return keep


def ref_prune_panel(g, chrom_codes, positions, window_bp, window_variants, step, r2):
    """-> (keep, LdRef with the counters of the run)."""
    ref = LdRef(g, r2)
    return ref_prune(ref.in_ld, ref.st["maf"], chrom_codes, positions, window_bp, window_variants, step), ref


def ref_ld_matrix(g):
    """`ld_r2_matrix_from_packed_rows_blas` (src/stats/ld.rs:1095-1198) in f64, the row mean rounded to f32 as there -> f64 (m, m)."""
    g = np.asarray(g)
    m = g.shape[0]
    if m == 0:
        return np.zeros((0, 0))
    if m == 1:
        return np.ones((1, 1))
    mu = ref_row_stats(g)["mean"].astype(np.float32).astype(np.float64)
    x = np.where(g >= 0, g.astype(np.float64) - mu[:, None], 0.0)
    gram = x @ x.T
    diag = np.maximum(np.diag(gram), 0.0)
    den = np.sqrt(diag[:, None] * diag[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = np.where(den > 1e-20, gram / np.where(den > 1e-20, den, 1.0), 0.0)
    r2 = corr * corr
    r2 = np.clip(np.where(np.isfinite(r2), r2, 0.0), 0.0, 1.0)
    np.fill_diagonal(r2, 1.0)
    return r2


PARAM_SETS = [(None, 50, 5, 0.2), (None, 200, 1, 0.5), (50000, None, 10, 0.2)]     # (window_bp, window_variants, step, r2)
PANELS = {"complete": (600, False), "missing": (601, True)}


def check_ref_conditions(keep, ref):
    """What the issue asks of the restatement on the LD panel, so that a comparison with it proves something."""
    share = keep.mean()
    assert 0.05 <= share <= 0.50, share
    assert ref.min_margin > 1e-9, ref.min_margin


# ---- the host layer against the restatement --------------------------------------------------------------------------------------

def _positions_layout(chrom_codes, positions, window_bp, window_variants, step):
    """The restatement's windows and band ends in the chromosome-grouped positions `jx_ld_window_ends` uses."""
    groups = ref_groups(chrom_codes)
    m = len(chrom_codes)
    order = np.array([i for grp in groups for i in grp], dtype=np.int64).reshape(-1)
    off = np.cumsum([0] + [len(grp) for grp in groups]).astype(np.int64)
    win_end, band_end = np.zeros(m, dtype=np.int64), np.arange(1, m + 1, dtype=np.int64)
    for gi, grp in enumerate(groups):
        c0 = int(off[gi])
        for bs, end in ref_windows(grp, positions, window_bp, window_variants, step):
            win_end[c0 + bs] = c0 + end
            band_end[c0 + bs:c0 + end] = np.maximum(band_end[c0 + bs:c0 + end], c0 + end)
    return order, off, win_end, band_end


def band_r2(ref, order, band_end, r0=0, r1=None, wpr=None):
    """The restatement's r^2 of every pair of the band of the rows [r0, r1) of the row list `order`, in the layout of
    `jxg_ld_band_mask_p32`: column o of row i - r0 is the pair (i, j = i + 1 + o), o < 32 wpr, and the pair is in the band when
    j < min(band_end[i], i + 1 + 32 wpr, len(order)).  `wpr` None: the words the widest band of the whole list needs.
    -> (r2 (r1 - r0, 32 wpr) f64, NaN outside the band and where the reference has no value; inband; took the clean formula)."""
    order, band_end = np.asarray(order, dtype=np.int64), np.asarray(band_end, dtype=np.int64)
    m = len(order)
    r1 = m if r1 is None else int(r1)
    if wpr is None:
        width = int(np.max(band_end - np.arange(m) - 1)) if m else 0
        wpr = max(1, (width + 31) // 32)
    w = 32 * int(wpr)
    rr = max(r1 - r0, 0)
    r2, inband, clean = np.full((rr, w), np.nan), np.zeros((rr, w), dtype=bool), np.zeros((rr, w), dtype=bool)
    o = np.arange(w, dtype=np.int64)
    for a in range(r0, r1, 64):
        b = min(a + 64, r1)
        ps = np.arange(a, b, dtype=np.int64)
        be = np.minimum(np.minimum(band_end[a:b], ps + 1 + w), m)
        top = int(be.max())
        if top <= a + 1:
            continue
        span = np.arange(a + 1, top, dtype=np.int64)
        v, c = ref.r2_rect(order[ps], order[span])
        ok = (ps[:, None] + 1 + o[None, :]) < be[:, None]
        at = np.minimum((ps - a)[:, None] + o[None, :], len(span) - 1)          # j = i + 1 + o is entry (i - a) + o of the span
        r2[a - r0:b - r0] = np.where(ok, np.take_along_axis(v, at, 1), np.nan)
        clean[a - r0:b - r0] = ok & np.take_along_axis(c, at, 1)
        inband[a - r0:b - r0] = ok
    return r2, inband, clean


def pack_band_bits(hits):
    """(rows, 32 wpr) bool -> (rows, wpr) uint32, bit o & 31 of word o >> 5."""
    hits = np.ascontiguousarray(hits)
    return np.packbits(hits, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(hits.shape[0], hits.shape[1] // 32)


def band_hits(r2, thresh):
    with np.errstate(invalid="ignore"):
        return np.isfinite(r2) & (r2 > thresh)


def band_margin(r2, thresh):
    """Smallest |r2 - thresh| / thresh over the band pairs that have a value (inf when there is none)."""
    v = r2[np.isfinite(r2)]
    return float(np.min(np.abs(v - thresh)) / thresh) if v.size else np.inf


def _numpy_band_mask(ref, order, band_end, r0=0, r1=None, wpr=None):
    """Band mask in the layout of `jxg_ld_band_mask_p32` from the restatement's predicate (every pair of the band of the rows
    [r0, r1), the band of row i cut at min(band_end[i], i + 1 + 32 wpr) as the kernel cuts it)."""
    r2, _inband, _clean = band_r2(ref, order, band_end, r0, r1, wpr)
    return pack_band_bits(band_hits(r2, ref.thresh))


def band_block_forms(hasmiss, band_end, nrows, r0, r1, wpr, i_block_only=False):
    """The launch arithmetic of `jxg_ld_band_mask_p32` restated: block (y, x) is the 32 rows from i0 = r0 + 32 y against the 32
    rows from j0 = i0 + 32 x, x <= wpr; it is computed when j0 < nrows and j0 < max band_end over the i-block's rows < r1, in
    the six-sum form when any row of the i-block (< r1) or of the j-block (< nrows) has a missing call, else in the clean form.
    -> int8 (i-blocks, wpr + 1): -1 not computed, 0 clean, 1 six.  `i_block_only`: what a launch that looked at the i-block
    alone would decide (for counting the pairs that depend on the j-block's part)."""
    hasmiss, band_end = np.asarray(hasmiss, dtype=bool), np.asarray(band_end, dtype=np.int64)
    ny = (max(r1 - r0, 0) + 31) // 32
    forms = np.full((ny, wpr + 1), -1, dtype=np.int8)
    for y in range(ny):
        i0 = r0 + 32 * y
        i1 = min(i0 + 32, r1)
        be = int(band_end[i0:i1].max())
        mi = bool(hasmiss[i0:i1].any())
        for x in range(wpr + 1):
            j0 = i0 + 32 * x
            if j0 >= nrows or j0 >= be:
                continue
            forms[y, x] = 1 if (mi or (not i_block_only and bool(hasmiss[j0:min(j0 + 32, nrows)].any()))) else 0
    return forms


def band_pair_forms(forms, r0, rows, wpr):
    """Form of the block that owns each pair of a (rows, 32 wpr) band layout."""
    i = r0 + np.arange(rows, dtype=np.int64)[:, None]
    j = i + 1 + np.arange(32 * wpr, dtype=np.int64)[None, :]
    y = (i - r0) // 32
    x = (j - (r0 + 32 * y)) // 32
    return forms[y, np.minimum(x, forms.shape[1] - 1)]


def band_form_meetings(hits, clean, pair_form):
    """-> (mask words that receive set bits from a clean-form block and from a six-form block, set bits of complete pairs (clean
    formula) inside six-form blocks, set bits by formula)."""
    rows, w = hits.shape
    by_word = lambda sel: (hits & sel).reshape(rows, w // 32, 32).any(axis=2)   # noqa: E731
    both = by_word(pair_form == 0) & by_word(pair_form == 1)
    return int(both.sum()), int((hits & clean & (pair_form == 1)).sum()), {"clean": int((hits & clean).sum()),
                                                                            "pairwise": int((hits & ~clean).sum())}


def describe_band_diff(got, want, r2, clean, r0, pair_form=None):
    """Text for a failed mask comparison: the first differing pair, its block, the formula and the restatement's r^2."""
    diff = np.asarray(got, dtype=np.uint32) ^ np.asarray(want, dtype=np.uint32)
    if got.shape != want.shape:
        return f"mask shapes differ: {got.shape} vs {want.shape}"
    if not diff.any():
        return "masks equal"
    row, word = [int(k[0]) for k in np.nonzero(diff)]
    bit = int(diff[row, word])
    o = 32 * word + ((bit & -bit).bit_length() - 1)
    i, j = r0 + row, r0 + row + 1 + o
    y = row // 32
    x = (j - (r0 + 32 * y)) // 32
    form = "" if pair_form is None else f", block form {('none', 'clean', 'six')[int(pair_form[row, o]) + 1]}"
    return (f"{int(np.count_nonzero(np.unpackbits(diff.view(np.uint8))))} bits differ; first at pair (i={i}, j={j}), mask row {row} "
            f"word {word} bit {o & 31}, block (y={y}, x={x}){form}, device bit {(int(got[row, word]) >> (o & 31)) & 1}, restatement "
            f"formula {'clean' if clean[row, o] else 'pairwise'}, restatement r2 {r2[row, o]!r}")


# one row; longer than 32 rows; across the 32-row boundary 1504; the second half of an LD block, from a boundary, 40 % missing
SPARSE_STRETCHES = ((777, 778, 0.03), (1030, 1070, 0.03), (1500, 1530, 0.03), (2048, 2052, 0.4))


def sparse_missing_panel(m, seed=13):
    """`ld_panel(601, m)` without missing calls, then missing calls on the rows of SPARSE_STRETCHES only: blocks of both launch
    forms lie side by side and share mask words.  The panel's LD blocks of 8 rows are moved by 4 rows, so that they straddle the
    32-row block boundaries (rows 1020 - 1027 are one of them: a clean block, then one with the row 1030).  Rows 2044 - 2047 are
    complete and in a block without a missing call; their LD partners 2048 - 2051 lack 40 % of their calls, so the block pair
    is of the six-sum form through its j-block alone and the clean formula would be far off for these pairs."""
    g, pos = ld_panel(601, m + 4, seed)
    g, pos = g[4:].copy(), pos[4:].copy()
    rng = np.random.default_rng(seed + 1)
    for a, b, rate in SPARSE_STRETCHES:
        hole = rng.random((b - a, g.shape[1])) < rate
        hole[:, 0] = True                                     # every row of a stretch has at least one
        sub = g[a:b]
        sub[hole] = -9
    return g, pos


def valueless_panel(m=1003):
    """Rows whose pairs have no r^2 or an extreme one, inside any band of a few rows: every call missing, one and two calls,
    monomorphic rows (complete: 0 and 2; with missing calls), identical neighbours and a complement (2 - g), each among complete
    rows and among rows with missing calls.  -> (g, positions, {kind: rows})."""
    g, pos = ld_panel(601, 4000, 11, True)
    g, pos = g[:m].copy(), pos[:m].copy()
    full = np.nonzero((g >= 0).all(axis=1))[0]
    holed = np.nonzero((g < 0).any(axis=1))[0]
    c = int(full[(full > 400) & (full < 600)][0])
    h = int(holed[(holed > 600) & (holed < 800)][0])
    g[100] = -9
    g[101] = -9
    g[101, :2] = [1, 2]
    g[102] = -9
    g[102, 5] = 1
    g[200] = 0
    g[201] = np.where(g[201] >= 0, 2, -9)
    g[201, 7] = -9
    g[202] = 2
    g[c + 1] = g[c]
    g[c + 2] = 2 - g[c]
    g[h + 1] = g[h]
    g[h + 2] = np.where(g[h] >= 0, 2 - g[h], -9)
    kinds = dict(all_missing=[100], few_calls=[101, 102], mono_complete=[200, 202], mono_missing=[201],
                 twins_complete=[c, c + 1, c + 2], twins_missing=[h, h + 1, h + 2])
    return g, pos, kinds


def band_value_kinds(ref, order, r2, inband, clean):
    """Counts of the band pairs by what the restatement made of them."""
    order = np.asarray(order, dtype=np.int64)
    rows, w = r2.shape
    i = np.arange(rows, dtype=np.int64)[:, None] + np.zeros((1, w), dtype=np.int64)
    j = np.minimum(i + 1 + np.arange(w, dtype=np.int64)[None, :], len(order) - 1)
    gi, gj = order[i[inband]], order[j[inband]]
    v, cl = r2[inband], clean[inband]
    st = ref.st
    nn = np.minimum(st["non_missing"][gi], st["non_missing"][gj])           # N <= min of the two rows' called calls
    tiny = (st["std"][gi] == 1e-6) | (st["std"][gj] == 1e-6)
    with np.errstate(invalid="ignore"):
        return dict(pairs=int(v.size), nan=int(np.isnan(v).sum()), n_le_1=int((~cl & (nn <= 1) & np.isnan(v)).sum()),
                    zero_variance=int((~cl & (nn > 1) & np.isnan(v)).sum()), std_floor=int((cl & tiny).sum()),
                    r2_one=int((np.abs(v - 1.0) <= 1e-12).sum()), r2_one_clean=int((cl & (np.abs(v - 1.0) <= 1e-12)).sum()))


def _host_prune(g, chrom_codes, positions, window_bp, window_variants, step, r2, split=None):
    ref = LdRef(g, r2)
    order, off, win_end, band_end = jx._ld_window_ends(chrom_codes, positions, window_bp, window_variants, step)
    m = len(order)
    mask = _numpy_band_mask(ref, order, band_end)
    first_unchecked = np.arange(1, m + 1, dtype=np.int64)
    dropped = np.zeros(m, dtype=np.uint8)
    maf = np.ascontiguousarray(ref.st["maf"][order])
    if split is None:
        jx._ld_prune_greedy(maf, off, win_end, 0, m, mask, 0, m, first_unchecked, dropped)
    else:                                                 # range by range, as the device path runs it
        budget = split * 4 * mask.shape[1]
        for a, ws1, r1, _wpr in jx._ld_ranges(win_end, band_end, budget):
            jx._ld_prune_greedy(maf, off, win_end, a, ws1, mask[a:r1], a, r1, first_unchecked, dropped)
    keep = np.ones(m, dtype=bool)
    keep[order] = dropped == 0
    return keep


@pytest.fixture(scope="module")
def panels():
    out = {}
    for name, (n, missing) in PANELS.items():
        g, pos = ld_panel(n, 1200, 11 if missing else 7, missing)
        out[name] = (g, pos, np.zeros(g.shape[0], dtype=np.int32))
    return out


@pytest.mark.parametrize("panel", ["complete", "missing"])
@pytest.mark.parametrize("window", [(None, 50), (50000, None)])
@pytest.mark.parametrize("step", [1, 5, 10])
def test_greedy_equals_restatement(panels, panel, window, step):
    g, pos, chrom = panels[panel]
    want, ref = ref_prune_panel(g, chrom, pos, window[0], window[1], step, 0.2)
    check_ref_conditions(want, ref)
    assert ref.hits["clean"] > 0 and (panel == "complete" or ref.hits["pairwise"] > 0)
    got = _host_prune(g, chrom, pos, window[0], window[1], step, 0.2)
    assert np.array_equal(got, want)


def test_greedy_range_by_range(panels):
    g, pos, chrom = panels["missing"]
    want, _ = ref_prune_panel(g, chrom, pos, None, 50, 5, 0.2)
    for rows in (64, 200, 333):
        assert np.array_equal(_host_prune(g, chrom, pos, None, 50, 5, 0.2, split=rows), want)


def test_greedy_r2_one_prunes_nothing(panels):
    g, pos, chrom = panels["missing"]
    want, _ = ref_prune_panel(g, chrom, pos, None, 50, 5, 1.0)
    assert want.all()
    assert _host_prune(g, chrom, pos, None, 50, 5, 1.0).all()


def test_greedy_interleaved_chromosomes(panels):
    g, pos, _ = panels["missing"]
    g, pos = g[:800], pos[:800]
    chrom = (np.arange(800) % 2).astype(np.int32) * 7 + 3           # rows of two codes alternating
    for window in ((None, 30), (40000, None)):
        want, ref = ref_prune_panel(g, chrom, pos, window[0], window[1], 3, 0.2)
        assert 0 < (~want).sum() < 800
        assert np.array_equal(_host_prune(g, chrom, pos, window[0], window[1], 3, 0.2), want)


def test_greedy_unsorted_positions_and_small_chromosomes(panels):
    g, pos, _ = panels["complete"]
    g, pos = g[:600], pos[:600].copy()
    rng = np.random.default_rng(5)
    chrom = np.zeros(600, dtype=np.int32)
    chrom[300:301] = 1                                               # a one-row chromosome
    chrom[301:] = 2
    pos[301:] = pos[301:][rng.permutation(299)]                      # a chromosome with unsorted positions
    pos[40:48] = pos[40]                                             # ties
    for window in ((20000, None), (None, 25)):
        want, ref = ref_prune_panel(g, chrom, pos, window[0], window[1], 2, 0.2)
        assert want[300] and 0 < (~want).sum() < 600
        assert np.array_equal(_host_prune(g, chrom, pos, window[0], window[1], 2, 0.2), want)
    # no rows at all, and chromosomes of one row only
    order, off, win_end, band_end = jx._ld_window_ends(np.zeros(0, np.int32), np.zeros(0, np.int64), None, 5, 1)
    assert len(order) == 0 and len(off) == 1 and len(win_end) == 0 and len(band_end) == 0
    order, off, win_end, band_end = jx._ld_window_ends(np.array([4, 2, 9], np.int32), np.array([1, 2, 3], np.int64), 100, None, 1)
    assert order.tolist() == [0, 1, 2] and off.tolist() == [0, 1, 2, 3] and not win_end.any() and band_end.tolist() == [1, 2, 3]


@pytest.mark.parametrize("window", [(None, 50), (None, 7), (50000, None), (1, None), (10 ** 12, None)])
@pytest.mark.parametrize("step", [1, 5, 10, 80])
def test_window_and_band_ends_equal_restatement(panels, window, step):
    _, pos, _ = panels["complete"]
    rng = np.random.default_rng(3)
    pos = pos.copy()
    chrom = np.repeat(np.array([5, 1, 5, 8], dtype=np.int32), 300)   # code 5 comes back: the groups are not contiguous
    pos[900:] = pos[900:][rng.permutation(300)]                      # group 8 unsorted
    want = _positions_layout(chrom, pos, window[0], window[1], step)
    got = jx._ld_window_ends(chrom, pos, window[0], window[1], step)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_greedy_refuses_a_window_outside_its_mask():
    maf = np.full(8, 0.3)
    off = np.array([0, 8], dtype=np.int64)
    win_end = np.zeros(8, dtype=np.int64)
    win_end[0] = 8
    fu, dr = np.arange(1, 9, dtype=np.int64), np.zeros(8, dtype=np.uint8)
    with pytest.raises(RuntimeError, match="outside the mask rows"):
        jx._ld_prune_greedy(maf, off, win_end, 0, 8, np.zeros((4, 1), np.uint32), 0, 4, fu, dr)
    off2 = np.array([0, 4, 8], dtype=np.int64)
    with pytest.raises(RuntimeError, match="crosses its chromosome group"):
        jx._ld_prune_greedy(maf, off2, win_end, 0, 8, np.zeros((8, 1), np.uint32), 0, 8, fu, dr)


def test_ranges_cover_every_window_once():
    _, pos = ld_panel(8, 3000, 1)
    chrom = np.repeat(np.arange(3, dtype=np.int32), 1000)
    _o, _off, win_end, band_end = jx._ld_window_ends(chrom, pos, 50000, None, 10)
    wpr_all = (int(np.max(band_end - np.arange(3000) - 1)) + 31) // 32
    ranges = jx._ld_ranges(win_end, band_end, 400 * 4 * wpr_all)
    assert len(ranges) > 3
    starts = np.nonzero(win_end)[0]
    seen = []
    for a, ws1, r1, wpr in ranges:
        mine = starts[(starts >= a) & (starts < ws1)]
        assert mine.size and (win_end[mine] <= r1).all() and (r1 - a) * wpr * 4 <= 400 * 4 * wpr_all
        assert 32 * wpr >= int(np.max(band_end[a:r1] - np.arange(a, r1) - 1))
        seen.extend(mine.tolist())
    assert seen == starts.tolist()
    with pytest.raises(RuntimeError, match="longest window"):
        jx._ld_ranges(win_end, band_end, 16 * 4 * wpr_all)


# ---- parsers and argument errors -------------------------------------------------------------------------------------------------

def test_parse_prune_window_and_args():
    assert cli._parse_prune_window("500") == (500, None)
    assert cli._parse_prune_window("500kb") == (None, 500000)
    assert cli._parse_prune_window("100bp") == (None, 100)
    assert cli._parse_prune_window("0.5kb") == (None, 500)
    assert cli._parse_prune_window(" 2KB ") == (None, 2000)
    with pytest.raises(ValueError, match="Use an integer variant count, or add kb/bp suffix for a physical window"):
        cli._parse_prune_window("1.5")
    with pytest.raises(ValueError, match="Invalid prune window: 0"):
        cli._parse_prune_window("0")
    with pytest.raises(ValueError, match=r"Invalid prune window \(kb\): 0kb"):
        cli._parse_prune_window("0kb")
    with pytest.raises(ValueError, match="Empty prune window token"):
        cli._parse_prune_window("  ")
    assert cli._parse_prune_args(None) is None
    assert cli._parse_prune_args(["50", "5", "0.2"]) == (50, None, 5, 0.2)
    assert cli._parse_prune_args(["50kb", "10.0", "1"]) == (None, 50000, 10, 1.0)
    with pytest.raises(ValueError, match=r"--prune step must be > 0, got '0'"):
        cli._parse_prune_args(["50", "0", "0.2"])
    with pytest.raises(ValueError, match=r"--prune r\^2 threshold must be in \(0, 1\], got '0'"):
        cli._parse_prune_args(["50", "5", "0"])
    with pytest.raises(ValueError, match=r"--prune r\^2 threshold must be in \(0, 1\], got '1.0001'"):
        cli._parse_prune_args(["50", "5", "1.0001"])
    with pytest.raises(ValueError, match="Expected 3 values"):
        cli._parse_prune_args(["50", "5"])
    assert cli._prune_chrom_codes(["2", "1", "2", "X", "1"]).tolist() == [0, 1, 0, 2, 1]


def test_gformat_refuses_what_is_not_built(tmp_path):
    for argv, text in ((["gformat", "-bfile", "x", "-fmt", "vcf", "-prune", "50", "5", "0.2"], "-fmt"),
                       (["gformat", "-bfile", "x", "-maf", "0.05", "-prune", "50", "5", "0.2"], "-maf"),
                       (["gformat", "-vcf", "x.vcf", "-prune", "50", "5", "0.2"], "-vcf"),
                       (["gformat", "-bfile", "x"], "-prune WINDOW STEP R2"),
                       (["gformat", "-bfile", "x", "-prune", "1.5", "5", "0.2"], "Invalid prune window"),
                       (["gformat", "-prune", "50", "5", "0.2"], "-bfile")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert text in str(e.value), (argv, e.value)


def test_prune_argument_errors_come_before_any_device_call(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(jx, "_panel", no_device)
    n, m = 10, 6
    pk = np.zeros((m, 3), dtype=np.uint8)
    cc, ps = np.zeros(m, dtype=np.int32), np.arange(m, dtype=np.int64)
    f = jx.bed_packed_ld_prune_maf_priority
    cases = [
        (dict(packed=np.zeros(4, np.uint8)), "packed must be 2D (m, bytes_per_snp)"),
        (dict(n_samples=0), "n_samples must be > 0"),
        (dict(r2_threshold=0.0), "r2_threshold must be finite and in (0, 1]"),
        (dict(r2_threshold=1.5), "r2_threshold must be finite and in (0, 1]"),
        (dict(r2_threshold=float("nan")), "r2_threshold must be finite and in (0, 1]"),
        (dict(step_variants=0), "step_variants must be > 0"),
        (dict(window_variants=None), "provide one of window_bp or window_variants"),
        (dict(window_bp=0), "window_bp must be > 0"),
        (dict(window_variants=0), "window_variants must be > 0"),
        (dict(packed=np.zeros((m, 4), np.uint8)), "packed second dimension mismatch: got 4, expected 3 for n_samples=10"),
        (dict(chrom_codes=cc[:-1]), "chrom_codes length mismatch: got 5, expected 6"),
        (dict(positions=ps[:-2]), "positions length mismatch: got 4, expected 6"),
    ]
    for change, text in cases:
        kw = dict(packed=pk, n_samples=n, chrom_codes=cc, positions=ps, window_variants=5)
        kw.update(change)
        with pytest.raises(RuntimeError) as e:
            f(**kw)
        assert str(e.value) == text, (change, str(e.value))
    # the order of the reference: the threshold is looked at before the shapes
    with pytest.raises(RuntimeError, match="r2_threshold"):
        f(np.zeros((m, 4), np.uint8), n, cc, ps, window_variants=5, r2_threshold=2.0)
    # no rows: an empty mask, no device
    out = f(np.zeros((0, 3), np.uint8), n, np.zeros(0, np.int32), np.zeros(0, np.int64), window_variants=5)
    assert out.dtype == bool and out.shape == (0,)
    # no window of two rows: everything is kept, no device
    assert f(pk, n, np.arange(m, dtype=np.int32), ps, window_variants=5, threads=3).all()


# ---- .bim selection of the LD-block function -------------------------------------------------------------------------------------

def _write_prefix(tmp_path, chroms, positions, n=5):
    m = len(chroms)
    g = np.random.default_rng(0).integers(0, 3, size=(m, n)).astype(np.int8)
    prefix = str(tmp_path / "sel")
    bed.write_bed(prefix, bed.pack_dosage(g), [f"s{i}" for i in range(n)],
                  bed.Bim(list(chroms), [f"rs{i}" for i in range(m)], list(positions), ["A"] * m, ["G"] * m))
    return prefix, g


def test_ldblock_bim_selection(tmp_path):
    chroms = ["1", "1", "chr1", "2", "Chr2", "2", "1"]
    positions = [100, 200, 300, 150, 250, 350, 900]
    prefix, _ = _write_prefix(tmp_path, chroms, positions)
    total, idx, ch, ps = jx._ld_select_bim(prefix, ["chr1"], [150], [950])                 # `chr` prefix on either side
    assert (total, idx, ch, ps) == (7, [1, 2, 6], ["1", "1", "1"], [200, 300, 900])
    assert jx._ld_select_bim(prefix + ".bed", ["2"], [350], [200])[1] == [4, 5]             # reversed range, inclusive ends
    assert jx._ld_select_bim(prefix, ["1", "2"], [0, 0], [1000, 1000], ["CHR1", "2", "3"], [300, 150, 100])[1] == [2, 3]
    assert jx._ld_select_bim(prefix, ["1", "1"], [100, 850], [100, 900])[1] == [0, 6]       # two ranges of one chromosome
    assert jx._ld_select_bim(prefix, ["7"], [0], [1000])[1] == []
    r2, ch, ps = jx.bed_ldblock_r2_rust(prefix, ["7"], [0], [1000])                         # empty: no device
    assert r2.shape == (0, 0) and r2.dtype == np.float32 and ch == [] and ps == []
    for args, text in ((([], [], []), "bimrange list must not be empty"),
                       ((["1"], [1, 2], [3]), "bimrange length mismatch: chrom_ranges=1, start_bp=2, end_bp=1"),
                       ((["1"], [-1], [3]), "bimrange[0] start/end must be >= 0, got (-1, 3)")):
        with pytest.raises(RuntimeError) as e:
            jx._ld_select_bim(prefix, *args)
        assert str(e.value) == text
    with pytest.raises(RuntimeError, match="selected_chrom and selected_pos must be provided together"):
        jx.bed_ldblock_r2_rust(prefix, ["1"], [0], [10], selected_chrom=["1"])
    with pytest.raises(RuntimeError, match="selected_chrom/selected_pos length mismatch: 1 vs 2"):
        jx.bed_ldblock_r2_rust(prefix, ["1"], [0], [10], selected_chrom=["1"], selected_pos=[1, 2])
    with pytest.raises(RuntimeError, match="bfile must not be empty"):
        jx.bed_ldblock_r2_rust("  ", ["1"], [0], [10])
    with pytest.raises(RuntimeError, match=r"nowhere\.bim"):
        jx.bed_ldblock_r2_rust(os.path.join(str(tmp_path), "nowhere"), ["1"], [0], [10])


def test_row_stats_equal_restatement():
    g, _ = ld_panel(37, 64, 2, missing=True)
    g[5] = -9                                                         # every call missing
    g[6] = 2                                                          # monomorphic
    v = g >= 0
    counts = np.stack([(~v).sum(1), (g == 1).sum(1), (g == 2).sum(1)], axis=1).astype(np.int32)
    mean, std, maf, has = jx._ld_row_stats(counts, 37)
    st = ref_row_stats(g)
    assert np.array_equal(mean, st["mean"]) and np.array_equal(std, st["std"]) and np.array_equal(maf, st["maf"])
    assert np.array_equal(has, st["has_missing"])
    assert (mean[5], std[5], maf[5], has[5]) == (0.0, 1e-6, 0.0, True) and std[6] == 1e-6 and maf[6] == 0.0


# ---- the vectorised band restatement and the inputs of tests/test_gpu_ld_kernel.py --------------------------------------------------

def _slow_band_mask(ref, order, band_end, wpr):
    """The band mask pair by pair through `LdRef.r2_block`, one row at a time (what `_numpy_band_mask` was before it was
    vectorised)."""
    m = len(order)
    mask = np.zeros((m, wpr), dtype=np.uint32)
    for p in range(m):
        be = min(int(band_end[p]), p + 1 + 32 * wpr, m)
        if be > p + 1:
            js = np.arange(p + 1, be)
            r2, _ = ref.r2_block(order[p], order[js])
            for o in np.nonzero(np.isfinite(r2) & (r2 > ref.thresh))[0]:
                mask[p, o >> 5] |= np.uint32(1 << (o & 31))
    return mask


def test_vectorised_band_mask_equals_the_row_by_row_one(panels):
    g, pos, chrom = panels["missing"]
    g = g[:500]
    ref = LdRef(g, 0.2)
    rng = np.random.default_rng(4)
    order = rng.permutation(500)
    idx = np.arange(500)
    band_end = np.minimum(idx + 1 + rng.integers(0, 150, size=500), 500)
    for wpr in (5, 2, 1):
        want = _slow_band_mask(ref, order, band_end, wpr)
        assert 0 < np.count_nonzero(want)
        assert np.array_equal(_numpy_band_mask(ref, order, band_end, wpr=wpr), want)
        assert np.array_equal(_numpy_band_mask(ref, order, band_end, 37, 103, wpr), want[37:103])
    assert _numpy_band_mask(ref, order, band_end, 60, 60, 3).shape == (0, 3)
    assert np.array_equal(ref_six_sums_chunked(g[:40], chunk=128), ref_six_sums(g, np.arange(40), np.arange(40)))


def test_sparse_missing_panel_makes_the_two_launch_forms_meet():
    """On the sparse-missing panel, under the production bands, mask words receive set bits from a clean-form block and from a
    six-form block, and six-form blocks hold complete pairs (clean formula) with set bits."""
    m = 2200
    g, pos = sparse_missing_panel(m)
    chrom = np.zeros(m, dtype=np.int32)
    st = ref_row_stats(g)
    assert st["has_missing"].sum() == sum(b - a for a, b, _ in SPARSE_STRETCHES)
    all_clean = dict(st, has_missing=np.zeros(m, dtype=bool))
    for wbp, wv, step, thr in PARAM_SETS:
        order, _off, _win_end, band_end = jx._ld_window_ends(chrom, pos, wbp, wv, step)
        ref = LdRef(g, thr)
        r2, inband, clean = band_r2(ref, order, band_end)
        wpr = r2.shape[1] // 32
        forms = band_block_forms(st["has_missing"][order], band_end, m, 0, m, wpr)
        assert (forms == 0).any() and (forms == 1).any()
        pf = band_pair_forms(forms, 0, m, wpr)
        assert (pf[inband] >= 0).all()                                # every band pair lies in a block that is computed
        hits = band_hits(r2, ref.thresh)
        both, complete_in_six, by_formula = band_form_meetings(hits, clean, pf)
        print(f"sparse panel {(wbp, wv, step, thr)}: {both} mask words fed by both forms, {complete_in_six} set bits of complete "
              f"pairs in six-form blocks, set bits by formula {by_formula}, margin {band_margin(r2, ref.thresh):.3e}")
        assert both > 0 and complete_in_six > 0
        assert by_formula["clean"] > 0 and by_formula["pairwise"] > 0
        assert band_margin(r2, ref.thresh) > 1e-9
        # pairs whose block is of the six-sum form through its j-block alone, and whose bit the clean formula would get wrong
        i_only = band_pair_forms(band_block_forms(st["has_missing"][order], band_end, m, 0, m, wpr, i_block_only=True), 0, m, wpr)
        wrong = band_hits(band_r2(LdRef(g, thr, st=all_clean), order, band_end)[0], ref.thresh) != hits
        print(f"  {int(((pf == 1) & (i_only == 0) & inband).sum())} band pairs are six-form through the j-block alone, "
              f"{int(((pf == 1) & (i_only == 0) & wrong).sum())} of them with a bit the clean formula gets wrong")
        assert ((pf == 1) & (i_only == 0) & wrong).sum() > 0


def test_valueless_panel_holds_every_kind_of_pair():
    g, pos, kinds = valueless_panel()
    m = g.shape[0]
    order, _off, _win_end, band_end = jx._ld_window_ends(np.zeros(m, dtype=np.int32), pos, None, 50, 5)
    ref = LdRef(g, 0.2)
    r2, inband, clean = band_r2(ref, order, band_end)
    k = band_value_kinds(ref, order, r2, inband, clean)
    print(f"valueless panel: {k}, margin {band_margin(r2, ref.thresh):.3e}")
    assert k["nan"] > 0 and k["n_le_1"] > 0 and k["zero_variance"] > 0 and k["std_floor"] > 0
    assert k["r2_one"] >= 4 and k["r2_one_clean"] >= 2               # identical and complement, complete and with missing calls
    assert band_margin(r2, ref.thresh) > 1e-9


def test_ld_entry_points_refuse_before_they_touch_the_device():
    """Every refusal returns 1 with its message.  The buffers are host arrays of the size the arguments claim: a refusal comes
    before the first device call, so nothing reads them."""
    from janusx_amd._lib import lib
    L = lib()
    p = lambda a: a.ctypes.data                                      # noqa: E731

    def band(m_total, n, nrows, r0, r1, wpr, tiles=None, mask_words=None):
        tiles = L.jxg_num_tiles(max(n, 1)) if tiles is None else tiles
        p32 = np.full((tiles, m_total, 32), 0x55, dtype=np.uint8)
        be = np.arange(1, nrows + 1, dtype=np.int32)
        mean, sd, hm = np.zeros(nrows), np.ones(nrows), np.zeros(nrows, dtype=np.uint8)
        mask = np.zeros(max(1, (max(r1 - r0, 0) * max(wpr, 0)) if mask_words is None else mask_words), dtype=np.uint32)
        st = L.jxg_ld_band_mask_p32(p(p32), m_total, n, None, nrows, r0, r1, p(be), p(mean), p(sd), p(hm), 0.2, wpr, p(mask), None)
        assert not mask.any()
        return st, L.jx_last_error().decode()

    def sums(m_total, n, nrows, i0, i1, j0, j1):
        p32 = np.full((L.jxg_num_tiles(max(n, 1)), m_total, 32), 0x55, dtype=np.uint8)
        out = np.zeros(6 * max(i1 - i0, 1) * max(j1 - j0, 1), dtype=np.int32)
        st = L.jxg_ld_sums_p32(p(p32), m_total, n, None, nrows, i0, i1, j0, j1, p(out), None)
        assert not out.any()
        return st, L.jx_last_error().decode()

    too_many = (1 << 24) + 1
    for n in (0, -5):
        assert band(4, n, 4, 0, 4, 1) == (1, "jxg_ld_band_mask_p32: n must be > 0")
        assert sums(4, n, 4, 0, 4, 0, 4) == (1, "jxg_ld_sums_p32: n must be > 0")
    st, msg = band(2, too_many, 2, 0, 2, 1)
    assert st == 1 and msg.startswith("jxg_ld_band_mask_p32: at most 16 777 216 samples")
    st, msg = sums(2, too_many, 2, 0, 2, 0, 2)
    assert st == 1 and msg.startswith("jxg_ld_sums_p32: at most 16 777 216 samples")
    for r0, r1 in ((-1, 3), (3, 2), (0, 5), (5, 5)):
        assert band(4, 100, 4, r0, r1, 1) == (1, "jxg_ld_band_mask_p32: row range outside the row list"), (r0, r1)
    for blk in ((-1, 2, 0, 2), (0, 5, 0, 2), (2, 1, 0, 2), (0, 2, -1, 2), (0, 2, 0, 5), (0, 2, 3, 2)):
        assert sums(4, 100, 4, *blk) == (1, "jxg_ld_sums_p32: block outside the row list"), blk
    for wpr in (0, -1, too_many):
        assert band(4, 100, 4, 0, 1, wpr) == (1, "jxg_ld_band_mask_p32: words per mask row must be in [1, 2^24]"), wpr
    assert band(4, 100, 0, 0, 0, 1)[0] == 1 and sums(4, 100, 0, 0, 0, 0, 0)[0] == 1      # no rows
    # empty ranges inside the list: nothing to do, no device call
    assert band(4, 100, 4, 2, 2, 1)[0] == 0
    assert sums(4, 100, 4, 1, 1, 0, 4)[0] == 0 and sums(4, 100, 4, 0, 4, 3, 3)[0] == 0
