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
    non_missing = v.sum(axis=1).astype(np.int64)
    alt_sum = g0.sum(axis=1)
    sq_sum = (g0 * g0).sum(axis=1)
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
    """D, N, S_i, S_j, Q_i, Q_j (int64, (len(rows_i), len(rows_j))) of row pairs."""
    g = np.asarray(g)
    vi, vj = (g[rows_i] >= 0).astype(np.int64), (g[rows_j] >= 0).astype(np.int64)
    gi, gj = np.where(vi > 0, g[rows_i], 0).astype(np.int64), np.where(vj > 0, g[rows_j], 0).astype(np.int64)
    return np.stack([gi @ gj.T, vi @ vj.T, gi @ vj.T, vi @ gj.T, (gi * gi) @ vj.T, vi @ (gj * gj).T])


class LdRef:
    """The pair predicate "in LD" of the reference (src/stats/ld.rs:339-368) with its two formulas, asked lazily."""

    def __init__(self, g, r2_threshold):
        self.g = np.asarray(g)
        self.n = self.g.shape[1]
        self.st = ref_row_stats(self.g)
        self.thresh = float(r2_threshold) * (1.0 + 1e-12)
        self.hits = {"clean": 0, "pairwise": 0}           # pairs in LD the greedy met, by the formula that decided them
        self.asked = 0
        self.min_margin = np.inf                          # smallest |r2 - thresh| / thresh over the pairs the greedy asked for
        self._cache = {}

    def r2_block(self, gi, gjs):
        """r^2 of row gi against the rows gjs (NaN where the reference has no value), and which pairs took the clean formula."""
        st, n = self.st, self.n
        s = ref_six_sums(self.g, [gi], gjs)[:, 0, :].astype(np.float64)
        d, nn, si, sj, si2, sj2 = s
        denom = float(max(n - 1, 1))
        cov = d - float(n) * st["mean"][gi] * st["mean"][gjs]
        denom_corr = denom * st["std"][gi] * st["std"][gjs]
        with np.errstate(divide="ignore", invalid="ignore"):
            corr = np.where(denom_corr > 0.0, cov / denom_corr, 0.0)
            clean = corr * corr
            cov_num = d * nn - si * sj
            var_i = si2 * nn - si * si
            var_j = sj2 * nn - sj * sj
            den = var_i * var_j
            pw = (cov_num * cov_num) / den
        pw = np.where((nn > 1) & np.isfinite(den) & (den > 0.0) & np.isfinite(cov_num), pw, np.nan)
        is_clean = ~st["has_missing"][gi] & ~st["has_missing"][gjs]
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


def _numpy_band_mask(ref, order, band_end):
    """Band mask in the layout of `jxg_ld_band_mask_p32` from the restatement's predicate (every pair of the band)."""
    m = len(order)
    width = int(np.max(band_end - np.arange(m) - 1)) if m else 0
    wpr = max(1, (width + 31) // 32)
    mask = np.zeros((m, wpr), dtype=np.uint32)
    for p in range(m):
        if band_end[p] > p + 1:
            js = np.arange(p + 1, band_end[p])
            r2, _ = ref.r2_block(order[p], order[js])
            for o in np.nonzero(np.isfinite(r2) & (r2 > ref.thresh))[0]:
                mask[p, o >> 5] |= np.uint32(1 << (o & 31))
    return mask


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
