"""Host tests of `jx gstats` (site / sample statistics and LD scores), no GPU: the windows of the host layer
(`jx_ldsc_window_bounds`) against a numpy restatement of the reference, the window parsers, and the refusals of the mirror functions
and of the command line that come before any device call.

The restatement below is the one `tests/test_gpu_gstats.py` compares the device results with.  Nothing of the reference pins
gstats, so it is pinned by reading (file:line in the docstrings) and guarded independently: on a complete panel the restated LD
score must equal the sum of `np.corrcoef`^2 over the same windows, and on a panel with missing calls sampled pairs must equal
`np.corrcoef` on their jointly called samples."""
import os

import numpy as np
import pytest

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx

from test_ld_host import PANELS, LdRef, ld_panel, ref_groups   # noqa: E402

M = 1003                                                      # not a multiple of the 32-row block


# ---- restatement -----------------------------------------------------------------------------------------------------------------

def ref_window_bounds(chrom_codes, positions, cm_positions, kind, w):
    """`build_sorted_chrom_groups` (src/stats/gstats.rs:873-896) and `compute_window_bounds` (:898-953), literally: all rows of a
    code form one group, stably sorted by position (cM window: by cM, then position); the two-pointer loops with their one-sided
    comparisons and `w + 1e-12` for cM.  Groups in order of first appearance (the reference's order is a hash map's and decides
    nothing).  -> (order, group offsets, start, end) with start / end in positions of the whole order."""
    positions = [int(p) for p in positions]
    cms = None if cm_positions is None else [float(c) for c in cm_positions]
    order, off, starts, ends = [], [0], [], []
    for group in ref_groups(chrom_codes):
        if kind == "cm":
            group = sorted(group, key=lambda a: (cms[a], positions[a]))       # Python's sort is stable, as Rust's sort_by
        else:
            group = sorted(group, key=lambda a: positions[a])
        n, c0 = len(group), len(order)
        st, en = [0] * n, [0] * n
        if kind == "variants":
            for i in range(n):
                st[i] = max(i - w, 0)
                en[i] = min(n, i + w + 1)
        elif kind == "bp":
            left = right = 0
            for i in range(n):
                pos_i = positions[group[i]]
                while left < i and pos_i - positions[group[left]] > w:
                    left += 1
                if right < i:
                    right = i
                while right + 1 < n and positions[group[right + 1]] - pos_i <= w:
                    right += 1
                st[i], en[i] = left, right + 1
        else:
            eps = 1e-12
            left = right = 0
            for i in range(n):
                cm_i = cms[group[i]]
                while left < i and (cm_i - cms[group[left]]) > w + eps:
                    left += 1
                if right < i:
                    right = i
                while right + 1 < n and (cms[group[right + 1]] - cm_i) <= w + eps:
                    right += 1
                st[i], en[i] = left, right + 1
        order += group
        off.append(len(order))
        starts += [c0 + v for v in st]
        ends += [c0 + v for v in en]
    as64 = lambda a: np.asarray(a, dtype=np.int64)   # noqa: E731
    return as64(order), as64(off), as64(starts), as64(ends)


def ref_pair_values(ref, gis, gjs):
    """The value a pair adds to the LD score of its row i (src/stats/gstats.rs:956-1000, 1063-1100), each from i's side: the clean
    formula (0 without a positive denominator or with a non-finite covariance) or the pairwise-complete one ("no value" -> 0),
    clamped to [0, 1]; a non-finite value adds nothing (0 here)."""
    r2, _clean = ref.r2_rect(gis, gjs)                        # NaN where the reference has no value or a non-finite one
    return np.clip(np.where(np.isfinite(r2), r2, 0.0), 0.0, 1.0)


def ref_ldscore(g, chrom_codes, positions, cm_positions, kind, w, ref=None):
    """`compute_ldscore_core`, src/stats/gstats.rs:1002-1171 -> (M int64, ldsc f64): per row the window size and self term (1 iff
    non_missing > 1 and maf > 0) + the pair values of the other rows of its window, added one after the other in window order."""
    ref = LdRef(g, 1.0) if ref is None else ref
    st = ref.st
    order, _off, start, end = ref_window_bounds(chrom_codes, positions, cm_positions, kind, w)
    m = len(order)
    m_counts, ldsc = np.zeros(m, dtype=np.int64), np.zeros(m)
    for b0 in range(0, m, 64):
        b1 = min(m, b0 + 64)
        lo, hi = int(start[b0:b1].min()), int(end[b0:b1].max())
        vals = ref_pair_values(ref, order[b0:b1], order[lo:hi])
        for p in range(b0, b1):
            gi = int(order[p])
            row = vals[p - b0, start[p] - lo:end[p] - lo].copy()
            row[p - start[p]] = 0.0                           # `continue` at the row itself
            self_term = 1.0 if st["non_missing"][gi] > 1 and st["maf"][gi] > 0.0 else 0.0
            ldsc[gi] = np.cumsum(np.concatenate([[self_term], row]))[-1]       # sequential, as the reference's loop
            m_counts[gi] = end[p] - start[p]
    return m_counts, ldsc


def ref_site_rates(g):
    """`packed_site_rates`, src/stats/gstats.rs:158-177, in f32 scalars -> (maf, miss, het) f32 (m)."""
    g = np.asarray(g)
    m, n = g.shape
    out = np.zeros((3, m), dtype=np.float32)
    f = np.float32
    for i in range(m):
        missing, het_count, hom_alt = int((g[i] < 0).sum()), int((g[i] == 1).sum()), int((g[i] == 2).sum())
        non_missing = n - missing
        out[1, i] = f(missing) / f(n)
        if non_missing == 0:
            continue
        p_alt = f(het_count + 2 * hom_alt) / (f(2.0) * f(non_missing))
        out[0, i] = min(p_alt, f(1.0) - p_alt)
        out[2, i] = f(het_count) / f(non_missing)
    return out[0], out[1], out[2]


def ref_sample_counts(g):
    """`accumulate_individual_row_counts`, src/stats/gstats.rs:180-220 -> (2, n) int64: rows with a missing call, with a het call."""
    g = np.asarray(g)
    return np.stack([(g < 0).sum(axis=0), (g == 1).sum(axis=0)]).astype(np.int64)


def ref_sample_rates(g):
    """`finalize_individual_rates`, src/stats/gstats.rs:222-245, in f32 scalars -> (miss, het) f32 (n)."""
    m = np.asarray(g).shape[0]
    miss_ct, het_ct = ref_sample_counts(g)
    f = np.float32
    miss = np.array([f(c) / f(m) for c in miss_ct], dtype=np.float32)
    het = np.array([f(h) / f(m - c) if m - c > 0 else f(0.0) for c, h in zip(miss_ct, het_ct)], dtype=np.float32)
    return miss, het


def render_table(header, leads, name, values):
    """A gstats text table (python/janusx/script/gstats.py:183-304): header line, then the lead columns and the value as `%.6f`."""
    return f"{header}\t{name}\n" + "".join(f"{a}\t{b}\t{float(v):.6f}\n" for (a, b), v in zip(leads, values))


def gstats_panel(name):
    """The LD panels of `test_ld_host.PANELS` at m = 1003 -> (dosage (m, n) int8, positions, cM = position / 1e5)."""
    n, missing = PANELS[name]
    g, pos = ld_panel(n, M, 11 if missing else 7, missing)
    return g, pos, pos / 1.0e5


# ---- the restatement's guard -------------------------------------------------------------------------------------------------------

def test_restatement_is_corrcoef_on_the_complete_panel():
    g, pos, cm = gstats_panel("complete")
    m = g.shape[0]
    assert (g >= 0).all() and (g.std(axis=1) > 0).all()
    c2 = np.corrcoef(g.astype(np.float64)) ** 2
    ref = LdRef(g, 1.0)
    chrom = np.zeros(m, dtype=np.int32)
    for kind, w in (("variants", 1), ("variants", 32), ("bp", 50000), ("cm", 0.5), ("variants", 2000)):
        order, _off, start, end = ref_window_bounds(chrom, pos, cm, kind, w)
        assert np.array_equal(order, np.arange(m))            # positions ascend
        want = np.array([c2[i, start[i]:end[i]].sum() for i in range(m)])
        m_counts, got = ref_ldscore(g, chrom, pos, cm, kind, w, ref)
        assert np.array_equal(m_counts, end - start)
        err = float(np.max(np.abs(got - want)))
        print(f"complete panel {kind} {w}: mean score {got.mean():.3f}, max |restated - corrcoef^2 sum| {err:.2e}")
        assert err <= 1e-9


def test_restatement_is_corrcoef_of_the_called_samples_on_the_missing_panel():
    g, _pos, _cm = gstats_panel("missing")
    m = g.shape[0]
    ref = LdRef(g, 1.0)
    rng = np.random.default_rng(5)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, m, size=(200, 2)) if a != b]
    pairs += [(i, i + 1) for i in range(0, 2 * (200 - len(pairs)), 2)]
    assert len(pairs) == 200
    seen = {"clean": 0, "pairwise": 0}
    for i, j in pairs:
        got = float(ref_pair_values(ref, [i], [j])[0, 0])
        both = (g[i] >= 0) & (g[j] >= 0)
        want = float(np.corrcoef(g[i, both].astype(np.float64), g[j, both].astype(np.float64))[0, 1] ** 2)
        seen["pairwise" if ref.st["has_missing"][i] or ref.st["has_missing"][j] else "clean"] += 1
        assert abs(got - want) <= 1e-9, (i, j, got, want)
    assert seen["clean"] > 0 and seen["pairwise"] > 0, seen


# ---- jx_ldsc_window_bounds against the restatement ---------------------------------------------------------------------------------

def _bounds(chrom, pos, cm, kind, w):
    code = {"variants": 0, "bp": 1, "cm": 2}[kind]
    return jx._ldsc_window_bounds(chrom, pos, cm, code, 0 if code == 2 else w, w if code == 2 else 0.0)


@pytest.mark.parametrize("kind,windows", [("variants", (1, 3, 40, 5000)), ("bp", (1, 7, 300, 10 ** 7)), ("cm", (0.01, 0.07, 3.0, 1e5))])
def test_window_bounds_equal_the_restatement(kind, windows):
    """Interleaved chromosome codes, positions unsorted inside a chromosome, duplicate positions (stable order), cM ties broken by
    position, a window larger than a group, a window of 1 bp."""
    rng = np.random.default_rng(17)
    for trial in range(6):
        m = int(rng.integers(1, 400))
        chrom = rng.integers(0, 4, size=m).astype(np.int32) * 7 - 3           # interleaved, not consecutive, one negative
        pos = rng.integers(0, 60 if trial % 2 else 3000, size=m).astype(np.int64)     # unsorted; many duplicates on odd trials
        cm = np.round(pos / 400.0, 1)                                             # ties in cM at different positions
        for w in windows:
            got = _bounds(chrom, pos, cm, kind, w)
            want = ref_window_bounds(chrom, pos, cm, kind, w)
            for a, b, what in zip(got, want, ("order", "offsets", "start", "end")):
                assert np.array_equal(a, b), (kind, w, trial, what)
            order, off, start, end = got
            idx = np.arange(m)
            assert (start <= idx).all() and (idx < end).all()
            grp = np.searchsorted(off, idx, side="right") - 1
            assert (start >= off[grp]).all() and (end <= off[grp + 1]).all()  # a window stays in its group
        if kind != "cm":
            big = _bounds(chrom, pos, cm, kind, windows[-1])                      # larger than any group: the whole group
            grp = np.searchsorted(big[1], np.arange(m), side="right") - 1
            assert np.array_equal(big[2], big[1][grp]) and np.array_equal(big[3], big[1][grp + 1])


def test_window_bounds_stable_order_and_ties():
    chrom = np.array([1, 0, 1, 1, 0, 1], dtype=np.int32)
    pos = np.array([50, 9, 50, 10, 9, 50], dtype=np.int64)
    order, off, start, end = _bounds(chrom, pos, None, "bp", 1)
    assert order.tolist() == [3, 0, 2, 5, 1, 4] and off.tolist() == [0, 4, 6]     # duplicates keep their file order
    assert start.tolist() == [0, 1, 1, 1, 4, 4] and end.tolist() == [1, 4, 4, 4, 6, 6]
    cm = np.array([0.5, 0.0, 0.5, 0.5, 0.0, 0.2])
    order, _off, start, end = _bounds(chrom, pos, cm, "cm", 0.3)
    assert order.tolist() == [5, 3, 0, 2, 1, 4]                                   # by cM, ties by position, then file order
    assert start.tolist() == [0, 0, 0, 0, 4, 4] and end.tolist() == [4, 4, 4, 4, 6, 6]
    with pytest.raises(RuntimeError, match="NaN"):
        _bounds(chrom, pos, np.array([0.0, 0.1, np.nan, 0.2, 0.3, 0.4]), "cm", 0.3)
    assert _bounds(chrom, pos, np.array([0.0, 0.1, np.nan, 0.2, 0.3, 0.4]), "bp", 5)[0].shape == (6,)   # unused: not looked at
    with pytest.raises(RuntimeError, match="needs cM positions"):
        _bounds(chrom, pos, None, "cm", 0.3)


def test_ranges_start_at_multiples_of_32_and_respect_the_budget():
    m = 1003
    chrom = np.zeros(m, dtype=np.int32)
    _order, _off, start, end = _bounds(chrom, np.arange(m, dtype=np.int64), None, "variants", 100)
    whole = jx._ldsc_ranges(start, end, jx.LDSC_PARTIAL_BUDGET_BYTES)
    assert whole == [(0, m, 9)]                               # rows 480 .. 511 reach the rows 380 .. 611: blocks 11 .. 19
    cut = jx._ldsc_ranges(start, end, 32 * 9 * 8 * 3)
    assert len(cut) >= 8 and cut[0][0] == 0 and cut[-1][1] == m
    for (a0, a1, npb), (b0, _b1, _n) in zip(cut, cut[1:] + [(m, m, 0)]):
        assert a0 % 32 == 0 and a1 == b0 and (a1 - a0) * npb * 8 <= 32 * 9 * 8 * 3
    with pytest.raises(RuntimeError, match=r"budget of 1000 bytes is below the \d+ bytes"):
        jx._ldsc_ranges(start, end, 1000)


# ---- text: parsers and refusals ----------------------------------------------------------------------------------------------------

def test_cli_window_grammar_and_labels():
    p = cli._parse_ldsc_window
    assert p("100") == ("variants", 100.0, "100snp")
    assert p("100snps") == ("variants", 100.0, "100snp")
    assert p("100kb") == ("bp", 100000.0, "100kb")
    assert p(" 0.1 MB ") == ("bp", 100000.0, "0.1mb")
    assert p("100000b") == ("bp", 100000.0, "100000b")
    assert p("2500bp") == ("bp", 2500.0, "2500b")
    assert p("10cm") == ("cm", 10.0, "10cm")
    assert p("0.5cm") == ("cm", 0.5, "0.5cm")
    assert p(None) == p("") == ("bp", 100000.0, "100kb")
    for text, msg in (("abc", "Invalid -ldsc window: 'abc'. Use forms like 100, 100kb, 0.1mb, 100000b, or 10cm."),
                      ("-5", "Invalid -ldsc window: '-5'."), ("0", "-ldsc window must be > 0, got '0'."),
                      ("1.5", "SNP-count LD-score window must be an integer, got '1.5'."),
                      ("1.5snp", "SNP-count LD-score window must be an integer, got '1.5snp'."),
                      ("10furlongs", "Unsupported -ldsc unit in '10furlongs'.")):
        with pytest.raises(ValueError) as e:
            p(text)
        assert msg in str(e.value)


def test_mirror_window_kinds_and_error_texts():
    p = jx._ldsc_parse_window
    assert p("variants", 100.0) == (0, 100, 0.0) and p(" SNP ", 3) == (0, 3, 0.0) and p("snps", 3.0000000001) == (0, 3, 0.0)
    assert p("bp", 1e5) == (1, 100000, 0.0) and p("kb", 7.0) == (1, 7, 0.0) and p("b", 2.0000004) == (1, 2, 0.0)
    assert p("cm", 0.5) == (2, 0, 0.5) and p("Genetic", 2) == (2, 0, 2.0)
    for kind, value, msg in (("bp", 0.0, "window_value must be finite and > 0, got 0"),
                             ("bp", float("nan"), "window_value must be finite and > 0, got NaN"),
                             ("cm", float("inf"), "window_value must be finite and > 0, got inf"),
                             ("cm", -1.5, "window_value must be finite and > 0, got -1.5"),
                             ("snp", 2.5, "variant-count LD-score window must be an integer, got 2.5"),
                             ("snp", 0.4, "variant-count LD-score window must be an integer, got 0.4"),
                             ("bp", 10.5, "bp LD-score window must resolve to an integer, got 10.5"),
                             ("bp", 0.0000001, "bp LD-score window must be > 0, got 0"),
                             ("miles", 3.0, "window_kind must be one of: variants, bp, cm; got 'miles'")):
        with pytest.raises(RuntimeError) as e:
            p(kind, value)
        assert str(e.value) == msg


def _write_prefix(tmp_path, name, g, chroms, pos, cm):
    """A small PLINK prefix whose `.bim` carries real cM values (`write_bed` writes zeros)."""
    m, n = g.shape
    prefix = str(tmp_path / name)
    bed.write_bed(prefix, bed.pack_dosage(g), [f"id{i}" for i in range(n)],
                  bed.Bim(list(chroms), [f"rs{i}" for i in range(m)], [int(p) for p in pos], ["A"] * m, ["G"] * m))
    with open(prefix + ".bim", "w") as fh:
        for i in range(m):
            fh.write(f"{chroms[i]}\trs{i}\t{float(cm[i])!r}\t{int(pos[i])}\tA\tG\n")
    return prefix


def test_mirror_refusals_come_before_the_device(tmp_path):
    g = (np.arange(40 * 9).reshape(40, 9) % 3).astype(np.int8)
    m, n = g.shape
    packed = bed.pack_dosage(g)
    chrom, pos = np.zeros(m, dtype=np.int32), np.arange(m, dtype=np.int64)
    with pytest.raises(RuntimeError, match="packed must be 2D"):
        jx.ldscore_packed(packed.ravel(), n, chrom, pos)
    with pytest.raises(RuntimeError, match="n_samples must be > 0"):
        jx.ldscore_packed(packed, 0, chrom, pos)
    with pytest.raises(RuntimeError, match="packed second dimension mismatch: got 3, expected 4 for n_samples=13"):
        jx.ldscore_packed(packed, 13, chrom, pos)
    with pytest.raises(RuntimeError, match="chrom_codes length mismatch: got 39, expected 40"):
        jx.ldscore_packed(packed, n, chrom[1:], pos)
    with pytest.raises(RuntimeError, match="positions length mismatch: got 39, expected 40"):
        jx.ldscore_packed(packed, n, chrom, pos[1:])
    with pytest.raises(RuntimeError, match="window_kind must be one of"):
        jx.ldscore_packed(packed, n, chrom, pos, window_kind="miles")
    with pytest.raises(RuntimeError, match="needs cm_positions"):
        jx.ldscore_packed(packed, n, chrom, pos, window_kind="cm", window_value=1.0)
    with pytest.raises(RuntimeError, match="cm_positions length mismatch"):
        jx.ldscore_packed(packed, n, chrom, pos, np.zeros(3), "cm", 1.0)
    with pytest.raises(RuntimeError, match="NaN"):
        jx.ldscore_packed(packed, n, chrom, pos, np.full(m, np.nan), "cm", 1.0)
    with pytest.raises(RuntimeError, match="budget of 64 bytes is below"):
        jx.ldscore_packed(packed, n, chrom, pos, window_kind="snp", window_value=2, partial_budget_bytes=64)
    m0, l0 = jx.ldscore_packed(packed[:0], n, chrom[:0], pos[:0])
    assert m0.shape == (0,) and m0.dtype == np.int64 and l0.shape == (0,) and l0.dtype == np.float64
    # through a prefix
    with pytest.raises(RuntimeError, match="window_kind must be one of"):
        jx.gstats_bed_ldscore(str(tmp_path / "absent"), "miles", 1.0)              # the window is parsed first
    for call in (lambda p: jx.gstats_bed_ldscore(p, "bp", 100.0), jx.gstats_bed_site_stats, jx.gstats_bed_individual_stats,
                 jx.gstats_bed_joint_stats):
        with pytest.raises(RuntimeError, match=r"absent\.fam"):
            call(str(tmp_path / "absent.bed"))
    prefix = _write_prefix(tmp_path, "p", g, ["1"] * m, pos, pos / 10.0)
    good_bim = open(prefix + ".bim").read()
    lines = good_bim.splitlines(keepends=True)
    open(prefix + ".bim", "w").write("".join(lines[:-1]))
    with pytest.raises(RuntimeError, match="BED/BIM row mismatch: bed=40, bim=39"):
        jx.gstats_bed_ldscore(prefix, "bp", 100.0)
    for bad, msg in (("1\trs\t0\n", r"p\.bim:3: malformed BIM row, expect at least 4 columns"),
                     ("1\trs\tx.5\t7\tA\tG\n", r"p\.bim:3: invalid cM value 'x\.5': "),
                     ("1\trs\t0.5\t7.0\tA\tG\n", r"p\.bim:3: invalid BP value '7\.0': ")):
        open(prefix + ".bim", "w").write("".join(lines[:2]) + bad + "".join(lines[3:]))
        with pytest.raises(RuntimeError, match=msg):
            jx.gstats_bed_ldscore(prefix, "bp", 100.0)
    open(prefix + ".bim", "w").write(good_bim.replace("\t0.5\t", "\tnan\t"))
    with pytest.raises(RuntimeError, match="NaN"):
        jx.gstats_bed_ldscore(prefix, "cm", 1.0)
    open(prefix + ".bim", "w").write(good_bim)
    raw = open(prefix + ".bed", "rb").read()
    for payload, msg in ((raw[:2], "BED too small"), (b"\x6c\x1b\x00" + raw[3:], "unsupported BED header"),
                         (raw + b"\x00", r"invalid payload length data_len=121, bytes_per_snp=3"), (raw[:3], "no variant rows found")):
        open(prefix + ".bed", "wb").write(payload)
        with pytest.raises(RuntimeError, match=msg):
            jx.gstats_bed_site_stats(prefix)
    open(prefix + ".fam", "w").write("")
    with pytest.raises(RuntimeError, match="no samples found in PLINK input"):
        jx.gstats_bed_individual_stats(prefix)
    assert not hasattr(jx, "gstats_bed_site_stats_compare")


def test_site_and_sample_rates_equal_the_scalar_restatement():
    g, _pos, _cm = gstats_panel("missing")
    g = g[:200].copy()
    g[3] = -9                                                 # every call missing
    g[4] = 2                                                  # monomorphic
    g[:, 5] = -9                                              # a sample without a call
    n = g.shape[1]
    counts = np.stack([(g < 0).sum(axis=1), (g == 1).sum(axis=1), (g == 2).sum(axis=1)], axis=1)
    for got, want in zip(jx._gstats_site_rates(counts, n), ref_site_rates(g)):
        assert got.dtype == np.float32 and np.array_equal(got, want)
    for got, want in zip(jx._gstats_sample_rates(ref_sample_counts(g), g.shape[0]), ref_sample_rates(g)):
        assert got.dtype == np.float32 and np.array_equal(got, want)


def test_cli_refusals(tmp_path):
    for argv, msg in ((["gstats", "-bfile", "x"], "select at least one statistic: -freq / -miss / -het / -ldsc"),
                      (["gstats", "-freq"], "gstats needs -bfile PREFIX"),
                      (["gstats", "-vcf", "x.vcf", "-freq"], "-vcf input is not supported"),
                      (["gstats", "-hmp", "x.hmp", "-miss"], "-hmp input is not supported"),
                      (["gstats", "-file", "x", "-het"], "-file input is not supported"),
                      (["gstats", "-bfile", "x", "-ldsc", "1.5"], "SNP-count LD-score window must be an integer, got '1.5'."),
                      (["gstats", "-bfile", "x", "-ldsc", "5parsec"], "Unsupported -ldsc unit in '5parsec'."),
                      (["gstats", "-bfile", str(tmp_path / "absent"), "-t", "4", "-ldsc"], "absent.fam")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert msg in str(e.value), (argv, str(e.value))
