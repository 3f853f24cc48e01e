"""Host side of `jx tree -nj` (no GPU): the chunk loader's site filter, the letters, Newick rendering, the distance-matrix
normalisation, every argument error of the mirrors and the command's refusals, against tests/tree_ref.py."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tree_ref as R   # noqa: E402
from janusx_amd import cli, stats   # noqa: E402
from janusx_amd import janusx as jx   # noqa: E402
from janusx_amd import tree as T   # noqa: E402

F32 = np.float32


def _keep_loop(counts, n, maf, geno, het):
    out = [R.row_keep_scalar(int(a), int(b), int(c), n, maf, geno, het) for a, b, c in counts]
    return np.array([k for k, _ in out], dtype=bool), np.array([f for _, f in out], dtype=bool)


def test_site_filter_matches_scalar_loop_on_random_counts():
    rng = np.random.default_rng(11)
    n = 200
    missing = rng.integers(0, 30, 4000)
    het = np.array([rng.integers(0, n - mi + 1) for mi in missing]) // rng.integers(1, 40, 4000)
    hom = np.array([rng.integers(0, n - mi - h + 1) for mi, h in zip(missing, het)])
    counts = np.stack([missing, het, hom], axis=1)
    for maf, geno, het_thr in ((0.02, 0.05, 0.02), (0.0, 1.0, 1.0), (0.05, 0.1, 0.5), (0.5, 0.0, 0.0)):
        keep, flip = stats.chunk_loader_row_keep(counts, n, maf, geno, het_thr)
        rk, rf = _keep_loop(counts, n, maf, geno, het_thr)
        assert np.array_equal(keep, rk)
        assert np.array_equal(flip[keep], rf[keep])
        assert 0 < keep.sum() or maf == 0.5


def test_site_filter_edges():
    n = 100
    rows = {
        "all_missing": (100, 0, 0),
        "monomorphic_ref": (0, 0, 0),
        "monomorphic_alt": (0, 0, 100),
        "miss_at_threshold": (5, 1, 20),           # 1 - 95 / 100 -> f32 0.05 against f32(0.05): equal, kept
        "miss_above": (6, 1, 20),
        "het_at_threshold": (0, 2, 30),            # 2 / 100 = 0.02 in f64 against f64(f32(0.02)) = 0.0199999995...: dropped
        "het_below": (0, 1, 30),
        "maf_at_threshold": (0, 0, 2),             # af = 4 / 200 = 0.02 -> f32 equals f32(0.02): kept
        "maf_below": (0, 1, 0),                    # af = 0.005
        "flip": (0, 0, 98),                        # af 0.98 -> maf 0.02 (f64 1 - 0.98 = 0.020000000000000018 -> f32 0.02): kept, flipped
    }
    counts = np.array(list(rows.values()))
    keep, flip = stats.chunk_loader_row_keep(counts, n, 0.02, 0.05, 0.02)
    got = dict(zip(rows, zip(keep.tolist(), flip.tolist())))
    assert got["all_missing"][0] is False and got["monomorphic_ref"][0] is False and got["monomorphic_alt"][0] is False
    assert got["miss_at_threshold"][0] is True and got["miss_above"][0] is False
    assert got["het_at_threshold"][0] is False and got["het_below"][0] is True
    assert got["maf_at_threshold"] == (True, False) and got["maf_below"][0] is False
    assert got["flip"] == (True, True)
    rk, _ = _keep_loop(counts, n, 0.02, 0.05, 0.02)
    assert np.array_equal(keep, rk)
    # the all-missing row passes only with a zero MAF threshold and a missing-rate threshold of 1
    k0, _ = stats.chunk_loader_row_keep(counts[:1], n, 0.0, 1.0, 0.02)
    k1, _ = stats.chunk_loader_row_keep(counts[:1], n, 1e-9, 1.0, 0.02)
    assert k0.tolist() == [True] and k1.tolist() == [False]
    # the het filter is on below 1.0 and off at 1.0 (not "on above 0" as in packed_prep_row_stats): with a threshold of 0.0 a row
    # with one het call is dropped here and kept there
    one_het = np.array([[0, 1, 30]])
    assert stats.chunk_loader_row_keep(one_het, n, 0.02, 0.05, 0.0)[0].tolist() == [False]
    assert stats.packed_prep_row_stats(one_het, n, 0.02, 0.05, 0.0)[0].tolist() == [True]
    assert stats.chunk_loader_row_keep(np.array([[0, 100, 0]]), n, 0.02, 0.05, 1.0)[0].tolist() == [True]


def test_site_filter_f32_f64_boundaries():
    # missing rate: the f64 value is cast to f32 before the compare: n = 10, seven missing: 1 - 3/10 = 0.7 in f64, above the
    # widened threshold f64(f32(0.7)) = 0.699999988..., but f32(0.7) equals the f32 threshold: kept
    keep, _ = stats.chunk_loader_row_keep(np.array([[7, 0, 1]]), 10, 0.0, 0.7, 1.0)
    assert keep.tolist() == [True] and (1.0 - 3.0 / 10.0) > float(F32(0.7)) and R.row_keep_scalar(7, 0, 1, 10, 0.0, 0.7, 1.0)[0]
    thr = 0.7
    # het rate: f64 against the widened f32 threshold: 1/10 = 0.1 > f64(f32(0.1)) = 0.10000000149 is false: kept; in f32 both are equal too;
    # 3/10 = 0.3 > f64(f32(0.3)) = 0.30000001192 false; 7/10 = 0.7 > f64(f32(0.7)) = 0.69999998808: dropped, an f32 compare would keep
    k = stats.chunk_loader_row_keep(np.array([[0, 1, 4], [0, 3, 3], [0, 7, 1]]), 10, 0.0, 1.0, 0.1)[0]
    assert k.tolist()[0] is True
    k7 = stats.chunk_loader_row_keep(np.array([[0, 7, 1]]), 10, 0.0, 1.0, 0.7)[0]
    assert k7.tolist() == [False] and not (F32(0.7) > F32(0.7))
    # MAF: f64 value cast to f32: af = 1 / 50 = 0.02 -> f32(0.02) == threshold f32(0.02): kept
    assert stats.chunk_loader_row_keep(np.array([[0, 1, 0]]), 25, 0.02, 1.0, 1.0)[0].tolist() == [True]
    for row, n, maf, geno, het in (((7, 0, 1), 10, 0.0, thr, 1.0), ((0, 7, 1), 10, 0.0, 1.0, 0.7), ((0, 1, 0), 25, 0.02, 1.0, 1.0)):
        assert stats.chunk_loader_row_keep(np.array([row]), n, maf, geno, het)[0][0] == R.row_keep_scalar(*row, n, maf, geno, het)[0]


ALLELE_PAIRS = [("A", "G"), ("a", "t"), ("N", "C"), ("A", "N"), ("N", "A"), ("G", "N"), ("*", "*"), ("A", "AT"), ("at", "A"), ("*", "A"),
                ("C", "*"), (" g", "\tc"), ("", "T"), ("<DEL>", "A"), ("T", "T"), ("R", "Y")]


def test_letters_table():
    for ref, alt in ALLELE_PAIRS:
        rc, ac = R.first_base_code(ref), R.first_base_code(alt)
        assert T.first_base_code(ref) == rc and T.first_base_code(alt) == ac
        r, a = T.sanitize_base_pairs(np.array([rc], dtype=np.uint8), np.array([ac], dtype=np.uint8))
        assert (int(r[0]), int(a[0])) == R.sanitize_base_pair(rc, ac)
        assert int(T.het_iupac(r, a)[0]) == R.het_iupac(int(r[0]), int(a[0]))
    # lower-case bytes handed straight to the byte form
    r, a = T.sanitize_base_pairs(np.frombuffer(b"ac*", dtype=np.uint8), np.frombuffer(b"gn*", dtype=np.uint8))
    assert bytes(r) == b"ACA" and bytes(a) == b"GGG"


def test_alignment_conversion_flipped_and_unflipped():
    g = np.array([[0.0, 1.0, 2.0, -9.0, np.nan, 0.5, 1.5, 0.51, 1.49]] * len(ALLELE_PAIRS), dtype=np.float32)
    refs, alts = [p[0] for p in ALLELE_PAIRS], [p[1] for p in ALLELE_PAIRS]
    rc = np.array([R.first_base_code(s) for s in refs], dtype=np.uint8)
    ac = np.array([R.first_base_code(s) for s in alts], dtype=np.uint8)
    want = R.convert_geno_to_alignment(g, rc, ac)
    assert np.array_equal(jx.geno_chunk_to_alignment_u8(g, rc, ac), want)
    assert np.array_equal(jx.geno_chunk_to_alignment_u8_sites(g, refs, alts), want)
    sites = [SimpleNamespace(ref_allele=r, alt_allele=a) for r, a in ALLELE_PAIRS]
    assert np.array_equal(jx.geno_chunk_to_alignment_u8_siteinfo(g, sites), want)
    assert bytes(want[:, 0]) == b"ARGNNAGRR" and bytes(want[:, 7]) == b"AAANNAAAA"      # A/G; A/AT: one letter, hets included
    # packed form: every code of every pair, flipped and unflipped, against the value form of the reference's loader
    from janusx_amd import bed
    codes = np.array([[0, 1, 2, -1, 2, 0, 1]] * len(ALLELE_PAIRS))
    packed = bed.pack_dosage(codes)
    for flip in (np.zeros(len(ALLELE_PAIRS), dtype=bool), np.ones(len(ALLELE_PAIRS), dtype=bool),
                 np.arange(len(ALLELE_PAIRS)) % 2 == 0):
        l00, l10, l11 = T.packed_site_letters(refs, alts, flip)
        got = T.packed_to_alignment_u8(packed, 7, l00, l10, l11)
        assert np.array_equal(got, R.bed_alignment(packed, 7, refs, alts, flip))
    # the flip is visible where an allele is not A/C/G/T: ("A", "N") is A/G unflipped and C/A flipped
    l00, _l10, l11 = T.packed_site_letters(["A"], ["N"], [False])
    f00, _f10, f11 = T.packed_site_letters(["A"], ["N"], [True])
    assert (chr(l00[0]), chr(l11[0]), chr(f00[0]), chr(f11[0])) == ("A", "G", "A", "C")
    with pytest.raises(ValueError, match="ref/alt length mismatch: expected 16, got 15/16"):
        jx.geno_chunk_to_alignment_u8(g, rc[:-1], ac)
    with pytest.raises(ValueError, match="ref_alleles/alt_alleles length mismatch: 16/15"):
        jx.geno_chunk_to_alignment_u8_sites(g, refs, alts[:-1])
    with pytest.raises(ValueError, match="sites length mismatch: expected 16, got 15"):
        jx.geno_chunk_to_alignment_u8_siteinfo(g, sites[:-1])
    assert jx.geno_chunk_to_alignment_u8(np.zeros((0, 3), dtype=np.float32), [], []).shape == (3, 0)


def test_name_quoting():
    for name in ("s1", "a_b.c-d", "", "a b", "it's", "x:y", "(z)", "é", "a,b", "A9"):
        assert T.quote_newick_name(name) == R.quote_newick_name(name)
    assert T.quote_newick_name("it's me") == "'it_s me'" and T.quote_newick_name("ok-1.x_") == "ok-1.x_" and T.quote_newick_name("é") == "'é'"


def test_length_rendering_and_deep_caterpillar():
    for x, want in ((0.0, "0.0000000000"), (-0.0, "-0.0000000000"), (0.5, "0.5000000000"), (1e-11, "0.0000000000"),
                    (5e-11, "0.0000000001"), (2.0 ** -11, "0.0004882812"), (3 * 2.0 ** -11, "0.0014648438"), (123456.7, "123456.7000000000")):
        assert T.format_branch_length(x) == want
    n = 5000
    names = [f"s{i}" for i in range(n)]
    joins = [(0, 1, 0.1, -0.0)] + [(n + t - 1, t + 1, 0.25, 1.0 / (t + 1)) for t in range(1, n - 1)]
    text = T.render_newick(names, joins, n + len(joins) - 1) + ";"
    assert text == R.render_newick(names, joins)
    assert text.startswith("(" * (n - 1) + "s0:0.1000000000,s1:-0.0000000000):0.2500000000,s2:0.5000000000)") and text.endswith(";")
    # lengths of both routes from one log entry
    for dij, ri, rj, m in ((0.3, 2.0, 1.0, 5), (0.1, 0.0, 3.0, 4), (0.0, 1.0, 1.0, 3), (-0.0, 0.0, 0.0, 3), (1.0, np.inf, 1.0, 6)):
        assert T.nj_branch_lengths(dij, ri, rj, m, "alignment") == _lengths(dij, ri, rj, m, "alignment")
        assert T.nj_branch_lengths(dij, ri, rj, m, "distance") == _lengths(dij, ri, rj, m, "distance")
    li, lj = T.nj_branch_lengths(-0.0, 0.0, 0.0, 3, "distance")
    assert str(lj) == "-0.0" and str(T.nj_branch_lengths(-0.0, 0.0, 0.0, 3, "alignment")[1]) == "0.0"


def _lengths(dij, ri, rj, m, route):
    import math
    if route == "alignment":
        li = 0.5 * (dij + (ri - rj) / (m - 2.0))
        lj = dij - li
        return (li if math.isfinite(li) and li > 0.0 else 0.0), (lj if math.isfinite(lj) and lj > 0.0 else 0.0)
    li = 0.5 * dij + (ri - rj) / (2.0 * max(m - 2.0, 1.0))
    lj = dij - li
    return (0.0 if not math.isfinite(li) or li < 0.0 else li), (0.0 if not math.isfinite(lj) or lj < 0.0 else lj)


def test_newick_from_merge_log_matches_reference_rendering():
    rng = np.random.default_rng(5)
    n = 30
    x = rng.random((n, n))
    d = x + x.T
    np.fill_diagonal(d, 0.0)
    names = [f"id {i}" if i % 7 == 0 else f"id{i}" for i in range(n)]
    for route in ("alignment", "distance"):
        log_ij, log_vals, last, joins = R.nj(d, route)
        assert T.newick_from_merge_log(names, log_ij, log_vals, last, route) == R.render_newick(names, joins)


def test_normalize_distance_matrix_values_and_errors():
    rng = np.random.default_rng(2)
    d = rng.normal(size=(9, 9))
    d[1, 4] = np.nan
    d[6, 2] = np.inf
    d[3, 5] = d[5, 3] = -0.0
    got, want = T.normalize_distance_matrix(d), R.normalize_distance_matrix(d)
    assert got.tobytes() == want.tobytes()
    assert got[1, 4] == d[4, 1] or (d[4, 1] < 0 and got[1, 4] == 0.0)
    assert str(got[3, 5]) == "-0.0"                                              # `v < 0.0` is false for -0.0
    cases = []
    e = d.copy()
    e[4, 4] = np.nan
    e[2, 7] = e[7, 2] = np.inf                                                   # an earlier row wins
    cases.append(e)
    e = d.copy()
    e[4, 4] = np.inf
    e[4, 7] = e[7, 4] = np.nan                                                   # same row: the diagonal is checked first
    cases.append(e)
    e = d.copy()
    e[0, 8] = e[8, 0] = 1.7e308                                                  # finite both ways, the mean overflows? no: 0.5 (a + b)
    cases.append(e)
    e = d.copy()
    e[0, 1] = e[1, 0] = -np.inf
    cases.append(e)
    for e in cases + [np.zeros((3, 4)), np.zeros((1, 1)), np.zeros(4)]:
        try:
            want = R.normalize_distance_matrix(e)
        except ValueError as err:
            with pytest.raises(ValueError) as got_err:
                T.normalize_distance_matrix(e)
            assert str(got_err.value) == str(err)
        else:
            assert T.normalize_distance_matrix(e).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match=r"distance matrix diagonal has NaN/Inf at \(4,4\)"):
        T.normalize_distance_matrix(cases[1])
    with pytest.raises(ValueError, match=r"NaN/Inf in both directions at \(2, 7\) and \(7, 2\)"):
        T.normalize_distance_matrix(cases[0])
    with pytest.raises(ValueError, match=r"invalid value after symmetrization at \(0, 8\)"):
        T.normalize_distance_matrix(cases[2])


def test_jc69_distance_host():
    valid = np.array([[9, 8, 0, 4], [8, 9, 2, 4], [0, 2, 3, 3], [4, 4, 3, 9]])
    mism = np.array([[0, 2, 0, 4], [2, 0, 0, 3], [0, 0, 0, 1], [4, 3, 1, 0]])
    for min_ov in (0, 1, 3, 5):
        got = jx.tree_jc69_distance(valid, mism, min_ov)
        assert got.tobytes() == R.distance_matrix(valid, mism, min_ov).tobytes()
    d = jx.tree_jc69_distance(valid, mism, 1)
    assert d[0, 2] == 1.0 and str(d[1, 2]) == "0.0" and d[0, 0] == 0.0
    assert d[0, 3] == -0.75 * np.log(1.0 - (4.0 * (0.75 - 1e-12) / 3.0))          # p = 1 clamped to 0.75 - 1e-12


def test_alignment_repack():
    aln = np.frombuffer(b"ACGTNaG-CAACRcGT", dtype=np.uint8).reshape(4, 4)
    packed = T.alignment_to_packed(aln)
    valid, mism = R.pair_counts(aln)
    # the codes give the same counts as the letters: 00 / 11 known, 01 unknown
    codes = np.stack([(packed >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(packed.shape[0], -1)[:, :4]
    u = np.isin(codes, (0, 3)).astype(np.int64)
    w = np.where(codes == 0, 1, np.where(codes == 3, -1, 0))
    assert np.array_equal(u.T @ u, valid) and np.array_equal((u.T @ u - w.T @ w) // 2, mism)
    with pytest.raises(RuntimeError, match="alignment column 1 holds 3 distinct bases"):
        T.alignment_to_packed(np.frombuffer(b"AAACAGAA", dtype=np.uint8).reshape(4, 2))


def test_mirror_argument_errors_come_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(T, "_nj_run_device", boom)
    monkeypatch.setattr(T, "_tree_counts_device", boom)
    aln = np.frombuffer(b"ACAC", dtype=np.uint8).reshape(2, 2)
    ids = ["a", "b"]
    for args, kwargs, exc, text in (
            ((np.zeros(4, dtype=np.uint8), ids), {}, ValueError, "alignment must be a 2D uint8 matrix: (n_samples, n_sites)"),
            ((aln[:1], ["a"]), {}, ValueError, "need at least 2 samples to build a tree"),
            ((aln[:, :0], ids), {}, ValueError, "alignment has zero sites"),
            ((aln, ["a"]), {}, ValueError, "sample_ids length mismatch: got 1, expected 2"),
            ((aln, ids), {"max_taxa": 0}, ValueError, "max_taxa must be > 0"),
            ((np.tile(aln, (2, 1)), ids * 2), {"max_taxa": 3}, ValueError, "n_samples=4 exceeds max_taxa=3; NJ in phase-1 is O(N^3)"),
            ((aln, ids), {"nj_approx": "fast"}, ValueError,
             "invalid nj_approx='fast' (expected 'exact', 'bionj', 'bionj-dist', 'bionj-jc', 'bionj-binom', 'bionj-auto', 'top-hits', "
             "'rapidnj', 'lt-lazyq', or 'rapid-core')"),
            ((aln, ids), {"nj_approx": "top-hits", "top_hits_k": 0}, ValueError, "top_hits_k must be > 0 when nj_approx='top-hits'"),
    ):
        with pytest.raises(exc) as err:
            jx.nj_newick_from_alignment_u8(*args, **kwargs)
        assert str(err.value) == text
    for mode, name in (("BIONJ", "bionj"), ("bionj_dist", "bionj-dist"), ("bionj-jc69", "bionj-jc"), ("bionjbinom", "bionj-binom"),
                       ("bionj-auto", "bionj-auto"), ("tophits", "top-hits"), ("rapid_nj", "rapidnj"), ("lazyq", "lt-lazyq"),
                       ("rapidcore", "rapid-core")):
        with pytest.raises(RuntimeError, match=f"nj_approx='{name}' is not built"):
            jx.nj_newick_from_alignment_u8(aln, ids, nj_approx=mode)
    with pytest.raises(RuntimeError, match="alignment column 0 holds 3 distinct bases"):
        jx.nj_newick_from_alignment_u8(np.frombuffer(b"ACG", dtype=np.uint8).reshape(3, 1), ["a", "b", "c"])
    sq = np.zeros((3, 3))
    for args, kwargs, text in (
            ((np.zeros(3), ["a"] * 3), {}, "distance matrix must be a 2D float matrix: (n_samples, n_samples)"),
            ((np.zeros((1, 1)), ["a"]), {}, "need at least 2 samples to build a tree"),
            ((np.zeros((3, 2)), ["a"] * 3), {}, "distance matrix must be square, got 3x2"),
            ((sq, ["a"] * 2), {}, "sample_ids length mismatch: got 2, expected 3"),
            ((sq, ["a"] * 3), {"max_taxa": 0}, "max_taxa must be > 0"),
            ((sq, ["a"] * 3), {"max_taxa": 2}, "n_samples=3 exceeds max_taxa=2; distance-NJ is O(N^3)"),
            ((np.full((3, 3), np.nan), ["a"] * 3), {}, "distance matrix diagonal has NaN/Inf at (0,0)"),
    ):
        with pytest.raises(ValueError) as err:
            jx.nj_newick_from_distance_matrix(*args, **kwargs)
        assert str(err.value) == text
    with pytest.raises(ValueError, match="need at least 2 samples"):
        jx.nj_newick_from_packed(np.zeros((3, 1), dtype=np.uint8), 1, ["a"])
    with pytest.raises(RuntimeError, match="packed must be 2D"):
        jx.tree_pair_counts_packed(np.zeros((3, 2), dtype=np.uint8), 3)
    import inspect
    sig = inspect.signature(jx.nj_newick_from_alignment_u8)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:] == [("min_overlap", 1), ("max_taxa", 2000), ("threads", 0),
                                                                        ("nj_approx", "exact"), ("top_hits_k", 64)]
    assert inspect.signature(jx.nj_newick_from_distance_matrix).parameters["max_taxa"].default == 20000


def test_phylip_names_and_fasta_text(tmp_path):
    assert T.sanitize_phylip_names(["a b", "a_b", " x'y ", "", "a b"]) == ["a_b", "a_b_2", "x_y", "sample", "a_b_3"]
    aln = np.frombuffer((b"ACGT" * 41)[:162], dtype=np.uint8).reshape(2, 81)
    T.write_fasta(tmp_path / "x.fasta", ["s1", "s 2"], aln)
    assert (tmp_path / "x.fasta").read_text() == R.fasta_text(["s1", "s 2"], aln)
    T.write_phylip(tmp_path / "x.phy", ["s1", "s 2"], aln)
    lines = (tmp_path / "x.phy").read_text().split("\n")
    assert lines[0] == "2 81" and lines[1] == "s1   " + bytes(aln[0]).decode() and lines[2].startswith("s_2  ")


@pytest.mark.parametrize("argv,text", [
    (["tree", "-bfile", "x", "-nj", "bionj"], "tree: -nj bionj is not built"),
    (["tree", "-bfile", "x", "-nj", "bionj-dist"], "tree: -nj bionj-dist is not built"),
    (["tree", "-bfile", "x", "-nj", "approx"], "tree: -nj approx is not built"),
    (["tree", "-bfile", "x", "-nj", "nearest"], "tree: unknown -nj mode 'nearest'"),
    (["tree", "-bfile", "x", "-ml"], "tree: -ml (FastTree maximum likelihood) is not built"),
    (["tree", "-fa", "x.fa", "-nj"], "tree: -fa input is not supported"),
    (["tree", "-vcf", "x.vcf", "-nj"], "tree: -vcf input is not supported"),
    (["tree", "-hmp", "x.hmp", "-nj"], "tree: -hmp input is not supported"),
    (["tree", "-file", "x.txt", "-nj"], "tree: -file input is not supported"),
    (["tree", "-nj"], "tree needs -bfile PREFIX"),
])
def test_cli_refusals(argv, text):
    with pytest.raises(SystemExit) as err:
        cli.main(argv)
    assert str(err.value).startswith(text) and "\n" not in str(err.value)
