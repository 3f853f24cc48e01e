"""CPU tests of the host half of `jx gwas -farmcpu` (janusx_amd/farmcpu.py): the grids, lead selection, the merge rules, the legacy
scorer against a dense GLS likelihood, the writers, and the conditions the whole-procedure fixture of tests/farmcpu_ref.py must
meet on the restatement, so that the GPU comparison of tests/test_gpu_farmcpu.py exercises every rule."""
import math

import numpy as np
import pytest

import farmcpu_ref as R
from janusx_amd import farmcpu as fc


def test_grids():
    assert fc.qtn_bound_auto(400) == 12                          # floor(sqrt(400 / log10 400)) = floor(12.39)
    assert fc.nbin_values(12, 5) == [2, 4, 6, 8, 10, 12]
    assert fc.nbin_values(3, 5) == [1, 2, 3]                     # step = max(1, 3 // 5)
    assert fc.nbin_values(1, 5) == [1]
    assert fc.qtn_bound_auto(2) == 1
    assert fc.szbin_values([5e5, 5e6, 5e7]) == [500000, 5000000, 50000000]
    assert fc.szbin_values([0.0, float("nan"), -3.0]) == list(fc.DEFAULT_SZBIN)
    assert fc.szbin_values([0.4]) == [1]
    assert R.grids(400)[1] == [2, 4, 6, 8, 10, 12]


def test_global_positions_rank_the_chromosome_names_as_strings():
    gp = fc.global_positions(["2", "10", "1", "10"], [5, 7, 9, 7])
    assert gp.tolist() == [5 + 2 * 10 ** 12, 7 + 10 ** 12, 9, 7 + 10 ** 12]      # "1" < "10" < "2"
    assert np.array_equal(gp, R.global_positions(["2", "10", "1", "10"], [5, 7, 9, 7]))


def test_bin_selection_on_a_hand_made_table():
    # two chromosomes whose positions collide: without the chromosome block the markers 0, 1, 3, 4 would share a bin
    chrom = ["1", "1", "1", "2", "2", "2"]
    pos = [100, 900, 1500, 100, 950, 1100]
    p = np.array([0.2, 0.01, 0.5, 0.03, 0.03, 0.001])
    gp = fc.global_positions(chrom, pos)
    # bins of 1000: {0, 1} {2} | {3, 4} {5}; best per bin 1, 2, 3 (tie with 4: the lower index), 5
    assert fc.select_lead_indices(1000, 10, p, gp).tolist() == [1, 2, 3, 5]
    assert fc.select_lead_indices(1000, 2, p, gp).tolist() == [1, 5]
    assert fc.select_lead_indices(1000, 3, p, gp).tolist() == [1, 3, 5]
    assert fc.select_lead_indices(10 ** 6, 10, p, gp).tolist() == [1, 5]          # one bin per chromosome
    assert fc.select_lead_indices(1000, 0, p, gp).tolist() == []
    assert fc.select_lead_indices(1000, 10, p, np.array(pos)).tolist() == [1, 5]  # the collision, were the block missing
    for sz, nn in ((1000, 10), (1000, 2), (1000, 3), (10 ** 6, 10)):
        assert fc.select_lead_indices(sz, nn, p, gp).tolist() == R.select_lead_indices(sz, nn, p, gp)


def test_prepare_seq_qtn_threshold_keep_saved_and_positions():
    femp = np.array([1e-9, 0.5, 1e-4, 1e-6, 0.02, 1e-4])
    gpos = np.array([10, 20, 30, 30, 40, 50])
    # saved 1 (p 0.5) stays only under keep_saved; lead 4 fails the threshold; 2 and 3 share a position: the better p stays
    assert fc.prepare_seq_qtn([1], [0, 2, 3, 4], femp, gpos, 0.01, True) == [0, 3, 1]
    assert fc.prepare_seq_qtn([1], [0, 2, 3, 4], femp, gpos, 0.01, False) == [0, 3]
    assert fc.prepare_seq_qtn([], [2, 5], femp, gpos, 0.01, False) == [2, 5]      # equal p: the lower index first
    assert fc.prepare_seq_qtn([], [4], femp, gpos, 0.01, False) == []
    assert fc.prepare_seq_qtn([0], [0, 2], femp, gpos, 0.01, True) == [0, 2]      # a lead that is a saved QTN counts once
    assert fc.prepare_seq_qtn([1], [0, 2, 3, 4], femp, gpos, 0.01, True) == R.prepare_seq_qtn([1], [0, 2, 3, 4], femp, gpos, 0.01, True)


def test_super_rule_counts_dropped_columns():
    rng = np.random.default_rng(2)
    n = 200
    a = rng.standard_normal(n)
    b = a + 0.6 * rng.standard_normal(n)                         # r(a, b) = 0.84
    c = b + 0.9 * rng.standard_normal(n)                         # r(b, c) = 0.80, r(a, c) = 0.68
    d = rng.standard_normal(n)
    s = np.stack([a, b, c, d, np.ones(n)], axis=1)
    r = np.corrcoef(s[:, :3].T)
    assert abs(r[0, 1]) > 0.7 and abs(r[1, 2]) > 0.7 and abs(r[0, 2]) < 0.7
    # b falls to a; c is clear of a but falls to b although b is already gone; a constant column has no correlation
    assert fc.super_keep(s).tolist() == [True, False, False, True, True]
    assert fc.super_keep(s).tolist() == R.super_keep(s)


def test_fix_zero_pvalues():
    p = np.array([0.0, 1e-10, 0.5, -0.0, np.nan])
    out = fc.fix_zero_pvalues(p.copy())
    assert out[0] == 1e-12 and out[3] == 1e-12 and out[1] == 1e-10 and math.isnan(out[4])
    assert np.array_equal(fc.fix_zero_pvalues(np.zeros(3)), np.zeros(3))          # nothing positive: untouched
    assert fc.fix_zero_pvalues(np.array([0.0, 1e-307]))[0] == fc.MIN_POSITIVE


def test_overlap_and_cycle_tests():
    assert fc.overlap_ratio([], []) == 0.0
    assert fc.overlap_ratio([1, 2], [2, 1]) == 1.0
    assert fc.overlap_ratio([1, 2], [2, 3]) == pytest.approx(1.0 / 3.0)


def test_pinv_and_design_operands_of_a_rank_deficient_design():
    rng = np.random.default_rng(2)
    n = 60
    x = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 2))])
    x = np.hstack([x, x[:, 1:2], rng.integers(0, 3, size=(n, 1)).astype(float)])      # column 3 repeats column 1
    y = rng.standard_normal(n)
    des = fc.design_operands(x, 3, y)
    assert des.q.shape[1] == 4 and des.df == n - 5 - 1
    assert np.allclose(des.ixx, np.linalg.pinv(x.T @ x, rcond=1e-12, hermitian=True), atol=1e-10)
    g = rng.integers(0, 3, size=n).astype(float)
    b21 = (x.T @ g) @ des.ixx
    assert np.allclose(des.w @ (des.q.T @ g), b21[3:], atol=1e-12)
    assert float(g @ g - b21 @ (x.T @ g)) == pytest.approx(float(g @ g - (des.q.T @ g) @ (des.q.T @ g)), rel=1e-11)
    assert float(g @ des.r_y) == pytest.approx(float(g @ y - (x.T @ g) @ des.bg_beta), abs=1e-11)


def _dense_gls_score(y, x, s):
    """-2 max over the delta grid of the profile log-likelihood of y ~ N(X b, sigma^2 (S S' + delta I)), dense."""
    n = len(y)
    best = -math.inf
    e = -5.0
    while e <= 5.0 + 1e-12:
        v = s @ s.T + math.exp(e) * np.eye(n)
        vi = np.linalg.inv(v)
        b = np.linalg.solve(x.T @ vi @ x, x.T @ vi @ y)
        r = y - x @ b
        sig = float(r @ vi @ r) / n
        ll = -0.5 * (n * math.log(2.0 * math.pi) + np.linalg.slogdet(v)[1] + n + n * math.log(sig))
        best = max(best, ll)
        e += 0.1
    return -2.0 * best


def test_scorer_is_the_dense_gls_profile_likelihood():
    rng = np.random.default_rng(3)
    n = 40
    s = rng.integers(0, 3, size=(n, 3)).astype(float)
    x = np.hstack([np.ones((n, 1)), rng.standard_normal((n, 1))])
    y = s @ np.array([0.7, -0.4, 0.2]) + rng.standard_normal(n)
    want = _dense_gls_score(y, x, s)
    assert fc.ll_score(y, x, s) == pytest.approx(want, rel=1e-9)
    assert R.ll_score(y, x, s) == pytest.approx(want, rel=1e-9)
    # two identical lead columns: the zero singular value is dropped, the score is that of the set without the repeat
    s2 = np.hstack([s, s[:, :1]])
    assert fc.ll_score(y, x, s2) == pytest.approx(_dense_gls_score(y, x, s2), rel=1e-9)
    # a constant lead column collapses the grid to delta = e^100
    s3 = np.hstack([s, np.full((n, 1), 2.0)])
    assert fc.ll_score(y, x, s3) == pytest.approx(R.ll_score(y, x, s3), rel=1e-12)
    assert fc.ll_score(y, x, s3) != pytest.approx(fc.ll_score(y, x, s), rel=1e-3)


def test_writers_byte_for_byte(tmp_path):
    from janusx_amd import _lib
    _lib.lib()
    chrom, pos = ["1", "1", "2", "10"], [100, 250, 77, 5]
    snp, a0, a1 = ["rs1", ".", "rs3", ""], ["A", "C", "G", "T"], ["G", "T", "A", "C"]
    af = np.array([0.25, 0.49995, 0.1, 0.333333], dtype=np.float32)
    miss = np.array([0, 3, 12, 1])
    stats = np.array([[0.12345, 0.05, 1.2e-5], [np.nan, np.nan, 1.0], [-2.5, 0.25, 3.3e-19], [1e-5, 2.0, 0.99996]])
    src = [10, 11, 15, 20]
    names = [fc.resolve_snp_name(s, c, p) for s, c, p in zip(snp, chrom, pos)]
    main, qtn = R.render_tables(stats, [2, 0], chrom, pos, names, a0, a1, af, miss, src)
    fc.write_main_tsv(str(tmp_path / "t.tsv"), chrom, pos, snp, a0, a1, af, miss, stats)
    fc.write_qtn_tsv(str(tmp_path / "t.qtn"), [2, 0], chrom, pos, snp, a0, a1, af, miss, stats, src)
    assert (tmp_path / "t.tsv").read_text() == main
    assert (tmp_path / "t.qtn").read_text() == qtn
    assert main.splitlines()[1] == "1\t100\trs1\tA\tG\t0.2500\t0\t0.1235\t0.0500\t6.0960e0\t1.2000e-5"
    assert main.splitlines()[2] == "1\t250\t1_250\tC\tT\t0.4999\t3\tNaN\tNaN\tNaN\t1.0000e0"
    assert qtn.splitlines()[1].endswith("\t10") and qtn.splitlines()[2].endswith("\t15")


# ---- the fixture conditions, on the restatement ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_run():
    fx = R.make_fixture()
    gd = R.fixture_decoded(fx)
    return fx, gd, R.run_raw(gd, fx["y"], fx["x_base"], fx["chrom"], fx["pos"], 1.0 / len(gd))


def test_fixture_shape(fixture_run):
    fx, gd, _res = fixture_run
    assert gd.shape == (3000, 400)
    gp = R.global_positions(fx["chrom"], fx["pos"])
    nb = [len(np.unique(gp // sz)) for sz in (500_000, 5_000_000, 50_000_000)]
    assert nb[0] > nb[1] > nb[2] >= 9                            # the three sizes give different bins
    # no duplicate genotype rows (the marker at the position of another one differs from it)
    assert len({r.tobytes() for r in fx["g"]}) == len(fx["g"])


def test_fixture_exercises_every_rule(fixture_run):
    _fx, _gd, res = fixture_run
    tr = res["trace"]
    assert len(tr) >= 3 and len(res["qtn"]) >= 3
    later = tr[1:]
    assert sum(t["dropped_by_super"] for t in later) >= 1
    assert sum(t["dropped_by_position"] for t in later) >= 1
    assert sum(len(t["lead_failed_threshold"]) for t in later) >= 1
    assert not any(t["loop2_null"] for t in later)


def test_fixture_choices_are_not_near_ties(fixture_run):
    """A disagreement at the 1e-10 level cannot flip a discrete choice: every selected lead beats the runner-up of its bin by
    1e-6 relative in -log10 p, and the best combo score beats that of every other lead set by 1e-6 relative (combos with the
    same lead set carry the same score bit for bit; the first wins in either implementation)."""
    fx, _gd, res = fixture_run
    nbins = R.grids(400)[1]
    for t in res["trace"][1:]:
        prior, gp = t["prior"], t["gpos"]
        lp = -np.log10(prior)
        combos = [(sz, nn) for sz in (500_000, 5_000_000, 50_000_000) for nn in nbins]
        for (sz, nn), score in zip(combos, t["scores"]):
            bins = gp // sz
            for i in R.select_lead_indices(sz, nn, prior, gp):
                rest = lp[(bins == bins[i]) & (np.arange(len(lp)) != i)]
                if rest.size:
                    assert lp[i] - rest.max() >= 1e-6 * lp[i], (sz, nn, i)
        sets = {}
        for (sz, nn), score in zip(combos, t["scores"]):
            sets.setdefault(tuple(R.select_lead_indices(sz, nn, prior, gp)), score)
        scores = sorted(sets.values())
        assert len(scores) >= 2 and scores[1] - scores[0] >= 1e-6 * abs(scores[0]), scores[:3]
