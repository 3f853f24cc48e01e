"""Host pieces of `jx fvlmm2 -screen` (janusx_amd/fvlmm2.py: variants, the chi^2 quantile, the screen-table writer; the refusals of
cli.cmd_fvlmm2 and janusx.fvlmm2_screen_packed) and the restatement tests/pairscreen_ref.py against itself: f64 against
rational.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import pairscreen_ref as P
from janusx_amd import fvlmm2 as f2

CLASS_CODES = [0, 2, 3]            # the 2-bit codes of the classes hom-ref, het, hom-alt


def _all_patterns():
    return [("*", False, False), ("^", False, False)] + [(op, a, b) for op in "&|" for a in (False, True) for b in (False, True)]


def test_default_spec_gives_ten_variants_in_order():
    got = [(v.op, v.neg1, v.neg2) for v in f2.screen_variants()]
    assert got == [("*", False, False), ("&", False, False), ("&", True, False), ("&", False, True), ("&", True, True),
                   ("|", False, False), ("|", True, False), ("|", False, True), ("|", True, True), ("^", False, False)]
    assert [(v.op, v.neg1, v.neg2) for v in f2.screen_variants("!&, |! ,^,^")] == [("&", True, False), ("|", False, True),
                                                                                  ("^", False, False)]
    assert f2.screen_variants("&")[3].spelled("a", "b") == "!a&!b" and f2.screen_variants("*")[0].spelled("a", "b") == "a*b"


@pytest.mark.parametrize("op,neg1,neg2", _all_patterns())
def test_variant_tables_equal_pair_tables_on_hard_calls(op, neg1, neg2):
    """The class tables are `pair_tables` on the decoded values of hard calls ([0, mean, 1, 2] by code), read at the codes of the
    three classes; the mean of the missing code does not enter."""
    lut = np.array([[0.0, 0.7, 1.0, 2.0]], dtype=np.float32)
    tab, _pos = f2.pair_tables(lut, lut, [op], [neg1], [neg2])
    v = f2.variant_tables(op, neg1, neg2)
    exp = tab.reshape(4, 4)[np.ix_(CLASS_CODES, CLASS_CODES)].astype(np.float64)
    assert np.array_equal(v.combo, exp)
    assert np.array_equal(v.lit1, f2.literal_values(lut, [neg1])[0, CLASS_CODES].astype(np.float64))
    assert np.array_equal(v.lit2, f2.literal_values(lut, [neg2])[0, CLASS_CODES].astype(np.float64))
    arr = f2.variant_array([v])
    assert arr.shape == (1, 15) and np.array_equal(arr[0, :9].reshape(3, 3), v.combo)
    assert np.array_equal(arr[0, 9:12], v.lit1) and np.array_equal(arr[0, 12:], v.lit2)


@pytest.mark.parametrize("op,neg1,neg2", _all_patterns())
def test_flip_and_negation_are_class_permutations(op, neg1, neg2):
    """A flipped row decodes as [2, mean, 1, 0]: `pair_tables` on flipped LUTs equals the unflipped variant read at class 2 - a;
    negating a literal of a logic operator is the same permutation of that side's tables."""
    plain, flipped = np.array([[0.0, 0.7, 1.0, 2.0]], dtype=np.float32), np.array([[2.0, 1.3, 1.0, 0.0]], dtype=np.float32)
    v = f2.variant_tables(op, neg1, neg2)
    for f1 in (False, True):
        for fl2 in (False, True):
            tab, _ = f2.pair_tables(flipped if f1 else plain, flipped if fl2 else plain, [op], [neg1], [neg2])
            exp = tab.reshape(4, 4)[np.ix_(CLASS_CODES, CLASS_CODES)].astype(np.float64)
            got = f2.permute_classes(v, f1, fl2)
            assert np.array_equal(got.combo, exp), (f1, fl2)
            assert np.array_equal(got.lit1, v.lit1[::-1] if f1 else v.lit1) and np.array_equal(got.lit2, v.lit2[::-1] if fl2 else v.lit2)
    if op in "&|":
        base = f2.variant_tables(op, False, False)
        perm = f2.permute_classes(base, neg1, neg2)
        assert np.array_equal(perm.combo, v.combo) and np.array_equal(perm.lit1, v.lit1) and np.array_equal(perm.lit2, v.lit2)


def test_bad_specs_are_refused():
    for spec, text in (("+", "unsupported entry '+'"), ("&,,|", "unsupported entry ''"), ("", "no operator given"), ("!*", "takes no negation"),
                       ("^!", "takes no negation"), ("!!&", "unsupported entry"), ("a&b", "unsupported entry")):
        with pytest.raises(ValueError, match=text.replace("+", r"\+").replace("*", r"\*").replace("^", r"\^")):
            f2.screen_variants(spec)
    with pytest.raises(ValueError, match=r"Negated literals are not supported"):
        f2.variant_tables("*", True, False)
    assert len(f2.screen_variants("*,&,|,^")) == 10 <= f2.SCREEN_MAX_VARIANTS


def test_more_than_sixteen_variants_are_refused(monkeypatch):
    monkeypatch.setattr(f2, "SCREEN_MAX_VARIANTS", 8)
    with pytest.raises(ValueError, match="at most 8 variants, got 10"):
        f2.screen_variants()
    import janusx_amd.janusx as jx
    with pytest.raises(RuntimeError, match="between 1 and 16 variants, got 17"):
        jx.fvlmm2_screen_packed(np.zeros((2, 2), np.uint8), 8, [False, False], np.zeros(8), 1.0, np.zeros((17, 15)), 1.0)
    with pytest.raises(RuntimeError, match="sigma2 must be finite and positive"):
        jx.fvlmm2_screen_packed(np.zeros((2, 2), np.uint8), 8, [False, False], np.zeros(8), 0.0, np.zeros((1, 15)), 1.0)


def test_quantile_round_trip():
    """P -> t_min -> P through the forward p-value of the project (lm2.chi2_sf): the bisection ends at neighbouring doubles."""
    for p in (0.5, 0.05, 1e-5, 1e-8, 1e-12, 1e-30, 1e-100):
        t = f2.chi2_1_quantile(p)
        assert abs(f2.chi2_1_pvalue(t) - p) <= 1e-9 * p, (p, t)
        assert f2.chi2_1_pvalue(t) <= p < f2.chi2_1_pvalue(math.nextafter(t, 0.0)) or f2.chi2_1_pvalue(t) == p
    assert abs(f2.chi2_1_quantile(0.05) - 3.841458820694124) < 1e-9
    assert abs(f2.chi2_1_quantile(1e-5) - 19.511420964666268) < 1e-7
    for bad in (0.0, 1.0, -1.0, 2.0, math.nan):
        with pytest.raises(ValueError, match=r"within \(0, 1\)"):
            f2.chi2_1_quantile(bad)


def test_screen_table_text(tmp_path):
    path = tmp_path / "s.tsv"
    n = f2.write_screen_table(path, ["rs1", "rs3"], ["rs2", "1_500"], ["rs1&!rs2", "rs3*1_500"], [160, 97], [30.25, 19.6])
    assert n == 2
    assert path.read_text() == ("snp1\tsnp2\tcombo_id\tn_complete\tstat\tp_screen\n"
                                f"rs1\trs2\trs1&!rs2\t160\t30.2500\t{f2.format_sci4(f2.chi2_1_pvalue(30.25))}\n"
                                f"rs3\t1_500\trs3*1_500\t97\t19.6000\t{f2.format_sci4(f2.chi2_1_pvalue(19.6))}\n")
    assert f2.format_sci4(f2.chi2_1_pvalue(30.25)) == "3.7979e-8"        # 2 (1 - Phi(5.5))
    assert f2.write_screen_table(path, [], [], [], [], []) == 0 and path.read_text().count("\n") == 1


def test_screen_residual_is_the_gls_residual_in_sample_space():
    rng = np.random.default_rng(5)
    n, lbd = 40, 0.7
    a = rng.normal(size=(n, n))
    s, u = np.linalg.eigh(a @ a.T / n)
    x, y = np.column_stack([np.ones(n), rng.normal(size=n)]), rng.normal(size=n)
    r, sigma2 = f2.screen_residual(s, u.T @ x, u.T @ y, u.T.astype(np.float32), lbd)
    vinv = np.linalg.inv(u @ np.diag(s + lbd) @ u.T)                    # V^-1 (y - X b), b the GLS estimate
    beta = np.linalg.solve(x.T @ vinv @ x, x.T @ vinv @ y)
    exp = vinv @ (y - x @ beta)
    assert np.max(np.abs(r - exp)) <= 1e-5 * np.max(np.abs(exp))        # U^T is handed over in f32
    assert sigma2 == pytest.approx(float(r @ r) / (n - 2), rel=1e-14)


def test_cli_refusals(tmp_path):
    from janusx_amd import cli
    ph = tmp_path / "ph.tsv"
    ph.write_text("id\tT\ns0\t1.0\n")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a*b\n")

    def msg(*argv):
        with pytest.raises(SystemExit) as e:
            cli.main(["fvlmm2", "-bfile", "x", "-p", str(ph), *argv])
        return str(e.value)
    assert "-screen finds its own pairs and cannot be combined with -i or -among" in msg("-screen", "-i", str(pairs))
    assert "-screen finds its own pairs and cannot be combined with -i or -among" in msg("-screen", "1e-4", "-among", str(pairs))
    assert "unsupported entry '+'" in msg("-screen", "-screen-ops", "+")
    assert "-screen P must be within (0, 1)" in msg("-screen", "0")
    assert "-screen-top must be >= 1" in msg("-screen", "-screen-top", "0")
    assert "-screen-min-dist must be >= 0" in msg("-screen", "-screen-min-dist", "-5")
    assert "-screen-among file not found" in msg("-screen", "-screen-among", str(tmp_path / "none.txt"))
    assert "needs an interaction file" in msg()                       # without -screen nothing changed


def _random_tables(rng, count):
    """Class tables of random genotype pairs (n in 8 .. 200, class frequencies from random allele frequencies, 3 % missing, LD by
    copying part of the first row) against a random r through the digit split."""
    for _ in range(count):
        n = int(rng.integers(8, 201))
        p1, p2 = rng.uniform(0.05, 0.95, size=2)
        g1 = rng.binomial(2, p1, size=n)
        g2 = np.where(rng.random(n) < rng.uniform(0.0, 0.9), g1, rng.binomial(2, p2, size=n))
        c1 = np.where(rng.random(n) < 0.03, -1, g1).astype(np.int8)
        c2 = np.where(rng.random(n) < 0.03, -1, g2).astype(np.int8)
        r = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)
        _d, scale, units = P.digit_split(r)
        n_tab, r_tab = P.class_tables(c1[None, :], c2[None, :], units)
        yield n_tab[0, 0], r_tab[0, 0], scale, float(r @ r) / n


def test_f64_restatement_against_the_rational_one():
    """Measured on this set (1500 random tables x 10 variants x 4 flip patterns): the largest |T64 - T| / max(T, 1) is 2.298e-14
    (`pairscreen_ref.STAT_F64_ERR` holds the bound this test asserts); the void pattern is identical.  8 times that is the tolerance
    of the GPU statistic (tests/test_gpu_fvlmm2_screen.py)."""
    rng = np.random.default_rng(20260722)
    variants = f2.variant_array(f2.screen_variants())
    worst, live, void = 0.0, 0, 0
    for k, (n_tab, r_tab, scale, sigma2) in enumerate(_random_tables(rng, 1500)):
        for var in variants:
            fi, fj = bool(k & 1), bool(k & 2)
            exact = P.stat_exact(n_tab, r_tab, scale, var, fi, fj, sigma2)
            got = P.stat_f64(n_tab, r_tab, scale, var, fi, fj, sigma2)
            assert (exact is None) == math.isnan(got), (k, n_tab, var)
            if exact is None:
                void += 1
                continue
            live += 1
            worst = max(worst, P.stat_error(got, exact))
    print(f"f64 against rational: {live} statistics, {void} void, largest error {worst:.3e}")
    assert live > 10000 and void > 50
    assert worst <= P.STAT_F64_ERR


def test_exact_statistic_is_the_textbook_score_test():
    """The fraction-free solve against the definition: T = (xc' M r)^2 / (sigma2 xc' M xc), M the projector off [1, x1, x2], on
    the expanded samples of a small table."""
    rng = np.random.default_rng(3)
    c1, c2 = rng.integers(0, 3, size=60), rng.integers(0, 3, size=60)
    r = np.ldexp(rng.integers(-2 ** 20, 2 ** 20, size=60).astype(np.float64), -20)
    _d, scale, units = P.digit_split(r)
    assert np.array_equal(units.astype(np.float64) * scale, r)           # dyadic: split exactly
    n_tab, r_tab = P.class_tables(c1[None, :].astype(np.int8), c2[None, :].astype(np.int8), units)
    for v in f2.screen_variants():
        var = f2.variant_array([v])[0]
        z = np.column_stack([np.ones(60), v.lit1[c1], v.lit2[c2]])
        xc = v.combo[c1, c2]
        proj = np.eye(60) - z @ np.linalg.solve(z.T @ z, z.T)
        exp = float(xc @ proj @ r) ** 2 / (0.9 * float(xc @ proj @ xc))
        got = P.stat_exact(n_tab[0, 0], r_tab[0, 0], scale, var, False, False, 0.9)
        assert isinstance(got, Fraction) and float(got) == pytest.approx(exp, rel=1e-9)
