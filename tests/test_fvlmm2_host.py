"""Host pieces of `jx fvlmm2` (janusx_amd/fvlmm2.py, the argument checks of janusx.fvlmm2_assoc_chunk_f32, the refusals of
cli.cmd_fvlmm2) against the rules of python/janusx/script/fvlmm2.py and src/stats/fvlmm2.rs:57-149.  No GPU."""
import numpy as np
import pytest

import fvlmm2_ref as R
from janusx_amd import fvlmm2 as f2

NOT_FOUND = "\"SNP token '%s' was not found among active filtered variants.\""


def _name_map():
    chrom = ["1", "1", "2", "2", "2", "X"]
    pos = [100, 200, 100, 300, 400, 7]
    snp = ["rsA", "rsB", ".", "dup", "dup", "rsX"]
    return f2.build_name_map(chrom, pos, snp)


def test_name_map_and_tokens():
    names, nm = _name_map()
    assert names == ["rsA", "rsB", "2_100", "dup", "dup", "rsX"]
    assert nm["rsA"] == [0] and nm["1_100"] == [0] and nm["2_100"] == [2] and nm["dup"] == [3, 4] and nm["2_300"] == [3]
    assert f2.resolve_snp_token(" rsB ", nm) == 1
    with pytest.raises(f2.NameLookupError) as e:
        f2.resolve_snp_token("dup", nm)
    assert e.value.reason == "SNP token 'dup' is ambiguous after filtering; matched 2 active rows."
    with pytest.raises(f2.NameLookupError) as e:
        f2.resolve_snp_token("nope", nm)
    assert e.value.reason == NOT_FOUND % "nope"
    assert f2.split_literal_token("!!rsA") == ("rsA", False) and f2.split_literal_token("! rsA") == ("rsA", True) and f2.split_literal_token("!!!x") == ("x", True)
    with pytest.raises(ValueError, match="Literal token has no SNP name after '!'."):
        f2.split_literal_token("!!")


def test_parser_every_operator_and_skip_reason(tmp_path):
    _names, nm = _name_map()
    path = tmp_path / "pairs.txt"
    path.write_text("# comment\n"
                    "\n"
                    "rsA*rsB trailing words\n"
                    "rsA&!rsB\n"
                    "!rsA|rsB\n"
                    "!!rsA^!rsX\n"
                    "1_100&2_400\n"
                    "   2_100|rsX\n"
                    "!rsA*rsB\n"
                    "rsA*!!!rsB\n"
                    "rsA&dup\n"
                    "rsA&nope\n"
                    "rsA+rsB\n"
                    "rsA&&rsB\n"
                    "rsA&!\n"
                    "rsA\n")
    specs, skipped = f2.parse_interaction_file(str(path), nm)
    assert [(s.expr, s.snp1, s.op, s.snp2, s.row1, s.row2, s.neg1, s.neg2) for s in specs] == [
        ("rsA*rsB", "rsA", "*", "rsB", 0, 1, False, False),
        ("rsA&!rsB", "rsA", "&", "rsB", 0, 1, False, True),
        ("!rsA|rsB", "rsA", "|", "rsB", 0, 1, True, False),
        ("rsA^!rsX", "rsA", "^", "rsX", 0, 5, False, True),
        ("1_100&2_400", "1_100", "&", "2_400", 0, 4, False, False),
        ("2_100|rsX", "2_100", "|", "rsX", 2, 5, False, False)]
    assert skipped == [
        ("9", "!rsA*rsB", "negated_literals_not_supported_for_multiplicative_interaction"),
        ("10", "rsA*!rsB", "negated_literals_not_supported_for_multiplicative_interaction"),
        ("11", "rsA&dup", "SNP token 'dup' is ambiguous after filtering; matched 2 active rows."),
        ("12", "rsA&nope", NOT_FOUND % "nope"),
        ("13", "rsA+rsB", "invalid_expression"),
        ("14", "rsA&&rsB", "invalid_expression"),
        ("15", "rsA&!", "Literal token has no SNP name after '!'."),
        ("16", "rsA", "invalid_expression")]
    out = tmp_path / "x.skip"
    f2.write_skip(str(out), skipped[2:4])
    assert out.read_text().splitlines() == [
        "line\texpr\treason",
        "11\trsA&dup\tSNP token 'dup' is ambiguous after filtering; matched 2 active rows.",
        "12\trsA&nope\t\"\"\"SNP token 'nope' was not found among active filtered variants.\"\"\""]


def test_among_pairs_in_row_order(tmp_path):
    names, nm = _name_map()
    path = tmp_path / "among.txt"
    path.write_text("rsX\n# c\nrsA extra\n2_100\nrsA\nnope\n")
    got = f2.read_among_names(str(path))
    assert got == ["rsX", "rsA", "2_100", "rsA", "nope"]
    specs, skipped = f2.among_specs(got, nm, names, "&")
    assert [(s.expr, s.row1, s.row2, s.op) for s in specs] == [("rsA&2_100", 0, 2, "&"), ("rsA&rsX", 0, 5, "&"), ("2_100&rsX", 2, 5, "&")]
    assert skipped == [("among:5", "nope", NOT_FOUND % "nope")]
    with pytest.raises(ValueError, match="Unsupported interaction operator"):
        f2.among_specs(got, nm, names, "+")
    path.write_text("".join(f"s{i}\n" for i in range(4097)))
    with pytest.raises(ValueError, match="at most 4096 SNP names, got 4097"):
        f2.read_among_names(str(path))


def _lut(mean, flip):
    return np.array([2.0 if flip else 0.0, mean, 1.0, 0.0 if flip else 2.0], dtype=np.float32)


@pytest.mark.parametrize("flip1", [False, True])
@pytest.mark.parametrize("flip2", [False, True])
def test_tables_equal_the_restated_rules(flip1, flip2):
    means = [np.float32(0.5), np.float32(1.5), np.float32(2.5e-8), np.float32(0.3), np.float32(1.7)]
    for m1 in means:
        for m2 in means:
            l1, l2 = _lut(m1, flip1), _lut(m2, flip2)
            # the 16 code pairs as two decoded "rows" of 16 samples
            g1 = np.repeat(l1, 4)[None, :]
            g2 = np.tile(l2, 4)[None, :]
            for op in "*&|^":
                for n1 in ((False,) if op == "*" else (False, True)):
                    for n2 in ((False,) if op == "*" else (False, True)):
                        tab, pos = f2.pair_tables(l1[None], l2[None], [op], [n1], [n2])
                        exp, _a1, _a2, _ac = R.combo_rows(g1, g2, [op], [n1], [n2])
                        assert tab.dtype == np.float32 and tab.tobytes() == exp.tobytes(), (op, n1, n2, m1, m2)
                        lit1, lit2 = R.literalize(l1[None], [n1])[0], R.literalize(l2[None], [n2])[0]
                        bits = np.concatenate([lit1 > 0, lit2 > 0, exp[0] > 0])
                        assert int(pos[0]) == int(sum(1 << k for k in range(24) if bits[k]))
    # half to even: means 0.5 and 2.5e-8 are literal 0, 1.5 is literal 2
    assert f2.literal_values(np.array([[0.5, 1.5, 2.5e-8, 2.5]], dtype=np.float32), [False]).tolist() == [[0.0, 2.0, 0.0, 2.0]]
    assert f2.literal_values(np.array([[0.5, 1.5, 2.5e-8, 2.5]], dtype=np.float32), [True]).tolist() == [[2.0, 0.0, 2.0, 0.0]]


def test_xor_has_nine_cases():
    lut = np.array([[0.0, 9.0, 1.0, 2.0]], dtype=np.float32)             # code 1 is not used below
    tab, _pos = f2.pair_tables(lut, lut, ["^"], [False], [False])
    val = {0: 0, 2: 1, 3: 2}                                             # code -> hard call
    got = {(val[c1], val[c2]): float(tab[0, 4 * c1 + c2]) for c1 in val for c2 in val}
    assert got == {(0, 0): 0.0, (0, 1): 1.0, (0, 2): 2.0, (1, 0): 1.0, (1, 1): 1.0, (1, 2): 1.0, (2, 0): 2.0, (2, 1): 1.0, (2, 2): 0.0}


def test_tables_refuse_what_the_reference_refuses():
    lut = np.array([[0.0, 0.4, 1.0, 2.0]], dtype=np.float32)
    with pytest.raises(ValueError, match="Negated literals are not supported for multiplicative interaction"):
        f2.pair_tables(lut, lut, ["*"], [True], [False])
    with pytest.raises(ValueError, match="Unsupported interaction operator: %"):
        f2.pair_tables(lut, lut, ["%"], [False], [False])


def test_bh_adjust():
    p = np.array([0.01, np.nan, 0.04, -0.5, 0.03, 0.03, 2.0, 0.0])
    got = f2.bh_adjust(p)
    # valid: 0.01, 0.04, 0.03, 0.03, 1.0 (clipped), 0.0 -> m = 6
    exp = np.array([0.03, np.nan, 0.048, np.nan, 0.045, 0.045, 1.0, 0.0])
    assert np.allclose(got, exp, rtol=1e-15, atol=0, equal_nan=True)
    assert np.array_equal(f2.bh_adjust(p, n_tests=3), got, equal_nan=True)          # below the valid count: the valid count
    got12 = f2.bh_adjust(p, n_tests=12)
    assert np.allclose(got12, np.array([0.06, np.nan, 0.096, np.nan, 0.09, 0.09, 1.0, 0.0]), rtol=1e-15, atol=0, equal_nan=True)
    assert np.isnan(f2.bh_adjust([np.nan, -1.0])).all() and f2.bh_adjust([]).shape == (0,)
    rng = np.random.default_rng(3)
    q = rng.random(200)
    q[::17] = np.nan
    q[5] = q[6]
    for nt in (None, 10, 1000):
        assert np.array_equal(f2.bh_adjust(q, nt), R.bh(q, nt), equal_nan=True)


def test_number_formats(tmp_path):
    assert f2.format_sci4(1.2000e-05) == "1.2e-5" and f2.format_sci4(0) == "0e0" and f2.format_sci4(1.0) == "1e0"
    assert f2.format_sci4(1.23456e-300) == "1.2346e-300" and f2.format_sci4(-4.5e10) == "-4.5e10"
    assert f2.format_sci4(float("nan")) == "NA" and f2.format_sci4(float("inf")) == "NA" and f2.format_sci4("x") == "NA"
    assert f2.format_fixed4(0.123449) == "0.1234" and f2.format_fixed4(-2) == "-2.0000" and f2.format_fixed4(None) == "NA"
    assert f2.format_pos_int(1234.4) == "1234" and f2.format_pos_int(12.5) == "12" and f2.format_pos_int(13.5) == "14"
    assert f2.format_pos_int(float("nan")) == "NA"
    for v in (1.2e-5, 0.0, 0.05, 3.14159e-7, 1.0, float("nan")):
        assert f2.format_sci4(v) == R.sci4(v)
    joint = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 1.23456, 0.5, 1.2e-5], [np.nan] * 9])
    path = tmp_path / "t.tsv"
    assert f2.write_table(str(path), ["1", "2"], [10, 20], ["a*b", "c&d"], [0.25, 0.5], joint, [2.4e-5, np.nan]) == 2
    assert path.read_text().splitlines() == [R.HEADER, "1\t10\ta*b\t0.2500\t.\t1.2346\t0.5000\t1.2e-5\t2.4e-5\t3e-1\t6e-1",
                                             "2\t20\tc&d\t0.5000\t.\tNA\tNA\tNA\tNA\tNA\tNA"]
    assert f2.write_table(str(path), ["1", "2"], [10, 20], ["a*b", "c&d"], [0.25, 0.5], joint, [2.4e-5, np.nan], keep=[False, True]) == 1
    assert f2.trait_label("a/b\\c") == "a_b_c" and f2.trait_label(" ") == "trait"


def test_mirror_messages_before_any_device_call(monkeypatch):
    import janusx_amd.janusx as jx
    from janusx_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("device layer reached")))
    monkeypatch.setattr(jx, "lib", _lib.lib)
    n, p = 12, 2
    s, x, y = np.ones(n), np.ones((n, p)), np.arange(n, dtype=np.float64)
    g = np.ones((3, n), dtype=np.float32)

    def msg(*a):
        with pytest.raises(RuntimeError) as e:
            jx.fvlmm2_assoc_chunk_f32(*a)
        return str(e.value)
    assert msg(s, x, np.zeros(0), 0.0, g, g, g) == "y_rot must not be empty"
    assert msg(s, x[:5], y, 0.0, g, g, g) == "xcov.n_rows must equal len(y_rot)"
    assert msg(s[:5], x, y, 0.0, g, g, g) == "len(S) must equal len(y_rot)"
    assert msg(s, x, y, float("nan"), g, g, g) == "log10_lbd must be finite"
    assert msg(s, x, y, 0.0, g[:, :5], g, g) == "snp1_chunk.n_cols must equal len(y_rot)"
    assert msg(s, x, y, 0.0, g, g[:2], g) == "snp2_chunk must have the same shape as snp1_chunk"
    assert msg(s, x, y, 0.0, g, g, g[:, :4]) == "combo_chunk must have the same shape as snp1_chunk"
    assert msg(s, x, y, 400.0, g, g, g) == "log10_lbd must map to a finite positive lambda"
    assert msg(s, x, y, -400.0, g, g, g) == "log10_lbd must map to a finite positive lambda"
    assert msg(s[:5], x[:5], y[:5], 0.0, g[:, :5], g[:, :5], g[:, :5]) == "n must be > p_cov + 3 for the joint test, got n=5, p_cov=2"
    assert "at most 13 covariate columns" in msg(np.ones(40), np.ones((40, 14)), np.ones(40), 0.0, *([np.ones((1, 40), dtype=np.float32)] * 3))
    assert msg(np.where(np.arange(n) == 2, -1.0, s), x, y, 0.0, g, g, g) == "S + lambda must stay finite and positive for all samples"
    yb, xb = y.copy(), x.copy()
    yb[7] = np.inf
    xb[3, 1] = np.nan
    assert msg(s, x, yb, 0.0, g, g, g) == "y_rot contains non-finite values"
    assert msg(s, xb, y, 0.0, g, g, g) == "xcov contains non-finite values"
    assert msg(s, xb, yb, 0.0, g, g, g) == "xcov contains non-finite values"       # sample 3 comes before sample 7


def test_cli_refusals(tmp_path):
    from janusx_amd import cli
    ph = tmp_path / "ph.tsv"
    ph.write_text("id\tT\ns0\t1.0\n")
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("a*b\n")

    def msg(*argv):
        with pytest.raises(SystemExit) as e:
            cli.main(["fvlmm2", *argv])
        return str(e.value)
    assert "needs an interaction file (-i PAIRS.txt) and/or -among" in msg("-bfile", "x", "-p", str(ph))
    assert "-vcf input is not supported" in msg("-vcf", "x.vcf", "-p", str(ph), "-i", str(pairs))
    assert "-hmp input is not supported" in msg("-hmp", "x", "-p", str(ph), "-i", str(pairs))
    assert "-file input is not supported" in msg("-file", "x", "-p", str(ph), "-i", str(pairs))
    assert msg("-p", str(ph), "-i", str(pairs)) == "fvlmm2 needs -bfile PREFIX"
    assert msg("-bfile", "x", "-p", str(ph), "-i", str(pairs), "--n-tests", "-1") == "--n-tests must be >= 0"
    assert "--op must be one of" in msg("-bfile", "x", "-p", str(ph), "-i", str(pairs), "--op", "+")
    assert "-pmax must be within [0, 1]" in msg("-bfile", "x", "-p", str(ph), "-i", str(pairs), "-pmax", "2")
    among = tmp_path / "among.txt"
    among.write_text("".join(f"s{i}\n" for i in range(4097)))
    assert "at most 4096 SNP names, got 4097" in msg("-bfile", "x", "-p", str(ph), "-among", str(among))
    assert "Interaction file not found" in msg("-bfile", "x", "-p", str(ph), "-i", str(tmp_path / "none.txt"))
