"""CPU tests of the multi-trait LM scan's host side (`jx gwas -lm -trait-level`): the f64 restatement of the reference's
shared-projection route (tests/lm_traits_ref.py) against ordinary least squares, the combined table's text, the grouping of traits
by sample mask, and the argument checks of the mirrors and of the command line (all before the GPU library is touched)."""
import math

import numpy as np
import pytest

from lm_traits_ref import MIN_POSITIVE, decode_rows, lm_traits_restatement, mgs_basis, student_t_two_sided


def _panel_rows(n, m, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.5, size=m)
    g = rng.binomial(2, p[:, None], size=(m, n)).astype(np.int8)
    g[rng.random(g.shape) < 0.03] = -9
    called = (g >= 0).sum(1)
    af = (np.where(g < 0, 0, g).sum(1) / np.maximum(2 * called, 1)).astype(np.float32)
    return g, af, rng.random(m) < 0.3


def test_restatement_is_ordinary_least_squares_per_trait(oracle):
    """Per (SNP, trait) the restatement reproduces the f64 least-squares fit of y_t on [X, g], its standard error and scipy's
    two-sided Student t, within the tolerances the single-trait restatement is held to; chisq is n ln(1 + t^2 / df)."""
    from scipy import stats as sst
    n, m, T = 211, 40, 5
    g, af, flip = _panel_rows(n, m, 1)
    g[7] = 0                                                 # monomorphic: void
    rng = np.random.default_rng(2)
    x = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, 2))], axis=1)
    y = rng.standard_normal((T, n)) + 0.5 * np.where(g[3] < 0, 0, g[3])[None, :] * np.arange(T)[:, None]
    v = decode_rows(g, af, flip)
    out, rank = lm_traits_restatement(v, x, y)
    assert rank == 3 and out.shape == (T, m, 4)
    assert np.isnan(out[:, 7, :3]).all() and np.all(out[:, 7, 3] == 1.0)
    df = n - 4
    for t in range(T):
        for j in range(m):
            if j == 7:
                continue
            d = np.concatenate([x, v[j][:, None]], axis=1)
            coef, *_ = np.linalg.lstsq(d, y[t], rcond=None)
            r = y[t] - d @ coef
            se = math.sqrt(float(r @ r) / df * np.linalg.inv(d.T @ d)[3, 3])
            b, s, c, p = out[t, j]
            assert abs(b - coef[3]) <= 2e-6 * abs(coef[3]) + 2e-6 * se
            assert abs(s - se) <= 2e-6 * se
            tt = b / s
            want_p = 2.0 * sst.t.sf(abs(tt), df)
            assert abs(p - want_p) <= 1e-9 * want_p
            assert abs(c - n * math.log1p(tt * tt / df)) <= 1e-12 * n
    assert out[T - 1, 3, 3] < 1e-6                          # the causal SNP of the strongest trait
    # the vectorised tail is the reference's own function (src/stats/glm.rs:458-481, restated in the checker)
    for tt, dfv in ((0.0, 10), (1.5, 3), (-4.0, 207), (12.0, 50), (40.0, 296)):
        a, b = float(student_t_two_sided(np.float64(tt), dfv)), oracle.student_t_p_two_sided(tt, dfv)
        assert abs(a - b) <= 1e-9 * b
    assert float(student_t_two_sided(np.float64(np.inf), 10)) == MIN_POSITIVE


def test_restatement_counts_the_rank_not_the_columns():
    """A duplicated column and an all-zero column are dropped by the Gram-Schmidt rule: df = n - rank - 1."""
    from scipy import stats as sst
    n, m = 120, 12
    g, af, flip = _panel_rows(n, m, 3)
    rng = np.random.default_rng(4)
    z = rng.standard_normal((n, 2))
    x = np.stack([np.ones(n), z[:, 0], z[:, 1], 3.0 * z[:, 0], np.zeros(n)], axis=1)
    assert mgs_basis(x).shape == (n, 3)
    y = rng.standard_normal((2, n))
    v = decode_rows(g, af, flip)
    out, rank = lm_traits_restatement(v, x, y)
    full, rank_full = lm_traits_restatement(v, x[:, :3], y)
    assert rank == rank_full == 3
    assert np.allclose(out, full, rtol=1e-10, atol=0.0, equal_nan=True)
    tt = out[0, :, 0] / out[0, :, 1]
    assert np.allclose(out[0, :, 3], 2.0 * sst.t.sf(np.abs(tt), n - 3 - 1), rtol=1e-9)
    assert np.allclose(out[0, :, 2], n * np.log1p(tt * tt / (n - 4)), rtol=1e-12)


def test_combined_table_text(tmp_path):
    """Byte for byte against lines written out by hand from the reference's format strings (lm_trait.rs:254-283, 645-654):
    `{:.4}` af, `{:.4}` rate or integer count, `{:.4}` beta / se, format_chisq_value, `{:.4e}` p with Rust's exponent."""
    from janusx_amd import tsv
    chrom, pos, snp, a0, a1 = ["1", "X", "2"], [100, 2000, 5], ["rs1", ".", "rs3"], ["A", "AT", "G"], ["G", "A", "T"]
    af = np.float32([0.12345, 0.5, 0.99996])
    stats = np.array([[0.123449, 0.05, 6.0957, 1.3554e-2],
                      [np.nan, np.nan, np.nan, 1.0],
                      [-2.5, 0.25, np.inf, 1e-320]])
    rate = np.float32([0.0123, 0.0, 1.0])
    assert tsv.row_missing_is_rate(rate) and not tsv.row_missing_is_rate(np.float32([0.0, 3.0, 1.0]))
    assert not tsv.row_missing_is_rate(np.float32([0.5, np.nan]))
    path = str(tmp_path / "t.lm.tsv")
    w = tsv.TraitTableWriter(path)
    w.put(tsv.trait_site_prefixes(chrom, pos, snp, a0, a1, af, rate), stats, "height")
    cnt = tsv.trait_site_prefixes(chrom, pos, snp, a0, a1, af, np.float32([3.0, 2.5, 117.0]))
    w.put(cnt, stats[[2, 0]], "bmi 2", np.array([2, 0]))
    assert w.close() == 5
    want = ("chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\tphenotype\n"
            "1\t100\trs1\tA\tG\t0.1235\t0.0123\t0.1234\t0.0500\t6.0957e0\t1.3554e-2\theight\n"
            "X\t2000\t.\tAT\tA\t0.5000\t0.0000\tNaN\tNaN\tNaN\t1.0000e0\theight\n"
            "2\t5\trs3\tG\tT\t1.0000\t1.0000\t-2.5000\t0.2500\tinf\t9.9999e-321\theight\n"
            "2\t5\trs3\tG\tT\t1.0000\t117\t-2.5000\t0.2500\tinf\t9.9999e-321\tbmi 2\n"
            "1\t100\trs1\tA\tG\t0.1235\t3\t0.1234\t0.0500\t6.0957e0\t1.3554e-2\tbmi 2\n")
    assert open(path, "rb").read() == want.encode()
    assert cnt[1].split("\t")[6] == "3"                      # 2.5 rounds away from zero, as Rust's f32::round
    assert [f.name for f in tmp_path.iterdir()] == ["t.lm.tsv"]          # written through a temporary file and renamed


def test_traits_are_grouped_by_sample_mask():
    from janusx_amd import cli
    masks = {4: [0, 1, 2, 5], 1: [0, 1, 2], 7: [0, 1, 2, 5], 2: [0, 1, 2], 9: [3]}
    groups = cli.group_traits_by_samples([4, 1, 7, 2, 9], lambda ti: np.array(masks[ti], dtype=np.int64))
    assert [(list(k), members) for k, members in groups] == [([0, 1, 2, 5], [4, 7]), ([0, 1, 2], [1, 2]), ([3], [9])]


@pytest.fixture()
def tiny_prefix(tmp_path):
    from janusx_amd import bed
    n, m = 12, 6
    g = np.random.default_rng(0).integers(0, 3, size=(m, n)).astype(np.int8)
    pre = str(tmp_path / "tiny")
    bed.write_bed(pre, bed.pack_dosage(g), [f"s{i}" for i in range(n)],
                  bed.Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * m, ["G"] * m))
    return pre, n, m


def test_mirrors_validate_before_any_device_work(tiny_prefix, tmp_path, monkeypatch):
    from janusx_amd import _lib
    from janusx_amd import janusx as jx

    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(jx, "lib", no_library)
    monkeypatch.setattr(jx, "_lmt_run", lambda *a, **k: no_library())
    pre, n, m = tiny_prefix
    out = str(tmp_path / "o.tsv")
    y = np.zeros((2, n))
    x = np.ones((n, 1))
    ok = dict(prefix=pre, trait_names=["a", "b"], y_trait_major=y, x=x, sample_indices=np.arange(n), row_indices=np.arange(m),
              row_flip=np.zeros(m, bool), row_missing=np.zeros(m, np.float32), row_maf=np.full(m, 0.3, np.float32), out_tsv=out)

    def matrix(match, **change):
        with pytest.raises(ValueError, match=match):
            jx.lm_trait_assoc_bed_matrix_to_tsv(**{**ok, **change})

    matrix("chunk_size must be > 0", chunk_size=0)
    matrix("mmap_window_mb must be > 0", mmap_window_mb=0)
    matrix("trait_names must not contain empty values", trait_names=["a", "  "])
    matrix(r"y_trait_major rows \(2\) must equal len\(trait_names\) \(3\)", trait_names=["a", "b", "c"])
    matrix("x must have at least one column", x=np.ones((n, 0)))
    matrix(r"x rows \(11\) must equal y_trait_major cols \(12\)", x=np.ones((n - 1, 1)))
    matrix(r"sample_indices length \(3\) must equal y_trait_major cols \(12\)", sample_indices=np.arange(3))
    matrix("prepared row metadata length mismatch: row_indices=6, row_flip=5, row_missing=6, row_maf=6", row_flip=np.zeros(5, bool))
    matrix("sample index 12 out of range for n_samples=12", sample_indices=np.arange(1, n + 1))
    matrix("row index 6 out of range for n_snps=6", row_indices=np.arange(1, m + 1))
    matrix("sorted in ascending BED order", row_indices=np.arange(m)[::-1].copy())
    assert jx.lm_trait_assoc_bed_matrix_to_tsv(**{**ok, "trait_names": [], "y_trait_major": np.zeros((0, n))}) == []

    spec = dict(trait_name="a", y=np.zeros(n), x=x, sample_indices=np.arange(n), row_indices=np.arange(m), row_flip=np.zeros(m, bool),
                row_missing=np.zeros(m, np.float32), row_maf=np.full(m, 0.3, np.float32))

    def specs(match, second=None, **change):
        with pytest.raises(ValueError, match=match):
            jx.lm_trait_assoc_bed_to_tsv(pre, [spec, {**spec, **change} if second is None else second], out)

    with pytest.raises(ValueError, match="chunk_size must be > 0"):
        jx.lm_trait_assoc_bed_to_tsv(pre, [spec], out, chunk_size=0)
    with pytest.raises(ValueError, match="trait_specs must be a list"):
        jx.lm_trait_assoc_bed_to_tsv(pre, (spec,), out)
    assert jx.lm_trait_assoc_bed_to_tsv(pre, [], out) == []
    specs(r"trait_specs\[1\] must be a dict", second=[1, 2])
    specs(r"trait_specs\[1\].trait_name must not be empty", trait_name=" ")
    specs(r"trait_specs\[1\].x must have at least one column", x=np.ones((n, 0)))
    specs(r"trait_specs\[1\] x rows \(5\) must equal len\(y\) \(12\)", x=np.ones((5, 1)))
    specs(r"trait_specs\[1\] sample_indices length \(4\) must equal len\(y\) \(12\)", sample_indices=np.arange(4))
    specs(r"trait_specs\[1\] sample index -1 out of range for n_samples=12", sample_indices=np.arange(-1, n - 1))
    specs(r"trait_specs\[1\] sample_ids length \(2\) must equal len\(y\) \(12\)", sample_indices=None, sample_ids=["s0", "s1"])
    specs(r"trait_specs\[1\] sample ID 'zz' not found in BED/FAM", sample_indices=None, sample_ids=["zz"] + [f"s{i}" for i in range(1, n)])
    specs(r"trait_specs\[1\] prepared row metadata length mismatch", row_maf=np.zeros(2, np.float32))
    specs(r"trait_specs\[1\] row index 9 out of range for n_snps=6", row_indices=np.array([0, 1, 2, 3, 4, 9]))
    specs(r"trait_specs\[1\] prepared row_indices must be sorted", row_indices=np.array([0, 1, 3, 2, 4, 5]))
    specs("missing required key 'row_flip'", row_flip=None)


def test_trait_level_needs_lm_and_two_traits(tiny_prefix, tmp_path, monkeypatch):
    from janusx_amd import cli
    monkeypatch.setattr(cli, "_dist_setup", lambda: pytest.fail("the run started"))
    pre, n, _m = tiny_prefix
    ph = str(tmp_path / "ph.tsv")
    with open(ph, "w") as fh:
        fh.write("id\tt1\tt2\n")
        for i in range(n):
            fh.write(f"s{i}\t{i * 0.5}\t{i % 3}\n")
    with pytest.raises(SystemExit, match="the LM trait-level route requires -lm"):
        cli.main(["gwas", "-bfile", pre, "-p", ph, "-lmm", "-trait-level"])
    with pytest.raises(SystemExit, match="LM trait-level route requires at least 2 traits."):
        cli.main(["gwas", "-bfile", pre, "-p", ph, "-lm", "-trait-level", "-n", "t2"])
    with pytest.raises(SystemExit, match="-trait-pmax belongs to -trait-level"):
        cli.main(["gwas", "-bfile", pre, "-p", ph, "-lm", "-trait-pmax", "0.01"])
    with pytest.raises(SystemExit, match=r"-trait-pmax must be within \[0, 1\]"):
        cli.main(["gwas", "-bfile", pre, "-p", ph, "-lm", "-trait-level", "-trait-pmax", "2"])
