"""`jx adamixture -cverror` on the host: the switch's grammar and refusals, the fold hash (`admx_cv_fold_ids`) against the
published SplitMix64 outputs and a scalar restatement of `cv_fold_hash64` (src/stats/adamixture.rs:1641-1653), and the text of
the summary table."""

import argparse

import numpy as np
import pytest

from janusx_amd import cli
from janusx_amd import janusx as jx

U64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def _args(*argv):
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli._add_admixture_parser(sub, "adamixture")
    cli._add_admixture_parser(sub, "fastpop")
    return ap.parse_args(list(argv))


def _hash(flat, seed):
    """Python integers, masked to 64 bits after every multiplication."""
    x = (flat ^ ((seed & U64) ^ GOLDEN)) & U64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & U64
    return x ^ (x >> 31)


def test_cverror_parsing():
    assert _args("adamixture", "-bfile", "x", "-k", "2").cverror is None
    assert _args("adamixture", "-bfile", "x", "-k", "2", "-cverror").cverror == 5
    assert _args("adamixture", "-bfile", "x", "-cverror", "-k", "2").cverror == 5
    assert _args("fastpop", "-bfile", "x", "-k", "2", "-cverror", "3").cverror == 3
    assert _args("fastpop", "-bfile", "x", "-k", "2", "--cverror", "0").cverror == 0
    for argv in (("-cverror",), ("-cverror", "3"), ("-cverror", "0"), ("-cverror", "2"), ("-cverror", "256"), ("-cv", "0")):
        assert cli._admx_check_args(_args("adamixture", "-bfile", "x", "-k", "2..3", *argv)) == [2, 3]


@pytest.mark.parametrize("n", ["1", "300", "257", "-2"])
def test_cverror_out_of_range(n):
    with pytest.raises(SystemExit, match=f"-cverror {n}.*256"):
        cli._admx_check_args(_args("adamixture", "-bfile", "x", "-k", "2", "-cverror", n))


def test_cv_points_to_cverror():
    with pytest.raises(SystemExit) as e:
        cli._admx_check_args(_args("adamixture", "-bfile", "x", "-k", "2", "-cv", "5"))
    assert "-cv 5" in str(e.value) and "-cverror 5" in str(e.value)
    assert cli.ADMX_CV_MAX_FOLDS == jx.ADMX_CV_MAX_FOLDS == 256


def test_fold_hash_published_vectors():
    """The first two outputs of SplitMix64 from the state 0: with seed 0 the key is the golden increment G, so the flat indices
    0 and G ^ 2G hash the states G and 2G."""
    assert _hash(0, 0) == 0xE220A8397B1DCDAF
    assert _hash(GOLDEN ^ ((2 * GOLDEN) & U64), 0) == 0x6E789E6AA1B965F4
    flat = np.array([0, GOLDEN ^ ((2 * GOLDEN) & U64)], dtype=np.uint64)
    for folds in (2, 3, 5, 7, 256, 1000003):
        want = [0xE220A8397B1DCDAF % folds, 0x6E789E6AA1B965F4 % folds]
        assert jx.admx_cv_fold_ids(flat, folds, 0).tolist() == want


@pytest.mark.parametrize("seed", [0, 42, U64, -1, (1 << 63) + 5])
def test_fold_ids_equal_the_formula(seed):
    rng = np.random.default_rng(3)
    flat = np.concatenate([np.arange(0, 300, dtype=np.uint64), rng.integers(0, 1 << 62, 200).astype(np.uint64),
                           np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345, (1 << 63) + 7, U64], dtype=np.uint64)])
    for folds in (2, 3, 5, 10, 255, 256):
        got = jx.admx_cv_fold_ids(flat, folds, seed)
        assert got.dtype == np.int64 and got.shape == flat.shape
        assert got.tolist() == [_hash(int(f), seed) % folds for f in flat]
    assert jx.admx_cv_fold_ids(flat.reshape(2, -1), 5, seed).shape == (2, flat.size // 2)


def test_seed_is_taken_mod_2_64():
    flat = np.arange(1000, dtype=np.uint64)
    assert np.array_equal(jx.admx_cv_fold_ids(flat, 5, -1), jx.admx_cv_fold_ids(flat, 5, U64))
    assert np.array_equal(jx.admx_cv_fold_ids(flat, 5, (1 << 64) + 42), jx.admx_cv_fold_ids(flat, 5, 42))
    assert not np.array_equal(jx.admx_cv_fold_ids(flat, 5, 42), jx.admx_cv_fold_ids(flat, 5, 43))
    share = np.bincount(jx.admx_cv_fold_ids(np.arange(100000, dtype=np.uint64), 5, 42), minlength=5) / 100000.0
    assert np.all(np.abs(share - 0.2) < 0.01)                      # 6 sd of a fair fifth is 0.0076


def test_summary_table_text(tmp_path):
    rows = [dict(k=2, cverror=0.9451234, cverror_se=0.00123449, cv_folds=3, wall=1.23456, q_out="o/p.2.Q.txt",
                 p_npy_out="o/p.2.P.npy", p_site_out="o/p.2.P.site", log_path="o/p.2.fastpop.log"),
            dict(k=3, cverror=0.8710006, cverror_se=0.0, cv_folds=3, wall=12.0, q_out="o/p.3.Q.txt", p_npy_out="o/p.3.P.npy",
                 p_site_out="o/p.3.P.site", log_path="o/p.3.fastpop.log")]
    path = tmp_path / "p.fastpop.cverror.summary.tsv"
    cli.write_cverror_summary_tsv(str(path), rows)
    assert path.read_text() == (
        "K\tCVerror\tCVerror_SE\tCV_folds\tWallTime_sec\tQ_output\tP_npy_output\tP_site_output\tStructure_plot\tLog_file\n"
        "2\t0.945123\t0.001234\t3\t1.235\to/p.2.Q.txt\to/p.2.P.npy\to/p.2.P.site\t\to/p.2.fastpop.log\n"
        "3\t0.871001\t0.000000\t3\t12.000\to/p.3.Q.txt\to/p.3.P.npy\to/p.3.P.site\t\to/p.3.fastpop.log\n")


def test_session_refusals_need_no_device():
    """The range checks of the fold arguments run before anything touches the device."""
    with pytest.raises(RuntimeError, match="CVerror requires folds >= 2, got 1"):
        jx._admx_cv_check(1)
    with pytest.raises(RuntimeError, match="at most 256"):
        jx._admx_cv_check(257)
    with pytest.raises(RuntimeError, match=r"fold_id must be within \[0, 3\), got 3"):
        jx._admx_cv_check(3, 3)
    assert jx._admx_cv_check(256, 255) == 256
    with pytest.raises(ValueError, match="CVerror requires folds >= 2, got 1"):
        jx.admx_evaluate_cverror(None, 2, 1)
    with pytest.raises(ValueError, match="at most 256"):
        jx.admx_evaluate_cverror(None, 2, 257)
