"""Host-side parts of `jx pca`: the refusals of the command line and the deterministic start block of the randomized SVD."""
import numpy as np
import pytest

from janusx_amd import bed, cli
from janusx_amd.janusx import rsvd_omega


def _tiny_bed(tmp_path):
    g = np.random.default_rng(0).integers(0, 3, (30, 12))
    prefix = str(tmp_path / "t")
    bim = bed.Bim(["1"] * 30, [f"rs{j}" for j in range(30)], list(range(1, 31)), ["A"] * 30, ["G"] * 30)
    bed.write_bed(prefix, bed.pack_dosage(g), [f"s{i}" for i in range(12)], bim)
    return prefix


def test_cli_pca_refusals(tmp_path, monkeypatch):
    prefix = _tiny_bed(tmp_path)
    bad = [["pca", "-vcf", "x.vcf"], ["pca", "-hmp", "x.hmp"], ["pca", "-file", "x.txt"],
           ["pca", "-bfile", prefix, "-plot"], ["pca", "-bfile", prefix, "-plot3D"], ["pca", "-bfile", prefix, "-c", "3"],
           ["pca", "-bfile", prefix, "-group", "g.tsv"], ["pca", "-bfile", prefix, "-palette", "x"],
           ["pca", "-k", prefix, "-rsvd"], ["pca", "-bfile", prefix, "-dim", "0"], ["pca", "-bfile", prefix, "-k", prefix],
           ["pca"], ["pca", "-bfile", prefix, "-rsvd", "1", "2", "3"], ["pca", "-bfile", prefix, "-rsvd", "-1"],
           ["pca", "-bfile", prefix, "-rsvd", "3", "0"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            cli.main(argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU"):
        cli.main(["pca", "-bfile", prefix])


def test_rsvd_omega_is_a_deterministic_standard_normal():
    a = rsvd_omega(42, 4000, 24)
    np.testing.assert_array_equal(a, rsvd_omega(42, 4000, 24))
    np.testing.assert_array_equal(a[:100, :5], rsvd_omega(42, 100, 24)[:, :5])      # entry (r, c) depends on (seed, r, c) only
    assert not np.array_equal(a, rsvd_omega(43, 4000, 24))
    assert abs(a.mean()) < 0.01 and abs(a.std() - 1.0) < 0.01


def test_product_entry_points_refuse_before_any_device_work():
    """`jxg_packed_mm_cols` / `jxg_packed_tmm_cols` check kp and the sample count (exact i32 plane sums up to 2^23 samples)
    before they touch a pointer or the device: called here with null pointers on a machine without a GPU."""
    from janusx_amd._lib import check, lib
    with pytest.raises(RuntimeError, match=r"jxg_packed_mm_cols: kp must be >= 1"):
        check(lib().jxg_packed_mm_cols(None, 10, 10, None, 10, None, None, 0, None, None))
    with pytest.raises(RuntimeError, match=r"jxg_packed_tmm_cols: kp must be >= 1"):
        check(lib().jxg_packed_tmm_cols(None, 10, 10, None, None, 0, None, None))
    with pytest.raises(RuntimeError, match=r"jxg_packed_mm_cols: at most 8 388 608 samples \(exact i32 plane sums\)"):
        check(lib().jxg_packed_mm_cols(None, 10, (1 << 23) + 1, None, 10, None, None, 1, None, None))
    # an empty row list or panel is a no-op at the limit itself, not a refusal
    assert lib().jxg_packed_mm_cols(None, 10, 1 << 23, None, 0, None, None, 1, None, None) == 0
    assert lib().jxg_packed_tmm_cols(None, 0, 10, None, None, 1, None, None) == 0


def test_admx_rsvd_refuses_out_of_range_thresholds(tmp_path):
    from janusx_amd.janusx import admx_rsvd_stream_sample
    prefix = _tiny_bed(tmp_path)
    for kw, msg in (({"maf": 0.6}, "maf"), ({"maf": -0.1}, "maf"), ({"missing_rate": 1.5}, "missing_rate"),
                    ({"missing_rate": -0.1}, "missing_rate")):
        with pytest.raises(RuntimeError, match=msg):
            admx_rsvd_stream_sample(prefix, 3, **kw)
