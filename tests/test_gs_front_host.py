"""Argument front end of the genomic-selection mirrors (`rrblup_pcg_bed`, `rrblup_exact_snp_packed`, `he_pcg_bed`,
`gblup_reml_grm`, `gblup_reml_packed_bed`, `gblup_effect_from_meta_stream`): every refusal below is raised before the library is
touched, so this file runs without a GPU.  The table pins exception type, message text and which check fires first; the
prepared inputs (kept rows, row standardisation, value table) are compared bit for bit with a restatement of the reference's
rule written out here."""
import numpy as np
import pytest

from janusx_amd import bed
from janusx_amd import janusx as jx
from janusx_amd import stats as st

N, M = 10, 6
PACKED = np.zeros((M, 3), dtype=np.uint8)
MAF = np.full(M, 0.2, dtype=np.float32)
FLIP = np.arange(M) == 1
TR = np.arange(8)
Y = np.arange(8.0)
PFX = "<prefix>"                  # stands for the six-variant, ten-sample fileset of the `prefix` fixture
ROWS = np.array([0, 2, 3])
NAN, INF = float("nan"), float("inf")
F5, T5 = np.zeros(5, dtype=np.float32), np.zeros(5, dtype=bool)
Y_NAN = np.where(np.arange(8) == 3, NAN, Y)
TR_10 = np.array([0, 1, 2, 3, 4, 5, 6, 10])
TOGETHER = "rrBLUP standardization requires row_mean and row_inv_sd together when overriding row stats."


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gsfront") / "six")
    bim = bed.Bim(["1"] * M, [f"rs{j}" for j in range(M)], list(range(1, M + 1)), ["A"] * M, ["C"] * M)
    bed.write_bed(p, PACKED, [f"s{i}" for i in range(N)], bim)
    return p


def _case(fn, base, over):
    kw = dict(base)
    kw.update(over)
    return fn, kw


def pcg(**over):
    return _case("rrblup_pcg_bed", dict(prefix="", train_sample_indices=TR, y_train=Y, packed=PACKED, packed_n_samples=N,
                                        maf=MAF, row_flip=FLIP), over)


def pcg_stream(**over):
    return pcg(**dict(dict(prefix=PFX, packed=None), **over))


def exact(**over):
    return _case("rrblup_exact_snp_packed", dict(packed=PACKED, n_samples=N, train_sample_indices=TR, y_train=Y, maf=MAF,
                                                 row_flip=FLIP), over)


def he(**over):
    return _case("he_pcg_bed", dict(prefix="", train_sample_indices=TR, y_train=Y, packed=PACKED, packed_n_samples=N, maf=MAF,
                                    row_flip=FLIP), over)


def he_meta(**over):
    return he(**dict(dict(prefix=PFX, packed=None, packed_n_samples=0, row_source_indices=ROWS, maf=MAF[:3],
                          row_flip=FLIP[:3]), **over))


def grm(**over):
    return _case("gblup_reml_grm", dict(grm=np.eye(N), train_sample_indices=TR, y_train=Y), over)


def gb(**over):
    return _case("gblup_reml_packed_bed", dict(prefix=PFX, train_sample_indices=TR, y_train=Y, row_source_indices=ROWS,
                                               row_flip=FLIP[:3], row_maf=MAF[:3]), over)


E = RuntimeError
Z6 = np.zeros(M, dtype=np.float32)
# (call, exception type, full message), as observed on the commit before the shared front end: one row per bad call
TABLE = [
    (pcg(max_iter=0), E, "max_iter must be > 0"),
    (pcg(tol=NAN), E, "tol must be finite and > 0"),
    (pcg(std_eps=0.0), E, "std_eps must be finite and > 0"),
    (pcg(lambda_value=-1.0), E, "lambda_value must be finite and >= 0"),
    (pcg(tol=NAN, maf=None), E, "tol must be finite and > 0"),
    (pcg(maf=None), E, "rrblup_pcg_bed: packed payload path requires `maf` argument."),
    (pcg(row_flip=None), E, "rrblup_pcg_bed: packed payload path requires `row_flip` argument."),
    (pcg(packed_n_samples=0), E, "rrblup_pcg_bed: packed payload path requires packed_n_samples > 0."),
    (pcg(packed=np.zeros(M, dtype=np.uint8)), E, "packed BED payload must be 2D (m, bytes_per_snp)."),
    (pcg_stream(maf=None), E, "rrblup_pcg_bed: streaming stats path requires `maf` argument."),
    (pcg_stream(row_flip=None), E, "rrblup_pcg_bed: streaming stats path requires `row_flip` argument."),
    (pcg_stream(packed_n_samples=0), E, "rrblup_pcg_bed: streaming stats path requires packed_n_samples > 0."),
    (pcg_stream(prefix=" "), E, "rrblup_pcg_bed: streaming stats path requires non-empty prefix."),
    (pcg_stream(packed_n_samples=9), E, "packed_n_samples mismatch: got 9, BED has 10"),
    (pcg(packed=PACKED[:0], maf=MAF[:0], row_flip=FLIP[:0]), E, "No SNP rows found in BED input."),
    (pcg(packed=PACKED[:, :2]), E, "packed second dimension mismatch: got 2, expected 3"),
    (pcg(maf=F5), E, "maf length mismatch: got 5, expected 6"),
    (pcg(row_flip=T5), E, "row_flip length mismatch: got 5, expected 6"),
    (pcg(site_keep=np.ones(5, dtype=bool)), E, "site_keep length mismatch: got 5, expected 6"),
    (pcg(site_keep=np.zeros(M, dtype=bool)), E, "No SNPs remained after applying site_keep mask."),
    (pcg(site_keep=np.zeros(M, dtype=bool), train_sample_indices=TR[:0]), E, "No SNPs remained after applying site_keep mask."),
    (pcg(train_sample_indices=TR[:0], y_train=Y[:0]), E, "train_sample_indices must not be empty."),
    (pcg(train_sample_indices=TR_10), E, "train_sample_indices out of range"),
    (pcg(y_train=Y[:7]), E, "y_train length mismatch: got 7, expected 8"),
    (pcg(y_train=Y_NAN), E, "y_train contains non-finite values."),
    (pcg(y_train=Y_NAN, row_mean=MAF), E, "y_train contains non-finite values."),
    (pcg(test_sample_indices=np.array([9, 10])), E, "test_sample_indices out of range"),
    (pcg(train_pred_local_indices=np.array([0, 8])), E, "train_pred_local_indices out of range"),
    (pcg(row_mean=MAF), E, TOGETHER),
    (pcg(row_inv_sd=MAF), E, TOGETHER),
    (pcg(row_mean=MAF[:4], row_inv_sd=MAF[:4]), E,
     "External row_mean/row_inv_sd length mismatch: mean=4, inv=4, expected active=6 or full=6."),
    (pcg(site_keep=FLIP, row_mean=F5, row_inv_sd=F5), E,
     "External row_mean/row_inv_sd length mismatch: mean=5, inv=5, expected active=1 or full=6."),
    (pcg(row_mean=MAF, row_inv_sd=Z6), E, "rrBLUP standardization received zero effective markers from external row_inv_sd."),

    (exact(n_samples=0), E, "n_samples must be > 0"),
    (exact(log10_lambda_low=-INF), E, "rrblup_exact_snp_packed requires finite log10(lambda) bounds."),
    (exact(log10_lambda_high=INF), E, "rrblup_exact_snp_packed requires finite log10(lambda) bounds."),
    (exact(reml_tol=0.0), E, "rrblup_exact_snp_packed requires finite reml_tol > 0."),
    (exact(reml_max_iter=0), E, "rrblup_exact_snp_packed requires reml_max_iter > 0."),
    (exact(std_eps=NAN), E, "rrblup_exact_snp_packed requires finite std_eps > 0."),
    (exact(reml_tol=0.0, maf=None), E, "rrblup_exact_snp_packed requires finite reml_tol > 0."),
    (exact(packed=np.zeros(M, dtype=np.uint8)), E, "packed must be 2D (m, bytes_per_snp)."),
    (exact(packed=PACKED[:, :2]), E, "packed second dimension mismatch: got 2, expected 3"),
    (exact(maf=None), E, "rrblup_exact_snp_packed requires `maf` argument."),
    (exact(row_flip=None), E, "rrblup_exact_snp_packed requires `row_flip` argument."),
    (exact(maf=F5), E, "maf length mismatch: got 5, expected 6"),
    (exact(row_flip=T5), E, "row_flip length mismatch: got 5, expected 6"),
    (exact(site_keep=np.ones(5, dtype=bool)), E, "site_keep length mismatch: got 5, expected 6"),
    (exact(site_keep=np.zeros(M, dtype=bool)), E, "No SNPs remained after applying site_keep mask."),
    (exact(packed=PACKED[:0], maf=MAF[:0], row_flip=FLIP[:0]), E, "rrblup_exact_snp_packed received zero active markers."),
    (exact(train_sample_indices=TR[:1], y_train=Y[:1]), E, "rrblup_exact_snp_packed requires at least two training samples."),
    (exact(train_sample_indices=TR[:0], y_train=Y[:0]), E, "rrblup_exact_snp_packed requires at least two training samples."),
    (exact(train_sample_indices=TR_10), E, "train_sample_indices out of range"),
    (exact(train_sample_indices=np.array([10]), y_train=Y[:1]), E, "train_sample_indices out of range"),
    (exact(y_train=Y[:7]), E, "y_train length mismatch: got 7, expected 8"),
    (exact(y_train=Y_NAN), E, "y_train contains non-finite values."),
    (exact(test_sample_indices=np.array([-1])), E, "test_sample_indices out of range"),
    (exact(train_pred_local_indices=np.array([8])), E, "train_pred_local_indices out of range"),
    (exact(row_mean=MAF), E, TOGETHER),
    (exact(row_mean=MAF[:4], row_inv_sd=MAF[:4]), E,
     "External row_mean/row_inv_sd length mismatch: mean=4, inv=4, expected active=6 or full=6."),
    (exact(site_keep=FLIP, row_mean=F5, row_inv_sd=F5), E,
     "External row_mean/row_inv_sd length mismatch: mean=5, inv=5, expected active=1 or full=6."),
    (exact(row_mean=MAF, row_inv_sd=Z6), E, "rrblup_exact_snp_packed found zero effective markers after standardization."),
    (exact(maf=Z6), E, "rrblup_exact_snp_packed found zero effective markers after standardization."),

    (he(trace_samples=0), E, "trace_samples must be > 0"),
    (he(trace_probe_batch=0), E, "trace_probe_batch must be > 0"),
    (he(max_iter=0), E, "max_iter must be > 0"),
    (he(tol=0.0), E, "tol must be finite and > 0"),
    (he(std_eps=0.0), E, "std_eps must be finite and > 0"),
    (he(tol=0.0, row_source_indices=ROWS), E, "tol must be finite and > 0"),
    (he(row_source_indices=ROWS), E,
     "he_pcg_bed: provide either packed payload inputs or row_source_indices metadata streaming inputs, not both."),
    (he(packed=None, packed_n_samples=0), E,
     "he_pcg_bed: external maf/row_flip without packed payload requires row_source_indices for metadata streaming."),
    (he(packed=None), E, "he_pcg_bed: packed payload path requires `packed` argument."),
    (he(maf=None), E, "he_pcg_bed: packed payload path requires `maf` argument."),
    (he(row_flip=None), E, "he_pcg_bed: packed payload path requires `row_flip` argument."),
    (he(packed_n_samples=0), E, "he_pcg_bed: packed payload path requires packed_n_samples > 0."),
    (he(packed=np.zeros(M, dtype=np.uint8)), E, "packed BED payload must be 2D (m, bytes_per_snp)."),
    (he_meta(site_keep=np.ones(M, dtype=bool)), E,
     "he_pcg_bed: metadata streaming path does not accept site_keep; subset rows via row_source_indices instead."),
    (he_meta(maf=None), E, "he_pcg_bed: metadata streaming path requires `maf` argument."),
    (he_meta(row_flip=None), E, "he_pcg_bed: metadata streaming path requires `row_flip` argument."),
    (he_meta(row_source_indices=ROWS[:0], maf=MAF[:0], row_flip=FLIP[:0]), E,
     "row_source_indices must not be empty for metadata streaming path."),
    (he_meta(row_source_indices=np.array([-1, 2, 3])), E, "row_source_indices must be non-negative."),
    (he_meta(row_source_indices=np.array([0, 2, 6])), E, "row source index out of bounds"),
    (he_meta(maf=MAF[:2]), E, "metadata length mismatch between row_source_indices, maf and row_flip"),
    (he_meta(row_flip=FLIP[:2]), E, "metadata length mismatch between row_source_indices, maf and row_flip"),
    (he(packed=PACKED[:0], maf=MAF[:0], row_flip=FLIP[:0]), E, "No SNP rows found in BED input."),
    (he(packed=PACKED[:, :2]), E, "packed second dimension mismatch: got 2, expected 3"),
    (he(maf=F5), E, "maf length mismatch: got 5, expected 6"),
    (he(row_flip=T5), E, "row_flip length mismatch: got 5, expected 6"),
    (he(site_keep=np.ones(5, dtype=bool)), E, "site_keep length mismatch: got 5, expected 6"),
    (he(site_keep=np.zeros(M, dtype=bool)), E, "No SNPs remained after applying site_keep mask."),
    (he(train_sample_indices=TR[:0], y_train=Y[:0]), E, "train_sample_indices must not be empty."),
    (he(train_sample_indices=TR_10), E, "train_sample_indices out of range"),
    (he(y_train=Y[:7]), E, "y_train length mismatch: got 7, expected 8"),
    (he(y_train=Y_NAN), E, "y_train contains non-finite values."),
    (he(x_cov=np.ones(8)), E, "x_cov must be 2D (n, p_cov)"),
    (he(x_cov=np.ones((8, 0))), E, "x_cov must have at least one column"),
    (he(x_cov=np.ones((3, 1))), E, "x_cov rows mismatch: got 3, expected either n_samples=10 or n_train=8"),
    (he(maf=np.where(np.arange(M) == 2, np.float32(NAN), MAF)), E, "row_maf contains non-finite values"),
    (he(maf=Z6, use_train_maf=False), E, "No effective SNPs after std_eps filtering"),

    (grm(g_eps=-1.0), E, "g_eps must be finite and >= 0"),
    (grm(low=2.0, high=1.0), E, "low/high must be finite and low < high"),
    (grm(max_iter=0), E, "max_iter must be > 0"),
    (grm(tol=0.0), E, "tol must be finite and > 0"),
    (grm(grm=np.ones((N, N - 1))), E, "GRM must be a square matrix"),
    (grm(y_train=Y[:7]), E, "y_train length must equal train_sample_indices length"),

    (gb(g_eps=-1.0), E, "g_eps must be finite and >= 0"),
    (gb(low=2.0, high=1.0), E, "low/high must be finite and low < high"),
    (gb(max_iter=0), E, "max_iter must be > 0"),
    (gb(tol=0.0), E, "tol must be finite and > 0"),
    (gb(tol=0.0, row_source_indices=ROWS[:0]), E, "tol must be finite and > 0"),
    (gb(row_source_indices=ROWS[:0], row_flip=FLIP[:0], row_maf=MAF[:0]), E,
     "row_source_indices must not be empty for metadata streaming path."),
    (gb(row_source_indices=np.array([-1, 2, 3])), E, "row_source_indices must be non-negative."),
    (gb(row_maf=MAF[:2]), E, "metadata length mismatch: row_source_indices=3, row_flip=3, row_maf=2"),
    (gb(row_flip=FLIP[:2]), E, "metadata length mismatch: row_source_indices=3, row_flip=2, row_maf=3"),
    (gb(row_source_indices=np.array([0, 2, 6])), E, "row_source_indices out of range"),
    (gb(train_sample_indices=TR[:0], y_train=Y[:0]), E, "train_sample_indices must not be empty."),
    (gb(train_sample_indices=TR_10), E, "train_sample_indices out of range"),
    (gb(y_train=Y[:7]), E, "y_train length mismatch: got 7, expected 8"),
    (gb(y_train=Y_NAN), E, "y_train contains non-finite values."),
    (gb(test_sample_indices=np.array([10])), E, "test_sample_indices out of range"),
    (gb(train_sample_indices=TR[:1], y_train=Y[:1]), E, "GBLUP REML requires at least 2 training samples."),
]


def _row_id(row):
    (fn, kw), _exc, _msg = row
    base = {"rrblup_pcg_bed": pcg, "rrblup_exact_snp_packed": exact, "he_pcg_bed": he, "gblup_reml_grm": grm,
            "gblup_reml_packed_bed": gb}[fn]()[1]
    changed = [k for k, v in kw.items() if k not in base or v is not base[k]]
    return fn + ":" + ",".join(changed)


@pytest.mark.parametrize("row", TABLE, ids=[f"{i:03d}-{_row_id(r)}" for i, r in enumerate(TABLE)])
def test_refusal_type_message_and_order(row, prefix):
    (fn, kw), exc, msg = row
    kw = {k: (prefix if isinstance(v, str) and v == PFX else v) for k, v in kw.items()}
    with pytest.raises(exc) as info:
        getattr(jx, fn)(**kw)
    assert type(info.value) is exc and str(info.value) == msg


# ---- prepared inputs ---------------------------------------------------------------------------------------------------------

def test_kept_rows():
    maf = np.linspace(0.05, 0.3, M).astype(np.float32)
    keep = np.array([False, True, True, False, True, True])
    rows, maf_keep, flip_keep = jx._gs_kept_rows(M, maf, FLIP, keep)
    assert rows.dtype == np.int64 and rows.tolist() == [1, 2, 4, 5]
    assert np.array_equal(maf_keep, maf[[1, 2, 4, 5]]) and maf_keep.dtype == np.float32
    assert np.array_equal(flip_keep, FLIP[[1, 2, 4, 5]]) and flip_keep.dtype == bool
    for all_rows in (None, np.ones(M, dtype=bool)):
        rows, maf_keep, flip_keep = jx._gs_kept_rows(M, maf, FLIP, all_rows)
        assert rows is None and np.array_equal(maf_keep, maf) and np.array_equal(flip_keep, FLIP)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _restated(maf, flip, std_eps):
    """The reference's rule (`rrblup_subset_or_validate_stats`, `rrblup_value_lut`), every operation in f32."""
    f32 = np.float32
    p = np.clip(maf.astype(f32), f32(0.0), f32(0.5))
    rm = f32(2.0) * p
    v = np.maximum(f32(2.0) * p * (f32(1.0) - p), f32(0.0))
    cut = f32(max(float(std_eps), 1e-12))
    ri = np.zeros(len(p), dtype=f32)
    for j in range(len(p)):
        if v[j] > cut:
            ri[j] = f32(1.0) / np.sqrt(v[j])
    return rm, ri, int(np.count_nonzero(ri)), _restated_lut(rm, ri, flip)


def _restated_lut(rm, ri, flip):
    f32 = np.float32
    lut = np.zeros((len(rm), 4), dtype=f32)
    for j in range(len(rm)):
        g0, g2 = (f32(2.0), f32(0.0)) if flip[j] else (f32(0.0), f32(2.0))
        lut[j] = [(g0 - rm[j]) * ri[j], f32(0.0), (f32(1.0) - rm[j]) * ri[j], (g2 - rm[j]) * ri[j]]
    return lut


def test_row_standardisation_and_value_table():
    maf = np.array([0.0, 1e-13, 0.2, 0.5, 0.7, 0.31], dtype=np.float32)
    flip = np.array([False, True, False, False, True, False])
    # the default cut (rows 0 and 1 fall under it); one below the 1e-12 floor; one that drops polymorphic rows as well
    for std_eps, n_eff in ((1e-12, 4), (1e-30, 4), (0.45, 2)):
        rm_ref, ri_ref, me_ref, lut_ref = _restated(maf, flip, std_eps)
        rm, ri, me = jx._rrblup_row_stats(maf, None, M, None, None, std_eps)
        assert me == me_ref == n_eff
        assert np.array_equal(_bits(rm), _bits(rm_ref)) and np.array_equal(_bits(ri), _bits(ri_ref))
        assert np.array_equal(_bits(st.grm_lut_from_mean_scale(rm, ri, flip)), _bits(lut_ref))
    # a subset: the statistics of the kept rows are those rows of the full statistics
    keep = np.array([False, True, True, False, True, True])
    rows, maf_keep, flip_keep = jx._gs_kept_rows(M, maf, flip, keep)
    rm_ref, ri_ref, _me, lut_ref = _restated(maf, flip, 1e-12)
    rm, ri, me = jx._rrblup_row_stats(maf_keep, rows, M, None, None, 1e-12)
    assert me == 3 and np.array_equal(_bits(rm), _bits(rm_ref[rows])) and np.array_equal(_bits(ri), _bits(ri_ref[rows]))
    assert np.array_equal(_bits(st.grm_lut_from_mean_scale(rm, ri, flip_keep)), _bits(lut_ref[rows]))
    # external statistics: of the active length as they are, of the full length through the kept rows
    ext_m = np.array([0.1, 0.4, 0.9, 1.0, 0.6, 0.62], dtype=np.float32)
    ext_i = np.array([2.0, 0.0, 1.5, NAN, 1.25, -1.0], dtype=np.float32)
    for em, ei, r, mk in ((ext_m[rows], ext_i[rows], rows, maf_keep), (ext_m, ext_i, rows, maf_keep), (ext_m, ext_i, None, maf)):
        rm, ri, me = jx._rrblup_row_stats(mk, r, M, em, ei, 1e-12)
        want_m, want_i = (ext_m, ext_i) if r is None else (ext_m[rows], ext_i[rows])
        assert np.array_equal(_bits(rm), _bits(want_m)) and np.array_equal(_bits(ri), _bits(want_i))
        assert me == int(np.count_nonzero(np.isfinite(want_i) & (want_i > 0)))
        fl = flip if r is None else flip_keep
        assert np.array_equal(_bits(st.grm_lut_from_mean_scale(rm, ri, fl)), _bits(_restated_lut(rm, ri, fl)))
