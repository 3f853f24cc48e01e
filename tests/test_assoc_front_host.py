"""Argument front end of the association mirrors (the null-model helpers, the exact, fixed-lambda and LMM2 chunk functions, the
packed scans, the BED -> TSV routes and the LM block and streaming scans): every refusal below is raised before the library or
the device is touched, so this file runs without a GPU.  The table pins exception type, message text and which check fires
first, as observed on the commit before the shared front end; the prepared values (Brent's start, the warm-start chain offsets,
the BIM columns of a row selection) are compared with a restatement written out here, and one test pins what the packed
scans hand on to `pipeline.scan_rows`."""
import numpy as np
import pytest

from janusx_amd import bed
from janusx_amd import janusx as jx

N, M = 10, 6
S = np.linspace(1.0, 2.0, N)
X2 = np.stack([np.ones(N), np.arange(float(N))], axis=1)
YR = np.arange(float(N)) - 4.0
UT = np.eye(N, dtype=np.float32)
G = np.zeros((M, N), dtype=np.float32)
PACKED = np.zeros((M, 3), dtype=np.uint8)
FLIP = np.zeros(M, dtype=bool)
MAF = np.full(M, 0.2, dtype=np.float32)
MISS = np.zeros(M, dtype=np.float32)
IXX = np.eye(2)
COV = np.arange(3.0 * N).reshape(N, 3)
PFX = "<prefix>"                  # stands for the six-variant, ten-sample fileset of the `prefix` fixture
IDS = [f"s{i}" for i in range(N)]
NAN, INF = float("nan"), float("inf")
UT9 = np.eye(9, dtype=np.float32)
X_WIDE = np.ones((N, 9))          # n <= p + 1
META = dict(chrom=["1"] * M, pos=list(range(1, M + 1)), snp=[f"rs{j}" for j in range(M)], allele0=["A"] * M, allele1=["C"] * M)
NO_META = dict(chrom=[], pos=[], snp=[], allele0=[], allele1=[])
ROWS3 = np.array([0, 2, 3])
PREP3 = dict(row_indices=ROWS3, row_flip=FLIP[:3], row_missing=MISS[:3], row_maf=MAF[:3])
ALL_OR_NONE = "prepared row metadata must provide all or none of: row_indices, row_flip, row_missing, row_maf"
GM = "model must be one of: add, dom, rec, het"
UT_MSG = "u_t must be (n, n) and row-major U^T"
UT_SHAPE_MSG = "u_t must be shape (n, n) and row-major U^T"
XCOV_MSG = "Xcov.n_rows must equal len(y_rot)"
DIM2 = "packed second dimension mismatch: got 2, expected 3"


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("assocfront") / "six")
    bim = bed.Bim(["1", "1", "2", "2", "X", "X"], [f"rs{j}" for j in range(M)], [11, 12, 23, 24, 35, 36],
                  ["A", "C", "G", "T", "AT", "A"], ["C", "A", "T", "G", "A", "N"])
    bed.write_bed(p, PACKED, IDS, bim)
    return p


BIM_COLUMNS = (["1", "1", "2", "2", "X", "X"], [11, 12, 23, 24, 35, 36], [f"rs{j}" for j in range(M)],
               ["A", "C", "G", "T", "AT", "A"], ["C", "A", "T", "G", "A", "N"])

BASES = {}


def _entry(fn, **base):
    BASES[fn] = base

    def make(**over):
        kw = dict(base)
        kw.update(over)
        return fn, kw
    return make


NULL = dict(s=S, xcov=X2, y_rot=YR)
rot_xy = _entry("lmm_rotate_x_y_with_ut_f64", u_t=UT, x=X2, y=YR)
rot_y = _entry("lmm_rotate_y_with_ut_f64", u_t=UT, y=YR)
null = _entry("lmm_reml_null_f32", **NULL, low=-5.0, high=5.0)
ml_null = _entry("ml_loglike_null_f32", **NULL, log10_lbd=0.0)
chunk = _entry("lmm_reml_chunk_f32", **NULL, low=-5.0, high=5.0, g_rot_chunk=G)
chunk_snp = _entry("lmm_reml_chunk_from_snp_f32", **NULL, low=-5.0, high=5.0, snp_chunk=G, u_t=UT)
fv = _entry("fvlmm_assoc_chunk_f32", **NULL, log10_lbd=0.0, g_rot_chunk=G)
fv_snp = _entry("fvlmm_assoc_chunk_from_snp_f32", **NULL, log10_lbd=0.0, snp_chunk=G, u_t=UT)
la = _entry("lmm_assoc_chunk_f32", **NULL, log10_lbd=0.0, g_rot_chunk=G)
la_snp = _entry("lmm_assoc_chunk_from_snp_f32", **NULL, log10_lbd=0.0, snp_chunk=G, u_t=UT)
prep = _entry("fvlmm_assoc_prepare_cache_f32", **NULL, log10_lbd=0.0)
CACHE = jx.fvlmm_assoc_prepare_cache_f32(S, X2, YR, 0.0)
wc = _entry("fvlmm_assoc_chunk_with_cache_f32", cache=CACHE, g_rot_chunk=G)
wc_snp = _entry("fvlmm_assoc_chunk_from_snp_with_cache_f32", cache=CACHE, snp_chunk=G, u_t=UT)
fv_tsv = _entry("fvlmm_assoc_chunk_from_snp_to_tsv_f32", **NULL, log10_lbd=0.0, snp_chunk=G, u_t=UT, **META, maf=MAF, miss=MISS)
l2 = _entry("lmm_reml_lmm2_chunk_from_snp_f32", **NULL, low=-5.0, high=5.0, snp_chunk=G, u_t=UT, nullml=-3.0)
PK = dict(packed=PACKED, n_samples=N, row_flip=FLIP, row_maf=MAF)
lp = _entry("lmm_reml_assoc_packed_f32", **PK, **NULL, u_t=UT)
fp = _entry("fvlmm_assoc_packed_f32", **PK, **NULL, u_t=UT, log10_lbd=0.0)
ap = _entry("_assoc_packed", **PK, **NULL, u_t=UT, sample_indices=None, row_indices=None)
BED = dict(bed_prefix=PFX, out_tsv="<unused>", **NULL, u_t=UT, maf_thr=0.02, miss_thr=0.05, het_thr=1.0)
lb = _entry("lmm_reml_assoc_bed_to_tsv_f32", **BED)
l2b = _entry("lmm_reml_lmm2_assoc_bed_to_tsv_f32", **BED, nullml=-3.0)
fb = _entry("fvlmm_assoc_bed_to_tsv_f32", **BED, log10_lbd=0.0)
lpt = _entry("lmm_reml_assoc_packed_f32_to_tsv", **PK, row_missing=MISS, **NULL, u_t=UT, **META, out_tsv="<unused>")
fpt = _entry("fvlmm_assoc_packed_f32_to_tsv", **PK, row_missing=MISS, u=np.eye(N, dtype=np.float32), s=S.astype(np.float32),
             y=YR, x=X2[:, 1:], sample_indices=None, low=-5.0, high=5.0, max_iter=50, tol=1e-3, tau=0.0, threads=0, model="add",
             **META, out_tsv="<unused>")
LMB = dict(y=YR, x=X2, ixx=IXX)
lmp = _entry("lm_block_assoc_packed", **LMB, **PK)
lmd = _entry("lm_block_assoc_f32", **LMB, g=G)
lmt = _entry("lm_block_assoc_packed_to_tsv", **LMB, **PK, row_missing=MISS, **META, out_tsv="<unused>")
lms = _entry("lm_stream_bed_to_tsv", prefix=PFX, **LMB, out_tsv="<unused>")
lm2 = _entry("lm2_stream_bed_to_tsv", prefix=PFX, y=YR, x=X2, cov_all=COV, cov_indices=[0, 2], out_tsv="<unused>")

E, V, T = RuntimeError, ValueError, TypeError
# (call, exception type, full message), as observed on the commit before the shared front end: one row per bad call
TABLE = [
    (rot_xy(y=YR[:0]), E, "y must not be empty"),
    (rot_xy(x=YR), E, "x must be 2D (n, q)"),
    (rot_xy(x=YR, u_t=UT9), E, "x must be 2D (n, q)"),
    (rot_xy(x=X2[:9]), E, "x rows must equal len(y): rows=9, len(y)=10"),
    (rot_xy(u_t=UT9), E, UT_SHAPE_MSG),
    (rot_xy(u_t=UT[0]), E, UT_SHAPE_MSG),
    (rot_y(y=YR[:0]), E, "y must not be empty"),
    (rot_y(u_t=UT[0]), E, "u_t must be 2D (n, n)"),
    (rot_y(u_t=UT9), E, UT_SHAPE_MSG),

    (null(xcov=X2[:9]), E, XCOV_MSG),
    (null(xcov=YR), E, XCOV_MSG),
    (null(s=S[:9]), E, "len(S) must equal len(y_rot)"),
    (null(xcov=X2[:9], s=S[:9]), E, XCOV_MSG),
    (null(low=1.0, high=1.0), E, "low must be < high"),
    (null(low=1.0, high=1.0, xcov=X2[:9]), E, XCOV_MSG),
    (ml_null(s=S[:9]), E, "len(S) must equal len(y_rot)"),

    (chunk(xcov=X2[:9]), E, XCOV_MSG),
    (chunk(g_rot_chunk=G[:, :9]), E, "g_rot_chunk must be (m_chunk, n)"),
    (chunk(g_rot_chunk=G[0]), E, "g_rot_chunk must be (m_chunk, n)"),
    (chunk(low=2.0, high=1.0), E, "low must be < high"),
    (chunk(low=2.0, high=1.0, g_rot_chunk=G[0]), E, "g_rot_chunk must be (m_chunk, n)"),
    (chunk_snp(snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (chunk_snp(u_t=UT9), E, UT_MSG),
    (chunk_snp(u_t=UT9, snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (chunk_snp(low=2.0, high=1.0), E, "low must be < high"),
    (chunk_snp(low=2.0, high=1.0, u_t=UT9), E, UT_MSG),

    (fv(s=S[:9]), E, "len(S) must equal len(y_rot)"),
    (fv(g_rot_chunk=G[:, :9]), E, "g_rot_chunk must be (m_chunk, n)"),
    (fv_snp(snp_chunk=G[0]), E, "snp_chunk must be (m_chunk, n)"),
    (fv_snp(u_t=UT9), E, UT_MSG),
    (fv_snp(u_t=UT9, snp_chunk=G[0]), E, "snp_chunk must be (m_chunk, n)"),

    (la(xcov=X2[:9]), E, XCOV_MSG),
    (la(xcov=X_WIDE), E, "n must be > p_cov+1"),
    (la(log10_lbd=400.0), E, "invalid log10_lbd"),
    (la(log10_lbd=-400.0), E, "invalid log10_lbd"),
    (la(log10_lbd=NAN), E, "invalid log10_lbd"),
    (la(s=S - 3.0), E, "non-positive s[i]+lbd"),
    (la(xcov=X_WIDE, log10_lbd=NAN), E, "n must be > p_cov+1"),
    (la(log10_lbd=NAN, g_rot_chunk=G[0]), E, "invalid log10_lbd"),
    (la(g_rot_chunk=G[:, :9]), E, "g_rot_chunk must be (m_chunk, n)"),
    (la_snp(s=S - 3.0), E, "non-positive s[i]+lbd"),
    (la_snp(snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (la_snp(u_t=UT9), E, UT_MSG),
    (la_snp(u_t=UT9, log10_lbd=400.0), E, "invalid log10_lbd"),

    (prep(xcov=X2[:9]), E, XCOV_MSG),
    (prep(xcov=X_WIDE), E, "n must be > p_cov+1"),
    (prep(log10_lbd=INF), E, "invalid log10_lbd"),
    (prep(s=-S), E, "non-positive s[i]+lbd"),
    (wc(cache=None), T, "cache must come from fvlmm_assoc_prepare_cache_f32"),
    (wc(cache=None, g_rot_chunk=G[0]), T, "cache must come from fvlmm_assoc_prepare_cache_f32"),
    (wc(g_rot_chunk=G[:, :9]), E, "g_rot_chunk must be (m_chunk, n)"),
    (wc_snp(cache=(S, X2, YR, 0.0)), T, "cache must come from fvlmm_assoc_prepare_cache_f32"),
    (wc_snp(snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (wc_snp(u_t=UT9), E, UT_MSG),

    (fv_tsv(xcov=X_WIDE), E, "n must be > p_cov+1"),
    (fv_tsv(log10_lbd=400.0), E, "invalid log10_lbd"),
    (fv_tsv(snp_chunk=G[:, :9]), E, "snp_chunk must be (m, n)"),
    (fv_tsv(snp_chunk=G[0]), E, "snp_chunk must be (m, n)"),
    (fv_tsv(snp_chunk=G[0], log10_lbd=400.0), E, "invalid log10_lbd"),
    (fv_tsv(maf=MAF[:5]), E, "TSV metadata length mismatch with snp_chunk rows"),
    (fv_tsv(chrom=[]), E, "TSV metadata length mismatch with snp_chunk rows"),
    (fv_tsv(u_t=UT9), E, UT_MSG),
    (fv_tsv(u_t=UT9, miss=MISS[:5]), E, "TSV metadata length mismatch with snp_chunk rows"),

    (l2(xcov=X2[:9]), E, XCOV_MSG),
    (l2(snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (l2(u_t=UT9), E, UT_MSG),
    (l2(u_t=None), E, UT_MSG),
    (l2(low=5.0, high=-5.0), E, "low must be < high"),
    (l2(nullml=NAN), E, "nullml must be finite"),
    (l2(nullml=INF), E, "nullml must be finite"),
    (l2(u_t=UT9, snp_chunk=G[:, :9]), E, "snp_chunk must be (m_chunk, n)"),
    (l2(u_t=UT9, low=5.0, high=-5.0), E, UT_MSG),
    (l2(nullml=NAN, low=5.0, high=-5.0), E, "low must be < high"),

    (lp(low=5.0, high=5.0), E, "low must be < high"),
    (lp(tol=0.0), E, "tol must be positive and finite"),
    (lp(tol=NAN), E, "tol must be positive and finite"),
    (lp(tol=INF), E, "tol must be positive and finite"),
    (lp(low=5.0, high=5.0, tol=0.0), E, "low must be < high"),
    (lp(tol=0.0, u_t=UT9), E, "tol must be positive and finite"),
    (lp(low=5.0, high=5.0, packed=PACKED[:, :2]), E, "low must be < high"),
    (lp(warm_start="sometimes"), E, "warm_start must be 'chain' or 'none'"),
    (lp(warm_start="sometimes", tol=0.0), E, "tol must be positive and finite"),
    (lp(warm_chain_pieces=3, warm_start="chain"), E, "warm_chain_pieces must be a power of two >= 1"),
    (lp(warm_chain_pieces=0, warm_start="chain"), E, "warm_chain_pieces must be a power of two >= 1"),
    (lp(warm_chain_pieces=3, warm_start="chain", model="mult"), E, "warm_chain_pieces must be a power of two >= 1"),
    (lp(model="mult"), E, GM),
    (lp(model="mult", xcov=X2[:9]), E, GM),
    (lp(xcov=X2[:9]), E, XCOV_MSG),
    (lp(s=S[:9]), E, "len(S) must equal len(y_rot)"),
    (lp(packed=PACKED[0]), E, "packed must be 2D (m, bytes_per_snp)"),
    (lp(packed=PACKED[:, :2]), E, DIM2),
    (lp(packed=PACKED[:, :2], u_t=UT9), E, DIM2),
    (lp(packed=PACKED[:, :2], row_indices=ROWS3), E, DIM2),
    (lp(u_t=UT9), E, UT_MSG),
    (lp(sample_indices=np.arange(9)), E, "selected sample count 9 != len(y_rot) 10"),
    (lp(sample_indices=np.arange(9), u_t=UT9), E, UT_MSG),
    (lp(n_samples=0, packed=PACKED[:, :0], sample_indices=np.arange(N)), E, "n_samples must be > 0"),
    (ap(mode="lmm", low=-5.0, high=5.0, max_iter=50, tol=1e-2, chain_off=np.array([0])), E, "chain offsets are required"),
    (ap(mode="lmm", low=-5.0, high=5.0, max_iter=50, tol=1e-2, chain_off=np.array([0, 3, 5])), E,
     "chain offsets must run from 0 to m"),
    (ap(mode="lmm", low=-5.0, high=5.0, max_iter=50, tol=1e-2, chain_off=np.array([0, 4, 3, 6])), E, "chain offsets must ascend"),
    (ap(mode="lmm", low=5.0, high=-5.0, max_iter=50, tol=1e-2, chain_off=np.array([0])), E, "chain offsets are required"),
    (ap(mode="lmm", low=5.0, high=-5.0, max_iter=50, tol=1e-2), E, "low must be < high"),
    (ap(mode="lmm", low=-5.0, high=5.0, max_iter=50, tol=0.0), E, "tol must be positive and finite"),
    (ap(mode="lmm2", low=-5.0, high=5.0, max_iter=50, tol=1e-2), E, "nullml must be finite"),
    (ap(mode="lmm2", low=-5.0, high=5.0, max_iter=50, tol=1e-2, nullml=NAN), E, "nullml must be finite"),
    (ap(mode="lmm2", low=5.0, high=-5.0, max_iter=50, tol=1e-2, nullml=NAN), E, "nullml must be finite"),

    (fp(xcov=X2[:9]), E, XCOV_MSG),
    (fp(packed=PACKED[0]), E, "packed must be 2D (m, bytes_per_snp)"),
    (fp(packed=PACKED[:, :2]), E, DIM2),
    (fp(u_t=UT9), E, UT_MSG),
    (fp(sample_indices=np.arange(11)), E, "selected sample count 11 != len(y_rot) 10"),
    (fp(n_samples=0, packed=PACKED[:, :0], sample_indices=np.arange(N)), E, "n_samples must be > 0"),

    (lb(low=1.0, high=0.0), E, "low must be < high"),
    (lb(tol=-1.0), E, "tol must be positive and finite"),
    (lb(warm_start="later"), E, "warm_start must be 'chain' or 'none'"),
    (lb(genetic_model="mult"), E, GM),
    (lb(nullml=NAN), E, "nullml must be finite when provided"),
    (lb(xcov=X2[:9]), E, XCOV_MSG),
    (lb(xcov=X_WIDE), E, "n must be > p+1"),
    (lb(tol=-1.0, genetic_model="mult"), E, "tol must be positive and finite"),
    (lb(genetic_model="mult", nullml=NAN), E, GM),
    (lb(nullml=NAN, xcov=X_WIDE), E, "nullml must be finite when provided"),
    (lb(xcov=X_WIDE, bed_prefix="<no such fileset>"), E, "n must be > p+1"),
    (l2b(low=1.0, high=0.0), E, "low must be < high"),
    (l2b(tol=0.0), E, "tol must be positive and finite"),
    (l2b(nullml=INF), E, "nullml must be finite when provided"),
    (l2b(nullml=INF, tol=0.0), E, "tol must be positive and finite"),
    (l2b(genetic_model="mult"), E, GM),
    (l2b(xcov=X2[:9]), E, XCOV_MSG),
    (l2b(xcov=X_WIDE), E, "n must be > p+1"),
    (fb(genetic_model="mult"), E, GM),
    (fb(nullml=NAN), E, "nullml must be finite when provided"),
    (fb(s=S[:9]), E, "len(S) must equal len(y_rot)"),
    (fb(xcov=X_WIDE), E, "n must be > p+1"),
    (fb(xcov=X_WIDE, genetic_model="mult"), E, GM),

    (lpt(low=5.0, high=5.0), E, "low must be < high"),
    (lpt(tol=0.0), E, "tol must be positive and finite"),
    (lpt(warm_start="sometimes"), E, "warm_start must be 'chain' or 'none'"),
    (lpt(model="mult"), E, GM),
    (lpt(packed=PACKED[:, :2]), E, DIM2),
    (lpt(u_t=UT9), E, UT_MSG),
    (lpt(u_t=UT9, **NO_META), E, UT_MSG),
    (lpt(sample_indices=np.arange(9)), E, "selected sample count 9 != len(y_rot) 10"),

    (fpt(low=5.0, high=5.0), E, "low must be < high"),
    (fpt(tol=0.0), E, "tol must be positive and finite"),
    (fpt(low=5.0, high=5.0, fixed_lbd=1.0, tol=0.0), E, "tol must be positive and finite"),
    (fpt(tau=-1.0), E, "tau must be finite and >= 0"),
    (fpt(tau=NAN), E, "tau must be finite and >= 0"),
    (fpt(n_samples=0), E, "n_samples must be > 0"),
    (fpt(model="mult"), E, GM),
    (fpt(model="mult", n_samples=0), E, "n_samples must be > 0"),
    (fpt(packed=PACKED[0]), E, "packed must be 2D (m, bytes_per_snp)"),
    (fpt(packed=PACKED[:, :2]), E, DIM2),
    (fpt(low=5.0, high=5.0, packed=PACKED[:, :2]), E, "low must be < high"),
    (fpt(model="mult", packed=PACKED[:, :2]), E, GM),
    (fpt(row_flip=FLIP[:5]), E, "row_flip length mismatch: got 5, expected 6"),
    (fpt(row_maf=MAF[:5]), E, "row_maf length mismatch: got 5, expected 6"),
    (fpt(row_missing=MISS[:5]), E, "row_missing length mismatch: got 5, expected 6"),
    (fpt(row_indices=ROWS3), E, "row_flip length mismatch: got 6, expected 3"),
    (fpt(row_flip=FLIP[:5], packed=PACKED[:, :2]), E, DIM2),
    (fpt(y=YR[:0]), E, "y must not be empty"),
    (fpt(sample_indices=np.arange(9)), E, "sample_indices length mismatch: got 9, expected 10"),
    (fpt(sample_indices=np.arange(1, N + 1)), E, "sample_indices out of range"),
    (fpt(y=YR[:9], x=X2[:9, 1:]), E, "len(y)=9 must equal n_samples=10 when sample_indices is not provided"),
    (fpt(u=UT[0]), E, "u must be 2D (n_samples, k)"),
    (fpt(u=UT[:9]), E, "u row count mismatch: got 9, expected 10"),
    (fpt(s=S[:9].astype(np.float32)), E, "s length mismatch: got 9, expected 10"),
    (fpt(u=UT[:, :9], s=S[:9].astype(np.float32)), E,
     "u must provide full-rank eigenvectors for packed fixed-lambda scan: got k=9, expected >= n=10"),
    (fpt(s=np.where(np.arange(N) == 2, NAN, S).astype(np.float32)), E, "invalid s/tau produced non-finite values"),
    (fpt(x=YR), E, "x must be 2D (n, p0)"),
    (fpt(x=X2[:9]), E, "x row count mismatch: got 9, expected 10"),
    (fpt(x=np.ones((N, 9))), E, "n must be > p for null model: n=10, p=10"),
    (fpt(x=np.ones((N, 8))), E, "n must be > p+1 for SNP tests: n=10, p=9"),
    (fpt(x=YR, u=UT[0]), E, "u must be 2D (n_samples, k)"),

    (lmp(n_samples=0), E, "n_samples must be > 0"),
    (lmp(chunk_size=0), E, "chunk_size must be > 0"),
    (lmp(chunk_size=0, n_samples=0), E, "n_samples must be > 0"),
    (lmp(packed=PACKED[0]), E, "packed must be 2D (m, bytes_per_snp)"),
    (lmp(packed=PACKED[:, :2]), E, DIM2),
    (lmp(packed=PACKED[:, :2], chunk_size=0), E, "chunk_size must be > 0"),
    (lmp(row_flip=FLIP[:5]), E, "row_flip length mismatch: got 5, expected 6"),
    (lmp(row_maf=MAF[:5]), E, "row_maf length mismatch: got 5, expected 6"),
    (lmp(row_flip=FLIP[:5], packed=PACKED[:, :2]), E, DIM2),
    (lmp(sample_indices=np.arange(9)), E, "sample_indices length mismatch: got 9, expected len(y)=10"),
    (lmp(y=YR[:9]), E, "sample_indices length mismatch: got 10, expected len(y)=9"),
    (lmp(x=X2[:9]), E, "X.n_rows must equal len(y)"),
    (lmp(ixx=np.eye(3)), E, "ixx must be (q0,q0)"),
    (lmp(x=X_WIDE, ixx=np.eye(9)), E, "n too small: require n > q0+1, got n=10, q0=9"),
    (lmp(x=X2[:9], row_maf=MAF[:5]), E, "row_maf length mismatch: got 5, expected 6"),
    (lmd(chunk_size=-1), E, "chunk_size must be > 0"),
    (lmd(x=X2[:9]), E, "X.n_rows must equal len(y)"),
    (lmd(ixx=np.eye(3)), E, "ixx must be (q0,q0)"),
    (lmd(g=G[:, :9]), E, "g must be shape (m, n)"),
    (lmd(g=G[0]), E, "g must be shape (m, n)"),
    (lmd(g=G[0], ixx=np.eye(3)), E, "ixx must be (q0,q0)"),
    (lmd(x=X_WIDE, ixx=np.eye(9)), E, "n too small: require n > q0+1, got n=10, q0=9"),
    (lmd(x=X_WIDE, ixx=np.eye(9), g=G[0]), E, "g must be shape (m, n)"),

    (lmt(n_samples=0), E, "n_samples must be > 0"),
    (lmt(chunk_size=0), E, "chunk_size must be > 0"),
    (lmt(maf_threshold=0.6), V, "maf_threshold must be within [0, 0.5]"),
    (lmt(maf_threshold=NAN), V, "maf_threshold must be within [0, 0.5]"),
    (lmt(max_missing_rate=1.5), V, "max_missing_rate must be within [0, 1.0]"),
    (lmt(het_threshold=-0.1), V, "het_threshold must be within [0, 1.0]"),
    (lmt(het_threshold=-0.1, maf_threshold=0.6), V, "maf_threshold must be within [0, 0.5]"),
    (lmt(maf_threshold=0.6, chunk_size=0), E, "chunk_size must be > 0"),
    (lmt(packed=PACKED[0]), E, "packed must be 2D (m, bytes_per_snp)"),
    (lmt(packed=PACKED[0], het_threshold=2.0), V, "het_threshold must be within [0, 1.0]"),
    (lmt(row_indices=np.array([0, 6])), E, "row_indices out of range"),
    (lmt(row_indices=np.array([-1])), E, "row_indices out of range"),
    (lmt(row_flip=FLIP[:5]), E, "row_flip length mismatch"),
    (lmt(row_maf=MAF[:5]), E, "row_maf length mismatch"),
    (lmt(row_missing=MISS[:5]), E, "row_missing length mismatch"),
    (lmt(row_indices=ROWS3), E, "row_flip length mismatch"),
    (lmt(row_flip=FLIP[:5], packed=PACKED[:, :2]), E, "row_flip length mismatch"),
    (lmt(**NO_META), E, "empty TSV metadata requires non-empty bed_prefix"),
    (lmt(**NO_META, bed_prefix="  "), E, "empty TSV metadata requires non-empty bed_prefix"),
    (lmt(**NO_META, packed=PACKED[:, :2]), E, "empty TSV metadata requires non-empty bed_prefix"),
    (lmt(chrom=["1"] * 5), E, "TSV metadata length mismatch: rows=6, chrom=5, pos=6, snp=6, allele0=6, allele1=6"),
    (lmt(allele1=[]), E, "TSV metadata length mismatch: rows=6, chrom=6, pos=6, snp=6, allele0=6, allele1=0"),
    (lmt(**NO_META, bed_prefix=PFX, packed=PACKED[:5], row_flip=FLIP[:5], row_maf=MAF[:5], row_missing=MISS[:5]), E,
     "BIM metadata length mismatch: expected=5, chrom=6, pos=6, snp=6, allele0=6, allele1=6"),
    (lmt(packed=PACKED[:, :2]), E, DIM2),
    (lmt(y=YR[:9]), E, "sample_indices length mismatch: got 10, expected len(y)=9"),
    (lmt(ixx=np.eye(3)), E, "ixx must be (q0,q0)"),

    (lms(chunk_size=0), V, "chunk_size must be > 0"),
    (lms(maf_threshold=-0.1), V, "maf_threshold must be within [0, 0.5]"),
    (lms(max_missing_rate=NAN), V, "max_missing_rate must be within [0, 1.0]"),
    (lms(het_threshold=1.1), V, "het_threshold must be within [0, 1.0]"),
    (lms(het_threshold=1.1, chunk_size=0), V, "chunk_size must be > 0"),
    (lms(genetic_model="mult"), V, "genetic_model must be one of: add, dom, rec, het"),
    (lms(genetic_model="mult", x=X2[:9]), V, "genetic_model must be one of: add, dom, rec, het"),
    (lms(genetic_model="mult", het_threshold=1.1), V, "het_threshold must be within [0, 1.0]"),
    (lms(genetic_model=" Dom "), E, "genetic_model 'dom' is outside this build's scope (additive model only)"),
    (lms(mmap_window_mb=0), V, "mmap_window_mb must be > 0"),
    (lms(x=X2[:9]), E, "X.n_rows must equal len(y)"),
    (lms(x=X_WIDE, ixx=None), E, "n too small: require n > q0+1, got n=10, q0=9"),
    (lms(ixx=np.eye(3)), E, "ixx must be (q0,q0)"),
    (lms(row_indices=ROWS3), E, ALL_OR_NONE),
    (lms(row_indices=ROWS3, ixx=np.eye(3)), E, "ixx must be (q0,q0)"),
    (lms(**dict(PREP3, row_maf=MAF[:2])), E,
     "prepared row metadata length mismatch: row_indices=3, row_flip=3, row_missing=3, row_maf=2"),
    (lms(**dict(PREP3, row_indices=np.array([2, 0, 3]))), E, "prepared row_indices must be sorted in ascending BED order"),
    (lms(sample_ids=IDS[:9] + ["nobody"]), E, "sample id not found in FAM: nobody"),
    (lms(sample_ids=IDS[:9] + ["nobody"], row_maf=MAF[:3]), E, ALL_OR_NONE),
    (lms(sample_ids=IDS[:9]), E, "sample_ids length mismatch: selected n=9 but len(y)=10"),
    (lms(packed=PACKED), E, "the staged payload needs both `packed` and `packed_n_samples` > 0"),
    (lms(packed_n_samples=N), E, "the staged payload needs both `packed` and `packed_n_samples` > 0"),
    (lms(packed=PACKED, packed_n_samples=9), E, "packed_n_samples 9 != 10 samples of <prefix>.fam"),
    (lms(packed=PACKED, sample_ids=IDS[:9]), E, "sample_ids length mismatch: selected n=9 but len(y)=10"),

    (lm2(chunk_size=0), V, "chunk_size must be > 0"),
    (lm2(max_missing_rate=2.0), V, "max_missing_rate must be within [0, 1.0]"),
    (lm2(genetic_model="rec"), E, "genetic_model 'rec' is outside this build's scope (additive model only)"),
    (lm2(x=X2[:9]), E, "X.n_rows must equal len(y)"),
    (lm2(cov_all=COV[:9]), E, "cov_all.n_rows must equal len(y)"),
    (lm2(cov_all=COV[:9], x=X2[:9]), E, "X.n_rows must equal len(y)"),
    (lm2(cov_all=COV[:, :0]), E, "LM2 requires cov_all with at least one column"),
    (lm2(cov_indices=[0, -1]), E, "cov_indices must be >= 0"),
    (lm2(cov_indices=[0, 3]), E, "cov_indices out of range: 3 >= 3"),
    (lm2(cov_indices=[]), E, "LM2 requires at least one explicitly selected covariate column."),
    (lm2(x=np.ones((N, 7))), E, "n too small: require n > q_base + 1 + n_interactions, got n=10, q_base=7, n_interactions=2"),
    (lm2(x=np.ones((N, 0)), cov_all=np.ones((N, 9)), cov_indices=list(range(9))), E,
     "n too small: require n > q_base + 1 + n_interactions, got n=10, q_base=0, n_interactions=9"),
    (lm2(row_flip=FLIP[:3]), E, ALL_OR_NONE),
    (lm2(row_flip=FLIP[:3], cov_indices=[]), E, "LM2 requires at least one explicitly selected covariate column."),
    (lm2(**dict(PREP3, row_missing=MISS[:2])), E,
     "prepared row metadata length mismatch: row_indices=3, row_flip=3, row_missing=2, row_maf=3"),
    (lm2(sample_ids=[7] + IDS[1:]), E, "sample id not found in FAM: 7"),
    (lm2(sample_ids=IDS + IDS[:1]), E, "sample_ids length mismatch: selected n=11 but len(y)=10"),
    (lm2(packed=PACKED, packed_n_samples=11), E, "packed_n_samples 11 != 10 samples of <prefix>.fam"),

    # rows added later stand at the end: a row's number is part of its test id
    (rot_xy(x=np.ones((N, 16))), E, "x must have between 0 and 15 columns"),
    (rot_xy(x=np.ones((N, 16)), u_t=UT9), E, UT_SHAPE_MSG),
]


def _row_id(row):
    (fn, kw), _exc, _msg = row
    changed = [k for k, v in kw.items() if k not in BASES[fn] or v is not BASES[fn][k]]
    return fn + ":" + ",".join(changed)


@pytest.mark.parametrize("row", TABLE, ids=[f"{i:03d}-{_row_id(r)}" for i, r in enumerate(TABLE)])
def test_refusal_type_message_and_order(row, prefix):
    (fn, kw), exc, msg = row
    kw = {k: (prefix if isinstance(v, str) and v == PFX else v) for k, v in kw.items()}
    with pytest.raises(exc) as info:
        getattr(jx, fn)(**kw)
    assert type(info.value) is exc and str(info.value) == msg.replace(PFX, prefix)


def test_an_empty_payload_returns_before_the_device():
    none = PACKED[:0]
    for nullml, cols in ((None, 3), (-3.0, 4)):
        out = jx.lmm_reml_assoc_packed_f32(none, N, FLIP[:0], MAF[:0], S, X2, YR, UT, nullml=nullml)
        assert out.shape == (0, cols) and out.dtype == np.float64
        out = jx.fvlmm_assoc_packed_f32(none, N, FLIP[:0], MAF[:0], S, X2, YR, UT, 0.0, nullml=nullml)
        assert out.shape == (0, cols) and out.dtype == np.float64
    out = jx.lm_block_assoc_packed(YR, X2, IXX, none, N, FLIP[:0], MAF[:0])
    assert out.shape == (0, 4) and out.dtype == np.float64
    for out, shape in ((jx.lmm_reml_chunk_f32(S, X2, YR, -5.0, 5.0, G[:0]), (0, 3)),
                       (jx.fvlmm_assoc_chunk_f32(S, X2, YR, 0.0, G[:0]), (0, 3)),
                       (jx.lm_block_assoc_f32(YR, X2, IXX, G[:0]), (0, 4))):
        assert out.shape == shape and out.dtype == np.float64
    assert jx.fvlmm_assoc_chunk_from_snp_to_tsv_f32(S, X2, YR, 0.0, G[:0], UT9, [], [], [], [], [], [], []) == ([], 0)


# ---- prepared values ---------------------------------------------------------------------------------------------------------

def test_clamped_start():
    """Brent's start of the exact scans: `init_log10_lbd` clamped to [low, high]; None (the interval midpoint, chosen by the
    kernel) without one or with a non-finite one."""
    low, high = -2.0, 3.0
    for init, want in ((-7.5, -2.0), (0.25, 0.25), (3.5, 3.0), (-2.0, -2.0), (3.0, 3.0), (NAN, None), (INF, None), (None, None)):
        got = jx._assoc_start(init, low, high)
        assert got == want and (want is None or type(got) is float)
    assert type(jx._assoc_start(np.float32(0.5), -1, 1)) is float and jx._assoc_start(7, -1, 1) == 1.0


def _restated_chain(m, block, every, pieces):
    """The chains of `lmm_reml_assoc_packed_f32`: segments of `every` rows (`block` when 0) cut into blocks of `block` rows, a
    block of two rows or more cut at half its length once per doubling of `pieces`."""
    seg = block if every == 0 else every
    bounds = [b for s0 in range(0, m, seg) for b in range(s0, min(s0 + seg, m), block)] + [m]
    cuts = list(zip(bounds[:-1], bounds[1:]))
    while pieces > 1:
        cuts = [c for b0, b1 in cuts for c in ([(b0, b1)] if b1 - b0 < 2 else [(b0, b0 + (b1 - b0) // 2), (b0 + (b1 - b0) // 2, b1)])]
        pieces //= 2
    return [b0 for b0, _b1 in cuts] + [m]


CHAINS_70_16 = {(0, 1): [0, 16, 32, 48, 64, 70], (40, 1): [0, 16, 32, 40, 56, 70],
                (0, 2): [0, 8, 16, 24, 32, 40, 48, 56, 64, 67, 70], (40, 2): [0, 8, 16, 24, 32, 36, 40, 48, 56, 63, 70]}


def test_chain_offsets_of_the_packed_scan(monkeypatch):
    seen = []
    monkeypatch.setattr(jx, "_assoc_packed", lambda *a, **kw: seen.append(kw["chain_off"]))
    monkeypatch.delenv("JX_LMM_UNIFIED_NO_WARM_START", raising=False)
    m = 70
    pk = np.zeros((m, 3), dtype=np.uint8)

    def offsets(**kw):
        jx.lmm_reml_assoc_packed_f32(pk, N, np.zeros(m, dtype=bool), np.full(m, 0.2, dtype=np.float32), S, X2, YR, UT,
                                     rotate_block_rows=16, **kw)
        return seen.pop()

    for (every, pieces), want in CHAINS_70_16.items():
        assert _restated_chain(m, 16, every, pieces) == want
        got = offsets(progress_every=every, warm_chain_pieces=pieces)
        assert got.dtype == np.int64 and got.tolist() == want
    for spelling in ("chain", "carry", "on", "true", "1", " Chain ", "TRUE", 1, True):
        assert offsets(warm_start=spelling).tolist() == CHAINS_70_16[(0, 1)]
    for spelling in ("none", "off", "false", "0", " None", "OFF", 0, False):
        assert offsets(warm_start=spelling) is None
    # the rows of a selection are the chained rows
    assert offsets(row_indices=np.arange(0, 70, 2), warm_chain_pieces=2).tolist() == _restated_chain(35, 16, 0, 2)
    for value in ("1", "true", " Yes ", "y", "ON"):
        monkeypatch.setenv("JX_LMM_UNIFIED_NO_WARM_START", value)
        assert offsets() is None
        assert offsets(warm_start="chain").tolist() == CHAINS_70_16[(0, 1)]
    for value in ("0", "", "no"):
        monkeypatch.setenv("JX_LMM_UNIFIED_NO_WARM_START", value)
        assert offsets().tolist() == CHAINS_70_16[(0, 1)]


def test_bim_selects_its_own_rows(prefix):
    bim = bed.read_bim(prefix)
    assert bim.columns(range(M)) == BIM_COLUMNS and all(type(p) is int for p in bim.pos)
    assert bim.columns([]) == ([], [], [], [], []) and bim.columns(np.zeros(0, dtype=np.int64)) == ([], [], [], [], [])
    for sel in ([4, 4, 1], np.array([5, 0, 3, 0]), (2,)):
        want = tuple([col[int(j)] for j in sel] for col in BIM_COLUMNS)
        assert bim.columns(sel) == want
        sub = bim.take(sel)
        assert isinstance(sub, bed.Bim) and (sub.chrom, sub.pos, sub.snp, sub.a0, sub.a1) == want
    empty = bim.take([])
    assert (empty.chrom, empty.snp, empty.pos, empty.a0, empty.a1) == ([], [], [], [], [])
    assert bim.columns(range(M)) == BIM_COLUMNS                     # a selection leaves the table as it was
    assert bed.snps_only_mask(bim.take([3, 4, 5])).tolist() == [True, False, False]


def test_load_bim_columns(prefix):
    assert jx.load_bim_columns(prefix) == BIM_COLUMNS
    assert jx.load_bim_columns(prefix + ".bed") == BIM_COLUMNS
    got = jx.load_bim_columns(prefix, np.array([5, 0, 0]))
    assert got == (["X", "1", "1"], [36, 11, 11], ["rs5", "rs0", "rs0"], ["A", "A", "A"], ["N", "C", "C"])
    assert isinstance(got, tuple) and all(type(c) is list for c in got) and all(type(p) is int for p in got[1])
    assert jx.load_bim_columns(prefix, []) == ([], [], [], [], [])
    for bad, exc, msg in (("", ValueError, "path_or_prefix must not be empty"),
                          (prefix + ".none", ValueError,
                           "load_bim_columns requires a PLINK BED/BIM/FAM prefix or explicit PLINK file path")):
        with pytest.raises(exc) as info:
            jx.load_bim_columns(bad)
        assert type(info.value) is exc and str(info.value) == msg
    with pytest.raises(ValueError) as info:
        jx.load_bim_columns(prefix, [0, -2])
    assert str(info.value) == "row_indices must be non-negative, got -2"
    with pytest.raises(RuntimeError) as info:
        jx.load_bim_columns(prefix, [0, 6])
    assert type(info.value) is RuntimeError and str(info.value) == "BIM row index out of range: 6 >= 6"


# ---- what the packed scans hand on -------------------------------------------------------------------------------------------

def test_arguments_handed_to_the_scan(monkeypatch):
    """`pipeline.scan_rows`, `pipeline.SpectralModel.rotated` and `_panel` replaced by recorders: the keyword values below are
    those of the commit before the shared front end, the fixed-lambda scan's interval, iteration count and tolerance included."""
    import torch
    from janusx_amd import pipeline as pl
    m = 5
    pk, flip, maf = PACKED[:m], FLIP[:m], MAF[:m]
    calls = []

    class FakePanel:
        device = "cpu"

        def counts(self):
            return np.zeros((m, 3), dtype=np.int32)

    def panel(packed, n_samples, idx=None):
        calls.append(("panel", packed, n_samples, idx))
        return FakePanel()

    def rotated(s, u_t, xcov, y, device):
        calls.append(("rotated", s, u_t, xcov, y, device))
        return "model"

    def scan_rows(panel, model, rows, lut, mode, **kw):
        calls.append(("scan", panel, model, rows, lut, mode, kw))
        return torch.zeros((len(rows), 3), dtype=torch.float64)

    monkeypatch.setattr(jx, "_panel", panel)
    monkeypatch.setattr(pl.SpectralModel, "rotated", staticmethod(rotated))
    monkeypatch.setattr(pl, "scan_rows", scan_rows)
    monkeypatch.delenv("JX_LMM_UNIFIED_NO_WARM_START", raising=False)

    def handed(fn, *a, **kw):
        del calls[:]
        out = fn(*a, **kw)
        assert out.shape == (m, 3) and [c[0] for c in calls] == ["panel", "rotated", "scan"]
        (_p, packed, n_samples, idx), (_r, s, u_t, xcov, y, device), (_s, panel_, model, rows, lut, mode, opts) = calls
        assert np.array_equal(packed, pk) and n_samples == N and idx is None
        assert np.array_equal(s, S) and u_t.dtype == np.float32 and np.array_equal(u_t, UT) and np.array_equal(xcov, X2)
        assert np.array_equal(y, YR) and device == "cpu" and isinstance(panel_, FakePanel) and model == "model"
        assert rows.tolist() == list(range(m)) and lut.shape == (m, 4) and lut.dtype == np.float32
        assert sorted(opts) == ["block_rows", "chain_off", "high", "init_log10_lbd", "low", "max_iter", "nullml", "progress",
                                "progress_every", "tol"]
        assert opts["block_rows"] == 8192 and opts["progress"] is None
        for k in ("low", "high", "tol"):
            assert type(opts[k]) is float
        assert type(opts["max_iter"]) is int
        chain = opts.pop("chain_off")
        return mode, {k: opts[k] for k in ("low", "high", "max_iter", "tol", "init_log10_lbd", "nullml", "progress_every")}, chain

    args = (pk, N, flip, maf, S, X2, YR, UT)
    mode, opts, chain = handed(jx.lmm_reml_assoc_packed_f32, *args, low=-4, high=3, max_iter=40, tol=1e-3, init_log10_lbd=9.0,
                               rotate_block_rows=2, warm_chain_pieces=2, progress_every=3)
    assert mode == "lmm" and opts == dict(low=-4.0, high=3.0, max_iter=40, tol=1e-3, init_log10_lbd=3.0, nullml=None,
                                          progress_every=3)
    assert chain.dtype == np.int64 and chain.tolist() == [0, 1, 2, 3, 4, 5] and type(opts["init_log10_lbd"]) is float
    mode, opts, chain = handed(jx.lmm_reml_assoc_packed_f32, *args, warm_start="none", nullml=-12)
    assert mode == "lmm" and chain is None
    assert opts == dict(low=-5.0, high=5.0, max_iter=50, tol=1e-2, init_log10_lbd=None, nullml=-12.0, progress_every=0)
    assert type(opts["nullml"]) is float
    mode, opts, chain = handed(jx.lmm_reml_assoc_packed_f32, *args)
    assert mode == "lmm" and chain.tolist() == [0, 5] and opts["init_log10_lbd"] is None
    mode, opts, chain = handed(jx.fvlmm_assoc_packed_f32, *args, 0.75)
    assert mode == "fvlmm" and chain is None
    assert opts == dict(low=0.75, high=1.75, max_iter=0, tol=1e-2, init_log10_lbd=0.75, nullml=None, progress_every=0)
    assert type(opts["init_log10_lbd"]) is float
    mode, opts, chain = handed(jx._assoc_packed, *args, None, None, mode="lmm2", low=-3.0, high=2.0, max_iter=30, tol=1e-2,
                               init_log10_lbd=-8.0, nullml=-20.5, chain_off=np.array([0, 5]))
    assert mode == "lmm2" and chain is None
    assert opts == dict(low=-3.0, high=2.0, max_iter=30, tol=1e-2, init_log10_lbd=-3.0, nullml=-20.5, progress_every=0)
