// Multi-trait linear-model scan (`jx gwas -lm -trait-level`): the shared-projection route of the reference
// (`lm_trait_assoc_bed_to_tsv_shared_fast`, src/stats/lm_trait.rs:481-686: one QR of X, G Q and G Y as GEMMs, a per-(SNP, trait)
// epilogue `lm_assoc_from_shared_projection`, :303-335) with the tall-skinny product  G (m x n, 2 bit) [Q | R] (n x C)  on the int8
// matrix pipes.  R = Y - Q Q'Y is formed in f64 by the caller, so that the product's R columns are the residualised sums g'r
// directly (the reference's gy_raw - sum qg qty is the same algebra with worse conditioning).
//
// Operand: every column b of [Q | R] is split into FOUR signed radix-128 digit planes against a power-of-two scale S >= max |b|,
//     b / S = q1 / 2^6 + q2 / 2^13 + q3 / 2^20 + q4 / 2^27 + e,   |q| <= 64,   |e| <= 2^-28,
// q1 = rint(64 b / S), q2 = rint(128 (64 b / S - q1)), ...: every remainder is exact in f64, only the last rint rounds, and a column
// whose entries are multiples of S 2^-27 splits exactly.  Three planes (the rotation's count) leave 2^-21: 1e-5 on beta at
// n = 300 .. 20 000, over the bar; four leave 1e-7 (DESIGN 3.16 derives the bound).
//
// Product: the called genotypes are the exact int8 operand c in {0, 1, 2} (`counts16` of i8_tile.h), the missing calls a
// second exact operand e in {0, 1} (`missing16`); both meet the same four planes in v_mfma_i32_32x32x32_i8 products whose
// i32 sums are exact (|c q| <= 128 per sample: n < 2^31 / 254 is required).  Per (row, column) the epilogue combines the planes as
// 64-bit INTEGERS,  N_c = ((a1 128 + a2) 128 + a3) 128 + a4  and N_e likewise, takes a flipped row as 2 (colsum - N_e) - N_c
// (colsum = the integer column sum of the planes over the samples) and writes
//     sums = double(N_called) s + double(mean_r) (double(N_e) s),      s = S 2^-27  (a power of two: both products by s are exact)
// The form of a row is the same for every row and column (both operands, always): a (row, column) sum has the same bits in any
// row blocking, any column batching and at any column position, and on dyadic columns it is the exact value rounded once.
//
// Shape: 256 threads = 4 waves on 128 rows x 32 columns, one 32 x 32 tile and 2 operands x 4 planes = 8 accumulators (128
// registers) per wave.  A lane reads its 16 payload bytes of a 128-sample record straight from the P32 image (lane (row, h) takes
// the dwords 4 h .. 4 h + 3: the k slot (ks, h) of the MFMA is the 16-sample group 4 h + ks, as in rotate_i8_dma_kernel) and
// decodes them in registers; the four waves share the column tile's planes (4 x 32 x 128 B = 16 KB per 128-sample step) through
// LDS, double buffered from registers that were loaded two and three steps ahead, one barrier per step; rows are
// [column][128 B] with the 16-byte chunk index XOR (column >> 1) & 7.  No atomics: one workgroup owns a (row tile, column tile).
#include <cmath>

#include "i8_tile.h"
#include "jx_common.h"
#include "lm_pvalue.h"

namespace jx {

constexpr int LT_PLANES = 4;
constexpr int LT_TM = 128;                       // rows per workgroup (32 per wave)
constexpr int LT_TN = 32;                        // columns per workgroup
constexpr int LT_PLANE_LDS = LT_TN * 128;        // one plane of a 128-sample step
constexpr int LT_STAGE = LT_PLANES * LT_PLANE_LDS;

// ---- operand preparation ----------------------------------------------------------------------------------------------------
// b: column c at b + c ldb (n contiguous f64).  sexp[c] = e with S = 2^e the smallest power of two >= max |b_c| (0 for a zero or
// a pad column); scale[c] = 2^(e - 27).
__global__ __launch_bounds__(256) void lt_colmax_kernel(const double *__restrict__ b, int64_t ldb, int n, int ncols,
                                                        int32_t *__restrict__ sexp, double *__restrict__ scale) {
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0;
    if (c < ncols)
        for (int i = tid; i < n; i += 256) a = fmax(a, fabs(b[(int64_t)c * ldb + i]));
    red[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) {
        int e = 0;
        const double mx = red[0];
        if (mx > 0.0 && mx < INFINITY) {
            const double f = frexp(mx, &e);           // mx = f 2^e, f in [0.5, 1)
            if (f == 0.5) e -= 1;                     // mx is a power of two itself
        }
        sexp[c] = e;
        scale[c] = ldexp(1.0, e - 27);
    }
}

// thread = (column, 16-sample group): the group's 16 bytes of every plane, in the decode's byte order.  planes: (4, cpad, npad).
// rem (optional, laid out as b): what the four digits leave of every entry, b - S (q1 / 2^6 + ... + q4 / 2^27), exact in f64.
__global__ __launch_bounds__(256) void lt_quant_kernel(const double *__restrict__ b, int64_t ldb, int n, int ncols, int cpad,
                                                       int64_t npad, const int32_t *__restrict__ sexp,
                                                       int8_t *__restrict__ planes, double *__restrict__ rem) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t groups = npad / 16;
    if (idx >= (int64_t)cpad * groups) return;
    const int64_t c = idx / groups, gq = idx - c * groups;
    int8_t o[LT_PLANES][16];
    const int e = c < ncols ? sexp[c] : 0;
#pragma unroll
    for (int pos = 0; pos < 16; ++pos) {
        const int smp = ((pos & 3) << 2) | (pos >> 2);           // byte 4 q + b holds sample 4 b + q
        const int64_t i = gq * 16 + smp;
        double a = 0.0;
        if (c < ncols && i < n) a = ldexp(b[c * ldb + i], 6 - e);   // 64 b / S, |a| <= 64
#pragma unroll
        for (int pl = 0; pl < LT_PLANES; ++pl) {
            const double q = rint(a);
            o[pl][pos] = (int8_t)q;
            a = (a - q) * 128.0;
        }
        if (rem && c < ncols && i < n) rem[c * ldb + i] = ldexp(a, e - 34);     // a = what is left, in units of S 2^-34
    }
#pragma unroll
    for (int pl = 0; pl < LT_PLANES; ++pl)
        *reinterpret_cast<uint4 *>(planes + ((int64_t)pl * cpad + c) * npad + gq * 16) = *reinterpret_cast<const uint4 *>(o[pl]);
}

// colsum[c] = sum over the samples of the column's integer  ((q1 128 + q2) 128 + q3) 128 + q4  (the pad bytes are zero)
__global__ __launch_bounds__(256) void lt_colsum_kernel(const int8_t *__restrict__ planes, int cpad, int64_t npad,
                                                        long long *__restrict__ colsum) {
    __shared__ long long red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    long long a = 0;
    for (int64_t i = tid; i < npad; i += 256) {
        long long v = 0;
#pragma unroll
        for (int pl = 0; pl < LT_PLANES; ++pl) v = v * 128 + (long long)planes[((int64_t)pl * cpad + c) * npad + i];
        a += v;
    }
    red[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) colsum[c] = red[0];
}

// ---- product ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void lt_sums_kernel(const uint8_t *__restrict__ p32, int64_t m_total, int ntiles,
                                                      const int32_t *__restrict__ rows, int nrows,
                                                      const float *__restrict__ mean, const uint8_t *__restrict__ flip,
                                                      const int8_t *__restrict__ planes, int cpad, int64_t npad,
                                                      const double *__restrict__ scale, const long long *__restrict__ colsum,
                                                      int ncols, double *__restrict__ sums, int64_t lds) {
    __shared__ __attribute__((aligned(16))) uint8_t sm[2 * LT_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, frow = lane & 31;
    const int j0 = blockIdx.x * LT_TN;
    const int r0 = blockIdx.y * LT_TM + wave * 32;

    // payload: lane (row frow, half h) reads the 16 bytes 16 h .. 16 h + 15 of its row's record of every tile; a row beyond the
    // list reads record 0 (its sums are not written)
    const int myrow = r0 + frow;
    const int64_t rec = myrow < nrows ? (rows ? (int64_t)rows[myrow] : (int64_t)myrow) : 0;
    const uint8_t *asrc = p32 + rec * 32 + 16 * h;
    const int64_t atile = m_total * 32;

    // planes: thread = (column tid >> 3, 16-byte chunk tid & 7) of each plane; cpad is a multiple of LT_TN, so every column exists
    const int bcol = tid >> 3, bchunk = tid & 7;
    const int8_t *bsrc = planes + (int64_t)(j0 + bcol) * npad + bchunk * 16;
    const int64_t bplane = (int64_t)cpad * npad;
    const int bdst = bcol * 128 + ((bchunk ^ ((bcol >> 1) & 7)) << 4);

    i32x16 accc[LT_PLANES], acce[LT_PLANES];
#pragma unroll
    for (int pl = 0; pl < LT_PLANES; ++pl)
#pragma unroll
        for (int r = 0; r < 16; ++r) accc[pl][r] = 0, acce[pl][r] = 0;

    // Loads run ahead of their use: the payload dwords of the steps t + 1 .. t + 4 and the planes of the steps t + 2 and t + 3 are
    // in flight while step t is multiplied (a step is ~0.4 us of products, a load from HBM under traffic several times that).
    // Past the end the last step is loaded again and nothing reads it.
    const int last = ntiles - 1;
#define LT_LOAD_A(t) (*reinterpret_cast<const uint4 *>(asrc + (int64_t)((t) < last ? (t) : last) * atile))
#define LT_LOAD_B(pl, t) (*reinterpret_cast<const uint4 *>(bsrc + (pl) * bplane + (int64_t)((t) < last ? (t) : last) * 128))
    uint4 aq0 = LT_LOAD_A(0), aq1 = LT_LOAD_A(1), aq2 = LT_LOAD_A(2), aq3 = LT_LOAD_A(3);
    uint4 bn0 = LT_LOAD_B(0, 0), bn1 = LT_LOAD_B(1, 0), bn2 = LT_LOAD_B(2, 0), bn3 = LT_LOAD_B(3, 0);
    *reinterpret_cast<uint4 *>(sm + 0 * LT_PLANE_LDS + bdst) = bn0;
    *reinterpret_cast<uint4 *>(sm + 1 * LT_PLANE_LDS + bdst) = bn1;
    *reinterpret_cast<uint4 *>(sm + 2 * LT_PLANE_LDS + bdst) = bn2;
    *reinterpret_cast<uint4 *>(sm + 3 * LT_PLANE_LDS + bdst) = bn3;
    bn0 = LT_LOAD_B(0, 1), bn1 = LT_LOAD_B(1, 1), bn2 = LT_LOAD_B(2, 1), bn3 = LT_LOAD_B(3, 1);
    uint4 bf0 = LT_LOAD_B(0, 2), bf1 = LT_LOAD_B(1, 2), bf2 = LT_LOAD_B(2, 2), bf3 = LT_LOAD_B(3, 2);
    __syncthreads();

    const int fx = (frow >> 1) & 7;
    for (int t = 0; t < ntiles; ++t) {
        const uint8_t *st = sm + (t & 1) * LT_STAGE;
        const uint4 acur = aq0;
        aq0 = aq1, aq1 = aq2, aq2 = aq3;
        aq3 = LT_LOAD_A(t + 4);
        const uint4 bs0 = bn0, bs1 = bn1, bs2 = bn2, bs3 = bn3;      // the planes of step t + 1
        bn0 = bf0, bn1 = bf1, bn2 = bf2, bn3 = bf3;
        bf0 = LT_LOAD_B(0, t + 3), bf1 = LT_LOAD_B(1, t + 3), bf2 = LT_LOAD_B(2, t + 3), bf3 = LT_LOAD_B(3, t + 3);
        const bool more = t + 1 < ntiles;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const uint32_t w = ks == 0 ? acur.x : ks == 1 ? acur.y : ks == 2 ? acur.z : acur.w;
            const i32x4 ac = (i32x4)counts16(w), ae = (i32x4)missing16(w);
            const int boff = frow * 128 + (((4 * h + ks) ^ fx) << 4);
#pragma unroll
            for (int pl = 0; pl < LT_PLANES; ++pl) {
                const i32x4 b = *reinterpret_cast<const i32x4 *>(st + pl * LT_PLANE_LDS + boff);
                accc[pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac, b, accc[pl], 0, 0, 0);
                acce[pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ae, b, acce[pl], 0, 0, 0);
            }
        }
        if (more) {
            uint8_t *wr = sm + ((t + 1) & 1) * LT_STAGE;       // last read in step t - 1, behind that step's barrier
            *reinterpret_cast<uint4 *>(wr + 0 * LT_PLANE_LDS + bdst) = bs0;
            *reinterpret_cast<uint4 *>(wr + 1 * LT_PLANE_LDS + bdst) = bs1;
            *reinterpret_cast<uint4 *>(wr + 2 * LT_PLANE_LDS + bdst) = bs2;
            *reinterpret_cast<uint4 *>(wr + 3 * LT_PLANE_LDS + bdst) = bs3;
        }
        __syncthreads();
    }
#undef LT_LOAD_A
#undef LT_LOAD_B
    static_assert(LT_PLANES == 4, "the plane registers of the product kernel are written out for four planes");

    // the accumulators hold (cd_row, cd_col) of the 32 x 32 shapes
    const int gj = j0 + frow;
    if (gj >= ncols) return;
    const double s = scale[gj];
    const long long cs = colsum[gj];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gr = cd_row(r, h, r0);
        if (gr >= nrows) continue;
        long long nc = 0, ne = 0;
#pragma unroll
        for (int pl = 0; pl < LT_PLANES; ++pl) {
            nc = nc * 128 + (long long)accc[pl][r];
            ne = ne * 128 + (long long)acce[pl][r];
        }
        const long long called = flip[gr] ? 2 * (cs - ne) - nc : nc;
        const double miss = (double)mean[gr] * ((double)ne * s);
        sums[(int64_t)gr * lds + gj] = (double)called * s + miss;
    }
}

// ---- statistics (`lm_assoc_from_shared_projection`, lm_trait.rs:303-335; `sanitize_assoc_pvalue`, src/math/linalg.rs:99-108) ----
// thread = (row, trait), traits fastest.  qg (nrows, ldq): the Q columns' sums; gy (nrows, ldg): the residualised sums g'r_t.
// qg_lo (optional, as qg): the sums of what the digits of Q left over (`rem` of lt_quant_kernel), added to qg.  gg = d - sum qg^2
// is compared with an ABSOLUTE 1e-8: a row inside the span of the design (an all-heterozygous row against the intercept) is void
// only when qg carries f64 accuracy, and four digits leave n S 2^-28 on it (2e-6 on qg^2 at n = 300); eight leave 2^-56.
__global__ __launch_bounds__(256) void lt_stats_kernel(const double *__restrict__ qg, const double *__restrict__ qg_lo,
                                                       int64_t ldq, int rank,
                                                       const double *__restrict__ gy, int64_t ldg, int ntraits,
                                                       const double *__restrict__ dsum, int nrows,
                                                       const double *__restrict__ rss0, int n, int df, double ln_beta,
                                                       double *__restrict__ out, int64_t out_trait_stride, double pmax,
                                                       unsigned long long cap, int trait0, int row0,
                                                       int32_t *__restrict__ hit_trait, int32_t *__restrict__ hit_row,
                                                       double *__restrict__ hit_vals, unsigned long long *__restrict__ counter) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < (int64_t)nrows * ntraits;
    const int r = live ? (int)(idx / ntraits) : 0;
    const int t = live ? (int)(idx - (int64_t)r * ntraits) : 0;
    double beta = NAN, se = NAN, chisq = NAN, p = 1.0;
    if (live) {
        double gg = dsum[r];
        for (int k = 0; k < rank; ++k) {
            const double v = qg[(int64_t)r * ldq + k] + (qg_lo ? qg_lo[(int64_t)r * ldq + k] : 0.0);
            gg -= v * v;
        }
        if (isfinite(gg) && gg > 1e-8 && df > 0) {
            const double g = gy[(int64_t)r * ldg + t];
            const double b = g / gg;
            const double rss1 = fmax(rss0[t] - g * b, 0.0);
            const double ve = rss1 / (double)df;
            if (isfinite(b) && isfinite(ve) && ve > 0.0) {
                const double s = sqrt(ve / gg);
                if (isfinite(s) && s > 0.0) {
                    const double tt = b / s;
                    beta = b, se = s;
                    chisq = (double)n * log(1.0 + (tt * tt) / (double)df);
                    const double pw = lm_student_t_two_sided(tt, df, ln_beta);
                    p = isfinite(pw) ? fmin(fmax(pw, LM_MIN_POS), 1.0) : 1.0;
                }
            }
        }
    }
    if (out && live) {
        double *o = out + (int64_t)t * out_trait_stride + (int64_t)r * 4;
        o[0] = beta, o[1] = se, o[2] = chisq, o[3] = p;
    }
    if (counter) {
        const bool hit = live && p <= pmax;
        wave_append(hit, counter, cap, [=](unsigned long long slot) {
            hit_trait[slot] = trait0 + t;
            hit_row[slot] = row0 + r;
            double *o = hit_vals + slot * 4;
            o[0] = beta, o[1] = se, o[2] = chisq, o[3] = p;
        });
    }
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_lmt_cpad(int ncols) { return ncols <= 0 ? 0 : ((ncols + LT_TN - 1) / LT_TN) * LT_TN; }

extern "C" int jxg_lmt_prepare(const double *d_b, int64_t ldb, int n, int ncols, int8_t *d_planes, double *d_scale,
                               int64_t *d_colsum, int32_t *d_sexp, double *d_rem, void *stream) {
    if (n <= 0 || ncols <= 0) return fail("jxg_lmt_prepare: empty operand");
    if (ldb < n) return fail("jxg_lmt_prepare: ldb must be >= n");
    hipStream_t st = (hipStream_t)stream;
    const int cpad = jxg_lmt_cpad(ncols);
    const int64_t npad = (int64_t)num_tiles(n) * JXG_TILE;
    hipLaunchKernelGGL(lt_colmax_kernel, dim3(cpad), dim3(256), 0, st, d_b, ldb, n, ncols, d_sexp, d_scale);
    JX_LAUNCH_CHECK();
    const int64_t items = (int64_t)cpad * (npad / 16);
    if ((items + 255) / 256 > 0x7fffffffLL) return fail("jxg_lmt_prepare: grid too large");
    hipLaunchKernelGGL(lt_quant_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_b, ldb, n, ncols, cpad, npad,
                       d_sexp, d_planes, d_rem);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(lt_colsum_kernel, dim3(cpad), dim3(256), 0, st, d_planes, cpad, npad,
                       reinterpret_cast<long long *>(d_colsum));
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_lmt_sums_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                const float *d_mean, const uint8_t *d_flip, const int8_t *d_planes, const double *d_scale,
                                const int64_t *d_colsum, int ncols, double *d_sums, int64_t ld_sums, void *stream) {
    if (nrows <= 0 || ncols <= 0) return 0;
    if (n <= 0 || (int64_t)n * 254 > 0x7fffffffLL)
        return fail("jxg_lmt_sums_p32: n = " + std::to_string(n) + " leaves the exact i32 range (2 * 127 * n < 2^31)");
    if (ld_sums < ncols) return fail("jxg_lmt_sums_p32: ld_sums must be >= ncols");
    if (!d_mean || !d_flip || !d_planes || !d_scale || !d_colsum) return fail("jxg_lmt_sums_p32: operand missing");
    const int cpad = jxg_lmt_cpad(ncols);
    const int nrt = (nrows + LT_TM - 1) / LT_TM;
    if (nrt > 65535) return fail("jxg_lmt_sums_p32: at most 8 388 480 rows per call");
    const int ntiles = num_tiles(n);
    hipLaunchKernelGGL(lt_sums_kernel, dim3(cpad / LT_TN, nrt), dim3(256), 0, (hipStream_t)stream, d_p32, m_total, ntiles, d_rows,
                       nrows, d_mean, d_flip, d_planes, cpad, (int64_t)ntiles * JXG_TILE, d_scale,
                       reinterpret_cast<const long long *>(d_colsum), ncols, d_sums, ld_sums);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_lmt_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy, int64_t ldg,
                             int ntraits, const double *d_dsum, int nrows, const double *d_rss0, int n, double *d_out,
                             int64_t out_trait_stride, double pmax, int64_t capacity, int trait0, int row0, int32_t *d_hit_trait,
                             int32_t *d_hit_row, double *d_hit_vals, uint64_t *d_count, void *stream) {
    if (nrows <= 0 || ntraits <= 0) return 0;
    if (rank < 0 || ldq < rank || ldg < ntraits) return fail("jxg_lmt_stats: leading dimensions too small");
    if (!d_out && !d_count) return fail("jxg_lmt_stats: neither the dense output nor the hit counter is given");
    if (d_count && (capacity < 0 || !d_hit_trait || !d_hit_row || !d_hit_vals)) return fail("jxg_lmt_stats: hit buffers missing");
    if (d_count && !(pmax == pmax)) return fail("jxg_lmt_stats: pmax is NaN");
    const int64_t items = (int64_t)nrows * ntraits;
    if ((items + 255) / 256 > 0x7fffffffLL) return fail("jxg_lmt_stats: grid too large");
    const int df = n - rank - 1;
    const double ln_beta = df > 0 ? lgamma(0.5 * df) + lgamma(0.5) - lgamma(0.5 * df + 0.5) : 0.0;
    hipLaunchKernelGGL(lt_stats_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_qg, d_qg_lo, ldq,
                       rank, d_gy, ldg, ntraits, d_dsum, nrows, d_rss0, n, df, ln_beta, d_out, out_trait_stride, pmax,
                       (unsigned long long)capacity, trait0, row0, d_hit_trait, d_hit_row, d_hit_vals,
                       reinterpret_cast<unsigned long long *>(d_count));
    JX_LAUNCH_CHECK();
    return 0;
}
