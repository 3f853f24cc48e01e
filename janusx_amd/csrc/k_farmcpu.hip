// FarmCPU raw route (`jx gwas -farmcpu`): the per-marker statistics of the fixed-effect scan (`scan_packed_full_matrix_reduced`,
// src/stats/farmcpu.rs:2629-2941) and of the final scan (`write_farmcpu_packed_main_scan`, :3310-3760) over the sums of the
// tall-skinny product  G [Q | r_y]  of k_lm_traits.hip (`jxg_lmt_prepare`, `jxg_lmt_sums_p32`, unchanged).
//
// The reference works in the raw design X (n x q0, [1 | covariates | pseudo-QTN columns]) with ixx = pinv(X'X): per marker
// xs = X'g, b21 = xs ixx, b22 = g'g - b21 xs, sy_adj = g'y - xs bg_beta.  With Q the orthonormal basis of the columns of X and
// P = X pinv(X'X) X' = Q Q' (true of a rank-deficient X too) the same quantities are
//     b22 = g'g - |Q'g|^2,     sy_adj = g'(y - P y) = g'r_y,     b21[q_base + j] = W[j] . (Q'g),   W = (ixx X'Q)[q_base:, :],
// the conditioning argument of k_lm_traits.hip's header: nothing of size |y|^2 or |X|^2 is ever subtracted on the device.  The
// host (farmcpu.py) forms Q, r_y, bg_rss = |r_y|^2, W, bg_beta and diag(ixx) of the QTN slots in f64 from the reference's pinv.
//
// Statistics of a row (FEM form): void (p = 1) when df <= 0, b22 <= 1e-8 or not finite, or ve < 0 / not finite; otherwise
//     beta = sy_adj / b22,  ve = (bg_rss - sy_adj beta) / df,  se = sqrt(ve / b22),  p = two-sided Student t (lm_pvalue.h),
// then `sanitize_assoc_pvalue`.  Per QTN slot j of a non-void row:  beta_j = bg_beta[j] - b21_j beta,
// se_j^2 = (ixx_jj + b21_j^2 / b22) ve,  t_j^2 = beta_j^2 / se_j^2, and the MAXIMUM of t_j^2 over the rows is kept: Student t is
// monotone in t^2 at fixed df, so the reference's minimum of p_j over the markers is p at that maximum, evaluated once per slot
// by the caller.  The maximum of non-negative doubles is the maximum of their bit patterns: fmax across the wave, then one
// 64-bit integer atomicMax per (wave, slot) -- no floating-point atomics, the same bits in any row blocking.
// Final form: rss = max(bg_rss - sy_adj^2 / b22, 0), ve = rss / df, a row without a finite beta and a positive finite se is three
// NaN.
//
// Mapping: 256 threads = 4 waves on a tile of 64 rows.  lane = row; wave w owns the slots j = w (mod 4), 32 accumulators per
// thread: 128 slots per workgroup, and blockIdx.y counts batches of 128 slots (every batch recomputes the row's b22, beta and ve,
// batch 0 writes the row), up to FC_MAX_QTN = 512.  The tile's Q'g (digits plus what the digits left, added once) and W pass through LDS in chunks
// of 32 basis columns: Q'g transposed to [k][row] (65-double rows: the lanes of a wave read 64 consecutive doubles), W as
// [slot][k], read at a wave-uniform address.  16.6 KB + 32 KB of LDS.  Every wave sums |Q'g|^2 in the same ascending k order, so
// b22 has the same bits in all four, in every slot batch and in any blocking; wave 0 of batch 0 evaluates p and writes the row.
#include <cmath>

#include "jx_common.h"
#include "lm_pvalue.h"

namespace jx {

constexpr int FC_ROWS = 64;
constexpr int FC_KC = 32;
constexpr int FC_SLOTS_PER_WAVE = 32;
constexpr int FC_SLOT_BATCH = 4 * FC_SLOTS_PER_WAVE;
constexpr int FC_MAX_QTN = 512;
constexpr int FC_MAX_RANK = 512;

__global__ __launch_bounds__(256) void fc_stats_kernel(const double *__restrict__ qg, const double *__restrict__ qg_lo,
                                                       int64_t ldq, int rank, const double *__restrict__ gy, int64_t ldg,
                                                       const double *__restrict__ ss, int nrows, double bg_rss, int df,
                                                       double ln_beta, const double *__restrict__ w, int64_t ldw, int kq_all,
                                                       const double *__restrict__ bgb, const double *__restrict__ dixx,
                                                       int final_form, double *__restrict__ out,
                                                       unsigned long long *__restrict__ maxbits) {
    __shared__ double sq[FC_KC][FC_ROWS + 1];
    __shared__ double sw[FC_SLOT_BATCH][FC_KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this workgroup's batch of slots (blockIdx.y = 0 alone when there are none)
    const int s0 = blockIdx.y * FC_SLOT_BATCH;
    const int kq = kq_all - s0 < FC_SLOT_BATCH ? (kq_all - s0 > 0 ? kq_all - s0 : 0) : FC_SLOT_BATCH;
    if (kq > 0) w += (int64_t)s0 * ldw, bgb += s0, dixx += s0, maxbits += s0;
    const bool writer = blockIdx.y == 0 && wave == 0;
    const int r0 = blockIdx.x * FC_ROWS;
    const int row = r0 + lane;
    const bool live = row < nrows;

    double acc[FC_SLOTS_PER_WAVE];
#pragma unroll
    for (int s = 0; s < FC_SLOTS_PER_WAVE; ++s) acc[s] = 0.0;
    double b22 = live ? ss[row] : 0.0;

    for (int k0 = 0; k0 < rank; k0 += FC_KC) {
        __syncthreads();                                        // the previous chunk has been read
        for (int idx = tid; idx < FC_ROWS * FC_KC; idx += 256) {
            const int rr = idx / FC_KC, kk = idx - rr * FC_KC;
            double v = 0.0;
            if (r0 + rr < nrows && k0 + kk < rank) {
                const int64_t at = (int64_t)(r0 + rr) * ldq + k0 + kk;
                v = qg[at] + (qg_lo ? qg_lo[at] : 0.0);
            }
            sq[kk][rr] = v;
        }
        for (int idx = tid; idx < kq * FC_KC; idx += 256) {
            const int sl = idx / FC_KC, kk = idx - sl * FC_KC;
            sw[sl][kk] = k0 + kk < rank ? w[(int64_t)sl * ldw + k0 + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < FC_KC; ++kk) {
            const double v = sq[kk][lane];
            b22 -= v * v;
#pragma unroll
            for (int s = 0; s < FC_SLOTS_PER_WAVE; ++s) {
                const int sl = 4 * s + wave;                    // wave-uniform
                if (sl < kq) acc[s] += v * sw[sl][kk];
            }
        }
    }

    double beta = NAN, se = NAN, ve = NAN, p = final_form ? NAN : 1.0;
    bool ok = false;                                            // the row takes part in the slot maxima
    if (live && df > 0 && isfinite(b22) && b22 > 1e-8) {
        const double g = gy[(int64_t)row * ldg];
        const double b = g / b22;
        if (final_form) {
            const double rss = fmax(bg_rss - g * g / b22, 0.0);
            const double s = sqrt((rss / (double)df) / b22);
            if (isfinite(b) && isfinite(s) && s > 0.0) {
                beta = b, se = s;
                p = writer ? lm_student_t_two_sided(b / s, df, ln_beta) : 1.0;
            }
        } else {
            const double v = (bg_rss - g * b) / (double)df;
            if (isfinite(b) && isfinite(v) && v >= 0.0) {
                ok = true;
                beta = b, ve = v, se = sqrt(v / b22);
                if (writer) {
                    const double praw = (isfinite(se) && se > 0.0) ? lm_student_t_two_sided(b / se, df, ln_beta) : 1.0;
                    p = (isfinite(se) && se > 0.0 && isfinite(praw)) ? fmin(fmax(praw, LM_MIN_POS), 1.0) : 1.0;
                }
            }
        }
    }
    if (writer && live) {
        double *o = out + (int64_t)row * 3;
        o[0] = beta, o[1] = se, o[2] = p;
    }
    if (kq <= 0 || final_form) return;

#pragma unroll
    for (int s = 0; s < FC_SLOTS_PER_WAVE; ++s) {
        const int sl = 4 * s + wave;
        if (sl >= kq) break;                                    // wave-uniform
        double t2 = 0.0;
        if (ok) {
            const double b21 = acc[s];
            const double bq = bgb[sl] - b21 * beta;
            const double se2 = (dixx[sl] + b21 * b21 / b22) * ve;
            if (isfinite(bq) && isfinite(se2) && se2 > 0.0) {
                const double q = bq * bq / se2;
                if (q == q) t2 = q;                             // +inf stays: the largest pattern, p = the smallest positive
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t2 = fmax(t2, __shfl_xor(t2, off, 64));
        if (lane == 0 && t2 > 0.0) atomicMax(&maxbits[sl], (unsigned long long)__double_as_longlong(t2));
    }
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_farmcpu_max_qtn(void) { return FC_MAX_QTN; }

static int fc_launch(const char *who, const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy,
                     int64_t ldg, const double *d_ss, int nrows, double bg_rss, int df, const double *d_w, int64_t ldw, int k_qtn,
                     const double *d_bgb, const double *d_dixx, int final_form, double *d_out, uint64_t *d_maxbits,
                     void *stream) {
    if (nrows <= 0) return 0;
    const std::string me(who);
    if (rank < 0 || rank > FC_MAX_RANK)
        return fail(me + ": rank of the design = " + std::to_string(rank) + " is above the cap of " + std::to_string(FC_MAX_RANK));
    if (k_qtn < 0 || k_qtn > FC_MAX_QTN)
        return fail(me + ": " + std::to_string(k_qtn) + " pseudo-QTN columns are above the cap of " + std::to_string(FC_MAX_QTN) +
                    " (lower the QTN bound)");
    if (rank > 0 && (!d_qg || ldq < rank)) return fail(me + ": the sums of Q are missing or ldq < rank");
    if (!d_gy || ldg < 1 || !d_ss || !d_out) return fail(me + ": operand missing");
    if (k_qtn > 0 && (!d_w || ldw < rank || !d_bgb || !d_dixx || !d_maxbits)) return fail(me + ": pseudo-QTN operands missing");
    if (!(bg_rss == bg_rss)) return fail(me + ": the background RSS is NaN");
    const double ln_beta = df > 0 ? lgamma(0.5 * df) + lgamma(0.5) - lgamma(0.5 * df + 0.5) : 0.0;
    const int64_t blocks = ((int64_t)nrows + FC_ROWS - 1) / FC_ROWS;
    const int batches = k_qtn > 0 ? (k_qtn + FC_SLOT_BATCH - 1) / FC_SLOT_BATCH : 1;
    hipLaunchKernelGGL(fc_stats_kernel, dim3((unsigned)blocks, (unsigned)batches), dim3(256), 0, (hipStream_t)stream, d_qg, d_qg_lo, ldq, rank, d_gy,
                       ldg, d_ss, nrows, bg_rss, df, ln_beta, d_w, ldw, k_qtn, d_bgb, d_dixx, final_form, d_out,
                       reinterpret_cast<unsigned long long *>(d_maxbits));
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_farmcpu_fem_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy,
                                     int64_t ldg, const double *d_ss, int nrows, double bg_rss, int df, const double *d_w, int64_t ldw,
                                     int k_qtn, const double *d_bg_beta, const double *d_diag_ixx, double *d_out,
                                     uint64_t *d_max_t2_bits, void *stream) {
    return fc_launch("jxg_farmcpu_fem_stats", d_qg, d_qg_lo, ldq, rank, d_gy, ldg, d_ss, nrows, bg_rss, df, d_w, ldw, k_qtn, d_bg_beta,
                     d_diag_ixx, 0, d_out, d_max_t2_bits, stream);
}

extern "C" int jxg_farmcpu_final_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy,
                                       int64_t ldg, const double *d_ss, int nrows, double bg_rss, int df, double *d_out, void *stream) {
    return fc_launch("jxg_farmcpu_final_stats", d_qg, d_qg_lo, ldq, rank, d_gy, ldg, d_ss, nrows, bg_rss, df, nullptr, 0, 0, nullptr,
                     nullptr, 1, d_out, nullptr, stream);
}
