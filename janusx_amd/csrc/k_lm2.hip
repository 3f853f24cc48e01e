// SNP-by-covariate interaction scan (`jx gwas -lm2`, src/stats/glm2.rs:142-325): per SNP the model
//   y ~ X + g + g o c_1 + ... + g o c_k        (z_0 = v, z_j = v c_j, v = additive value of the 2-bit code)
// needs  e_a = sum z_a r_y,  C[t][a] = sum Q_it z_a,  D[a][b] = sum z_a z_b  over the samples.  Every one of them is a sum of
// v w or v^2 w for a weight column w that does not depend on the SNP:
//   v   against  c_a Q_t  and  c_a r_y     (c_0 = 1):  (q_rank + 1)(k + 1) columns, column a (q_rank + 1) + t, t = q_rank for r_y
//   v^2 against  c_a c_b  (b <= a):        (k + 1)(k + 2) / 2 columns, column a (a + 1) / 2 + b
// The host builds the weight columns once per trait, pads each group to whole blocks of 16 and lays them out as the A operand
// of v_mfma_f64_16x16x4_f64:  w[tile][block][ks][lane] = column 16 block + (lane & 15) at sample 128 tile + 4 ks + (lane >> 4),
// zero beyond n.  lm2_moments_kernel makes ONE streaming pass over the P32 records (p32[tile][snp][32 B], 128 samples per
// record) of 16 SNPs per wave: the decoded v (or v^2) of SNP lane & 15 at sample 4 ks + (lane >> 4) is the B operand, the
// 128-sample tile of up to L2_MAXB weight blocks is staged in LDS and shared by the workgroup's L2_WAVES waves, the sums stay in
// the accumulators over all tiles.  More than L2_MAXB blocks: one pass per L2_MAXB blocks.  No atomics: a SNP's sums depend on
// its own operand column alone, in a fixed order, so they are the same bits for every blocking of the rows.
// lm2_stats_kernel then does the per-SNP algebra (one thread per SNP, m = 1 + k <= 9).
#include <cmath>

#include "jx_common.h"
#include "lm_pvalue.h"

namespace jx {

constexpr int L2_WAVES = 4;                 // waves per workgroup
constexpr int L2_SNPS = 16;                 // SNPs per wave (the N side of the MFMA)
constexpr int L2_ROWS = L2_WAVES * L2_SNPS; // SNP rows per workgroup
constexpr int L2_MAXB = 4;                  // weight blocks (of 16 columns) per pass: 4 x 16 KB of LDS
constexpr int L2_BLK = 32 * 64;             // doubles of one weight block of one 128-sample tile
constexpr int L2_MAXM = 9;                  // 1 + k

typedef double l2_v4d __attribute__((ext_vector_type(4)));

// sums[r][16 (b0 + b) + e] = sum_i f_b(v(r, i)) column(16 (b0 + b) + e)[i],  f_b = v^2 where bit b of sq_mask is set, else v.
template <int NB>
__global__ __launch_bounds__(L2_WAVES * 64) void lm2_moments_kernel(const uint8_t *__restrict__ p32, int64_t m_total,
                                                                    const int32_t *__restrict__ rows, int nrows,
                                                                    const float *__restrict__ lut,
                                                                    const double *__restrict__ w, int nblk, int b0,
                                                                    uint32_t sq_mask, int ntiles,
                                                                    double *__restrict__ sums, int lds) {
    __shared__ __attribute__((aligned(16))) double wt[NB * L2_BLK];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, fk = lane >> 4;
    const int r = blockIdx.x * L2_ROWS + wave * L2_SNPS + fi;
    const bool live = r < nrows;
    const int64_t rec = live ? (rows ? (int64_t)rows[r] : (int64_t)r) : 0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (live) {
        const float4 l = *reinterpret_cast<const float4 *>(lut + (int64_t)r * 4);
        v0 = (double)l.x, v1 = (double)l.y, v2 = (double)l.z, v3 = (double)l.w;
    }
    const double s0 = v0 * v0, s1 = v1 * v1, s2 = v2 * v2, s3 = v3 * v3;
    l2_v4d acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = (l2_v4d){0.0, 0.0, 0.0, 0.0};
    for (int tile = 0; tile < ntiles; ++tile) {
        __syncthreads();
        {
            // 16-byte loads: the image is 16 KB per block and tile, so every block starts 16-byte aligned
            const double2 *src = reinterpret_cast<const double2 *>(w + ((int64_t)tile * nblk + b0) * L2_BLK);
            double2 *dst = reinterpret_cast<double2 *>(wt);
            for (int i = tid; i < NB * L2_BLK / 2; i += L2_WAVES * 64) dst[i] = src[i];
        }
        __syncthreads();
        const uint4 *p = reinterpret_cast<const uint4 *>(p32 + ((int64_t)tile * m_total + rec) * 32);
        const uint4 w0 = p[0], w1 = p[1];
        const uint32_t words[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) {
            // sample 4 ks + fk of the record: word (4 ks + fk) >> 4 = ks >> 2, code ((4 ks + fk) & 15)
            const uint32_t code = (words[ks >> 2] >> (2 * (4 * (ks & 3) + fk))) & 3u;
            const double lo = (code & 1u) ? v1 : v0, hi = (code & 1u) ? v3 : v2;
            const double slo = (code & 1u) ? s1 : s0, shi = (code & 1u) ? s3 : s2;
            const double v = (code & 2u) ? hi : lo;
            const double sq = (code & 2u) ? shi : slo;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double a = wt[(b * 32 + ks) * 64 + lane];
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ((sq_mask >> b) & 1u) ? sq : v, acc[b], 0, 0, 0);
            }
        }
    }
    if (!live) return;
    // D[column = (lane >> 4) + 4 j][SNP = lane & 15]
    double *o = sums + (int64_t)r * lds + (int64_t)b0 * 16 + fk;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[b * 16 + 4 * j] = acc[b][j];
}

// ---- chi-square tail (src/math/linalg.rs:20-96) ------------------------------------------------------------------------
__device__ double lm2_gamma_q(double a, double x) {
    if (!(isfinite(a) && isfinite(x)) || a <= 0.0) return NAN;
    if (x <= 0.0) return 1.0;
    const int itmax = 200;
    const double eps = 3e-14, fpmin = 1e-300;
    const double gln = lgamma(a);
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int i = 0; i < itmax; ++i) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (fabs(del) <= fabs(sum) * eps) break;
        }
        const double p = sum * exp(-x + a * log(x) - gln);
        return fmin(fmax(1.0 - p, 0.0), 1.0);
    }
    double b = x + 1.0 - a, c = 1.0 / fpmin, d = 1.0 / fmax(b, fpmin), h = d;
    for (int i = 1; i <= itmax; ++i) {
        const double fi = (double)i, an = -fi * (fi - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < fpmin) d = fpmin;
        c = b + an / c;
        if (fabs(c) < fpmin) c = fpmin;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return fmin(fmax(exp(-x + a * log(x) - gln) * h, 0.0), 1.0);
}

__device__ double lm2_chi2_sf(double stat, int df) {
    if (!isfinite(stat) || stat <= 0.0 || df <= 0) return 1.0;
    double p = (df == 1) ? erfc(sqrt(0.5 * stat)) : lm2_gamma_q(0.5 * (double)df, 0.5 * stat);
    if (!isfinite(p)) return 1.0;
    return fmin(fmax(p, LM_MIN_POS), 1.0);
}

// inv = a^-1 by Gauss-Jordan elimination with partial pivoting (a is destroyed; both m x m with row pitch L2_MAXM).
// false when a pivot is exactly zero or not finite: the caller leaves such a row to the host's pseudo-inverse.
__device__ bool lm2_invert(double *a, double *inv, int m) {
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) inv[i * L2_MAXM + j] = (i == j) ? 1.0 : 0.0;
    for (int c = 0; c < m; ++c) {
        int p = c;
        double best = fabs(a[c * L2_MAXM + c]);
        for (int i = c + 1; i < m; ++i) {
            const double t = fabs(a[i * L2_MAXM + c]);
            if (t > best) best = t, p = i;
        }
        const double piv = a[p * L2_MAXM + c];
        if (!isfinite(piv) || piv == 0.0) return false;
        if (p != c)
            for (int j = 0; j < m; ++j) {
                double t = a[c * L2_MAXM + j];
                a[c * L2_MAXM + j] = a[p * L2_MAXM + j], a[p * L2_MAXM + j] = t;
                t = inv[c * L2_MAXM + j];
                inv[c * L2_MAXM + j] = inv[p * L2_MAXM + j], inv[p * L2_MAXM + j] = t;
            }
        for (int j = 0; j < m; ++j) a[c * L2_MAXM + j] /= piv, inv[c * L2_MAXM + j] /= piv;
        for (int i = 0; i < m; ++i) {
            if (i == c) continue;
            const double f = a[i * L2_MAXM + c];
            if (f == 0.0) continue;
            for (int j = 0; j < m; ++j) {
                a[i * L2_MAXM + j] -= f * a[c * L2_MAXM + j];
                inv[i * L2_MAXM + j] -= f * inv[c * L2_MAXM + j];
            }
        }
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
            if (!isfinite(inv[i * L2_MAXM + j])) return false;
    return true;
}

// out[r] = (beta, se, chisq, pwald) x (1 + k), chisq_int_joint, p_int_joint, chisq_joint, p_joint;  flag[r] = 1 (and NaN in
// out[r]) where S or the interaction block of S^-1 has no plain inverse.  glm2.rs:238-325.
__global__ __launch_bounds__(64) void lm2_stats_kernel(const double *__restrict__ sums, int lds, int nrows, int qr, int k,
                                                      int sq0, double rss0, int df, double ln_beta,
                                                      double *__restrict__ out, int32_t *__restrict__ flag) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= nrows) return;
    const int m = 1 + k, ncol = 4 * m + 4;
    const double *u = sums + (int64_t)r * lds;
    double *o = out + (int64_t)r * ncol;
    double s[L2_MAXM * L2_MAXM], inv[L2_MAXM * L2_MAXM], e[L2_MAXM], beta[L2_MAXM];
    bool ok = true;
    for (int a = 0; a < m; ++a) {
        e[a] = u[a * (qr + 1) + qr];
        for (int b = 0; b <= a; ++b) {
            double cc = 0.0;
            for (int t = 0; t < qr; ++t) cc += u[a * (qr + 1) + t] * u[b * (qr + 1) + t];
            const double v = u[sq0 + a * (a + 1) / 2 + b] - cc;
            s[a * L2_MAXM + b] = s[b * L2_MAXM + a] = v;
            ok = ok && isfinite(v);
        }
    }
    ok = ok && lm2_invert(s, inv, m);
    double eb = 0.0, sigma2 = NAN;
    bool s2ok = false;
    if (ok) {
        for (int a = 0; a < m; ++a) {
            double acc = 0.0;
            for (int b = 0; b < m; ++b) acc += inv[a * L2_MAXM + b] * e[b];
            beta[a] = acc;
        }
        for (int a = 0; a < m; ++a) eb += e[a] * beta[a];
        sigma2 = fmax(rss0 - eb, 0.0) / (double)df;
        s2ok = isfinite(sigma2) && sigma2 > 0.0;
    }
    double ci = NAN, pi = 1.0;
    if (ok && k > 0 && s2ok) {
        double blk[L2_MAXM * L2_MAXM], binv[L2_MAXM * L2_MAXM];
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) blk[i * L2_MAXM + j] = inv[(1 + i) * L2_MAXM + 1 + j];
        if (lm2_invert(blk, binv, k)) {
            double q = 0.0;
            for (int i = 0; i < k; ++i) {
                double acc = 0.0;
                for (int j = 0; j < k; ++j) acc += binv[i * L2_MAXM + j] * beta[1 + j];
                q += beta[1 + i] * acc;
            }
            ci = fmax(q / sigma2, 0.0);
            pi = lm2_chi2_sf(ci, k);
        } else {
            ok = false;
        }
    }
    flag[r] = ok ? 0 : 1;
    if (!ok) {
        for (int j = 0; j < ncol; ++j) o[j] = NAN;
        return;
    }
    for (int a = 0; a < m; ++a) {
        const double b = beta[a], var = sigma2 * inv[a * L2_MAXM + a];
        const double se = (isfinite(var) && var > 0.0) ? sqrt(var) : NAN;
        double chisq = NAN, pw = 1.0;
        if (isfinite(b) && isfinite(se) && se > 0.0) {
            const double t = b / se;
            chisq = t * t;
            pw = lm_student_t_two_sided(t, df, ln_beta);
            pw = isfinite(pw) ? fmin(fmax(pw, LM_MIN_POS), 1.0) : 1.0;
        }
        o[4 * a] = b, o[4 * a + 1] = se, o[4 * a + 2] = chisq, o[4 * a + 3] = pw;
    }
    double cj = NAN, pj = 1.0;
    if (s2ok) {
        cj = fmax(eb / sigma2, 0.0);
        pj = lm2_chi2_sf(cj, m);
    }
    o[4 * m] = ci, o[4 * m + 1] = pi, o[4 * m + 2] = cj, o[4 * m + 3] = pj;
}

}  // namespace jx

using namespace jx;

// LM2 scan of `nrows` SNPs of a resident P32 image.  d_lut (nrows, 4) f32 = additive value by 2-bit code; d_w = the weight image
// described at the top, (tiles, nblk, 32, 64) f64, blocks [0, nblk_v) against v and [nblk_v, nblk) against v^2; d_sums
// (nrows, 16 nblk) f64; d_out (nrows, 4 (1 + k) + 4) f64; d_flag (nrows) i32.  stage: 0 both kernels, 1 the moments, 2 the algebra.
extern "C" int jxg_lm2_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                const float *d_lut, const double *d_w, int nblk, int nblk_v, int q_rank, int k,
                                double rss0, int df, double *d_sums, double *d_out, int32_t *d_flag, int stage,
                                void *stream) {
    if (nrows <= 0) return 0;
    if (k < 1 || k > L2_MAXM - 1) return fail("LM2 supports 1 .. 8 interaction covariates, got " + std::to_string(k));
    if (q_rank < 0 || df <= 0 || n <= 0) return fail("n too small: require n > q_base + 1 + n_interactions");
    const int m = 1 + k;
    const int need_v = ((q_rank + 1) * m + 15) / 16, need_s = (m * (m + 1) / 2 + 15) / 16;
    if (nblk_v != need_v || nblk != need_v + need_s) return fail("jxg_lm2_scan_p32: weight image does not match q_rank and k");
    if (stage < 0 || stage > 2) return fail("jxg_lm2_scan_p32: stage must be 0, 1 or 2");
    hipStream_t st = (hipStream_t)stream;
    const int lds = nblk * 16, ntiles = num_tiles(n);
    if (stage != 2) {
        const dim3 grid((nrows + L2_ROWS - 1) / L2_ROWS), block(L2_WAVES * 64);
        for (int b0 = 0; b0 < nblk; b0 += L2_MAXB) {
            const int nb = std::min(L2_MAXB, nblk - b0);
            uint32_t mask = 0;
            for (int b = 0; b < nb; ++b)
                if (b0 + b >= nblk_v) mask |= 1u << b;
            switch (nb) {
            case 1: hipLaunchKernelGGL(lm2_moments_kernel<1>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, d_lut, d_w, nblk, b0, mask, ntiles, d_sums, lds); break;
            case 2: hipLaunchKernelGGL(lm2_moments_kernel<2>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, d_lut, d_w, nblk, b0, mask, ntiles, d_sums, lds); break;
            case 3: hipLaunchKernelGGL(lm2_moments_kernel<3>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, d_lut, d_w, nblk, b0, mask, ntiles, d_sums, lds); break;
            default: hipLaunchKernelGGL(lm2_moments_kernel<4>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, d_lut, d_w, nblk, b0, mask, ntiles, d_sums, lds); break;
            }
            JX_LAUNCH_CHECK();
        }
    }
    if (stage != 1) {
        const double ln_beta = lgamma(0.5 * df) + lgamma(0.5) - lgamma(0.5 * df + 0.5);
        hipLaunchKernelGGL(lm2_stats_kernel, dim3((nrows + 63) / 64), dim3(64), 0, st, d_sums, lds, nrows, q_rank, k,
                           nblk_v * 16, rss0, df, ln_beta, d_out, d_flag);
        JX_LAUNCH_CHECK();
    }
    return 0;
}
