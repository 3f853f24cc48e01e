// Joint SNP-pair interaction test under the fixed-lambda LMM (`jx fvlmm2`, src/stats/fvlmm2.rs:37-290;
// rows of python/janusx/script/fvlmm2.py:648-806).  Per pair r the model is
//   y ~ X + g1 + g2 + combo(g1, g2)        with weights W = 1 / (s + lambda) on rotated rows,
// a Wald test for each of the three pair terms.
//
// fvlmm2_combo_kernel: g1, g2 and the combo row of every pair straight from the P32 image.  All three are functions of the
//   two 2-bit codes alone (decoded rows are lut[code]; literals, min / max / xor and the f32 product are tables of the two
//   codes), so the host hands three small tables per pair and the kernel makes one pass over the two 32-byte records of each
//   128-sample tile.  One wave per pair, a lane owns four consecutive samples (one byte of each record, one 16-byte store per
//   output row where the address allows it); the positive-value counts of the af columns are summed in the wave, no atomics.
// fvlmm2_prep_kernel / fvlmm2_base_kernel: 1 / (s + lambda) with the argument checks of :119-149, and the covariate block
//   X'WX, X'Wy that every pair shares (:130-149).
// fvlmm2_joint_kernel: one wave per pair.  Pass 1: the 9 + 3 p_cov pair-specific weighted sums in f64, lanes striding the
//   samples, butterfly reduction.  Lane 0 assembles Z'WZ in LDS, adds the 1e-6 ridge, factors (pivot floor 1e-18) and solves.
//   Pass 2 (the rows are hot in L2): r'Wr with r = y - Z beta, explicitly, as the reference does.  Lane 0 then writes the
//   three tests.  The file is compiled without FMA contraction (csrc/Makefile: -ffp-contract=off), so every product and sum
//   below is rounded as written.
#include <algorithm>
#include <cmath>

#include "jx_common.h"
#include "scan_common.h"

namespace jx {

constexpr int F2_MAXD = 16;                 // p_cov + 3 <= 16: the largest MAXD the scan kernels instantiate
constexpr int F2_MAXP = F2_MAXD - 3;

// pos[r]: bits 0..3 literal 1 > 0 by code, bits 4..7 literal 2 > 0 by code, bits 8..23 combo > 0 by 4 c1 + c2
__global__ __launch_bounds__(64) void fvlmm2_combo_kernel(const uint8_t *__restrict__ p32, int64_t m_total,
                                                          const int32_t *__restrict__ rows1,
                                                          const int32_t *__restrict__ rows2, int nrows,
                                                          const float *__restrict__ lut1, const float *__restrict__ lut2,
                                                          const float *__restrict__ tab, const uint32_t *__restrict__ pos,
                                                          int n, int ntiles, float *__restrict__ g1,
                                                          float *__restrict__ g2, float *__restrict__ gc, int64_t ld,
                                                          int32_t *__restrict__ cnt) {
    __shared__ float t[24];                 // lut1 (4), lut2 (4), tab (16) of this pair
    const int lane = threadIdx.x;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        __syncthreads();
        if (lane < 4) t[lane] = lut1[(int64_t)r * 4 + lane];
        else if (lane < 8) t[lane] = lut2[(int64_t)r * 4 + lane - 4];
        else if (lane < 24) t[lane] = tab[(int64_t)r * 16 + lane - 8];
        __syncthreads();
        const int64_t rec1 = rows1[r], rec2 = rows2[r];
        const bool inside = rec1 >= 0 && rec1 < m_total && rec2 >= 0 && rec2 < m_total;   // a record outside the image is never read
        const uint32_t pm = pos[r];
        const int half = lane >> 5, q = lane & 31;
        float *o1 = g1 + (int64_t)r * ld, *o2 = g2 + (int64_t)r * ld, *oc = gc + (int64_t)r * ld;
        int n1 = 0, n2 = 0, nc = 0;
        for (int t0 = 0; t0 < ntiles; t0 += 2) {
            const int tile = t0 + half;
            const int i0 = tile * JXG_TILE + 4 * q;
            if (tile >= ntiles || i0 >= n) continue;
            uint32_t b1 = 0x55u, b2 = 0x55u;
            if (inside) {
                b1 = p32[((int64_t)tile * m_total + rec1) * 32 + q];     // byte q of a record: samples 4 q .. 4 q + 3
                b2 = p32[((int64_t)tile * m_total + rec2) * 32 + q];
            }
            float v1[4], v2[4], vc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t c1 = (b1 >> (2 * k)) & 3u, c2 = (b2 >> (2 * k)) & 3u;
                v1[k] = inside ? t[c1] : NAN;
                v2[k] = inside ? t[4 + c2] : NAN;
                vc[k] = inside ? t[8 + 4 * c1 + c2] : NAN;
                if (inside && i0 + k < n) {
                    n1 += (int)((pm >> c1) & 1u);
                    n2 += (int)((pm >> (4 + c2)) & 1u);
                    nc += (int)((pm >> (8 + 4 * c1 + c2)) & 1u);
                }
            }
            const bool vec = i0 + 3 < n &&                                         // 16-byte aligned in all three blocks
                             (((uintptr_t)(o1 + i0) | (uintptr_t)(o2 + i0) | (uintptr_t)(oc + i0)) & 15u) == 0;
            if (vec) {
                *reinterpret_cast<float4 *>(o1 + i0) = make_float4(v1[0], v1[1], v1[2], v1[3]);
                *reinterpret_cast<float4 *>(o2 + i0) = make_float4(v2[0], v2[1], v2[2], v2[3]);
                *reinterpret_cast<float4 *>(oc + i0) = make_float4(vc[0], vc[1], vc[2], vc[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i0 + k < n) o1[i0 + k] = v1[k], o2[i0 + k] = v2[k], oc[i0 + k] = vc[k];
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n1 += __shfl_xor(n1, off, 64);
            n2 += __shfl_xor(n2, off, 64);
            nc += __shfl_xor(nc, off, 64);
        }
        if (lane == 0) cnt[(int64_t)r * 3] = n1, cnt[(int64_t)r * 3 + 1] = n2, cnt[(int64_t)r * 3 + 2] = nc;
    }
}

// vinv[i] = 1 / (s[i] + lambda).  first[0] = the lowest sample whose s + lambda is not finite and positive; first[1] = the lowest
// key 2 i + (y_i finite) among the samples with a non-finite y_i or covariate: the sample the reference's loop meets first, and
// whether it stops at its y (looked at before its covariates).  Both start at 0xffffffff = none.
__global__ __launch_bounds__(256) void fvlmm2_prep_kernel(const double *__restrict__ s, const double *__restrict__ xcov,
                                                          const double *__restrict__ y, int n, int p, double lbd,
                                                          double *__restrict__ vinv, uint32_t *__restrict__ first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double vv = s[i] + lbd;
    vinv[i] = 1.0 / vv;
    if (!isfinite(vv) || vv <= 0.0) atomicMin(&first[0], (uint32_t)i);
    const bool y_ok = isfinite(y[i]);
    bool x_ok = true;
    for (int c = 0; c < p; ++c) x_ok = x_ok && isfinite(xcov[(int64_t)i * p + c]);
    if (!(y_ok && x_ok)) atomicMin(&first[1], 2u * (uint32_t)i + (y_ok ? 1u : 0u));
}

// base[r * dim + c] = sum_i vinv x_ir x_ic (r, c < p; zero elsewhere), base[dim * dim + r] = sum_i vinv x_ir y_i.
// One workgroup per entry: blockIdx.x = r * (p + 1) + c, c = p for the right-hand side.
__global__ __launch_bounds__(256) void fvlmm2_base_kernel(const double *__restrict__ vinv, const double *__restrict__ xcov,
                                                          const double *__restrict__ y, int n, int p, int dim,
                                                          double *__restrict__ base) {
    __shared__ double red[SCAN_WAVES];
    const int r = blockIdx.x / (p + 1), c = blockIdx.x % (p + 1);
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double vx = vinv[i] * xcov[(int64_t)i * p + r];
        acc += vx * (c < p ? xcov[(int64_t)i * p + c] : y[i]);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = red[0];
        for (int w = 1; w < SCAN_WAVES; ++w) tot += red[w];
        if (c < p) base[r * dim + c] = tot;
        else base[dim * dim + r] = tot;
    }
}

// Cholesky factor of the dim x dim matrix m (pitch dim, LDS, one lane) into its lower triangle, column by column: the pivot of
// column c, then the entries below it.  False at the first pivot that is not above the floor 1e-18 (a NaN pivot included).
__device__ bool f2_factor(double *m, int dim) {
    for (int c = 0; c < dim; ++c) {
        double *rc = m + c * dim;
        double piv = rc[c];
        for (int k = 0; k < c; ++k) piv -= rc[k] * rc[k];
        if (!(piv > 1e-18)) return false;
        rc[c] = sqrt(piv);
        for (int r = c + 1; r < dim; ++r) {
            double *rr = m + r * dim;
            double v = rr[c];
            for (int k = 0; k < c; ++k) v -= rr[k] * rc[k];
            rr[c] = v / rc[c];
        }
    }
    return true;
}

// x <- (L L')^-1 x in place with the lower factor L: each solved unknown is taken out of the equations that still hold it
__device__ void f2_solve_inplace(const double *l, int dim, double *x) {
    for (int c = 0; c < dim; ++c) {                 // L z = x
        x[c] /= l[c * dim + c];
        for (int r = c + 1; r < dim; ++r) x[r] -= l[r * dim + c] * x[c];
    }
    for (int c = dim - 1; c >= 0; --c) {            // L' w = z
        x[c] /= l[c * dim + c];
        for (int r = 0; r < c; ++r) x[r] -= l[c * dim + r] * x[c];
    }
}

__device__ __forceinline__ void f2_nan9(double *o) {
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = NAN;
}

// out[r] = (beta1, se1, p1, beta2, se2, p2, betac, sec, pc).  PC: compile-time bound of p (the accumulators stay in registers).
template <int PC>
__global__ __launch_bounds__(64) void fvlmm2_joint_kernel(const float *__restrict__ g1b, const float *__restrict__ g2b,
                                                          const float *__restrict__ gcb, int nrows, int n, int64_t ld,
                                                          const double *__restrict__ vinv, const double *__restrict__ xcov,
                                                          int p, const double *__restrict__ y,
                                                          const double *__restrict__ base, double *__restrict__ out) {
    __shared__ double a[F2_MAXD * F2_MAXD];
    __shared__ double beta[F2_MAXD], col[F2_MAXD];
    __shared__ int ok_s;
    const int lane = threadIdx.x;
    const int dim = p + 3, j1 = p, j2 = p + 1, jc = p + 2;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {      // r and every branch below are uniform over the wave
        const float *g1 = g1b + (int64_t)r * ld, *g2 = g2b + (int64_t)r * ld, *gc = gcb + (int64_t)r * ld;
        double *o = out + (int64_t)r * 9;
        __syncthreads();                                       // the previous row's lane 0 is done with the LDS state
        double ey1 = 0.0, ey2 = 0.0, eyc = 0.0, s11 = 0.0, s12 = 0.0, s1c = 0.0, s22 = 0.0, s2c = 0.0, scc = 0.0;
        double x1[PC], x2[PC], xc[PC];
#pragma unroll
        for (int c = 0; c < PC; ++c) x1[c] = x2[c] = xc[c] = 0.0;
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const double a1 = (double)g1[i], a2 = (double)g2[i], ac = (double)gc[i];
            if (!(isfinite(a1) && isfinite(a2) && isfinite(ac))) bad = true;
            const double vi = vinv[i], yi = y[i];
            ey1 += vi * a1 * yi;
            ey2 += vi * a2 * yi;
            eyc += vi * ac * yi;
#pragma unroll
            for (int c = 0; c < PC; ++c)
                if (c < p) {
                    const double xic = xcov[(int64_t)i * p + c];
                    x1[c] += vi * xic * a1;
                    x2[c] += vi * xic * a2;
                    xc[c] += vi * xic * ac;
                }
            s11 += vi * a1 * a1;
            s12 += vi * a1 * a2;
            s1c += vi * a1 * ac;
            s22 += vi * a2 * a2;
            s2c += vi * a2 * ac;
            scc += vi * ac * ac;
        }
        if (__any(bad)) {                                      // any non-finite value of the 3 n: nine NaN
            if (lane == 0) f2_nan9(o);
            continue;
        }
        ey1 = wave_allsum(ey1), ey2 = wave_allsum(ey2), eyc = wave_allsum(eyc);
        s11 = wave_allsum(s11), s12 = wave_allsum(s12), s1c = wave_allsum(s1c);
        s22 = wave_allsum(s22), s2c = wave_allsum(s2c), scc = wave_allsum(scc);
#pragma unroll
        for (int c = 0; c < PC; ++c)
            if (c < p) x1[c] = wave_allsum(x1[c]), x2[c] = wave_allsum(x2[c]), xc[c] = wave_allsum(xc[c]);
        for (int k = lane; k < dim * dim; k += 64) a[k] = base[k];
        if (lane < dim) beta[lane] = lane < p ? base[dim * dim + lane] : 0.0;      // Z'Wy, solved in place into beta
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < PC; ++c)
                if (c < p) {
                    a[c * dim + j1] = a[j1 * dim + c] = x1[c];
                    a[c * dim + j2] = a[j2 * dim + c] = x2[c];
                    a[c * dim + jc] = a[jc * dim + c] = xc[c];
                }
            a[j1 * dim + j1] = s11;
            a[j1 * dim + j2] = a[j2 * dim + j1] = s12;
            a[j1 * dim + jc] = a[jc * dim + j1] = s1c;
            a[j2 * dim + j2] = s22;
            a[j2 * dim + jc] = a[jc * dim + j2] = s2c;
            a[jc * dim + jc] = scc;
            beta[j1] = ey1, beta[j2] = ey2, beta[jc] = eyc;
            for (int d = 0; d < dim; ++d) a[d * dim + d] += 1e-6;
            const bool ok = f2_factor(a, dim);
            if (ok) f2_solve_inplace(a, dim, beta);
            ok_s = ok ? 1 : 0;
        }
        __syncthreads();
        if (!ok_s) {
            if (lane == 0) f2_nan9(o);
            continue;
        }
        double rr = 0.0;
        const double b1 = beta[j1], b2 = beta[j2], bc = beta[jc];
        for (int i = lane; i < n; i += 64) {
            double xb = (double)g1[i] * b1 + (double)g2[i] * b2 + (double)gc[i] * bc;
            for (int c = 0; c < p; ++c) xb += xcov[(int64_t)i * p + c] * beta[c];
            const double ri = y[i] - xb;
            rr += vinv[i] * ri * ri;
        }
        rr = wave_allsum(rr);
        if (lane == 0) {
            const double df = (double)(n - dim);
            const double sigma2 = rr / df;
            f2_nan9(o);
            if (isfinite(rr) && rr > 0.0 && df > 0.0 && isfinite(sigma2) && sigma2 > 0.0) {
                const int cols[3] = {j1, j2, jc};
                for (int t = 0; t < 3; ++t) {
                    const int ci = cols[t];
                    for (int d = 0; d < dim; ++d) col[d] = d == ci ? 1.0 : 0.0;
                    f2_solve_inplace(a, dim, col);
                    const double var = sigma2 * col[ci];
                    if (!(isfinite(var) && var > 0.0)) break;          // the earlier coefficients stay written (:257-281)
                    const double se = sqrt(var), bj = beta[ci], z = bj / se;
                    const double pv = isfinite(z) ? fmin(fmax(2.0 * normal_sf_dev(fabs(z)), 2.2250738585072014e-308), 1.0) : NAN;
                    o[3 * t] = bj, o[3 * t + 1] = se, o[3 * t + 2] = pv;
                }
            }
        }
    }
}

}  // namespace jx

using namespace jx;

// g1, g2, combo rows and positive-value counts of `nrows` SNP pairs of a P32 image (see include/jxgpu.h).
extern "C" int jxg_fvlmm2_combo_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows1,
                                    const int32_t *d_rows2, int nrows, const float *d_lut1, const float *d_lut2,
                                    const float *d_tab, const uint32_t *d_pos, float *d_g1, float *d_g2, float *d_gc,
                                    int64_t ld, int32_t *d_counts, void *stream) {
    if (nrows <= 0) return 0;
    if (n <= 0 || m_total <= 0) return fail("jxg_fvlmm2_combo_p32: empty image");
    if (ld < n) return fail("jxg_fvlmm2_combo_p32: ld must be >= n");
    const int grid = std::min(nrows, 1 << 20);
    hipLaunchKernelGGL(fvlmm2_combo_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, d_p32, m_total, d_rows1,
                       d_rows2, nrows, d_lut1, d_lut2, d_tab, d_pos, n, num_tiles(n), d_g1, d_g2, d_gc, ld, d_counts);
    JX_LAUNCH_CHECK();
    return 0;
}

// Joint test of `nrows` pairs on rows that are used as given (see include/jxgpu.h).
extern "C" int jxg_fvlmm2_joint(const float *d_g1, const float *d_g2, const float *d_gc, int nrows, int n, int64_t ld,
                                const double *d_s, const double *d_xcov, int p_cov, const double *d_y, double lbd,
                                double *d_out, void *stream) {
    if (n <= 0) return fail("y_rot must not be empty");
    if (p_cov < 0 || p_cov > F2_MAXP)
        return fail("fvlmm2 joint test supports at most " + std::to_string(F2_MAXP) + " covariate columns (p_cov + 3 <= " +
                    std::to_string(F2_MAXD) + "), got p_cov=" + std::to_string(p_cov));
    if (!std::isfinite(lbd) || lbd <= 0.0) return fail("log10_lbd must map to a finite positive lambda");
    const int dim = p_cov + 3;
    if (n <= dim)
        return fail("n must be > p_cov + 3 for the joint test, got n=" + std::to_string(n) + ", p_cov=" + std::to_string(p_cov));
    if (ld < n) return fail("jxg_fvlmm2_joint: ld must be >= n");
    hipStream_t st = (hipStream_t)stream;
    AsyncBlock work;                        // vinv (n), base (dim^2 + dim), the two first-offender words
    const size_t nd = (size_t)n + (size_t)dim * dim + dim;
    if (work.alloc(sizeof(double) * nd + 16, st)) return 1;
    double *vinv = (double *)work.p, *base = vinv + n;
    uint32_t *first = (uint32_t *)(base + dim * dim + dim);
    JX_HIP(hipMemsetAsync(base, 0, sizeof(double) * ((size_t)dim * dim + dim), st));
    JX_HIP(hipMemsetAsync(first, 0xff, 2 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(fvlmm2_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_s, d_xcov, d_y, n, p_cov, lbd,
                       vinv, first);
    JX_LAUNCH_CHECK();
    uint32_t h_first[2] = {0, 0};
    JX_HIP(hipMemcpyAsync(h_first, first, sizeof(h_first), hipMemcpyDeviceToHost, st));
    JX_HIP(hipStreamSynchronize(st));
    if (h_first[0] != 0xffffffffu) return fail("S + lambda must stay finite and positive for all samples");
    if (h_first[1] != 0xffffffffu) return fail((h_first[1] & 1u) ? "xcov contains non-finite values" : "y_rot contains non-finite values");
    if (nrows <= 0) return 0;
    if (p_cov > 0) {
        hipLaunchKernelGGL(fvlmm2_base_kernel, dim3((unsigned)(p_cov * (p_cov + 1))), dim3(256), 0, st, vinv, d_xcov, d_y, n,
                           p_cov, dim, base);
        JX_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)std::min(nrows, 1 << 20)), block(64);
    if (p_cov <= 1)
        hipLaunchKernelGGL(fvlmm2_joint_kernel<1>, grid, block, 0, st, d_g1, d_g2, d_gc, nrows, n, ld, vinv, d_xcov, p_cov, d_y, base, d_out);
    else if (p_cov <= 4)
        hipLaunchKernelGGL(fvlmm2_joint_kernel<4>, grid, block, 0, st, d_g1, d_g2, d_gc, nrows, n, ld, vinv, d_xcov, p_cov, d_y, base, d_out);
    else if (p_cov <= 8)
        hipLaunchKernelGGL(fvlmm2_joint_kernel<8>, grid, block, 0, st, d_g1, d_g2, d_gc, nrows, n, ld, vinv, d_xcov, p_cov, d_y, base, d_out);
    else
        hipLaunchKernelGGL(fvlmm2_joint_kernel<F2_MAXP>, grid, block, 0, st, d_g1, d_g2, d_gc, nrows, n, ld, vinv, d_xcov, p_cov, d_y, base, d_out);
    JX_LAUNCH_CHECK();
    return 0;
}
