// ADMIXTURE / FastPop training passes over the resident P32 image (`jx adamixture`; reference
// `adam_optimize_packed_inplace_impl`, src/stats/adamixture.rs:5608-5898, `em_step_packed_f32_impl`, :5434-5606,
// `loglikelihood_packed_f32_impl`, :2957-3005).  Per called genotype g (minor-allele count after the row flip) of SNP j and
// sample i, with rec = clamp(sum_k p_jk q_ik, 1e-6, 1 - 1e-6) (an f32 dot product in k order, as the reference):
//     aa = g / rec,  bb = (2 - g) / (1 - rec)
//     a_jk += q_ik aa,  b_jk += q_ik bb,  t_ik += p_jk (aa - bb) + bb
// all from the same (P, Q); missing calls (code 01, and the padding samples of the last tile) contribute nothing.
//
// EM pass.  Workgroup (s1, s2) of 128 lanes owns SNP slice s1 (whole groups of 32 rows of the row list) and sample slice s2
// (whole 128-sample P32 tiles).  For every tile of its slice, lane = sample holds q_i and t_i in registers and walks the
// slice's SNP groups: phase 1 decodes the lane's code of each of the 32 rows, forms rec, aa and bb (one reciprocal of
// rec (1 - rec)), adds into t_i and parks aa / bb in LDS; phase 2 turns the 32 x 128 block around (lane = (row, quarter of
// the columns)) and adds AA Q and BB Q into the slice's partial rows of A and B (read-modify-write by this workgroup alone).
// At the end of a tile t_i is complete over the SNP slice and stored as partial s1.  Finalise kernels add the partials in a
// fixed order (f64): no float atomics, and two runs give the same bits.  Partial memory: 4 K (2 S2 nrows + S1 n) bytes, with
// S1 x S2 chosen by `ax_grid` under a fixed cap.
//
// K runs from 1 to 64: the kernels are instantiated for K padded to 1, 2, 4, 8, 16, 32 or 64 with zero columns (a zero column
// adds +0 to rec and is never written back).
#include <math.h>
#include <stdlib.h>

#include "jx_common.h"

namespace jx {

constexpr int AX_THREADS = 128;                // lanes per workgroup = samples per P32 tile
constexpr int AX_G = 32;                       // SNP rows per LDS group
constexpr int AX_LD = AX_THREADS + 1;          // row stride of the aa / bb blocks (phase 2 reads a column of rows)
constexpr int AX_MAX_K = 64;
constexpr float AX_EPS = 1e-5f;                // clip32 (src/stats/adamixture.rs:50-60)
constexpr float AX_REC_LO = 1e-6f, AX_REC_HI = 1.0f - 1e-6f;
constexpr int64_t AX_PART_CAP = (int64_t)8 << 30;   // partial-sum bytes at most (S1, S2 shrink to fit)

__device__ __forceinline__ float ax_clip(float v) { return fminf(fmaxf(v, AX_EPS), 1.0f - AX_EPS); }

// minor-allele count of a 2-bit code after the row flip (`packed_code_minor_allele_g`, :1632-1639); -1 = missing
__device__ __forceinline__ float ax_geno(uint32_t code, bool flip) {
    if (code == 1u) return -1.0f;
    const float d = code == 0u ? 0.0f : (code == 2u ? 1.0f : 2.0f);
    return flip ? 2.0f - d : d;
}

// the lane's code of row `rec` in sample tile `tile` (lane = sample within the tile)
__device__ __forceinline__ uint32_t ax_code(const uint32_t *__restrict__ p32, int64_t m_total, int tile, int64_t rec, int lane) {
    const uint32_t w = p32[((int64_t)tile * m_total + rec) * 8 + (lane >> 4)];
    return (w >> (2 * (lane & 15))) & 3u;
}

struct AxGrid {
    int s1, s2;          // SNP slices, sample slices
    int gps, tps;        // SNP groups per slice, sample tiles per slice
};

// slices: SNP groups and sample tiles spread over about 2048 workgroups, then halved (the larger partial first) until the
// partial sums fit AX_PART_CAP
static AxGrid ax_grid(int nrows, int n, int k) {
    const int ngroups = (nrows + AX_G - 1) / AX_G, ntiles = (n + AX_THREADS - 1) / AX_THREADS;
    int s1 = ngroups < 256 ? ngroups : 256;
    int s2 = 2048 / (s1 > 0 ? s1 : 1);
    if (s2 > ntiles) s2 = ntiles;
    if (s1 < 1) s1 = 1;
    if (s2 < 1) s2 = 1;
    for (;;) {
        const int64_t pa = 8LL * k * s2 * (int64_t)nrows, pt = 4LL * k * s1 * (int64_t)n;
        if (pa + pt <= AX_PART_CAP || (s1 == 1 && s2 == 1)) break;
        if ((pt >= pa && s1 > 1) || s2 == 1) s1 = (s1 + 1) / 2;
        else s2 = (s2 + 1) / 2;
    }
    AxGrid g;
    g.gps = (ngroups + s1 - 1) / s1;
    g.s1 = (ngroups + g.gps - 1) / g.gps;
    g.tps = (ntiles + s2 - 1) / s2;
    g.s2 = (ntiles + g.tps - 1) / g.tps;
    if (g.s1 < 1) g.s1 = 1;
    return g;
}

struct AxWork {
    float *apart, *bpart, *tpart, *qe;
    double *llpart;
    int *called;
};

static int64_t ax_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static int64_t ax_work_bytes(const AxGrid &g, int nrows, int n, int k) {
    return 2 * ax_align(4LL * k * g.s2 * (int64_t)nrows) + ax_align(4LL * k * g.s1 * (int64_t)n) + ax_align(4LL * k * n) +
           ax_align(8LL * g.s1 * g.s2) + ax_align(4LL * n);
}

static AxWork ax_carve(void *base, const AxGrid &g, int nrows, int n, int k) {
    char *p = (char *)base;
    AxWork w;
    w.apart = (float *)p; p += ax_align(4LL * k * g.s2 * (int64_t)nrows);
    w.bpart = (float *)p; p += ax_align(4LL * k * g.s2 * (int64_t)nrows);
    w.tpart = (float *)p; p += ax_align(4LL * k * g.s1 * (int64_t)n);
    w.qe = (float *)p; p += ax_align(4LL * k * n);
    w.llpart = (double *)p; p += ax_align(8LL * g.s1 * g.s2);
    w.called = (int *)p;
    return w;
}

// P rows j0 .. j0 + 31 of the slice into LDS, zero-padded to KB columns and past the slice end
template <int KB>
__device__ __forceinline__ void ax_load_p(float (*p_sh)[KB], const float *__restrict__ p, int k, int j0, int j1) {
    for (int e = threadIdx.x; e < AX_G * KB; e += AX_THREADS) {
        const int jj = e / KB, kk = e % KB;
        const int j = j0 + jj;
        p_sh[jj][kk] = (j < j1 && kk < k) ? p[(int64_t)j * k + kk] : 0.0f;
    }
}

template <int KB>
__global__ __launch_bounds__(AX_THREADS) void admx_em_pass_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                  const int32_t *__restrict__ rows, int nrows,
                                                                  const uint8_t *__restrict__ flip, int n, int k,
                                                                  const float *__restrict__ p, const float *__restrict__ q,
                                                                  int gps, int tps, int ntiles, float *__restrict__ apart,
                                                                  float *__restrict__ bpart, float *__restrict__ tpart) {
    constexpr int KC = KB >= 4 ? KB / 4 : 1;      // columns per lane in phase 2
    __shared__ float p_sh[AX_G][KB];
    __shared__ float q_sh[AX_THREADS][KB];
    __shared__ float aa_sh[AX_G * AX_LD];
    __shared__ float bb_sh[AX_G * AX_LD];
    const int lane = threadIdx.x;
    const int s1 = blockIdx.x, s2 = blockIdx.y;
    const int js0 = s1 * gps * AX_G;
    const int js1 = min(nrows, js0 + gps * AX_G);
    const int t0 = s2 * tps, t1 = min(ntiles, t0 + tps);
    const int jj2 = lane >> 2, kq = lane & 3;      // phase 2: row of the group, quarter of the columns
    for (int tile = t0; tile < t1; ++tile) {
        const int i = tile * AX_THREADS + lane;
        float qv[KB], tv[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            qv[kk] = (i < n && kk < k) ? q[(int64_t)i * k + kk] : 0.0f;
            tv[kk] = 0.0f;
        }
        __syncthreads();                              // the previous tile's phase 2 is done with q_sh
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) q_sh[lane][kk] = qv[kk];
        for (int j0 = js0; j0 < js1; j0 += AX_G) {
            __syncthreads();                          // the previous group's phase 2 is done with p_sh, aa_sh, bb_sh
            ax_load_p<KB>(p_sh, p, k, j0, js1);
            __syncthreads();
            float tg[KB];                             // the group's share of t, added to tv once (a two-level sum)
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) tg[kk] = 0.0f;
            for (int jj = 0; jj < AX_G; ++jj) {
                const int j = j0 + jj;
                float aa = 0.0f, bb = 0.0f;
                if (j < js1) {
                    const int64_t rec_idx = rows ? (int64_t)rows[j] : (int64_t)j;
                    const float g = ax_geno(ax_code(p32, m_total, tile, rec_idx, lane), flip ? flip[j] != 0 : false);
                    if (g >= 0.0f) {
                        float rec = 0.0f;
#pragma unroll
                        for (int kk = 0; kk < KB; ++kk) rec += p_sh[jj][kk] * qv[kk];
                        rec = fminf(fmaxf(rec, AX_REC_LO), AX_REC_HI);
                        const float om = 1.0f - rec;
                        const float r = 1.0f / (rec * om);
                        aa = g * om * r;
                        bb = (2.0f - g) * rec * r;
#pragma unroll
                        for (int kk = 0; kk < KB; ++kk) tg[kk] += p_sh[jj][kk] * (aa - bb) + bb;
                    }
                }
                aa_sh[jj * AX_LD + lane] = aa;
                bb_sh[jj * AX_LD + lane] = bb;
            }
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) tv[kk] += tg[kk];
            __syncthreads();
            // phase 2: A[j][c] += sum_i aa[j][i] q[i][c], same for B, over the tile's 128 samples
            const int j = j0 + jj2;
            if (kq * KC < KB && j < js1) {
                float av[KC], bv[KC];
#pragma unroll
                for (int c = 0; c < KC; ++c) av[c] = bv[c] = 0.0f;
                for (int s0 = 0; s0 < AX_THREADS; s0 += 16) {  // two-level sum: 16 samples, then into the lane's total
                    float ac[KC], bc[KC];
#pragma unroll
                    for (int c = 0; c < KC; ++c) ac[c] = bc[c] = 0.0f;
                    for (int s = s0; s < s0 + 16; ++s) {
                        const float a = aa_sh[jj2 * AX_LD + s], b = bb_sh[jj2 * AX_LD + s];
#pragma unroll
                        for (int c = 0; c < KC; ++c) {
                            const float qq = q_sh[s][kq * KC + c];
                            ac[c] += a * qq;
                            bc[c] += b * qq;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < KC; ++c) {
                        av[c] += ac[c];
                        bv[c] += bc[c];
                    }
                }
                const int64_t base = ((int64_t)s2 * nrows + j) * k;
#pragma unroll
                for (int c = 0; c < KC; ++c) {
                    const int kk = kq * KC + c;
                    if (kk < k) {
                        if (tile == t0) {
                            apart[base + kk] = av[c];
                            bpart[base + kk] = bv[c];
                        } else {
                            apart[base + kk] += av[c];
                            bpart[base + kk] += bv[c];
                        }
                    }
                }
            }
        }
        if (i < n) {
#pragma unroll
            for (int kk = 0; kk < KB; ++kk)
                if (kk < k) tpart[((int64_t)s1 * n + i) * k + kk] = tv[kk];
        }
    }
}

// P update per (row, column): A and B added over the sample slices in order, p_em, then either the plain EM output
// (clip(p_em) into p_em_out) or Adam in place on P with clip
__global__ __launch_bounds__(256) void admx_fin_p_kernel(int nrows, int k, int s2, const float *__restrict__ apart,
                                                         const float *__restrict__ bpart, float *__restrict__ p,
                                                         float *__restrict__ p_em_out, float *__restrict__ mp, float *__restrict__ vp,
                                                         float lr, float beta1, float beta2, float eps, float m_scale,
                                                         float v_scale) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)nrows * k) return;
    double sa = 0.0, sb = 0.0;
    for (int s = 0; s < s2; ++s) {
        sa += (double)apart[(int64_t)s * nrows * k + idx];
        sb += (double)bpart[(int64_t)s * nrows * k + idx];
    }
    const float a = (float)sa, b = (float)sb, pv = p[idx];
    const float denom = pv * (a - b) + b;
    const float pem = fabsf(denom) < 1e-8f ? pv : (a * pv) / denom;
    if (mp == nullptr) {
        p_em_out[idx] = ax_clip(pem);
        return;
    }
    const float delta = pem - pv;
    const float mcur = beta1 * mp[idx] + (1.0f - beta1) * delta;
    const float vcur = beta2 * vp[idx] + (1.0f - beta2) * delta * delta;
    const float step = lr * (mcur * m_scale) / (sqrtf(vcur * v_scale) + eps);
    p[idx] = ax_clip(pv + step);
    mp[idx] = mcur;
    vp[idx] = vcur;
}

// Q update per sample: T added over the SNP slices in order, q_em = clip(q t / qb) (clip(q) when qb <= 0), normalised; then
// either the plain EM output (q_em_out) or Adam in place on Q, clip and normalise again.  A non-finite or non-positive row sum
// gives 1/K.
__global__ __launch_bounds__(256) void admx_fin_q_kernel(int n, int k, int s1, const float *__restrict__ tpart,
                                                         const float *__restrict__ qb, float *__restrict__ q, float *__restrict__ qe,
                                                         float *__restrict__ mq, float *__restrict__ vq, float lr, float beta1,
                                                         float beta2, float eps, float m_scale, float v_scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t row = (int64_t)i * k;
    const float qbi = qb[i];
    const float fill = 1.0f / fmaxf((float)k, 1.0f);
    float sum = 0.0f;
    for (int kk = 0; kk < k; ++kk) {
        float v;
        if (qbi <= 0.0f) {
            v = ax_clip(q[row + kk]);
        } else {
            double t = 0.0;
            for (int s = 0; s < s1; ++s) t += (double)tpart[(int64_t)s * n * k + row + kk];
            const float inv = 1.0f / qbi;
            v = ax_clip(q[row + kk] * (float)t * inv);
        }
        qe[row + kk] = v;
        sum += v;
    }
    const bool bad = !(sum > 0.0f) || !isfinite(sum);
    for (int kk = 0; kk < k; ++kk) qe[row + kk] = bad ? fill : qe[row + kk] / sum;
    if (mq == nullptr) return;
    float sum2 = 0.0f;
    for (int kk = 0; kk < k; ++kk) {
        const float qv = q[row + kk];
        const float delta = qe[row + kk] - qv;
        const float mcur = beta1 * mq[row + kk] + (1.0f - beta1) * delta;
        const float vcur = beta2 * vq[row + kk] + (1.0f - beta2) * delta * delta;
        const float step = lr * (mcur * m_scale) / (sqrtf(vcur * v_scale) + eps);
        const float nv = ax_clip(qv + step);
        q[row + kk] = nv;
        mq[row + kk] = mcur;
        vq[row + kk] = vcur;
        sum2 += nv;
    }
    const bool bad2 = !(sum2 > 0.0f) || !isfinite(sum2);
    for (int kk = 0; kk < k; ++kk) q[row + kk] = bad2 ? fill : q[row + kk] / sum2;
}

// log-likelihood partial of workgroup (s1, s2): f64 per lane over its tiles and rows, then a fixed tree over the lanes
template <int KB>
__global__ __launch_bounds__(AX_THREADS) void admx_loglik_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                 const int32_t *__restrict__ rows, int nrows,
                                                                 const uint8_t *__restrict__ flip, int n, int k,
                                                                 const float *__restrict__ p, const float *__restrict__ q, int gps,
                                                                 int tps, int ntiles, double *__restrict__ part) {
    __shared__ float p_sh[AX_G][KB];
    __shared__ double red[AX_THREADS];
    const int lane = threadIdx.x;
    const int s1 = blockIdx.x, s2 = blockIdx.y;
    const int js0 = s1 * gps * AX_G;
    const int js1 = min(nrows, js0 + gps * AX_G);
    const int t0 = s2 * tps, t1 = min(ntiles, t0 + tps);
    double acc = 0.0;
    for (int tile = t0; tile < t1; ++tile) {
        const int i = tile * AX_THREADS + lane;
        float qv[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) qv[kk] = (i < n && kk < k) ? q[(int64_t)i * k + kk] : 0.0f;
        for (int j0 = js0; j0 < js1; j0 += AX_G) {
            __syncthreads();
            ax_load_p<KB>(p_sh, p, k, j0, js1);
            __syncthreads();
            const int jend = min(AX_G, js1 - j0);
            for (int jj = 0; jj < jend; ++jj) {
                const int j = j0 + jj;
                const int64_t rec_idx = rows ? (int64_t)rows[j] : (int64_t)j;
                const float g = ax_geno(ax_code(p32, m_total, tile, rec_idx, lane), flip ? flip[j] != 0 : false);
                if (g < 0.0f) continue;
                float rec = 0.0f;
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) rec += p_sh[jj][kk] * qv[kk];
                const double r = (double)fminf(fmaxf(rec, AX_REC_LO), AX_REC_HI);
                const double gd = (double)g;
                acc += gd * log(r) + (2.0 - gd) * log(1.0 - r);
            }
        }
    }
    red[lane] = acc;
    __syncthreads();
    for (int off = AX_THREADS / 2; off > 0; off >>= 1) {
        if (lane < off) red[lane] += red[lane + off];
        __syncthreads();
    }
    if (lane == 0) part[(int64_t)s2 * gridDim.x + s1] = red[0];
}

__global__ void admx_loglik_sum_kernel(const double *__restrict__ part, int count, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < count; ++c) s += part[c];
    out[0] = s;
}

// called[i] += number of called genotypes of sample i over the rows of slice blockIdx.y (integer atomics: order-free)
__global__ __launch_bounds__(AX_THREADS) void admx_called_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                 const int32_t *__restrict__ rows, int nrows, int n, int rps,
                                                                 int *__restrict__ called) {
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int i = tile * AX_THREADS + lane;
    const int r0 = blockIdx.y * rps, r1 = min(nrows, r0 + rps);
    int c = 0;
    for (int j = r0; j < r1; ++j) {
        const int64_t rec_idx = rows ? (int64_t)rows[j] : (int64_t)j;
        c += ax_code(p32, m_total, tile, rec_idx, lane) != 1u;
    }
    if (i < n && c) atomicAdd(&called[i], c);
}

__global__ __launch_bounds__(256) void admx_qb_kernel(const int *__restrict__ called, int n, float *__restrict__ qb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) qb[i] = 2.0f * (float)called[i];
}

static int ax_check(const char *who, int n, int nrows, int k) {
    if (k < 1 || k > AX_MAX_K) return fail(std::string(who) + ": K must be within [1, 64] (got " + std::to_string(k) + ")");
    if (n < 1 || nrows < 1) return fail(std::string(who) + ": empty panel (n = " + std::to_string(n) + ", rows = " +
                                        std::to_string(nrows) + ")");
    if (k > n) return fail(std::string(who) + ": K = " + std::to_string(k) + " exceeds the number of samples " + std::to_string(n));
    return 0;
}

static int ax_kb(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

#define AX_DISPATCH(KERNEL, GRID, ...)                                                                                   \
    switch (ax_kb(k)) {                                                                                                  \
    case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                          \
    case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                          \
    case 4: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                          \
    case 8: hipLaunchKernelGGL(KERNEL<8>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                          \
    case 16: hipLaunchKernelGGL(KERNEL<16>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                        \
    case 32: hipLaunchKernelGGL(KERNEL<32>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                        \
    default: hipLaunchKernelGGL(KERNEL<64>, GRID, dim3(AX_THREADS), 0, st, __VA_ARGS__); break;                        \
    }

}  // namespace jx

using namespace jx;

extern "C" int64_t jxg_admx_work_bytes(int nrows, int n, int k) {
    if (k < 1 || k > AX_MAX_K || n < 1 || nrows < 1) return 0;
    return ax_work_bytes(ax_grid(nrows, n, k), nrows, n, k);
}

extern "C" int jxg_admx_called(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, void *d_work,
                               int64_t work_bytes, float *d_qb, void *stream) {
    if (n < 1 || nrows < 1) return fail("jxg_admx_called: empty panel");
    if (work_bytes < 4LL * n) return fail("jxg_admx_called: work buffer too small");
    hipStream_t st = (hipStream_t)stream;
    int *called = (int *)d_work;
    JX_HIP(hipMemsetAsync(called, 0, sizeof(int) * (size_t)n, st));
    const int ntiles = num_tiles(n);
    int sl = (2048 + ntiles - 1) / ntiles;
    if (sl > nrows) sl = nrows;
    if (sl > 65535) sl = 65535;
    const int rps = (nrows + sl - 1) / sl;
    sl = (nrows + rps - 1) / rps;
    hipLaunchKernelGGL(admx_called_kernel, dim3(ntiles, sl), dim3(AX_THREADS), 0, st, (const uint32_t *)d_p32, m_total, d_rows, nrows,
                       n, rps, called);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(admx_qb_kernel, dim3((n + 255) / 256), dim3(256), 0, st, called, n, d_qb);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_admx_em_step(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                const uint8_t *d_flip, int k, float *d_p, float *d_q, const float *d_qb, void *d_work,
                                int64_t work_bytes, float *d_p_em, float *d_q_em, float *d_mp, float *d_vp, float *d_mq,
                                float *d_vq, float lr, float beta1, float beta2, float eps, float m_scale, float v_scale,
                                void *stream) {
    if (ax_check("jxg_admx_em_step", n, nrows, k)) return 1;
    const bool adam = d_mp != nullptr;
    if (adam && (!d_vp || !d_mq || !d_vq)) return fail("jxg_admx_em_step: Adam needs all four moment buffers");
    if (!adam && (!d_p_em || !d_q_em)) return fail("jxg_admx_em_step: the EM step needs P_em and Q_em outputs");
    const AxGrid g = ax_grid(nrows, n, k);
    if (work_bytes < ax_work_bytes(g, nrows, n, k)) return fail("jxg_admx_em_step: work buffer too small (jxg_admx_work_bytes)");
    const AxWork w = ax_carve(d_work, g, nrows, n, k);
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = num_tiles(n);
    AX_DISPATCH(admx_em_pass_kernel, dim3(g.s1, g.s2), (const uint32_t *)d_p32, m_total, d_rows, nrows, d_flip, n, k, d_p, d_q,
                g.gps, g.tps, ntiles, w.apart, w.bpart, w.tpart);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(admx_fin_p_kernel, dim3((unsigned)(((int64_t)nrows * k + 255) / 256)), dim3(256), 0, st, nrows, k, g.s2,
                       w.apart, w.bpart, d_p, d_p_em, d_mp, d_vp, lr, beta1, beta2, eps, m_scale, v_scale);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(admx_fin_q_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, k, g.s1, w.tpart, d_qb, d_q,
                       adam ? w.qe : d_q_em, d_mq, d_vq, lr, beta1, beta2, eps, m_scale, v_scale);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_admx_loglik(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                               const uint8_t *d_flip, int k, const float *d_p, const float *d_q, void *d_work, int64_t work_bytes,
                               double *d_out, void *stream) {
    if (ax_check("jxg_admx_loglik", n, nrows, k)) return 1;
    const AxGrid g = ax_grid(nrows, n, k);
    if (work_bytes < ax_work_bytes(g, nrows, n, k)) return fail("jxg_admx_loglik: work buffer too small (jxg_admx_work_bytes)");
    const AxWork w = ax_carve(d_work, g, nrows, n, k);
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = num_tiles(n);
    AX_DISPATCH(admx_loglik_kernel, dim3(g.s1, g.s2), (const uint32_t *)d_p32, m_total, d_rows, nrows, d_flip, n, k, d_p, d_q,
                g.gps, g.tps, ntiles, w.llpart);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(admx_loglik_sum_kernel, dim3(1), dim3(64), 0, st, w.llpart, g.s1 * g.s2, d_out);
    JX_LAUNCH_CHECK();
    return 0;
}
