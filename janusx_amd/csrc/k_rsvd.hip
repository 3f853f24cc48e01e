// Skinny products of the centred additive design with a dense block of columns, for the randomized SVD of `jx pca -rsvd`
// (`rsvd_packed_subset`, src/stats/rsvd.rs:1548-1661; `rsvd_stream_sample_packed_impl`, src/stats/adamixture.rs:3527-3720):
//     W = Z Q    (nrows x kp, markers <- samples)   from the SNP-major P32 image
//     Y = Z' W   (n x kp,     samples <- markers)   from the sample-major T32 image (`jxg_p32_transpose`)
// with Z[r][i] = a_r + b_r g_ri for a called genotype (g = 0 / 1 / 2 for the codes 00 / 10 / 11) and 0 for a missing call (01):
// the GRM method-1 design (`prepare_packed_block_centered_mean_scale_f32`, src/decode/decode.rs:509-532: a = -2 maf, b = 1, or
// a = 2 - 2 maf, b = -1 on a flipped row).
//
// The form is the one of k_pcg_i8.hip, widened from one vector to a block of columns.  Per 2-bit code two 0/1/2 planes
//     G = g (dose: hi + (lo & hi)),   M = [missing] (lo & ~hi)
// are decoded in registers from the lane's own payload dword; the dense block is written once per product as four signed base-254
// digit planes per column against the column's largest magnitude (x = xmax (q1/127 + q2/(127 254) + q3/(127 254^2) +
// q4/(127 254^3)), 2^-31 of xmax).  An A operand of v_mfma_i32_16x16x64_i8 holds four columns x four digits; the B operand is
// one plane of 16 SNPs (samples) x 64 samples (SNPs).  Sums are exact in i32 and merged in f64:
//     W[r][c] = qmax_c (a_r (sum_i q_ic - M.q_c) + b_r G.q_c)
//     Y[i][c] = sum_r a_r W[r][c] + umax_c G.u_c - vmax_c M.v_c,   u = b W, v = a W (two digit images)
// Every lane keeps whole units (16 SNPs / samples) for the whole K range.  Y cuts the SNP tiles into slices whose partial sums
// a small kernel adds in a fixed order, and the column constant is a fixed-order tree sum: no float atomics, and two runs give
// the same bits.  Up to 32 columns are one pass over the payload (8 A tiles); more columns loop over passes of 32.
#include <stdlib.h>

#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

constexpr int RS_WAVES = 8;          // waves per workgroup
constexpr int RS_U = 2;              // units of 16 SNPs (samples) per wave
// |digit x plane value| <= 127 x 2 per K element: an i32 accumulator stays exact over at most 2^23 elements of K (samples of
// Z Q, SNPs of one slice of Z' W; 2^31 / 254 = 8.45 M)
constexpr int RS_MAX_K = 1 << 23;

__device__ __forceinline__ void rs_digits(double x, double inv, int q[4]) {
    double a = x * inv * 127.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double d = rint(a);
        a = (a - d) * 254.0;
        d = fmin(fmax(d, -127.0), 127.0);
        q[k] = (int)d;
    }
}

__device__ __forceinline__ double rs_combine(const i32x4 a) {
    constexpr double W1 = 1.0 / 127.0, R = 1.0 / 254.0;
    return (((double)a.w * R + (double)a.z) * R + (double)a.y) * R * W1 + (double)a.x * W1;
}

__device__ __forceinline__ double rs_combine_ll(const long long *t) {
    return (((double)t[3] / 254.0 + (double)t[2]) / 254.0 + (double)t[1]) / 254.0 / 127.0 + (double)t[0] / 127.0;
}

// x[r][c] * (wsel < 0 ? 1 : ab[r][wsel]) for r < rows, c < kp
__device__ __forceinline__ double rs_val(const double *__restrict__ x, const double *__restrict__ ab, int wsel, int r, int c, int kp) {
    const double v = x[(int64_t)r * kp + c];
    return wsel < 0 ? v : v * ab[(int64_t)r * 2 + wsel];
}

// maxb[vec * kpad + c] = bits of max_r |value|: block (x: rows, grid-strided; y: column c), a wave maximum, then one integer
// atomic per wave (independent of scheduling)
__global__ __launch_bounds__(256) void rs_absmax_kernel(const double *__restrict__ x, const double *__restrict__ ab, int rows, int kp,
                                                        int kpad, int nvec, unsigned long long *__restrict__ maxb) {
    const int c = blockIdx.y;
    unsigned long long b[2] = {0ull, 0ull};
    for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256)
        for (int v = 0; v < nvec; ++v) {
            const double a = fabs(rs_val(x, ab, nvec == 1 ? -1 : 1 - v, r, c, kp));    // two vectors: u = b x, v = a x
            const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
            b[v] = bits > b[v] ? bits : b[v];
        }
    for (int v = 0; v < nvec; ++v) {
        unsigned long long m = b[v];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off, 64);
            m = o > m ? o : m;
        }
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&maxb[v * kpad + c], m);
    }
}

// digit image of one pass: img[cb][tile][slot][R = nvec 16 NT rows][16 B]; row vec 16 NT + 16 (j / 4) + 4 (j % 4) + digit for the
// pass's column j.  Thread = (cb, tile, slot, vec, j).  tot[c][4] (nvec == 1): sums of the digit planes (exact integers).
__global__ __launch_bounds__(256) void rs_quant_kernel(const double *__restrict__ x, const double *__restrict__ ab, int rows, int kp,
                                                       int kpad, int nvec, int nt, int ntiles, const unsigned long long *__restrict__ maxb,
                                                       long long *__restrict__ tot, int8_t *__restrict__ img) {
    const int cpp = 4 * nt;                                   // columns per pass
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)(kpad / cpp) * ntiles * 8 * nvec * cpp;
    if (idx >= total) return;
    int64_t t = idx;
    const int j = (int)(t % cpp); t /= cpp;
    const int vec = (int)(t % nvec); t /= nvec;
    const int slot = (int)(t % 8); t /= 8;
    const int tile = (int)(t % ntiles); t /= ntiles;
    const int cb = (int)t;
    const int c = cb * cpp + j, h = slot >> 2, kq = slot & 3;
    const double xmax = __longlong_as_double((long long)maxb[vec * kpad + c]);
    const double inv = (xmax > 0.0 && xmax < 1.0e300) ? 1.0 / xmax : 0.0;
    const int wsel = nvec == 1 ? -1 : 1 - vec;
    int8_t o[4][16];
    long long s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int pos = 0; pos < 16; ++pos) {
        const int e = ((pos & 3) << 2) | (pos >> 2);          // byte 4 q + b holds element 4 b + q
        const int r = tile * 128 + 16 * (2 * kq + h) + e;
        int q[4] = {0, 0, 0, 0};
        if (r < rows && c < kp) rs_digits(rs_val(x, ab, wsel, r, c, kp), inv, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k][pos] = (int8_t)q[k];
            s[k] += q[k];
        }
    }
    const int R = 16 * nt * nvec;
    const int64_t base = ((((int64_t)cb * ntiles + tile) * 8 + slot) * R + vec * 16 * nt + 16 * (j >> 2) + 4 * (j & 3)) * 16;
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<uint4 *>(img + base + k * 16) = *reinterpret_cast<const uint4 *>(o[k]);
    if (nvec == 1 && c < kp) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s[k]) atomicAdd((unsigned long long *)&tot[(int64_t)c * 4 + k], (unsigned long long)s[k]);
    }
}

// Main loop of both products.  Unit u of the wave covers outputs o0 + 16 u + s; K runs over the record tiles [t_lo, t_hi) of
// `src` (record of output o in tile t at src + (t tstride + o) 32 -- P32 with the row list, or T32).  NV digit vectors:
// A tiles 0..NT-1 of vector 0 meet the dose plane, tiles of vector NV-1 the missing plane.
template <int NT, int NV>
__device__ __forceinline__ void rs_main(const uint8_t *__restrict__ src, int64_t tstride, const int32_t *__restrict__ rows, int nout,
                                        int t_lo, int t_hi, const int8_t *__restrict__ img, int8_t *a_sh, int o0,
                                        i32x4 (&acc_g)[RS_U][NT], i32x4 (&acc_m)[RS_U][NT]) {
    constexpr int R = 16 * NT * NV;                          // A rows of one slot
    constexpr int TB = 8 * R * 16;                           // image bytes per record tile
    constexpr int ST = (256 / R) > 8 ? 8 : ((256 / R) < 1 ? 1 : 256 / R);   // tiles per LDS stage (32 KB at most)
    constexpr int SB = ST * TB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int s = lane & 15, kq = lane >> 4;
    const uint8_t *gsrc[RS_U];
#pragma unroll
    for (int u = 0; u < RS_U; ++u) {
        const int o = o0 + 16 * u + s;
        const int64_t rec = (o < nout) ? (rows ? (int64_t)rows[o] : (int64_t)o) : 0;
        gsrc[u] = src + rec * 32 + 8 * kq;
    }
#pragma unroll
    for (int u = 0; u < RS_U; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc_g[u][t] = acc_m[u][t] = i32x4{0, 0, 0, 0};
    const int ntl = t_hi - t_lo;
    if (ntl <= 0) return;
    const int nstage = (ntl + ST - 1) / ST;
    const int64_t img_end = (int64_t)t_hi * TB;
    auto stage_load = [&](int sg, int buf) {
        const int64_t base = ((int64_t)t_lo + (int64_t)sg * ST) * TB;
#pragma unroll
        for (int q = 0; q < SB / (RS_WAVES * 64 * 16); ++q) {
            const int off = (q * RS_WAVES * 64 + tid) * 16;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (base + off < img_end) v = *reinterpret_cast<const uint4 *>(img + base + off);
            *reinterpret_cast<uint4 *>(a_sh + buf * SB + off) = v;
        }
    };
    stage_load(0, 0);
    for (int sg = 0; sg < nstage; ++sg) {
        const int buf = sg & 1;
        __syncthreads();                                     // stage sg is in LDS, nobody reads the other buffer any more
        if (sg + 1 < nstage) stage_load(sg + 1, buf ^ 1);
        const int t0 = t_lo + sg * ST;
        uint2 g[ST][RS_U];
#pragma unroll
        for (int j = 0; j < ST; ++j) {
            const int t = (t0 + j < t_hi) ? t0 + j : t_hi - 1;   // past the end: a record whose digits are zero
#pragma unroll
            for (int u = 0; u < RS_U; ++u) g[j][u] = *reinterpret_cast<const uint2 *>(gsrc[u] + (int64_t)t * tstride);
        }
        const int8_t *ab = a_sh + buf * SB;
#pragma unroll
        for (int j = 0; j < ST; ++j) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                i32x4 dose[RS_U], miss[RS_U];
#pragma unroll
                for (int u = 0; u < RS_U; ++u) counts_missing16(h ? g[j][u].y : g[j][u].x, dose[u], miss[u]);
                const int8_t *arow = ab + (int64_t)j * TB + ((h * 4 + kq) * R + s) * 16;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const i32x4 a_g = *reinterpret_cast<const i32x4 *>(arow + t * 256);
                    const i32x4 a_m = *reinterpret_cast<const i32x4 *>(arow + ((NV - 1) * NT + t) * 256);
#pragma unroll
                    for (int u = 0; u < RS_U; ++u) {
                        acc_g[u][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_g, dose[u], acc_g[u][t], 0, 0, 0);
                        acc_m[u][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_m, miss[u], acc_m[u][t], 0, 0, 0);
                    }
                }
            }
        }
    }
}

template <int NT>
constexpr int rs_lds_bytes(int nv) {
    return 2 * ((256 / (16 * NT * nv)) > 8 ? 8 : ((256 / (16 * NT * nv)) < 1 ? 1 : 256 / (16 * NT * nv))) * 8 * 16 * NT * nv * 16;
}

// W = Z Q: block (x: 16 RS_U RS_WAVES rows of the list, y: column pass)
template <int NT>
__global__ __launch_bounds__(RS_WAVES * 64) void rs_mm_kernel(const uint8_t *__restrict__ p32, int64_t m_total, const int32_t *__restrict__ rows,
                                                              int nrows, int ntiles, int kp, int kpad, const int8_t *__restrict__ img,
                                                              const unsigned long long *__restrict__ maxb, const long long *__restrict__ tot,
                                                              const double *__restrict__ ab, double *__restrict__ w) {
    __shared__ __attribute__((aligned(16))) int8_t a_sh[rs_lds_bytes<NT>(1)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int o0 = (blockIdx.x * RS_WAVES + wave) * 16 * RS_U;
    const int cb = blockIdx.y;
    i32x4 acc_g[RS_U][NT], acc_m[RS_U][NT];
    rs_main<NT, 1>(p32, m_total * 32, rows, nrows, 0, ntiles, img + (int64_t)cb * ntiles * (8 * 16 * NT * 16), a_sh, o0, acc_g, acc_m);
    // D rows 4 kq + digit of column s: lane (s, kq) holds the four digit sums of column 4 t + kq of the pass for output o0 + 16 u + s
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = cb * 4 * NT + 4 * t + kq;
        if (c >= kp) continue;
        const double qmax = __longlong_as_double((long long)maxb[c]);
        const double qtot = rs_combine_ll(tot + (int64_t)c * 4);
#pragma unroll
        for (int u = 0; u < RS_U; ++u) {
            const int r = o0 + 16 * u + s;
            if (r < nrows) {
                const double gs = rs_combine(acc_g[u][t]), ms = rs_combine(acc_m[u][t]);
                w[(int64_t)r * kp + c] = qmax * (ab[(int64_t)r * 2] * (qtot - ms) + ab[(int64_t)r * 2 + 1] * gs);
            }
        }
    }
}

// Y partials: block (x: 16 RS_U RS_WAVES samples, y: SNP-tile slice, z: column pass); part[slice][i][c]
template <int NT>
__global__ __launch_bounds__(RS_WAVES * 64) void rs_tmm_kernel(const uint8_t *__restrict__ t32, int n, int nst, int tiles_per_slice,
                                                               int kp, int kpad, const int8_t *__restrict__ img,
                                                               const unsigned long long *__restrict__ maxb, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) int8_t a_sh[rs_lds_bytes<NT>(2)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int o0 = (blockIdx.x * RS_WAVES + wave) * 16 * RS_U;
    const int cb = blockIdx.z;
    const int st0 = blockIdx.y * tiles_per_slice;
    const int st1 = (st0 + tiles_per_slice < nst) ? st0 + tiles_per_slice : nst;
    i32x4 acc_g[RS_U][NT], acc_m[RS_U][NT];
    rs_main<NT, 2>(t32, (int64_t)n * 32, nullptr, n, st0, st1, img + (int64_t)cb * nst * (8 * 32 * NT * 16), a_sh, o0, acc_g, acc_m);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = cb * 4 * NT + 4 * t + kq;
        if (c >= kp) continue;
        const double umax = __longlong_as_double((long long)maxb[c]), vmax = __longlong_as_double((long long)maxb[kpad + c]);
#pragma unroll
        for (int u = 0; u < RS_U; ++u) {
            const int i = o0 + 16 * u + s;
            if (i < n) part[((int64_t)blockIdx.y * n + i) * kp + c] = umax * rs_combine(acc_g[u][t]) - vmax * rs_combine(acc_m[u][t]);
        }
    }
}

// cst[c] = sum_r a_r W[r][c]: one block per column, strided partial sums and a fixed tree
__global__ __launch_bounds__(256) void rs_colconst_kernel(const double *__restrict__ w, const double *__restrict__ ab, int nrows, int kp,
                                                          double *__restrict__ cst) {
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double v = 0.0;
    for (int r = threadIdx.x; r < nrows; r += 256) v += ab[(int64_t)r * 2] * w[(int64_t)r * kp + c];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) cst[c] = sh[0];
}

__global__ __launch_bounds__(256) void rs_tmm_reduce_kernel(const double *__restrict__ part, int n, int kp, int slices,
                                                            const double *__restrict__ cst, double *__restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * kp) return;
    const int c = (int)(idx % kp);
    double v = cst[c];
    for (int q = 0; q < slices; ++q) v += part[(int64_t)q * n * kp + idx];
    y[idx] = v;
}

// columns per pass: the smallest of 4, 8, 16, 32 that holds kp (32 above that, in several passes)
static int rs_nt(int kp) { return kp <= 4 ? 1 : (kp <= 8 ? 2 : (kp <= 16 ? 4 : 8)); }

static unsigned rs_blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

static dim3 rs_absmax_grid(int rows, int kp) { return dim3(rs_blocks(rows) < 256 ? rs_blocks(rows) : 256, kp); }

}  // namespace jx

using namespace jx;

extern "C" int jxg_packed_mm_cols(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const double *d_ab,
                                  const double *d_q, int kp, double *d_w, void *stream) {
    if (kp < 1) return fail("jxg_packed_mm_cols: kp must be >= 1");
    if (n > RS_MAX_K) return fail("jxg_packed_mm_cols: at most 8 388 608 samples (exact i32 plane sums)");
    if (nrows <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) {
        JX_HIP(hipMemsetAsync(d_w, 0, sizeof(double) * (size_t)nrows * kp, st));
        return 0;
    }
    const int nt = rs_nt(kp), cpp = 4 * nt, ncb = (kp + cpp - 1) / cpp, kpad = ncb * cpp;
    const int ntiles = (n + 127) / 128;
    const size_t b_sc = 8 * (size_t)kpad + 32 * (size_t)kpad, b_img = (size_t)ncb * ntiles * 8 * 16 * nt * 16;
    AsyncBlock ab;
    if (ab.alloc(b_sc + b_img, st)) return 1;
    char *blk = (char *)ab.p;
    unsigned long long *maxb = (unsigned long long *)blk;
    long long *tot = (long long *)(blk + 8 * (size_t)kpad);
    int8_t *img = (int8_t *)(blk + b_sc);
    JX_HIP(hipMemsetAsync(blk, 0, b_sc, st));
    hipLaunchKernelGGL(rs_absmax_kernel, rs_absmax_grid(n, kp), dim3(256), 0, st, d_q, nullptr, n, kp, kpad, 1, maxb);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_quant_kernel, dim3(rs_blocks((int64_t)kpad * ntiles * 8)), dim3(256), 0, st, d_q, nullptr, n, kp, kpad, 1, nt,
                       ntiles, maxb, tot, img);
    JX_LAUNCH_CHECK();
    const dim3 grid((nrows + RS_WAVES * 16 * RS_U - 1) / (RS_WAVES * 16 * RS_U), ncb), block(RS_WAVES * 64);
    switch (nt) {
    case 1: hipLaunchKernelGGL(rs_mm_kernel<1>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, ntiles, kp, kpad, img, maxb, tot, d_ab, d_w); break;
    case 2: hipLaunchKernelGGL(rs_mm_kernel<2>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, ntiles, kp, kpad, img, maxb, tot, d_ab, d_w); break;
    case 4: hipLaunchKernelGGL(rs_mm_kernel<4>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, ntiles, kp, kpad, img, maxb, tot, d_ab, d_w); break;
    default: hipLaunchKernelGGL(rs_mm_kernel<8>, grid, block, 0, st, d_p32, m_total, d_rows, nrows, ntiles, kp, kpad, img, maxb, tot, d_ab, d_w); break;
    }
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_packed_tmm_cols(const uint8_t *d_t32, int n, int nrows, const double *d_ab, const double *d_w, int kp, double *d_y,
                                   void *stream) {
    if (kp < 1) return fail("jxg_packed_tmm_cols: kp must be >= 1");
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (nrows <= 0) {
        JX_HIP(hipMemsetAsync(d_y, 0, sizeof(double) * (size_t)n * kp, st));
        return 0;
    }
    const int nt = rs_nt(kp), cpp = 4 * nt, ncb = (kp + cpp - 1) / cpp, kpad = ncb * cpp;
    const int nst = (nrows + 127) / 128;
    const int gx = (n + RS_WAVES * 16 * RS_U - 1) / (RS_WAVES * 16 * RS_U);
    int slices = (1024 + gx * ncb - 1) / (gx * ncb);          // ~1024 workgroups
    if (slices > 64) slices = 64;
    if (slices > nst) slices = nst;
    if (slices < 1) slices = 1;
    int tps = (nst + slices - 1) / slices;
    if (tps > RS_MAX_K / 128) tps = RS_MAX_K / 128;            // a slice's i32 plane sums stay exact
    slices = (nst + tps - 1) / tps;
    const size_t b_sc = 16 * (size_t)kpad + 8 * (size_t)kpad, b_img = (size_t)ncb * nst * 8 * 32 * nt * 16;
    const size_t b_part = sizeof(double) * (size_t)slices * (size_t)n * (size_t)kp;
    AsyncBlock ab;
    if (ab.alloc(b_sc + b_img + b_part, st)) return 1;
    char *blk = (char *)ab.p;
    unsigned long long *maxb = (unsigned long long *)blk;
    double *cst = (double *)(blk + 16 * (size_t)kpad);
    int8_t *img = (int8_t *)(blk + b_sc);
    double *part = (double *)(blk + b_sc + b_img);
    JX_HIP(hipMemsetAsync(blk, 0, b_sc, st));
    hipLaunchKernelGGL(rs_absmax_kernel, rs_absmax_grid(nrows, kp), dim3(256), 0, st, d_w, d_ab, nrows, kp, kpad, 2, maxb);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_quant_kernel, dim3(rs_blocks((int64_t)kpad * nst * 16)), dim3(256), 0, st, d_w, d_ab, nrows, kp, kpad, 2, nt,
                       nst, maxb, nullptr, img);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_colconst_kernel, dim3(kp), dim3(256), 0, st, d_w, d_ab, nrows, kp, cst);
    JX_LAUNCH_CHECK();
    const dim3 grid(gx, slices, ncb), block(RS_WAVES * 64);
    switch (nt) {
    case 1: hipLaunchKernelGGL(rs_tmm_kernel<1>, grid, block, 0, st, d_t32, n, nst, tps, kp, kpad, img, maxb, part); break;
    case 2: hipLaunchKernelGGL(rs_tmm_kernel<2>, grid, block, 0, st, d_t32, n, nst, tps, kp, kpad, img, maxb, part); break;
    case 4: hipLaunchKernelGGL(rs_tmm_kernel<4>, grid, block, 0, st, d_t32, n, nst, tps, kp, kpad, img, maxb, part); break;
    default: hipLaunchKernelGGL(rs_tmm_kernel<8>, grid, block, 0, st, d_t32, n, nst, tps, kp, kpad, img, maxb, part); break;
    }
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_tmm_reduce_kernel, dim3(rs_blocks((int64_t)n * kp)), dim3(256), 0, st, part, n, kp, slices, cst, d_y);
    JX_LAUNCH_CHECK();
    return 0;
}
