// Dense f64 Cholesky, triangular solves and the small reductions of multi-kernel AI-REML (src/stats/reml.rs:703-1049: every
// likelihood evaluation there is `v.cholesky()` of V = sum_j theta_j K_j + theta_e I followed by `chol_v.solve(..)`; with q > 1
// kernels there is no shared eigenbasis, so the O(n^3) factor is the whole cost).  Column-major, lower triangle only.
//   potrf   right-looking, two block levels: 64-column diagonal blocks are factored AND inverted by one workgroup in LDS
//           (potrf_diag_kernel), the panel below is the product A21 inv(L11)' (jx::dgemm), the update stays inside the 512-column
//           outer block (dsyr2k_lower_nt on its square part, dgemm below it) and the trailing matrix sees one rank-512 update per
//           outer block.  An estimate, not a measurement: a rank-64 update of the whole trailing matrix per panel reads and writes
//           its lower triangle, n^3 / 24 bytes in all (333 GB at n = 20 000: about twice the time n^3 / 3 flops take at the f64
//           matrix peak); one update per 512 columns moves n^3 / 192.
//   potrs   blocked forward and back substitution: the inverses of all diagonal blocks in one launch (trtri_diag_kernel), then per
//           block one 64 x nrhs product with the inverse and one dgemm for the rest.
//   reml_combine / sym_dot / potrf_logdet: memory-bound one-pass kernels; sums in a fixed order (no floating-point atomics).
// A pivot that is not positive and finite never reaches a square root or a division: the block is left as it was, the 1-based pivot
// index goes to a device word, every later diagonal block of the call sees the word and leaves its block alone as well (its
// "inverse" is the identity, so the products behind it stay defined), and the host stops at the next outer block.
#include <math.h>

#include "jx_common.h"

namespace jx {
int dgemm(hipStream_t st, bool ta, bool tb, int m, int n, int k, double alpha, const double *a, int64_t lda, const double *b,
          int64_t ldb, double beta, double *c, int64_t ldc, int ksplit, double *ws, size_t ws_doubles);
int dsyr2k_lower_nt(hipStream_t st, int m, int k, double alpha, const double *a, int64_t lda, const double *b, int64_t ldb,
                    double beta, double *c, int64_t ldc);
}  // namespace jx

using namespace jx;

namespace {

constexpr int PF_NB = 64;            // diagonal block (jxg_potrf_block())
constexpr int PF_P = PF_NB + 1;      // LDS pitch in doubles: a column of 64 rows covers the 64 banks twice, conflict-free both ways
constexpr int PF_OB = 512;           // outer block: one trailing update per 512 columns
constexpr int PF_T = 256;
constexpr size_t PF_SMEM = sizeof(double) * 2 * PF_NB * PF_P;
constexpr int PF_MAX_Q = 16;

// s[r + c PF_P] = the jb x jb lower block at `a`, padded to 64 x 64 with the identity (the padding factors and inverts to itself)
__device__ __forceinline__ void pf_load(const double *__restrict__ a, int64_t lda, int jb, double *__restrict__ s) {
    for (int idx = threadIdx.x; idx < PF_NB * PF_NB; idx += PF_T) {
        const int r = idx % PF_NB, c = idx / PF_NB;
        double v = (r == c) ? 1.0 : 0.0;
        if (r < jb && c < jb && r >= c) v = a[r + (int64_t)c * lda];
        s[r + c * PF_P] = v;
    }
}

// unblocked right-looking Cholesky of s in place; returns 0, or the 1-based index of the first pivot that is not positive and
// finite (the same value in every thread: all of them read the one LDS word), with nothing derived from that pivot
__device__ __forceinline__ int pf_factor(double *__restrict__ s) {
    const int t = threadIdx.x;
    for (int k = 0; k < PF_NB; ++k) {
        __syncthreads();
        const double d = s[k + k * PF_P];
        if (!(d > 0.0) || !(d < INFINITY)) return k + 1;
        const double rd = sqrt(d);
        __syncthreads();
        if (t >= k && t < PF_NB) s[t + k * PF_P] = (t == k) ? rd : s[t + k * PF_P] / rd;
        __syncthreads();
        const int cnt = (PF_NB - 1 - k) * PF_NB;
        for (int idx = t; idx < cnt; idx += PF_T) {
            const int r = idx % PF_NB, c = k + 1 + idx / PF_NB;
            if (r >= c) s[r + c * PF_P] -= s[r + k * PF_P] * s[c + k * PF_P];
        }
    }
    __syncthreads();
    return 0;
}

// w = inverse of the lower triangle in s (forward substitution on the identity, row by row)
__device__ __forceinline__ void pf_invert(const double *__restrict__ s, double *__restrict__ w) {
    const int t = threadIdx.x;
    for (int idx = t; idx < PF_NB * PF_NB; idx += PF_T) {
        const int r = idx % PF_NB, c = idx / PF_NB;
        w[r + c * PF_P] = (r == c) ? 1.0 : 0.0;
    }
    for (int r = 0; r < PF_NB; ++r) {
        __syncthreads();
        const double lrr = s[r + r * PF_P];
        if (t <= r) w[r + t * PF_P] = w[r + t * PF_P] / lrr;
        __syncthreads();
        const int cnt = (r + 1) * PF_NB;           // columns 0 .. r of the rows below r
        for (int idx = t; idx < cnt; idx += PF_T) {
            const int r2 = idx % PF_NB, c = idx / PF_NB;
            if (r2 > r) w[r2 + c * PF_P] -= s[r2 + r * PF_P] * w[r + c * PF_P];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void pf_write_inverse(const double *__restrict__ w, double *__restrict__ dinv, bool identity) {
    for (int idx = threadIdx.x; idx < PF_NB * PF_NB; idx += PF_T) {
        const int r = idx % PF_NB, c = idx / PF_NB;
        dinv[idx] = identity ? ((r == c) ? 1.0 : 0.0) : w[r + c * PF_P];
    }
}

// `a`: the diagonal block (row and column j0 of the matrix), jb <= 64 of its columns inside the matrix
__global__ __launch_bounds__(PF_T) void potrf_diag_kernel(double *__restrict__ a, int64_t lda, int j0, int jb, double *__restrict__ dinv,
                                                          int *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double pf_smem[];
    double *s = pf_smem, *w = pf_smem + PF_NB * PF_P;
    int bad = *(volatile int *)info;               // an earlier block of this call failed
    if (bad == 0) {
        pf_load(a, lda, jb, s);
        bad = pf_factor(s);
        if (bad != 0 && threadIdx.x == 0) *info = j0 + bad;
    }
    if (bad != 0) {
        pf_write_inverse(w, dinv, true);
        return;
    }
    for (int idx = threadIdx.x; idx < PF_NB * PF_NB; idx += PF_T) {
        const int r = idx % PF_NB, c = idx / PF_NB;
        if (r < jb && c < jb && r >= c) a[r + (int64_t)c * lda] = s[r + c * PF_P];
    }
    pf_invert(s, w);
    pf_write_inverse(w, dinv, false);
}

// inverses of all diagonal blocks of a factor: block b -> dinv + 4096 b
__global__ __launch_bounds__(PF_T) void trtri_diag_kernel(const double *__restrict__ l, int64_t ldl, int n, double *__restrict__ dinv) {
    extern __shared__ __attribute__((aligned(16))) double pf_smem[];
    double *s = pf_smem, *w = pf_smem + PF_NB * PF_P;
    const int j0 = (int)blockIdx.x * PF_NB, jb = min(PF_NB, n - j0);
    pf_load(l + j0 + (int64_t)j0 * ldl, ldl, jb, s);
    __syncthreads();
    pf_invert(s, w);
    pf_write_inverse(w, dinv + (int64_t)blockIdx.x * PF_NB * PF_NB, false);
}

// sum of 256 values in a fixed tree order; the result in thread 0
__device__ __forceinline__ double pf_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = PF_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

struct CombineTheta {
    double v[PF_MAX_Q + 1];
};

// V = theta_q I + sum_j theta_j K_j in the order of reml.rs:834-837; only the entries i >= j are written
__global__ __launch_bounds__(PF_T) void reml_combine_kernel(const double *__restrict__ k, int q, int n, CombineTheta th,
                                                            double *__restrict__ v) {
    const int j = blockIdx.y, i0 = (int)blockIdx.x * PF_T, i = i0 + (int)threadIdx.x;
    if (i < j || i >= n) return;
    const int64_t off = (int64_t)i + (int64_t)j * n, nn = (int64_t)n * n;
    double acc = (i == j) ? th.v[q] : 0.0;
    for (int t = 0; t < q; ++t) acc += k[(int64_t)t * nn + off] * th.v[t];
    v[off] = acc;
}

// column j: sum_i a_ij b_ij over the full symmetric column pair, read from the lower triangles (off-diagonal entries count twice)
__global__ __launch_bounds__(PF_T) void sym_dot_cols_kernel(const double *__restrict__ a, int64_t lda, const double *__restrict__ b,
                                                            int64_t ldb, int n, double *__restrict__ part) {
    __shared__ double red[PF_T];
    const int j = blockIdx.x;
    double acc = 0.0;
    for (int i = j + (int)threadIdx.x; i < n; i += PF_T) {
        const double p = a[i + (int64_t)j * lda] * b[i + (int64_t)j * ldb];
        acc += (i == j) ? p : 2.0 * p;
    }
    const double s = pf_block_sum(acc, red);
    if (threadIdx.x == 0) part[j] = s;
}

__global__ __launch_bounds__(PF_T) void sum_fixed_kernel(const double *__restrict__ part, int n, double *__restrict__ out) {
    __shared__ double red[PF_T];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += PF_T) acc += part[i];
    const double s = pf_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(PF_T) void logdet_kernel(const double *__restrict__ l, int64_t ldl, int n, double *__restrict__ out) {
    __shared__ double red[PF_T];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += PF_T) acc += log(l[i + (int64_t)i * ldl]);
    const double s = pf_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = 2.0 * s;
}

// device workspace of the calls below, grown on demand and kept.  It and the attribute flag of pf_smem_attr are per PROCESS, not per
// device or thread: these entries serve one GPU and one call at a time (`jx reml` is a one-GPU command; under a launcher rank 0 alone
// works).  A second device in one process would need the attribute set and a workspace of its own.
struct PfWork {
    DevBuf panel, dinv, small;
    int grow(DevBuf &b, size_t bytes) { return b.bytes >= bytes ? 0 : b.alloc(bytes); }
};
PfWork &pf_work() {
    static PfWork w;
    return w;
}

int pf_smem_attr() {
    static bool set = false;
    if (!set) {
        JX_HIP(hipFuncSetAttribute((const void *)potrf_diag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PF_SMEM));
        JX_HIP(hipFuncSetAttribute((const void *)trtri_diag_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PF_SMEM));
        set = true;
    }
    return 0;
}

}  // namespace

extern "C" int jxg_potrf_block(void) { return PF_NB; }

extern "C" int jxg_dpotrf_lower_f64(double *d_a, int n, int64_t lda, int *h_info, void *stream) {
    if (!h_info) return fail("jxg_dpotrf_lower_f64: h_info is NULL");
    h_info[0] = 0;
    if (n < 0 || (n > 0 && (!d_a || lda < n))) return fail("jxg_dpotrf_lower_f64: need n >= 0, lda >= n and a device matrix");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PfWork &w = pf_work();
    const int64_t ldt = n + (n & 1);                  // even: the panel copy stays eligible for dgemm's 16-byte loads
    if (w.grow(w.panel, sizeof(double) * (size_t)ldt * PF_NB) || w.grow(w.dinv, sizeof(double) * PF_NB * PF_NB) ||
        w.grow(w.small, 256) || pf_smem_attr())
        return 1;
    double *tmp = w.panel.as<double>(), *dinv = w.dinv.as<double>();
    int *d_info = w.small.as<int>();
    JX_HIP(hipMemsetAsync(d_info, 0, sizeof(int), st));
    auto at = [&](int r, int c) { return d_a + r + (int64_t)c * lda; };
    for (int o0 = 0; o0 < n; o0 += PF_OB) {
        const int oend = min(n, o0 + PF_OB);
        for (int j0 = o0; j0 < oend; j0 += PF_NB) {
            const int jb = min(PF_NB, oend - j0), j1 = j0 + jb, m2 = n - j1;
            hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(PF_T), PF_SMEM, st, at(j0, j0), lda, j0, jb, dinv, d_info);
            JX_LAUNCH_CHECK();
            if (m2 == 0) continue;
            // panel: L21 = A21 inv(L11)'
            JX_HIP(hipMemcpy2DAsync(tmp, sizeof(double) * ldt, at(j1, j0), sizeof(double) * lda, sizeof(double) * m2, jb,
                                    hipMemcpyDeviceToDevice, st));
            if (dgemm(st, false, true, m2, jb, jb, 1.0, tmp, ldt, dinv, PF_NB, 0.0, at(j1, j0), lda, 1, nullptr, 0)) return 1;
            // the rest of the outer block: its square part by lower tiles, the rows below it as a plain product
            const int wc = oend - j1, mr = n - oend;
            if (wc > 0) {
                if (dsyr2k_lower_nt(st, wc, jb, -1.0, at(j1, j0), lda, at(j1, j0), lda, 1.0, at(j1, j1), lda)) return 1;
                if (mr > 0 &&
                    dgemm(st, false, true, mr, wc, jb, -1.0, at(oend, j0), lda, at(j1, j0), lda, 1.0, at(oend, j1), lda, 1, nullptr, 0))
                    return 1;
            }
        }
        if (n - oend > 0 &&
            dsyr2k_lower_nt(st, n - oend, oend - o0, -1.0, at(oend, o0), lda, at(oend, o0), lda, 1.0, at(oend, oend), lda))
            return 1;
        JX_HIP(hipMemcpyAsync(h_info, d_info, sizeof(int), hipMemcpyDeviceToHost, st));
        JX_HIP(hipStreamSynchronize(st));
        if (h_info[0] != 0) break;
    }
    return 0;
}

extern "C" int jxg_dpotrs_lower_f64(const double *d_l, int n, int64_t ldl, double *d_b, int nrhs, int64_t ldb, void *stream) {
    if (n < 0 || nrhs < 0 || (n > 0 && nrhs > 0 && (!d_l || !d_b || ldl < n || ldb < n)))
        return fail("jxg_dpotrs_lower_f64: need n, nrhs >= 0, ldl >= n, ldb >= n and device matrices");
    if (n == 0 || nrhs == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PfWork &w = pf_work();
    const int nblk = ceil_div(n, PF_NB);
    if (w.grow(w.panel, sizeof(double) * (size_t)PF_NB * nrhs) || w.grow(w.dinv, sizeof(double) * PF_NB * PF_NB * (size_t)nblk) ||
        pf_smem_attr())
        return 1;
    double *tmp = w.panel.as<double>(), *dinv = w.dinv.as<double>();
    hipLaunchKernelGGL(trtri_diag_kernel, dim3(nblk), dim3(PF_T), PF_SMEM, st, d_l, ldl, n, dinv);
    JX_LAUNCH_CHECK();
    auto put = [&](int j0, int jb) -> int {
        JX_HIP(hipMemcpy2DAsync(d_b + j0, sizeof(double) * ldb, tmp, sizeof(double) * PF_NB, sizeof(double) * jb, nrhs,
                                hipMemcpyDeviceToDevice, st));
        return 0;
    };
    // L Y = B
    for (int b = 0; b < nblk; ++b) {
        const int j0 = b * PF_NB, jb = min(PF_NB, n - j0), j1 = j0 + jb;
        const double *inv = dinv + (int64_t)b * PF_NB * PF_NB;
        if (dgemm(st, false, false, jb, nrhs, jb, 1.0, inv, PF_NB, d_b + j0, ldb, 0.0, tmp, PF_NB, 1, nullptr, 0) || put(j0, jb)) return 1;
        if (n - j1 > 0 &&
            dgemm(st, false, false, n - j1, nrhs, jb, -1.0, d_l + j1 + (int64_t)j0 * ldl, ldl, tmp, PF_NB, 1.0, d_b + j1, ldb, 1, nullptr, 0))
            return 1;
    }
    // L' X = Y
    for (int b = nblk - 1; b >= 0; --b) {
        const int j0 = b * PF_NB, jb = min(PF_NB, n - j0);
        const double *inv = dinv + (int64_t)b * PF_NB * PF_NB;
        if (dgemm(st, true, false, jb, nrhs, jb, 1.0, inv, PF_NB, d_b + j0, ldb, 0.0, tmp, PF_NB, 1, nullptr, 0) || put(j0, jb)) return 1;
        if (j0 > 0 && dgemm(st, true, false, j0, nrhs, jb, -1.0, d_l + j0, ldl, tmp, PF_NB, 1.0, d_b, ldb, 1, nullptr, 0)) return 1;
    }
    return 0;
}

extern "C" int jxg_reml_combine_f64(const double *d_kstack, int q, int n, const double *h_theta, double *d_v, void *stream) {
    if (q < 1 || q > PF_MAX_Q) return fail("jxg_reml_combine_f64: 1 <= q <= 16 kernels");
    if (n < 1 || n > 65535 || !d_kstack || !h_theta || !d_v) return fail("jxg_reml_combine_f64: need 1 <= n <= 65535 and non-NULL arguments");
    CombineTheta th;
    for (int j = 0; j <= q; ++j) th.v[j] = h_theta[j];
    hipLaunchKernelGGL(reml_combine_kernel, dim3(ceil_div(n, PF_T), n), dim3(PF_T), 0, (hipStream_t)stream, d_kstack, q, n, th, d_v);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_sym_dot_f64(const double *d_a, const double *d_b, int n, int64_t lda, int64_t ldb, double *d_out, void *stream) {
    if (n < 1 || !d_a || !d_b || !d_out || lda < n || ldb < n) return fail("jxg_sym_dot_f64: need n >= 1, lda, ldb >= n and non-NULL arguments");
    PfWork &w = pf_work();
    if (w.grow(w.small, sizeof(double) * ((size_t)n + 32))) return 1;
    double *part = w.small.as<double>() + 32;         // the first 256 bytes: the status word of the factorisation
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sym_dot_cols_kernel, dim3(n), dim3(PF_T), 0, st, d_a, lda, d_b, ldb, n, part);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_fixed_kernel, dim3(1), dim3(PF_T), 0, st, part, n, d_out);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_potrf_logdet_f64(const double *d_l, int n, int64_t ldl, double *h_out, void *stream) {
    if (n < 1 || !d_l || !h_out || ldl < n) return fail("jxg_potrf_logdet_f64: need n >= 1, ldl >= n and non-NULL arguments");
    PfWork &w = pf_work();
    if (w.grow(w.small, 256)) return 1;
    double *d_out = w.small.as<double>() + 8;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(PF_T), 0, st, d_l, ldl, n, d_out);
    JX_LAUNCH_CHECK();
    JX_HIP(hipMemcpyAsync(h_out, d_out, sizeof(double), hipMemcpyDeviceToHost, st));
    JX_HIP(hipStreamSynchronize(st));
    return 0;
}
