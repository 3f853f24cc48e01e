// Cross-validation passes of `jx adamixture -cverror` over the resident P32 image (reference `cv_fold_hash64`,
// src/stats/adamixture.rs:1641-1661; `cv_observed_fold_counts_packed_impl`, :3056-3128; `cv_training_row_freq_packed_impl`,
// :3130-3214; `holdout_nll_packed_fold_f32_impl`, :4551-4631).  The called genotype of kept row j (position in the row list)
// and sample i (0 .. n - 1, the true sample count) belongs to fold hash(j n + i) mod folds, a SplitMix64 step keyed by the
// seed; missing calls (code 01) and the padding samples of the last tile belong to no fold.
//
// Fold counts and fold image.  A workgroup of 128 lanes owns 16 rows of the row list and a slice of the sample tiles; lane
// (row, word) reads one 32-bit word of the P32 record (16 samples of one row: the 16 rows of one tile are 512 contiguous
// bytes when the row list is the identity) and hashes its 16 genotypes.  The counts pass adds into a histogram in LDS
// (several copies, so that lanes seldom meet on one counter) and then into the 64-bit global counters; the image pass writes
// the word back with the fold's calls turned into 01 and keeps the row's three integers in registers over its tiles, folds
// them over the row's 8 lanes and adds them to the row's counters.  Integer atomics only: the order does not matter.
//
// Hold-out likelihood.  The layout of `admx_loglik_kernel` (lane = sample with q_i in registers, 32 rows of P in LDS, f32
// dot product in k order, f64 logarithms), the clamp in f64 and the ln 2 of a heterozygote.  A lane first hashes its 32 calls
// of a group and notes the held-out ones in a bit mask, then walks the set bits: a wavefront pays for the logarithms of its
// busiest lane's held-out calls, not of every row.  Per-workgroup partial sums and counts, added by one thread in a fixed
// order: run-to-run identical bits.
//
// The three passes are bound by the hash (two 64-bit multiplies and a modulo per genotype of 2 bits), not by memory.
#include <math.h>

#include "jx_common.h"

namespace jx {

constexpr int CV_THREADS = 128;                 // lanes per workgroup = samples per P32 tile
constexpr int CV_ROWS = 16;                     // rows per workgroup of the count and image passes (8 words per row and tile)
constexpr int CV_G = 32;                        // rows of P per LDS group of the hold-out pass
constexpr int CV_MAX_FOLDS = JXG_ADMX_CV_MAX_FOLDS;
constexpr int CV_HIST = 2048;                   // LDS counters of the counts pass: min(32, CV_HIST / folds) copies
constexpr int CV_MAX_K = 64;
constexpr int CV_MAX_TPS = 1 << 19;             // tiles per slice: 16 rows x 128 samples x 2^19 < 2^31 per LDS counter
constexpr double CV_REC_LO = 1e-8, CV_REC_HI = 1.0 - 1e-8;
constexpr double CV_LN2 = 0.69314718055994530942;

__device__ __forceinline__ uint64_t cv_hash(uint64_t flat, uint64_t mix) {
    uint64_t x = flat ^ mix;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// x mod f for f <= 256 by long division in base 2^16: x = h 2^32 + a 2^16 + b gives
// ((((h mod f) 2^16 + a) mod f) 2^16 + b) mod f, and every dividend stays below 2^8 2^16 + 2^16 <= 2^25 (32-bit arithmetic,
// exact for every f)
__device__ __forceinline__ uint32_t cv_mod(uint64_t x, uint32_t f) {
    uint32_t r = (uint32_t)(x >> 32) % f;
    r = ((r << 16) | ((uint32_t)(x >> 16) & 0xffffu)) % f;
    return ((r << 16) | ((uint32_t)x & 0xffffu)) % f;
}

__device__ __forceinline__ uint32_t cv_fold(uint64_t flat, uint64_t mix, uint32_t folds) {
    return cv_mod(cv_hash(flat, mix), folds);
}

// tile slices of the count and image passes: about 2048 workgroups, every slice within CV_MAX_TPS tiles
static void cv_slices(int nrows, int ntiles, int *groups, int *sl, int *tps) {
    *groups = (nrows + CV_ROWS - 1) / CV_ROWS;
    int s = (2048 + *groups - 1) / *groups;
    const int need = (ntiles + CV_MAX_TPS - 1) / CV_MAX_TPS;
    if (s < need) s = need;
    if (s > ntiles) s = ntiles;
    if (s < 1) s = 1;
    *tps = (ntiles + s - 1) / s;
    *sl = (ntiles + *tps - 1) / *tps;
}

__global__ __launch_bounds__(CV_THREADS) void admx_cv_counts_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                    const int32_t *__restrict__ rows, int nrows, int n,
                                                                    int ntiles, int tps, uint32_t folds, uint64_t mix,
                                                                    unsigned long long *__restrict__ counts) {
    __shared__ uint32_t hist[CV_HIST];
    const int lane = threadIdx.x;
    for (int e = lane; e < CV_HIST; e += CV_THREADS) hist[e] = 0u;
    __syncthreads();
    const uint32_t copies = min(32u, (uint32_t)CV_HIST / folds);
    uint32_t *mine = hist + ((uint32_t)lane % copies) * folds;
    const int j = blockIdx.x * CV_ROWS + (lane >> 3), w = lane & 7;
    const int t0 = blockIdx.y * tps, t1 = min(ntiles, t0 + tps);
    if (j < nrows) {
        const int64_t rec = rows ? (int64_t)rows[j] : (int64_t)j;
        for (int tile = t0; tile < t1; ++tile) {
            const uint32_t word = p32[((int64_t)tile * m_total + rec) * 8 + w];
            const int i0 = tile * CV_THREADS + w * 16;
            const uint64_t flat0 = (uint64_t)j * (uint64_t)n + (uint64_t)i0;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                if (((word >> (2 * s)) & 3u) == 1u || i0 + s >= n) continue;
                atomicAdd(&mine[cv_fold(flat0 + (uint64_t)s, mix, folds)], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t f = lane; f < folds; f += CV_THREADS) {
        unsigned long long c = 0;
        for (uint32_t cp = 0; cp < copies; ++cp) c += hist[cp * folds + f];
        if (c) atomicAdd(&counts[f], c);
    }
}

// out: (ntiles, nrows, 8) words in row-list order; stats: (nrows, 3) = training calls, held-out calls, minor-allele sum of
// the training calls (zeroed by the caller)
__global__ __launch_bounds__(CV_THREADS) void admx_cv_image_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                   const int32_t *__restrict__ rows, int nrows,
                                                                   const uint8_t *__restrict__ flip, int n, int ntiles, int tps,
                                                                   uint32_t folds, uint64_t mix, uint32_t fold_id,
                                                                   uint32_t *__restrict__ out, int32_t *__restrict__ stats) {
    const int lane = threadIdx.x;
    const int j = blockIdx.x * CV_ROWS + (lane >> 3), w = lane & 7;
    const int t0 = blockIdx.y * tps, t1 = min(ntiles, t0 + tps);
    int train = 0, held = 0, sum = 0;
    if (j < nrows) {
        const int64_t rec = rows ? (int64_t)rows[j] : (int64_t)j;
        const bool fl = flip ? flip[j] != 0 : false;
        for (int tile = t0; tile < t1; ++tile) {
            uint32_t word = p32[((int64_t)tile * m_total + rec) * 8 + w];
            const int i0 = tile * CV_THREADS + w * 16;
            const uint64_t flat0 = (uint64_t)j * (uint64_t)n + (uint64_t)i0;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const uint32_t code = (word >> (2 * s)) & 3u;
                if (code == 1u || i0 + s >= n) continue;
                if (cv_fold(flat0 + (uint64_t)s, mix, folds) == fold_id) {
                    word = (word & ~(3u << (2 * s))) | (1u << (2 * s));
                    ++held;
                } else {
                    const int d = code == 0u ? 0 : (code == 2u ? 1 : 2);
                    ++train;
                    sum += fl ? 2 - d : d;
                }
            }
            out[((int64_t)tile * nrows + j) * 8 + w] = word;
        }
    }
    // the row's 8 lanes are neighbours within one wavefront; rows past the end carry zeros
    for (int off = 4; off > 0; off >>= 1) {
        train += __shfl_xor(train, off);
        held += __shfl_xor(held, off);
        sum += __shfl_xor(sum, off);
    }
    if (w == 0 && j < nrows) {
        if (train) atomicAdd(&stats[(int64_t)j * 3 + 0], train);
        if (held) atomicAdd(&stats[(int64_t)j * 3 + 1], held);
        if (sum) atomicAdd(&stats[(int64_t)j * 3 + 2], sum);
    }
}

struct CvGrid {
    int s1, s2, gps, tps;
};

// slices of the hold-out pass: SNP groups and sample tiles over at most 2048 workgroups (= JXG_ADMX_CV_WORK_BYTES / 16)
static CvGrid cv_grid(int nrows, int ntiles) {
    const int ngroups = (nrows + CV_G - 1) / CV_G;
    int s1 = ngroups < 256 ? ngroups : 256;
    if (s1 < 1) s1 = 1;
    int s2 = 2048 / s1;
    if (s2 > ntiles) s2 = ntiles;
    if (s2 < 1) s2 = 1;
    CvGrid g;
    g.gps = (ngroups + s1 - 1) / s1;
    g.s1 = (ngroups + g.gps - 1) / g.gps;
    g.tps = (ntiles + s2 - 1) / s2;
    g.s2 = (ntiles + g.tps - 1) / g.tps;
    if (g.s1 < 1) g.s1 = 1;
    return g;
}

template <int KB>
__global__ __launch_bounds__(CV_THREADS) void admx_cv_holdout_kernel(const uint32_t *__restrict__ p32, int64_t m_total,
                                                                     const int32_t *__restrict__ rows, int nrows,
                                                                     const uint8_t *__restrict__ flip, int n, int k,
                                                                     const float *__restrict__ p, const float *__restrict__ q,
                                                                     int gps, int tps, int ntiles, uint32_t folds, uint64_t mix,
                                                                     uint32_t fold_id, double *__restrict__ llpart,
                                                                     long long *__restrict__ npart) {
    __shared__ float p_sh[CV_G][KB];
    __shared__ double red[CV_THREADS];
    __shared__ long long nred[CV_THREADS];
    const int lane = threadIdx.x;
    const int s1 = blockIdx.x, s2 = blockIdx.y;
    const int js0 = s1 * gps * CV_G;
    const int js1 = min(nrows, js0 + gps * CV_G);
    const int t0 = s2 * tps, t1 = min(ntiles, t0 + tps);
    double acc = 0.0;
    long long cnt = 0;
    for (int tile = t0; tile < t1; ++tile) {
        const int i = tile * CV_THREADS + lane;
        float qv[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) qv[kk] = (i < n && kk < k) ? q[(int64_t)i * k + kk] : 0.0f;
        for (int j0 = js0; j0 < js1; j0 += CV_G) {
            __syncthreads();
            for (int e = lane; e < CV_G * KB; e += CV_THREADS) {
                const int jj = e / KB, kk = e % KB;
                p_sh[jj][kk] = (j0 + jj < js1 && kk < k) ? p[(int64_t)(j0 + jj) * k + kk] : 0.0f;
            }
            __syncthreads();
            const int jend = min(CV_G, js1 - j0);
            // the lane's held-out calls of the group first (a bit per row, and their codes): about one call in `folds` is
            // held out, and a wavefront that went through the logarithms whenever one of its 64 lanes holds a call would go
            // through them for nearly every row
            uint32_t heldmask = 0u;
            uint64_t codes = 0ull;
            if (i < n) {
                for (int jj = 0; jj < jend; ++jj) {
                    const int j = j0 + jj;
                    const int64_t rec_idx = rows ? (int64_t)rows[j] : (int64_t)j;
                    const uint32_t word = p32[((int64_t)tile * m_total + rec_idx) * 8 + (lane >> 4)];
                    const uint32_t code = (word >> (2 * (lane & 15))) & 3u;
                    if (code == 1u) continue;
                    if (cv_fold((uint64_t)j * (uint64_t)n + (uint64_t)i, mix, folds) != fold_id) continue;
                    heldmask |= 1u << jj;
                    codes |= (uint64_t)code << (2 * jj);
                }
            }
            while (heldmask) {                        // in row order: the lane's sum keeps one order
                const int jj = __ffs((int)heldmask) - 1;
                heldmask &= heldmask - 1u;
                const uint32_t code = (uint32_t)(codes >> (2 * jj)) & 3u;
                const int d = code == 0u ? 0 : (code == 2u ? 1 : 2);
                const int g = (flip ? flip[j0 + jj] != 0 : false) ? 2 - d : d;
                float rec = 0.0f;
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) rec += p_sh[jj][kk] * qv[kk];
                const double r = fmin(fmax((double)rec, CV_REC_LO), CV_REC_HI);
                // a factor of zero leaves its logarithm out: 0 x ln = 0 exactly (r is clamped away from 0 and 1)
                const double lr = g > 0 ? log(r) : 0.0;
                const double l1 = g < 2 ? log(1.0 - r) : 0.0;
                const double gd = (double)g;
                acc += (g == 1 ? CV_LN2 : 0.0) + gd * lr + (2.0 - gd) * l1;
                ++cnt;
            }
        }
    }
    red[lane] = acc;
    nred[lane] = cnt;
    __syncthreads();
    for (int off = CV_THREADS / 2; off > 0; off >>= 1) {
        if (lane < off) {
            red[lane] += red[lane + off];
            nred[lane] += nred[lane + off];
        }
        __syncthreads();
    }
    if (lane == 0) {
        llpart[(int64_t)s2 * gridDim.x + s1] = red[0];
        npart[(int64_t)s2 * gridDim.x + s1] = nred[0];
    }
}

__global__ void admx_cv_holdout_sum_kernel(const double *__restrict__ llpart, const long long *__restrict__ npart, int count,
                                           double *__restrict__ ll, long long *__restrict__ n_eval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    long long c = 0;
    for (int e = 0; e < count; ++e) {
        s += llpart[e];
        c += npart[e];
    }
    ll[0] = s;
    n_eval[0] = c;
}

static int cv_check(const char *who, int n, int nrows, int folds, int fold_id) {
    if (n < 1 || nrows < 1) return fail(std::string(who) + ": empty panel (n = " + std::to_string(n) + ", rows = " +
                                        std::to_string(nrows) + ")");
    if (folds < 2) return fail("CVerror requires folds >= 2, got " + std::to_string(folds) + ".");
    if (folds > CV_MAX_FOLDS) return fail(std::string(who) + ": folds must be at most " + std::to_string(CV_MAX_FOLDS) +
                                          " on this build (got " + std::to_string(folds) + ")");
    if (fold_id < 0 || fold_id >= folds) return fail("fold_id must be within [0, " + std::to_string(folds) + "), got " +
                                                     std::to_string(fold_id));
    return 0;
}

static uint64_t cv_mix(uint64_t seed) { return seed ^ 0x9E3779B97F4A7C15ull; }

static int cv_kb(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

#define CV_HOLDOUT(KB)                                                                                                  \
    hipLaunchKernelGGL(admx_cv_holdout_kernel<KB>, dim3(g.s1, g.s2), dim3(CV_THREADS), 0, st, (const uint32_t *)d_p32, \
                       m_total, d_rows, nrows, d_flip, n, k, d_p, d_q, g.gps, g.tps, ntiles, (uint32_t)folds,           \
                       cv_mix(seed), (uint32_t)fold_id, llpart, npart)

}  // namespace jx

using namespace jx;

extern "C" int jxg_admx_cv_fold_counts(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int folds,
                                       uint64_t seed, int64_t *d_counts, void *stream) {
    if (cv_check("jxg_admx_cv_fold_counts", n, nrows, folds, 0)) return 1;
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)folds, st));
    const int ntiles = num_tiles(n);
    int groups, sl, tps;
    cv_slices(nrows, ntiles, &groups, &sl, &tps);
    hipLaunchKernelGGL(admx_cv_counts_kernel, dim3(groups, sl), dim3(CV_THREADS), 0, st, (const uint32_t *)d_p32, m_total, d_rows,
                       nrows, n, ntiles, tps, (uint32_t)folds, cv_mix(seed), (unsigned long long *)d_counts);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_admx_cv_fold_image(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                      const uint8_t *d_flip, int folds, uint64_t seed, int fold_id, uint8_t *d_out_p32,
                                      int32_t *d_row_stats, void *stream) {
    if (cv_check("jxg_admx_cv_fold_image", n, nrows, folds, fold_id)) return 1;
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_row_stats, 0, sizeof(int32_t) * 3 * (size_t)nrows, st));
    const int ntiles = num_tiles(n);
    int groups, sl, tps;
    cv_slices(nrows, ntiles, &groups, &sl, &tps);
    hipLaunchKernelGGL(admx_cv_image_kernel, dim3(groups, sl), dim3(CV_THREADS), 0, st, (const uint32_t *)d_p32, m_total, d_rows,
                       nrows, d_flip, n, ntiles, tps, (uint32_t)folds, cv_mix(seed), (uint32_t)fold_id, (uint32_t *)d_out_p32,
                       d_row_stats);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_admx_cv_holdout_nll(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                       const uint8_t *d_flip, int folds, uint64_t seed, int fold_id, int k, const float *d_p,
                                       const float *d_q, void *d_work, int64_t work_bytes, double *d_ll, int64_t *d_n_eval,
                                       void *stream) {
    if (cv_check("jxg_admx_cv_holdout_nll", n, nrows, folds, fold_id)) return 1;
    if (k < 1 || k > CV_MAX_K)
        return fail("jxg_admx_cv_holdout_nll: K must be within [1, 64] (got " + std::to_string(k) + ")");
    if (k > n)
        return fail("jxg_admx_cv_holdout_nll: K = " + std::to_string(k) + " exceeds the number of samples " + std::to_string(n));
    if (work_bytes < JXG_ADMX_CV_WORK_BYTES) return fail("jxg_admx_cv_holdout_nll: work buffer too small (JXG_ADMX_CV_WORK_BYTES)");
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = num_tiles(n);
    const CvGrid g = cv_grid(nrows, ntiles);
    double *llpart = (double *)d_work;
    long long *npart = (long long *)((char *)d_work + JXG_ADMX_CV_WORK_BYTES / 2);
    switch (cv_kb(k)) {
    case 1: CV_HOLDOUT(1); break;
    case 2: CV_HOLDOUT(2); break;
    case 4: CV_HOLDOUT(4); break;
    case 8: CV_HOLDOUT(8); break;
    case 16: CV_HOLDOUT(16); break;
    case 32: CV_HOLDOUT(32); break;
    default: CV_HOLDOUT(64); break;
    }
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(admx_cv_holdout_sum_kernel, dim3(1), dim3(64), 0, st, llpart, npart, g.s1 * g.s2, d_ll, (long long *)d_n_eval);
    JX_LAUNCH_CHECK();
    return 0;
}
