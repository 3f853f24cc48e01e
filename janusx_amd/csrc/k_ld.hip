// Banded SNP x SNP Gram of the P32 image over the samples, for LD pruning (`jx gformat -prune`: `bed_packed_ld_prune_maf_priority`,
// src/stats/ld.rs:4245-4361, greedy of :270-402) and the LD-block r^2 matrix (`bed_ldblock_r2_rust`, :4721-4811).
//
// Everything that decides whether a pair of SNPs is "in LD" is a function of six integer sums over the samples.  With g the
// dosage (0 at a missing call) and v the called indicator of a row:
//     D = sum g_i g_j,  N = sum v_i v_j,  S_i = sum g_i v_j,  S_j = sum v_i g_j,  Q_i = sum g_i^2 v_j,  Q_j = sum v_i g_j^2
// The planes g (0/1/2), g^2 (0/1/4) and v (0/1) of 16 two-bit codes are decoded in registers from the lane's own payload dword,
// with the decoders of i8_tile.h, and are both operands of v_mfma_i32_16x16x64_i8: A holds 16 SNPs i (row = lane & 15), B 16
// SNPs j (column = lane & 15), the lane's quarter (lane >> 4) its 16 samples of a 64-sample step.  Lane (s, kq) then holds the
// sums of the pairs (i0 + 4 kq + r, j0 + s), r = 0..3.  Pad samples of the image are code 01 (missing) and add nothing.
//
// One wave owns one block of 32 x 32 pairs (2 x 2 MFMA tiles) for the whole sample range: whole units per wave, no float
// atomics, a fixed order.  Block (x, y) of the grid is the i-block y of the row range against the j-block x blocks to its right;
// a wave whose j-block lies beyond the band of every row of its i-block ends at once.  Two forms of the main loop:
//     clean  one product (D): no row of either block has a missing call
//     six    the six products: some row of either block has one
// and two epilogues:
//     (a) prune  r^2 in f64 in the reference's operation order (src/stats/ld.rs:339-367, src/math/ld.rs:817-834) from the sums
//                and the per-row mean / std / has_missing, compared with the threshold; one bit per pair (i, j > i) in a band
//                mask: bit (j - i - 1) of row i, `wpr` 32-bit words per row.  The 16 lanes of a quarter hold 16 consecutive j of
//                one i: a wave ballot gives their bits, one lane per quarter ORs them into the row (integer OR: any order gives
//                the same words).
//     (b) sums   the six i32 sums of a rectangular block of pairs, for the LD-block matrix and for tests.
//     (c) score  LD scores (`jx gstats -ldsc`: `compute_ldscore_core`, src/stats/gstats.rs:1002-1171): l_i = self_i + sum of r^2(i, j)
//                over the two-sided window start[i] <= j < end[i], j != i.  The band is computed two-sided: block (i-block, j-block)
//                serves the rows of the i-block only, because the clean formula rounds n mean_i mean_j and denom std_i std_j left to
//                right from i's side and the reference evaluates every pair from the side of the row it adds to.  j-blocks are
//                the 32-row blocks of the row list (absolute multiples of 32), from the one that holds the smallest start of
//                the i-block to the one that holds its largest end; a wave adds its 32 x 32 values along j (in lane over its two
//                j tiles, then over the 16 lanes of a quarter) and writes one f64 per (row, j-block); a second kernel adds the
//                self term and the partials of a row in ascending j-block.
#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

constexpr int LD_WAVES = 4;          // waves per workgroup: four j-blocks of one i-block
constexpr int LD_U = 2;              // MFMA tiles of 16 SNPs per side of a wave's block
constexpr int LD_B = 16 * LD_U;      // SNPs per side of a wave's block
// a sample adds at most 4 to a sum (g^2 v, or g g): an i32 accumulator is exact up to 2^29 samples.  The pairwise formula
// multiplies two sums in f64 (D N, Q N, S S <= 4 n^2), exact below 2^53: n <= 2^24 keeps every product an exact integer.
constexpr int LD_MAX_N = 1 << 24;

// g^2 (0 / 1 / 4) from the dose bytes (`counts16` of i8_tile.h)
__device__ __forceinline__ i32x4 ld_square(const i32x4 g) {
    i32x4 q;
    q.x = (g.x & 0x01010101) | ((g.x & 0x02020202) << 1);
    q.y = (g.y & 0x01010101) | ((g.y & 0x02020202) << 1);
    q.z = (g.z & 0x01010101) | ((g.z & 0x02020202) << 1);
    q.w = (g.w & 0x01010101) | ((g.w & 0x02020202) << 1);
    return q;
}

// record (row of the P32 image) of position o of the row list, positions past the end read the last row (their sums are unused)
__device__ __forceinline__ int64_t ld_record(const int32_t *__restrict__ rows, int nrows, int o) {
    const int c = o < nrows ? o : nrows - 1;
    return rows ? (int64_t)rows[c] : (int64_t)c;
}

// acc[p][ui][uj]: p = 0 D, and with SIX 1 N, 2 S_i, 3 S_j, 4 Q_i, 5 Q_j
template <bool SIX>
__device__ __forceinline__ void ld_main(const uint8_t *__restrict__ p32, int64_t tstride, int ntiles, const int32_t *__restrict__ rows,
                                        int nrows, int i0, int j0, i32x4 (&acc)[SIX ? 6 : 1][LD_U][LD_U]) {
    const int lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const uint8_t *pi[LD_U], *pj[LD_U];
#pragma unroll
    for (int u = 0; u < LD_U; ++u) {
        pi[u] = p32 + ld_record(rows, nrows, i0 + 16 * u + s) * 32 + 8 * kq;
        pj[u] = p32 + ld_record(rows, nrows, j0 + 16 * u + s) * 32 + 8 * kq;
    }
#pragma unroll
    for (int p = 0; p < (SIX ? 6 : 1); ++p)
#pragma unroll
        for (int a = 0; a < LD_U; ++a)
#pragma unroll
            for (int b = 0; b < LD_U; ++b) acc[p][a][b] = i32x4{0, 0, 0, 0};
    uint2 ni[LD_U], nj[LD_U];                                 // the next tile's words are in flight under this tile's products
#pragma unroll
    for (int u = 0; u < LD_U; ++u) {
        ni[u] = *reinterpret_cast<const uint2 *>(pi[u]);
        nj[u] = *reinterpret_cast<const uint2 *>(pj[u]);
    }
    for (int t = 0; t < ntiles; ++t) {
        uint2 wi[LD_U], wj[LD_U];
        const int tn = t + 1 < ntiles ? t + 1 : t;
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            wi[u] = ni[u];
            wj[u] = nj[u];
            ni[u] = *reinterpret_cast<const uint2 *>(pi[u] + (int64_t)tn * tstride);
            nj[u] = *reinterpret_cast<const uint2 *>(pj[u] + (int64_t)tn * tstride);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            i32x4 gi[LD_U], gj[LD_U];
#pragma unroll
            for (int u = 0; u < LD_U; ++u) {
                gi[u] = (i32x4)counts16(h ? wi[u].y : wi[u].x);
                gj[u] = (i32x4)counts16(h ? wj[u].y : wj[u].x);
            }
#pragma unroll
            for (int a = 0; a < LD_U; ++a)
#pragma unroll
                for (int b = 0; b < LD_U; ++b) acc[0][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(gi[a], gj[b], acc[0][a][b], 0, 0, 0);
            if constexpr (SIX) {
                i32x4 vi[LD_U], vj[LD_U], qi[LD_U], qj[LD_U];
#pragma unroll
                for (int u = 0; u < LD_U; ++u) {
                    vi[u] = (i32x4)called16(h ? wi[u].y : wi[u].x);
                    vj[u] = (i32x4)called16(h ? wj[u].y : wj[u].x);
                    qi[u] = ld_square(gi[u]);
                    qj[u] = ld_square(gj[u]);
                }
#pragma unroll
                for (int a = 0; a < LD_U; ++a)
#pragma unroll
                    for (int b = 0; b < LD_U; ++b) {
                        acc[1][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vi[a], vj[b], acc[1][a][b], 0, 0, 0);
                        acc[2][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(gi[a], vj[b], acc[2][a][b], 0, 0, 0);
                        acc[3][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vi[a], gj[b], acc[3][a][b], 0, 0, 0);
                        acc[4][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qi[a], vj[b], acc[4][a][b], 0, 0, 0);
                        acc[5][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vi[a], qj[b], acc[5][a][b], 0, 0, 0);
                    }
            }
        }
    }
}

__device__ __forceinline__ int ld_elem(const i32x4 a, int r) { return r == 0 ? a.x : (r == 1 ? a.y : (r == 2 ? a.z : a.w)); }

// r^2 of a pair with both rows complete: src/stats/ld.rs:339-355
__device__ __forceinline__ double ld_r2_clean(int d, double nf, double denom, double mean_i, double mean_j, double sd_i, double sd_j) {
    const double dot = (double)d;
    const double cov = dot - nf * mean_i * mean_j;
    const double denom_corr = denom * sd_i * sd_j;
    const double corr = denom_corr > 0.0 ? cov / denom_corr : 0.0;
    return corr * corr;
}

// pairwise-complete r^2 from the integer sums: src/math/ld.rs:817-834 (NaN where the reference has no value)
__device__ __forceinline__ double ld_r2_pairwise(int d, int nn, int s_i, int s_j, int q_i, int q_j) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (nn <= 1) return nan;
    const double n = (double)nn, si = (double)s_i, sj = (double)s_j, si2 = (double)q_i, sj2 = (double)q_j, sij = (double)d;
    const double cov_num = sij * n - si * sj;
    const double var_i_num = si2 * n - si * si;
    const double var_j_num = sj2 * n - sj * sj;
    const double den = var_i_num * var_j_num;
    if (!(isfinite(den) && den > 0.0 && isfinite(cov_num))) return nan;
    return (cov_num * cov_num) / den;
}

template <bool SIX>
__device__ __forceinline__ void ld_band_block(const uint8_t *__restrict__ p32, int64_t tstride, int ntiles, int n,
                                              const int32_t *__restrict__ rows, int nrows, int r0, int r1, int i0, int j0,
                                              const int32_t *__restrict__ band_end, const double *__restrict__ mean,
                                              const double *__restrict__ sd, const uint8_t *__restrict__ hasmiss, double thresh,
                                              int wpr, uint32_t *__restrict__ mask) {
    i32x4 acc[SIX ? 6 : 1][LD_U][LD_U];
    ld_main<SIX>(p32, tstride, ntiles, rows, nrows, i0, j0, acc);
    const int lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const double nf = (double)n, denom = (double)(n - 1 > 1 ? n - 1 : 1);
#pragma unroll
    for (int b = 0; b < LD_U; ++b) {
        const int j = j0 + 16 * b + s;
        const bool jin = j < nrows;
        const double mean_j = jin ? mean[j] : 0.0, sd_j = jin ? sd[j] : 0.0;
        const bool hm_j = jin ? hasmiss[j] != 0 : true;
#pragma unroll
        for (int a = 0; a < LD_U; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * a + 4 * kq + r;
                bool hit = false;
                if (i < r1 && jin && j > i) {
                    int64_t be = band_end[i];                               // never beyond the mask row or the row list
                    const int64_t cap = (int64_t)i + 1 + 32 * (int64_t)wpr;
                    be = be < cap ? be : cap;
                    if ((int64_t)j < be) {
                        double r2;
                        if (!SIX || (!hasmiss[i] && !hm_j))
                            r2 = ld_r2_clean(ld_elem(acc[0][a][b], r), nf, denom, mean[i], mean_j, sd[i], sd_j);
                        else
                            r2 = ld_r2_pairwise(ld_elem(acc[0][a][b], r), ld_elem(acc[SIX ? 1 : 0][a][b], r),
                                                ld_elem(acc[SIX ? 2 : 0][a][b], r), ld_elem(acc[SIX ? 3 : 0][a][b], r),
                                                ld_elem(acc[SIX ? 4 : 0][a][b], r), ld_elem(acc[SIX ? 5 : 0][a][b], r));
                        hit = isfinite(r2) && r2 > thresh;
                    }
                }
                const unsigned long long bal = __ballot(hit);
                const uint32_t bits = (uint32_t)(bal >> (16 * kq)) & 0xffffu;  // j = j0 + 16 b + 0..15 of this lane's row i
                if (s == 0 && bits) {                                       // bits are set only where i < r1 and j < be
                    int64_t o = (int64_t)j0 + 16 * b - i - 1;               // bit index of the first of them: >= -32
                    unsigned long long v = bits;
                    if (o < 0) {
                        v >>= (int)(-o);
                        o = 0;
                    }
                    v <<= (int)(o & 31);
                    uint32_t *row = mask + (int64_t)(i - r0) * wpr + (o >> 5);
                    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
                    if (lo) atomicOr(row, lo);
                    if (hi) atomicOr(row + 1, hi);
                }
            }
        }
    }
}

// grid (x: ceil(njb / LD_WAVES), y: i-blocks of [r0, r1)); wave = one (i-block, j-block) pair.  One launch per form: a wave
// whose pair is of the other form ends at once, so the clean form keeps its small register budget.
template <bool SIX>
__global__ __launch_bounds__(LD_WAVES * 64) void ld_band_kernel(const uint8_t *__restrict__ p32, int64_t m_total, int ntiles, int n,
                                                                const int32_t *__restrict__ rows, int nrows, int r0, int r1,
                                                                const int32_t *__restrict__ band_end, const double *__restrict__ mean,
                                                                const double *__restrict__ sd, const uint8_t *__restrict__ hasmiss,
                                                                double thresh, int wpr, int njb, uint32_t *__restrict__ mask) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * LD_WAVES + wave;
    const int64_t i0l = (int64_t)r0 + (int64_t)blockIdx.y * LD_B, j0l = i0l + (int64_t)x * LD_B;
    if (x >= njb || i0l >= r1 || j0l >= nrows) return;
    const int i0 = (int)i0l, j0 = (int)j0l;
    // reach of the i-block's band, and whether either block holds a row with a missing call
    int be = 0, miss = 0;
    if (lane < LD_B) {
        const int i = i0 + lane, j = j0 + lane;
        if (i < r1) {
            be = band_end[i];
            miss = hasmiss[i];
        }
        if (j < nrows) miss |= hasmiss[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(be, off, 64);
        be = o > be ? o : be;
    }
    if (j0 >= be) return;                                     // wave-uniform
    if ((__ballot(miss != 0) != 0ull) != SIX) return;         // wave-uniform
    ld_band_block<SIX>(p32, m_total * 32, ntiles, n, rows, nrows, r0, r1, i0, j0, band_end, mean, sd, hasmiss, thresh, wpr, mask);
}

// sums[p][i - i0][j - j0] for i in [i0, i1), j in [j0, j1) of the row list; grid (x: j-blocks / LD_WAVES, y: i-blocks)
__global__ __launch_bounds__(LD_WAVES * 64) void ld_sums_kernel(const uint8_t *__restrict__ p32, int64_t m_total, int ntiles,
                                                                const int32_t *__restrict__ rows, int nrows, int i0, int i1, int j0,
                                                                int j1, int32_t *__restrict__ sums) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int64_t ibl = (int64_t)i0 + (int64_t)blockIdx.y * LD_B, jbl = (int64_t)j0 + ((int64_t)blockIdx.x * LD_WAVES + wave) * LD_B;
    if (ibl >= i1 || jbl >= j1) return;
    const int ib = (int)ibl, jb = (int)jbl;
    i32x4 acc[6][LD_U][LD_U];
    ld_main<true>(p32, m_total * 32, ntiles, rows, nrows, ib, jb, acc);
    const int64_t ni = i1 - i0, nj = j1 - j0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int a = 0; a < LD_U; ++a)
#pragma unroll
            for (int b = 0; b < LD_U; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ib + 16 * a + 4 * kq + r, j = jb + 16 * b + s;
                    if (i < i1 && j < j1) sums[((int64_t)p * ni + (i - i0)) * nj + (j - j0)] = ld_elem(acc[p][a][b], r);
                }
}

// r^2 of one pair as the LD score adds it (src/stats/gstats.rs:956-1000, 1063-1100): clamped to [0, 1]; 0 where the clean formula
// has no positive denominator or a non-finite covariance (a finite covariance cannot give a non-finite square here: the square
// stays below 1e40) and where the pairwise-complete formula has no value
template <bool SIX>
__device__ __forceinline__ double ld_score_pair(const i32x4 (&acc)[SIX ? 6 : 1][LD_U][LD_U], int a, int b, int r, bool clean, double nf,
                                                double denom, double mean_i, double mean_j, double sd_i, double sd_j) {
    double r2;
    if (!SIX || clean)
        r2 = ld_r2_clean(ld_elem(acc[0][a][b], r), nf, denom, mean_i, mean_j, sd_i, sd_j);
    else
        r2 = ld_r2_pairwise(ld_elem(acc[0][a][b], r), ld_elem(acc[SIX ? 1 : 0][a][b], r), ld_elem(acc[SIX ? 2 : 0][a][b], r),
                            ld_elem(acc[SIX ? 3 : 0][a][b], r), ld_elem(acc[SIX ? 4 : 0][a][b], r), ld_elem(acc[SIX ? 5 : 0][a][b], r));
    if (!isfinite(r2)) return 0.0;
    return r2 < 0.0 ? 0.0 : (r2 > 1.0 ? 1.0 : r2);
}

// grid (x: ceil(npb / LD_WAVES), y: i-blocks of [r0, r1), r0 a multiple of LD_B); wave = the i-block against the x-th j-block of
// its reach.  part ((r1 - r0) rows of npb f64, zeroed by the caller): part[i - r0][x] = sum over the j of that block inside row
// i's window.  One launch per form, as for the mask.  Two waves per SIMD are asked for: the six form then keeps its 96 accumulators
// in 156 VGPRs without scratch (left alone the compiler takes 266 registers: one wave per SIMD).
template <bool SIX>
__global__ __launch_bounds__(LD_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2))) void ld_score_kernel(
    const uint8_t *__restrict__ p32, int64_t m_total, int ntiles, int n, const int32_t *__restrict__ rows, int nrows, int r0, int r1,
    const int32_t *__restrict__ start, const int32_t *__restrict__ end, const double *__restrict__ mean, const double *__restrict__ sd,
    const uint8_t *__restrict__ hasmiss, int npb, double *__restrict__ part) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int x = blockIdx.x * LD_WAVES + wave;
    const int64_t i0l = (int64_t)r0 + (int64_t)blockIdx.y * LD_B;
    if (x >= npb || i0l >= r1) return;
    const int i0 = (int)i0l;
    // reach of the i-block: the j-blocks that hold the smallest start and the largest end of its rows
    int lo = nrows, hi = 0, miss = 0;
    if (lane < LD_B && i0 + lane < r1) {
        lo = start[i0 + lane];
        hi = end[i0 + lane];
        miss = hasmiss[i0 + lane];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int l = __shfl_xor(lo, off, 64), h = __shfl_xor(hi, off, 64);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    lo = lo < 0 ? 0 : lo;                                     // never outside the row list
    hi = hi > nrows ? nrows : hi;
    if (hi <= lo) return;
    const int jb0 = lo / LD_B, jb1 = (hi - 1) / LD_B;
    if (x > jb1 - jb0) return;                                // wave-uniform: its partials stay zero
    const int j0 = (jb0 + x) * LD_B;                          // <= hi - 1 < nrows
    if (lane < LD_B && j0 + lane < nrows) miss |= hasmiss[j0 + lane];
    if ((__ballot(miss != 0) != 0ull) != SIX) return;         // wave-uniform
    i32x4 acc[SIX ? 6 : 1][LD_U][LD_U];
    ld_main<SIX>(p32, m_total * 32, ntiles, rows, nrows, i0, j0, acc);
    const double nf = (double)n, denom = (double)(n - 1 > 1 ? n - 1 : 1);
#pragma unroll
    for (int a = 0; a < LD_U; ++a) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 16 * a + 4 * kq + r;
            const bool iin = i < r1;
            const int si = iin ? start[i] : 0, ei = iin ? end[i] : 0;
            const double mean_i = iin ? mean[i] : 0.0, sd_i = iin ? sd[i] : 0.0;
            const bool hm_i = iin ? hasmiss[i] != 0 : true;
            double sum = 0.0;
#pragma unroll
            for (int b = 0; b < LD_U; ++b) {                  // in lane over the j tiles
                const int j = j0 + 16 * b + s;
                if (iin && j < nrows && j >= si && j < ei && j != i)
                    sum += ld_score_pair<SIX>(acc, a, b, r, !hm_i && !hasmiss[j], nf, denom, mean_i, mean[j], sd_i, sd[j]);
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off, 64);   // the 16 lanes of a quarter: one row i
            if (s == 0 && iin) part[(int64_t)(i - r0) * npb + x] = sum;
        }
    }
}

// score[i] = self[i] + part[i - r0][0] + part[i - r0][1] + ... in that order, for the positions [r0, r1)
__global__ __launch_bounds__(256) void ld_score_reduce_kernel(const double *__restrict__ part, const double *__restrict__ self, int r0,
                                                              int r1, int npb, double *__restrict__ score) {
    const int64_t i = (int64_t)r0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r1) return;
    const double *p = part + (i - r0) * npb;
    double sum = self[i];
    for (int x = 0; x < npb; ++x) sum += p[x];
    score[i] = sum;
}

static int ld_check(const char *who, int64_t m_total, int n, int nrows) {
    if (n <= 0) return fail(std::string(who) + ": n must be > 0");
    if (n > LD_MAX_N) return fail(std::string(who) + ": at most 16 777 216 samples (exact i32 sums and exact f64 products of them)");
    if (nrows <= 0 || m_total <= 0) return fail(std::string(who) + ": no rows");
    return 0;
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_ld_band_mask_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int r0, int r1,
                                    const int32_t *d_band_end, const double *d_mean, const double *d_std, const uint8_t *d_hasmiss,
                                    double r2_threshold, int wpr, uint32_t *d_mask, void *stream) {
    if (ld_check("jxg_ld_band_mask_p32", m_total, n, nrows)) return 1;
    if (r0 < 0 || r1 < r0 || r1 > nrows) return fail("jxg_ld_band_mask_p32: row range outside the row list");
    if (wpr < 1 || wpr > (1 << 24)) return fail("jxg_ld_band_mask_p32: words per mask row must be in [1, 2^24]");
    if (r1 == r0) return 0;
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_mask, 0, sizeof(uint32_t) * (size_t)(r1 - r0) * (size_t)wpr, st));
    const int njb = wpr + 1;                                  // j-blocks at i0 + 32 x <= i0 + 31 + 32 wpr
    const double thresh = r2_threshold * (1.0 + 1e-12);       // src/stats/ld.rs:121-122
    const dim3 grid((njb + LD_WAVES - 1) / LD_WAVES, (r1 - r0 + LD_B - 1) / LD_B), block(LD_WAVES * 64);
    if (grid.y > 65535u) return fail("jxg_ld_band_mask_p32: at most 2 097 120 rows per range");
    hipLaunchKernelGGL(ld_band_kernel<false>, grid, block, 0, st, d_p32, m_total, num_tiles(n), n, d_rows, nrows, r0, r1, d_band_end,
                       d_mean, d_std, d_hasmiss, thresh, wpr, njb, d_mask);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_band_kernel<true>, grid, block, 0, st, d_p32, m_total, num_tiles(n), n, d_rows, nrows, r0, r1, d_band_end,
                       d_mean, d_std, d_hasmiss, thresh, wpr, njb, d_mask);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_ld_sums_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int i0, int i1, int j0,
                               int j1, int32_t *d_sums, void *stream) {
    if (ld_check("jxg_ld_sums_p32", m_total, n, nrows)) return 1;
    if (i0 < 0 || i1 < i0 || i1 > nrows || j0 < 0 || j1 < j0 || j1 > nrows) return fail("jxg_ld_sums_p32: block outside the row list");
    if (i1 == i0 || j1 == j0) return 0;
    const int jblocks = (j1 - j0 + LD_B - 1) / LD_B;
    const dim3 grid((jblocks + LD_WAVES - 1) / LD_WAVES, (i1 - i0 + LD_B - 1) / LD_B), block(LD_WAVES * 64);
    if (grid.y > 65535u) return fail("jxg_ld_sums_p32: at most 2 097 120 rows per block");
    hipLaunchKernelGGL(ld_sums_kernel, grid, block, 0, (hipStream_t)stream, d_p32, m_total, num_tiles(n), d_rows, nrows, i0, i1, j0, j1,
                       d_sums);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_ld_score_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int r0, int r1,
                                const int32_t *d_start, const int32_t *d_end, const double *d_mean, const double *d_std,
                                const uint8_t *d_hasmiss, const double *d_self, int npb, double *d_part, double *d_score,
                                void *stream) {
    if (ld_check("jxg_ld_score_p32", m_total, n, nrows)) return 1;
    if (r0 < 0 || r1 < r0 || r1 > nrows) return fail("jxg_ld_score_p32: row range outside the row list");
    if (r0 % LD_B) return fail("jxg_ld_score_p32: a row range starts at a multiple of 32 of the row list");
    if (npb < 1 || npb > (1 << 26)) return fail("jxg_ld_score_p32: partials per row must be in [1, 2^26]");
    if (r1 == r0) return 0;
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_part, 0, sizeof(double) * (size_t)(r1 - r0) * (size_t)npb, st));
    const dim3 grid((npb + LD_WAVES - 1) / LD_WAVES, (r1 - r0 + LD_B - 1) / LD_B), block(LD_WAVES * 64);
    if (grid.y > 65535u) return fail("jxg_ld_score_p32: at most 2 097 120 rows per range");
    hipLaunchKernelGGL(ld_score_kernel<false>, grid, block, 0, st, d_p32, m_total, num_tiles(n), n, d_rows, nrows, r0, r1, d_start,
                       d_end, d_mean, d_std, d_hasmiss, npb, d_part);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_score_kernel<true>, grid, block, 0, st, d_p32, m_total, num_tiles(n), n, d_rows, nrows, r0, r1, d_start,
                       d_end, d_mean, d_std, d_hasmiss, npb, d_part);
    JX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ld_score_reduce_kernel, dim3((r1 - r0 + 255) / 256), dim3(256), 0, st, d_part, d_self, r0, r1, npb, d_score);
    JX_LAUNCH_CHECK();
    return 0;
}
