// Exhaustive SNP-pair screen of the P32 image (`jx fvlmm2 -screen`; an extension: the reference finds its pairs with GARFIELD's
// logic-gate search, which is not built here).  Every combo of `fvlmm2.pair_tables` on hard calls is a function of the two 2-bit
// codes of a pair, so every first-order statistic of a combo against a fixed sample vector r follows from the 3 x 3 class table
// of the pair over the samples called at both SNPs:
//     N_ab = sum_s [c1_s = a][c2_s = b],      R_ab = sum_s [c1_s = a][c2_s = b] r_s,      classes: 00 -> 0, 10 -> 1, 11 -> 2
// (code 01, a missing call or a pad sample, belongs to no class).  Both are SNP x SNP Grams over the sample axis with 0/1
// operands, the second against r split into the four signed radix-128 digit planes of k_lm_traits.hip (`jxg_lmt_prepare`: the
// ONE definition of the split; this file only reads its plane image).
//
// Operands, per 64-sample step of v_mfma_i32_16x16x64_i8, with the lane / payload map of `ld_main` (k_ld.hip): lane (s, kq)
// decodes its own 16 samples (dword 2 kq + h of the 128-sample record, h = 0, 1) in registers with `spread16` of i8_tile.h;
//     A (16 SNPs i, row = lane & 15):     I_a(i), a = 0..2, 0/1 bytes
//     B (16 SNPs j, column = lane & 15):  I_b(j), and I_b(j) o q_p: the digit byte of plane p kept where the indicator is 1
// The digit bytes of a group are the same for every SNP: lane (s, kq) reads the 16 bytes of group 2 kq + h of each plane, which
// `lt_quant_kernel` wrote in the decode's byte order.  9 products give N, 4 x 9 = 36 give the plane sums A_p: the FULL form, 45
// products a step, serves any block (rows with missing calls included).  A clean form (classes {1, 2} and per-SNP marginals for
// blocks without a missing call, 4 + 16 products) is not built: one form, one set of tables.
// Every i32 sum is exact: a sample adds at most 64, n <= 2^24 (`PS_MAX_N`, as LD_MAX_N) keeps |A_p| <= 2^30.  The epilogue
// rebuilds the 64-bit INTEGER  R_ab = ((A_1 128 + A_2) 128 + A_3) 128 + A_4;  the real sum is R_ab S 2^-27 (S 2^-27 = `scale` of
// jxg_lmt_prepare, a power of two).
//
// Work split: one wave owns ONE 16 x 16 tile of pairs for the whole sample range: whole units per wave, no float atomics, a
// fixed order.  Register budget: 45 accumulators of 4 registers = 180, the payload words of this and the next record 8, the
// digit bytes of this and the next record 2 x 32, the decoded operands 28: one tile per wave fits the 512 registers of a wave
// that has its SIMD to itself (4 waves per workgroup, one per SIMD); a second tile (360 accumulator registers) does not.
// The scan walks the blocks of the triangle with JX_TRI_TILE, the smaller block on the A side, and keeps the pairs i < j.
//
// Epilogues:
//     (a) tables  N (Ri, Rj, 3, 3) int32 and R (Ri, Rj, 3, 3) int64 of a rectangular block of two row lists: tests, small callers.
//     (b) scan    for every pair i < j of one row list and every variant v (<= 16) the score statistic of the combo term given the
//                 intercept and both literals in the linear model of r on the pair's complete samples, error variance sigma2
//                 given.  A variant is 15 f64: C_v[a][b] (9), L1_v[a] (3), L2_v[b] (3); a flipped row reads its tables at
//                 class 2 - a.  With Z = [1, x1, x2]: Z'Z, Z'xc, xc'xc from N, Z'r, xc'r from R (f64 sums, a major, b minor),
//                 then the 3 x 3 solve written out by fraction-free elimination (n times the centred moments):
//                     d11 = n s11 - s1 s1, d12 = n s12 - s1 s2, d22 = n s22 - s2 s2, det = d11 d22 - d12 d12
//                     e_k = n c_k - s_k c_0, f_k = n r_k - s_k r_0, ecc = n cc - c_0 c_0, ecr = n cr - c_0 r_0
//                     b1 = (e1 d22 - e2 d12) / det, b2 = (e2 d11 - e1 d12) / det
//                     den = (ecc - b1 e1 - b2 e2) / n, num = (ecr - b1 f1 - b2 f2) / n, T = num^2 / (sigma2 den)
//                 The pivots of Z'Z are n, d11 / n and det / (n d11): "a pivot is not positive" is tested as d11 <= 0 or det <= 0,
//                 which for tables of small integers (every variant the host builds) are exact integers in f64 up to 2^53, so a
//                 monomorphic literal and a pair of identical or complementary rows are void exactly.  Void (T = NaN, never a
//                 hit): fewer than 5 complete samples, such a pivot, or den <= 1e-10 xc'xc (the combo lies in the span of the
//                 literals).  A hit (T >= t_min) is appended with `wave_append`; every hit is counted beyond the capacity too.
//                 Optional exclusion: a pair on one chromosome with |pos_i - pos_j| < min_dist is skipped (min_dist = 0: off).
#include <cmath>

#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

constexpr int PS_WAVES = 4;             // waves per workgroup: four tiles
constexpr int PS_PLANES = 4;            // digit planes of r (k_lm_traits.hip)
constexpr int PS_MAX_N = 1 << 24;       // |A_p| <= 64 n <= 2^30; N products below 2^53
constexpr int PS_MAX_VARIANTS = 16;
constexpr int PS_VARIANT_DOUBLES = 15;  // C (9), L1 (3), L2 (3)
constexpr int PS_MIN_COMPLETE = 5;

// the class indicators of 16 two-bit codes as 0 / 1 bytes
__device__ __forceinline__ void ps_classes16(uint32_t w, i32x4 (&c)[3]) {
    const uint32_t lo = w & P32_LO, hi = (w >> 1) & P32_LO;
    c[0] = (i32x4)spread16(~(lo | hi) & P32_LO, KEEP_BIT);
    c[1] = (i32x4)spread16(hi & ~lo, KEEP_BIT);
    c[2] = (i32x4)spread16(hi & lo, KEEP_BIT);
}

// digit bytes kept where the indicator byte is 1 (0 / 1 bytes times 255: 0x00 / 0xff, no carry between the bytes)
__device__ __forceinline__ i32x4 ps_keep(const i32x4 ind, const uint4 q) {
    i32x4 o;
    o.x = (int)(((uint32_t)ind.x * 255u) & q.x);
    o.y = (int)(((uint32_t)ind.y * 255u) & q.y);
    o.z = (int)(((uint32_t)ind.z * 255u) & q.z);
    o.w = (int)(((uint32_t)ind.w * 255u) & q.w);
    return o;
}

struct PsAcc {
    i32x4 n[3][3];                      // [a of i][b of j]
    i32x4 r[PS_PLANES][3][3];
};

// reci, recj: this lane's records (row lane & 15 of the A tile, column lane & 15 of the B tile), valid rows of the image.
// planes: plane p of r at planes + p pstride, ntiles * 128 bytes.
__device__ __forceinline__ void ps_main(const uint8_t *__restrict__ p32, int64_t tstride, int ntiles, int64_t reci, int64_t recj,
                                        const int8_t *__restrict__ planes, int64_t pstride, PsAcc &acc) {
    const int lane = threadIdx.x & 63, kq = lane >> 4;
    const uint8_t *pi = p32 + reci * 32 + 8 * kq, *pj = p32 + recj * 32 + 8 * kq;
    const int8_t *pq = planes + 32 * kq;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            acc.n[a][b] = i32x4{0, 0, 0, 0};
#pragma unroll
            for (int p = 0; p < PS_PLANES; ++p) acc.r[p][a][b] = i32x4{0, 0, 0, 0};
        }
    uint2 ni = *reinterpret_cast<const uint2 *>(pi), nj = *reinterpret_cast<const uint2 *>(pj);
    uint4 nq[PS_PLANES][2];                                   // the next record's words are in flight under this record's products
#pragma unroll
    for (int p = 0; p < PS_PLANES; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h) nq[p][h] = *reinterpret_cast<const uint4 *>(pq + p * pstride + 16 * h);
    for (int t = 0; t < ntiles; ++t) {
        const int tn = t + 1 < ntiles ? t + 1 : t;
        const uint2 wi = ni, wj = nj;
        uint4 q[PS_PLANES][2];
        ni = *reinterpret_cast<const uint2 *>(pi + (int64_t)tn * tstride);
        nj = *reinterpret_cast<const uint2 *>(pj + (int64_t)tn * tstride);
#pragma unroll
        for (int p = 0; p < PS_PLANES; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                q[p][h] = nq[p][h];
                nq[p][h] = *reinterpret_cast<const uint4 *>(pq + p * pstride + (int64_t)tn * 128 + 16 * h);
            }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            i32x4 ia[3], ib[3];
            ps_classes16(h ? wi.y : wi.x, ia);
            ps_classes16(h ? wj.y : wj.x, ib);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) acc.n[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ia[a], ib[b], acc.n[a][b], 0, 0, 0);
#pragma unroll
            for (int p = 0; p < PS_PLANES; ++p)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const i32x4 mb = ps_keep(ib[b], q[p][h]);
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        acc.r[p][a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ia[a], mb, acc.r[p][a][b], 0, 0, 0);
                }
        }
    }
}

__device__ __forceinline__ int ps_elem(const i32x4 a, int r) { return r == 0 ? a.x : (r == 1 ? a.y : (r == 2 ? a.z : a.w)); }

// R_ab of register r: the four plane sums as one 64-bit integer
__device__ __forceinline__ long long ps_combine(const PsAcc &acc, int a, int b, int r) {
    long long v = 0;
#pragma unroll
    for (int p = 0; p < PS_PLANES; ++p) v = v * 128 + (long long)ps_elem(acc.r[p][a][b], r);
    return v;
}

// position o of a row list -> record; positions past the end read the last row (their sums are unused)
__device__ __forceinline__ int64_t ps_record(const int32_t *__restrict__ rows, int nrows, int o) {
    const int c = o < nrows ? o : nrows - 1;
    return rows ? (int64_t)rows[c] : (int64_t)c;
}

// grid (x: ceil(j-blocks / PS_WAVES), y: i-blocks); wave = one 16 x 16 tile of (rows_i, rows_j)
__global__ __launch_bounds__(PS_WAVES * 64) void ps_tables_kernel(const uint8_t *__restrict__ p32, int64_t m_total, int ntiles,
                                                                  const int32_t *__restrict__ rows_i, int ni,
                                                                  const int32_t *__restrict__ rows_j, int nj,
                                                                  const int8_t *__restrict__ planes, int64_t pstride,
                                                                  int32_t *__restrict__ out_n, long long *__restrict__ out_r) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int64_t i0l = (int64_t)blockIdx.y * 16, j0l = ((int64_t)blockIdx.x * PS_WAVES + wave) * 16;
    if (i0l >= ni || j0l >= nj) return;                       // wave-uniform
    const int i0 = (int)i0l, j0 = (int)j0l;
    PsAcc acc;
    ps_main(p32, m_total * 32, ntiles, ps_record(rows_i, ni, i0 + s), ps_record(rows_j, nj, j0 + s), planes, pstride, acc);
    const int j = j0 + s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * kq + r;
        if (i >= ni || j >= nj) continue;
        const int64_t o = ((int64_t)i * nj + j) * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                out_n[o + 3 * a + b] = ps_elem(acc.n[a][b], r);
                out_r[o + 3 * a + b] = ps_combine(acc, a, b, r);
            }
    }
}

// The statistic of one variant from the tables of one pair (N as f64, R already times `scale`); `var`: the variant's 15 values;
// fi, fj: the rows' flip bits.  NaN where the pair / variant is void.  The sums run a major, b minor, in the written order.
__device__ __forceinline__ double ps_stat(const double (&nt)[9], const double (&rt)[9], const double *__restrict__ var, bool fi, bool fj,
                                          double sigma2) {
    double n = 0.0, s1 = 0.0, s2 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0, cc = 0.0;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, cr = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int pa = fi ? 2 - a : a;
        const double x1 = var[9 + pa];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int pb = fj ? 2 - b : b;
            const double x2 = var[12 + pb], xc = var[3 * pa + pb];
            const double w = nt[3 * a + b], rr = rt[3 * a + b];
            n += w;
            s1 += w * x1;
            s2 += w * x2;
            s11 += w * (x1 * x1);
            s12 += w * (x1 * x2);
            s22 += w * (x2 * x2);
            c0 += w * xc;
            c1 += w * (x1 * xc);
            c2 += w * (x2 * xc);
            cc += w * (xc * xc);
            r0 += rr;
            r1 += rr * x1;
            r2 += rr * x2;
            cr += rr * xc;
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!(n >= (double)PS_MIN_COMPLETE)) return nan;
    const double d11 = n * s11 - s1 * s1, d12 = n * s12 - s1 * s2, d22 = n * s22 - s2 * s2;
    if (!(d11 > 0.0)) return nan;
    const double det = d11 * d22 - d12 * d12;
    if (!(det > 0.0)) return nan;
    const double e1 = n * c1 - s1 * c0, e2 = n * c2 - s2 * c0, f1 = n * r1 - s1 * r0, f2 = n * r2 - s2 * r0;
    const double ecc = n * cc - c0 * c0, ecr = n * cr - c0 * r0;
    const double b1 = (e1 * d22 - e2 * d12) / det, b2 = (e2 * d11 - e1 * d12) / det;
    const double den = (ecc - b1 * e1 - b2 * e2) / n, num = (ecr - b1 * f1 - b2 * f2) / n;
    if (!(den > 1e-10 * cc)) return nan;
    return (num * num) / (sigma2 * den);
}

// grid (x: ceil(tiles of the triangle / PS_WAVES)); wave = block (tj <= ti) of the row list: A = block tj, B = block ti, the
// pairs i < j.  counts[0]: hits (beyond the capacity too), counts[1]: pairs screened (i < j, not excluded).
__global__ __launch_bounds__(PS_WAVES * 64) void ps_scan_kernel(
    const uint8_t *__restrict__ p32, int64_t m_total, int ntiles, const int32_t *__restrict__ rows, int nrows, int nblocks,
    const uint8_t *__restrict__ flip, const int32_t *__restrict__ chrom, const long long *__restrict__ pos, long long min_dist,
    const int8_t *__restrict__ planes, int64_t pstride, double scale, double sigma2, const double *__restrict__ variants, int nvariants,
    double t_min, unsigned long long cap, int32_t *__restrict__ hit_i, int32_t *__restrict__ hit_j, int32_t *__restrict__ hit_v,
    int32_t *__restrict__ hit_n, double *__restrict__ hit_stat, unsigned long long *__restrict__ counts) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, kq = lane >> 4;
    const int64_t w = (int64_t)blockIdx.x * PS_WAVES + wave;
    if (w >= (int64_t)nblocks * (nblocks + 1) / 2) return;    // wave-uniform
    int ti, tj;
    JX_TRI_TILE((int)w, ti, tj);
    const int i0 = 16 * tj, j0 = 16 * ti;                     // i0 <= j0
    PsAcc acc;
    ps_main(p32, m_total * 32, ntiles, ps_record(rows, nrows, i0 + s), ps_record(rows, nrows, j0 + s), planes, pstride, acc);
    const int j = j0 + s;
    const bool jin = j < nrows;
    const bool fj = jin ? flip[j] != 0 : false;
    const int cj = (jin && min_dist > 0) ? chrom[j] : 0;
    const long long bj = (jin && min_dist > 0) ? pos[j] : 0;
    unsigned long long screened = 0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * kq + r;
        bool live = jin && i < j;                             // i < j < nrows
        if (live && min_dist > 0 && chrom[i] == cj) {
            const long long d = pos[i] - bj;
            live = (d < 0 ? -d : d) >= min_dist;
        }
        screened += (unsigned long long)__popcll(__ballot(live));
        if (__ballot(live) == 0ull) continue;                 // wave-uniform
        const bool fi = live ? flip[i] != 0 : false;
        double nt[9], rt[9];
        int ncomp = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int c = ps_elem(acc.n[a][b], r);
                ncomp += c;
                nt[3 * a + b] = (double)c;
                rt[3 * a + b] = (double)ps_combine(acc, a, b, r) * scale;
            }
        for (int v = 0; v < nvariants; ++v) {                 // wave-uniform
            const double t = ps_stat(nt, rt, variants + v * PS_VARIANT_DOUBLES, fi, fj, sigma2);
            const bool hit = live && t >= t_min;              // NaN is never a hit
            wave_append(hit, counts, cap, [=](unsigned long long slot) {
                hit_i[slot] = i;
                hit_j[slot] = j;
                hit_v[slot] = v;
                hit_n[slot] = ncomp;
                hit_stat[slot] = t;
            });
        }
    }
    if (lane == 0 && screened) atomicAdd(counts + 1, screened);   // integer: any order gives the same count
}

static int ps_check(const char *who, int64_t m_total, int n, const void *d_p32, const void *d_planes, int64_t pstride) {
    if (n <= 0) return fail(std::string(who) + ": n must be > 0");
    if (n > PS_MAX_N) return fail(std::string(who) + ": at most 16 777 216 samples (exact i32 plane sums)");
    if (m_total <= 0 || !d_p32) return fail(std::string(who) + ": empty image");
    if (!d_planes || pstride < (int64_t)num_tiles(n) * JXG_TILE)
        return fail(std::string(who) + ": the digit planes of r are missing or shorter than the padded sample axis");
    return 0;
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_pairscreen_max_variants(void) { return PS_MAX_VARIANTS; }

extern "C" int jxg_pairscreen_tables_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows_i, int ni,
                                         const int32_t *d_rows_j, int nj, const int8_t *d_planes, int64_t plane_stride, int32_t *d_n,
                                         int64_t *d_r, void *stream) {
    if (ps_check("jxg_pairscreen_tables_p32", m_total, n, d_p32, d_planes, plane_stride)) return 1;
    if (ni < 0 || nj < 0) return fail("jxg_pairscreen_tables_p32: negative row count");
    if (ni == 0 || nj == 0) return 0;
    if (!d_rows_i || !d_rows_j || !d_n || !d_r) return fail("jxg_pairscreen_tables_p32: row lists or outputs missing");
    const int jblocks = (nj + 15) / 16;
    const dim3 grid((jblocks + PS_WAVES - 1) / PS_WAVES, (ni + 15) / 16), block(PS_WAVES * 64);
    if (grid.y > 65535u) return fail("jxg_pairscreen_tables_p32: at most 1 048 560 rows in the first list");
    hipLaunchKernelGGL(ps_tables_kernel, grid, block, 0, (hipStream_t)stream, d_p32, m_total, num_tiles(n), d_rows_i, ni, d_rows_j, nj,
                       d_planes, plane_stride, d_n, reinterpret_cast<long long *>(d_r));
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_pairscreen_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                                       const uint8_t *d_flip, const int32_t *d_chrom, const int64_t *d_pos, int64_t min_dist,
                                       const int8_t *d_planes, int64_t plane_stride, double scale, double sigma2,
                                       const double *d_variants, int nvariants, double t_min, int64_t capacity, int32_t *d_hit_i,
                                       int32_t *d_hit_j, int32_t *d_hit_v, int32_t *d_hit_n, double *d_hit_stat, uint64_t *d_counts,
                                       void *stream) {
    if (ps_check("jxg_pairscreen_scan_p32", m_total, n, d_p32, d_planes, plane_stride)) return 1;
    if (nrows < 0) return fail("jxg_pairscreen_scan_p32: negative row count");
    if (nrows > 16 * 46340) return fail("jxg_pairscreen_scan_p32: at most 741 440 rows per call (the blocks of the triangle are counted in 31 bits)");
    if (nvariants < 1 || nvariants > PS_MAX_VARIANTS)
        return fail("jxg_pairscreen_scan_p32: between 1 and " + std::to_string(PS_MAX_VARIANTS) + " variants, got " + std::to_string(nvariants));
    if (!(sigma2 > 0.0) || !std::isfinite(sigma2)) return fail("jxg_pairscreen_scan_p32: sigma2 must be finite and positive");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail("jxg_pairscreen_scan_p32: scale must be finite and positive");
    if (!(t_min == t_min)) return fail("jxg_pairscreen_scan_p32: t_min is NaN");
    if (min_dist < 0) return fail("jxg_pairscreen_scan_p32: min_dist must be >= 0");
    if (min_dist > 0 && (!d_chrom || !d_pos)) return fail("jxg_pairscreen_scan_p32: min_dist needs chromosome ids and positions");
    if (capacity < 0 || !d_flip || !d_variants || !d_hit_i || !d_hit_j || !d_hit_v || !d_hit_n || !d_hit_stat || !d_counts)
        return fail("jxg_pairscreen_scan_p32: operand or hit buffers missing");
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), st));
    if (nrows < 2) return 0;
    const int nblocks = (nrows + 15) / 16;
    const int64_t tiles = (int64_t)nblocks * (nblocks + 1) / 2;
    hipLaunchKernelGGL(ps_scan_kernel, dim3((unsigned)((tiles + PS_WAVES - 1) / PS_WAVES)), dim3(PS_WAVES * 64), 0, st, d_p32, m_total,
                       num_tiles(n), d_rows, nrows, nblocks, d_flip, d_chrom, reinterpret_cast<const long long *>(d_pos),
                       (long long)min_dist, d_planes, plane_stride, scale, sigma2, d_variants, nvariants, t_min,
                       (unsigned long long)capacity, d_hit_i, d_hit_j, d_hit_v, d_hit_n, d_hit_stat,
                       reinterpret_cast<unsigned long long *>(d_counts));
    JX_LAUNCH_CHECK();
    return 0;
}
