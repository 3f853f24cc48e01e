// KING robust kinship (Manichaikul et al. 2010) of all sample pairs of a P32 image on the int8 matrix pipes: `jx grm -king`.
// Behaviour: src/math/KING.rs (`king_related_pairs_from_bitplanes` :430-528, `king_stats_from_counts` :217-243) over the pair
// counts of `king_pair_counts_serial` (src/math/bitwise.rs:259-300, fields of `KingBitCounts` :127-135).
//
// With Z / H / A the indicators of the codes 00 (hom-ref) / 10 (het) / 11 (hom-alt) of a sample over the SNP rows and N = Z + H + A
// (called; 01 = missing and the pad samples of the last tile count nowhere), every pair count is an integer Gram over the SNP axis:
//     shared = N_i N_j   ibs0 = Z_i A_j + A_i Z_j   same_hom = Z_i Z_j + A_i A_j   both_het = H_i H_j   het_i = H_i N_j   het_j = N_i H_j
// and kinship = (both_het - 2 ibs0) / (het_i + het_j) in f64, NaN when the denominator is 0.
//
// Design (gfx950):
//  * the LDS images are the [k = SNP][position] byte images of i8_tile.h (its pitch, its 4 x 4 position order inside a 16-sample
//    group, its transposed fragment reads), but the byte is the raw 2-bit CODE (0..3), not a value: one image per
//    side serves every indicator.  A lane turns its fragment (16 code bytes of one position) into an indicator operand with four
//    v_perm_b32 against a compile-time byte LUT, in registers, right in front of the MFMAs that consume it.  Decoding into four
//    indicator images per side instead would cost four times the LDS writes and four times the fragment reads, and the fragment
//    reads are what a 128 x 128 tile with three accumulator sets is short of;
//  * fused form (`jxg_king_related_p32`): lower-triangle tiles, three i32 accumulator sets (ibs0, both_het, het_i + het_j) fed by
//    five v_mfma_i32_32x32x32_i8 passes per k-step (Z A + A Z; H H; H N + N H: the per-side LUT is free), then the kinship and the
//    threshold in the epilogue: a wave counts its rows with a ballot, its first active lane takes that many slots from one 64-bit
//    device counter, and every row whose slot lies below the caller's capacity is written.  The counter ends at the true total:
//    the host runs again with a larger buffer when it exceeds the capacity.  No n x n matrix exists at any point;
//  * counts form (`jxg_king_counts_p32`): six accumulator sets, eight passes, a rectangular range of 64 x 64 tiles, for
//    `king_pair_stats` and tests;
//  * rows beyond the last SNP and tiles beyond the panel are masked to the code 01 (missing) - NOT to 00 as in the count Gram,
//    where 00 has the value 0: here N(00) = Z(00) = 1;
//  * no split over the SNP axis: the threshold needs whole sums.  A small panel (a few tiles) leaves most of the chip idle.
// An indicator product adds at most 1 per SNP and the sum of two at most 2: i32 is exact for 2^29 rows and more are refused.
#include <stdlib.h>

#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

constexpr int64_t KING_MAX_ROWS = (int64_t)1 << 29;
constexpr int KING_BK = 64;                        // SNP rows per step of every form

// byte c of a LUT = value of the 2-bit code c (0 = 00 hom-ref, 1 = 01 missing, 2 = 10 het, 3 = 11 hom-alt)
constexpr uint32_t KG_Z = 0x00000001u, KG_H = 0x00010000u, KG_A = 0x01000000u, KG_N = 0x01010001u;

#define KG_MFMA(a, b, c) c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0)

// TM x TM tile per workgroup of (TM / WT)^2 waves, each WT x WT.  COUNTS = false: tile blockIdx.x of the lower triangle, fused
// epilogue.  COUNTS = true: tile (ti0 + blockIdx.y, tj0 + blockIdx.x), the six sums of the pairs inside [i0, i1) x [j0, j1).
template <int TM, int WT, bool COUNTS>
__global__ __launch_bounds__(64 * (TM / WT) * (TM / WT), 2) void king_kernel(
    const uint8_t *__restrict__ p32, int64_t m, int n, int nt128, double threshold, unsigned long long cap, uint32_t *__restrict__ out_i,
    uint32_t *__restrict__ out_j, uint32_t *__restrict__ out_ibs0, double *__restrict__ out_kin, unsigned long long *__restrict__ counter,
    int ti0, int tj0, int i0, int i1, int j0, int j1, int32_t *__restrict__ counts) {
    constexpr int BK = KING_BK;
    constexpr int NW = TM / WT;
    constexpr int NTHREADS = 64 * NW * NW;
    constexpr int FI = WT / 32;                    // 32 x 32 MFMA tiles per side of a wave
    constexpr int NACC = COUNTS ? 6 : 3;
    using Reader = PanelReader<TM, BK, NTHREADS, P32_ALL_MISSING>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[Reader::SET];

    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / NW, wn = wave % NW;

    int ti, tj;
    if constexpr (COUNTS) {
        ti = ti0 + (int)blockIdx.y;
        tj = tj0 + (int)blockIdx.x;
    } else {
        JX_TRI_TILE(blockIdx.x, ti, tj);              // lower-triangle tile (ti >= tj)
    }

    const Reader rd(p32, m, nt128, ti, tj);
    constexpr int NL = Reader::NL, PITCH = Reader::PITCH, IMG = Reader::IMG;
    uint32_t wA[NL], wB[NL];                       // payload dwords, loaded one step ahead of their use
    auto load_payload = [&](int u, int64_t kbase) { rd.load(rd.row(u, kbase, m), wA[u], wB[u]); };
    auto store_codes = [&](int u, int64_t kbase) { rd.store(smem, u, kbase, m, wA[u], wB[u], [](uint32_t w) { return codes16(w); }); };

    i32x16 c[NACC][FI][FI];
#pragma unroll
    for (int p = 0; p < NACC; ++p)
#pragma unroll
        for (int a = 0; a < FI; ++a)
#pragma unroll
            for (int b = 0; b < FI; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) c[p][a][b][r] = 0;

    const int lane_off = frag_lane_off<PITCH>(lane, h);
    auto mfma_ks = [&](int ks) {
        const uint8_t *sA = smem + lane_off + wm * WT + ks * 32 * PITCH, *sB = smem + IMG + lane_off + wn * WT + ks * 32 * PITCH;
        i32x4 ca[FI], cb[FI];
#pragma unroll
        for (int a = 0; a < FI; ++a) ca[a] = tr8_frag<PITCH>(sA + a * 32);
#pragma unroll
        for (int b = 0; b < FI; ++b) cb[b] = tr8_frag<PITCH>(sB + b * 32);
        i32x4 zb[FI], hb[FI], ab[FI], nb[FI];
#pragma unroll
        for (int b = 0; b < FI; ++b) {
            zb[b] = lut_frag<KG_Z>(cb[b]);
            hb[b] = lut_frag<KG_H>(cb[b]);
            ab[b] = lut_frag<KG_A>(cb[b]);
            nb[b] = lut_frag<KG_N>(cb[b]);
        }
#pragma unroll
        for (int a = 0; a < FI; ++a) {
            const i32x4 za = lut_frag<KG_Z>(ca[a]), ha = lut_frag<KG_H>(ca[a]), aa = lut_frag<KG_A>(ca[a]), na = lut_frag<KG_N>(ca[a]);
#pragma unroll
            for (int b = 0; b < FI; ++b) {
                if constexpr (COUNTS) {            // plane order: the fields of KingBitCounts
                    KG_MFMA(na, nb[b], c[0][a][b]);
                    KG_MFMA(za, ab[b], c[1][a][b]);
                    KG_MFMA(aa, zb[b], c[1][a][b]);
                    KG_MFMA(za, zb[b], c[2][a][b]);
                    KG_MFMA(aa, ab[b], c[2][a][b]);
                    KG_MFMA(ha, hb[b], c[3][a][b]);
                    KG_MFMA(ha, nb[b], c[NACC - 2][a][b]);
                    KG_MFMA(na, hb[b], c[NACC - 1][a][b]);
                } else {                           // 0 ibs0, 1 both_het, 2 het_i + het_j
                    KG_MFMA(za, ab[b], c[0][a][b]);
                    KG_MFMA(aa, zb[b], c[0][a][b]);
                    KG_MFMA(ha, hb[b], c[1][a][b]);
                    KG_MFMA(ha, nb[b], c[2][a][b]);
                    KG_MFMA(na, hb[b], c[2][a][b]);
                }
            }
        }
    };

    // several workgroups per CU: other workgroups' MFMAs cover this one's stores and barriers
#pragma unroll
    for (int u = 0; u < NL; ++u) load_payload(u, 0);
    for (int64_t kbase = 0; kbase < m; kbase += BK) {
#pragma unroll
        for (int u = 0; u < NL; ++u) store_codes(u, kbase);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NL; ++u) load_payload(u, kbase + BK);
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) mfma_ks(ks);
        __syncthreads();
    }

    // the accumulators hold tile POSITIONS (cd_row, cd_col)
#pragma unroll
    for (int a = 0; a < FI; ++a)
#pragma unroll
        for (int b = 0; b < FI; ++b) {
            const int64_t gj = (int64_t)tj * TM + pos_to_sample(wn * WT + b * 32 + cd_col(lane));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gi = (int64_t)ti * TM + pos_to_sample(cd_row(r, h, wm * WT + a * 32));
                if constexpr (COUNTS) {
                    if (gi >= i0 && gi < i1 && gj >= j0 && gj < j1) {
                        const int64_t ni = i1 - i0, nj = j1 - j0, o = (gi - i0) * nj + (gj - j0);
#pragma unroll
                        for (int p = 0; p < NACC; ++p) counts[(int64_t)p * ni * nj + o] = c[p][a][b][r];
                    }
                } else {
                    // pair (sample_i = gj) < (sample_j = gi): diagonal tiles drop gi <= gj, pad samples lie at or beyond n
                    const int ibs0 = c[0][a][b][r], hh = c[1][a][b][r], den = c[2][a][b][r];
                    double kin = 0.0;
                    bool hit = false;
                    if (gi < n && gj < gi && den > 0) {
                        kin = ((double)hh - 2.0 * (double)ibs0) / (double)den;
                        hit = kin >= threshold;
                    }
                    wave_append(hit, counter, cap, [&](unsigned long long slot) {
                        out_i[slot] = (uint32_t)gj;
                        out_j[slot] = (uint32_t)gi;
                        out_ibs0[slot] = (uint32_t)ibs0;
                        out_kin[slot] = kin;
                    });
                }
            }
        }
}

static int king_check(const char *who, int64_t m, int n) {
    if (n <= 0) return fail(std::string(who) + ": n must be > 0");
    if (m <= 0) return fail(std::string(who) + ": no rows");
    if (m > KING_MAX_ROWS) return fail(std::string(who) + ": at most 536 870 912 rows (exact i32 pair sums)");
    return 0;
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_king_related_p32(const uint8_t *d_p32, int64_t m, int n, double kinship_threshold, int64_t capacity, uint32_t *d_i,
                                    uint32_t *d_j, uint32_t *d_ibs0, double *d_kinship, uint64_t *d_count, void *stream) {
    if (king_check("jxg_king_related_p32", m, n)) return 1;
    if (!(kinship_threshold - kinship_threshold == 0.0)) return fail("KING kinship_threshold must be finite");
    if (capacity < 0) return fail("jxg_king_related_p32: negative capacity");
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    const int nt128 = num_tiles(n);
    // JXGPU_KING_TILE = 64 / 128 forces a tile shape.  128 x 128 (64 x 64 per wave) halves the fragment reads and code stores per
    // MFMA; 64 x 64 quadruples the workgroups of a panel whose 128-tiles would not fill the chip twice over.
    const int tile_env = getenv("JXGPU_KING_TILE") ? atoi(getenv("JXGPU_KING_TILE")) : 0;
    if (tile_env != 0 && tile_env != 64 && tile_env != 128) return fail("JXGPU_KING_TILE must be 64 or 128");
    const int64_t tiles128 = (int64_t)nt128 * (nt128 + 1) / 2;
    const bool big = tile_env ? tile_env == 128 : tiles128 >= 4 * 256;
    const int64_t nt = big ? nt128 : ((int64_t)n + 63) / 64;
    const int64_t ntiles = nt * (nt + 1) / 2;
    if (ntiles > 0x7fffffffLL) return fail("jxg_king_related_p32: too many tiles");
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(d_count);
    if (big)
        hipLaunchKernelGGL((king_kernel<128, 64, false>), dim3((unsigned)ntiles), dim3(256), 0, st, d_p32, m, n, nt128, kinship_threshold,
                           (unsigned long long)capacity, d_i, d_j, d_ibs0, d_kinship, cnt, 0, 0, 0, 0, 0, 0, (int32_t *)nullptr);
    else
        hipLaunchKernelGGL((king_kernel<64, 32, false>), dim3((unsigned)ntiles), dim3(256), 0, st, d_p32, m, n, nt128, kinship_threshold,
                           (unsigned long long)capacity, d_i, d_j, d_ibs0, d_kinship, cnt, 0, 0, 0, 0, 0, 0, (int32_t *)nullptr);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_king_counts_p32(const uint8_t *d_p32, int64_t m, int n, int i0, int i1, int j0, int j1, int32_t *d_counts,
                                   void *stream) {
    if (king_check("jxg_king_counts_p32", m, n)) return 1;
    if (i0 < 0 || i1 < i0 || i1 > n || j0 < 0 || j1 < j0 || j1 > n) return fail("jxg_king_counts_p32: block outside the samples");
    if (i1 == i0 || j1 == j0) return 0;
    const int ti0 = i0 / 64, tj0 = j0 / 64;
    const dim3 grid((unsigned)((j1 - 1) / 64 - tj0 + 1), (unsigned)((i1 - 1) / 64 - ti0 + 1));
    if (grid.y > 65535u) return fail("jxg_king_counts_p32: at most 4 194 240 samples per block side");
    hipLaunchKernelGGL((king_kernel<64, 32, true>), grid, dim3(256), 0, (hipStream_t)stream, d_p32, m, n, num_tiles(n), 0.0, 0ull,
                       (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (double *)nullptr, (unsigned long long *)nullptr, ti0,
                       tj0, i0, i1, j0, j1, d_counts);
    JX_LAUNCH_CHECK();
    return 0;
}
