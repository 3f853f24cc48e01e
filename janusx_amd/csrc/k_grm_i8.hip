// Exact-integer GRM Gram term on the int8 matrix pipes: acc(lower tiles) += C C^T, C = allele counts {0,1,2} decoded on the
// fly from the 2-bit P32 payload.
//
// Reference path being replaced: decode_additive_grm_block_f32 (src/decode/decode.rs:728-886) -> cblas_ssyrk per SNP block
// -> f64 merge (src/stats/grm.rs:1638-1667, 1700-1772).  With method 1 the design row of a SNP without missing calls among
// the selected samples is z_ij = b_j + s_j c_ij (c = count of the payload's second allele, s_j = -1 when the reference
// flips the SNP, b_j the centring term), so
//     sum_j z_ij z_kj = sum_j c_ij c_kj + r_i + r_k + B,   r = C (b .* s),   B = sum_j b_j^2
// (s_j^2 = 1: the Gram term does not see the flips).  The Gram term has operands in {0,1,2} and integer sums: it runs on
// v_mfma_i32_32x32x32_i8 (twice the f16 rate, one byte per operand element, exact for 2^29 SNPs per chunk) and the affine
// terms are one f64 matrix-vector product over the payload (jxg_packed_dot), added in the first chunk's merge.
//
// Design (gfx950):
//  * decode is pure VALU, 11 instructions per payload dword (16 samples): `counts16` of i8_tile.h (code 00 -> 0, 10 -> 1,
//    11 -> 2, 01 = missing / pad -> 0).  No table lookups, no per-SNP value LUT, no flips.  i8_tile.h defines the byte order inside
//    a 16-group, `pos_to_sample` that undoes it once in the merge, the LDS images ([k = SNP][position], one BYTE per element: half
//    the LDS traffic of the fp16 images, one ds_write_b128 per payload dword), their pitch, the masking of rows beyond the chunk
//    and tiles beyond the panel, and the transposed fragment reads (two ds_read_b64_tr_b8 per MFMA operand);
//  * large n: 256 x 256 output tile per 512-thread workgroup (8 waves of 128 x 64), one workgroup per CU, two image sets:
//    the decode of step k + 1 shares a barrier interval with the MFMAs of step k (decode bytes and fragment reads per
//    MFMA are half those of a 128 x 128 tile); few tiles / row panels: 128 x 128 per 256-thread workgroup, 4 per CU.
#include <stdlib.h>

#include <algorithm>

#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

// LUT = true: the operand bytes come from a per-SNP byte LUT `luts[k]` (byte c = value of the 2-bit code c; k = position in the
// row list) instead of the counts {0, 0, 1, 2}, and the i32 Gram is scaled by `gscale` in the merge: the two-Gram form of rows
// with missing calls (k_grm.hip, "dense missing-call path").
template <int TM, int TN, int WM, int WN, int BK, bool DBUF, int MINW, bool LUT = false>
__global__ __launch_bounds__(64 * (TM / WM) * (TN / WN), MINW) void grm_i8_kernel(
    const uint8_t *__restrict__ p32, int64_t m_total, const int32_t *__restrict__ rows, int64_t k_begin, int64_t k_end,
    int64_t kchunk, int nt128, double *__restrict__ acc, int64_t ld, int use_atomic, const double *__restrict__ corr,
    int tile_base, const uint32_t *__restrict__ luts, double gscale) {
    static_assert(TM == TN, "square workgroup tiles");
    constexpr int NWN = TN / WN;
    constexpr int NTHREADS = 64 * (TM / WM) * NWN;
    constexpr int MI = WM / 32, NI = WN / 32;
    using Reader = PanelReader<TM, BK, NTHREADS, 0u>;   // fill 0: code 00 = count 0 = byte 0 of a LUT, masked rows / tiles vanish
    constexpr int PITCH = Reader::PITCH, IMG = Reader::IMG, SET = Reader::SET, NL = Reader::NL;
    __shared__ __attribute__((aligned(16))) uint8_t smem[(DBUF ? 2 : 1) * SET];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;

    int ti, tj;                                    // lower-triangle tile (ti >= tj) of TM x TM blocks
    JX_TRI_TILE(blockIdx.x + tile_base, ti, tj);

    const int64_t k0 = k_begin + (int64_t)blockIdx.y * kchunk;
    const int64_t k1 = (k0 + kchunk < k_end) ? (k0 + kchunk) : k_end;

    const Reader rd(p32, m_total, nt128, ti, tj);
    int32_t rec[NL];                               // payload record (SNP row), loaded two steps ahead of its payload's use
    uint32_t lutn[NL], lutw[NL];                   // LUT: the SNP's byte LUT, travelling with rec (lutn) and with the payload (lutw)
    uint32_t wA[NL], wB[NL];                       // payload dwords, loaded one step ahead of their decode
    auto load_rec = [&](int u, int64_t kbase) {
        const int64_t k = rd.row(u, kbase, k1);
        rec[u] = rows[k];
        if constexpr (LUT) lutn[u] = luts[k];
    };
    auto load_payload = [&](int u) {               // consumes rec[u]
        rd.load(rec[u], wA[u], wB[u]);
        if constexpr (LUT) lutw[u] = lutn[u];
    };
    auto decode_to = [&](uint8_t *base, int u, int64_t kbase) {     // payload of the step that starts at kbase
        if constexpr (LUT) {
            rd.store(base, u, kbase, k1, wA[u], wB[u], [&](uint32_t w) { return lut16(w, lutw[u]); });
        } else {
            rd.store(base, u, kbase, k1, wA[u], wB[u], [](uint32_t w) { return counts16(w); });
        }
    };

    i32x16 c[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) c[mi][ni][r] = 0;

    const int h = lane >> 5;
    const int lane_off = frag_lane_off<PITCH>(lane, h);
    auto mfma_ks = [&](const uint8_t *base, int ks) {
        const uint8_t *sA = base + lane_off + wm * WM + ks * 32 * PITCH, *sB = base + IMG + lane_off + wn * WN + ks * 32 * PITCH;
        i32x4 a[MI], b[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) a[mi] = tr8_frag<PITCH>(sA + mi * 32);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) b[ni] = tr8_frag<PITCH>(sB + ni * 32);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                c[mi][ni] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[mi], b[ni], c[mi][ni], 0, 0, 0);
    };

    constexpr int KS = BK / 32;
#pragma unroll
    for (int u = 0; u < NL; ++u) load_rec(u, k0);
#pragma unroll
    for (int u = 0; u < NL; ++u) load_payload(u);
#pragma unroll
    for (int u = 0; u < NL; ++u) load_rec(u, k0 + BK);
    if constexpr (!DBUF) {
        // 4 workgroups per CU: other workgroups' MFMAs cover this one's decode
        for (int64_t kbase = k0; kbase < k1; kbase += BK) {
#pragma unroll
            for (int u = 0; u < NL; ++u) decode_to(smem, u, kbase);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NL; ++u) {
                load_payload(u);                   // step kbase + BK
                load_rec(u, kbase + 2 * BK);
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mfma_ks(smem, ks);
            __syncthreads();
        }
    } else {
        static_assert(!DBUF || NL % KS == 0 || KS % NL == 0, "decode pieces per k-step");
#pragma unroll
        for (int u = 0; u < NL; ++u) decode_to(smem, u, k0);
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            load_payload(u);
            load_rec(u, k0 + 2 * BK);
        }
        __syncthreads();
        int cur = 0;
        for (int64_t kbase = k0; kbase < k1; kbase += BK) {
            // one barrier interval: the MFMAs of this step from image set `cur`, the decode of the next step into the other
            // set, piece by piece between the k-steps (VALU and LDS writes ride in the MFMA issue gaps), and behind every
            // decoded piece the loads that refill its registers for the step after
            const uint8_t *rd = smem + cur * SET;
            uint8_t *wr = smem + (cur ^ 1) * SET;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                mfma_ks(rd, ks);
#pragma unroll
                for (int u = ks * NL / KS; u < (ks + 1) * NL / KS; ++u) {
                    decode_to(wr, u, kbase + BK);
                    load_payload(u);               // step kbase + 2 BK (rec loaded during the previous step)
                    load_rec(u, kbase + 3 * BK);
                }
                // keep every piece's loads in its own k-step: sunk to the end of the iteration (what the scheduler does
                // otherwise) they have a quarter of a step instead of a whole one to land before their decode
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    // f64 merge.  The accumulators hold tile POSITIONS (cd_row, cd_col), mapped to samples by pos_to_sample.
    const bool add_corr = corr != nullptr && k0 == k_begin;
    const double corr_b = add_corr ? corr[ld] : 0.0;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int64_t gj = (int64_t)tj * TN + pos_to_sample(wn * WN + ni * 32 + cd_col(lane));
            const double corr_j = (add_corr && gj < ld) ? corr[gj] + corr_b : 0.0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t gi = (int64_t)ti * TM + pos_to_sample(cd_row(r, h, wm * WM + mi * 32));
                if (gi < ld && gj < ld) {
                    double *dst = acc + gi * ld + gj;
                    double v = (double)c[mi][ni][r];
                    if constexpr (LUT) v *= gscale;
                    if (add_corr) v += corr[gi] + corr_j;
                    if (use_atomic) {
                        unsafeAtomicAdd(dst, v);
                    } else {
                        *dst += v;
                    }
                }
            }
        }
}

// k_grm_fp4.hip: the same Gram on the fp4 pipes from a nibble image of the counts
bool grm_fp4_enabled();
int launch_grm_fp4(hipStream_t st, const uint8_t *p32, int64_t m_total, const int32_t *rows, int64_t r0, int64_t r1, int nt128,
                   double *d_acc, int64_t ld, const double *corr, int64_t base256, int64_t ntl256);

// Launch over the SNP range [r0, r1) of the (reordered) list `rows`.  Lower-triangle tiles of the n_sel x n_sel accumulator
// (ld = 128 nt128); panel mode: tile rows [tile_row_begin, tile_row_end) of 128-row tiles only (d_acc already shifted so
// that global sample rows index it).  `corr`: r[0 .. ld) and B at [ld], added once.
int launch_grm_i8(hipStream_t st, const uint8_t *p32, int64_t m_total, const int32_t *rows, int64_t r0, int64_t r1, int nt128,
                  double *d_acc, int64_t ld, const double *corr, bool panel, int tile_row_begin, int tile_row_end) {
    const int64_t cnt = r1 - r0;
    if (cnt <= 0) return 0;
    if (!rows) return fail("launch_grm_i8: the SNP row list is required");
    const int tile_env = getenv("JXGPU_GRM_I8_TILE") ? atoi(getenv("JXGPU_GRM_I8_TILE")) : 0;   // 256 / 128 force a tile shape
    const int nt256 = (nt128 + 1) / 2;
    // 256 x 256 tiles (one workgroup per CU) once they fill the chip a few times over; row panels (tile rows counted in
    // 128-row units) take them when the panel starts on a 256-row boundary: rows [begin / 2, ceil(end / 2)) of the 256-tile
    // triangle (a trailing half tile is masked by the kernel's row guards)
    const int pb256 = panel ? tile_row_begin / 2 : 0, pe256 = panel ? (tile_row_end + 1) / 2 : nt256;
    const int64_t base256 = (int64_t)pb256 * (pb256 + 1) / 2;
    const int64_t ntl256 = (int64_t)pe256 * (pe256 + 1) / 2 - base256;
    const bool big = (!panel || (tile_row_begin % 2 == 0 && (tile_row_end % 2 == 0 || tile_row_end == nt128))) &&
                     (tile_env ? tile_env >= 256 : ntl256 >= 3 * 256);
    if (big) {
        if (base256 + ntl256 > 0x7fffffffLL) return fail("jxg_grm_accumulate: too many tiles");
        if (grm_fp4_enabled()) return launch_grm_fp4(st, p32, m_total, rows, r0, r1, nt128, d_acc, ld, corr, base256, ntl256);
        // i32 sums stay exact for 2^29 SNPs per chunk: one launch for the whole range
        for (int64_t kb = r0; kb < r1; kb += (int64_t)1 << 29) {
            const int64_t ke = (kb + ((int64_t)1 << 29) < r1) ? kb + ((int64_t)1 << 29) : r1;
            hipLaunchKernelGGL((grm_i8_kernel<256, 256, 128, 64, 128, true, 2>), dim3((unsigned)ntl256, 1), dim3(512), 0, st,
                               p32, m_total, rows, kb, ke, (int64_t)1 << 29, nt128, d_acc, ld, 0, kb == r0 ? corr : nullptr,
                               (int)base256, (const uint32_t *)nullptr, 1.0);
            JX_LAUNCH_CHECK();
        }
        return 0;
    }
    const int64_t tile_base = panel ? (int64_t)tile_row_begin * (tile_row_begin + 1) / 2 : 0;
    const int64_t ntiles = panel ? (int64_t)tile_row_end * (tile_row_end + 1) / 2 - tile_base : (int64_t)nt128 * (nt128 + 1) / 2;
    if (tile_base + ntiles > 0x7fffffffLL) return fail("jxg_grm_accumulate: too many tiles");
    const int64_t slots = 4 * 256;                 // resident workgroups on 256 CUs
    if (ntiles < 2 * slots && cnt > 4096) {
        // few tiles: SNP chunks over blockIdx.y, f64 atomics (the i32 partial sums are exact, the f64 adds commute up to
        // rounding of the affine terms only)
        int64_t want = (2 * slots + ntiles - 1) / ntiles;
        int64_t kc = (cnt + want - 1) / want;
        kc = ((kc + 63) / 64) * 64;
        if (kc < 2048) kc = 2048;
        const int64_t ny = (cnt + kc - 1) / kc;
        if (ny > 65535) return fail("jxg_grm_accumulate: too many chunks");
        hipLaunchKernelGGL((grm_i8_kernel<128, 128, 64, 64, 64, false, 4>), dim3((unsigned)ntiles, (unsigned)ny), dim3(256), 0,
                           st, p32, m_total, rows, r0, r1, kc, nt128, d_acc, ld, 1, corr, (int)tile_base, (const uint32_t *)nullptr, 1.0);
        JX_LAUNCH_CHECK();
        return 0;
    }
    for (int64_t kb = r0; kb < r1; kb += (int64_t)1 << 29) {
        const int64_t ke = (kb + ((int64_t)1 << 29) < r1) ? kb + ((int64_t)1 << 29) : r1;
        hipLaunchKernelGGL((grm_i8_kernel<128, 128, 64, 64, 64, false, 4>), dim3((unsigned)ntiles, 1), dim3(256), 0, st, p32,
                           m_total, rows, kb, ke, (int64_t)1 << 29, nt128, d_acc, ld, 0, kb == r0 ? corr : nullptr,
                           (int)tile_base, (const uint32_t *)nullptr, 1.0);
        JX_LAUNCH_CHECK();
    }
    return 0;
}

// The same Gram with the operand bytes taken from the per-SNP LUTs `luts` (positions r0 .. r1 of the list) and the i32 sums
// scaled by `gscale`: whole lower triangle only (no row panels).  |byte| <= 127, so the i32 sums are exact for 2^31 / 127^2 SNPs:
// chunks of 131072.
int launch_grm_i8_lut(hipStream_t st, const uint8_t *p32, int64_t m_total, const int32_t *rows, const uint32_t *luts, int64_t r0,
                      int64_t r1, int nt128, double *d_acc, int64_t ld, const double *corr, double gscale) {
    if (r1 <= r0) return 0;
    const int nt256 = (nt128 + 1) / 2;
    const int64_t ntl256 = (int64_t)nt256 * (nt256 + 1) / 2;
    const int64_t ntiles = (int64_t)nt128 * (nt128 + 1) / 2;
    if (ntiles > 0x7fffffffLL) return fail("jxg_grm_accumulate: too many tiles");
    const int64_t kc = 131072;
    const int tile_env = getenv("JXGPU_GRM_I8_TILE") ? atoi(getenv("JXGPU_GRM_I8_TILE")) : 0;   // 256 / 128 force a tile shape, as in launch_grm_i8
    const bool big = tile_env ? tile_env >= 256 : ntl256 >= 3 * 256;
    for (int64_t kb = r0; kb < r1; kb += kc) {
        const int64_t ke = std::min(r1, kb + kc);
        if (big)
            hipLaunchKernelGGL((grm_i8_kernel<256, 256, 128, 64, 128, true, 2, true>), dim3((unsigned)ntl256, 1), dim3(512), 0, st,
                               p32, m_total, rows, kb, ke, kc, nt128, d_acc, ld, 0, kb == r0 ? corr : nullptr, 0, luts, gscale);
        else
            hipLaunchKernelGGL((grm_i8_kernel<128, 128, 64, 64, 64, false, 4, true>), dim3((unsigned)ntiles, 1), dim3(256), 0, st,
                               p32, m_total, rows, kb, ke, kc, nt128, d_acc, ld, 0, kb == r0 ? corr : nullptr, 0, luts, gscale);
        JX_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace jx
