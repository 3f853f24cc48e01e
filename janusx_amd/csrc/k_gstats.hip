// Per-sample counts over the SNP axis of a P32 image, for `jx gstats -miss -het` (`accumulate_individual_row_counts`,
// src/stats/gstats.rs:180-220): for each of the n samples the number of SNP rows with code 01 (missing) and with code 10 (het).
//
// The kernel reads the image once and is bound by that read.  A record (SNP row, tile) is 32 bytes = 8 dwords of 16 two-bit
// codes, sample 16 d + k of the tile in bits 2k, 2k + 1 of dword d.  A thread owns one half record column (4 dwords = 64 samples)
// and one of the SC_LANES row lanes of its workgroup, and walks the rows of the workgroup's SNP chunk in steps of SC_LANES.  Per
// dword the two indicator planes are two bit operations on the whole dword,
//     missing = lo & ~hi,  het = hi & ~lo      (lo = w & 0x5555..., hi = (w >> 1) & 0x5555...)
// 16 one-bit flags in 2-bit fields.  They are added as whole dwords into 2-bit fields (3 rows at most), those are split into
// two dwords of 4-bit fields (15 rows at most), and those into four dwords of 8-bit fields, which hold the SC_STEPS <= 255 rows a
// thread sees in its chunk.  At the end of the chunk the byte fields go to LDS, thread o of the workgroup adds the SC_LANES bytes
// of its (plane, sample) and adds the sum to the sample's counter with one integer atomic: any order gives the same integers.
// Pad samples of the last tile are code 01 in the image; they have no counter and their sums are dropped.
#include "jx_common.h"

namespace jx {

constexpr int SC_LANES = 128;                      // row lanes of a workgroup (256 threads = 128 row lanes x 2 half records)
constexpr int SC_INNER = 3;                        // rows added into the 2-bit fields before they are widened
constexpr int SC_MID = 5;                          // widenings into the 4-bit fields before those are widened (3 x 5 = 15)
constexpr int SC_OUTER = 4;                        // widenings into the 8-bit fields (15 x 4 = 60 <= 255)
constexpr int SC_STEPS = SC_INNER * SC_MID * SC_OUTER;
constexpr int SC_CHUNK = SC_LANES * SC_STEPS;      // SNP rows per workgroup: 7680

__device__ __forceinline__ uint32_t sc_dword(const uint4 v, int d) { return d == 0 ? v.x : (d == 1 ? v.y : (d == 2 ? v.z : v.w)); }

// counts (2, n) int32, zeroed by the caller: [0] missing, [1] het.  grid (x: SNP chunks, y: tiles)
__global__ __launch_bounds__(256) void sample_counts_kernel(const uint8_t *__restrict__ p32, int64_t m, int n,
                                                            int32_t *__restrict__ counts) {
    __shared__ uint32_t lds[SC_LANES * 2 * 32];    // [row lane][half][plane 2][dword 4][byte-field register 4]
    const int half = threadIdx.x & 1, rl = threadIdx.x >> 1;
    const int64_t tile = blockIdx.y, row0 = (int64_t)blockIdx.x * SC_CHUNK + rl;
    const uint8_t *base = p32 + tile * m * 32 + 16 * half;
    uint32_t a8[2][4][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) a8[p][d][q] = 0u;
    for (int o = 0; o < SC_OUTER; ++o) {
        uint32_t a4[2][4][2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d) a4[p][d][0] = a4[p][d][1] = 0u;
#pragma unroll
        for (int k = 0; k < SC_MID; ++k) {
            uint4 w[SC_INNER];
#pragma unroll
            for (int e = 0; e < SC_INNER; ++e) {
                const int64_t row = row0 + (int64_t)((o * SC_MID + k) * SC_INNER + e) * SC_LANES;
                w[e] = row < m ? *reinterpret_cast<const uint4 *>(base + row * 32) : uint4{0u, 0u, 0u, 0u};   // 00: counts nothing
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t miss = 0u, het = 0u;                  // 2-bit fields, <= 3
#pragma unroll
                for (int e = 0; e < SC_INNER; ++e) {
                    const uint32_t v = sc_dword(w[e], d), lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
                    miss += lo & ~hi;
                    het += hi & ~lo;
                }
                a4[0][d][0] += miss & 0x33333333u;             // samples 0, 2, .. 14 of the dword in 4-bit fields, <= 15
                a4[0][d][1] += (miss >> 2) & 0x33333333u;      // samples 1, 3, .. 15
                a4[1][d][0] += het & 0x33333333u;
                a4[1][d][1] += (het >> 2) & 0x33333333u;
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int h = 0; h < 2; ++h) {                  // 8-bit fields, <= 60: register 2 c + h, byte b = sample 4 b + 2 c + h
                    a8[p][d][h] += a4[p][d][h] & 0x0f0f0f0fu;
                    a8[p][d][2 + h] += (a4[p][d][h] >> 4) & 0x0f0f0f0fu;
                }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) lds[((rl * 2 + half) * 2 + p) * 16 + d * 4 + q] = a8[p][d][q];
    __syncthreads();
    // thread o: plane o >> 7, sample s = o & 127 of the tile: half s >> 6, dword (s >> 4) & 3, k = s & 15 = 4 b + 2 c + h
    const int p = threadIdx.x >> 7, s = threadIdx.x & 127, k = s & 15;
    const int word = (((s >> 6) * 2 + p) * 16) + ((s >> 4) & 3) * 4 + (((k >> 1) & 1) * 2 + (k & 1)), shift = 8 * (k >> 2);
    uint32_t sum = 0u;
    for (int l = 0; l < SC_LANES; ++l) sum += (lds[l * 64 + word] >> shift) & 0xffu;
    const int64_t sample = tile * JXG_TILE + s;
    if (sample < n && sum) atomicAdd(counts + (int64_t)p * n + sample, (int)sum);
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_sample_counts_p32(const uint8_t *d_p32, int64_t m, int n, int32_t *d_counts, void *stream) {
    if (n <= 0) return fail("jxg_sample_counts_p32: n must be > 0");
    if (m <= 0) return fail("jxg_sample_counts_p32: no rows");
    if (m > 0x7fffffffLL) return fail("jxg_sample_counts_p32: at most 2 147 483 647 rows (int32 counts)");
    hipStream_t st = (hipStream_t)stream;
    JX_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * 2 * (size_t)n, st));
    const int64_t chunks = (m + SC_CHUNK - 1) / SC_CHUNK;
    const int nt = num_tiles(n);
    if (nt > 65535) return fail("jxg_sample_counts_p32: at most 8 388 480 samples");
    hipLaunchKernelGGL(sample_counts_kernel, dim3((unsigned)chunks, (unsigned)nt), dim3(256), 0, st, d_p32, m, n, d_counts);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int jxg_sample_counts_chunk(void) { return SC_CHUNK; }
