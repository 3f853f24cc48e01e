// Shared pieces of the int8-MFMA kernels that keep [k = SNP][position] byte images of a P32 panel in LDS (k_grm_i8.hip, k_king.hip).
#pragma once
#include "jx_common.h"

namespace jx {

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// position inside a tile -> sample inside the tile (involution: 4 x 4 transposition inside every group of 16)
__device__ __forceinline__ int pos_to_sample(int p) { return (p & ~15) | ((p & 3) << 2) | ((p >> 2) & 3); }

// MFMA operand of this lane (16 consecutive k of one position) from a [k][position] byte image: two transposed reads.
// `lane_base` = image + (k0 + 16 (lane >> 5) + ((lane & 15) >> 1)) * PITCH + pos0 + 16 ((lane >> 4) & 1) + 8 (lane & 1).
template <int PITCH>
__device__ __forceinline__ i32x4 tr8_frag(const uint8_t *lane_base) {
    typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
    const i32x2 a = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2 *)(lane_base));
    const i32x2 b = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2 *)(lane_base + 8 * PITCH));
    i32x4 r;
    r.x = a.x;
    r.y = a.y;
    r.z = b.x;
    r.w = b.y;
    return r;
}

}  // namespace jx
