// The front end of the P32 image for the matrix pipes: the ONE place that defines
//   * the 2-bit code table and the byte order of a decoded 16-sample group (`spread16`, the decoders, `pos_to_sample`),
//   * the [k = SNP][position] LDS image of a panel, its pitch (`PanelGeom`), the clamped loads and the masking fill (`PanelReader`),
//   * the fragment lane map of the transposed reads and the C/D map of the 32 x 32 shapes (`frag_lane_off`, `tr8_frag`, `cd_row`),
//   * the lower-triangle tile index (`JX_TRI_TILE`), the wave-ballot append (`wave_append`) and the register vector types.
// Users: k_grm_i8, k_grm_fp4, k_king, k_tree (panel images); k_rotate_i8, k_lm_traits, k_ld, k_pcg_i8, k_rsvd (decoders);
// k_grm (JX_TRI_TILE, cd_row), k_ozgemm (vector types, cd_row), k_sb2st (vector types).
#pragma once
#include "jx_common.h"

namespace jx {

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// ---- the 2-bit codes ---------------------------------------------------------------------------------------------------------
// A payload dword holds 16 samples, sample s in bits 2 s, 2 s + 1 (a "field"):
//     00 hom-ref (count 0)    01 missing    10 het (count 1)    11 hom-alt (count 2)
// P32_LO is bit 0 of every field.  Read as a payload word it is 16 codes 01: the all-missing word (`P32_ALL_MISSING`), what the
// pad samples of the last record hold.
constexpr uint32_t P32_LO = 0x55555555u;
constexpr uint32_t P32_ALL_MISSING = P32_LO;

// The byte spreader: the four 2-bit lanes of a field word as bytes, dword q = (f >> 2 q) & keep, so that byte 4 q + b of the 16
// holds sample 4 b + q.  One ds_write_b128 stores a group; no table lookups.  The sample order inside a 16-group is therefore a
// fixed 4 x 4 transposition, undone by `pos_to_sample` where positions go back to samples.  `keep` = 0x03030303 keeps a whole
// field, 0x01010101 its bit 0.
__device__ __forceinline__ u32x4v spread16(uint32_t f, uint32_t keep) {
    u32x4v o;
    o.x = f & keep;
    o.y = (f >> 2) & keep;
    o.z = (f >> 4) & keep;
    o.w = (f >> 6) & keep;
    return o;
}
constexpr uint32_t KEEP_FIELD = 0x03030303u, KEEP_BIT = 0x01010101u;

// position inside a tile -> sample inside the tile (involution: 4 x 4 transposition inside every group of 16)
__device__ __forceinline__ int pos_to_sample(int p) { return (p & ~15) | ((p & 3) << 2) | ((p >> 2) & 3); }

// field words of a payload dword, from its bit planes lo = b0 and hi = b1: the count b1 + (b0 & b1) (0, 1, 2; missing -> 0: no
// carry into the next field) and the missing-call indicator b0 & ~b1 in bit 0
__device__ __forceinline__ void count_missing_fields(uint32_t w, uint32_t &count, uint32_t &missing) {
    const uint32_t lo = w & P32_LO, hi = (w >> 1) & P32_LO;
    count = hi + (lo & hi);
    missing = lo & ~hi;
}
__device__ __forceinline__ uint32_t count_field(uint32_t w) {
    uint32_t c, e;
    count_missing_fields(w, c, e);
    return c;
}
__device__ __forceinline__ uint32_t missing_field(uint32_t w) {
    uint32_t c, e;
    count_missing_fields(w, c, e);
    return e;
}

// 16 two-bit codes -> 16 operand bytes: the raw codes (0..3), the counts, 1 at a missing call, 1 at a called sample
__device__ __forceinline__ u32x4v codes16(uint32_t w) { return spread16(w, KEEP_FIELD); }
__device__ __forceinline__ u32x4v counts16(uint32_t w) { return spread16(count_field(w), KEEP_FIELD); }
__device__ __forceinline__ u32x4v missing16(uint32_t w) { return spread16(missing_field(w), KEEP_BIT); }
__device__ __forceinline__ u32x4v called16(uint32_t w) { return spread16(((w & P32_LO) ^ P32_LO) | ((w >> 1) & P32_LO), KEEP_BIT); }
// both of one word, sharing its planes
__device__ __forceinline__ void counts_missing16(uint32_t w, i32x4 &counts, i32x4 &missing) {
    uint32_t c, e;
    count_missing_fields(w, c, e);
    counts = (i32x4)spread16(c, KEEP_FIELD);
    missing = (i32x4)spread16(e, KEEP_BIT);
}
// the bit planes b0 (`lo`), b1 (`hi`) and b0 & b1 (`both`) as 0 / 1 bytes: spread16 with KEEP_BIT of both planes, written out
// (through spread16 the int8 PCG kernels, which keep three planes of two words live, get another instruction stream)
__device__ __forceinline__ void planes16(uint32_t w, i32x4 &lo, i32x4 &hi, i32x4 &both) {
    const uint32_t l = w & P32_LO, h = (w >> 1) & P32_LO;
    lo.x = (int)(l & KEEP_BIT);
    lo.y = (int)((l >> 2) & KEEP_BIT);
    lo.z = (int)((l >> 4) & KEEP_BIT);
    lo.w = (int)((l >> 6) & KEEP_BIT);
    hi.x = (int)(h & KEEP_BIT);
    hi.y = (int)((h >> 2) & KEEP_BIT);
    hi.z = (int)((h >> 4) & KEEP_BIT);
    hi.w = (int)((h >> 6) & KEEP_BIT);
    both = lo & hi;
}

// Byte LUTs: byte c of a LUT = value of the 2-bit code c, applied with v_perm_b32 (the code bytes are the selectors).
// Run-time LUT of a SNP applied to a payload dword (the four dwords of `codes16`, each through v_perm; written out: through
// `codes16` the 256-tile LUT Gram comes out in another instruction order); compile-time LUT applied to a fragment of code bytes,
// in registers.
__device__ __forceinline__ u32x4v lut16(uint32_t w, uint32_t lut) {
    u32x4v o;
    o.x = __builtin_amdgcn_perm(lut, lut, w & KEEP_FIELD);
    o.y = __builtin_amdgcn_perm(lut, lut, (w >> 2) & KEEP_FIELD);
    o.z = __builtin_amdgcn_perm(lut, lut, (w >> 4) & KEEP_FIELD);
    o.w = __builtin_amdgcn_perm(lut, lut, (w >> 6) & KEEP_FIELD);
    return o;
}
template <uint32_t LUT>
__device__ __forceinline__ i32x4 lut_frag(const i32x4 c) {
    i32x4 o;
    o.x = (int)__builtin_amdgcn_perm(LUT, LUT, (uint32_t)c.x);
    o.y = (int)__builtin_amdgcn_perm(LUT, LUT, (uint32_t)c.y);
    o.z = (int)__builtin_amdgcn_perm(LUT, LUT, (uint32_t)c.z);
    o.w = (int)__builtin_amdgcn_perm(LUT, LUT, (uint32_t)c.w);
    return o;
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------------
// tile t of the lower triangle in row-major order -> (ti >= tj); ti, tj: int lvalues.  A macro, not a function: as a function
// its two correction loops are laid out apart from the kernel's code and the f16 GRM kernels come out with another stream.
#define JX_TRI_TILE(t, ti, tj)                                               \
    do {                                                                     \
        const int tri_t_ = (t);                                              \
        (ti) = (int)((sqrtf(8.0f * (float)tri_t_ + 1.0f) - 1.0f) * 0.5f);    \
        while ((int64_t)(ti) * ((ti) + 1) / 2 > tri_t_) --(ti);              \
        while ((int64_t)((ti) + 1) * ((ti) + 2) / 2 <= tri_t_) ++(ti);       \
        (tj) = tri_t_ - (int)((int64_t)(ti) * ((ti) + 1) / 2);               \
    } while (0)

// C/D layout of the 32 x 32 MFMA shapes: register r of a lane in half h = lane >> 5 of the wave holds row cd_row, column cd_col
// of the tile (`row0`: the tile's first row in the caller's frame).  The kernels hold h anyway: it is the k half of their fragments.
template <class T = int>
__device__ __forceinline__ T cd_row(int r, int h, T row0 = 0) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ int cd_col(int lane) { return lane & 31; }

// Fragment reads from a [k][position] byte image.  ds_read_b64_tr_b8 lane map (measured with scripts/probes/i8_probe.hip): inside
// a 16-lane group supplier lane 2 e + c provides row e, columns 8 c .. 8 c + 7, and lane i receives column i.  A lane's offset
// inside a 32-k x 32-position block of the image (h = lane >> 5, as for cd_row):
template <int PITCH>
__device__ __forceinline__ int frag_lane_off(int lane, int h) {
    return (16 * h + ((lane & 15) >> 1)) * PITCH + 16 * ((lane >> 4) & 1) + 8 * (lane & 1);
}
// MFMA operand of this lane (16 consecutive k of one position): two transposed reads.
// `lane_base` = image + k0 * PITCH + pos0 + frag_lane_off<PITCH>(lane, h).
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

// ---- append --------------------------------------------------------------------------------------------------------------------
// Every lane of the wave calls it; the lanes with `hit` get consecutive slots of one 64-bit device counter: a ballot counts them,
// the first of them takes that many slots with one atomic, the others add their rank, and `emit(slot)` runs for every hit whose
// slot lies below the caller's capacity.  The counter ends at the true total whatever the capacity.  A wave without a hit leaves
// through one uniform branch: that is why the writes are a callable and no slot is returned - writes behind a returned slot
// sit outside that branch, and the KING and statistics kernels changed.
template <class Emit>
__device__ __forceinline__ void wave_append(bool hit, unsigned long long *counter, unsigned long long cap, Emit emit) {
    const int lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(hit);
    if (bal) {                                              // wave-uniform
        const int leader = __ffsll((long long)bal) - 1;
        unsigned long long base = 0ull;
        if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(bal));
        base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), leader, 64) << 32) |
               (unsigned long long)(uint32_t)__shfl((int)(base & 0xffffffffull), leader, 64);
        const unsigned long long slot = base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
        if (hit && slot < cap) emit(slot);
    }
}

// ---- panel geometry and reader ---------------------------------------------------------------------------------------------------
// A workgroup's two panels (A = tile ti, B = tile tj of the sample axis, TM samples each) of a record image
//     [record of 128 samples][row = SNP][8 words],   word = one 16-sample group
// go BK rows at a time into two LDS images [k = SNP][position], A at `set`, B at `set + IMG`.  EBITS = 8: the P32 payload (a
// word is a dword of 2-bit codes) decoded to one byte per element, 16 bytes per group; EBITS = 4: a nibble image (a word is 8
// bytes) copied as it is.  The pitch (row + 32 B; nibbles: row + 8 B) puts the rows of a transposed read (eight rows of 8 bytes;
// nibbles: sixteen) on disjoint banks.
//
// Word idx = tid + u NTHREADS of a step, u < NL, is (SNP kk_of + u KSTRIDE = idx / DW of the step, group d_of = idx % DW of the
// panel row); both panels use the same (kk, d), so one row index per u serves both.  Group ti DW + d of the sample axis lies in
// record (ti DW + d) / 8 at word (ti DW + d) % 8.
template <int TM, int BK, int NTHREADS, int EBITS = 8>
struct PanelGeom {
    static_assert(EBITS == 8 || EBITS == 4, "one byte or one nibble per element");
    static constexpr int GROUP = 2 * EBITS;              // image bytes of a 16-sample group
    static constexpr int DW = TM / 16;                   // words per row of a panel
    static constexpr int NL = BK * DW / NTHREADS;        // words per thread, step and panel
    static constexpr int KSTRIDE = NTHREADS / DW;
    static constexpr int PITCH = DW * GROUP + (EBITS == 8 ? 32 : 8);   // bytes per row of an image
    static constexpr int IMG = BK * PITCH;
    static constexpr int SET = 2 * IMG;                  // A image, B image
    static_assert(NL * NTHREADS == BK * DW && NL >= 1 && BK % 32 == 0, "panel words must divide evenly");
    static_assert(128 % TM == 0 || TM % 128 == 0, "a panel row is a whole number of records or a whole fraction of one");
};

// The reader of the P32 payload (byte images).  Nothing in the step loop is conditional: loads go to clamped (always valid)
// addresses and are consumed one step later, where rows beyond the range and records beyond the panel are replaced by FILL.  A
// guarded load is a branch around the load plus a wait right behind it, and branches keep the decode out of the MFMA gaps.
// FILL is the caller's "adds nothing" word: 0 where the bytes are values and code 00 has the value 0 (the count Gram and its
// LUT form); P32_ALL_MISSING where the bytes are codes and 00 counts as a called sample (KING, the tree).
// The kernels keep their step loops (load ahead, store, barrier, products, barrier): handed to a shared helper the 128-tile KING
// form took four more registers and ran 1 % slower.
template <int TM, int BK, int NTHREADS, uint32_t FILL>
struct PanelReader : PanelGeom<TM, BK, NTHREADS, 8> {
    using G = PanelGeom<TM, BK, NTHREADS, 8>;
    static constexpr int DW = G::DW, KSTRIDE = G::KSTRIDE, PITCH = G::PITCH, IMG = G::IMG, GROUP = G::GROUP;
    static constexpr int REC = 32;                       // bytes of one row of a record

    int d_of, kk_of;
    uint32_t keepA, keepB;                               // all ones: the panel's record lies inside the image; else 0
    const uint8_t *baseA, *baseB;                        // dword of this thread in row 0 of its (clamped) record

    __device__ __forceinline__ PanelReader(const uint8_t *img, int64_t rows, int nt128, int ti, int tj) {
        const int tid = threadIdx.x;
        d_of = tid % DW;
        kk_of = tid / DW;
        // a tile of several records (TM > 128) starts at record ti DW / 8: its groups are counted from there
        constexpr int RPT = DW > 8 ? DW / 8 : 0;
        const int gdA = RPT ? d_of : ti * DW + d_of, gdB = RPT ? d_of : tj * DW + d_of;
        const int recA = ti * RPT + (gdA >> 3), recB = tj * RPT + (gdB >> 3);
        keepA = recA < nt128 ? 0xffffffffu : 0u;
        keepB = recB < nt128 ? 0xffffffffu : 0u;
        baseA = img + (int64_t)(recA < nt128 ? recA : nt128 - 1) * rows * REC + 4 * (gdA & 7);
        baseB = img + (int64_t)(recB < nt128 ? recB : nt128 - 1) * rows * REC + 4 * (gdB & 7);
    }
    // row of word u in the step that starts at kbase, clamped to the range [.., kend)
    __device__ __forceinline__ int64_t row(int u, int64_t kbase, int64_t kend) const {
        const int64_t k = kbase + kk_of + u * KSTRIDE;
        return k < kend ? k : kend - 1;
    }
    // the two dwords of image row `r` (any valid row: the caller's clamped row, or its row list's entry)
    __device__ __forceinline__ void load(int64_t r, uint32_t &wa, uint32_t &wb) const {
        wa = *reinterpret_cast<const uint32_t *>(baseA + r * REC);
        wb = *reinterpret_cast<const uint32_t *>(baseB + r * REC);
    }
    // w where `keep` is all ones, FILL where it is 0
    static __device__ __forceinline__ uint32_t pick(uint32_t keep, uint32_t w) { return (w & keep) | (FILL & ~keep); }
    // the dwords of step `kbase` (loaded for u) through `xf` (dword -> 16 bytes) into the image set
    template <class Xf>
    __device__ __forceinline__ void store(uint8_t *set, int u, int64_t kbase, int64_t kend, uint32_t wa, uint32_t wb, Xf xf) const {
        const bool valid = kbase + kk_of + u * KSTRIDE < kend;
        const int o = (kk_of + u * KSTRIDE) * PITCH + d_of * GROUP;
        *reinterpret_cast<u32x4v *>(set + o) = xf(pick(valid ? keepA : 0u, wa));
        *reinterpret_cast<u32x4v *>(set + IMG + o) = xf(pick(valid ? keepB : 0u, wb));
    }
};

}  // namespace jx
