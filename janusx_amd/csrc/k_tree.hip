// Neighbour-joining tree of packed genotypes: `jx tree -nj`.  Behaviour: src/stats/tree.rs (`build_distance_matrix` :464-502 over
// `pair_mismatch_stats_bitset` :377-403; the exact loop of `nj_newick_from_alignment_u8` :7502-7849 and of
// `nj_newick_from_distance_exact` :7062-7167).
//
// A. Pair counts (`jxg_tree_counts_p32`).  Of a biallelic site only the two homozygous codes carry a letter (00 the first, 11 the
//    second; 10 = IUPAC het code and 01 = missing are unknown), so with U = [code is 00 or 11] and W = +1 (00) / -1 (11) / 0
//        valid = U U^T          S = W W^T = same - differ          mismatch = valid - same = (valid - S) / 2   (exact)
//    are two int8 Grams over the SNP axis.  The kernel reads code images through `PanelReader` of i8_tile.h ([k = SNP][position] code image
//    in LDS, transposed fragment reads, pad samples and rows beyond the last SNP masked to 01) with two v_perm_b32 LUTs
//    per side, two v_mfma_i32_32x32x32_i8 passes per k-step and two i32 accumulator sets.  A site whose two letters are equal adds to
//    `valid` alone, and its het calls carry that letter as well: the caller passes those rows as a second image with `same_base` = 1
//    (one pass, N N^T with N = [code is not 01]) and `accumulate` = 1.
//    Every output element is written by one thread; no atomics.
//
// B. The NJ loop (`jxg_nj_run`) on the n x n f64 matrix, n - 2 steps of three ordinary launches in stream order:
//      row sums -> argmin of q over the pairs (one partial per matrix row) -> one workgroup: final argmin, log, merge.
//    The m active nodes always occupy the storage slots 0 .. m - 1: the new node takes the lower of the two joined slots and the node
//    of slot m - 1 moves into the higher one, so every row read is one contiguous run of m doubles.  Arithmetic follows node ids, not
//    slots: a row sum adds in ascending node id (the list `order`), q = ((m - 2) d_ij - r_i) - r_j has i = the smaller id, and the
//    winner is the least (q, i, j) in lexicographic order with NaN never winning - what the reference's scans give (:6483-6497 first
//    strict minimum in (i, j) order; :7089-7102 with its explicit tie rule).  Branch lengths are the caller's: the log carries
//    (i, j, d_ij, r_i, r_j) of every join.  Products and sums are written with the round-to-nearest intrinsics: never fused.
#include "i8_tile.h"
#include "jx_common.h"

namespace jx {

constexpr int64_t TREE_MAX_ROWS = (int64_t)1 << 29;
constexpr int TREE_BK = 64;                        // SNP rows per step
constexpr int TREE_TM = 64;                        // samples per tile side
constexpr int TREE_WT = 32;                        // samples per wave side

// byte c of a LUT = value of the 2-bit code c (0 = 00 first letter, 1 = 01 missing, 2 = 10 het, 3 = 11 second letter)
constexpr uint32_t TR_U = 0x01000001u, TR_W = 0xff000001u, TR_CALLED = 0x01010001u;

#define TR_MFMA(a, b, c) c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0)

// 64 x 64 tile (blockIdx.y, blockIdx.x) of the n x n pair counts per workgroup of four waves, each 32 x 32.  SAME: the rows are
// equal-letter sites (valid only).  accumulate: add to the stored counts instead of replacing them.
template <bool SAME>
__global__ __launch_bounds__(256, 2) void tree_counts_kernel(const uint8_t *__restrict__ p32, int64_t m, int n, int nt128, int accumulate,
                                                             int32_t *__restrict__ out_valid, int32_t *__restrict__ out_mismatch) {
    constexpr int BK = TREE_BK, TM = TREE_TM, WT = TREE_WT;
    constexpr int NW = TM / WT;
    static_assert(WT == 32, "one 32 x 32 MFMA tile per wave");
    using Reader = PanelReader<TM, BK, 64 * NW * NW, P32_ALL_MISSING>;
    __shared__ __attribute__((aligned(16))) uint8_t smem[Reader::SET];

    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / NW, wn = wave % NW;
    const int ti = (int)blockIdx.y, tj = (int)blockIdx.x;

    const Reader rd(p32, m, nt128, ti, tj);
    constexpr int NL = Reader::NL, PITCH = Reader::PITCH, IMG = Reader::IMG;
    uint32_t wA[NL], wB[NL];                       // payload dwords, loaded one step ahead of their use
    auto load_payload = [&](int u, int64_t kbase) { rd.load(rd.row(u, kbase, m), wA[u], wB[u]); };
    auto store_codes = [&](int u, int64_t kbase) { rd.store(smem, u, kbase, m, wA[u], wB[u], [](uint32_t w) { return codes16(w); }); };

    i32x16 cv, cs;                                 // valid, S
#pragma unroll
    for (int r = 0; r < 16; ++r) cv[r] = 0, cs[r] = 0;

    const int lane_off = frag_lane_off<PITCH>(lane, h);
    auto mfma_ks = [&](int ks) {
        const i32x4 ca = tr8_frag<PITCH>(smem + lane_off + wm * WT + ks * 32 * PITCH);
        const i32x4 cb = tr8_frag<PITCH>(smem + IMG + lane_off + wn * WT + ks * 32 * PITCH);
        // equal letters: the het code of the site is that letter too (`het_iupac`, :310-313), every called sample is known
        const i32x4 ua = lut_frag<SAME ? TR_CALLED : TR_U>(ca), ub = lut_frag<SAME ? TR_CALLED : TR_U>(cb);
        TR_MFMA(ua, ub, cv);
        if constexpr (!SAME) {
            const i32x4 wa = lut_frag<TR_W>(ca), wb = lut_frag<TR_W>(cb);
            TR_MFMA(wa, wb, cs);
        }
    };

    // single buffered, payload loaded one step ahead of its store: the other workgroup of the CU covers the stores and barriers
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
    const int64_t gj = (int64_t)tj * TM + pos_to_sample(wn * WT + cd_col(lane));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t gi = (int64_t)ti * TM + pos_to_sample(cd_row(r, h, wm * WT));
        if (gi < n && gj < n) {
            const int64_t o = gi * n + gj;
            const int v = cv[r];
            const int mis = SAME ? 0 : (v - cs[r]) / 2;
            if (accumulate) {
                out_valid[o] += v;
                if constexpr (!SAME) out_mismatch[o] += mis;
            } else {
                out_valid[o] = v;
                out_mismatch[o] = mis;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// NJ loop
// ---------------------------------------------------------------------------------------------------------------------------

constexpr int NJ_SUM_WAVES = 8;                    // waves per 64 columns of the row sums
constexpr int NJ_SUM_CHUNK = 64;                   // rows per half of their LDS ring
constexpr int NJ_ROW_THREADS = 256;                // threads per matrix row of the argmin
constexpr int NJ_MERGE_THREADS = 1024;

struct NjKey {
    double q;
    int i, j;                                      // node ids, i < j
    int si, sj;                                    // their slots
};

// a replaces b: the comparison of tree.rs:7096 on node ids; a NaN q never wins (every compare with it is false)
__device__ __forceinline__ bool nj_better(const NjKey &a, const NjKey &b) {
    return a.q < b.q || (a.q == b.q && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

__device__ __forceinline__ NjKey nj_none() {
    NjKey k;
    k.q = __builtin_inf();
    k.i = k.j = 0x7fffffff;
    k.si = k.sj = -1;
    return k;
}

struct NjWork {                                    // views into d_work
    int32_t *slot_id;                              // [n] node id of a slot
    int32_t *order[2];                             // [n] each: slots of the active nodes in ascending node id, step parity
    double *r;                                     // [n] row sum of a slot
    NjKey *partial;                                // [n] one key per matrix row
};

static inline size_t nj_align(size_t b) { return (b + 255) & ~(size_t)255; }

static NjWork nj_views(void *d_work, int n) {
    NjWork w;
    uint8_t *p = static_cast<uint8_t *>(d_work);
    w.slot_id = reinterpret_cast<int32_t *>(p);
    p += nj_align(sizeof(int32_t) * (size_t)n);
    w.order[0] = reinterpret_cast<int32_t *>(p);
    p += nj_align(sizeof(int32_t) * (size_t)n);
    w.order[1] = reinterpret_cast<int32_t *>(p);
    p += nj_align(sizeof(int32_t) * (size_t)n);
    w.r = reinterpret_cast<double *>(p);
    p += nj_align(sizeof(double) * (size_t)n);
    w.partial = reinterpret_cast<NjKey *>(p);
    return w;
}

__global__ void nj_init_kernel(int n, int32_t *__restrict__ slot_id, int32_t *__restrict__ order) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) slot_id[s] = s, order[s] = s;
}

// r[c] = sum over the active nodes k in ascending node id of d[k][c] (= d[c][k]; the diagonal holds +0.0).  A workgroup owns 64
// consecutive slots c, one per lane, so every wave reads 64 consecutive doubles of a row per term.  There is one add chain per
// column and only m / 64 workgroups, so the loads in flight per workgroup carry the bandwidth.  Round c of a workgroup: wave 0 adds
// the NJ_SUM_CHUNK rows of round c out of one half of an LDS ring, in list order, while all NJ_SUM_WAVES waves put the rows of round
// c + 1 (loaded one round ago) into the other half, issue the loads of round c + 2, and fetch the list entries of round c + 3 (a
// row's address depends on its list entry: fetched a round ahead, the two latencies do not add up).  Rows beyond the list are
// +0.0: the running sum starts at +0.0 and can never be -0.0, so they change nothing.
__global__ __launch_bounds__(64 * NJ_SUM_WAVES) void nj_rowsum_kernel(const double *__restrict__ d, int64_t ld, int m,
                                                                      const int32_t *__restrict__ order, double *__restrict__ r) {
    constexpr int PER = NJ_SUM_CHUNK / NJ_SUM_WAVES;
    __shared__ double buf[2][NJ_SUM_CHUNK][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const double *col = d + (c < m ? c : m - 1);   // a clamped (valid) address for the lanes beyond the last slot
    int idx[PER];
    double va[PER], vb[PER];
    // list entries of a round (slot 0, a valid row, beyond the list), rows of fetched entries, rows into a half (+0.0 beyond the list)
    auto fetch_idx = [&](int round) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int row = round * NJ_SUM_CHUNK + wave * PER + u;
            idx[u] = row < m ? order[row] : 0;
        }
    };
    auto fetch_rows = [&](double (&v)[PER]) {
#pragma unroll
        for (int u = 0; u < PER; ++u) v[u] = col[(int64_t)idx[u] * ld];
    };
    auto stash = [&](int half, int round, const double (&v)[PER]) {
#pragma unroll
        for (int u = 0; u < PER; ++u) buf[half][wave * PER + u][lane] = round * NJ_SUM_CHUNK + wave * PER + u < m ? v[u] : 0.0;
    };
    fetch_idx(0);
    fetch_rows(va);
    stash(0, 0, va);
    fetch_idx(1);
    fetch_rows(va);
    fetch_idx(2);
    __syncthreads();
    double s = 0.0;
    int half = 0;
    for (int round = 0; round * NJ_SUM_CHUNK < m; ++round) {
        fetch_rows(vb);                            // round + 2
        fetch_idx(round + 3);
        if (wave == 0) {
#pragma unroll 16
            for (int k = 0; k < NJ_SUM_CHUNK; ++k) s = __dadd_rn(s, buf[half][k][lane]);
        }
        stash(half ^ 1, round + 1, va);            // the half wave 0 read one round ago: free since the last barrier
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) va[u] = vb[u];
        half ^= 1;
    }
    if (wave == 0 && c < m) r[c] = s;
}

__device__ __forceinline__ NjKey nj_block_min(NjKey best, NjKey *sh) {
    const int tid = threadIdx.x;
    sh[tid] = best;
    __syncthreads();
    for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
        if (tid < w) {
            const NjKey o = sh[tid + w];
            if (nj_better(o, sh[tid])) sh[tid] = o;
        }
        __syncthreads();
    }
    return sh[0];
}

// least key of the pairs (a, b), b > a, of matrix row a = blockIdx.x: every unordered pair of slots is visited once
__global__ __launch_bounds__(NJ_ROW_THREADS) void nj_argmin_rows_kernel(const double *__restrict__ d, int64_t ld, int m,
                                                                        const int32_t *__restrict__ slot_id, const double *__restrict__ r,
                                                                        NjKey *__restrict__ partial) {
    __shared__ NjKey sh[NJ_ROW_THREADS];
    const int a = blockIdx.x;
    const double m2 = (double)(m - 2);
    const int ida = slot_id[a];
    const double ra = r[a];
    const double *row = d + (int64_t)a * ld;
    NjKey best = nj_none();
    for (int b = a + 1 + threadIdx.x; b < m; b += NJ_ROW_THREADS) {
        const int idb = slot_id[b];
        const double rb = r[b];
        const bool a_first = ida < idb;
        const double t = __dmul_rn(m2, row[b]);
        NjKey k;
        k.q = __dsub_rn(__dsub_rn(t, a_first ? ra : rb), a_first ? rb : ra);
        k.i = a_first ? ida : idb;
        k.j = a_first ? idb : ida;
        k.si = a_first ? a : b;
        k.sj = a_first ? b : a;
        if (nj_better(k, best)) best = k;
    }
    best = nj_block_min(best, sh);
    if (threadIdx.x == 0) partial[a] = best;
}

// One workgroup: the least key of the m - 1 partials, the log entry of join t, the new node's row and column in the lower of the two
// slots, the node of slot m - 1 moved into the higher one, the active list without the two nodes and with the new one at its end.
// keep_negzero = 0: a new distance is `if finite { max(0) } else { 0 }` with the zero canonical +0.0 (alignment route, :7709-7710);
// 1: `if !finite || < 0 { 0 }` (distance-matrix route, :7134-7137: -0.0 stays).
__global__ __launch_bounds__(NJ_MERGE_THREADS) void nj_merge_kernel(double *__restrict__ d, int64_t ld, int n, int m, int t, int keep_negzero,
                                                                    int32_t *__restrict__ slot_id, const int32_t *__restrict__ order_old,
                                                                    int32_t *__restrict__ order_new, const double *__restrict__ r,
                                                                    const NjKey *__restrict__ partial, int32_t *__restrict__ log_ij,
                                                                    double *__restrict__ log_vals) {
    __shared__ NjKey sh[NJ_MERGE_THREADS];
    __shared__ int sh_pos[2];
    const int tid = threadIdx.x;
    NjKey best = nj_none();
    for (int p = tid; p < m - 1; p += NJ_MERGE_THREADS) {
        const NjKey k = partial[p];
        if (nj_better(k, best)) best = k;
    }
    best = nj_block_min(best, sh);
    if (!(best.q < __builtin_inf())) {             // no pair below +inf: the scans leave their start, the first two active nodes
        best.si = order_old[0];
        best.sj = order_old[1];
        best.i = slot_id[best.si];
        best.j = slot_id[best.sj];
    }
    const int si = best.si, sj = best.sj;
    const int a = si < sj ? si : sj, b = si < sj ? sj : si, last = m - 1;
    const double *row_i = d + (int64_t)si * ld, *row_j = d + (int64_t)sj * ld;
    const double dij = row_i[sj];
    if (tid == 0) {
        log_ij[2 * t] = best.i;
        log_ij[2 * t + 1] = best.j;
        log_vals[3 * (int64_t)t] = dij;
        log_vals[3 * (int64_t)t + 1] = r[si];
        log_vals[3 * (int64_t)t + 2] = r[sj];
    }
    // new node -> slot a.  Thread c reads d[si][c], d[sj][c] and writes d[a][c] (a is si or sj: its own column) and d[c][a] (a row
    // that is neither si nor sj): no element is read by one thread and written by another
    double *row_a = d + (int64_t)a * ld;
    for (int c = tid; c < m; c += NJ_MERGE_THREADS) {
        if (c == si || c == sj) continue;
        double v = __dmul_rn(0.5, __dsub_rn(__dadd_rn(row_i[c], row_j[c]), dij));
        const bool finite = v - v == 0.0;
        if (keep_negzero) {
            if (!finite || v < 0.0) v = 0.0;
        } else {
            if (!finite || !(v > 0.0)) v = 0.0;
        }
        row_a[c] = v;
        d[(int64_t)c * ld + a] = v;
    }
    for (int pos = tid; pos < m; pos += NJ_MERGE_THREADS) {
        const int s = order_old[pos];
        if (s == si) sh_pos[0] = pos;
        if (s == sj) sh_pos[1] = pos;
    }
    __syncthreads();                               // the new row is visible to the workgroup; sh_pos is set
    // node of slot `last` -> slot b (the slots 0 .. m - 2 stay in use): reads row `last`, writes row b and column b
    if (b != last) {
        const double *row_l = d + (int64_t)last * ld;
        double *row_b = d + (int64_t)b * ld;
        for (int c = tid; c < last; c += NJ_MERGE_THREADS) {
            const double v = c == b ? 0.0 : row_l[c];
            row_b[c] = v;
            d[(int64_t)c * ld + b] = v;
        }
    }
    const int pi = sh_pos[0], pj = sh_pos[1];
    for (int pos = tid; pos < m; pos += NJ_MERGE_THREADS) {
        int s = order_old[pos];
        if (s == si || s == sj) continue;
        if (s == last) s = b;                      // only reached when b != last
        order_new[pos - (pos > pi ? 1 : 0) - (pos > pj ? 1 : 0)] = s;
    }
    __syncthreads();                               // every read of slot_id[last] / slot_id[si, sj] above is done
    if (tid == 0) {
        const int id_last = slot_id[last];
        slot_id[a] = n + t;
        if (b != last) slot_id[b] = id_last;
        order_new[m - 2] = a;
    }
}

// the last two nodes: ids in ascending order and their distance
__global__ void nj_last_kernel(const double *__restrict__ d, int64_t ld, int t, const int32_t *__restrict__ slot_id,
                               const int32_t *__restrict__ order, int32_t *__restrict__ log_ij, double *__restrict__ last) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int s0 = order[0], s1 = order[1];
        log_ij[2 * t] = slot_id[s0];
        log_ij[2 * t + 1] = slot_id[s1];
        last[0] = d[(int64_t)s0 * ld + s1];
    }
}

}  // namespace jx

using namespace jx;

extern "C" int jxg_tree_counts_p32(const uint8_t *d_p32, int64_t m, int n, int same_base, int accumulate, int32_t *d_valid,
                                   int32_t *d_mismatch, void *stream) {
    if (n <= 0) return fail("jxg_tree_counts_p32: n must be > 0");
    if (m <= 0) return fail("jxg_tree_counts_p32: no rows");
    if (m > TREE_MAX_ROWS) return fail("jxg_tree_counts_p32: at most 536 870 912 rows (exact i32 pair sums)");
    if (!d_p32 || !d_valid || !d_mismatch) return fail("jxg_tree_counts_p32: null pointer");
    const unsigned nt = (unsigned)(((int64_t)n + TREE_TM - 1) / TREE_TM);
    if (nt > 65535u) return fail("jxg_tree_counts_p32: at most 4 194 240 samples");
    const dim3 grid(nt, nt);
    if (same_base)
        hipLaunchKernelGGL((tree_counts_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, d_p32, m, n, num_tiles(n), accumulate ? 1 : 0,
                           d_valid, d_mismatch);
    else
        hipLaunchKernelGGL((tree_counts_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, d_p32, m, n, num_tiles(n), accumulate ? 1 : 0,
                           d_valid, d_mismatch);
    JX_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t jxg_nj_work_bytes(int n) {
    if (n < 2) return 0;
    return (int64_t)(3 * nj_align(sizeof(int32_t) * (size_t)n) + nj_align(sizeof(double) * (size_t)n) + nj_align(sizeof(NjKey) * (size_t)n));
}

extern "C" int jxg_nj_run(double *d_dist, int n, int keep_negzero, int32_t *d_log_ij, double *d_log_vals, double *d_last, void *d_work,
                          void *stream) {
    if (n < 2) return fail("need at least 2 samples to build a tree");
    if (n > (1 << 30)) return fail("jxg_nj_run: node ids are int32: at most 1 073 741 824 samples");
    if (!d_dist || !d_log_ij || !d_log_vals || !d_last || !d_work) return fail("jxg_nj_run: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const NjWork w = nj_views(d_work, n);
    const int64_t ld = n;
    hipLaunchKernelGGL(nj_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w.slot_id, w.order[0]);
    JX_LAUNCH_CHECK();
    for (int t = 0; t < n - 2; ++t) {
        const int m = n - t;                       // active nodes, slots 0 .. m - 1
        const int32_t *order = w.order[t & 1];
        hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64 * NJ_SUM_WAVES), 0, st, d_dist, ld, m, order, w.r);
        hipLaunchKernelGGL(nj_argmin_rows_kernel, dim3((unsigned)(m - 1)), dim3(NJ_ROW_THREADS), 0, st, d_dist, ld, m, w.slot_id, w.r,
                           w.partial);
        hipLaunchKernelGGL(nj_merge_kernel, dim3(1), dim3(NJ_MERGE_THREADS), 0, st, d_dist, ld, n, m, t, keep_negzero ? 1 : 0, w.slot_id,
                           order, w.order[(t + 1) & 1], w.r, w.partial, d_log_ij, d_log_vals);
        JX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(nj_last_kernel, dim3(1), dim3(64), 0, st, d_dist, ld, n - 2, w.slot_id, w.order[(n - 2) & 1], d_log_ij, d_last);
    JX_LAUNCH_CHECK();
    return 0;
}
