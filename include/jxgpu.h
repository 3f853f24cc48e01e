/* jxgpu.h -- C ABI of libjxgpu.so: the MI355X (gfx950) implementation of JanusX's mixed-model hot path.
 *
 * Drop-in boundary: the reference exposes this path as PyO3 functions of the `janusx.janusx` extension
 * module (/root/reference/src/lib.rs:691-1005).  Each entry point below names the reference function it
 * replaces (file:line).  Plain pointers and sizes only; no Python/torch types.
 *
 * Two layers:
 *   jxg_*  device layer : every pointer is a DEVICE pointer (HBM), `stream` is a hipStream_t (may be NULL).
 *                         Used when inputs are already resident in HBM (bench.py, multi-GPU pipeline).
 *   jx_*   host layer   : every pointer is a HOST pointer; the call stages through HBM itself.  These have
 *                         the argument meaning of the reference's PyO3 functions (numpy arrays -> C arrays).
 *
 * Return value: 0 on success, non-zero on failure; `jx_last_error()` returns a thread-local message
 * (the reference raises RuntimeError(msg), e.g. src/stats/grm.rs:3079-3086).
 * Per-SNP numerical failures are not errors: rows are (NaN, NaN, 1.0) for the exact scan
 * (src/stats/lmm.rs:74-81) and (NaN, NaN, NaN) for the fixed-lambda scan (src/stats/fvlmm.rs:1753-1761).
 */
#ifndef JXGPU_H
#define JXGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JXG_TILE 128          /* sample tile of the internal packed layout ("P32": 128 samples = 32 bytes) */
#define JXG_MAX_COV 15        /* max fixed-effect columns (incl. intercept) handled by the scan kernels */

const char *jx_last_error(void);
int jx_version(void);

int jxg_device_count(void);
int jxg_set_device(int dev);
/* device properties: out[0]=CU count, out[1]=clock kHz, out[2]=total HBM MiB, out[3]=LDS bytes/CU */
int jxg_device_info(int64_t *out4);

/* ------------------------------------------------------------------------------------------------
 * Device layer
 * ---------------------------------------------------------------------------------------------- */

/* number of 128-sample tiles and padded sample count for n samples */
int jxg_num_tiles(int n);

/* A1. Re-tile a PLINK SNP-major 2-bit payload (m, bps) into the internal P32 layout
 *   p32[(tile * m_out + j) * 32 + b]  =  samples tile*128 + 4b .. 4b+3 of output SNP j,
 * optionally gathering a sample subset (sample_idx, n_sel) and a row subset (row_idx, m_out).
 * Samples beyond n_sel are encoded 01 (missing).  Replaces the subset/gather plans of
 * src/math/bedmath.rs:1359-1441 and `SubsetDecodePlan`. */
int jxg_repack_p32(const uint8_t *d_packed, int64_t bps, int n_src, int64_t m_src,
                   const int32_t *d_sample_idx, int n_sel, const int64_t *d_row_idx, int64_t m_out,
                   uint8_t *d_p32, void *stream);

/* A1. per-SNP (missing, het, hom_alt) counts over the n_sel real samples of a P32 buffer
 * -> d_counts (m,3) int32.  src/io/gfreader.rs:1378-1395 `count_packed_row_counts`. */
int jxg_row_counts_p32(const uint8_t *d_p32, int64_t m, int n_sel, int32_t *d_counts, void *stream);
/* The same counts over a duplicate-free sample subset straight from a device-resident PLINK payload (m rows of bps bytes), without a
 * P32 image: d_mask (bps bytes) has both bits set at every selected sample.  jx_row_counts takes this route for device payloads. */
int jxg_row_counts_raw_masked(const uint8_t *d_packed, int64_t bps, int64_t m, const uint8_t *d_mask, int32_t *d_counts,
                              void *stream);

/* A3+A4. acc(lower tiles) += Z Z^T over the SNPs rows[k], k in [0, mk), where
 * z = lut[k][code] (4 f32 values per SNP indexed by the 2-bit code; lut[k][1] must be 0).
 * d_rows may be NULL (identity).  d_acc is (n_pad, n_pad) f64 row-major, n_pad = 128*tiles; only tiles
 * (ti >= tj) are written.  Numerics: value LUT split into fp16 hi+lo, three MFMA products with f32
 * accumulation over <= kchunk SNPs, f64 merge -- the counterpart of the reference's f32 SSYRK per block +
 * f64 merge (src/stats/grm.rs:1638-1667, 1700-1772).  SNPs whose values are b + {0, 1, 2} (either orientation) run as
 * an exact integer Gram on the int8 matrix pipes with f64 affine terms; with missing calls they additionally get the sparse
 * correction of k_grm_miss.hip (whole-triangle calls; f64, independent of scheduling).  precision: 0 = default,
 * 2 = rows with missing calls stay on the fp16 split kernel (what row-panel calls always do; the sparse-GRM builder
 * passes it so that its file does not depend on the memory plan), 1 = exact f32 MFMA (not built).  kchunk <= 0 selects
 * the default (8192). */
int jxg_grm_accumulate(const uint8_t *d_p32, int64_t m_total, int n_sel, const int32_t *d_rows,
                       const float *d_lut, int64_t mk, double *d_acc, int kchunk, int precision,
                       void *stream);
/* Tile rows [tile_row_begin, tile_row_end) of the lower triangle only (128-row tiles; end < 0: all); d_acc is then the
 * panel buffer: (end - begin) * 128 rows of the full leading dimension, row 0 = sample row begin * 128. */
int jxg_grm_accumulate_rows(const uint8_t *d_p32, int64_t m_total, int n_sel, const int32_t *d_rows, const float *d_lut,
                            int64_t mk, double *d_acc, int kchunk, int precision, int tile_row_begin, int tile_row_end,
                            void *stream);

/* A5. K = acc * inv_scale, mirrored lower -> upper, written as (n,n) f32 or f64 row-major.
 * src/stats/grm.rs:2771-2785 `grm_scale_and_symmetrize_raw_f64`. */
int jxg_grm_finalize(const double *d_acc, int n, double inv_scale, void *d_out, int out_is_f64,
                     void *stream);

/* A6 (next row 8f-3). Sparse GRM: threshold + order-preserving compaction of the accumulator into the lower-triangle
 * CSC image of the reference's `.spgrm` file (`compute_spgrm_task_entries`, src/stats/spgrm.rs:3422-3554; keep rule
 * `spgrm_keep_value` :1956-1965 — diagonal always, |v| > thr with abs_threshold, everything for thr < 0, else v > thr;
 * order (col, row) as `spgrm_entry_cmp` :1401; layout `coo_lower_to_csc` :3637-3683).
 * jxg_spgrm_count fills d_colptr (n + 1, u64; d_colptr[n] = nnz) and the per-band offsets in d_work
 * (jxg_spgrm_work_bytes(n) bytes), synchronises, and fails on a non-finite value as the reference does;
 * jxg_spgrm_fill writes d_rows (nnz, u32) and d_vals (nnz, f64 = acc * inv_scale). */
int64_t jxg_spgrm_work_bytes(int n);
int jxg_spgrm_count(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold, void *d_work,
                    uint64_t *d_colptr, void *stream);
int jxg_spgrm_fill(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold,
                   const void *d_work, const uint64_t *d_colptr, uint32_t *d_rows, double *d_vals, void *stream);
/* Row-panel forms for a sparse GRM whose n x n f64 accumulator does not fit in HBM (`jx_spgrm_packed_to_jxgrm` switches to
 * them above JXGPU_SPGRM_ACC_GB = 96 GB, or when JXGPU_SPGRM_PANEL_ROWS is set): bands [band0, band1) of 256 sample rows
 * (band1 < 0: all); d_acc is the panel holding exactly those rows (row 0 = sample row band0 * 256, leading dimension
 * num_tiles(n) * 128), d_work needs (band1 - band0) * n * 4 + 16 bytes, and d_colptr / d_rows / d_vals describe the entries of
 * these rows only (merged column by column by the caller). */
int jxg_spgrm_count_bands(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold, int band0,
                          int band1, void *d_work, uint64_t *d_colptr, void *stream);
int jxg_spgrm_fill_bands(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold, int band0,
                         int band1, const void *d_work, const uint64_t *d_colptr, uint32_t *d_rows, double *d_vals,
                         void *stream);

/* Dense symmetric image (n_out, n_out) f64 of a lower-triangle CSC sparse GRM in HBM, optionally restricted / reordered
 * by d_map (n int32: new index of every original sample, -1 = dropped; NULL = identity, n_out = n) — the operand of the
 * sparse REML null model (`subset_sparse_grm_csc`, src/math/cholesky.rs:618-690, then K + lambda I, src/stats/spreml.rs:
 * 384-512), which this library evaluates spectrally (jxg_eigh_f64 of the dense image) instead of by a sparse LLT. */
int jxg_spgrm_densify(const uint64_t *d_colptr, const uint32_t *d_rows, const double *d_vals, int n,
                      const int32_t *d_map, int n_out, double *d_out, void *stream);

/* B1. symmetric eigendecomposition, f64, ascending.  d_a (n,n) is overwritten with U^T row-major
 * (row j = eigenvector j); d_w receives the n eigenvalues.  Replaces LAPACK dsyevd/dsyevr behind
 * src/math/eigh.rs:1422-1528: own Householder tridiagonalisation (k_sytrd.hip), divide and conquer (k_stedc.hip) and
 * compact-WY back-transformation (k_ormtr.hip); rocSOLVER dsyevd only below n = 256.  `ridge` is added to the diagonal first
 * (python/janusx/assoc/workflow.py:5639-5641). */
int jxg_eigh_f64(double *d_a, int n, double ridge, double *d_w, void *stream);
/* 1 when every n-dependent launch grid of jxg_eigh_f64 is inside the HIP limits for an n-row problem (no GPU needed). */
int jxg_eigh_grid_check(int n);

/* Node-level distribution of B1 (no counterpart in the reference, whose LAPACK call is single-process): every rank
 * calls jxg_eigh_f64 on the same matrix; for n >= min_n (<= 0: keep the default 16384) each rank streams 1 / world of
 * the trailing-matrix tiles in every column of the tridiagonalisation and `allreduce(user)` has to sum the
 * `jxg_eigh_dist_staging_doubles(n)` doubles at d_staging over the ranks, ordered on the stream given to jxg_eigh_f64
 * (RCCL through torch.distributed in janusx_amd/pipeline.py).  The replicated part of every column is computed without
 * floating-point atomics in this mode, so the ranks' copies stay bit-identical.  world = 1 or allreduce = NULL: off. */
int64_t jxg_eigh_dist_staging_doubles(int n);
int jxg_eigh_set_dist(int rank, int world, int (*allreduce)(void *), void *user, double *d_staging,
                      int64_t staging_doubles, int min_n);
/* on != 0: the following jxg_eigh_f64 calls of this process decompose matrices of its own (no collective, no sharding, the
 * one-rank thresholds) although a distribution is registered; on = 0 restores it.  Used where a multi-rank job deals whole
 * small problems over the ranks instead of sharding one (the diagonal blocks of the sparse GRM, janusx._SpectralSparseReml). */
int jxg_eigh_set_local(int on);
/* Node-level distribution of the two-stage path of B1 (one rank: n >= 1500; several ranks: n >= 10000): with rank / world set by jxg_eigh_set_dist and a
 * gather callback registered here, every rank runs the (bit-reproducible) reduction stages and the divide and conquer on
 * the same matrix, back-transforms only the eigenvectors [n r / world, n (r + 1) / world) -- two thirds of the flops of
 * the decomposition shard this way -- and gather(user) must then deliver the other ranks' rows of the row-major result
 * into d_a (janusx_amd/pipeline.py: one broadcast per rank over RCCL).  NULL: off (the rank-sharded one-stage
 * tridiagonalisation of jxg_eigh_set_dist is used instead; JXGPU_DIST_EIGH_ONESTAGE=1 forces that too). */
int jxg_eigh_set_gather(int (*gather)(void *), void *user);
/* Guard of that mode: before the sharded back-transformations every rank hashes its replicated intermediate results
 * (eigenvalues of the tridiagonal matrix, the divide and conquer's permutation, the first row of its eigenvector matrix)
 * and agree(user, checksum) must return 1 when every rank reports the same value, 0 when they differ (every rank then
 * back-transforms ALL its eigenvectors itself: slower, self-consistent), < 0 on failure.  NULL: no check.
 * jxg_eigh_last_dist_agree: -1 not checked, 1 the replicas agreed, 0 they differed, for the last decomposition. */
int jxg_eigh_set_agree(int (*agree)(void *, uint64_t checksum), void *user);
int jxg_eigh_last_dist_agree(void);
/* Band reduction of the two-stage path with the trailing matrix SHARDED over the ranks (B1 on several GPUs; no counterpart in
 * the reference, which factors on one host: src/math/eigh.rs:1422-1528): ownership by block rows of `block` samples (<= 0:
 * 2048) dealt cyclically; per panel two collectives through allreduce(user, count) = the sum over the ranks of the first
 * `count` doubles of d_staging (jxg_eigh_band_staging_doubles(n) doubles) on the stream passed to jxg_eigh_f64: the partial
 * symmetric products Z = A22 V, and the gather of the next panel's block column.  From min_n rows on (<= 0: 8192), on the
 * multi-rank two-stage path only.  jxg_eigh_last_band_sharded: 1 when the last decomposition took it. */
int jxg_eigh_set_band_dist(int rank, int world, int (*allreduce)(void *, int64_t count), void *user, double *d_staging,
                           int64_t staging_doubles, int min_n, int block);
int64_t jxg_eigh_band_staging_doubles(int n);
int jxg_eigh_last_band_sharded(void);
/* 1 when the last multi-rank decomposition's divide and conquer formed only this rank's eigenvector columns in its top-level
 * merge (three quarters of its product flops; JXGPU_DIST_DC_WINDOW=0 switches that off). */
int jxg_eigh_last_dc_windowed(void);

/* Building blocks of B1's two-stage reduction, exported for tests and timing scripts (no counterpart in the reference,
 * which calls LAPACK dsyevd, src/math/eigh.rs:1320-1400).  All matrices column-major f64 in HBM.
 *   jxg_dgemm_f64:            C = alpha op(A) op(B) + beta C on the f64 matrix pipes (ksplit <= 0: automatic split over K)
 *   jxg_oz_dgemm_f64:         the same product on the int8 matrix pipes (csrc/k_ozgemm.hip: operands sliced into jxg_oz_planes()
 *                             signed base-254 digit planes, exact i32 digit products, f64 combination; ~254^-planes relative
 *                             to max|row of op(A)| max|column of op(B)|); h_ms (optional, 3 floats): slice A / slice B / product ms
 *   jxg_dsymm_lower_f64:      C = alpha A B + beta C, A (m,m) symmetric with only its lower triangle stored
 *   jxg_dsyr2k_lower_nt_f64:  lower tiles of C (m,m) = alpha A B' + beta C, A, B (m,k)
 *   jxg_sy2st_f64:            dense symmetric -> band (half bandwidth 64) -> tridiagonal (d_d, d_e); d_ab_out (optional,
 *                             128 x n) = the band after stage 1; h_flags[0] / [1] = stage-1 failure / stage-2 abort flag
 *   jxg_sy2st_reflectors_f64: the same, and the reflectors of both stages: d_tau (n) with the columns of d_a below the band
 *                             (reflector j = [0 (j + 64 rows); 1; A(j + 65 : n, j)], tau = 0: identity), d_v2 (n x n: column s =
 *                             the reflectors of sweep s by matrix row, unit entry explicit, step k on the rows
 *                             [s + 1 + 64 k, + min(64, n - that)); only those entries are written) and d_tau2
 *                             (n x jxg_sb2st_steps(n): [s ks + k], zero where no step exists)
 *   jxg_sb2st_steps / jxg_eigh_bandwidth: the stride ks of d_tau2 for n rows / the half bandwidth (64)
 *   jxg_stedc_f64:            the divide and conquer alone (csrc/k_stedc.hip, for every n >= 4: no rocSOLVER shortcut by size): d_d (n)
 *                             and d_e (n - 1) hold the tridiagonal matrix, both are overwritten, d_d receives the eigenvalues
 *                             ascending; d_z is ROW-major, row r = eigenvector of the r-th smallest eigenvalue (the layout the
 *                             eigensolver hands on): n x n, or with 0 <= sel_lo < sel_hi <= n the (sel_hi - sel_lo) x n rows ranked
 *                             [sel_lo, sel_hi) -- the top-level merge then forms only those columns, as on the multi-rank path
 *                             (sel_lo = sel_hi: no window).  leaf <= 0: the product's value (1280, own QL leaves of <= 128 rows),
 *                             else as jxg_eigh_f64 passes JXGPU_STEDC_LEAF
 *   jxg_sbback_apply_f64:     C (n x ncols, ld = n) <- Q2 C from reflectors in that layout (n >= 131).  form = -1: the product's
 *                             own plan; 0 / 1 / 2 / 3: the three-waves-per-unit / one-wave / two-groups-per-pass / balanced kernel
 *                             with nu 16-column units per slab (1..5 / 4..11 / 4..7 / 4..7; a plan that leaves a slab fewer than
 *                             nu - 1 units is refused); groups_per_launch = 0: the product's choice.  h_info (optional, 4 ints):
 *                             form, nu, slabs, apply launches
 *   jxg_ormtr_apply_f64:      C (n x ncols, ld = n) <- Q1 C, Q1 = H_0 .. H_(nref-1), reflector j = [0 (j + off rows); 1;
 *                             A(j + off + 1 : n, j)] with d_tau[j] (the eigensolver's call; JXGPU_ORMTR_NB is read per call) */
int jxg_dgemm_f64(int ta, int tb, int m, int n, int k, double alpha, const double *d_a, int64_t lda, const double *d_b,
                  int64_t ldb, double beta, double *d_c, int64_t ldc, int ksplit, void *stream);
int jxg_oz_dgemm_f64(int ta, int tb, int m, int n, int k, double alpha, const double *d_a, int64_t lda, const double *d_b,
                     int64_t ldb, double beta, double *d_c, int64_t ldc, float *h_ms, void *stream);
int jxg_oz_planes(void);
/* Digit planes per operand of the sliced products for the calls that follow (4 .. 6; anything else: back to the default of
 * JXGPU_OZ_PLANES / 6); returns the previous override.  pipeline.eigh_from_grm(f32_consumer=True) runs Q1 and the
 * divide-and-conquer merges with 5 planes (15 int8 products instead of 21) when the eigenvectors are only kept as the f32
 * U^T the reference's scan consumes (src/stats/reml.rs:109-198): orthogonality 4e-10 instead of 2e-12, far inside f32. */
int jxg_oz_set_planes(int planes);
int jxg_dsymm_lower_f64(int m, int n, double alpha, const double *d_a, int64_t lda, const double *d_b, int64_t ldb,
                        double beta, double *d_c, int64_t ldc, void *stream);
int jxg_dsyr2k_lower_nt_f64(int m, int k, double alpha, const double *d_a, int64_t lda, const double *d_b, int64_t ldb,
                            double beta, double *d_c, int64_t ldc, void *stream);
int jxg_sy2st_f64(double *d_a, int n, double *d_d, double *d_e, double *d_ab_out, int *h_flags, void *stream);
int jxg_sy2st_reflectors_f64(double *d_a, int n, double *d_d, double *d_e, double *d_ab_out, int *h_flags, double *d_tau,
                             double *d_v2, double *d_tau2, void *stream);
int jxg_sb2st_steps(int n);
int jxg_eigh_bandwidth(void);
int jxg_stedc_f64(double *d_d, double *d_e, int n, double *d_z, int leaf, int sel_lo, int sel_hi, void *stream);
int jxg_sbback_apply_f64(const double *d_v2, const double *d_tau2, int n, double *d_c, int ncols, int form, int nu,
                         int groups_per_launch, int *h_info, void *stream);
int jxg_ormtr_apply_f64(const double *d_a, const double *d_tau, int n, int off, int nref, double *d_c, int ncols, void *stream);

/* Multi-GPU reduce of the partial GRMs (no counterpart in the single-process reference): the lower-triangle
 * tiles (ti >= tj, 128 x 128) of the (npad, npad) f64 accumulator <-> a packed buffer of jxg_tri_tiles_doubles(npad)
 * doubles, so the all-reduce over xGMI moves n (n + 1) / 2 values instead of the n^2 square. */
int64_t jxg_tri_tiles_doubles(int npad);
int jxg_tri_tiles_pack_f64(double *d_acc, int npad, double *d_buf, int unpack, void *stream);

/* a <- (a + a^T)/2 (src/math/eigh.rs:179-207); dst = src^T; dst (k,k) f64 = src[idx, idx] of an (n,n)
 * f32/f64 matrix (trait-sample subset, python/janusx/assoc/workflow.py:5509-5560). */
int jxg_symmetrize_f64(double *d_a, int n, void *stream);
int jxg_transpose_f64(const double *d_src, double *d_dst, int n, void *stream);
int jxg_gather_sub_f64(const void *d_src, int src_is_f64, int n, const int32_t *d_idx, int k, double *d_dst,
                       void *stream);

/* f64 U^T -> f32 U^T (row-major), python/janusx/pyBLUP/assoc.py:1818 (`Dh`). */
int jxg_cast_f64_to_f32(const double *d_src, float *d_dst, int64_t count, void *stream);

/* C1. X~ = U^T X, y~ = U^T y; U^T f32, f64 accumulation.  d_xy (n, q) f64 row-major (covariates and y
 * side by side) -> d_out (n, q).  src/stats/reml.rs:109-198. */
int jxg_rotate_xy(const float *d_ut, int n, const double *d_xy, int q, double *d_out, void *stream);

/* C2-C4. null REML: Brent on log10(lambda) in [low, high].  d_out3 (DEVICE) = (lbd, ml, reml).
 * src/stats/reml.rs:572-616 `lmm_reml_null_f32`. */
int jxg_lmm_reml_null(const double *d_s, const double *d_xcov, const double *d_y, int n, int p, double low,
                      double high, int max_iter, double tol, double *d_out3, void *stream);

/* D2 (prep). split f32 U^T (n,n) into two fp16 planes (n_pad, n_pad), scaled by 2^scale_exp, zero padded. */
int jxg_ut_split(const float *d_ut, int n, uint16_t *d_hi, uint16_t *d_lo, int scale_exp, void *stream);

/* D1+D2. rotate a block of SNP rows straight from the packed payload:
 *   out[r, j] = sum_i lut[r][code(rows[r], i)] * u_t[j, i],   r in [0, nrows), j in [0, n)
 * lut (nrows,4) f32 holds the already centred design values (src/decode/decode.rs:192-271);
 * d_out (nrows, n) f32 row-major.  src/stats/lmm.rs:728-784 `rotate_snp_block_with_ut_blas`. */
int jxg_rotate_packed(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                      const float *d_lut, const uint16_t *d_uhi, const uint16_t *d_ulo, int scale_exp,
                      float *d_out, void *stream);

/* D1+D2 split form for block loops: `jxg_lut_split` converts (mk,4) f32 design LUTs into the 16-byte fp16 hi/lo
 * records once (range-checked, synchronises once); `jxg_rotate_packed16` then only launches the MFMA kernel
 * (no allocation, no synchronisation) on rows[r] / lut16[r], r in [0, nrows). */
int jxg_lut_split(const float *d_lut, int64_t mk, void *d_lut16, void *stream);
int jxg_rotate_packed16(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                        const void *d_lut16, const uint16_t *d_uhi, const uint16_t *d_ulo, int scale_exp,
                        float *d_out, void *stream);

/* D1+D2, exact-row form.  A design row whose three genotype values are beta + {0,1,2} (the scan design g - row mean,
 * src/decode/decode.rs:192-271, either allele orientation) and that has no missing call among the n selected samples
 * is rotated as  (c U) + beta * usum:  `jxg_lut_split_rows` stores its integer LUT (fp16-exact, lo plane zero) and
 * beta in d_rowoff[k]; every other row keeps the hi/lo split and gets d_rowoff[k] = NaN.  `jxg_ut_rowsum` gives
 * usum[j] = sum_i u_t[j][i] (n_pad floats).  `jxg_rotate_packed16x` = `jxg_rotate_packed16` plus the affine term; a
 * 128-row tile whose rows all qualify skips the lo plane of the design (two MFMA products instead of three). */
int jxg_lut_split_rows(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, const float *d_lut,
                       int64_t mk, void *d_lut16, float *d_rowoff, void *stream);
/* jxg_lut_split_rows with a tolerance for rows that hold 1 .. miss_max missing calls (jxg_rot_miss_max(n, mean number of
 * missing calls per row) is the default limit: 256 up to n / 300 missing calls per row on average, else 0 -- one decision per
 * scan, a block is not split between the kernels for a handful of rows): they keep the exact path (finite d_rowoff) and d_rowmiss[k] = lut[k][missing] - (value of the int8 rotation's clean
 * form at a missing call = offset + 2 [flipped]) is the weight of their
 * missing-call term, which jxg_rotate_missing_correct adds behind the rotation: out[r][j] += d_r * sum over the row's missing
 * samples i of U[i][j].  d_usamp (n, n) f32 = U with one row per sample (jxg_transpose_f32 of u_t).  Rows with more missing
 * calls stay general (NaN offset, fp16 kernel) as before.  Beyond n / 300 missing calls per row on average jxg_rot_miss_max
 * returns a value > 256 ("no limit"): every affine row keeps the exact path and its missing-call term is ONE MORE int8 product
 * with the indicator of the missing calls as the integer operand, jxg_rotate_missing_dense (d_sel: positions, inside the block,
 * of the rows with d_rowmiss != 0; d_q / d_umax: the three planes of jxg_ut_quant3) -- the cost of the fp16 kernel those rows
 * took before, but exact; JXGPU_ROT_MISS_DENSE=0 restores the fp16 kernel.  src/stats/lmm.rs:728-784 with the decode of
 * src/decode/decode.rs:192-271. */
int jxg_rot_miss_max(int n, double mean_missing_per_row);
int jxg_rotate_missing_dense(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, const int32_t *d_sel, int nsel,
                             const float *d_rowmiss, const int8_t *d_q, const float *d_umax, float *d_out, int64_t ld_out,
                             void *stream);
int jxg_lut_split_rows_m(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, const float *d_lut,
                         int64_t mk, void *d_lut16, float *d_rowoff, float *d_rowmiss, int miss_max, void *stream);
int jxg_transpose_f32(const float *d_src, int n, float *d_dst, void *stream);
int jxg_rotate_missing_correct(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                               const float *d_rowmiss, const float *d_usamp, float *d_out, int64_t ld_out, void *stream);

int jxg_ut_rowsum(const float *d_ut, int n, float *d_usum, void *stream);
int jxg_rotate_packed16x(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                         const void *d_lut16, const float *d_rowoff, const float *d_usum, const uint16_t *d_uhi,
                         const uint16_t *d_ulo, int scale_exp, float *d_out, void *stream);
/* The same with a row pitch `ld_out` >= n (floats) of d_out: writes a block of eigenvector columns of a wider rotated-row
 * buffer (block-diagonal rotation of the sparse-GRM routes, one call per diagonal block). */
int jxg_rotate_packed16x_ld(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                            const void *d_lut16, const float *d_rowoff, const float *d_usum, const uint16_t *d_uhi,
                            const uint16_t *d_ulo, int scale_exp, float *d_out, int64_t ld_out, void *stream);
/* D2 on the int8 matrix pipes for exact design rows (no counterpart in the reference, which runs one f32 SGEMM,
 * src/stats/lmm.rs:728-784).  jxg_ut_quant3: U^T (n x n f32, row j = eigenvector j) -> three int8 planes d_q (3 x npad x npad
 * bytes, npad = 128 ceil(n / 128)) + one scale per eigenvector d_umax (npad f32): U_ij = umax_j (q1 / 127 + q2 / (127 254) +
 * q3 / (127 254^2)) to 2^-24 umax_j.  jxg_rotate_packed16x_q = jxg_rotate_packed16x with those planes and the block's rows
 * split into two lists of positions: d_sel_exact (rows that factor as beta + {0,1,2} without missing calls, i.e. finite
 * d_rowoff: three exact v_mfma_i32_32x32x32_i8 products combined in f64) and d_sel_rest (fp16 hi / lo kernel); together
 * they must cover 0 .. nrows-1.  A row's path, and its bits, do not depend on the block it is scanned in. */
int jxg_ut_quant3(const float *d_ut, int n, int8_t *d_q, float *d_umax, void *stream);
int jxg_rotate_packed16x_q(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const void *d_lut16,
                           const float *d_rowoff, const float *d_usum, const uint16_t *d_uhi, const uint16_t *d_ulo,
                           int scale_exp, const int8_t *d_q, const float *d_umax, const int32_t *d_sel_exact, int n_exact,
                           const int32_t *d_sel_rest, int n_rest, float *d_out, void *stream);

/* Rotation with the fused fixed-lambda reduction (src/stats/fvlmm.rs:1691-1805 consumes G~ only through three weighted sums):
 * G~ is not written; column tile t of this call (128 eigenvector columns, t < jxg_num_tiles(n)) writes its share of
 * (sum_j w_j g~_rj^2, sum_j g~_rj py_j, sum_j g~_rj wx_jk) to d_part[tile0 + t][r][0 .. p+1]; d_w, d_py (n) f32 and d_wx (n, p)
 * f32 are the state of jxg_fvlmm_prepare on this call's columns; d_part (tiles of all calls, nrows, lds_sums >= p + 2) f64.
 * Successive calls with tile0 advancing serve the diagonal blocks of the block route; p <= 8.  jxg_fvlmm_finish_dev adds the
 * ntiles tiles in index order (no atomics: bit-reproducible) and turns the sums into (beta, se, p[, plrt]) -- score_mode != 0:
 * the SparseLMM exact scan (src/stats/splmm.rs:2517-2538, df = n - p). */
int jxg_rotate_packed16x_fused(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                               const void *d_lut16, const float *d_rowoff, const float *d_usum, const uint16_t *d_uhi,
                               const uint16_t *d_ulo, int scale_exp, const float *d_w, const float *d_py,
                               const float *d_wx, int p, double *d_part, int lds_sums, int tile0, void *stream);
int jxg_fvlmm_finish_dev(const double *d_part, int ntiles, int lds, int nrows, int n, int p, const double *d_a_chol,
                         double ypy, int df, int with_plrt, double nullml, double log_det_v, int score_mode,
                         double *d_out, void *stream);

/* D2 (dense input). out[r, j] = sum_i g[r, i] * u_t[j, i] in exact f32 (f32 MFMA).
 * src/stats/lmm.rs:520-552 `rotate_snp_block_with_ut`. */
int jxg_rotate_dense_f32(const float *d_g, int nrows, int n, const float *d_ut, float *d_out, void *stream);

/* D3-D5. exact per-SNP scan of an already rotated block: Brent over -REML per SNP, GLS beta/SE, Wald p.
 * warm = 0: no warm start (reference core API, src/stats/lmm.rs:1577-1579); warm = 1: every SNP starts at
 * init_log10_lbd.  d_out (nrows, 3 or 4) f64 = [beta, se, p(, plrt)]; d_evals (nrows) int32 or NULL.
 * src/stats/lmm.rs:94-199. */
int jxg_lmm_scan(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov,
                 const double *d_y, int p, double low, double high, double tol, int max_iter, int warm,
                 double init_log10_lbd, int with_plrt, double nullml, double *d_out, int32_t *d_evals,
                 void *stream);

/* D3 split form for block loops: the lambda-only REML sums (sum ln v, X'V^-1X, X'V^-1y, y'V^-1y) are tabulated
 * once per (model, [low, high]) as 32-term Chebyshev series per width-2 segment in a caller-provided device
 * workspace of jxg_lmm_tables_bytes() bytes (0 = this configuration needs jxg_lmm_scan_exact); jxg_lmm_scan_tab
 * then scans rotated blocks with one pass over the n samples per objective evaluation, without allocating or
 * synchronising.  jxg_lmm_scan = build + scan. */
int64_t jxg_lmm_tables_bytes(int n, int p, double low, double high);
int jxg_lmm_tables_build(const double *d_s, const double *d_xcov, const double *d_y, int n, int p, double low,
                         double high, void *d_work, void *stream);
int jxg_lmm_scan_tab(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, int p, double low,
                     double high, const void *d_work, double tol, int max_iter, int warm, double init_log10_lbd,
                     int with_plrt, double nullml, double *d_out, int32_t *d_evals, void *stream);

/* Same contract as jxg_lmm_scan, evaluated with the reference's two-pass formulas (normal equations + explicit
 * residual quadratic form per evaluation, src/stats/reml.rs:286-344) instead of the tabulated lambda-only sums;
 * selected automatically when high - low > 16 or when JXGPU_SCAN_EXACT is set.  Used to validate the fast path. */
int jxg_lmm_scan_exact(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov,
                       const double *d_y, int p, double low, double high, double tol, int max_iter, int warm,
                       double init_log10_lbd, int with_plrt, double nullml, double *d_out, int32_t *d_evals,
                       void *stream);

/* D3 along the reference's warm-start chains (`carry_warm_start`, src/stats/lmm.rs:134-161: each SNP's Brent starts from the
 * optimum of the valid SNP before it; the default of `lmm_reml_assoc_packed_f32`, src/stats/lmm.rs:3244-3245, and of the BED
 * route, :2627).  d_chain_off: nchains + 1 ascending int32 row offsets into this block (device); d_carry: nchains doubles
 * (device): the log10 lambda a chain starts from on entry (NaN: none -- the interval midpoint), the optimum of its last valid
 * SNP on return, so that a chain cut by the caller's blocking continues in the next call.  One wave per chain, the chains in
 * parallel.  _tab: tables from jxg_lmm_tables_build; jxg_lmm_scan_chain = build + scan (and jxg_lmm_scan_exact_chain, the
 * reference-formulation kernel, for configurations outside the tables). */
int jxg_lmm_scan_chain_tab(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, int p, double low,
                           double high, const void *d_work, double tol, int max_iter, const int32_t *d_chain_off, int nchains,
                           double *d_carry, int with_plrt, double nullml, double *d_out, int32_t *d_evals, void *stream);
int jxg_lmm_scan_chain(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, const double *d_y, int p,
                       double low, double high, double tol, int max_iter, const int32_t *d_chain_off, int nchains,
                       double *d_carry, int with_plrt, double nullml, double *d_out, int32_t *d_evals, void *stream);
int jxg_lmm_scan_exact_chain(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, const double *d_y,
                             int p, double low, double high, double tol, int max_iter, const int32_t *d_chain_off, int nchains,
                             double *d_carry, int with_plrt, double nullml, double *d_out, int32_t *d_evals, void *stream);
/* D3 for MANY traits along warm-start chains on one block of rotated rows (trait-level LMM; `jx gwas -lmm -trait-level-lmm`).
 * Shared by all traits: d_grot (nrows, n), d_s, d_xcov and the chain offsets (nchains + 1, relative to this block).  Per trait
 * t < ntraits: its table workspace at d_work + t work_stride_bytes (jxg_lmm_tables_build with the trait's y~; a multiple of 16 and
 * at least jxg_lmm_tables_bytes), d_out + t out_rows 3 (beta, se, p; no plrt column), d_evals + t out_rows (or NULL) and the carried
 * states d_carry + t carry_stride (as jxg_lmm_scan_chain_tab).  One workgroup per (chain, trait): its waves split the samples of
 * every evaluation and add their parts in a fixed order -- the table of a trait has the same bits alone or in any batch, in one
 * call or cut into blocks.  p <= 7 (beyond, loop jxg_lmm_scan_chain_tab); ntraits <= 65535.
 * _nw: the same with the number of waves per workgroup given (4, 8 or 16) -- the measurement behind the fixed choice; results
 * depend on it in the last bits. */
int jxg_lmm_traits_chain_tab(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, int p, double low,
                             double high, const void *d_work, int64_t work_stride_bytes, int ntraits, double tol, int max_iter,
                             const int32_t *d_chain_off, int nchains, double *d_carry, int64_t carry_stride, double *d_out,
                             int64_t out_rows, int32_t *d_evals, void *stream);
int jxg_lmm_traits_chain_tab_nw(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov, int p, double low,
                                double high, const void *d_work, int64_t work_stride_bytes, int ntraits, double tol, int max_iter,
                                const int32_t *d_chain_off, int nchains, double *d_carry, int64_t carry_stride, double *d_out,
                                int64_t out_rows, int32_t *d_evals, int nw, void *stream);
/* The series form of D3 in two steps (csrc/k_scan_fast.hip): jxg_lmm_series_coef_tab turns a block of rotated rows into every
 * SNP's Chebyshev series of its SNP-specific sums (one pass over the rows on the f64 matrix pipes; d_scoef: nrows x
 * jxg_lmm_series_doubles(p, low, high) doubles, d_ssq: nrows), jxg_lmm_series_brent_tab runs the Brent searches on stored series
 * -- one per row (d_chain_off NULL; warm / init as jxg_lmm_scan_tab) or along chains (as jxg_lmm_scan_chain_tab).  Chain scans of
 * a whole payload keep the series of many blocks and walk all chains in ONE launch.  jxg_lmm_series_doubles = 0: this
 * (p, low, high) has no series form (more than two width-2 segments, p > 14). */
int64_t jxg_lmm_series_doubles(int p, double low, double high);
int jxg_lmm_series_coef_tab(const float *d_grot, int nrows, int n, const double *d_xcov, int p, double low, double high,
                            const void *d_work, double *d_scoef, double *d_ssq, void *stream);
int jxg_lmm_series_brent_tab(int nrows, int n, const double *d_s, const double *d_xcov, int p, double low, double high,
                             const void *d_work, double tol, int max_iter, int warm, double init_log10_lbd, const double *d_scoef,
                             const double *d_ssq, const int32_t *d_chain_off, int nchains, double *d_carry, int with_plrt,
                             double nullml, double *d_out, int32_t *d_evals, void *stream);

/* E1. fixed-lambda cache (device vectors): w f32(n), py f32(n), wx f32(n,p); scalars to HOST out:
 * a_chol (p*p), ypy, log_det_v, df.  src/stats/fvlmm.rs:1484-1563. */
int jxg_fvlmm_prepare(const double *d_s, const double *d_xcov, const double *d_y, int n, int p, double lbd,
                      float *d_w, float *d_py, float *d_wx, double *h_a_chol, double *h_scalars3);

/* E2. fixed-lambda scan of a rotated block -> d_out (nrows, 3 or 4) f64 = [beta, se, p(, plrt)]; with_plrt adds
 * the ML likelihood-ratio column against nullml (log_det_v from jxg_fvlmm_prepare).  src/stats/fvlmm.rs:1691-1805.
 * The Cholesky factor is on the device: launch only (no allocation, no synchronisation). */
int jxg_fvlmm_scan_dev(const float *d_grot, int nrows, int n, int p, const float *d_w, const float *d_py,
                       const float *d_wx, const double *d_a_chol, double ypy, int df, int with_plrt, double nullml,
                       double log_det_v, double *d_out, void *stream);

/* LMM2 scan of a rotated block ("next" row 8f-2): per SNP a REML Brent, `final_beta_se`, then a second Brent on
 * -ml_loglike seeded with the REML optimum and the LRT against nullml.  d_out6 (nrows, 6) f64 =
 * [beta, se, pwald, lambda_reml, ml_alt, plrt]; invalid rows (NaN, NaN, 1, NaN, NaN, 1).  warm as jxg_lmm_scan.
 * `run_rotated_lmm2_assoc_block_f32`, src/stats/lmm.rs:202-330. */
int jxg_lmm2_scan(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov,
                  const double *d_y, int p, double low, double high, double tol, int max_iter, int warm,
                  double init_log10_lbd, double nullml, double *d_out6, void *stream);

/* The same scan through the reference-formulation kernel (one wave per SNP, every evaluation a pass over the n samples);
 * jxg_lmm2_scan takes the tabulated tiled kernel whenever the lambda range and p fit its tables, this one otherwise. */
int jxg_lmm2_scan_exact(const float *d_grot, int nrows, int n, const double *d_s, const double *d_xcov,
                        const double *d_y, int p, double low, double high, double tol, int max_iter, int warm,
                        double init_log10_lbd, double nullml, double *d_out6, void *stream);

/* Null ML for the LMM2 scan: Brent on -ml_loglike without a SNP column -> d_out2 = (log10 lambda, ml0).
 * src/stats/lmm.rs:2902-2921. */
int jxg_lmm2_null_ml(const double *d_s, const double *d_xcov, const double *d_y, int n, int p, double low,
                     double high, int max_iter, double tol, int has_init, double init, double *d_out2,
                     void *stream);

/* C2. `ml_loglike` and `reml_loglike` of the null model at log10 lambda -> d_out2 = (ml, reml); -1e8 on failure.
 * src/stats/reml.rs:255-470. */
int jxg_lmm_loglike_null(const double *d_s, const double *d_xcov, const double *d_y, int n, int p,
                         double log10_lbd, double *d_out2, void *stream);

/* Duration (ms, HIP events on the launch stream) of the MFMA kernel(s) issued by the most recent
 * jxg_grm_accumulate (which = 0) or jxg_rotate_packed (which = 1) call of this process; which = 2: mean duration
 * of the symv launches sampled by the most recent jxg_eigh_f64 (one per 64-column panel), which = 3: the mean
 * algorithmic megabytes (lower triangle of the trailing matrix, f64) of those launches; which = 4 / 5: duration (ms) and algorithmic
 * GFLOP of the Q2 back-transformation of the most recent two-stage decomposition, 6 - 9: band reduction, bulge chasing, divide and
 * conquer, Q1 (ms; 6 includes the Q1 reflector blocks prepared beside the band reduction's last panels, JXGPU_Q1_TAIL_NT, and 9 only
 * the blocks prepared in line), 10: 1 when the two-stage path ran, 16: apply launches of that Q2, 17: its form (0 three waves per unit, 1 one
 * wave per unit, 2 two sweep groups per pass, 3 balanced five / four units per CU); 18 - 21: the last jx_rrblup_pcg_packed solve --
 * wall ms of its iteration loop, its iterations, the summed HIP-event ms of its two streaming operator kernels (Z'p and Z (Z'p):
 * 2 x n_train x m / 4 payload bytes per application), wall ms of its set-up (images + pre-pass); 22 / 23: summed operator kernel
 * ms and operator applications of the last jx_he_traces_packed call.  Counterpart of the
 * reference's JX_GRM_*_STAGE_TIMING / JX_LMM_*_STAGE_TIMING stage timers (src/stats/grm.rs:3521-3568). */
float jxg_last_kernel_ms(int which);

/* G1 ("next" row). GBLUP on a training GRM: eigh + intercept-only REML (Brent on log10 lambda,
 * v floored at 1e-12) + alpha = U (V^-1 r).  d_k (n,n) f64 is overwritten with U^T; d_yc = y - mean(y).
 * h_out = (lambda, beta_rot, r'V^-1r, ml, reml, mean eigenvalue).  src/stats/gblup.rs:1105-1240. */
int jxg_gblup_fit(double *d_k, int n, double ridge, const double *d_yc, double low, double high, double tol,
                  int max_iter, double *d_alpha, double *h_out, void *stream);
/* d_out[i] = beta0 + sum_j K[rows[i], cols[j]] alpha[j]; K (n_full, n_full) f32/f64 row-major on the device
 * (`square_matrix_subset_cross_dot_f64`, src/stats/gblup.rs:1446-1460). */
int jxg_cross_dot(const void *d_k, int k_is_f64, int64_t n_full, const int32_t *d_rows, int nrows,
                  const int32_t *d_cols, int ncols, const double *d_alpha, double beta0, double *d_out,
                  void *stream);

/* Decoded rows of a P32 image: d_out[r][i] = d_lut[r][code(rows[r], i)] for the n selected samples, d_out (nrows, ld >= n)
 * f32, d_rows = SNP records or NULL for 0 .. nrows-1.  `bed_packed_decode_rows_f32`, src/stats/packed.rs:577-672 (the decode
 * the reference's Python layer asks for when it wants genotype rows as numbers). */
int jxg_decode_rows_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                        const float *d_lut, float *d_out, int64_t ld, void *stream);

/* Matrix-free products with the 2-bit genotype matrix of a P32 image (n selected samples, rows = SNP records or NULL
 * for all m_total); the decoded value of (SNP r, sample i) is d_lut[r][code], d_lut (nrows, 4) f32:
 *   jxg_packed_tdot: d_out[r] = sum_i lut[r][code(r,i)] alpha[i]   (nrows)  `compute_malpha_from_meta_stream`,
 *                    src/stats/gblup.rs:859-925 (and the Z'v half of src/math/pcg.rs:578-640);
 *   jxg_packed_dot : d_out[i] = sum_r lut[r][code(r,i)] beta[r]    (n)      `predict_from_effect_stream`,
 *                    src/stats/gblup.rs:1037-1103 (the Z v half). f64 accumulation; outputs are overwritten. */
int jxg_packed_tdot(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                    const float *d_lut, const double *d_alpha, double *d_out, void *stream);
int jxg_packed_dot(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                   const float *d_lut, const double *d_beta, double *d_out, void *stream);
/* jxg_packed_tdot with the vector rounded to f32 (the Z u half of the PCG operator of `rrblup_pcg_bed`, whose vectors are
 * f32: src/stats/rrblup.rs:1220-1372).  From 1024 samples and SNPs on: the bit planes of the codes against a four-digit int8
 * image of the vector on v_mfma_i32_16x16x64_i8, exact sums (csrc/k_pcg_i8.hip); below that, or with JXGPU_PCG_I8=0: the
 * bit-plane table form (three LDS lookups per four genotypes, f32 partial sums inside a 128-sample tile). */
int jxg_packed_tdot_f32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                        const float *d_lut, const double *d_u, double *d_out, void *stream);
/* The Z'p half of the same operator from a sample-major image of the payload: `jxg_p32_transpose` builds
 * t32[snp_tile][sample][32 B] (128 consecutive SNPs of the row list per record; `jxg_t32_bytes` bytes) once per solve,
 * `jxg_packed_dot_t32` then evaluates d_out[i] = sum_r f32(lut[r][code] * f32(beta[r])) -- the same int8 form (the three
 * per-SNP weight vectors as digit planes) or, below 1024 / with JXGPU_PCG_I8=0, the same bit-plane tables; d_work needs
 * 16 * nrows + 16 bytes. */
int64_t jxg_t32_bytes(int n, int nrows);
int jxg_p32_transpose(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, uint8_t *d_t32,
                      void *stream);
int jxg_packed_dot_t32(const uint8_t *d_t32, int n, int nrows, const float *d_lut, const double *d_beta, void *d_work,
                       double *d_out, void *stream);
/* Skinny products of the randomized SVD (`jx pca -rsvd`; src/stats/rsvd.rs:1548-1661) with the centred additive design
 * Z[r][i] = d_ab[r][0] + d_ab[r][1] g (g = 0 / 1 / 2 for the codes 00 / 10 / 11, missing calls 01 -> 0; d_ab (nrows, 2) f64):
 *   jxg_packed_mm_cols : d_w (nrows, kp) = Z Q,   d_q (n, kp) f64 row-major, P32 image + row list as jxg_packed_tdot;
 *   jxg_packed_tmm_cols: d_y (n, kp)     = Z' W,  d_w (nrows, kp) f64, sample-major T32 image of the same rows
 *                        (`jxg_p32_transpose`).
 * Dose and missing bit planes against a four-digit int8 image of each column on v_mfma_i32_16x16x64_i8 (exact sums, f64
 * merge, csrc/k_rsvd.hip); Z' W adds its SNP slices in a fixed order (run-to-run identical bits).  1 <= kp; up to 32 columns
 * are one pass over the payload, more loop over passes of 32.  The i32 plane sums are exact over 2^23 elements: Z Q refuses
 * n > 8 388 608, Z' W cuts its SNP slices at that length.  Outputs are overwritten. */
int jxg_packed_mm_cols(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const double *d_ab,
                       const double *d_q, int kp, double *d_w, void *stream);
int jxg_packed_tmm_cols(const uint8_t *d_t32, int n, int nrows, const double *d_ab, const double *d_w, int kp, double *d_y,
                        void *stream);
/* ADMIXTURE / FastPop training passes (`jx adamixture`; src/stats/adamixture.rs:2957-3005, 5434-5898) over the rows d_rows
 * (nrows; NULL = rows 0..nrows-1) of a P32 image, genotypes = minor-allele counts after the row flip d_flip (nrows bytes, NULL =
 * no flip), missing calls contribute nothing.  P (nrows, k) and Q (n, k) are f32 row-major, 1 <= k <= 64 and k <= n.
 *   jxg_admx_work_bytes: bytes of the work buffer of the three calls below (partial sums of the EM pass, bounded by a fixed cap);
 *   jxg_admx_called    : d_qb (n) = 2 x the called count of each sample over the rows (a constant of the panel);
 *   jxg_admx_em_step   : one EM pass (a, b, t from the same P, Q; fixed-order merges, run-to-run identical bits) and its
 *                        finalise.  d_mp == NULL: the plain EM step, P_em (clip) -> d_p_em, Q_em (clip, normalised) -> d_q_em,
 *                        P and Q unchanged.  Otherwise one Adam step in place on P, Q and the moments (lr, beta1, beta2, eps, the
 *                        bias-correction scales m_scale, v_scale), clip, Q rows normalised;
 *   jxg_admx_loglik    : d_out[0] = sum g ln rec + (2 - g) ln(1 - rec) (f64; per-workgroup partials added in a fixed order). */
int64_t jxg_admx_work_bytes(int nrows, int n, int k);
int jxg_admx_called(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, void *d_work, int64_t work_bytes,
                    float *d_qb, void *stream);
int jxg_admx_em_step(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const uint8_t *d_flip, int k,
                     float *d_p, float *d_q, const float *d_qb, void *d_work, int64_t work_bytes, float *d_p_em, float *d_q_em,
                     float *d_mp, float *d_vp, float *d_mq, float *d_vq, float lr, float beta1, float beta2, float eps,
                     float m_scale, float v_scale, void *stream);
int jxg_admx_loglik(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const uint8_t *d_flip, int k,
                    const float *d_p, const float *d_q, void *d_work, int64_t work_bytes, double *d_out, void *stream);

/* Cross-validation error of `jx adamixture -cverror` (csrc/k_admx_cv.hip; `cv_fold_hash64`, src/stats/adamixture.rs:1641-1661).
 * The called genotype of listed row j (its position in d_rows, NULL = 0 .. nrows - 1) and sample i < n belongs to fold
 * splitmix(j n + i; seed) mod folds, 2 <= folds <= JXG_ADMX_CV_MAX_FOLDS; missing calls and padding samples to none.
 *   jxg_admx_cv_fold_counts: d_counts (folds) = called genotypes per fold over the rows (integer atomics);
 *   jxg_admx_cv_fold_image : d_out_p32 = compact P32 image (tiles, nrows, 32 bytes) of the rows in list order with the called
 *                            genotypes of fold_id turned into code 01, everything else copied; d_row_stats (nrows, 3) = training
 *                            calls, held-out calls, minor-allele sum of the training calls after the flip d_flip;
 *   jxg_admx_cv_holdout_nll: over the FULL image, for the called genotypes g of fold_id: rec = f32 dot product of P_j and Q_i in
 *                            k order, clamped in f64 to [1e-8, 1 - 1e-8]; d_ll[0] = sum [g == 1] ln 2 + g ln rec + (2 - g)
 *                            ln(1 - rec) (f64, partials added in a fixed order), d_n_eval[0] = their number.  d_work holds
 *                            JXG_ADMX_CV_WORK_BYTES. */
#define JXG_ADMX_CV_MAX_FOLDS 256
#define JXG_ADMX_CV_WORK_BYTES 32768
int jxg_admx_cv_fold_counts(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int folds, uint64_t seed,
                            int64_t *d_counts, void *stream);
int jxg_admx_cv_fold_image(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const uint8_t *d_flip,
                           int folds, uint64_t seed, int fold_id, uint8_t *d_out_p32, int32_t *d_row_stats, void *stream);
int jxg_admx_cv_holdout_nll(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const uint8_t *d_flip,
                            int folds, uint64_t seed, int fold_id, int k, const float *d_p, const float *d_q, void *d_work,
                            int64_t work_bytes, double *d_ll, int64_t *d_n_eval, void *stream);

/* SparseLMM exact scan on rotated rows (`exact_scan_blocks_core`, src/stats/splmm.rs:2567-2880, with V = K + lambda I
 * handled spectrally): per row g~ = U'g the sums g~'Wg~, g~'(W X~), g~.(Py)~ of E2, then the score-form Wald test of
 * `splmm_wald_from_score_denom` (:2517-2538) with the NULL model's sigma2 = ypy / df (df = n - p): out (nrows, 3) =
 * (beta, se, p), rows with g'Pg <= 1e-30 are (NaN, NaN, 1).  d_w, d_py, d_wx, d_a_chol, ypy as produced by
 * jxg_fvlmm_prepare at the null lambda. */
int jxg_splmm_exact_scan_dev(const float *d_grot, int nrows, int n, int p, const float *d_w, const float *d_py,
                             const float *d_wx, const double *d_a_chol, double ypy, int df, double *d_out,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Host layer (reference PyO3 signatures with C arrays)
 * ---------------------------------------------------------------------------------------------- */

/* per-SNP (missing, het, hom_alt) counts over the selected samples -> out_counts (m,3) int32
 * (src/io/gfreader.rs:1378-1395 `count_packed_row_counts`, the QC input of src/stats/lmm.rs:1258-1320). */
int jx_row_counts(const uint8_t *packed, int64_t m, int n_samples, const int64_t *sample_indices, int n_sel,
                  int32_t *out_counts);

/* `grm_packed_f32` / `grm_packed_f64_with_stats` (src/stats/grm.rs:3053-3066, 5611-5651).
 * packed (m, ceil(n_samples/4)) u8; row_flip (m) u8 0/1; row_maf (m) f32; sample_indices (n_sel) i64 or
 * NULL.  out_k (n,n) f32 or f64; out_row_sum (m) f64 or NULL; out_varsum (1) f64 or NULL. */
int jx_grm_packed(const uint8_t *packed, int64_t m, int n_samples, const uint8_t *row_flip,
                  const float *row_maf, const int64_t *sample_indices, int n_sel, int method,
                  void *out_k, int out_is_f64, double *out_row_sum, double *out_varsum);

/* `grm_stream_bed_f32` (src/stats/grm.rs:4676-4703) on an in-memory payload: QC pass + GRM.
 * out_k (n,n) f32; out_eff_m (1); out_keep (m) u8 or NULL. */
int jx_grm_stream_payload_f32(const uint8_t *packed, int64_t m, int n_samples, int method,
                              float maf_threshold, float max_missing_rate, float het_threshold,
                              float *out_k, int64_t *out_eff_m, uint8_t *out_keep);

/* The dense-chunk mirrors (`lmm_reml_chunk*_f32`, `fvlmm_assoc_chunk*_f32`, `lmm_reml_lmm2_chunk_from_snp_f32`, the null-model
 * helpers, `lmm_rotate_x_y_with_ut_f64`, `rust_eigh_from_array_f64`, `lm_block_assoc_f32`) have no host-pointer entry point: they
 * compose the jxg_* pieces above on device buffers (`pipeline.scan_dense_rows`). */

/* `lm_block_assoc_packed` (src/stats/glm.rs:3550-3860): the plain LM scan `jx gwas -lmm / -fvlmm` switches to when the null
 * likelihood-ratio test (jx_gwas_lmm_lm_null_lrt_decision) finds no polygenic variance
 * (python/janusx/assoc/workflow_model_stream.py:930-963).  x (n, q0) row-major INCLUDING the intercept column, ixx (q0, q0) =
 * (X'X)^-1 (`_lm_precompute_ixx_qr`, python/janusx/pyBLUP/assoc.py:453-480), decode = mean-imputed additive
 * ([0, clamp(2 maf, 0, 2), 1, 2] or flipped, src/math/bedmath.rs:984-989).  out (m, 4) = beta, se, pwald (two-sided Student t,
 * df = n - q0 - 1), plrt: `jx_lm_residualize` on the host, `jxg_lm_scan_p32` on the device (`pipeline.scan_rows_lm`). */
/* Host half of the LM scan (glm.rs:3635-3672): r_y = y - X (ixx X'y), *yy_r = r_y'r_y, xr_out (n, q0 + 1) = [X | r_y]
 * rounded through f32 as the reference does before its sgemm. */
int jx_lm_residualize(const double *y, const double *x, const double *ixx, int n, int q0, double *xr_out,
                      double *yy_r_out);
/* Device half on a resident P32 image: d_lut (nrows, 4) f32, d_xr (n, q0 + 1) f64, d_ixx (q0, q0) f64, d_work
 * (nrows * (q0 + 2)) f64 scratch, d_out (nrows, 4) f64. */
int jxg_lm_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const float *d_lut,
                    const double *d_xr, int q0, const double *d_ixx, double yy_r, double *d_work, double *d_out,
                    void *stream);
/* `lm2_stream_bed_to_tsv` (src/stats/glm2.rs:142-325): the SNP-by-covariate interaction scan y ~ X + g + g o c_1 .. g o c_k on a
 * resident P32 image.  d_lut (nrows, 4) f32 = additive value by 2-bit code.  d_w (tiles, nblk, 32, 64) f64 = the weight columns
 * in the operand layout of the 16x16x4 f64 matrix instruction: element [tile][b][ks][lane] = column 16 b + (lane & 15) at sample
 * 128 tile + 4 ks + (lane >> 4), zero beyond n; blocks [0, nblk_v) hold c_a Q_t and c_a r_y (column a (q_rank + 1) + t, t =
 * q_rank for r_y, c_0 = 1) and are summed against v, blocks [nblk_v, nblk) hold c_a c_b (b <= a, column a (a + 1) / 2 + b) and
 * are summed against v^2.  d_sums (nrows, 16 nblk) f64 receives the sums; d_out (nrows, 4 (1 + k) + 4) f64 = (beta, se, chisq,
 * pwald) per coefficient, then chisq_int_joint, p_int_joint, chisq_joint, p_joint; d_flag (nrows) i32 = 1 where the Schur
 * complement (or the interaction block of its inverse) met an exactly zero or non-finite pivot: such a row is NaN in d_out and
 * is left to the caller's pseudo-inverse.  df = n - (q_base + 1 + k).  stage: 0 = both kernels, 1 = the sums, 2 = the algebra. */
int jxg_lm2_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const float *d_lut,
                     const double *d_w, int nblk, int nblk_v, int q_rank, int k, double rss0, int df, double *d_sums,
                     double *d_out, int32_t *d_flag, int stage, void *stream);
/* Device half of `lm_block_assoc_f32` (src/stats/glm.rs:4313-4497): the same LM formulas on an already decoded SNP-major f32
 * block d_g (nrows, ld >= n) on the device, the other arguments as jxg_lm_scan_p32.  Row rules of that entry point (s must
 * exceed 1e-12; a non-finite variance or standard error voids the row, glm.rs:4457-4479). */
int jxg_lm_scan_dense(const float *d_g, int nrows, int n, int64_t ld, const double *d_xr, int q0, const double *d_ixx,
                      double yy_r, double *d_work, double *d_out, void *stream);

/* SparseLMM approximate (GRAMMAR-gamma) scan = `grammar_scan_blocks_core`, additive model (src/stats/splmm.rs:2935-3316; the
 * scan of `scan_with_py_and_rhat`, :3318-3363, behind `splmm_assoc_pcg_bed[_to_tsv]` in scan_mode "approx", :4641, 4814):
 * d_lut (nrows, 4) f32 = mean-imputed additive value by 2-bit code (not centred), d_xr (n, p + 1) f64 = [X | score vector]
 * already rounded through f32 (`pack_score_design_rhs_f32`), d_ixx (p, p) f64 = (X'X)^-1, d_work (nrows * (p + 2)) f64
 * scratch, d_out (nrows, 3) f64 = beta, se, p; score = score_scale g.score_vec, denominator = denom_scale g'M_X g. */
int jxg_splmm_grammar_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows,
                               const float *d_lut, const double *d_xr, int p, const double *d_ixx, double score_scale,
                               double denom_scale, double sigma2, double *d_work, double *d_out, void *stream);

/* Sums behind `estimate_gamma_from_markers` (src/stats/splmm_approx.rs:921-1068) over rotated marker rows g~ = U'g:
 * d_out (nrows, 3 + 2 p) = [g~'g~, g~'Wg~, g~'a~, X~'g~ (p), X~'Wg~ (p)]; d_w, d_a (n) f64, d_x (n, p) f64 row-major. */
int jxg_splmm_gamma_sums(const float *d_grot, int nrows, int n, int64_t ld, int p, const double *d_w, const double *d_a,
                         const double *d_x, double *d_out, void *stream);

/* `gblup_reml_npy_grm` (src/stats/gblup.rs:1242-1516) on an in-memory GRM: fit on K[train,train] + g_eps I, predict
 * K[*,train] alpha + beta0.  out_scalars = (pve, lambda, ml, reml, sigma_g2, sigma_e2, beta0). */
int jx_gblup_reml_grm(const void *k_full, int k_is_f64, int64_t n_full, const int64_t *train_idx, int n_train,
                      const double *y_train, const int64_t *test_idx, int n_test, double g_eps, double low,
                      double high, int max_iter, double tol, int estimate_only, double *out_pred_train,
                      double *out_pred_test, double *out_scalars);

/* `rrblup_pcg_bed` on a resident packed payload (src/stats/rrblup.rs:3494-4307): marker effects by
 * Jacobi-preconditioned conjugate gradients, (Z_c Z_c' + lambda I) beta = Z y_c, Z the standardised genotypes of the
 * training samples streamed from the 2-bit payload (never materialised).  value_lut (eff_m,4) f32 = design values by
 * 2-bit code [00, 01 (missing, must be 0), 10, 11] (src/math/bedmath.rs:1199-1214); row_indices (eff_m) selects the
 * kept SNP rows (NULL = all m_total).  out_beta (eff_m) f32; out_pred_train (n_train) and out_pred_test (n_test) f64
 * (either may be NULL); out_scalars = (converged, iterations, relative residual, sum of centred row sums of squares,
 * intercept).  The iteration follows `pcg_solve_into` for f32 (src/math/pcg.rs:870-949).  `packed` is a host pointer
 * (uploaded once) or a DEVICE pointer (a payload already resident in HBM is used in place -- BASELINE configs[4]: 50 GB);
 * jx_he_traces_packed likewise. */
int jx_rrblup_pcg_packed(const uint8_t *packed, int64_t m_total, int n_samples, const int64_t *row_indices,
                         int64_t eff_m, const float *value_lut, const int64_t *train_idx, int n_train,
                         const double *y_train, const int64_t *test_idx, int n_test, double lambda_value, double tol,
                         int max_iter, float *out_beta, double *out_pred_train, double *out_pred_test,
                         double *out_scalars);
/* Marker-sharded form of that solve over `world` ranks (last row: SNP-range shards, one all-reduce of an
 * n_train-vector per iteration; the reference has no distributed layer, src/math/pcg.rs:870-949 is the iteration every rank
 * runs).  After jx_pcg_set_dist every rank calls jx_rrblup_pcg_packed with ITS range of the kept rows (payload rows, value_lut
 * and out_beta of the shard; samples and y_train replicated): Z'p, mu'p and the three scalars of an iteration are summed over
 * the ranks through allreduce(user), which must add the first jx_pcg_dist_count() doubles of d_staging in place on every
 * rank; predictions and out_scalars are complete on every rank, out_beta is the shard's.  world <= 1 or allreduce NULL: off. */
int jx_pcg_set_dist(int rank, int world, int (*allreduce)(void *), void *user, double *d_staging, int64_t staging_doubles);
/* Image scope of the PCG / Haseman-Elston routes: between jx_pcg_image_scope(1) and jx_pcg_image_scope(0) the two images of the
 * training payload (SNP-major P32, sample-major T32) that jx_he_traces_packed / jx_rrblup_pcg_packed build stay in HBM, keyed by
 * (payload pointer, row list, training samples), and a second call on the same inputs reuses them (`jx gs -rrBLUP -rr-solver pcg`:
 * lambda by HE, then the solve).  The caller guarantees that the payload does not change inside the scope.  (0) frees them. */
int jx_pcg_image_scope(int on);

/* Releases the scratch blocks the library keeps between calls (the eigensolver's workspaces, at most 6 GB each; the reference's
 * CPU path has no counterpart: faer / LAPACK workspaces are freed per call, src/math/linalg.rs:120-184).  Blocks leased by a running call stay.
 * Returns the number of bytes handed back to the driver. */
int64_t jxg_scratch_trim(void);
int64_t jx_pcg_dist_count(void);
/* Exact marker-space rrBLUP on a resident payload: `rrblup_exact_snp_packed` (src/stats/rrblup.rs:3179-3490; cache
 * :1613-1899, fit :1951-2430).  A* = Z Z' - rs rs' / n_train over the training samples (f64), eigendecomposition, Brent on the
 * REML cost of the spectrum (:1568-1611) over log10 lambda in [low, high], beta = V diag(1 / (s + lambda)) V' Z y_c,
 * predictions alpha + Z' beta.  value_lut / row_indices / indices as for jx_rrblup_pcg_packed.  out_scalars (8):
 * pve_trainvar, lambda, REML, var_g, sigma_e2, rank, intercept alpha, mean of y_train. */
int jx_rrblup_exact_snp_packed(const uint8_t *packed, int64_t m_total, int n_samples, const int64_t *row_indices,
                               int64_t eff_m, const float *value_lut, const int64_t *train_idx, int n_train,
                               const double *y_train, const int64_t *test_idx, int n_test, double log10_lambda_low,
                               double log10_lambda_high, double reml_tol, int reml_max_iter, float *out_beta,
                               double *out_pred_train, double *out_pred_test, double *out_scalars);

/* `spgrm_packed_to_jxgrm` (src/stats/spgrm.rs:5201-5278 -> `spgrm_packed_to_jxgrm_core` :3769-3908) and, with
 * stream_denominator != 0, the stream core behind `spgrm_bed_to_jxgrm` (:3910-4264: denominator = sum of 2p(1-p) in
 * f64 whatever the sample selection, :3973-3989): GRM accumulation as jx_grm_packed, then A6; writes the file
 * (`write_sparse_grm_csc` :3745-3767: u64 n, u64 nnz, col_ptr u64 (n+1), row_indices u32 (nnz), zero padding to an
 * 8-byte boundary, values f64 (nnz), little endian) at out_path (already normalised, `normalize_spgrm_path` :450-469
 * is done by the caller).  Errors carry the reference's messages (`validate_spgrm_inputs` :2858-2915). */
int jx_spgrm_packed_to_jxgrm(const uint8_t *packed, int64_t m, int n_samples, const uint8_t *row_flip,
                             const float *row_maf, const int64_t *sample_indices, int n_sel, int method,
                             double threshold, int abs_threshold, int stream_denominator, const char *out_path,
                             int64_t *out_n, int64_t *out_nnz);

/* Several processes (one per GPU) build ONE sparse GRM (BASELINE.json configs[5]; the reference has no counterpart: its
 * tile plan runs on the threads of one process, src/stats/spgrm.rs:3769-3908).  jx_spgrm_set_part(part, nparts) makes the
 * next jx_spgrm_packed_to_jxgrm call of this process compute only the row panels dealt to `part` (back and forth over the
 * parts, so that the cost of the lower triangle's rows is even) and leave them in `<out_path>.part<part>` (out_nnz = the
 * entries of the part); after a barrier one process calls jx_spgrm_merge_parts, which joins the nparts files into the
 * `.spgrm` file of `write_sparse_grm_csc` (:3745-3767) -- byte-identical to the file of a single process -- and removes
 * them.  (0, 1) switches the mode off. */
int jx_spgrm_set_part(int part, int nparts);
int jx_spgrm_merge_parts(const char *out_path, int n, int nparts, int64_t *out_nnz);

/* Haseman-Elston sufficient statistics over the same matrix-free operator (`he_pcg_bed`, src/stats/he.rs:1633-2070,
 * 2101-2636): K = Z'Z / m_scale on the training samples, P the projector off [1, x_cov] (x_cov (n_train, p_cov)
 * row-major or NULL).  out5 = (y'PKPy, y'Py, tr(PKP), tr((PKP)^2), tr(P)); traces by `trace_samples` Rademacher probes
 * generated as the reference does (splitmix64 chains keyed by `seed`), or exactly (one probe per sample) when
 * exact_trace != 0.  The 2x2 HE normal equations are solved by the caller (janusx_amd/janusx.py `he_pcg_bed`). */
int jx_he_traces_packed(const uint8_t *packed, int64_t m_total, int n_samples, const int64_t *row_indices,
                        int64_t eff_m, const float *value_lut, const int64_t *train_idx, int n_train,
                        const double *y_train, const double *x_cov, int p_cov, int trace_samples, uint64_t seed,
                        int exact_trace, double m_scale, double *out5);

/* F2. Association TSV writer (host): replaces `append_assoc_block_from_arrays` / `append_assoc_row_from_fields` and the
 * writer thread behind them (src/io/assoc2tsv.rs:430-548, 604; src/stats/common.rs:374).  Row i = prefix i (the bytes
 * prefix_blob[prefix_off[i] .. prefix_off[i+1]) = `chrom\tpos\tsnp\tallele0\tallele1`) + af, miss, beta, se as `{:.4}`,
 * chisq = (beta/se)^2 and p as `{:.4e}` (Rust float text: unpadded exponent, `NaN`, `inf`; invalid beta / se -> chisq NaN,
 * p = 1, src/math/linalg.rs:111-121) [+ plrt | lambda, ml `{:.6e}`, plrt].  stats (rows, ncol) f64, ncol in {3, 4, 6}.
 * Returns the number of rows written, -1 on error (jx_last_error). */
int64_t jx_assoc_tsv_write(const char *path, const char *prefix_blob, const int64_t *prefix_off, int64_t rows,
                           const float *af, const float *miss, const double *stats, int ncol);
/* Same rows appended behind the present content of `path` (append bit 0 set: no header): the block-wise writer of the
 * streaming scan, counterpart of the reference's AsyncTsvWriter (src/stats/common.rs:374).  append bit 1 (+2): `miss` holds
 * counts of missing samples and is printed as an integer (`AssocMissValue::Count`, src/io/assoc2tsv.rs:452-458: the LM
 * routes) instead of a rate. */
int64_t jx_assoc_tsv_append(const char *path, const char *prefix_blob, const int64_t *prefix_off, int64_t rows,
                           const float *af, const float *miss, const double *stats, int ncol, int append);

/* ---- sparse symmetric solves on the device (csrc/k_spsolve.hip): SparseLMM on a relatedness graph with a connected component
 * beyond one dense eigenproblem.  The reference factorises K + lambda I sparsely on the host (src/math/cholesky.rs:733,
 * 1018-1183) and solves one system per SNP (`exact_scan_blocks_core`, src/stats/splmm.rs:2567-2880); here a block of decoded
 * SNP rows is the right-hand side of ONE Jacobi-preconditioned multi-vector CG over the CSR image (full symmetric pattern) of K.
 * Vectors are (n, ldr) row-major f64, ldr = jxg_sps_ldr(nrhs) (a multiple of 64): row i = entry i of every right-hand side.
 *   jxg_sps_rows_to_cols_f64: decoded rows (nrhs, ld) f32 -> that layout;
 *   jxg_sps_solve_multi:      X = (K + lambda I)^-1 B; d_dinv[i] = 1 / (K_ii + lambda); stops at |r| <= tol |b| for every
 *                             right-hand side; h_info (host) = [iterations, max |r| / |b|]; fails when max_iter is reached;
 *   jxg_sps_scan_sums:        per right-hand side [g'V^-1 g, g.Py, g.(V^-1 X)[:, k]] -> d_sums (nrhs, p + 2): what
 *                             jxg_fvlmm_finish_dev takes with ntiles = 1, score_mode = 1;
 *   d_work: jxg_sps_work_doubles(n, ldr) doubles, shared by the two calls. */
int jxg_sps_ldr(int nrhs);
int64_t jxg_sps_work_doubles(int n, int ldr);
int jxg_sps_rows_to_cols_f64(const float *d_rows, int nrhs, int n, int64_t ld, double *d_out, int ldr, void *stream);
int jxg_sps_solve_multi(int n, const int64_t *d_rowptr, const int32_t *d_col, const double *d_val, double lambda,
                        const double *d_dinv, const double *d_b, int nrhs, int ldr, double tol, int max_iter, double *d_x,
                        double *d_work, double *h_info, void *stream);
int jxg_sps_scan_sums(int n, const double *d_g, const double *d_z, int nrhs, int ldr, const double *d_py, const double *d_vinvx,
                      int p, double *d_sums, double *d_work, void *stream);

/* ---- LD pruning and LD-block r^2 on the packed genotypes (csrc/k_ld.hip; `bed_packed_ld_prune_maf_priority`, src/stats/ld.rs:4245-4361
 * with the strict greedy of :270-402, and `bed_ldblock_r2_rust`, :4721-4811).  A banded SNP x SNP Gram of the P32 image over the
 * samples on the int8 matrix pipes gives, per pair, the integer sums D = sum g_i g_j, N = sum v_i v_j, S_i = sum g_i v_j,
 * S_j = sum v_i g_j, Q_i = sum g_i^2 v_j, Q_j = sum v_i g_j^2 (g dosage with 0 at a missing call, v called indicator).
 * Rows are addressed by "position" p in a row list d_rows (nrows records of the image; NULL = records 0 .. nrows - 1).
 *   jx_ld_window_ends    : host.  Chromosome-grouped order of the file rows (order[p] = row, groups chrom_off[0 .. *n_chrom], m + 1
 *                          slots), the reference's window end win_end[p] of the window that starts at position p (0: none starts
 *                          there) for a base-pair window (window_bp > 0; it wins) or a variant-count window, and band_end[p] =
 *                          the largest end over the windows that contain p.
 *   jxg_ld_band_mask_p32 : bit (j - i - 1) of row i - r0 of d_mask ((r1 - r0) rows of wpr 32-bit words) = pair (i, j) is in LD
 *                          (r^2 finite and > r2_threshold (1 + 1e-12)) for i in [r0, r1), i < j < min(band_end[i], i + 1 + 32 wpr);
 *                          r^2 in f64 in the reference's operation order from the sums and the per-position d_mean, d_std,
 *                          d_hasmiss (row statistics of src/stats/ld.rs:469-543, computed by the caller from the row counts).
 *   jx_ld_prune_greedy   : host, no GPU call.  The strict greedy over the windows that start in [ws0, ws1), reading such a mask
 *                          of the rows [r0, r1); first_unchecked (start: p + 1) and dropped (start: 0) carry the state from range
 *                          to range.
 *   jxg_ld_sums_p32      : d_sums (6, i1 - i0, j1 - j0) int32 = D, N, S_i, S_j, Q_i, Q_j of the pairs i in [i0, i1), j in [j0, j1).
 * n <= 2^24 samples (exact i32 sums and exact f64 products of two of them). */
int jx_ld_window_ends(const int32_t *chrom_codes, const int64_t *positions, int64_t m, int64_t window_bp,
                      int64_t window_variants, int64_t step_variants, int64_t *order, int64_t *chrom_off, int64_t *n_chrom,
                      int64_t *win_end, int64_t *band_end);
int jx_ld_prune_greedy(const double *maf, int64_t nrows, const int64_t *chrom_off, int64_t n_chrom, const int64_t *win_end,
                       int64_t ws0, int64_t ws1, const uint32_t *mask, int64_t r0, int64_t r1, int64_t wpr,
                       int64_t *first_unchecked, uint8_t *dropped);
int jxg_ld_band_mask_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int r0, int r1,
                         const int32_t *d_band_end, const double *d_mean, const double *d_std, const uint8_t *d_hasmiss,
                         double r2_threshold, int wpr, uint32_t *d_mask, void *stream);
int jxg_ld_sums_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int i0, int i1, int j0,
                    int j1, int32_t *d_sums, void *stream);

/* ---- site / sample statistics and LD scores (`jx gstats`; src/stats/gstats.rs, python/janusx/script/gstats.py).
 *   jx_ldsc_window_bounds : host, no GPU call.  `build_sorted_chrom_groups` (src/stats/gstats.rs:873-896) and `compute_window_bounds`
 *                           (:898-953): all rows of a chromosome code form one group (groups by first appearance of the code),
 *                           stably sorted by position, for a cM window by cM and then position; order[p] = file row, groups
 *                           chrom_off[0 .. *n_chrom] (m + 1 slots), and the two-sided window [start[p], end[p]) of position p in
 *                           positions of that order.  kind 0: w_int variants to either side; 1: w_int base pairs; 2: w_cm cM
 *                           (compared against w_cm + 1e-12).  A NaN cM value is refused (the reference sorts with it).
 *   jxg_ld_score_p32      : LD scores (`compute_ldscore_core`, :1002-1171; pair values of :956-1000, 1063-1100) of the positions
 *                           [r0, r1) of a row list, r0 a multiple of 32: d_score[i] = d_self[i] + sum over d_start[i] <= j <
 *                           d_end[i], j != i of r^2(i, j) clamped to [0, 1], from the exact integer pair sums and the per-position
 *                           d_mean, d_std, d_hasmiss as in jxg_ld_band_mask_p32, every pair evaluated from i's side.  d_part:
 *                           (r1 - r0) * npb f64 of scratch, npb >= the number of 32-row blocks of the row list between the one
 *                           that holds the smallest start and the one that holds the largest end of any 32-row block of [r0, r1).
 *                           d_self, d_score are indexed by position like d_mean.
 *   jxg_sample_counts_p32 : per-sample counts over the SNP axis (`accumulate_individual_row_counts`, :180-220): d_counts (2, n)
 *                           int32 = the number of the m rows of the image with code 01 (missing) and with code 10 (het) at
 *                           each of the n samples; pad samples of the last tile are not counted.  m <= 2^31 - 1.
 *   jxg_sample_counts_chunk: SNP rows one workgroup of that kernel walks (for tests and sizing). */
int jx_ldsc_window_bounds(const int32_t *chrom_codes, const int64_t *positions, const double *cm_positions, int64_t m, int kind,
                          int64_t w_int, double w_cm, int64_t *order, int64_t *chrom_off, int64_t *n_chrom, int64_t *start,
                          int64_t *end);
int jxg_ld_score_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, int r0, int r1,
                     const int32_t *d_start, const int32_t *d_end, const double *d_mean, const double *d_std,
                     const uint8_t *d_hasmiss, const double *d_self, int npb, double *d_part, double *d_score, void *stream);
int jxg_sample_counts_p32(const uint8_t *d_p32, int64_t m, int n, int32_t *d_counts, void *stream);
int jxg_sample_counts_chunk(void);

/* ---- KING robust kinship and the unrelated-sample set (`jx grm -king`; csrc/k_king.hip; src/math/KING.rs, Manichaikul et al. 2010).
 * With Z / H / A the indicators of the codes 00 / 10 / 11 of a sample over the m rows of a P32 image and N = Z + H + A (01 = missing
 * and the pad samples of the last tile count nowhere), the pair counts of `king_pair_counts_serial` (src/math/bitwise.rs:259-300;
 * fields of `KingBitCounts`, :127-135) are integer Grams over the SNP axis on the int8 matrix pipes:
 *     shared_nonmissing = N_i N_j, ibs0 = Z_i A_j + A_i Z_j, same_hom = Z_i Z_j + A_i A_j, both_het = H_i H_j, het_i_obs = H_i N_j,
 *     het_j_obs = N_i H_j,   kinship = (both_het - 2 ibs0) / (het_i_obs + het_j_obs) in f64, NaN when the denominator is 0
 * (`king_stats_from_counts`, src/math/KING.rs:217-243).
 *   jxg_king_related_p32 : every pair i < j whose kinship is finite and >= kinship_threshold (finite), as rows (d_i, d_j, d_ibs0,
 *                          d_kinship) of `capacity` slots each, in no particular order (`king_related_pairs_from_bitplanes`,
 *                          :430-528, without its early stop: the exact set, see README "Known differences").  *d_count (device,
 *                          64 bits) ends at the number of such pairs whatever the capacity; rows beyond the capacity are not
 *                          written and the caller runs again with a larger buffer.  No n x n matrix is formed.
 *                          JXGPU_KING_TILE = 64 | 128 forces the tile shape (default: 128 from 1024 tiles of 128 x 128 on).
 *   jxg_king_counts_p32  : d_counts (6, i1 - i0, j1 - j0) int32, planes in the field order of `KingBitCounts`, of the pairs
 *                          (i, j), i in [i0, i1), j in [j0, j1) (any pairs: i >= j included).
 *   jx_king_prune        : host, no GPU call.  `king_prune_related_graph` (:669-743) on a CSR graph (offsets n + 1, neighbors): a
 *                          max-heap of (live degree, sample id) with lazy deletion, ties to the larger id, popped until the top live
 *                          degree is <= 0.  removed (pop order) and kept (ascending) hold n slots each.  A neighbour >= n is refused.
 * m <= 2^29 rows (exact i32 sums). */
int jxg_king_related_p32(const uint8_t *d_p32, int64_t m, int n, double kinship_threshold, int64_t capacity, uint32_t *d_i,
                         uint32_t *d_j, uint32_t *d_ibs0, double *d_kinship, uint64_t *d_count, void *stream);
int jxg_king_counts_p32(const uint8_t *d_p32, int64_t m, int n, int i0, int i1, int j0, int j1, int32_t *d_counts, void *stream);
int jx_king_prune(int64_t n, const int64_t *offsets, const uint32_t *neighbors, uint32_t *kept, int64_t *n_kept, uint32_t *removed,
                  int64_t *n_removed);

/* ---- Multi-trait LM scan (`jx gwas -lm -trait-level`; csrc/k_lm_traits.hip; the shared-projection route of
 * src/stats/lm_trait.rs:481-686): sums = G [Q | R] on the int8 matrix pipes, then the per-(SNP, trait) rule of
 * `lm_assoc_from_shared_projection` (:303-335).
 *   jxg_lmt_cpad     : columns of the plane image of an operand of `ncols` columns (the next multiple of 32).
 *   jxg_lmt_prepare  : d_b = `ncols` f64 columns of n samples, column c at d_b + c ldb -> d_planes (4, cpad, npad) int8 signed radix-128
 *                      digits (npad = 128 ceil(n / 128); k order inside a 16-sample group as the 2-bit decode produces it, byte 4 q + b
 *                      = sample 4 b + q; pad samples and pad columns zero), d_sexp (cpad) i32 = e with 2^e the smallest power of two
 *                      >= max |b_c| (0 for a zero column), d_scale (cpad) f64 = 2^(e - 27), d_colsum (cpad) i64 = the column's integer
 *                      sum over the samples.  b_c = scale ((q1 128 + q2) 128 + q3) 128 + q4) up to scale / 2: exact for a column whose
 *                      entries are multiples of 2^(e - 27).  The entries must be finite.  d_rem (optional, laid out as d_b): what the
 *                      digits leave of every entry, exact in f64; prepared as an operand of its own it adds 28 more bits.
 *   jxg_lmt_sums_p32 : d_sums[r][c] = sum_i v(r, i) b_c[i] for the rows d_rows[0 .. nrows) (nullptr: 0 .. nrows - 1) of a P32 image,
 *                      v = [0, mean_r, 1, 2] by 2-bit code, or [2, mean_r, 1, 0] where d_flip[r] != 0 (d_mean f32, d_flip u8, by
 *                      position in the row list).  Integer plane sums combined in 64 bits, one f64 rounding for the called part, one
 *                      for the missing-call part and one for their sum: the bits of a (row, column) depend on nothing else in the
 *                      call.  n < 2^31 / 254.
 *   jxg_lmt_stats    : per (row r, trait t): gg = d_dsum[r] - sum_k (d_qg[r][k] + d_qg_lo[r][k])^2 (d_qg_lo optional, same layout),
 *                      gy = d_gy[r][t], df = n - rank - 1 -> beta, se,
 *                      chisq = n ln(1 + t^2 / df), p (two-sided Student t; 1 for a void row whose beta, se and chisq are NaN).
 *                      d_out (when given): element [t][r] at d_out + t out_trait_stride + 4 r.  d_count (when given): every (t, r) with
 *                      p <= pmax takes the next slot of the 64-bit device counter (NOT reset by the call: the caller zeroes it once and
 *                      several calls append) and, when the slot is < capacity, writes d_hit_trait = trait0 + t, d_hit_row = row0 + r and
 *                      d_hit_vals (4 f64, the same bits as the dense form); the counter ends at the true total. */
int jxg_lmt_cpad(int ncols);
int jxg_lmt_prepare(const double *d_b, int64_t ldb, int n, int ncols, int8_t *d_planes, double *d_scale, int64_t *d_colsum,
                    int32_t *d_sexp, double *d_rem, void *stream);
int jxg_lmt_sums_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const float *d_mean,
                     const uint8_t *d_flip, const int8_t *d_planes, const double *d_scale, const int64_t *d_colsum, int ncols,
                     double *d_sums, int64_t ld_sums, void *stream);
int jxg_lmt_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy, int64_t ldg, int ntraits,
                  const double *d_dsum, int nrows, const double *d_rss0, int n, double *d_out, int64_t out_trait_stride, double pmax, int64_t capacity,
                  int trait0, int row0, int32_t *d_hit_trait, int32_t *d_hit_row, double *d_hit_vals, uint64_t *d_count,
                  void *stream);

/* ---- Neighbour-joining tree (`jx tree -nj`; csrc/k_tree.hip; src/stats/tree.rs).
 *   jxg_tree_counts_p32 : dense n x n int32 pair counts (both triangles, the diagonal included) of a P32 image of biallelic sites, as
 *                         `pair_mismatch_stats_bitset` (:377-403) counts an alignment whose letters are the two homozygous codes:
 *                         valid = sites where both samples carry 00 or 11, mismatch = sites where one carries 00 and the other 11
 *                         (10 = het and 01 = missing are unknown).  Two int8 Grams on the matrix pipes, mismatch = (valid - S) / 2
 *                         exactly.  same_base != 0: the rows are sites whose two letters are equal: every called sample (00, 10, 11) is
 *                         known there (`het_iupac` of equal letters is that letter), the site adds to valid alone and mismatch gets 0.  accumulate != 0: add to the stored counts (the second image of one panel).  m <= 2^29 rows.
 *   jxg_nj_work_bytes   : bytes of d_work for n leaves.
 *   jxg_nj_run          : exact neighbour joining on the symmetric n x n f64 matrix d_dist (row-major, zero diagonal; consumed), all on
 *                         the device in stream order.  Join t = 0 .. n - 3 creates node n + t from the nodes d_log_ij[2 t] <
 *                         d_log_ij[2 t + 1]: the least (q, i, j), q = ((m - 2) d_ij - r_i) - r_j with m active nodes, the row sums
 *                         r added in ascending node id from 0.0, nothing fused, NaN never the least (no q below +inf: the first two
 *                         active nodes).  d_log_vals[3 t ..] = d_ij, r_i, r_j.  New distances 0.5 ((d_ik + d_jk) - d_ij), made 0.0 when
 *                         not finite or not > 0 (keep_negzero = 0, `nj_newick_from_alignment_u8` :7709-7710 with a canonical +0.0) or
 *                         when not finite or < 0 (keep_negzero != 0, `nj_newick_from_distance_exact` :7134-7137).  The last two nodes:
 *                         d_log_ij[2 (n - 2) ..] (ascending) and their distance d_last[0].  d_log_ij holds 2 (n - 1) int32,
 *                         d_log_vals 3 (n - 2) doubles.  Branch lengths and the Newick text are the caller's. */
int jxg_tree_counts_p32(const uint8_t *d_p32, int64_t m, int n, int same_base, int accumulate, int32_t *d_valid, int32_t *d_mismatch,
                        void *stream);
int64_t jxg_nj_work_bytes(int n);
int jxg_nj_run(double *d_dist, int n, int keep_negzero, int32_t *d_log_ij, double *d_log_vals, double *d_last, void *d_work,
               void *stream);

/* ---- Joint SNP-pair interaction test under the fixed-lambda LMM (`jx fvlmm2`; csrc/k_fvlmm2.hip; src/stats/fvlmm2.rs:37-290).
 *   jxg_fvlmm2_combo_p32 : for pair r over the n selected samples of a P32 image, with c1 / c2 the 2-bit codes of the records
 *                          d_rows1[r] / d_rows2[r]:  d_g1[r][i] = d_lut1[r][c1],  d_g2[r][i] = d_lut2[r][c2],
 *                          d_gc[r][i] = d_tab[r][4 c1 + c2]  (three (nrows, ld >= n) f32 blocks; d_lut1, d_lut2
 *                          (nrows, 4) and d_tab (nrows, 16) f32 built by the host: decoded rows, literals and the combo of
 *                          python/janusx/script/fvlmm2.py:306-385 are functions of the two codes alone).  d_counts[r] = number of
 *                          samples whose literal 1, literal 2, combo value is > 0, by the masks d_pos[r]: bit c1 (literal 1), bit
 *                          4 + c2 (literal 2), bit 8 + 4 c1 + c2 (combo).  A record index outside [0, m_total) gives a NaN row.
 *   jxg_fvlmm2_joint     : `fvlmm2_assoc_chunk_f32` on device rows used as given: d_out (nrows, 9) f64 = (beta, se, p) of g1, g2
 *                          and the combo in  y ~ xcov + g1 + g2 + gc  with weights 1 / (d_s + lbd), ridge 1e-6 on the normal
 *                          equations, Cholesky pivot floor 1e-18, sigma^2 from an explicit residual pass, p = clamp(2 sf(|z|)).  A
 *                          row is nine NaN when one of its 3 n values is not finite, the factorisation fails or r'Wr / sigma^2 is
 *                          not finite and positive; a later coefficient whose variance is not finite and positive leaves the
 *                          earlier ones written.  d_xcov (n, p_cov) f64 row-major, p_cov <= 13 (more is refused), n > p_cov + 3.
 *                          Fails with the reference's messages on a non-positive d_s + lbd and non-finite d_y / d_xcov. */
int jxg_fvlmm2_combo_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows1, const int32_t *d_rows2, int nrows,
                         const float *d_lut1, const float *d_lut2, const float *d_tab, const uint32_t *d_pos, float *d_g1,
                         float *d_g2, float *d_gc, int64_t ld, int32_t *d_counts, void *stream);
int jxg_fvlmm2_joint(const float *d_g1, const float *d_g2, const float *d_gc, int nrows, int n, int64_t ld, const double *d_s,
                     const double *d_xcov, int p_cov, const double *d_y, double lbd, double *d_out, void *stream);

/* ---- FarmCPU raw route (`jx gwas -farmcpu`; csrc/k_farmcpu.hip; src/stats/farmcpu.rs:2629-2941, 3310-3760): the per-marker
 * statistics over the sums of jxg_lmt_sums_p32 against [Q | r_y], Q the orthonormal basis of the design X (n x q0, rank columns).
 *   d_qg, d_qg_lo (nrows, ldq >= rank): the sums of Q's digits and of what they leave (d_qg_lo optional); d_gy[r ldg]: g'r_y;
 *   d_ss (nrows): g'g; bg_rss = |r_y|^2; df = n - q0 - 1 (q0, not the rank: a rank-deficient design keeps the reference's df).
 *   jxg_farmcpu_fem_stats  : b22 = ss - |Q'g|^2; a row with df <= 0, b22 <= 1e-8 or not finite, or ve < 0 / not finite is void:
 *                            d_out (nrows, 3) f64 = (NaN, NaN, 1).  Otherwise beta = gy / b22, ve = (bg_rss - gy beta) / df,
 *                            se = sqrt(ve / b22), p = two-sided Student t through `sanitize_assoc_pvalue`.  k_qtn > 0: d_w
 *                            (k_qtn, ldw >= rank) maps Q'g to b21 of the QTN slots, d_bg_beta / d_diag_ixx (k_qtn) are the
 *                            background coefficients and diag(pinv(X'X)) of the slots; d_max_t2_bits[j] (uint64, zeroed by the
 *                            caller, kept across calls) takes the maximum over the non-void rows of the bit pattern of
 *                            t_j^2 = beta_j^2 / se_j^2, beta_j = bg_beta[j] - b21_j beta, se_j^2 = (ixx_jj + b21_j^2 / b22) ve
 *                            (integer atomicMax: deterministic).  Refuses k_qtn > jxg_farmcpu_max_qtn() = 512 and rank > 512.
 *   jxg_farmcpu_final_stats: the final scan's rule: rss = max(bg_rss - gy^2 / b22, 0), ve = rss / df; a void row, or one without a
 *                            finite beta and a positive finite se, is three NaN. */
int jxg_farmcpu_max_qtn(void);
int jxg_farmcpu_fem_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy, int64_t ldg,
                          const double *d_ss, int nrows, double bg_rss, int df, const double *d_w, int64_t ldw, int k_qtn, const double *d_bg_beta,
                          const double *d_diag_ixx, double *d_out, uint64_t *d_max_t2_bits, void *stream);
int jxg_farmcpu_final_stats(const double *d_qg, const double *d_qg_lo, int64_t ldq, int rank, const double *d_gy, int64_t ldg,
                            const double *d_ss, int nrows, double bg_rss, int df, double *d_out, void *stream);

/* ---- Exhaustive SNP-pair screen on the int8 pipes (`jx fvlmm2 -screen`; csrc/k_pairscreen.hip; an extension).  Classes of a 2-bit
 * code: 00 -> 0, 10 -> 1, 11 -> 2; code 01 (missing, pad) belongs to none.  The table of a pair runs over the samples called at both
 * SNPs: N_ab = number of samples of class a at the first and b at the second SNP, R_ab = the sum of r over them as the 64-bit
 * integer ((A1 128 + A2) 128 + A3) 128 + A4 of the digit-plane sums; the real sum is R_ab * scale.  d_planes: plane 0 of the one
 * column r of a jxg_lmt_prepare image (plane p at d_planes + p plane_stride, plane_stride = cpad * npad; scale = d_scale[0]).
 * n <= 2^24.
 *   jxg_pairscreen_max_variants : 16.
 *   jxg_pairscreen_tables_p32   : d_n (ni, nj, 3, 3) int32 and d_r (ni, nj, 3, 3) int64 of the pairs (d_rows_i[x], d_rows_j[y]),
 *                                 records of the image, lists of any length.
 *   jxg_pairscreen_scan_p32     : every pair i < j of the positions of d_rows (nrows records; NULL: the first nrows) against
 *                                 every variant v < nvariants <= 16.  d_variants (nvariants, 15) f64 = C_v[a][b] (9), L1_v[a] (3),
 *                                 L2_v[b] (3) by class; d_flip (nrows) uint8: a flipped row reads its tables at class 2 - a.  The
 *                                 statistic T = num^2 / (sigma2 den) is the score test of the combo term given the intercept and
 *                                 both literals in the linear model of r on the pair's complete samples (moments in f64, a major, b
 *                                 minor; the 3 x 3 solve by fraction-free elimination, csrc/k_pairscreen.hip).  Void (never a hit):
 *                                 fewer than 5 complete samples, a pivot of Z'Z not positive, den <= 1e-10 xc'xc.  A hit (T >= t_min)
 *                                 takes a slot below `capacity`: d_hit_i / d_hit_j (positions, i < j), d_hit_v, d_hit_n (complete
 *                                 samples), d_hit_stat.  d_counts (2 uint64, zeroed by the call): [0] hits, counted beyond the
 *                                 capacity too; [1] pairs screened.  min_dist > 0: a pair with d_chrom[i] == d_chrom[j] and
 *                                 |d_pos[i] - d_pos[j]| < min_dist is not screened (d_chrom int32, d_pos int64, per position). */
int jxg_pairscreen_max_variants(void);
int jxg_pairscreen_tables_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows_i, int ni, const int32_t *d_rows_j,
                              int nj, const int8_t *d_planes, int64_t plane_stride, int32_t *d_n, int64_t *d_r, void *stream);
int jxg_pairscreen_scan_p32(const uint8_t *d_p32, int64_t m_total, int n, const int32_t *d_rows, int nrows, const uint8_t *d_flip,
                            const int32_t *d_chrom, const int64_t *d_pos, int64_t min_dist, const int8_t *d_planes,
                            int64_t plane_stride, double scale, double sigma2, const double *d_variants, int nvariants, double t_min,
                            int64_t capacity, int32_t *d_hit_i, int32_t *d_hit_j, int32_t *d_hit_v, int32_t *d_hit_n,
                            double *d_hit_stat, uint64_t *d_counts, void *stream);

/* ---- Dense f64 Cholesky and the reductions of multi-kernel AI-REML (`jx reml`; csrc/k_potrf.hip).  Column-major device matrices; only
 * the lower triangle of a symmetric matrix or a factor is read or written.
 *   jxg_potrf_block      : the diagonal block size NB (64).
 *   jxg_dpotrf_lower_f64 : A = L L' in place.  h_info[0] = 0, or the 1-based index of the first pivot that is not positive and finite
 *                          (LAPACK's dpotrf rule); the call then still returns 0 and the lower triangle holds no usable factor.
 *   jxg_dpotrs_lower_f64 : B (n x nrhs) <- (L L')^-1 B, any nrhs >= 0.
 *   jxg_reml_combine_f64 : lower triangle of V (ld n) = theta[q] I + sum_j theta[j] K_j, d_kstack (q, n, n) of symmetric matrices,
 *                          h_theta q + 1 host doubles; q <= 16, n <= 65535.
 *   jxg_sym_dot_f64      : d_out[0] = sum_ij a_ij b_ij over the full symmetric matrices, read from the two lower triangles; sums in a
 *                          fixed order (reproducible run to run).
 *   jxg_potrf_logdet_f64 : h_out[0] = 2 sum_i ln L_ii. */
int jxg_potrf_block(void);
int jxg_dpotrf_lower_f64(double *d_a, int n, int64_t lda, int *h_info, void *stream);
int jxg_dpotrs_lower_f64(const double *d_l, int n, int64_t ldl, double *d_b, int nrhs, int64_t ldb, void *stream);
int jxg_reml_combine_f64(const double *d_kstack, int q, int n, const double *h_theta, double *d_v, void *stream);
int jxg_sym_dot_f64(const double *d_a, const double *d_b, int n, int64_t lda, int64_t ldb, double *d_out, void *stream);
int jxg_potrf_logdet_f64(const double *d_l, int n, int64_t ldl, double *h_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* JXGPU_H */
