// Host layer of libjxgpu: reference-shaped entry points (host arrays in, host arrays out) that stage through
// HBM and drive the device layer; per-SNP statistics / filter logic (integer counts -> f32/f64 decisions) is
// done on the host exactly as the reference writes it, so the kept-SNP set is bit-exact.
#include <errno.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <queue>
#include <chrono>
#include <vector>

#include "jx_common.h"

namespace jx {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(const std::string &msg) {
    g_err = msg;
    return 1;
}

namespace {
struct ScratchSlot {
    void *p = nullptr;
    size_t cap = 0;
    bool busy = false;
};
ScratchSlot g_scratch[8];
std::mutex g_scratch_mu;
}  // namespace

int scratch_acquire(int which, size_t bytes, void **p) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    ScratchSlot &s = g_scratch[which & 7];
    if (s.busy) return 1;
    if (s.cap < bytes) {
        if (s.p) (void)hipFree(s.p);
        s.p = nullptr;
        s.cap = 0;
        hipError_t e = hipMalloc(&s.p, bytes);
        if (e != hipSuccess) {
            s.p = nullptr;
            fail(std::string("hipMalloc(") + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
            return 2;
        }
        s.cap = bytes;
    }
    s.busy = true;
    *p = s.p;
    return 0;
}

void scratch_release(int which) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    g_scratch[which & 7].busy = false;
}

// Hand the kept scratch blocks (<= 6 GB each, grown on demand by the eigensolver's stages) back to the driver: for a long-lived
// host process between two problems of very different size.  Blocks leased by a running call stay.  -> bytes released
extern "C" int64_t jxg_scratch_trim(void) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    int64_t freed = 0;
    for (ScratchSlot &s : g_scratch) {
        if (s.busy || !s.p) continue;
        (void)hipFree(s.p);
        freed += (int64_t)s.cap;
        s.p = nullptr;
        s.cap = 0;
    }
    return freed;
}

// keep the stream-ordered pool's blocks across synchronisations (default threshold 0: every hipFreeAsync'ed block goes back to the
// driver at the next synchronisation and the next hipMallocAsync pays a fresh allocation): 256 MB cover the largest user
void async_pool_keep() {
    static bool pool_set = false;
    if (pool_set) return;
    int dev = 0;
    hipMemPool_t pool = nullptr;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
        uint64_t thr = (uint64_t)256 << 20;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
    }
    (void)hipGetLastError();
    pool_set = true;
}

// ---- value LUTs (host) ---------------------------------------------------------------------------

// GRM design LUT indexed by the 2-bit code [00, 01(missing), 10, 11]
// (src/decode/decode.rs:813-839, src/math/bedmath.rs:1208-1224, decode.rs:558-566).
static void grm_lut_from_maf(float maf, bool flip, int method, float out[4]) {
    float p = maf;
    if (p < 0.0f) p = 0.0f;
    if (p > 1.0f) p = 1.0f;
    const float mean_g = 2.0f * p;
    const float var = 2.0f * p * (1.0f - p);
    float sc = 1.0f;
    if (method == 2) sc = (var > 1e-12f) ? (1.0f / sqrtf(var)) : 0.0f;
    const float g0 = flip ? 2.0f : 0.0f, g1 = 1.0f, g2 = flip ? 0.0f : 2.0f;
    out[0] = (g0 - mean_g) * sc;
    out[1] = 0.0f;
    out[2] = (g1 - mean_g) * sc;
    out[3] = (g2 - mean_g) * sc;
}

// denominators, src/stats/grm.rs:91-111 (full-sample centred) and bedmath.rs:1411-1438 (subset route)
static double grm_varsum(const float *row_maf, int64_t m, int method, bool full) {
    if (method != 1) return (double)m;
    double acc = 0.0;
    if (full) {
        for (int64_t j = 0; j < m; ++j) {
            const double p = (double)row_maf[j];
            const double v = 2.0 * p * (1.0 - p);
            if (isfinite(v) && v > 0.0) acc += v;
        }
    } else {
        for (int64_t j = 0; j < m; ++j) {
            float p0 = row_maf[j];
            p0 = p0 < 0.0f ? 0.0f : (p0 > 1.0f ? 1.0f : p0);
            const float mean_g = 2.0f * p0;
            float pg = 0.5f * mean_g;
            pg = pg < 0.0f ? 0.0f : (pg > 1.0f ? 1.0f : pg);
            float v = 2.0f * pg * (1.0f - pg);
            if (v < 0.0f) v = 0.0f;
            acc += (double)v;
        }
    }
    return acc;
}

struct SampleSel {
    std::vector<int32_t> idx;
    bool identity = true;
    int n = 0;
};

static int make_sample_sel(const int64_t *sample_indices, int n_sel, int n_samples, SampleSel &s) {
    if (!sample_indices) {
        s.identity = true;
        s.n = n_samples;
        return 0;
    }
    if (n_sel <= 0) return fail("sample_indices must not be empty");
    s.idx.resize(n_sel);
    s.identity = (n_sel == n_samples);
    for (int i = 0; i < n_sel; ++i) {
        const int64_t v = sample_indices[i];
        if (v < 0 || v >= n_samples)
            return fail("sample index out of range: " + std::to_string(v) + " >= " + std::to_string(n_samples));
        s.idx[i] = (int32_t)v;
        if (v != i) s.identity = false;
    }
    s.n = n_sel;
    return 0;
}

// true when `p` points into device memory (a payload that is already resident in HBM: torch CUDA tensor, hipMalloc)
bool is_device_ptr(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                     // plain (unregistered) host memory: not an error for the caller
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

// Re-tile a PLINK payload to P32 (with optional sample subset). p32 must stay alive.  `packed` may be a host pointer
// (uploaded first) or a device pointer (used in place: no host copy of the payload exists anywhere).  Refuses with a
// clear message, before anything is allocated, when the device copies do not fit the free HBM.
static int stage_p32(const uint8_t *packed, int64_t m, int n_samples, const SampleSel &sel, DevBuf &p32) {
    const int64_t bps = (n_samples + 3) / 4;
    const bool on_device = is_device_ptr(packed);
    const int nt = num_tiles(sel.n);
    {
        size_t fr = 0, tot = 0;
        const double need = (on_device ? 0.0 : (double)m * (double)bps) + (double)nt * (double)m * 32.0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && need > 0.95 * (double)fr)
            return fail("packed payload of " + std::to_string((long long)(m * bps >> 20)) + " MiB: its device images need " +
                        std::to_string((long long)(need / 1048576.0)) + " MiB of HBM, " + std::to_string((long long)(fr >> 20)) +
                        " MiB are free (split the SNP rows over several calls)");
    }
    static const bool trace = getenv("JXGPU_PCG_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (!trace) return;
        (void)hipDeviceSynchronize();
        fprintf(stderr, "[jxgpu stage_p32] %-20s %8.1f ms\n", what,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    // every allocation of the staging BEFORE the first copy or launch: a hipMalloc behind work in flight (or right behind a large
    // hipFree) has been measured at hundreds of milliseconds to seconds on this stack, with the device idle 0.3 ms
    DevBuf raw, didx;
    if (!on_device && raw.alloc((size_t)(m * bps))) return 1;
    if (!sel.identity && didx.alloc(sizeof(int32_t) * sel.idx.size())) return 1;
    if (p32.alloc((size_t)nt * (size_t)m * 32)) return 1;
    mark("hipMalloc raw / idx / p32");
    const uint8_t *d_raw = packed;
    if (!on_device) {
        JX_HIP(hipMemcpy(raw.p, packed, (size_t)(m * bps), hipMemcpyHostToDevice));
        d_raw = raw.as<uint8_t>();
    }
    const int32_t *d_idx = nullptr;
    if (!sel.identity) {
        JX_HIP(hipMemcpy(didx.p, sel.idx.data(), sizeof(int32_t) * sel.idx.size(), hipMemcpyHostToDevice));
        d_idx = didx.as<int32_t>();
    }
    mark("uploads");
    if (jxg_repack_p32(d_raw, bps, n_samples, m, d_idx, sel.n, nullptr, m, p32.as<uint8_t>(), nullptr))
        return 1;
    JX_HIP(hipDeviceSynchronize());
    mark("repack");
    return 0;
}

}  // namespace jx

using namespace jx;

extern "C" const char *jx_last_error(void) { return g_err.c_str(); }
extern "C" int jx_version(void) { return 100; }

extern "C" int jxg_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

extern "C" int jxg_set_device(int dev) {
    JX_HIP(hipSetDevice(dev));
    return 0;
}

extern "C" int jxg_device_info(int64_t *out4) {
    int dev = 0;
    JX_HIP(hipGetDevice(&dev));
    hipDeviceProp_t pr;
    JX_HIP(hipGetDeviceProperties(&pr, dev));
    out4[0] = pr.multiProcessorCount;
    out4[1] = pr.clockRate;
    out4[2] = (int64_t)(pr.totalGlobalMem >> 20);
    out4[3] = (int64_t)pr.maxSharedMemoryPerMultiProcessor;
    return 0;
}

// per-SNP (missing, het, hom_alt) over the selected samples (src/io/gfreader.rs:1378-1395
// `count_packed_row_counts[_selected]`), host arrays in/out.
extern "C" int jx_row_counts(const uint8_t *packed, int64_t m, int n_samples, const int64_t *sample_indices,
                             int n_sel, int32_t *out_counts) {
    if (n_samples <= 0) return fail("n_samples must be > 0");
    if (m <= 0) return 0;
    SampleSel sel;
    if (make_sample_sel(sample_indices, n_sel, n_samples, sel)) return 1;
    DevBuf p32, dcnt;
    if (is_device_ptr(packed)) {
        // a payload that already lives in HBM: counts straight from it under a sample mask (no 40 GB image allocated, filled and
        // freed for three numbers per SNP) -- when the selection has no duplicate (a mask counts a sample once)
        const int64_t bps = ((int64_t)n_samples + 3) / 4;
        std::vector<uint8_t> mask((size_t)bps, 0);
        bool dup = false;
        if (sel.identity) {
            for (int i = 0; i < n_samples; ++i) mask[(size_t)(i >> 2)] |= (uint8_t)(3u << (2 * (i & 3)));
        } else {
            for (int32_t v : sel.idx) {
                const uint8_t bit = (uint8_t)(3u << (2 * (v & 3)));
                if (mask[(size_t)(v >> 2)] & bit) dup = true;
                mask[(size_t)(v >> 2)] |= bit;
            }
        }
        if (!dup) {
            DevBuf dmask;
            if (dmask.alloc((size_t)bps) || dcnt.alloc(sizeof(int32_t) * 3 * (size_t)m)) return 1;
            JX_HIP(hipMemcpy(dmask.p, mask.data(), (size_t)bps, hipMemcpyHostToDevice));
            if (jxg_row_counts_raw_masked(packed, bps, m, dmask.as<uint8_t>(), dcnt.as<int32_t>(), nullptr)) return 1;
            JX_HIP(hipMemcpy(out_counts, dcnt.p, sizeof(int32_t) * 3 * (size_t)m, hipMemcpyDeviceToHost));
            return 0;
        }
    }
    if (stage_p32(packed, m, n_samples, sel, p32)) return 1;
    if (dcnt.alloc(sizeof(int32_t) * 3 * (size_t)m)) return 1;
    if (jxg_row_counts_p32(p32.as<uint8_t>(), m, sel.n, dcnt.as<int32_t>(), nullptr)) return 1;
    JX_HIP(hipMemcpy(out_counts, dcnt.p, sizeof(int32_t) * 3 * (size_t)m, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// grm_packed_f32 / grm_packed_f64_with_stats (src/stats/grm.rs:204-360, 3066, 5611)
// ---------------------------------------------------------------------------------------------------
extern "C" int jx_grm_packed(const uint8_t *packed, int64_t m, int n_samples, const uint8_t *row_flip,
                             const float *row_maf, const int64_t *sample_indices, int n_sel, int method,
                             void *out_k, int out_is_f64, double *out_row_sum, double *out_varsum) {
    if (n_samples <= 0) return fail("n_samples must be > 0");
    if (method != 1 && method != 2)
        return fail("unsupported method=" + std::to_string(method) + "; expected 1 (centered) or 2 (standardized)");
    if (m <= 0) return fail("packed must contain at least one SNP row");
    SampleSel sel;
    if (make_sample_sel(sample_indices, n_sel, n_samples, sel)) return 1;
    const int n = sel.n;
    const double D = grm_varsum(row_maf, m, method, sel.identity);
    if (!(isfinite(D) && D > 0.0)) return fail("invalid centered GRM denominator: sum(2p(1-p)) <= 0");

    std::vector<float> lut((size_t)m * 4);
    for (int64_t j = 0; j < m; ++j) {
        grm_lut_from_maf(row_maf[j], row_flip[j] != 0, method, &lut[(size_t)j * 4]);
        if (out_row_sum) {
            float p = row_maf[j];
            p = p < 0.0f ? 0.0f : (p > 1.0f ? 1.0f : p);
            // decode.rs:795-799 (method 2) / :841 (method 1): mean_g * n_out
            out_row_sum[j] = (method == 2) ? 2.0 * (double)p * (double)n : (double)(2.0f * p) * (double)n;
        }
    }
    DevBuf p32, dlut, acc, dout;
    if (stage_p32(packed, m, n_samples, sel, p32)) return 1;
    if (dlut.alloc(lut.size() * sizeof(float))) return 1;
    JX_HIP(hipMemcpy(dlut.p, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    const int64_t npad = (int64_t)num_tiles(n) * JXG_TILE;
    if (acc.alloc(sizeof(double) * (size_t)(npad * npad))) return 1;
    JX_HIP(hipMemset(acc.p, 0, sizeof(double) * (size_t)(npad * npad)));
    if (jxg_grm_accumulate(p32.as<uint8_t>(), m, n, nullptr, dlut.as<float>(), m, acc.as<double>(), 0, 0, nullptr))
        return 1;
    const size_t esz = out_is_f64 ? sizeof(double) : sizeof(float);
    if (dout.alloc(esz * (size_t)n * (size_t)n)) return 1;
    if (jxg_grm_finalize(acc.as<double>(), n, 1.0 / D, dout.p, out_is_f64, nullptr)) return 1;
    JX_HIP(hipMemcpy(out_k, dout.p, esz * (size_t)n * (size_t)n, hipMemcpyDeviceToHost));
    if (out_varsum) *out_varsum = (method == 1) ? D : (double)m;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// spgrm_packed_to_jxgrm / the stream core behind spgrm_bed_to_jxgrm (src/stats/spgrm.rs:3769-3908, 3910-4264)
// ---------------------------------------------------------------------------------------------------
extern "C" int64_t jxg_spgrm_work_bytes(int n);
extern "C" int jxg_spgrm_count(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold,
                               void *d_work, uint64_t *d_colptr, void *stream);
extern "C" int jxg_spgrm_count_bands(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold,
                                     int band0, int band1, void *d_work, uint64_t *d_colptr, void *stream);
extern "C" int jxg_spgrm_fill_bands(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold,
                                    int band0, int band1, const void *d_work, const uint64_t *d_colptr, uint32_t *d_rows,
                                    double *d_vals, void *stream);
extern "C" int jxg_grm_accumulate_rows(const uint8_t *d_p32, int64_t m_total, int n_sel, const int32_t *d_rows,
                                       const float *d_lut, int64_t mk, double *d_acc, int kchunk, int precision,
                                       int tile_row_begin, int tile_row_end, void *stream);
extern "C" int jxg_spgrm_fill(const double *d_acc, int n, double inv_scale, double threshold, int abs_threshold,
                              const void *d_work, const uint64_t *d_colptr, uint32_t *d_rows, double *d_vals,
                              void *stream);

// ---- sparse GRM by row panels: entries of a panel, merge + file writer, part files for several ranks ---------------------
namespace {
struct PanelEntries {
    int64_t index = 0;                 // position of the panel (rows ascend with it)
    std::vector<uint64_t> cp;          // n + 1 offsets into r / v
    std::vector<uint32_t> r;
    std::vector<double> v;
};
// (part, nparts) of this process for jx_spgrm_packed_to_jxgrm: with nparts > 1 the row panels are dealt cyclically, a process
// builds only its own and writes them to `<out>.part<k>`; jx_spgrm_merge_parts joins the files (jx_spgrm_set_part)
int g_spgrm_part = 0, g_spgrm_nparts = 1;

// write_sparse_grm_csc (src/stats/spgrm.rs:3745-3767): u64 n, u64 nnz, col_ptr, row_indices, zero padding to 8 bytes, values (LE);
// the panels (ascending index) are merged column by column (rows ascend with the panels, so the order inside a column is kept)
int spgrm_merge_write(const std::vector<PanelEntries> &panels, int n, const char *out_path, uint64_t *out_nnz) {
    std::vector<uint64_t> colptr((size_t)n + 1);
    uint64_t nnz = 0;
    for (const auto &pe : panels) nnz += pe.cp[(size_t)n];
    colptr[0] = 0;
    for (int c = 0; c < n; ++c) {
        uint64_t k = 0;
        for (const auto &pe : panels) k += pe.cp[(size_t)c + 1] - pe.cp[(size_t)c];
        colptr[(size_t)c + 1] = colptr[(size_t)c] + k;
    }
    std::vector<uint32_t> rows;
    std::vector<double> vals;
    try {
        rows.resize((size_t)nnz);
        vals.resize((size_t)nnz);
    } catch (const std::bad_alloc &) {
        return fail("Sparse GRM: host allocation of " + std::to_string(nnz) + " entries failed");
    }
    std::vector<uint64_t> cursor(colptr.begin(), colptr.end() - 1);
    for (const auto &pe : panels)
        for (int c = 0; c < n; ++c)
            for (uint64_t k = pe.cp[(size_t)c]; k < pe.cp[(size_t)c + 1]; ++k) {
                rows[(size_t)cursor[(size_t)c]] = pe.r[(size_t)k];
                vals[(size_t)cursor[(size_t)c]++] = pe.v[(size_t)k];
            }
    FILE *fh = fopen(out_path, "wb");
    if (!fh) return fail(std::string("create ") + out_path + " failed");
    const uint64_t hdr[2] = {(uint64_t)n, nnz};
    const size_t pad = (size_t)((8 - ((nnz * 4) & 7)) & 7);
    const char zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = fwrite(hdr, 8, 2, fh) == 2 && fwrite(colptr.data(), 8, colptr.size(), fh) == colptr.size() &&
              fwrite(rows.data(), 4, rows.size(), fh) == rows.size() && fwrite(zeros, 1, pad, fh) == pad &&
              fwrite(vals.data(), 8, vals.size(), fh) == vals.size();
    const int werr = ok ? 0 : errno;
    const bool closed = fclose(fh) == 0;
    if (!ok || !closed) {
        const int e = ok ? errno : werr;
        remove(out_path);
        return fail(std::string("write sparse GRM file failed: ") + out_path + " (" + std::to_string(nnz) + " entries, " +
                    strerror(e) + ")");
    }
    if (out_nnz) *out_nnz = nnz;
    return 0;
}
}  // namespace

// Several processes (one per GPU) build ONE sparse GRM: process `part` of `nparts` computes the row panels p = part (mod nparts)
// in its next jx_spgrm_packed_to_jxgrm call and leaves them in `<out>.part<part>`; after a barrier ONE process calls
// jx_spgrm_merge_parts(out, n, nparts).  (0, 1): off.
extern "C" int jx_spgrm_set_part(int part, int nparts) {
    if (nparts < 1 || part < 0 || part >= nparts) return fail("jx_spgrm_set_part: bad part / nparts");
    g_spgrm_part = part;
    g_spgrm_nparts = nparts;
    return 0;
}

extern "C" int jx_spgrm_merge_parts(const char *out_path, int n, int nparts, int64_t *out_nnz) {
    if (!out_path || !out_path[0] || n <= 0 || nparts < 1) return fail("jx_spgrm_merge_parts: bad arguments");
    std::vector<PanelEntries> panels;
    for (int k = 0; k < nparts; ++k) {
        const std::string path = std::string(out_path) + ".part" + std::to_string(k);
        FILE *fh = fopen(path.c_str(), "rb");
        if (!fh) return fail("jx_spgrm_merge_parts: " + path + " is missing");
        uint64_t hdr[2] = {0, 0};
        bool ok = fread(hdr, 8, 2, fh) == 2 && hdr[0] == (uint64_t)n;
        for (uint64_t q = 0; ok && q < hdr[1]; ++q) {
            PanelEntries pe;
            uint64_t idx = 0;
            pe.cp.resize((size_t)n + 1);
            ok = fread(&idx, 8, 1, fh) == 1 && fread(pe.cp.data(), 8, pe.cp.size(), fh) == pe.cp.size();
            if (!ok) break;
            pe.index = (int64_t)idx;
            const uint64_t pn = pe.cp[(size_t)n];
            pe.r.resize((size_t)pn);
            pe.v.resize((size_t)pn);
            ok = fread(pe.r.data(), 4, (size_t)pn, fh) == (size_t)pn && fread(pe.v.data(), 8, (size_t)pn, fh) == (size_t)pn;
            panels.push_back(std::move(pe));
        }
        fclose(fh);
        if (!ok) return fail("jx_spgrm_merge_parts: " + path + " is truncated or belongs to another matrix");
    }
    std::sort(panels.begin(), panels.end(), [](const PanelEntries &a, const PanelEntries &b) { return a.index < b.index; });
    for (size_t q = 1; q < panels.size(); ++q)
        if (panels[q].index == panels[q - 1].index) return fail("jx_spgrm_merge_parts: a panel appears twice");
    uint64_t nnz = 0;
    if (spgrm_merge_write(panels, n, out_path, &nnz)) return 1;
    for (int k = 0; k < nparts; ++k) remove((std::string(out_path) + ".part" + std::to_string(k)).c_str());
    if (out_nnz) *out_nnz = (int64_t)nnz;
    return 0;
}

extern "C" int jx_spgrm_packed_to_jxgrm(const uint8_t *packed, int64_t m, int n_samples, const uint8_t *row_flip,
                                        const float *row_maf, const int64_t *sample_indices, int n_sel, int method,
                                        double threshold, int abs_threshold, int stream_denominator,
                                        const char *out_path, int64_t *out_n, int64_t *out_nnz) {
    // validate_spgrm_inputs (spgrm.rs:2858-2915)
    if (n_samples <= 0) return fail("Sparse GRM requires n_samples > 0");
    if (method != 1 && method != 2)
        return fail("Sparse GRM method must be 1 (centered) or 2 (standardized); got " + std::to_string(method));
    if (!isfinite(threshold)) return fail("Sparse GRM threshold must be finite");
    if (sample_indices && n_sel <= 0) return fail("Sparse GRM sample_indices must not be empty");
    if (m <= 0) return fail("Sparse GRM requires at least one SNP row");
    if (!out_path || !out_path[0]) return fail("Sparse GRM output prefix must not be empty");
    SampleSel sel;
    if (make_sample_sel(sample_indices, n_sel, n_samples, sel)) return 1;
    const int n = sel.n;
    // packed route: `centered_varsum_from_packed` (:2917-2979); stream route: sum of 2p(1-p) in f64 whatever the
    // sample selection (:3973-3989)
    const double D = grm_varsum(row_maf, m, method, sel.identity || stream_denominator != 0);
    if (!(isfinite(D) && D > 0.0))
        return fail(method == 1 ? "Sparse GRM centered denominator is not positive"
                                : "Sparse GRM denominator is not positive");
    std::vector<float> lut((size_t)m * 4);
    for (int64_t j = 0; j < m; ++j) grm_lut_from_maf(row_maf[j], row_flip[j] != 0, method, &lut[(size_t)j * 4]);
    DevBuf p32, dlut, acc, work, dcolptr, drows, dvals;
    if (stage_p32(packed, m, n_samples, sel, p32)) return 1;
    if (dlut.alloc(lut.size() * sizeof(float))) return 1;
    JX_HIP(hipMemcpy(dlut.p, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    const int64_t npad = (int64_t)num_tiles(n) * JXG_TILE;
    const double inv = 1.0 / D;
    std::vector<uint64_t> colptr((size_t)n + 1);
    std::vector<uint32_t> rows;
    std::vector<double> vals;
    uint64_t nnz = 0;
    // Row panels when the n x n f64 accumulator is too large for HBM (JXGPU_SPGRM_ACC_GB, default 96) or when
    // JXGPU_SPGRM_PANEL_ROWS asks for them: the GRM is computed and thresholded 256-row bands at a time (tile rows of the
    // lower triangle), every panel yields the CSC entries of its rows, and the panels are merged column by column on the
    // host (rows ascend with the panels, so the order inside a column is kept).  One pass over the payload per panel.
    const char *env_rows = getenv("JXGPU_SPGRM_PANEL_ROWS");
    const double acc_gb = getenv("JXGPU_SPGRM_ACC_GB") ? atof(getenv("JXGPU_SPGRM_ACC_GB")) : 96.0;
    int64_t panel_rows = 0;
    if (env_rows && atoll(env_rows) > 0) panel_rows = atoll(env_rows);
    else if ((double)npad * (double)npad * 8.0 > acc_gb * 1073741824.0) panel_rows = (int64_t)(32.0 * 1073741824.0 / (8.0 * npad));
    const int nparts = g_spgrm_nparts, part = g_spgrm_part;
    if (nparts > 1 && panel_rows <= 0)      // several processes: about four panels each (the same plan on every one of them)
        panel_rows = std::max<int64_t>(256, ((int64_t)n / (4 * nparts)) / 256 * 256);
    if (panel_rows > 0) {
        panel_rows = std::max<int64_t>(256, (panel_rows / 256) * 256);
        const int nbands = (n + 255) / 256;
        const int bands_per = (int)(panel_rows / 256);
        if (acc.alloc(sizeof(double) * (size_t)(panel_rows * npad))) return 1;
        if (work.alloc((size_t)((int64_t)bands_per * n * 4 + 16))) return 1;
        if (dcolptr.alloc(sizeof(uint64_t) * ((size_t)n + 1))) return 1;
        std::vector<PanelEntries> panels;
        int64_t pidx = 0;
        for (int b0 = 0; b0 < nbands; b0 += bands_per, ++pidx) {
            // dealt back and forth (0 .. nparts-1, nparts-1 .. 0, ...): a panel's cost grows with its row index (lower triangle)
            const int64_t round = pidx / nparts, pos = pidx % nparts;
            if (((round & 1) ? nparts - 1 - pos : pos) != part) continue;          // another process's panel
            const int b1 = std::min(nbands, b0 + bands_per);
            const int t0 = b0 * 2, t1 = std::min((int)num_tiles(n), b1 * 2);       // 128-row tiles of the bands
            JX_HIP(hipMemset(acc.p, 0, sizeof(double) * (size_t)((int64_t)(t1 - t0) * JXG_TILE * npad)));
            if (jxg_grm_accumulate_rows(p32.as<uint8_t>(), m, n, nullptr, dlut.as<float>(), m, acc.as<double>(), 0, 2, t0, t1,
                                        nullptr))
                return 1;
            if (jxg_spgrm_count_bands(acc.as<double>(), n, inv, threshold, abs_threshold, b0, b1, work.p,
                                      dcolptr.as<uint64_t>(), nullptr))
                return 1;
            PanelEntries pe;
            pe.index = pidx;
            pe.cp.resize((size_t)n + 1);
            JX_HIP(hipMemcpy(pe.cp.data(), dcolptr.p, sizeof(uint64_t) * pe.cp.size(), hipMemcpyDeviceToHost));
            const uint64_t pn = pe.cp[(size_t)n];
            if (pn) {
                DevBuf pr, pv;
                if (pr.alloc(sizeof(uint32_t) * (size_t)pn) || pv.alloc(sizeof(double) * (size_t)pn)) return 1;
                if (jxg_spgrm_fill_bands(acc.as<double>(), n, inv, threshold, abs_threshold, b0, b1, work.p,
                                         dcolptr.as<uint64_t>(), pr.as<uint32_t>(), pv.as<double>(), nullptr))
                    return 1;
                try {
                    pe.r.resize((size_t)pn);
                    pe.v.resize((size_t)pn);
                } catch (const std::bad_alloc &) {
                    return fail("Sparse GRM: host allocation of " + std::to_string(pn) + " entries failed");
                }
                JX_HIP(hipMemcpy(pe.r.data(), pr.p, sizeof(uint32_t) * (size_t)pn, hipMemcpyDeviceToHost));
                JX_HIP(hipMemcpy(pe.v.data(), pv.p, sizeof(double) * (size_t)pn, hipMemcpyDeviceToHost));
            }
            nnz += pn;
            panels.push_back(std::move(pe));
        }
        p32.release();
        if (nparts > 1) {
            // this process's panels only: left in `<out>.part<k>` for jx_spgrm_merge_parts
            const std::string path = std::string(out_path) + ".part" + std::to_string(part);
            FILE *fh = fopen(path.c_str(), "wb");
            if (!fh) return fail("create " + path + " failed");
            const uint64_t hdr[2] = {(uint64_t)n, (uint64_t)panels.size()};
            bool ok = fwrite(hdr, 8, 2, fh) == 2;
            for (const auto &pe : panels) {
                const uint64_t idx = (uint64_t)pe.index;
                ok = ok && fwrite(&idx, 8, 1, fh) == 1 && fwrite(pe.cp.data(), 8, pe.cp.size(), fh) == pe.cp.size() &&
                     fwrite(pe.r.data(), 4, pe.r.size(), fh) == pe.r.size() && fwrite(pe.v.data(), 8, pe.v.size(), fh) == pe.v.size();
            }
            const bool closed = fclose(fh) == 0;
            if (!ok || !closed) {
                remove(path.c_str());
                return fail("write sparse GRM part file failed: " + path);
            }
            if (out_n) *out_n = n;
            if (out_nnz) *out_nnz = (int64_t)nnz;
            return 0;
        }
        uint64_t total = 0;
        if (spgrm_merge_write(panels, n, out_path, &total)) return 1;
        if (out_n) *out_n = n;
        if (out_nnz) *out_nnz = (int64_t)total;
        return 0;
    } else {
        if (acc.alloc(sizeof(double) * (size_t)(npad * npad))) return 1;
        JX_HIP(hipMemset(acc.p, 0, sizeof(double) * (size_t)(npad * npad)));
        // precision 2: rows with missing calls on the general kernel, as in the row-panel form above (one file whatever the
        // memory plan)
        if (jxg_grm_accumulate(p32.as<uint8_t>(), m, n, nullptr, dlut.as<float>(), m, acc.as<double>(), 0, 2, nullptr))
            return 1;
        p32.release();
        if (work.alloc((size_t)jxg_spgrm_work_bytes(n))) return 1;
        if (dcolptr.alloc(sizeof(uint64_t) * ((size_t)n + 1))) return 1;
        if (jxg_spgrm_count(acc.as<double>(), n, inv, threshold, abs_threshold, work.p, dcolptr.as<uint64_t>(), nullptr))
            return 1;
        JX_HIP(hipMemcpy(colptr.data(), dcolptr.p, sizeof(uint64_t) * colptr.size(), hipMemcpyDeviceToHost));
        nnz = colptr[(size_t)n];
        try {   // up to n (n + 1) / 2 entries with a negative cut-off: 12 bytes each on the host
            rows.resize((size_t)nnz);
            vals.resize((size_t)nnz);
        } catch (const std::bad_alloc &) {
            return fail("Sparse GRM: host allocation of " + std::to_string(nnz) + " entries failed");
        }
        if (nnz) {
            if (drows.alloc(sizeof(uint32_t) * (size_t)nnz) || dvals.alloc(sizeof(double) * (size_t)nnz)) return 1;
            if (jxg_spgrm_fill(acc.as<double>(), n, inv, threshold, abs_threshold, work.p, dcolptr.as<uint64_t>(),
                               drows.as<uint32_t>(), dvals.as<double>(), nullptr))
                return 1;
            JX_HIP(hipMemcpy(rows.data(), drows.p, sizeof(uint32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
            JX_HIP(hipMemcpy(vals.data(), dvals.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
        }
    }
    // write_sparse_grm_csc (:3745-3767): u64 n, u64 nnz, col_ptr, row_indices, zero padding to 8 bytes, values (LE)
    FILE *fh = fopen(out_path, "wb");
    if (!fh) return fail(std::string("create ") + out_path + " failed");
    const uint64_t hdr[2] = {(uint64_t)n, nnz};
    const size_t pad = (size_t)((8 - ((nnz * 4) & 7)) & 7);
    const char zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = fwrite(hdr, 8, 2, fh) == 2 && fwrite(colptr.data(), 8, colptr.size(), fh) == colptr.size() &&
              fwrite(rows.data(), 4, rows.size(), fh) == rows.size() && fwrite(zeros, 1, pad, fh) == pad &&
              fwrite(vals.data(), 8, vals.size(), fh) == vals.size();
    const int werr = ok ? 0 : errno;
    const bool closed = fclose(fh) == 0;
    if (!ok || !closed) {
        const int e = ok ? errno : werr;
        remove(out_path);
        return fail(std::string("write sparse GRM file failed: ") + out_path + " (" + std::to_string(nnz) + " entries, " +
                    strerror(e) + ")");
    }
    if (out_n) *out_n = n;
    if (out_nnz) *out_nnz = (int64_t)nnz;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// grm_stream_bed_f32 on an in-memory payload (src/stats/grm.rs:1465-1536 prepare, 4690-5455 driver)
// ---------------------------------------------------------------------------------------------------
extern "C" int jx_grm_stream_payload_f32(const uint8_t *packed, int64_t m, int n_samples, int method,
                                         float maf_threshold, float max_missing_rate, float het_threshold,
                                         float *out_k, int64_t *out_eff_m, uint8_t *out_keep) {
    if (n_samples <= 0) return fail("n_samples must be > 0");
    if (method != 1 && method != 2) return fail("unsupported method=" + std::to_string(method));
    if (m <= 0) return fail("No SNPs remained after filtering; GRM is empty.");
    // grm.rs:4709-4711 threshold clamps
    const float maf_thr = fminf(fmaxf(maf_threshold, 0.0f), 0.5f);
    const float miss_thr = fminf(fmaxf(max_missing_rate, 0.0f), 1.0f);
    const float het_thr = fminf(fmaxf(het_threshold, 0.0f), 1.0f);
    SampleSel sel;
    make_sample_sel(nullptr, 0, n_samples, sel);
    DevBuf p32, dcnt;
    if (stage_p32(packed, m, n_samples, sel, p32)) return 1;
    if (dcnt.alloc(sizeof(int32_t) * 3 * (size_t)m)) return 1;
    if (jxg_row_counts_p32(p32.as<uint8_t>(), m, n_samples, dcnt.as<int32_t>(), nullptr)) return 1;
    std::vector<int32_t> cnt((size_t)m * 3);
    JX_HIP(hipMemcpy(cnt.data(), dcnt.p, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));

    std::vector<int32_t> rows;
    std::vector<float> lut;
    rows.reserve(m);
    lut.reserve((size_t)m * 4);
    double varsum = 0.0;
    const double eps = (double)1e-12f;
    for (int64_t j = 0; j < m; ++j) {
        if (out_keep) out_keep[j] = 0;
        const int64_t missing = cnt[j * 3], het = cnt[j * 3 + 1], hom = cnt[j * 3 + 2];
        const int64_t nm = n_samples - missing;
        if (het_thr > 0.0f && nm > 0) {
            const double het_rate = (double)het / (double)nm;
            if (het_rate > (double)het_thr) continue;
        }
        const double missing_rate = 1.0 - ((double)nm / (double)n_samples);
        if (missing_rate > (double)miss_thr) continue;
        float mean_g, sc;
        bool flip = false;
        double var = 0.0;
        if (nm == 0) {
            if (maf_thr > 0.0f) continue;
            mean_g = 0.0f;
            sc = (method == 2) ? 0.0f : 1.0f;
        } else {
            double alt_sum = (double)(het + 2 * hom);
            double alt_freq = alt_sum / (2.0 * (double)nm);
            flip = alt_freq > 0.5;
            if (flip) {
                alt_sum = 2.0 * (double)nm - alt_sum;
                alt_freq = alt_sum / (2.0 * (double)nm);
            }
            const double maf = fmin(alt_freq, 1.0 - alt_freq);
            if (maf < (double)maf_thr) continue;
            mean_g = (float)(alt_sum / (double)nm);
            var = fmax(2.0 * alt_freq * (1.0 - alt_freq), 0.0);
            sc = 1.0f;
            if (method == 2) sc = (var > eps) ? (float)(1.0 / sqrt(var)) : 0.0f;
        }
        if (out_keep) out_keep[j] = 1;
        rows.push_back((int32_t)j);
        varsum += var;
        const float g0 = flip ? 2.0f : 0.0f, g2 = flip ? 0.0f : 2.0f;
        // decode.rs:446-461 `apply_prepared_grm_stream_row_copy_f32`
        lut.push_back((g0 - mean_g) * sc);
        lut.push_back(0.0f);
        lut.push_back((1.0f - mean_g) * sc);
        lut.push_back((g2 - mean_g) * sc);
    }
    const int64_t eff = (int64_t)rows.size();
    if (out_eff_m) *out_eff_m = eff;
    if (eff == 0) return fail("No SNPs remained after filtering; GRM is empty.");
    const double D = (method == 1) ? varsum : (double)eff;
    if (!(isfinite(D) && D > 0.0)) return fail("invalid centered GRM denominator: sum(2p(1-p)) <= 0");

    DevBuf drows, dlut, acc, dout;
    if (drows.alloc(rows.size() * sizeof(int32_t))) return 1;
    JX_HIP(hipMemcpy(drows.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (dlut.alloc(lut.size() * sizeof(float))) return 1;
    JX_HIP(hipMemcpy(dlut.p, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    const int n = n_samples;
    const int64_t npad = (int64_t)num_tiles(n) * JXG_TILE;
    if (acc.alloc(sizeof(double) * (size_t)(npad * npad))) return 1;
    JX_HIP(hipMemset(acc.p, 0, sizeof(double) * (size_t)(npad * npad)));
    if (jxg_grm_accumulate(p32.as<uint8_t>(), m, n, drows.as<int32_t>(), dlut.as<float>(), eff, acc.as<double>(), 0, 0,
                           nullptr))
        return 1;
    if (dout.alloc(sizeof(float) * (size_t)n * (size_t)n)) return 1;
    if (jxg_grm_finalize(acc.as<double>(), n, 1.0 / D, dout.p, 0, nullptr)) return 1;
    JX_HIP(hipMemcpy(out_k, dout.p, sizeof(float) * (size_t)n * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// lm_block_assoc_packed (src/stats/glm.rs:3550-3860): the plain LM scan the mixed-model routes fall back to
// ---------------------------------------------------------------------------------------------------
// Host half of the packed and the dense LM scan (janusx_amd/pipeline.py): r_y = y - X (C X'y), y'M_X y, and [X | r_y]
// rounded through f32 (glm.rs:3635-3672).  xr_out (n, q0 + 1).
extern "C" int jx_lm_residualize(const double *y, const double *x, const double *ixx, int n, int q0, double *xr_out,
                                 double *yy_r_out) {
    if (n <= 0 || q0 < 0) return fail("X.n_rows must equal len(y)");
    if (n <= q0 + 1) return fail("n too small: require n > q0+1, got n=" + std::to_string(n) + ", q0=" + std::to_string(q0));
    std::vector<double> xy((size_t)q0, 0.0), cxy((size_t)q0, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < q0; ++j) xy[j] += x[(size_t)i * q0 + j] * y[i];
    for (int i = 0; i < q0; ++i) {
        double acc = 0.0;
        for (int j = 0; j < q0; ++j) acc += ixx[(size_t)i * q0 + j] * xy[j];
        cxy[i] = acc;
    }
    double yy = 0.0;
    const int ld = q0 + 1;
    for (int i = 0; i < n; ++i) {
        double pred = 0.0;
        for (int j = 0; j < q0; ++j) pred += x[(size_t)i * q0 + j] * cxy[j];
        const double resid = y[i] - pred;
        yy += resid * resid;
        for (int j = 0; j < q0; ++j) xr_out[(size_t)i * ld + j] = (double)(float)x[(size_t)i * q0 + j];
        xr_out[(size_t)i * ld + q0] = (double)(float)resid;
    }
    *yy_r_out = yy;
    return 0;
}

// ---- association TSV writer (host) ------------------------------------------------------------------------------------
// Native counterpart of the reference's row formatter + writer (src/io/assoc2tsv.rs:430-548, `AsyncTsvWriter`
// src/stats/common.rs:374): the numeric columns of every row are formatted here with Rust's float text (`{:.4}`,
// `{:.4e}` / `{:.6e}` with an unpadded exponent, `NaN`, `inf`), the per-row prefix `chrom\tpos\tsnp\tallele0\tallele1`
// comes from the caller as one byte blob with offsets.  stats: (rows, ncol) f64, ncol = 3 [beta, se, p], 4 [.., plrt] or
// 6 [beta, se, p, lambda, ml, plrt].  Writes `path` directly (the caller renames a temp file).
namespace {
inline char *put_str(char *o, const char *t) {
    while (*t) *o++ = *t++;
    return o;
}
inline char *put_fixed4(char *o, double v) {
    if (v != v) return put_str(o, "NaN");
    if (std::isinf(v)) return put_str(o, v > 0 ? "inf" : "-inf");
    // Rust's {:.4} prints every digit of a huge finite value (up to 309 before the point): the caller reserves
    // kRowReserve bytes per row, enough for four such fields
    const int len = snprintf(o, 336, "%.4f", v);
    return o + (len < 336 ? len : 335);
}
constexpr size_t kRowReserve = 2048;   // 4 fixed-point fields of <= 336 bytes + 5 exponent fields + tabs
inline char *put_exp(char *o, double v, int prec) {
    if (v != v) return put_str(o, "NaN");
    if (std::isinf(v)) return put_str(o, v > 0 ? "inf" : "-inf");
    char tmp[64];
    const int len = snprintf(tmp, sizeof(tmp), "%.*e", prec, v);
    int epos = len - 1;
    while (epos > 0 && tmp[epos] != 'e') --epos;
    memcpy(o, tmp, (size_t)epos + 1);          // mantissa and 'e'
    o += epos + 1;
    const char *x = tmp + epos + 1;
    if (*x == '-') *o++ = '-';
    if (*x == '-' || *x == '+') ++x;
    while (*x == '0' && x[1] != 0) ++x;        // Rust prints the exponent without padding: e-3, e0, e12
    return put_str(o, x);
}
}  // namespace

extern "C" int64_t jx_assoc_tsv_append(const char *path, const char *prefix_blob, const int64_t *prefix_off, int64_t rows,
                                       const float *af, const float *miss, const double *stats, int ncol, int append);

extern "C" int64_t jx_assoc_tsv_write(const char *path, const char *prefix_blob, const int64_t *prefix_off, int64_t rows,
                                      const float *af, const float *miss, const double *stats, int ncol) {
    return jx_assoc_tsv_append(path, prefix_blob, prefix_off, rows, af, miss, stats, ncol, 0);
}

// append bit 0: the rows go behind what `path` holds already, without a header (the block-wise writer of the streaming
// scan: header + first block with 0, every later block with 1); bit 1 (+2): `miss` holds COUNTS of missing samples and is
// printed as an integer (`AssocMissValue::Count`, src/io/assoc2tsv.rs:452-458: the LM routes) instead of a rate `{:.4}`
extern "C" int64_t jx_assoc_tsv_append(const char *path, const char *prefix_blob, const int64_t *prefix_off, int64_t rows,
                                       const float *af, const float *miss, const double *stats, int ncol, int append_flags) {
    const int append = append_flags & 1;
    const bool miss_count = (append_flags & 2) != 0;
    if (ncol != 3 && ncol != 4 && ncol != 6) {
        fail("unsupported GWAS result column count: " + std::to_string(ncol) + " (expected 3, 4, or 6)");
        return -1;
    }
    FILE *fh = fopen(path, append ? "ab" : "wb");
    if (!fh) {
        fail(std::string("cannot open ") + path + " for writing");
        return -1;
    }
    static const char *h3 = "chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\n";
    static const char *h4 = "chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\tplrt\n";
    static const char *h6 = "chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\tlambda\tml\tplrt\n";
    if (!append) fputs(ncol == 6 ? h6 : (ncol == 4 ? h4 : h3), fh);
    std::vector<char> buf((size_t)1 << 20);
    size_t used = 0;
    const double min_pos = 2.2250738585072014e-308;
    for (int64_t i = 0; i < rows; ++i) {
        const int64_t plen = prefix_off[i + 1] - prefix_off[i];
        if (used + (size_t)plen + kRowReserve > buf.size()) {
            if (fwrite(buf.data(), 1, used, fh) != used) {
                fclose(fh);
                fail(std::string("write to ") + path + " failed");
                return -1;
            }
            used = 0;
            if ((size_t)plen + kRowReserve > buf.size()) buf.resize((size_t)plen + 2 * kRowReserve);
        }
        char *o = buf.data() + used;
        memcpy(o, prefix_blob + prefix_off[i], (size_t)plen);
        o += plen;
        const double *r = stats + i * ncol;
        const double beta = r[0], se = r[1], p = r[2];
        double chisq, pv;
        if (std::isfinite(beta) && std::isfinite(se) && se > 0.0) {      // sanitize_assoc_pvalue, src/math/linalg.rs:111-121
            const double z = beta / se;
            chisq = z * z;
            pv = std::isfinite(p) ? std::min(std::max(p, min_pos), 1.0) : 1.0;
        } else {
            chisq = NAN;
            pv = 1.0;
        }
        *o++ = '\t'; o = put_fixed4(o, (double)af[i]);
        *o++ = '\t';
        if (miss_count) o += snprintf(o, 32, "%lld", (long long)llround((double)miss[i]));
        else o = put_fixed4(o, (double)miss[i]);
        *o++ = '\t'; o = put_fixed4(o, beta);
        *o++ = '\t'; o = put_fixed4(o, se);
        *o++ = '\t'; o = put_exp(o, chisq, 4);
        *o++ = '\t'; o = put_exp(o, pv, 4);
        if (ncol == 6) {
            *o++ = '\t'; o = put_exp(o, r[3], 6);
            *o++ = '\t'; o = put_exp(o, r[4], 6);
            *o++ = '\t'; o = put_exp(o, r[5], 4);
        } else if (ncol == 4) {
            *o++ = '\t'; o = put_exp(o, r[3], 4);
        }
        *o++ = '\n';
        used = (size_t)(o - buf.data());
    }
    const bool ok = fwrite(buf.data(), 1, used, fh) == used;
    if (fclose(fh) != 0 || !ok) {
        fail(std::string("write to ") + path + " failed");
        return -1;
    }
    return rows;
}

// ---- LD pruning, host half (src/stats/ld.rs:270-402, 545-549): windows and the strict greedy.  No GPU call.
//
// Rows are put in chromosome-grouped order (groups by first appearance of the code, file order inside a group), so that a
// chromosome is a contiguous range of "positions" p and every window is a range [p, win_end[p]) of them; all indices below are
// such positions.  order[p] = file row.  chrom_off[0 .. *n_chrom] bounds the groups.  win_end[p] = end (exclusive) of the window
// that starts at p, 0 where the reference starts none (p is not a multiple of the step inside its chromosome, lies behind the
// window whose end reached the chromosome's last row, or the chromosome has one row).  band_end[p] = the largest window end
// over the windows that contain p (p + 1 where none does).
//
// Why band_end bounds every pair the greedy can ask for: the greedy evaluates a pair (li, lj) only inside one window, with
// bs <= li < lj < end of that window.  That window contains li, so lj < end <= band_end[li].  Within a chromosome the windows
// are visited with growing start, so the largest end over the windows that start at or before p is a running maximum; if it
// exceeds p, the window that attains it starts at or before p and ends behind p, so it contains p and the maximum is band_end[p].
extern "C" int jx_ld_window_ends(const int32_t *chrom_codes, const int64_t *positions, int64_t m, int64_t window_bp,
                                 int64_t window_variants, int64_t step_variants, int64_t *order, int64_t *chrom_off, int64_t *n_chrom,
                                 int64_t *win_end, int64_t *band_end) {
    if (m < 0) return fail("jx_ld_window_ends: m must be >= 0");
    if (step_variants <= 0) return fail("step_variants must be > 0");
    if (window_bp <= 0 && window_variants <= 0) return fail("provide one of window_bp or window_variants");
    const bool use_bp = window_bp > 0;                        // the bp window wins when both are given
    // groups by first appearance
    std::vector<int32_t> codes;                               // code of group g
    std::vector<int64_t> group((size_t)m), count;
    {
        std::vector<std::pair<int32_t, int64_t>> seen;        // sorted (code, group)
        for (int64_t i = 0; i < m; ++i) {
            const int32_t c = chrom_codes[i];
            auto it = std::lower_bound(seen.begin(), seen.end(), std::make_pair(c, (int64_t)-1));
            if (it == seen.end() || it->first != c) {
                it = seen.insert(it, std::make_pair(c, (int64_t)codes.size()));
                codes.push_back(c);
                count.push_back(0);
            }
            group[(size_t)i] = it->second;
            ++count[(size_t)it->second];
        }
    }
    const int64_t ng = (int64_t)codes.size();
    *n_chrom = ng;
    chrom_off[0] = 0;
    for (int64_t g = 0; g < ng; ++g) chrom_off[g + 1] = chrom_off[g] + count[(size_t)g];
    {
        std::vector<int64_t> fill(chrom_off, chrom_off + ng);
        for (int64_t i = 0; i < m; ++i) order[fill[(size_t)group[(size_t)i]]++] = i;
    }
    for (int64_t p = 0; p < m; ++p) {
        win_end[p] = 0;
        band_end[p] = p + 1;
    }
    auto sat_add = [](int64_t a, int64_t b) {
        int64_t r;
        return __builtin_add_overflow(a, b, &r) ? (b > 0 ? INT64_MAX : INT64_MIN) : r;
    };
    auto sat_sub = [](int64_t a, int64_t b) {
        int64_t r;
        return __builtin_sub_overflow(a, b, &r) ? (b > 0 ? INT64_MIN : INT64_MAX) : r;
    };
    for (int64_t g = 0; g < ng; ++g) {
        const int64_t c0 = chrom_off[g], l = chrom_off[g + 1] - c0;
        if (l <= 1) continue;
        auto pos = [&](int64_t k) { return positions[order[c0 + k]]; };
        bool pos_sorted = true;
        for (int64_t k = 1; k < l; ++k)
            if (pos(k) < pos(k - 1)) {
                pos_sorted = false;
                break;
            }
        int64_t bp_end_ptr = 1, block_start = 0, run_max = 0, next_band = 0;
        while (block_start < l) {
            int64_t end;
            if (use_bp) {
                if (pos_sorted) {
                    if (bp_end_ptr < block_start + 1) bp_end_ptr = block_start + 1;
                    const int64_t target = sat_add(pos(block_start), window_bp);
                    while (bp_end_ptr < l && pos(bp_end_ptr) <= target) ++bp_end_ptr;
                    end = bp_end_ptr;
                } else {
                    int64_t e = block_start + 1;
                    const int64_t p0 = pos(block_start);
                    while (e < l) {
                        const int64_t d = sat_sub(pos(e), p0);
                        if (d <= window_bp) ++e;
                        else if (pos(e) > p0) break;
                        else ++e;
                    }
                    end = e;
                }
            } else {
                end = std::min(sat_add(block_start, window_variants), l);
            }
            // rows in front of this window's start have seen every window that can contain them
            for (; next_band < block_start; ++next_band)
                if (run_max > next_band) band_end[c0 + next_band] = c0 + run_max;
            run_max = std::max(run_max, end);
            win_end[c0 + block_start] = c0 + end;
            if (end >= l) break;
            block_start = sat_add(block_start, step_variants);
        }
        for (; next_band < l; ++next_band)
            if (run_max > next_band) band_end[c0 + next_band] = c0 + run_max;
    }
    return 0;
}

// ---- LD scores, host half (`jx gstats -ldsc`; src/stats/gstats.rs:873-953): chromosome groups, their sort and the two-sided
// windows.  No GPU call.  All rows of a code form one group wherever they lie in the file (groups by first appearance of the
// code; the reference's order of groups is that of a hash map and decides nothing).  A group is stably sorted by position, for a
// cM window by cM and then by position (`build_sorted_chrom_groups`, :873-896), and `compute_window_bounds` (:898-953) runs on it:
// kind 0 = variants (w_int rows to either side), 1 = base pairs (w_int), 2 = cM (w_cm).  order[p] = file row, chrom_off[0 .. *n_chrom]
// bounds the groups, and row order[p] adds the rows order[start[p] .. end[p]) (positions of the order, its own among them).
extern "C" int jx_ldsc_window_bounds(const int32_t *chrom_codes, const int64_t *positions, const double *cm_positions, int64_t m,
                                     int kind, int64_t w_int, double w_cm, int64_t *order, int64_t *chrom_off, int64_t *n_chrom,
                                     int64_t *start, int64_t *end) {
    if (m < 0) return fail("jx_ldsc_window_bounds: m must be >= 0");
    if (kind < 0 || kind > 2) return fail("jx_ldsc_window_bounds: kind must be 0 (variants), 1 (bp) or 2 (cM)");
    if (kind != 2 && w_int <= 0) return fail("jx_ldsc_window_bounds: the window must be > 0");
    if (kind == 2 && !(std::isfinite(w_cm) && w_cm > 0.0)) return fail("jx_ldsc_window_bounds: the cM window must be finite and > 0");
    if (kind == 2) {
        if (!cm_positions) return fail("jx_ldsc_window_bounds: a cM window needs cM positions");
        for (int64_t i = 0; i < m; ++i)
            if (std::isnan(cm_positions[i]))
                return fail("cM value of row " + std::to_string(i) + " is NaN: a cM window needs an ordered cM column");
    }
    std::vector<int64_t> group((size_t)m), count;
    {
        std::vector<std::pair<int32_t, int64_t>> seen;        // sorted (code, group)
        for (int64_t i = 0; i < m; ++i) {
            const int32_t c = chrom_codes[i];
            auto it = std::lower_bound(seen.begin(), seen.end(), std::make_pair(c, (int64_t)-1));
            if (it == seen.end() || it->first != c) {
                it = seen.insert(it, std::make_pair(c, (int64_t)count.size()));
                count.push_back(0);
            }
            group[(size_t)i] = it->second;
            ++count[(size_t)it->second];
        }
    }
    const int64_t ng = (int64_t)count.size();
    *n_chrom = ng;
    chrom_off[0] = 0;
    for (int64_t g = 0; g < ng; ++g) chrom_off[g + 1] = chrom_off[g] + count[(size_t)g];
    {
        std::vector<int64_t> fill(chrom_off, chrom_off + ng);
        for (int64_t i = 0; i < m; ++i) order[fill[(size_t)group[(size_t)i]]++] = i;
    }
    auto sat_sub = [](int64_t a, int64_t b) {
        int64_t r;
        return __builtin_sub_overflow(a, b, &r) ? (b > 0 ? INT64_MIN : INT64_MAX) : r;
    };
    for (int64_t g = 0; g < ng; ++g) {
        const int64_t c0 = chrom_off[g], n = chrom_off[g + 1] - c0;
        int64_t *grp = order + c0;
        if (kind == 2)
            std::stable_sort(grp, grp + n, [&](int64_t a, int64_t b) {
                if (cm_positions[a] != cm_positions[b]) return cm_positions[a] < cm_positions[b];
                return positions[a] < positions[b];
            });
        else
            std::stable_sort(grp, grp + n, [&](int64_t a, int64_t b) { return positions[a] < positions[b]; });
        int64_t *starts = start + c0, *ends = end + c0;
        if (kind == 0) {
            for (int64_t i = 0; i < n; ++i) {
                starts[i] = i > w_int ? i - w_int : 0;
                ends[i] = w_int >= n - i - 1 ? n : i + w_int + 1;   // min(n, i + w + 1) without overflow
            }
        } else if (kind == 1) {
            const int64_t w = w_int;
            int64_t left = 0, right = 0;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t pos_i = positions[grp[i]];
                while (left < i && sat_sub(pos_i, positions[grp[left]]) > w) ++left;
                if (right < i) right = i;
                while (right + 1 < n && sat_sub(positions[grp[right + 1]], pos_i) <= w) ++right;
                starts[i] = left;
                ends[i] = right + 1;
            }
        } else {
            const double w = w_cm, eps = 1e-12;
            int64_t left = 0, right = 0;
            for (int64_t i = 0; i < n; ++i) {
                const double cm_i = cm_positions[grp[i]];
                while (left < i && (cm_i - cm_positions[grp[left]]) > w + eps) ++left;
                if (right < i) right = i;
                while (right + 1 < n && (cm_positions[grp[right + 1]] - cm_i) <= w + eps) ++right;
                starts[i] = left;
                ends[i] = right + 1;
            }
        }
        for (int64_t i = 0; i < n; ++i) {                     // positions of the whole order
            starts[i] += c0;
            ends[i] += c0;
        }
    }
    return 0;
}

// The strict greedy over the windows that start at the positions [ws0, ws1), from a band mask of the rows [r0, r1) in the
// layout of `jxg_ld_band_mask_p32`: bit (lj - li - 1) of row li, wpr 32-bit words per row, set where the pair is in LD.
// maf, first_unchecked and dropped are indexed by position; first_unchecked (start: p + 1) and dropped (start: 0) carry the
// state from one call to the next, so a long panel is pruned range by range with a mask of bounded size.  Every window of the
// call must lie inside one chromosome group and inside [r0, r1).
extern "C" int jx_ld_prune_greedy(const double *maf, int64_t nrows, const int64_t *chrom_off, int64_t n_chrom, const int64_t *win_end,
                                  int64_t ws0, int64_t ws1, const uint32_t *mask, int64_t r0, int64_t r1, int64_t wpr,
                                  int64_t *first_unchecked, uint8_t *dropped) {
    if (nrows < 0 || ws0 < 0 || ws1 < ws0 || ws1 > nrows) return fail("jx_ld_prune_greedy: window starts outside the rows");
    if (r0 < 0 || r1 < r0 || r1 > nrows || wpr < 1) return fail("jx_ld_prune_greedy: mask rows outside the rows");
    const double eps = 1e-12;
    int64_t g = 0;
    for (int64_t bs = ws0; bs < ws1; ++bs) {
        const int64_t end = win_end[bs];
        if (end == 0) continue;
        while (g < n_chrom && chrom_off[g + 1] <= bs) ++g;
        if (g >= n_chrom || bs < chrom_off[g] || end > chrom_off[g + 1] || end <= bs)
            return fail("jx_ld_prune_greedy: window [" + std::to_string(bs) + ", " + std::to_string(end) + ") crosses its chromosome group");
        if (bs < r0 || end > r1)
            return fail("jx_ld_prune_greedy: window [" + std::to_string(bs) + ", " + std::to_string(end) + ") outside the mask rows");
        if (end - bs - 1 > 32 * wpr) return fail("jx_ld_prune_greedy: window wider than a mask row");
        if (end <= bs + 1) continue;
        for (;;) {
            bool at_least_one_prune = false;
            for (int64_t li = bs; li < end - 1; ++li) {
                if (dropped[li]) continue;
                const int64_t scan_min = std::max(first_unchecked[li], bs + 1);
                if (scan_min >= end) {
                    first_unchecked[li] = end;
                    continue;
                }
                const uint32_t *row = mask + (li - r0) * wpr;
                bool pruned_this_round = false;
                for (int64_t lj = scan_min; lj < end; ++lj) {
                    if (dropped[lj]) continue;
                    const int64_t o = lj - li - 1;
                    if (!((row[o >> 5] >> (o & 31)) & 1u)) continue;
                    at_least_one_prune = true;
                    pruned_this_round = true;
                    if (maf[li] < (1.0 - eps) * maf[lj]) {
                        dropped[li] = 1;
                    } else {
                        dropped[lj] = 1;
                        int64_t nxt = lj + 1;
                        while (nxt < end && dropped[nxt]) ++nxt;
                        first_unchecked[li] = nxt;
                    }
                    break;
                }
                if (!pruned_this_round && !dropped[li]) first_unchecked[li] = end;
            }
            if (!at_least_one_prune) break;
        }
    }
    return 0;
}

// Greedy unrelated set of a related-pair graph (`king_prune_related_graph`, src/math/KING.rs:669-743): CSR graph (offsets n + 1,
// neighbors), a max-heap of (live degree, sample id) with lazy deletion - ties go to the larger id - popped until the top live
// degree is <= 0.  removed: in pop order; kept: ascending; both hold n slots, the counts go to n_kept / n_removed.
extern "C" int jx_king_prune(int64_t n, const int64_t *offsets, const uint32_t *neighbors, uint32_t *kept, int64_t *n_kept,
                             uint32_t *removed, int64_t *n_removed) {
    if (n < 0 || n > 0xffffffffLL) return fail("KING adjacency uses u32 sample ids; got n_samples=" + std::to_string(n) + " > 4294967295");
    if (n > 0 && offsets[0] != 0) return fail("jx_king_prune: offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail("jx_king_prune: offsets must not decrease");
        if (offsets[i + 1] - offsets[i] > 0x7fffffffLL) return fail("jx_king_prune: degree beyond int32");
        for (int64_t e = offsets[i]; e < offsets[i + 1]; ++e)
            if ((int64_t)neighbors[e] >= n)
                return fail("KING neighbor index out of range: neighbors[" + std::to_string(i) + "] contains " +
                            std::to_string(neighbors[e]) + " >= " + std::to_string(n));
    }
    std::vector<int32_t> live((size_t)n);
    std::vector<uint8_t> active((size_t)n, 1);
    std::vector<std::pair<int32_t, uint32_t>> start;
    start.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        live[i] = (int32_t)(offsets[i + 1] - offsets[i]);
        start.emplace_back(live[i], (uint32_t)i);
    }
    std::priority_queue<std::pair<int32_t, uint32_t>> heap(std::less<std::pair<int32_t, uint32_t>>(), std::move(start));
    int64_t nr = 0;
    while (!heap.empty()) {
        const std::pair<int32_t, uint32_t> top = heap.top();
        heap.pop();
        const uint32_t id = top.second;
        if (!active[id] || top.first != live[id]) continue;      // a stale entry
        if (live[id] <= 0) break;
        active[id] = 0;
        live[id] = 0;
        removed[nr++] = id;
        for (int64_t e = offsets[id]; e < offsets[id + 1]; ++e) {
            const uint32_t nb = neighbors[e];
            if (active[nb]) heap.emplace(--live[nb], nb);
        }
    }
    int64_t nk = 0;
    for (int64_t i = 0; i < n; ++i)
        if (active[i]) kept[nk++] = (uint32_t)i;
    *n_kept = nk;
    *n_removed = nr;
    return 0;
}
