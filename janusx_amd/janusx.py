"""Drop-in mirror of the reference's native module ``janusx.janusx`` for the mixed-model hot path.

Every function here has the name, argument meaning, defaults and error behaviour of the PyO3 function it
replaces (signatures: /root/reference/src/lib.rs:691-1005 registrations, ``#[pyo3(signature=...)]`` at the cited
lines) and forwards to the HIP library through the C ABI (``include/jxgpu.h``, host layer).  Arguments that only
steer CPU threading in the reference (``threads``, ``block_cols``, ``rotate_block_rows``, ``mmap_window_mb``) are
accepted and ignored; ``progress_callback(done, total)`` follows the reference's cadence on the packed association
scans (`pipeline.scan_rows` / `scan_rows_lm`: every `progress_every` rows, default one 8192-row block; an exception raised by
the callback stops the scan) and is called once at completion elsewhere.  The packed association scans build a `Panel` of the
payload and run `pipeline.scan_rows` on a caller-rotated `SpectralModel`: the one orchestration `jx gwas` runs as well.

A reference call site such as ``jxrs.grm_packed_f32(packed, n, flip, maf, idx, method=1)`` works unchanged
with ``import janusx_amd.janusx as jxrs``.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from ._lib import check, lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _is_device_tensor(a):
    """A torch CUDA tensor (a payload that is already resident in HBM)."""
    return hasattr(a, "is_cuda") and bool(getattr(a, "is_cuda"))


def _payload(packed, n_samples):
    """Packed 2-bit payload (m, ceil(n / 4)) uint8 as (object that owns the memory, pointer, m): a C-contiguous numpy
    array on the host, or a torch CUDA tensor used in place (extension of the reference's numpy-only interface: a panel
    that already lives in HBM is never staged through the host)."""
    if _is_device_tensor(packed):
        import torch
        if packed.dtype != torch.uint8 or packed.dim() != 2:
            raise RuntimeError("packed must be 2D uint8 (m, bytes_per_snp)")
        pk = packed.contiguous()
        ptr, shape = C.c_void_p(pk.data_ptr()), tuple(pk.shape)
    else:
        pk = _c(packed, np.uint8)
        if pk.ndim != 2:
            raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
        _guard_host_payload(pk.nbytes, "packed")
        ptr, shape = _p(pk), pk.shape
    if shape[1] != (int(n_samples) + 3) // 4:
        raise RuntimeError(f"packed second dimension mismatch: got {shape[1]}, expected {(int(n_samples) + 3) // 4}")
    return pk, ptr, int(shape[0])


def _guard_host_payload(nbytes, what):
    """A host array handed to the device layer is copied once more on its way (contiguous copy / staging): refuse clearly
    when that cannot fit instead of driving the machine out of memory (an n = 200 000 x m = 1 000 000 payload is 50 GB)."""
    try:
        import psutil
        avail = int(psutil.virtual_memory().available)
    except Exception:   # noqa: BLE001 - no psutil: no guard
        return
    if int(nbytes) > (1 << 30) and int(nbytes) > avail // 2:
        raise RuntimeError(f"{what}: a host array of {int(nbytes) / 2**30:.1f} GiB with {avail / 2**30:.1f} GiB of host memory "
                           "available cannot be staged safely; pass the payload as a device (torch CUDA uint8) tensor or "
                           "split the SNP rows over several calls")


def _opt_idx(a):
    if a is None:
        return None, 0
    a = _c(a, np.int64).ravel()
    return a, int(a.shape[0])


def _done(cb, total):
    if cb is not None:
        cb(int(total), int(total))


def _device_payload(pk):
    """A payload checked by `_payload` as a torch CUDA tensor: a device tensor as it is, a host array uploaded."""
    import torch
    if _is_device_tensor(pk):
        return pk
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # a read-only host array: only read on its way to the device
        return torch.from_numpy(pk).to(torch.device("cuda", torch.cuda.current_device()))


def _panel(packed, n_samples, sample_indices=None):
    """`pipeline.Panel` (P32 image in HBM) of a host (numpy) or device (torch CUDA) payload over the selected samples.  Refuses,
    before anything is allocated, when the device images do not fit the free HBM; the raw device copy of a host payload is
    dropped once it is re-tiled."""
    import torch
    from . import pipeline as pl
    pk, _ptr_unused, m = _payload(packed, n_samples)
    if m == 0:
        raise RuntimeError("packed matrix has zero SNP rows")
    idx = None if sample_indices is None else _c(sample_indices, np.int64).ravel()
    bps = (int(n_samples) + 3) // 4
    n_sel = int(n_samples) if idx is None else int(idx.shape[0])
    need = (0.0 if _is_device_tensor(pk) else float(m * bps)) + float(lib().jxg_num_tiles(n_sel)) * m * 32.0
    free = torch.cuda.mem_get_info()[0]
    if need > 0.95 * free:
        raise RuntimeError(f"packed payload of {(m * bps) >> 20} MiB: its device images need {int(need / 1048576.0)} MiB of HBM, "
                           f"{free >> 20} MiB are free (split the SNP rows over several calls)")
    return pl.Panel(_device_payload(pk), int(n_samples), idx)


# ------------------------------------------------------------------------------------------------
# GRM  (src/stats/grm.rs)
# ------------------------------------------------------------------------------------------------

def _grm_packed(packed, n_samples, row_flip, row_maf, sample_indices, method, out_dtype, with_stats):
    packed = _c(packed, np.uint8)
    if packed.ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    m = int(packed.shape[0])
    n_samples = int(n_samples)
    if n_samples <= 0:
        raise RuntimeError("n_samples must be > 0")
    if m == 0:
        raise RuntimeError("packed must contain at least one SNP row")
    bps = (n_samples + 3) // 4
    if packed.shape[1] != bps:
        raise RuntimeError(f"packed length mismatch: got {packed.size}, expected {m * bps}")
    flip = _c(np.asarray(row_flip).astype(np.uint8), np.uint8).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if maf.shape[0] != m or flip.shape[0] != m:
        raise RuntimeError(f"row_maf length mismatch: got {maf.shape[0]}, expected {m}")
    idx, n_sel = _opt_idx(sample_indices)
    n = n_sel if idx is not None else n_samples
    out = np.empty((n, n), dtype=out_dtype)
    row_sum = np.zeros(m, dtype=np.float64) if with_stats else None
    varsum = np.zeros(1, dtype=np.float64)
    check(lib().jx_grm_packed(_p(packed), m, n_samples, _p(flip), _p(maf), _p(idx), n_sel, int(method), _p(out),
                              1 if out_dtype == np.float64 else 0, _p(row_sum), _p(varsum)))
    return out, row_sum, float(varsum[0])


def grm_packed_f32(packed, n_samples, row_flip, row_maf, sample_indices=None, method=1, block_cols=65536,
                   threads=0, progress_callback=None, progress_every=0):
    """src/stats/grm.rs:3053-3066 -> f32 (n, n)."""
    k, _, _ = _grm_packed(packed, n_samples, row_flip, row_maf, sample_indices, method, np.float32, False)
    _done(progress_callback, np.asarray(packed).shape[0])
    return k


def grm_packed_f64(packed, n_samples, row_flip, row_maf, sample_indices=None, method=1, block_cols=65536,
                   threads=0, progress_callback=None, progress_every=0):
    """src/stats/grm.rs:3596 -> f64 (n, n) (same f32-block/f64-merge arithmetic as the f32 entry)."""
    k, _, _ = _grm_packed(packed, n_samples, row_flip, row_maf, sample_indices, method, np.float64, False)
    _done(progress_callback, np.asarray(packed).shape[0])
    return k


def grm_packed_f32_with_stats(packed, n_samples, row_flip, row_maf, sample_indices=None, method=1,
                              block_cols=65536, threads=0, progress_callback=None, progress_every=0):
    """src/stats/grm.rs:5583 -> (f32 (n,n), row_sum f64 (m), varsum)."""
    k, rs, vs = _grm_packed(packed, n_samples, row_flip, row_maf, sample_indices, method, np.float32, True)
    _done(progress_callback, np.asarray(packed).shape[0])
    return k, rs, vs


def grm_packed_f64_with_stats(packed, n_samples, row_flip, row_maf, sample_indices=None, method=1,
                              block_cols=65536, threads=0, progress_callback=None, progress_every=0):
    """src/stats/grm.rs:5611-5651 -> (f64 (n,n), row_sum f64 (m), varsum)."""
    k, rs, vs = _grm_packed(packed, n_samples, row_flip, row_maf, sample_indices, method, np.float64, True)
    _done(progress_callback, np.asarray(packed).shape[0])
    return k, rs, vs


def _normalize_spgrm_path(prefix):
    """src/stats/spgrm.rs:450-469."""
    t = str(prefix).strip()
    if not t:
        return ""
    if t.lower().endswith(".spgrm") or t.lower().endswith(".jxgrm"):
        return t
    if os.path.exists(t + ".jxgrm") and not os.path.exists(t + ".spgrm"):
        return t + ".jxgrm"
    return t + ".spgrm"


def _spgrm_packed(packed, n_samples, row_flip, row_maf, out_prefix, sample_indices, method, threshold, abs_threshold,
                  stream_denominator):
    n_samples = int(n_samples)
    pk, pk_ptr, pk_rows = _payload(packed, n_samples)
    flip = np.ascontiguousarray(np.asarray(row_flip).astype(np.uint8)).ravel()
    maf = _c(row_maf, np.float32).ravel()
    m = int(flip.shape[0])
    if m and maf.shape[0] != m:
        raise RuntimeError(f"Sparse GRM row_maf length mismatch: got {maf.shape[0]}, expected {m}")
    if m and pk_rows != m:
        raise RuntimeError(f"Sparse GRM packed length mismatch: got {pk_rows * ((n_samples + 3) // 4)}, expected "
                           f"{m * ((n_samples + 3) // 4)}")
    idx, n_sel = _opt_idx(sample_indices)
    if sample_indices is not None and n_sel == 0:
        raise RuntimeError("Sparse GRM sample_indices must not be empty")
    out_path = _normalize_spgrm_path(out_prefix)
    if not out_path:
        raise RuntimeError("Sparse GRM output prefix must not be empty")
    out_n, out_nnz = C.c_int64(0), C.c_int64(0)
    from .pipeline import dist_info
    rank, world = dist_info()
    if world > 1:
        # one process per GPU (SURVEY.md 8(e), configs[5]): the row panels of the lower triangle are dealt over the ranks, every
        # rank thresholds its own and leaves them in `<out>.part<rank>`; rank 0 joins the parts into the one `.spgrm` file (the
        # output directory is shared: one node).  No data-path collective: two barriers around the merge.
        import torch.distributed as dist
        check(lib().jx_spgrm_set_part(rank, world))
    try:
        check(lib().jx_spgrm_packed_to_jxgrm(pk_ptr, m, n_samples, _p(flip), _p(maf), _p(idx) if idx is not None else None,
                                             n_sel, int(method), float(threshold), int(bool(abs_threshold)),
                                             int(bool(stream_denominator)), out_path.encode(), C.byref(out_n),
                                             C.byref(out_nnz)))
    finally:
        if world > 1:
            lib().jx_spgrm_set_part(0, 1)
    if world > 1:
        dist.barrier()
        if rank == 0:
            check(lib().jx_spgrm_merge_parts(out_path.encode(), int(out_n.value), world, C.byref(out_nnz)))
        dist.barrier()
        nnz_t = _bcast_int(int(out_nnz.value))
        return out_path, int(out_n.value), nnz_t
    return out_path, int(out_n.value), int(out_nnz.value)


def _bcast_int(v):
    """Rank 0's integer on every rank."""
    import torch
    import torch.distributed as dist
    t = torch.tensor([int(v)], dtype=torch.int64)
    if dist.get_backend() == "nccl":
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    dist.broadcast(t, src=0)
    return int(t.cpu()[0])


def _scan_my_rows(scan, rows, lut):
    """SNP-sharded SparseLMM scan: `scan(rows, lut)` over this rank's contiguous share of the rows, the per-rank tables
    concatenated in rank (= row) order on every rank.  One rank: the plain call."""
    from . import pipeline as pl
    if pl.dist_info()[1] == 1:
        return scan(rows, lut)
    lo, hi = pl._my_slice(len(rows), False)
    return pl.gather_results(scan(rows[lo:hi], lut[lo:hi]).contiguous())


def spgrm_packed_to_jxgrm(packed, n_samples, row_flip, row_maf, out_prefix, sample_indices=None, method=1,
                          threshold=0.05, abs_threshold=False, block_rows=0, sample_block=0, threads=0,
                          progress_callback=None, progress_every=0):
    """src/stats/spgrm.rs:5201-5278: sparse (thresholded, lower-triangle CSC) GRM of a packed panel written as
    `<out_prefix>.spgrm` -> (path, n_samples_used, nnz).  The tile / spill planning arguments of the reference
    (block_rows, sample_block, threads) have no counterpart: the whole accumulator lives in HBM."""
    out = _spgrm_packed(packed, n_samples, row_flip, row_maf, out_prefix, sample_indices, method, threshold,
                        abs_threshold, False)
    if progress_callback is not None:
        progress_callback(1, 1)
    return out


def prepare_bed_logic_meta_selected(prefix, sample_indices=None, maf_threshold=0.0, max_missing_rate=1.0, het_threshold=1.0,
                                    snps_only=False, mmap_window_mb=None, threads=1):
    """src/io/gfreader.rs:7108-7235 -> `prepare_bed_logic_meta_owned_for_stats_samples_with_mmap_window` (:5236-5480): the QC
    pre-pass of the SparseLMM / sparse-GRM routes over the selected samples (python/janusx/assoc/workflow_model_packed.py:1106,
    1248) -> (row_source_indices i64 (kept), missing_rate f32 (kept), maf f32 (kept) = ALT allele frequency, row_flip bool
    (kept, all False), site_keep bool (all rows), n_samples_full, n_snps_total).  Per-SNP counts are popcounts on the device,
    the O(m) f32 decisions run on the host with the reference's expressions (`stats.packed_prep_row_stats`)."""
    from . import stats as st
    from .bed import snps_only_mask, stage_bed_payload
    if not (0.0 <= maf_threshold <= 0.5):
        raise ValueError("maf_threshold must be within [0, 0.5]")
    if not (0.0 <= max_missing_rate <= 1.0):
        raise ValueError("max_missing_rate must be within [0, 1.0]")
    if not (0.0 <= het_threshold <= 1.0):
        raise ValueError("het_threshold must be within [0, 1.0]")
    packed, n_fam, bim = stage_bed_payload(_bed_prefix(prefix), mmap_window_mb)
    if n_fam == 0:
        raise RuntimeError("no samples found in PLINK input")
    idx, n_sel = _opt_idx(sample_indices)
    if idx is not None and n_sel and (idx.min() < 0 or idx.max() >= n_fam):
        bad = int(idx[(idx < 0) | (idx >= n_fam)][0])
        raise ValueError(f"sample index out of range: {bad} for n_samples={n_fam}")
    n_stats = n_sel if (idx is not None and n_sel) else n_fam
    counts = bed_row_counts(packed, n_fam, idx if (idx is not None and n_sel) else None)
    keep, miss, maf, _std = st.packed_prep_row_stats(counts, n_stats, np.float32(maf_threshold), np.float32(max_missing_rate),
                                                     np.float32(het_threshold))
    if snps_only:
        keep = keep & snps_only_mask(bim)
    if not keep.any():
        raise RuntimeError("No SNPs left after packed BED filtering. Please relax thresholds.")
    rows = np.nonzero(keep)[0].astype(np.int64)
    return (rows, np.ascontiguousarray(miss[rows], dtype=np.float32), np.ascontiguousarray(maf[rows], dtype=np.float32),
            np.zeros(len(rows), dtype=bool), np.ascontiguousarray(keep, dtype=bool), int(n_fam), int(packed.shape[0]))


def load_bim_columns(path_or_prefix, row_indices=None):
    """src/io/gfreader.rs:8813-8862 -> (chrom, pos, snp, allele0, allele1) lists of a PLINK prefix (or explicit .bed/.bim/.fam
    path), optionally of the rows `row_indices` (the result-table metadata of python/janusx/assoc/workflow.py:4633)."""
    from .bed import read_bim
    p = str(path_or_prefix).strip()
    if not p:
        raise ValueError("path_or_prefix must not be empty")
    explicit = p.lower().endswith((".bed", ".bim", ".fam"))
    if not (explicit or all(os.path.exists(p + e) for e in (".bed", ".bim", ".fam"))):
        raise ValueError("load_bim_columns requires a PLINK BED/BIM/FAM prefix or explicit PLINK file path")
    bim = read_bim(_bed_prefix(p))
    if row_indices is None:
        sel = range(len(bim.chrom))
    else:
        sel = [int(v) for v in np.asarray(row_indices).ravel()]
        for v in sel:
            if v < 0:
                raise ValueError(f"row_indices must be non-negative, got {v}")
            if v >= len(bim.chrom):
                raise RuntimeError(f"BIM row index out of range: {v} >= {len(bim.chrom)}")
    return bim.columns(sel)


def spgrm_bed_to_jxgrm(prefix, out_prefix=None, sample_indices=None, method=1, threshold=0.05, abs_threshold=False,
                       maf_threshold=0.02, max_missing_rate=0.05, het_threshold=0.0, snps_only=False, block_rows=0,
                       sample_block=0, threads=0, mmap_window_mb=None, progress_callback=None, progress_every=0):
    """src/stats/spgrm.rs:5280-5356 -> `spgrm_bed_to_jxgrm_core` :4937-5025: metadata pre-pass over the selected
    samples (`prepare_bed_logic_meta_owned_for_stats_samples_with_mmap_window`, src/io/gfreader.rs:5236-5480: the
    packed-prep QC rule, maf := alt allele frequency, no flips), then the stream core (:3910-4264) whose centred
    denominator is the f64 sum of 2p(1-p) whatever the sample selection.  -> (path, n_samples_used, nnz)."""
    from . import stats as st
    from .bed import read_bed_payload, snps_only_mask
    if not (0.0 <= maf_threshold <= 0.5):
        raise RuntimeError("maf_threshold must be within [0, 0.5]")
    if not (0.0 <= max_missing_rate <= 1.0):
        raise RuntimeError("max_missing_rate must be within [0, 1.0]")
    if not (0.0 <= het_threshold <= 1.0):
        raise RuntimeError("het_threshold must be within [0, 1.0]")
    bed_prefix = str(prefix).strip()
    if bed_prefix.lower().endswith((".bed", ".bim", ".fam")):
        bed_prefix = bed_prefix[:-4]
    if not bed_prefix:
        raise RuntimeError("Sparse GRM BED prefix must not be empty")
    import torch
    from .bed import stage_bed_payload
    packed, n_fam, bim = stage_bed_payload(bed_prefix, mmap_window_mb)      # windowed staging to HBM, used in place
    if n_fam == 0:
        raise RuntimeError("No samples found in BED input.")
    idx, n_sel = _opt_idx(sample_indices)
    if idx is not None and n_sel and (idx.min() < 0 or idx.max() >= n_fam):
        raise RuntimeError("selected sample index out of range for BED logic preparation")
    n_stats = n_sel if (idx is not None and n_sel) else n_fam
    counts = bed_row_counts(packed, n_fam, idx if (idx is not None and n_sel) else None)
    keep, _miss, maf, _std = st.packed_prep_row_stats(counts, n_stats, np.float32(maf_threshold),
                                                      np.float32(max_missing_rate), np.float32(het_threshold))
    if snps_only:
        keep &= snps_only_mask(bim)
    if not keep.any():
        raise RuntimeError("No SNPs left after packed BED filtering. Please relax thresholds.")
    rows = np.nonzero(keep)[0]
    pk = packed if len(rows) == int(packed.shape[0]) else packed[torch.from_numpy(rows).to(packed.device)]
    del packed
    out = _spgrm_packed(pk, n_fam, np.zeros(len(rows), dtype=bool), maf[rows],
                        out_prefix if out_prefix is not None else bed_prefix,
                        idx if (idx is not None and n_sel) else None, method, threshold, abs_threshold, True)
    if progress_callback is not None:
        progress_callback(1, 1)
    return out


def _write_spgrm(path, n, col_ptr, rows, vals):
    """`.spgrm` layout of `write_sparse_grm_csc` (src/stats/spgrm.rs:3745-3767)."""
    nnz = int(len(vals))
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as fh:
        fh.write(np.array([n, nnz], dtype="<u8").tobytes())
        fh.write(np.ascontiguousarray(col_ptr, dtype="<u8").tobytes())
        fh.write(np.ascontiguousarray(rows, dtype="<u4").tobytes())
        fh.write(b"\0" * ((-(4 * nnz)) % 8))
        fh.write(np.ascontiguousarray(vals, dtype="<f8").tobytes())
    os.replace(tmp, path)


def _spgrm_dense_to_jxgrm(k, out_prefix, threshold, abs_threshold, progress_callback):
    import math
    import torch
    from . import pipeline as pl
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise RuntimeError(f"Sparse GRM dense writer expects a square matrix, got shape {tuple(k.shape)}")
    if k.dtype not in (np.float32, np.float64):
        raise RuntimeError(f"Sparse GRM dense writer expects float32 or float64, got {k.dtype}")
    n = int(k.shape[0])
    if n == 0:
        raise RuntimeError("Sparse GRM dense writer requires n_samples > 0")
    if not math.isfinite(threshold):
        raise RuntimeError("Sparse GRM threshold must be finite")
    out_path = _normalize_spgrm_path(out_prefix)
    if not out_path:
        raise RuntimeError("Sparse GRM output prefix must not be empty")
    dev = torch.device("cuda", torch.cuda.current_device())
    ld = int(lib().jxg_num_tiles(n)) * 128
    acc = torch.zeros((ld, ld), dtype=torch.float64, device=dev)
    acc[:n, :n] = torch.from_numpy(np.array(k, copy=True)).to(dev).to(torch.float64)
    work = torch.empty(int(lib().jxg_spgrm_work_bytes(n)), dtype=torch.uint8, device=dev)
    colptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = pl._stream()
    check(lib().jxg_spgrm_count(acc.data_ptr(), n, 1.0, float(threshold), int(bool(abs_threshold)), work.data_ptr(),
                                colptr.data_ptr(), st))
    cp = colptr.cpu().numpy().view(np.uint64)
    nnz = int(cp[n])
    rows = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    vals = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
    check(lib().jxg_spgrm_fill(acc.data_ptr(), n, 1.0, float(threshold), int(bool(abs_threshold)), work.data_ptr(),
                               colptr.data_ptr(), rows.data_ptr(), vals.data_ptr(), st))
    _write_spgrm(out_path, n, cp, rows.cpu().numpy()[:nnz].view(np.uint32), vals.cpu().numpy()[:nnz])
    if progress_callback is not None:
        progress_callback(n, n)
    return out_path, n, nnz


def spgrm_dense_npy_to_jxgrm(npy_path, out_prefix, threshold=0.05, abs_threshold=False, progress_callback=None,
                             progress_every=0):
    """src/stats/spgrm.rs:5972-6003 -> `spgrm_dense_npy_to_jxgrm_core` :5103-5199 / `spgrm_dense_f32_to_jxgrm_core`
    :5027-5101: an existing dense GRM (`.npy`, f32 or f64, square) thresholded into `<out_prefix>.spgrm` — lower triangle
    of the stored matrix, values widened to f64, same keep rule, (col, row) order.  The matrix goes to HBM once and the
    count / fill kernels of the sparse GRM build compact it (bit-exact: no arithmetic besides the widening).
    -> (path, n_samples, nnz)."""
    return _spgrm_dense_to_jxgrm(np.load(npy_path, mmap_mode="r"), out_prefix, threshold, abs_threshold, progress_callback)


def spgrm_dense_f32_to_jxgrm(grm, out_prefix, threshold=0.05, abs_threshold=False, progress_callback=None,
                             progress_every=0):
    """src/stats/spgrm.rs:5924-5970 (core :5027-5101): an in-memory dense f32 GRM thresholded into `<out_prefix>.spgrm`
    (the `SparseLMM` API of python/janusx/assoc/api.py:769-780) -> (path, n_samples, nnz)."""
    grm = np.asarray(grm)
    if grm.ndim != 2:
        raise RuntimeError("grm must be 2D (n, n).")
    if grm.shape[0] != grm.shape[1]:
        raise RuntimeError(f"grm must be square, got shape=({grm.shape[0]}, {grm.shape[1]})")
    return _spgrm_dense_to_jxgrm(_c(grm, np.float32), out_prefix, threshold, abs_threshold, progress_callback)


def spgrm_bed_to_jxgrm_from_meta(prefix, row_source_indices, row_flip, row_maf, n_total_sites, out_prefix=None,
                                 sample_indices=None, method=1, threshold=0.05, abs_threshold=False, block_rows=0,
                                 sample_block=0, threads=0, mmap_window_mb=None, progress_callback=None, progress_every=0):
    """src/stats/spgrm.rs:5377-5500: the stream core of `spgrm_bed_to_jxgrm` (:3910-4264) on rows, flips and allele
    frequencies the caller prepared (`jx grm -sparse` after its own QC pass, python/janusx/script/grm.py:1771)
    -> (path, n_samples_used, nnz)."""
    import torch
    from .bed import stage_bed_payload
    bed_prefix = _bed_prefix(prefix)
    if int(n_total_sites) <= 0:
        raise RuntimeError("n_total_sites must be positive for sparse GRM meta route.")
    src = _c(row_source_indices, np.int64).ravel()
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if src.size == 0:
        raise RuntimeError("row_source_indices must not be empty")
    if (src < 0).any():
        raise RuntimeError(f"row_source_indices must be non-negative, got {int(src[src < 0][0])}")
    if flip.shape[0] != src.shape[0] or maf.shape[0] != src.shape[0]:
        raise RuntimeError(f"row meta length mismatch: row_source_indices={src.shape[0]}, row_flip={flip.shape[0]}, "
                           f"row_maf={maf.shape[0]}")
    if int(src.max()) >= int(n_total_sites):
        raise RuntimeError(f"row_source index out of range: {int(src[src >= int(n_total_sites)][0])} >= "
                           f"n_total_sites={int(n_total_sites)}")
    packed, n_fam, _bim = stage_bed_payload(bed_prefix, mmap_window_mb)
    if n_fam == 0:
        raise RuntimeError("No samples found in BED input.")
    if int(src.max()) >= int(packed.shape[0]):
        raise RuntimeError(f"row_source index out of range for the BED payload: {int(src.max())} >= {int(packed.shape[0])}")
    idx, n_sel = _opt_idx(sample_indices)
    pk = packed[torch.from_numpy(src).to(packed.device)]
    del packed
    out = _spgrm_packed(pk, n_fam, flip, maf, out_prefix if out_prefix is not None else bed_prefix,
                        idx if (idx is not None and n_sel) else None, method, threshold, abs_threshold, True)
    if progress_callback is not None:
        progress_callback(1, 1)
    return out


def load_spgrm(path):
    """Reader of the `.spgrm` layout (`write_sparse_grm_csc`, src/stats/spgrm.rs:3745-3767)
    -> (n, col_ptr u64 (n+1), row_indices u32 (nnz), values f64 (nnz))."""
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size < 16:
        raise RuntimeError(f"sparse GRM file too small: {path}")
    n, nnz = (int(v) for v in raw[:16].view("<u8"))
    at = 16
    need = at + 8 * (n + 1) + 4 * nnz + ((-(4 * nnz)) % 8) + 8 * nnz
    if raw.size != need:
        raise RuntimeError(f"sparse GRM file length mismatch: got {raw.size}, expected {need}")
    col_ptr = raw[at:at + 8 * (n + 1)].view("<u8").copy()
    at += 8 * (n + 1)
    rows = raw[at:at + 4 * nnz].view("<u4").copy()
    at += 4 * nnz + ((-(4 * nnz)) % 8)
    vals = raw[at:at + 8 * nnz].view("<f8").copy()
    return n, col_ptr, rows, vals


# ------------------------------------------------------------------------------------------------
# Sparse REML null model over a `.spgrm` (src/stats/spreml.rs)
# ------------------------------------------------------------------------------------------------

def _brent_minimize_with_init(f, low, high, tol, max_iter, init_x):
    """Host Brent of src/math/brent.rs (`brent_minimize_with_init`; the device twin is `brent_reml` in csrc/k_scan.hip):
    golden-section / parabolic steps, `e` kept on parabolic steps, start at init_x when it lies inside [low, high]."""
    import math
    a, c = (low, high) if low < high else (high, low)
    eps = float(np.finfo(np.float64).eps)
    tol = max(abs(tol), 1e-12)
    x = init_x if (init_x is not None and math.isfinite(init_x) and a <= init_x <= c) else 0.5 * (a + c)
    w = v = x
    fx = f(x)
    fw = fv = fx
    d = e = 0.0
    for _ in range(int(max_iter)):
        m = 0.5 * (a + c)
        tol1 = tol * abs(x) + eps
        tol2 = 2.0 * tol1
        if abs(x - m) <= tol2 - 0.5 * (c - a):
            break
        parabolic = False
        if abs(e) > tol1:
            pp = (x - v) * ((x - w) * (fx - fv)) - (x - w) * ((x - v) * (fx - fw))
            qq = 2.0 * (((x - v) * (fx - fw)) - ((x - w) * (fx - fv)))
            if qq > 0.0:
                pp = -pp
            else:
                qq = -qq
            if abs(qq) > eps:
                st = pp / qq
                u = x + st
                if (u - a) >= tol2 and (c - u) >= tol2 and abs(st) < 0.5 * abs(e):
                    d = st
                    if (u - a) < tol2 or (c - u) < tol2:
                        d = tol1 if x < m else -tol1
                    parabolic = True
        if not parabolic:
            e = (c - x) if x < m else (a - x)
            d = 0.3819660 * e
        if abs(d) < tol1:
            d = tol1 if d >= 0.0 else -tol1
        u = x + d
        fu = f(u)
        if fu <= fx:
            if u >= x:
                a = x
            else:
                c = x
            v, fv = w, fw
            w, fw = x, fx
            x, fx = u, fu
        else:
            if u >= x:
                c = u
            else:
                a = u
            if fu <= fw or w == x:
                v, fv = w, fw
                w, fw = u, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    return x, fx


def _spgrm_dense_device(path, sample_indices):
    """Dense symmetric image (HBM, f64) of a `.spgrm`, optionally K[idx][:, idx] in the given order
    (`subset_sparse_grm_csc`, src/math/cholesky.rs:618-690, + `sparse_grm_to_dense`, src/stats/splmm.rs:2024-2039).
    -> (tensor (n, n), idx or None)."""
    import torch
    from . import pipeline as pl
    n_all, col_ptr, rows, vals = load_spgrm(path)
    idx, n_sel = _opt_idx(sample_indices)
    if idx is not None:
        if n_sel == 0:
            raise RuntimeError("Sparse GRM subset requires at least one sample")
        if idx.min() < 0 or idx.max() >= n_all:
            raise RuntimeError(f"Sparse GRM subset index out of range for n_samples={n_all}")
        uniq, cnt = np.unique(idx, return_counts=True)
        if (cnt > 1).any():
            first = next(int(v) for v in idx if cnt[np.searchsorted(uniq, v)] > 1)
            raise RuntimeError(f"Sparse GRM subset contains duplicated sample index: {first}")
    n = n_sel if idx is not None else n_all
    if n == 0:
        raise RuntimeError("SPREML requires n > 0")
    dev = torch.device("cuda", torch.cuda.current_device())
    d_cp = torch.from_numpy(col_ptr.view(np.int64)).to(dev)
    d_ri = torch.from_numpy(rows.view(np.int32)).to(dev)
    d_va = torch.from_numpy(vals).to(dev)
    d_map = None
    if idx is not None:
        mp = np.full(n_all, -1, dtype=np.int32)
        mp[idx] = np.arange(n, dtype=np.int32)
        d_map = torch.from_numpy(mp).to(dev)
    k = torch.empty((n, n), dtype=torch.float64, device=dev)
    check(lib().jxg_spgrm_densify(d_cp.data_ptr(), d_ri.data_ptr(), d_va.data_ptr(), int(n_all),
                                  d_map.data_ptr() if d_map is not None else None, n, k.data_ptr(), pl._stream()))
    return k, idx


def splmm_sparse_grm_diag_stats(jxgrm_path, sample_indices=None):
    """src/stats/splmm.rs:4055-4111 (`sparse_diag_stats` :1978-2022) -> (mean |diag| floored at 1e-30, min diag, max
    diag [starting from 0], n, nnz) of the (subset of the) sparse GRM; host-side metadata pass over the CSC arrays."""
    n_all, col_ptr, rows, vals = load_spgrm(jxgrm_path)
    idx, n_sel = _opt_idx(sample_indices)
    cp = col_ptr.astype(np.int64)
    cols = np.repeat(np.arange(n_all, dtype=np.int64), np.diff(cp))
    if n_all == 0:
        raise RuntimeError("SparseLMM diagonal stats require n_samples > 0")
    if idx is not None and not (n_sel == n_all and np.array_equal(idx, np.arange(n_all))):
        if n_sel == 0:
            raise RuntimeError("Sparse GRM subset requires at least one sample")
        if idx.min() < 0 or idx.max() >= n_all:
            raise RuntimeError(f"Sparse GRM subset index out of range for n_samples={n_all}")
        if len(np.unique(idx)) != n_sel:
            dup = next(int(v) for k, v in enumerate(idx) if v in idx[:k])
            raise RuntimeError(f"Sparse GRM subset contains duplicated sample index: {dup}")
        inside = np.zeros(n_all, dtype=bool)
        inside[idx] = True
        sel = inside[rows.astype(np.int64)] & inside[cols]
        rows, cols, vals = rows[sel], cols[sel], vals[sel]
        n_out = n_sel
        want = np.sort(idx)
    else:
        n_out = n_all
        want = np.arange(n_all, dtype=np.int64)
    on_diag = rows.astype(np.int64) == cols
    dcols, dvals = cols[on_diag], vals[on_diag]
    first = np.unique(dcols, return_index=True)[1]                  # the first diagonal entry of every column counts
    dcols, dvals = dcols[first], dvals[first]
    missing = np.setdiff1d(want, dcols)
    if missing.size:
        raise RuntimeError(f"SparseLMM diagonal is missing at column {int(missing[0])}")
    if not np.isfinite(dvals).all():
        bad = int(dcols[np.nonzero(~np.isfinite(dvals))[0][0]])
        raise RuntimeError(f"SparseLMM diagonal contains non-finite value at column {bad}")
    mean_abs = max(float(np.abs(dvals).sum()) / float(n_out), 1e-30)
    return mean_abs, float(dvals.min()), float(max(dvals.max(), 0.0)), int(n_out), int(len(vals))


def splmm_load_sparse_grm_subset_dense(jxgrm_path, sample_indices=None):
    """src/stats/splmm.rs:4022-4054 -> dense (n, n) f64 image of the (subset of the) sparse GRM."""
    k, _ = _spgrm_dense_device(jxgrm_path, sample_indices)
    return k.cpu().numpy()


def _sparse_block_size():
    """Samples per diagonal block of the block route (JXGPU_SPLMM_BLOCK, default 4096)."""
    v = os.environ.get("JXGPU_SPLMM_BLOCK", "")
    return max(int(v), 2) if v.strip() else 4096


def _sparse_block_route(n):
    """Block-diagonal spectral form (connected components of the sparse GRM) instead of one dense n x n eigenproblem:
    from n = 16384 (JXGPU_SPLMM_BLOCK_MIN_N), or always / never with JXGPU_SPLMM_ROUTE=block / dense."""
    mode = os.environ.get("JXGPU_SPLMM_ROUTE", "").strip().lower()
    if mode == "block":
        return True
    if mode == "dense":
        return False
    v = os.environ.get("JXGPU_SPLMM_BLOCK_MIN_N", "")
    return int(n) >= (int(v) if v.strip() else 16384)


def _pack_components_into_blocks(lab, bsz):
    """Sample order of the block-diagonal route: `lab[i]` = connected component of sample i.  Whole components are packed
    (largest first, first fit among the most recent blocks) into blocks of at most `bsz` samples; a component of `bsz` or
    more samples is a block of its own.  -> (perm, offs): perm[pos] = sample at position pos of the block order (components
    contiguous inside a block), block b = positions offs[b] .. offs[b + 1]."""
    lab = np.asarray(lab, dtype=np.int64)
    ncomp = int(lab.max()) + 1 if lab.size else 0
    sizes = np.bincount(lab, minlength=ncomp)
    order = np.argsort(-sizes, kind="stable")
    block_of = np.empty(ncomp, dtype=np.int64)
    fill = []
    for c in order:
        placed = False
        if sizes[c] < bsz:
            for b in range(len(fill) - 1, max(len(fill) - 64, -1), -1):
                if fill[b] + sizes[c] <= bsz:
                    fill[b] += int(sizes[c])
                    block_of[c] = b
                    placed = True
                    break
        if not placed:
            fill.append(int(sizes[c]))
            block_of[c] = len(fill) - 1
    sample_block = block_of[lab]
    perm = np.lexsort((lab, sample_block)).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(np.bincount(sample_block, minlength=len(fill)))]).astype(np.int64)
    return perm, offs


def _hbm_free_agreed():
    """Free HBM in bytes.  When the caller has declared the sparse routes collective (`dist.enable_collective_size_checks()`:
    every rank makes the same calls) the MINIMUM over the ranks, so that a size check decides the same way on every rank (a rank
    that raised alone would leave the others waiting in their next collective).  Otherwise the local figure: these routes may be
    called on one rank only, or be answered from the spectral cache on some ranks, and a hidden collective would hang the rest."""
    import torch
    from . import dist as _jd
    free, _total = torch.cuda.mem_get_info()
    try:
        import torch.distributed as tdist
        if (_jd.collective_size_checks() and tdist.is_available() and tdist.is_initialized()
                and tdist.get_world_size() > 1):
            t = torch.tensor([float(free)], dtype=torch.float64)
            if tdist.get_backend() == "nccl":
                t = t.to(torch.device("cuda", torch.cuda.current_device()))
            tdist.all_reduce(t, op=tdist.ReduceOp.MIN)
            free = int(t.item())
    except Exception:   # noqa: BLE001 - no usable process group: the local figure
        pass
    return int(free)


def sparse_component_limit(free_bytes=None):
    """Largest connected component (samples) of a thresholded GRM the spectral SparseLMM / sparse-REML routes take: one dense
    eigenproblem per component on ONE GPU -- the f64 image of the component, its eigenvectors and the eigensolver's workspace,
    about 5 n^2 doubles -- so n <= sqrt(free HBM / 40 B): ~ 79 000 samples on an empty MI355X (288 GB; BASELINE configs[3] runs
    n = 50 000 in 16 s).  The reference factorises K + lambda I sparsely for any structure (src/math/cholesky.rs:776-1075,
    src/stats/spreml.rs:384-760); beyond this limit the routes here refuse with the size and the limit in the message.
    JXGPU_SPLMM_COMPONENT_MAX overrides (tests)."""
    import math
    v = os.environ.get("JXGPU_SPLMM_COMPONENT_MAX", "").strip()
    if v:
        return max(int(v), 1)
    free = _hbm_free_agreed() if free_bytes is None else int(free_bytes)
    return int(math.isqrt(max(free, 0) // 40))


class _ComponentTooLarge(RuntimeError):
    """A dense eigenproblem the spectral routes would need does not fit this GPU: the caller switches to the sparse-factor
    route (`_SparseFactorReml`) or, where none exists, lets the message through."""


def _check_spectral_sparse_size(n, what="the selected samples"):
    """The single-eigenproblem form of the sparse REML / SparseLMM routes holds a dense f64 image of K, its eigenvectors
    and the eigensolver's workspace (~5 n^2 doubles) in HBM.  Refuse clearly -- on every rank alike -- instead of failing
    inside hipMalloc."""
    limit = sparse_component_limit()
    if int(n) > limit:
        raise _ComponentTooLarge(
            f"sparse-GRM spectral route: {what} form one dense eigenproblem of {int(n)} samples; the limit on this GPU is "
            f"{limit} samples (about 5 n^2 doubles of HBM: the f64 image of K, its eigenvectors and the eigensolver's workspace). "
            "Raise the GRM cut-off so that the relatedness graph falls apart into smaller components, or restrict the samples; "
            "the reference's sparse factorisation of K + lambda I for arbitrary structure (src/math/cholesky.rs) is not "
            "rebuilt here")


# One-entry cache of the spectral form of a sparse GRM (eigenvalues + eigenvectors of the dense image or of its diagonal
# blocks, in HBM): the reference's workflow calls the null fit and then the scan of a trait as separate functions, each of
# which factorises the same K; here the second call (and every further trait on the same samples) reuses the decomposition.
# Keyed by the file's identity (path, size, mtime), the sample list and the route; `spectral_cache_clear()` frees the HBM.
_SPECTRAL_CACHE = {}


def _spectral_cache_key(path, sample_indices, route):
    import hashlib
    if os.environ.get("JXGPU_SPECTRAL_CACHE", "1").strip() == "0":
        return None
    try:
        st = os.stat(path)
    except OSError:
        return None
    idx, _n = _opt_idx(sample_indices)
    h = "all" if idx is None else hashlib.sha1(np.ascontiguousarray(idx, dtype=np.int64).tobytes()).hexdigest()
    return (os.path.abspath(path), st.st_size, st.st_mtime_ns, h, route)


def _spectral_cache_put(key, value):
    if key is None:
        return
    _SPECTRAL_CACHE.clear()
    _SPECTRAL_CACHE[key] = value


def spectral_cache_clear():
    """Drop the cached spectral form of the last sparse GRM (frees its eigenvector blocks in HBM)."""
    _SPECTRAL_CACHE.clear()


def release_device_scratch():
    """Hand everything this library keeps in HBM between calls back to the driver: the cached spectral form of the last sparse
    GRM and the eigensolver's kept workspaces (`jxg_scratch_trim`; at most 6 GB each).  For a long-lived process between two
    problems of very different size; returns the bytes of workspace released.  (The reference's CPU path frees per call.)"""
    _SPECTRAL_CACHE.clear()
    return int(lib().jxg_scratch_trim())


class _SpectralSparseReml:
    """K + lambda I of a (subset of a) sparse GRM handled through ONE eigendecomposition on the GPU instead of one
    sparse LLT per lambda (src/stats/spreml.rs:384-512 factorises at every evaluation): K = U diag(s) U', so
    (K + lambda I)^-1 = U diag(1 / (s + lambda)) U', log det = sum log(s + lambda), and the matrix is factorisable
    exactly when min(s) + lambda > 0.  Densify (jxg_spgrm_densify), eigh (jxg_eigh_f64) and the rotation of [y | X]
    (rocBLAS dgemm through torch) run on the device; an evaluation is then O(n p^2) on (n, p + 2) numbers."""

    def __init__(self, path, y, x_cov, sample_indices):
        import torch
        from . import pipeline as pl
        y = _c(y, np.float64).ravel()
        self.perm, self.blocks = None, None
        if _sparse_block_route(y.shape[0]):
            self._init_blocks(path, y, x_cov, sample_indices)
            return
        key = _spectral_cache_key(path, sample_indices, "dense")
        hit = _SPECTRAL_CACHE.get(key)
        if hit is None:
            _check_spectral_sparse_size(y.shape[0])
            k, idx = _spgrm_dense_device(path, sample_indices)
            n = int(k.shape[0])
        else:
            n, idx = int(hit[0].shape[0]), hit[2]
        if n != y.shape[0]:
            raise RuntimeError(f"SPREML subset sample size mismatch: sparse n={n}, phenotype n={y.shape[0]}")
        if n == 0:
            raise RuntimeError("SPREML requires n > 0")
        if x_cov is None:
            x = np.ones((n, 1), dtype=np.float64)
        else:
            xc = _c(x_cov, np.float64)
            if xc.ndim != 2 or xc.shape[0] != n:
                raise RuntimeError(f"x_cov shape mismatch: got {list(xc.shape)}, expected ({n}, p)")
            x = np.concatenate([np.ones((n, 1)), xc], axis=1)
        self.n, self.p = n, int(x.shape[1])
        if hit is None:
            s, ut = pl.eigh_from_grm(k, ridge=0.0)               # row j of ut = eigenvector j
            del k
            _spectral_cache_put(key, (s, ut, idx))
        else:
            s, ut = hit[0], hit[1]
        dev = s.device
        rot = ut @ torch.from_numpy(np.concatenate([y[:, None], x], axis=1)).to(dev)
        rot = rot.cpu().numpy()
        self.s = s.cpu().numpy()
        self.yr, self.xr = rot[:, 0].copy(), rot[:, 1:].copy()
        self.smin = float(self.s.min())
        self.s_dev, self.ut_dev, self.x_design, self.y_raw, self.sample_idx = s, ut, x, y, idx

    def _init_blocks(self, path, y, x_cov, sample_indices):
        """Block-diagonal form: the graph of the (subset of the) sparse GRM is split into connected components, whole
        components are packed into diagonal blocks of at most `_sparse_block_size()` samples (a larger component is its own
        block), every block is densified and eigendecomposed on the device on its own.  The model then lives in the BLOCK
        ORDER of the samples (`self.perm`: position -> index into the caller's sample list); likelihood evaluations only
        see (s, U'y, U'X) and are unchanged."""
        import torch
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from . import pipeline as pl
        n_all, col_ptr, rows, vals = load_spgrm(path)
        idx, n_sel = _opt_idx(sample_indices)
        if idx is not None:
            if n_sel == 0:
                raise RuntimeError("Sparse GRM subset requires at least one sample")
            if idx.min() < 0 or idx.max() >= n_all:
                raise RuntimeError(f"Sparse GRM subset index out of range for n_samples={n_all}")
            if len(np.unique(idx)) != n_sel:
                raise RuntimeError("Sparse GRM subset contains duplicated sample index")
        n = n_sel if idx is not None else n_all
        if n != y.shape[0]:
            raise RuntimeError(f"SPREML subset sample size mismatch: sparse n={n}, phenotype n={y.shape[0]}")
        if x_cov is None:
            x = np.ones((n, 1), dtype=np.float64)
        else:
            xc = _c(x_cov, np.float64)
            if xc.ndim != 2 or xc.shape[0] != n:
                raise RuntimeError(f"x_cov shape mismatch: got {list(xc.shape)}, expected ({n}, p)")
            x = np.concatenate([np.ones((n, 1)), xc], axis=1)
        self.n, self.p = n, int(x.shape[1])
        key = _spectral_cache_key(path, sample_indices, f"block{_sparse_block_size()}")
        hit = _SPECTRAL_CACHE.get(key)
        if hit is not None:
            # the eigendecompositions of the diagonal blocks depend on the GRM and the sample list only: a null fit followed by
            # a scan of the same trait (or the next trait on the same samples) reuses them and only rotates its own [y | X]
            perm, blocks, s_all, glob = hit
            dev = blocks[0][2].device
            yx = np.concatenate([y[:, None], x], axis=1)[perm]
            rot_all = np.empty((n, 1 + self.p), dtype=np.float64)
            for o0, nb, utb in blocks:
                rot_all[o0:o0 + nb] = (utb @ torch.from_numpy(yx[o0:o0 + nb]).to(dev)).cpu().numpy()
            self.s = s_all
            self.yr, self.xr = rot_all[:, 0].copy(), rot_all[:, 1:].copy()
            self.smin = float(self.s.min())
            self.perm, self.blocks = perm, blocks
            self.s_dev, self.ut_dev = torch.from_numpy(s_all).to(dev), None
            self.x_design, self.y_raw = x[perm], y[perm]
            self.sample_idx = glob
            return
        # connected components of the selected sub-graph (host: one pass over the nnz entries)
        cp = col_ptr.astype(np.int64)
        cols = np.repeat(np.arange(n_all, dtype=np.int64), np.diff(cp))
        r64 = rows.astype(np.int64)
        local = np.arange(n_all, dtype=np.int64)
        if idx is not None:
            local = np.full(n_all, -1, dtype=np.int64)
            local[idx] = np.arange(n, dtype=np.int64)
        lr, lc = local[r64], local[cols]
        ok = (lr >= 0) & (lc >= 0) & (lr != lc) & (vals != 0.0)
        graph = coo_matrix((np.ones(int(ok.sum()), dtype=np.int8), (lr[ok], lc[ok])), shape=(n, n))
        ncomp, lab = connected_components(graph, directed=False)
        sizes = np.bincount(lab, minlength=ncomp)
        bsz = _sparse_block_size()
        # a component beyond the block size is a block of its own, up to what one GPU's eigensolver holds (the same decision on
        # every rank once the caller has declared the call collective: dist.enable_collective_size_checks)
        if int(sizes.max()) > bsz:
            _check_spectral_sparse_size(int(sizes.max()), what="the samples of the largest connected component of the sparse GRM")
        perm, offs = _pack_components_into_blocks(lab, bsz)
        fill = np.diff(offs)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_cp = torch.from_numpy(col_ptr.view(np.int64)).to(dev)
        d_ri = torch.from_numpy(rows.view(np.int32)).to(dev)
        d_va = torch.from_numpy(vals).to(dev)
        glob = perm if idx is None else idx[perm]                        # sparse-GRM index of every position of the block order
        yx = np.concatenate([y[:, None], x], axis=1)[perm]
        s_all = np.empty(n, dtype=np.float64)
        rot_all = np.empty((n, 1 + self.p), dtype=np.float64)
        blocks = []
        # several ranks: the blocks are dealt over the ranks (largest first, each to the rank with the least n^3 so far), a rank
        # decomposes its own with the eigensolver's distribution paused (jxg_eigh_set_local) and the owner's (s, U) go to
        # everybody afterwards: same bits on every rank, the decompositions of the null fit in 1 / world of the time
        rank, world = pl.dist_info()
        owner = np.zeros(len(fill), dtype=np.int64)
        if world > 1:
            load = np.zeros(world)
            for b in np.argsort(-fill, kind="stable"):
                owner[b] = int(np.argmin(load))
                load[owner[b]] += float(fill[b]) ** 3
            check(lib().jxg_eigh_set_local(1))
        try:
            for b in range(len(fill)):
                o0, o1 = int(offs[b]), int(offs[b + 1])
                nb = o1 - o0
                if owner[b] != rank:
                    blocks.append((o0, nb, torch.empty((nb, nb), dtype=torch.float64, device=dev)))
                    continue
                mp = np.full(n_all, -1, dtype=np.int32)
                mp[glob[o0:o1]] = np.arange(nb, dtype=np.int32)
                d_map = torch.from_numpy(mp).to(dev)
                kb = torch.empty((nb, nb), dtype=torch.float64, device=dev)
                check(lib().jxg_spgrm_densify(d_cp.data_ptr(), d_ri.data_ptr(), d_va.data_ptr(), int(n_all), d_map.data_ptr(), nb,
                                              kb.data_ptr(), pl._stream()))
                if nb == 1:                                  # a lone sample: its own eigenpair
                    sb, utb = kb.reshape(1).clone(), torch.ones((1, 1), dtype=torch.float64, device=dev)
                else:
                    sb, utb = pl.eigh_from_grm(kb, ridge=0.0)
                del kb
                s_all[o0:o1] = sb.cpu().numpy()
                blocks.append((o0, nb, utb))
        finally:
            if world > 1:
                lib().jxg_eigh_set_local(0)
        if world > 1:
            import torch.distributed as dist
            through_host = dist.get_backend() != "nccl"        # functional mode on shared GPUs (gloo): through host memory
            s_t = torch.from_numpy(s_all)
            for b, (o0, nb, utb) in enumerate(blocks):
                src = int(owner[b])
                if through_host:
                    h = utb.cpu()
                    dist.broadcast(h, src=src)
                    if src != rank:
                        utb.copy_(h)
                    dist.broadcast(s_t[o0:o0 + nb], src=src)
                else:
                    dist.broadcast(utb, src=src)
                    sd = s_t[o0:o0 + nb].to(dev)
                    dist.broadcast(sd, src=src)
                    s_t[o0:o0 + nb] = sd.cpu()
        for o0, nb, utb in blocks:
            rot_all[o0:o0 + nb] = (utb @ torch.from_numpy(yx[o0:o0 + nb]).to(dev)).cpu().numpy()
        self.s = s_all
        self.yr, self.xr = rot_all[:, 0].copy(), rot_all[:, 1:].copy()
        self.smin = float(self.s.min())
        self.perm, self.blocks = perm, blocks
        self.s_dev, self.ut_dev = torch.from_numpy(s_all).to(dev), None
        self.x_design, self.y_raw = x[perm], y[perm]
        self.sample_idx = glob
        _spectral_cache_put(key, (perm, blocks, s_all, glob))

    def factorizable(self, lam):
        import math
        return math.isfinite(lam) and lam > 0.0 and (self.smin + lam) > 0.0

    def evaluate(self, log10_lambda, vp_fixed=None):
        import math
        lam = 10.0 ** log10_lambda
        if not (math.isfinite(lam) and lam > 0.0):
            raise RuntimeError(f"SPREML lambda is invalid at log10(lambda)={log10_lambda}")
        n, p = self.n, self.p
        if p == 0 or n <= p:
            raise RuntimeError(f"SPREML requires n > p, got n={n}, p={p}")
        d = self.s + lam
        if not (d.min() > 0.0):
            raise RuntimeError(f"K + lambda I is not positive definite at lambda={lam} (min eigenvalue {d.min():.3e})")
        wy = self.yr / d
        y_vinv_y = float(self.yr @ wy)
        xt_vinv_y = self.xr.T @ wy
        xt_vinv_x = self.xr.T @ (self.xr / d[:, None])
        chol = _spd_cholesky_with_jitter(xt_vinv_x, "SPREML XtVinvX")
        beta = np.linalg.solve(chol.T, np.linalg.solve(chol, xt_vinv_y))
        ypy = y_vinv_y - float(xt_vinv_y @ beta)
        if not math.isfinite(ypy) or ypy <= 1e-30:
            raise RuntimeError(f"SPREML profiled residual quadratic form is invalid at lambda={lam}: yPy={ypy}")
        df = float(n - p)
        log_det_m = float(np.log(d).sum())
        log_det_x = 2.0 * float(np.log(np.diag(chol)).sum())
        if vp_fixed is None:
            sigma_g2 = ypy / df
            if not math.isfinite(sigma_g2) or sigma_g2 <= 0.0:
                raise RuntimeError(f"SPREML sigma_g2 is invalid at lambda={lam}: sigma_g2={sigma_g2}")
            sigma_e2 = lam * sigma_g2
            reml = df * (math.log(df) - 1.0 - math.log(2.0 * math.pi)) * 0.5 - 0.5 * (
                df * math.log(ypy) + log_det_m + log_det_x)
            nf = float(n)
            ml = nf * (math.log(nf) - 1.0 - math.log(2.0 * math.pi)) * 0.5 - 0.5 * (nf * math.log(ypy) + log_det_m)
        else:
            if not (math.isfinite(vp_fixed) and vp_fixed > 0.0):
                raise RuntimeError(f"SPREML fastGWA fixed-Vp objective requires finite vp_fixed > 0, got {vp_fixed}")
            sigma_g2 = vp_fixed / (1.0 + lam)
            sigma_e2 = lam * sigma_g2
            reml = -0.5 * (df * math.log(sigma_g2) + log_det_m + log_det_x + ypy / sigma_g2)
            ml = float("nan")
        if not math.isfinite(reml) or not (math.isfinite(ml) or math.isnan(ml)):
            raise RuntimeError(f"SPREML likelihood is invalid at lambda={lam}: ml={ml}, reml={reml}")
        return (log10_lambda, lam, sigma_g2, sigma_e2, ml, reml)


class _SparseFactorReml:
    """K + lambda I of a (subset of a) sparse GRM whose relatedness graph holds a connected component beyond one dense
    eigenproblem on this GPU (`sparse_component_limit()`): no spectral form exists, so the matrix is handled as the reference
    handles every sparse GRM -- a sparse factorisation of K + lambda I per lambda ON THE HOST (`SparseJxgrmCholesky`,
    src/math/cholesky.rs:733, 1018-1183; one per objective evaluation, src/stats/spreml.rs:384-512): scipy's SuperLU in symmetric
    mode with a minimum-degree ordering of A + A' gives log det(K + lambda I) exactly (sum of the logs of U's diagonal; positive
    definite <=> every pivot positive) and the few solves of the null model (V^-1 [y | X]).  The per-SNP solves of the exact scan
    run on the device (`jxg_sps_solve_multi`: one multi-vector CG per block of SNP rows over the CSR image of K,
    csrc/k_spsolve.hip); the GRAMMAR-gamma route needs V^-1 for the <= 2000 sampled markers only (host factor) and scans in
    sample space as always.  Same interface as `_SpectralSparseReml` for the likelihood searches (`evaluate`, `factorizable`)."""

    factor_route = True

    def __init__(self, path, y, x_cov, sample_indices):
        import scipy.sparse as sp
        y = _c(y, np.float64).ravel()
        n_all, col_ptr, rows, vals = load_spgrm(path)
        idx, n_sel = _opt_idx(sample_indices)
        low = sp.csc_matrix((vals, rows.astype(np.int64), col_ptr.astype(np.int64)), shape=(n_all, n_all))
        full = low + sp.tril(low, -1).T                       # the file holds the lower triangle, diagonal first in every column
        if idx is not None:
            if n_sel == 0:
                raise RuntimeError("Sparse GRM subset requires at least one sample")
            if idx.min() < 0 or idx.max() >= n_all:
                raise RuntimeError(f"Sparse GRM subset index out of range for n_samples={n_all}")
            if len(np.unique(idx)) != n_sel:
                raise RuntimeError("Sparse GRM subset contains duplicated sample index")
            full = full.tocsr()[idx][:, idx]
        self.k = full.tocsr()
        self.k.sort_indices()
        n = int(self.k.shape[0])
        if n != y.shape[0]:
            raise RuntimeError(f"SPREML subset sample size mismatch: sparse n={n}, phenotype n={y.shape[0]}")
        if n == 0:
            raise RuntimeError("SPREML requires n > 0")
        if x_cov is None:
            x = np.ones((n, 1), dtype=np.float64)
        else:
            xc = _c(x_cov, np.float64)
            if xc.ndim != 2 or xc.shape[0] != n:
                raise RuntimeError(f"x_cov shape mismatch: got {list(xc.shape)}, expected ({n}, p)")
            x = np.concatenate([np.ones((n, 1)), xc], axis=1)
        self.n, self.p = n, int(x.shape[1])
        self.x_design, self.y_raw, self.sample_idx = x, y, idx
        self.perm, self.blocks = None, None
        self.diag = np.asarray(self.k.diagonal(), dtype=np.float64)
        self._fac = (None, None)         # (lambda, SuperLU) of the last factorisation
        self._dev = None                 # CSR image in HBM (exact scan)

    def _factor(self, lam):
        """SuperLU of K + lambda I without row pivoting, or None when a pivot is not positive (not positive definite)."""
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu
        if self._fac[0] == lam:
            return self._fac[1]
        a = (self.k + lam * sp.identity(self.n, format="csr")).tocsc()
        try:
            lu = splu(a, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        except RuntimeError:             # exactly singular
            lu = None
        if lu is not None:
            d = lu.U.diagonal()
            if not (np.all(np.isfinite(d)) and np.all(d > 0.0) and np.array_equal(lu.perm_r, lu.perm_c)):
                lu = None                # an indefinite matrix shows as a non-positive pivot or as a row interchange
        self._fac = (lam, lu)
        return lu

    def factorizable(self, lam):
        import math
        return bool(math.isfinite(lam) and lam > 0.0 and self._factor(float(lam)) is not None)

    @property
    def smin(self):
        """Sign of the smallest eigenvalue of K (the spectral form's `smin` is only ever compared with 0 by the callers)."""
        return 1.0 if self._factor(0.0) is not None else -1.0

    def solve(self, lam, b):
        """(K + lambda I)^-1 b for a vector or an (n, k) block (host sparse factor)."""
        lu = self._factor(float(lam))
        if lu is None:
            raise RuntimeError(f"K + lambda I is not positive definite at lambda={lam}")
        return lu.solve(np.ascontiguousarray(b, dtype=np.float64))

    def evaluate(self, log10_lambda, vp_fixed=None):
        """`sparse_reml_evaluate` (src/stats/spreml.rs:384-512): the same formulas as the spectral form, V^-1 and log det V from
        the sparse factor."""
        import math
        lam = 10.0 ** log10_lambda
        if not (math.isfinite(lam) and lam > 0.0):
            raise RuntimeError(f"SPREML lambda is invalid at log10(lambda)={log10_lambda}")
        n, p = self.n, self.p
        if p == 0 or n <= p:
            raise RuntimeError(f"SPREML requires n > p, got n={n}, p={p}")
        lu = self._factor(lam)
        if lu is None:
            raise RuntimeError(f"K + lambda I is not positive definite at lambda={lam}")
        vi = lu.solve(np.concatenate([self.y_raw[:, None], self.x_design], axis=1))
        y_vinv_y = float(self.y_raw @ vi[:, 0])
        xt_vinv_y = self.x_design.T @ vi[:, 0]
        xt_vinv_x = self.x_design.T @ vi[:, 1:]
        xt_vinv_x = 0.5 * (xt_vinv_x + xt_vinv_x.T)
        chol = _spd_cholesky_with_jitter(xt_vinv_x, "SPREML XtVinvX")
        beta = np.linalg.solve(chol.T, np.linalg.solve(chol, xt_vinv_y))
        ypy = y_vinv_y - float(xt_vinv_y @ beta)
        if not math.isfinite(ypy) or ypy <= 1e-30:
            raise RuntimeError(f"SPREML profiled residual quadratic form is invalid at lambda={lam}: yPy={ypy}")
        df = float(n - p)
        log_det_m = float(np.log(lu.U.diagonal()).sum())          # L has a unit diagonal, no interchanges: det = prod U_ii
        log_det_x = 2.0 * float(np.log(np.diag(chol)).sum())
        if vp_fixed is None:
            sigma_g2 = ypy / df
            if not math.isfinite(sigma_g2) or sigma_g2 <= 0.0:
                raise RuntimeError(f"SPREML sigma_g2 is invalid at lambda={lam}: sigma_g2={sigma_g2}")
            sigma_e2 = lam * sigma_g2
            reml = df * (math.log(df) - 1.0 - math.log(2.0 * math.pi)) * 0.5 - 0.5 * (
                df * math.log(ypy) + log_det_m + log_det_x)
            nf = float(n)
            ml = nf * (math.log(nf) - 1.0 - math.log(2.0 * math.pi)) * 0.5 - 0.5 * (nf * math.log(ypy) + log_det_m)
        else:
            if not (math.isfinite(vp_fixed) and vp_fixed > 0.0):
                raise RuntimeError(f"SPREML fastGWA fixed-Vp objective requires finite vp_fixed > 0, got {vp_fixed}")
            sigma_g2 = vp_fixed / (1.0 + lam)
            sigma_e2 = lam * sigma_g2
            reml = -0.5 * (df * math.log(sigma_g2) + log_det_m + log_det_x + ypy / sigma_g2)
            ml = float("nan")
        if not math.isfinite(reml) or not (math.isfinite(ml) or math.isnan(ml)):
            raise RuntimeError(f"SPREML likelihood is invalid at lambda={lam}: ml={ml}, reml={reml}")
        return (log10_lambda, lam, sigma_g2, sigma_e2, ml, reml)

    def null_state(self, lam):
        """Null state of the exact scan (`build_sparse_splmm_null_state`, src/stats/splmm.rs:3500-3660) in SAMPLE space:
        V^-1 X, A = X'V^-1 X (jittered only if it fails), Py = V^-1 (y - X b), yPy -> (V^-1 X (n, p), Py (n), chol(A), yPy)."""
        vi = self.solve(lam, np.concatenate([self.y_raw[:, None], self.x_design], axis=1))
        vinv_x = vi[:, 1:]
        a = self.x_design.T @ vinv_x
        a_chol = _spd_cholesky_with_jitter(0.5 * (a + a.T), "SparseLMM XtWX")
        b0 = np.linalg.solve(a_chol.T, np.linalg.solve(a_chol, vinv_x.T @ self.y_raw))
        py = vi[:, 0] - vinv_x @ b0
        ypy = float(self.y_raw @ py)
        if not (np.isfinite(ypy) and ypy > 0.0):
            raise RuntimeError(f"SparseLMM exact scan requires finite positive yPy on K + lambda I scale, got {ypy}")
        return vinv_x, py, a_chol, ypy

    def device_csr(self):
        """(rowptr int64, col int32, val f64) of K in HBM, uploaded once."""
        import torch
        if self._dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            self._dev = (torch.from_numpy(self.k.indptr.astype(np.int64)).to(dev),
                         torch.from_numpy(self.k.indices.astype(np.int32)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(self.k.data, dtype=np.float64)).to(dev))
        return self._dev


def _sparse_reml_model(path, y, x_cov, sample_indices):
    """The model of K + lambda I for the sparse-GRM routes: the spectral form (one dense or block-diagonal eigendecomposition on
    the GPU) wherever every connected component fits one dense eigenproblem, the sparse-factor form beyond that
    (`sparse_component_limit()`; JXGPU_SPLMM_ROUTE=factor forces it)."""
    if os.environ.get("JXGPU_SPLMM_ROUTE", "").strip().lower() == "factor":
        return _SparseFactorReml(path, y, x_cov, sample_indices)
    try:
        return _SpectralSparseReml(path, y, x_cov, sample_indices)
    except _ComponentTooLarge:
        return _SparseFactorReml(path, y, x_cov, sample_indices)


def _spd_cholesky_with_jitter(mat, label):
    """src/stats/spreml.rs:324-351 (pivot floor 1e-18 of `cholesky_inplace`, src/math/linalg.rs:341-363)."""
    def try_chol(a):
        try:
            l = np.linalg.cholesky(a)
        except np.linalg.LinAlgError:
            return None
        return l if (np.diag(l) ** 2 > 1e-18).all() else None
    dim = mat.shape[0]
    l = try_chol(mat)
    if l is not None:
        return l
    base = max(float(np.abs(np.diag(mat)).sum()) / max(dim, 1), 1.0) * 1e-10
    for k in range(8):
        l = try_chol(mat + np.eye(dim) * (base * 10.0 ** k))
        if l is not None:
            return l
    raise RuntimeError(f"{label} is not SPD even after diagonal jitter")


def _spreml_grid(model, low, high, grid_size, vp_fixed):
    import math
    if not (math.isfinite(low) and math.isfinite(high)) or low >= high:
        raise RuntimeError(f"SPREML grid search requires finite low < high, got low={low}, high={high}")
    grid_n = max(int(grid_size), 2)
    evals, best, first_err = [], None, None
    for i in range(grid_n):
        x = low + (high - low) * (i / (grid_n - 1))
        try:
            ev = model.evaluate(x, vp_fixed)
        except RuntimeError as e:
            if first_err is None:
                first_err = str(e)
            continue
        if best is None or ev[5] > best[5]:
            best = ev
        evals.append(ev)
    if best is None:
        tail = f"; first failure: {first_err}" if first_err else ""
        raise RuntimeError(f"SPREML sparse grid search found no valid lambda in [{low}, {high}]{tail}")
    return best, evals


def _spreml_tuple(best, grid):
    return (best[1], best[2], best[3], best[4], best[5], best[0], [g[0] for g in grid], [g[5] for g in grid],
            [g[2] for g in grid], [g[3] for g in grid])


def _spreml_brent(model, low, high, grid_size, tol, max_iter, vp_fixed, progress_callback):
    """`sparse_reml_brent_search_with_progress` (src/stats/spreml.rs:591-757)."""
    import math
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError(f"SPREML Brent tol must be finite and > 0, got {tol}")
    if int(max_iter) == 0:
        raise RuntimeError("SPREML Brent max_iter must be > 0")
    grid_n = max(int(grid_size), 2)
    total = 1 + grid_n + max(int(max_iter), 1)
    best, grid = _spreml_grid(model, low, high, grid_size, vp_fixed)
    bi = next((i for i, g in enumerate(grid) if g[0] == best[0]), 0)
    b_low = grid[bi - 1][0] if bi > 0 else low
    b_high = grid[bi + 1][0] if bi + 1 < len(grid) else high
    if bi == 0 and grid and grid_n > 1:
        raw_step = (high - low) / (grid_n - 1)
        first_valid = grid[0][0]
        prev_raw = max(first_valid - raw_step, low)
        if prev_raw < first_valid:     # `refine_monotone_valid_lower_bound` (:152-186), 24 bisections
            valid = lambda v: model.factorizable(10.0 ** v)   # noqa: E731
            if valid(first_valid):
                if valid(prev_raw):
                    b_low = prev_raw
                else:
                    lo, hi, tol_use = prev_raw, first_valid, max(abs(min(tol, 1e-2)), 1e-6)
                    for _ in range(24):
                        if abs(hi - lo) <= tol_use:
                            break
                        mid = 0.5 * (lo + hi)
                        if valid(mid):
                            hi = mid
                        else:
                            lo = mid
                    b_low = hi
            else:
                b_low = first_valid
    if not (math.isfinite(b_low) and math.isfinite(b_high) and b_low < b_high):
        b_low, b_high = low, high

    def cost(v):
        try:
            return -model.evaluate(v, vp_fixed)[5]
        except RuntimeError:
            return 1e300

    x_best, _ = _brent_minimize_with_init(cost, b_low, b_high, tol, max_iter, best[0])
    out = model.evaluate(x_best, vp_fixed)
    if progress_callback is not None:
        progress_callback(total, total)
    return _spreml_tuple(out, grid)


def spreml_sparse_reml_grid_from_jxgrm(jxgrm_path, y, x_cov=None, sample_indices=None, low=-5.0, high=5.0,
                                       grid_size=33, threads=1):
    """src/stats/spreml.rs:826-918 -> (lambda, sigma_g2, sigma_e2, ml, reml, log10_lambda, grid_log10, grid_reml,
    grid_sigma_g2, grid_sigma_e2): REML profile of y ~ [1, x_cov] + g, Var g = sigma_g2 K (sparse), on a lambda grid."""
    model = _sparse_reml_model(jxgrm_path, y, x_cov, sample_indices)
    return _spreml_tuple(*_spreml_grid(model, low, high, grid_size, None))


def spreml_sparse_reml_brent_from_jxgrm(jxgrm_path, y, x_cov=None, sample_indices=None, low=-5.0, high=5.0,
                                        grid_size=9, tol=1e-3, max_iter=20, threads=1, progress_callback=None):
    """src/stats/spreml.rs:920-1042: grid, then Brent between the best point's neighbours (same 10-tuple)."""
    model = _sparse_reml_model(jxgrm_path, y, x_cov, sample_indices)
    return _spreml_brent(model, low, high, grid_size, tol, max_iter, None, progress_callback)


def spreml_sparse_fastgwa_fixed_vp_brent_from_jxgrm(jxgrm_path, y_resid, vp_fixed, sample_indices=None, low=-5.0,
                                                    high=5.0, grid_size=9, tol=1e-3, max_iter=20, threads=1,
                                                    progress_callback=None):
    """src/stats/spreml.rs:1044-1160: the fastGWA objective (Vp fixed, intercept-only design on residuals)."""
    model = _sparse_reml_model(jxgrm_path, y_resid, None, sample_indices)
    return _spreml_brent(model, low, high, grid_size, tol, max_iter, float(vp_fixed), progress_callback)


def _splmm_exact_null_state(model, lam):
    """Null state of the exact scan on the K + lambda I scale from the f64 spectrum (`build_sparse_splmm_null_state`,
    src/stats/splmm.rs:3500-3660): W = 1 / (s + lambda), A = X~'WX~ (jittered only if it fails, :1947-1976),
    Py~ = W (y~ - X~ b), yPy -> (w, Py~, WX~ as f32 device tensors, chol(A), yPy)."""
    import torch
    dev = model.s_dev.device
    d = model.s + lam
    wxh = model.xr / d[:, None]
    a_chol = _spd_cholesky_with_jitter(model.xr.T @ wxh, "SparseLMM XtWX")
    b0 = np.linalg.solve(a_chol.T, np.linalg.solve(a_chol, wxh.T @ model.yr))
    pyh = (model.yr - model.xr @ b0) / d
    ypy = float(model.yr @ pyh)
    if not (np.isfinite(ypy) and ypy > 0.0):
        raise RuntimeError(f"SparseLMM exact scan requires finite positive yPy on K + lambda I scale, got {ypy}")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    return f32(1.0 / d), f32(pyh), f32(wxh), a_chol, ypy


def splmm_assoc_pcg_dense_f32(g, y, lbd, sparse_jxgrm_path, x_cov=None, sparse_sample_indices=None, threads=0, block_rows=0):
    """src/stats/splmm.rs:5464-5650: SparseLMM exact scan of an already decoded SNP-major f32 matrix `g` (m, n) at a GIVEN
    lambda against the sparse GRM file (the `SparseLMM.gwas` API of python/janusx/assoc/api.py:898-940): null state of
    `build_sparse_splmm_null_state`, then `exact_scan_blocks_core` with the rows taken as they are (no flip, no imputation)
    -> f64 (m, 3) = beta, se, p.  V = K + lambda I through the eigenbasis of the sparse K (one dense or block-diagonal
    decomposition, cached per GRM): rows rotated on the device, g'V^-1 g / X'V^-1 g / g.Py as weighted sums."""
    import torch
    from . import pipeline as pl
    lbd = float(lbd)
    if not (np.isfinite(lbd) and lbd >= 0.0):
        raise RuntimeError("lbd must be finite and >= 0")
    g = np.asarray(g)
    if g.ndim != 2:
        raise RuntimeError("g must be 2D SNP-major (m, n)")
    m, n = int(g.shape[0]), int(g.shape[1])
    if m == 0 or n == 0:
        raise RuntimeError("g must have positive shape (m > 0, n > 0)")
    g = _c(g, np.float32)
    y = _c(y, np.float64).ravel()
    if y.shape[0] != n:
        raise RuntimeError(f"Dense SparseLMM requires len(y) to equal g.shape[1], got len(y)={y.shape[0]} and n={n}")
    p = 1
    if x_cov is not None:
        xc = _c(x_cov, np.float64)
        if xc.ndim != 2:
            raise RuntimeError("x_cov must be 2D (n, p_cov)")
        if xc.shape[0] != n:
            raise RuntimeError(f"x_cov row count mismatch: got {xc.shape[0]}, expected {n}")
        p += int(xc.shape[1])
    if n <= p:
        raise RuntimeError(f"Dense SparseLMM requires n > p, got n={n}, p={p}")
    if sparse_sample_indices is not None and len(np.asarray(sparse_sample_indices).ravel()) != n:
        raise RuntimeError("Dense SparseLMM scan requires factor subset n to match g/y n; "
                           f"factor_n={len(np.asarray(sparse_sample_indices).ravel())}, y_n={n}")
    model = _sparse_reml_model(sparse_jxgrm_path, y, x_cov, sparse_sample_indices)
    if not model.factorizable(lbd):
        raise RuntimeError(f"K + lambda I is not positive definite at lambda={lbd}")
    if getattr(model, "factor_route", False):
        # a connected component beyond one dense eigenproblem: multi-vector CG over the CSR image of K per block of rows
        dev = torch.device("cuda", torch.cuda.current_device())
        vinv_x, py, a_chol, ypy = model.null_state(lbd)
        rows_f32 = lambda r0, nr: torch.from_numpy(g[r0:r0 + nr]).to(dev)      # noqa: E731
        out = pl.scan_rows_splmm_factor(rows_f32, m, n, model.p, model.device_csr(), model.diag, lbd, vinv_x, py, a_chol, ypy, dev)
        return out.cpu().numpy()
    fv_state = _splmm_exact_null_state(model, lbd)
    dev = model.s_dev.device
    if model.blocks is not None:
        parts = [(off, nb, ut64.to(torch.float32), torch.from_numpy(np.ascontiguousarray(model.perm[off:off + nb])).to(dev))
                 for off, nb, ut64 in model.blocks]
    else:
        parts = [(0, n, model.ut_dev.to(torch.float32), None)]
    out = pl.scan_rows_splmm_dense(g, parts, n, model.p, fv_state, dev, int(block_rows) if int(block_rows) > 0 else 8192)
    return out.cpu().numpy()


def splmm_exact_scan_from_jxgrm(jxgrm_path, y, packed, packed_n_samples, maf, row_flip, x_cov=None,
                                sample_indices=None, row_indices=None, log10_lambda=None, low=-5.0, high=5.0,
                                grid_size=9, tol=1e-3, max_iter=20, grm_sample_indices=None):
    """SparseLMM exact association scan: the null model of `spreml_sparse_reml_brent_from_jxgrm` (or a given
    log10_lambda) followed by `exact_scan_blocks_core` (src/stats/splmm.rs:2567-2880) over the packed rows — the two
    stages the reference's `splmm_assoc_pcg_bed` workflow chains for its exact mode.  V = K + lambda I is never
    factorised: the eigenvectors of the sparse K rotate every SNP (the MFMA rotation kernel of the dense LMM, LUT
    [0, 2 maf, 1, 2] or flipped, missing = mean, not centred), and g'V^-1 g, X'V^-1 g, g.Py are weighted sums over the
    rotated row (`jxg_splmm_exact_scan_dev`).  -> (stats (m, 3) f64 [beta, se, p], log10_lambda, null 10-tuple or None).
    `grm_sample_indices` (extension): positions of the same samples inside the sparse GRM when its sample order is not
    the genotype file's (`sample_indices` then indexes the packed payload only); default: the same indices for both."""
    import torch
    from . import pipeline as pl
    model = _sparse_reml_model(jxgrm_path, y, x_cov, sample_indices if grm_sample_indices is None else grm_sample_indices)
    panel_idx = model.sample_idx if grm_sample_indices is None else (
        None if sample_indices is None else _c(sample_indices, np.int64).ravel())
    if grm_sample_indices is not None and panel_idx is not None and panel_idx.shape[0] != model.n:
        raise RuntimeError(f"sample_indices ({panel_idx.shape[0]}) and grm_sample_indices ({model.n}) differ in length")
    if model.blocks is not None and grm_sample_indices is not None:
        # block route: the model lives in its block order of the samples; the payload samples follow it
        panel_idx = model.perm if panel_idx is None else panel_idx[model.perm]
    null = None
    if log10_lambda is None:
        null = _spreml_brent(model, low, high, grid_size, tol, max_iter, None, None)
        log10_lambda = null[5]
    lam = 10.0 ** float(log10_lambda)
    if not model.factorizable(lam):
        raise RuntimeError(f"K + lambda I is not positive definite at lambda={lam}")
    n_full = int(packed_n_samples)
    pk, _pk_ptr, _pk_rows = _payload(packed, n_full)
    maf32 = _c(maf, np.float32).ravel()
    flip = np.asarray(row_flip).astype(bool).ravel()
    if maf32.shape[0] != pk.shape[0] or flip.shape[0] != pk.shape[0]:
        raise RuntimeError("maf / row_flip length must match packed rows")
    rows = np.arange(pk.shape[0], dtype=np.int64) if row_indices is None else _c(row_indices, np.int64).ravel()
    if rows.size and (rows.min() < 0 or rows.max() >= pk.shape[0]):
        raise RuntimeError("row_indices out of range")
    mean_g = np.clip(np.float32(2.0) * maf32[rows], np.float32(0.0), np.float32(2.0)).astype(np.float32)
    lut = np.empty((len(rows), 4), dtype=np.float32)
    lut[:, 0] = np.where(flip[rows], 2.0, 0.0)
    lut[:, 1] = mean_g
    lut[:, 2] = 1.0
    lut[:, 3] = np.where(flip[rows], 0.0, 2.0)
    if getattr(model, "factor_route", False):
        panel = _panel(pk, n_full, panel_idx)
        dev = panel.device
        rows_t = torch.from_numpy(rows.astype(np.int32)).to(dev)
        lut_t = torch.from_numpy(lut).to(dev)
        vinv_x, py, a_chol, ypy = model.null_state(lam)

        def rows_f32(r0, nr):
            buf = torch.empty((nr, model.n), dtype=torch.float32, device=dev)
            check(lib().jxg_decode_rows_p32(panel.p32.data_ptr(), panel.m, model.n, rows_t[r0:].data_ptr(), nr,
                                            lut_t[r0:].data_ptr(), buf.data_ptr(), model.n, pl._stream()))
            return buf
        out = pl.scan_rows_splmm_factor(rows_f32, len(rows), model.n, model.p, model.device_csr(), model.diag, lam, vinv_x, py,
                                        a_chol, ypy, dev)
        return out.cpu().numpy(), float(log10_lambda), null
    fv_state = _splmm_exact_null_state(model, lam)
    if model.blocks is not None:
        if panel_idx is None:
            panel_idx = np.arange(n_full, dtype=np.int64)
        rot = pl.BlockRotation(_device_payload(pk), n_full, panel_idx, model.blocks)
        out = _scan_my_rows(lambda r, l: pl.scan_rows_splmm_blocks(rot, model.p, r, l, fv_state), rows.astype(np.int32), lut)
    else:
        panel = _panel(pk, n_full, panel_idx)
        sm = pl.SpectralModel(model.s_dev, model.ut_dev, model.x_design, model.y_raw, fit_null=False)
        out = _scan_my_rows(lambda r, l: pl.scan_rows(panel, sm, r, l, mode="splmm", fv_state=fv_state),
                            rows.astype(np.int32), lut)
    return out.cpu().numpy(), float(log10_lambda), null


# ------------------------------------------------------------------------------------------------
# `jx gwas -splmm` / `-splmm-exact`: splmm_assoc_pcg_bed[_to_tsv] (src/stats/splmm.rs:4641-5026)
# ------------------------------------------------------------------------------------------------

SPLMM_DEFAULT_RHAT_MARKERS = 30          # src/stats/splmm.rs:65-66
SPLMM_DEFAULT_RHAT_SEED = 20260527


class _StdRngU32:
    """`StdRng::seed_from_u64` of rand 0.9.2 (Cargo.toml:42; the crate is not part of /root/reference): ChaCha12 keyed from a
    PCG32 expansion of the seed, words in block order; `random_range(0..m)` with Canon's single-sample method (u32 draws
    when the range fits 32 bits).  Restated from the published algorithm; the ChaCha core is pinned to RFC 7539, the seeding
    and range-sampling conventions are not pinned by any vector of the reference."""

    def __init__(self, seed):
        state = int(seed) & 0xffffffffffffffff
        key = []
        for _ in range(8):
            state = (state * 6364136223846793005 + 11634580027462260723) & 0xffffffffffffffff
            xs = (((state >> 18) ^ state) >> 27) & 0xffffffff
            rot = state >> 59
            key.append(((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xffffffff)
        self.key, self.counter, self.buf = key, 0, []

    def _block(self):
        def rotl(v, c):
            return ((v << c) & 0xffffffff) | (v >> (32 - c))
        st = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + self.key + [self.counter & 0xffffffff,
                                                                            (self.counter >> 32) & 0xffffffff, 0, 0]
        x = list(st)

        def qr(a, b, c, d):
            x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 16)
            x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 12)
            x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 8)
            x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 7)
        for _ in range(6):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        self.counter += 1
        return [(x[i] + st[i]) & 0xffffffff for i in range(16)]

    def next_u32(self):
        if not self.buf:
            self.buf = self._block()
        return self.buf.pop(0)

    def random_range(self, m):
        if m - 1 > 0xffffffff:
            bits, draw = 64, lambda: self.next_u32() | (self.next_u32() << 32)
        else:
            bits, draw = 32, self.next_u32
        mask = (1 << bits) - 1
        prod = draw() * m
        result, lo = prod >> bits, prod & mask
        if lo > ((-m) & mask):
            if lo + ((draw() * m) >> bits) > mask:
                result += 1
        return result


def splmm_choose_rhat_rows(m, count, seed):
    """`choose_rhat_rows` (src/stats/splmm.rs:1493-1507)."""
    soft_cap = min(int(count), int(m))
    if soft_cap == m:
        return np.arange(m, dtype=np.int64)
    rng = _StdRngU32(seed)
    return np.unique(np.array([rng.random_range(int(m)) for _ in range(max(2 * soft_cap, soft_cap))], dtype=np.int64))


def _splmm_prepare_inputs(prefix, y, x_cov, sample_indices, operator_sample_indices, site_keep, packed, packed_n_samples,
                          maf, row_flip, row_missing, row_indices, model, mmap_window_mb):
    """`prepare_splmm_assoc_inputs` (src/stats/splmm.rs:1302-1490): the three input forms -- external packed payload,
    BED prefix with the caller's row metadata, BED prefix alone (row statistics on the scan samples, no filter)."""
    from . import bed as _bed
    from . import stats as st
    gm_code = st.genetic_model_code(model)     # add / dom / rec / het, case-insensitive (`PackedGeneticModel::parse`, decode.rs:107-119)
    bed_prefix = _bed_prefix(prefix)
    if not bed_prefix:
        raise RuntimeError("BED-prefix mode requires a non-empty prefix")
    yv = _c(y, np.float64).ravel()
    n = int(yv.shape[0])
    if n == 0:
        raise RuntimeError("y must not be empty")
    xc = None
    if x_cov is not None:
        xc = _c(x_cov, np.float64)
        if xc.ndim != 2:
            raise RuntimeError("x_cov must be 2D (n, p_cov)")
        if xc.shape[0] != n:
            raise RuntimeError(f"x_cov row count mismatch: got {xc.shape[0]}, expected {n}")
    p = 1 + (0 if xc is None else int(xc.shape[1]))
    if n <= p:
        raise RuntimeError(f"n must be > p for SparseLMM: n={n}, p={p}")
    use_packed = packed is not None or int(packed_n_samples) > 0
    use_meta = (not use_packed) and any(a is not None for a in (maf, row_flip, row_missing, row_indices))
    if use_packed:
        for name, arr in (("packed", packed), ("maf", maf), ("row_flip", row_flip)):
            if arr is None:
                raise RuntimeError(f"splmm_assoc_pcg_bed: packed payload path requires `{name}` argument.")
        if int(packed_n_samples) <= 0:
            raise RuntimeError("splmm_assoc_pcg_bed: packed payload path requires packed_n_samples > 0")
        n_full = int(packed_n_samples)
        pk, _ptr_, m_packed = _payload(packed, n_full)
    else:
        if use_meta:
            for name, arr in (("maf", maf), ("row_flip", row_flip), ("row_indices", row_indices)):
                if arr is None:
                    raise RuntimeError(f"splmm_assoc_pcg_bed: mmap metadata path requires `{name}` argument.")
        pk, n_full, _bim = _bed.stage_bed_payload(bed_prefix, mmap_window_mb)
        m_packed = int(pk.shape[0])
    if n_full == 0:
        raise RuntimeError("No samples found in BED input.")

    def idx(a, label):
        if a is None:
            return None
        v = _c(a, np.int64).ravel()
        if v.size and (v.min() < 0 or v.max() >= n_full):
            raise RuntimeError(f"{label} out of range for n_samples={n_full}")
        return v
    scan_idx = idx(sample_indices, "sample_indices")
    op_idx = idx(operator_sample_indices, "operator_sample_indices")
    if op_idx is None:
        op_idx = scan_idx
    for v, label in ((scan_idx, "sample_indices"), (op_idx, "operator_sample_indices")):
        if v is not None and v.shape[0] != n:
            raise RuntimeError(f"{label} length mismatch: got {v.shape[0]}, expected {n}")
    if scan_idx is None and n != n_full:
        raise RuntimeError(f"len(y)={n} must equal scan n_samples={n_full} when sample_indices is not provided")
    if use_packed or use_meta:
        rows = None if row_indices is None else _c(row_indices, np.int64).ravel()
        if rows is not None and rows.size and (rows.min() < 0 or rows.max() >= m_packed):
            raise RuntimeError("row_indices out of range")
        m = m_packed if rows is None else int(rows.shape[0])
        maf32 = _c(maf, np.float32).ravel()
        flip = np.asarray(row_flip).astype(bool).ravel()
        miss = np.full(m, np.nan, dtype=np.float32) if row_missing is None else _c(row_missing, np.float32).ravel()
        if maf32.shape[0] != m or flip.shape[0] != m or miss.shape[0] != m:
            raise RuntimeError(f"{'packed' if use_packed else 'mmap'} metadata length mismatch: rows={m}, "
                               f"row_maf={maf32.shape[0]}, row_flip={flip.shape[0]}, row_missing={miss.shape[0]}")
        if rows is None:
            rows = np.arange(m, dtype=np.int64)
    else:
        # `prepare_prefix_input` (:1248-1290): packed-prep row statistics on the scan samples, thresholds (0, 1, 0); the
        # logic meta keeps maf = ALT frequency and never flips (src/io/gfreader.rs:5139, 5378-5460)
        counts = bed_row_counts(pk, n_full, scan_idx)
        keep, miss_all, maf_all, _std = st.packed_prep_row_stats(counts, n if scan_idx is not None else n_full, 0.0, 1.0, 0.0)
        flip_all = np.zeros(m_packed, dtype=bool)
        if site_keep is not None:
            sk = np.asarray(site_keep).astype(bool).ravel()
            if sk.shape[0] != m_packed:
                raise RuntimeError(f"site_keep length mismatch: got {sk.shape[0]}, expected {m_packed}")
            keep = keep & sk
        rows = np.nonzero(keep)[0].astype(np.int64)
        maf32, flip, miss = maf_all[rows].astype(np.float32), flip_all[rows], miss_all[rows].astype(np.float32)
    return dict(pk=pk, n_full=n_full, rows=rows, maf=maf32, flip=flip, miss=miss, y=yv, x_cov=xc, scan_idx=scan_idx,
                op_idx=op_idx, bed_prefix=None if use_packed else bed_prefix, n=n, p=p, gm_code=gm_code)


def _splmm_approx_scan(model, lam, pk, n_full, maf32, flip, rows, scan_idx, rhat_markers, rhat_seed, rhat_rows=None,
                       on_block=None, gm_code=0):
    """`estimate_residualized_approx_scan_sparse` (src/stats/splmm_approx.rs:701-795) on the spectral form of K + lambda I
    (`_SpectralSparseReml`): residualised response, a = V^-1 y_r / sigma2 through the eigenbasis, gamma from the sampled
    markers (their rotation by the MFMA kernel + `jxg_splmm_gamma_sums`), scan model a_r = M_X a, GRAMMAR scan in sample
    space (`jxg_splmm_grammar_scan_p32`).  -> (gamma, stats (m, 3) on the device, markers requested, markers used)."""
    import math
    import torch
    from . import pipeline as pl
    n, p = model.n, model.p
    x, yv = model.x_design, model.y_raw                   # the model's sample order (block order on the block route)
    xtx = x.T @ x
    cx = _spd_cholesky_with_jitter(xtx, "SparseLMM approx XtX")
    solve = lambda b: np.linalg.solve(cx.T, np.linalg.solve(cx, b))        # noqa: E731
    c_y = solve(x.T @ yv)
    y_resid = yv - x @ c_y
    rss = float(y_resid @ y_resid)
    if not (math.isfinite(rss) and rss > 1e-30):
        raise RuntimeError(f"SparseLMM residualized approx produced invalid residualized RSS: {rss}")
    sigma2 = rss / (float(n - p) * (1.0 + lam))
    if not (math.isfinite(sigma2) and sigma2 > 0.0):
        raise RuntimeError(f"SparseLMM residualized approx produced invalid scan sigma2 at lambda={lam}: {sigma2}")
    factor = getattr(model, "factor_route", False)
    if factor:
        # no spectral form (a connected component beyond one dense eigenproblem): V^-1 from the host sparse factor, as the
        # reference does (`SparseJxgrmCholesky`): one solve for a, one multi-vector solve for the sampled markers
        dev = torch.device("cuda", torch.cuda.current_device())
        a_vec = model.solve(lam, y_resid) / sigma2
    else:
        w = 1.0 / (model.s + lam)
        a_rot = w * (model.yr - model.xr @ c_y) / sigma2      # U'a,  a = (K + lambda I)^-1 y_r / sigma2
        dev = model.s_dev.device
        a_rot_t = torch.from_numpy(a_rot).to(dev)
        if model.blocks is not None:
            a_t = torch.empty(n, dtype=torch.float64, device=dev)
            for off, nb, utb in model.blocks:
                a_t[off:off + nb] = utb.T @ a_rot_t[off:off + nb]
        else:
            a_t = model.ut_dev.T @ a_rot_t
        a_vec = a_t.cpu().numpy()
    # ---- gamma from sampled markers
    m = len(rows)
    rr = splmm_choose_rhat_rows(m, rhat_markers, rhat_seed) if rhat_rows is None else _c(rhat_rows, np.int64).ravel()
    if rr.size and (rr.min() < 0 or rr.max() >= m):
        raise RuntimeError("rhat rows out of range")
    mean_g = np.clip(np.float32(2.0) * maf32, np.float32(0.0), np.float32(2.0)).astype(np.float32)
    lut = np.empty((m, 4), dtype=np.float32)
    lut[:, 0] = np.where(flip, 2.0, 0.0)
    lut[:, 1] = mean_g
    lut[:, 2] = 1.0
    lut[:, 3] = np.where(flip, 0.0, 2.0)
    if int(gm_code) != 0:
        # dom / rec / het (`decode_packed_row_model_into_f64`, src/decode/decode.rs:305-364, as the GRAMMAR scan's non-additive
        # branch and the sampled-marker decode call it: src/stats/splmm.rs:3211-3262, 1514-1560): the genetic model applied to
        # the raw values [0 | 2, max(2 maf, 0), 1, 2 | 0] INCLUDING the imputed entry, no centring (the scan residualises on X)
        from .stats import _apply_genetic_model
        lut[:, 1] = np.maximum(np.float32(2.0) * maf32, np.float32(0.0))
        for c in range(4):
            lut[:, c] = _apply_genetic_model(int(gm_code), lut[:, c])
    if _is_device_tensor(pk):
        packed_t = pk.to(dev)
    else:
        packed_t = torch.from_numpy(pk if pk.flags.writeable else pk.copy()).to(dev)
    panel_idx = scan_idx
    if model.perm is not None:
        panel_idx = model.perm if scan_idx is None else scan_idx[model.perm]
    sub = packed_t[torch.from_numpy(rows[rr]).to(dev)]    # payload of the sampled markers only
    sub_rows = np.arange(len(rr), dtype=np.int32)
    if factor:
        # the sampled markers decoded on the device, their sums in sample space on the host: gg, g'V^-1 g (one multi-vector
        # solve per 256 markers), g'a, X'g, X'V^-1 g = (V^-1 X)'g
        sp_panel = pl.Panel(sub, n_full, panel_idx)
        gdec = torch.empty((len(rr), n), dtype=torch.float32, device=dev)
        lut_s = torch.from_numpy(np.ascontiguousarray(lut[rr])).to(dev)
        check(lib().jxg_decode_rows_p32(sp_panel.p32.data_ptr(), sp_panel.m, n, None, len(rr), lut_s.data_ptr(), gdec.data_ptr(), n,
                                        pl._stream()))
        gh = gdec.cpu().numpy().astype(np.float64)
        del gdec, sp_panel
        vinv_x = model.solve(lam, x)
        sums = np.empty((len(rr), 3 + 2 * p), dtype=np.float64)
        for k0 in range(0, len(rr), 256):
            gb = gh[k0:k0 + 256]
            zb = model.solve(lam, gb.T)                     # (n, <= 256)
            sums[k0:k0 + 256, 0] = np.einsum("kn,kn->k", gb, gb)
            sums[k0:k0 + 256, 1] = np.einsum("kn,nk->k", gb, zb)
            sums[k0:k0 + 256, 2] = gb @ a_vec
            sums[k0:k0 + 256, 3:3 + p] = gb @ x
            sums[k0:k0 + 256, 3 + p:] = gb @ vinv_x
        del gh, sub
        xtwx = x.T @ vinv_x
        xta = x.T @ a_vec
    else:
        if model.blocks is not None:
            full_idx = np.arange(n_full, dtype=np.int64) if panel_idx is None else panel_idx
            rot = pl.BlockRotation(sub, n_full, full_idx, model.blocks)
            grot = pl.rotate_rows_blocks(rot, sub_rows, lut[rr])
            del rot
        else:
            sm = pl.SpectralModel(model.s_dev, model.ut_dev, model.x_design, model.y_raw, fit_null=False)
            grot = pl.rotate_rows(pl.Panel(sub, n_full, panel_idx), sm, sub_rows, lut[rr])
        sums = torch.empty((len(rr), 3 + 2 * p), dtype=torch.float64, device=dev)
        xr_t = torch.from_numpy(np.ascontiguousarray(model.xr)).to(dev)
        w_t = torch.from_numpy(w).to(dev)
        check(lib().jxg_splmm_gamma_sums(grot.data_ptr(), len(rr), n, n, p, w_t.data_ptr(), a_rot_t.data_ptr(), xr_t.data_ptr(),
                                         sums.data_ptr(), pl._stream()))
        sums = sums.cpu().numpy()
        del grot, sub
        xtwx = model.xr.T @ (model.xr * w[:, None])
        xta = model.xr.T @ a_rot
    fast_sum = res_sum = 0.0
    n_used = res_used = 0
    for k in range(len(rr)):
        gg, wgg, ag = sums[k, 0], sums[k, 1], sums[k, 2]
        xg, wxg = sums[k, 3:3 + p], sums[k, 3 + p:]
        c = solve(xg)
        s_ms = gg - float(xg @ c)
        if not (math.isfinite(s_ms) and math.isfinite(gg)) or s_ms <= max(1e-10, 1e-12 * max(abs(gg), 1.0)):
            continue
        svs = wgg - 2.0 * float(c @ wxg) + float(c @ xtwx @ c)
        if not (math.isfinite(svs) and svs > 1e-30):
            continue
        ratio = svs / s_ms
        if not (math.isfinite(ratio) and ratio > 0.0):
            continue
        res_sum += ratio
        res_used += 1
        score = ag - float(c @ xta)
        chisq = score * score / svs
        if math.isfinite(chisq) and chisq < 5.0:
            fast_sum += ratio
            n_used += 1
        if k + 1 >= rhat_markers and n_used >= 100:
            break
    if n_used == 0 and res_used == 0:
        raise RuntimeError("SparseLMM residualized approx gamma estimation found no valid sampled markers")
    gamma, used = (fast_sum / n_used, n_used) if n_used >= 100 else (res_sum / res_used, res_used)
    gamma *= 1.0 / sigma2
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise RuntimeError(f"SparseLMM residualized approx gamma must be finite and > 0, got {gamma}")
    # ---- scan model + scan, in the caller's sample order
    a_resid = a_vec - x @ solve(x.T @ a_vec)
    if model.perm is not None:
        inv = np.empty(n, dtype=np.int64)
        inv[model.perm] = np.arange(n)
        a_resid, x_scan = a_resid[inv], x[inv]
    else:
        x_scan = x
    panel = pl.Panel(packed_t, n_full, scan_idx)
    if pl.dist_info()[1] > 1:
        on_block = None        # block offsets are those of a rank's share: the gathered table is handed on by the caller
    out = _scan_my_rows(lambda r, l: pl.scan_rows_grammar(panel, r, l, x_scan, a_resid, gamma, on_block=on_block),
                        rows.astype(np.int32), lut)
    return float(gamma), out, int(len(rr)), int(used)


def _splmm_assoc(prefix, y, lbd, x_cov, sample_indices, operator_sample_indices, site_keep, tol, max_iter, block_rows,
                 std_eps, threads, model, rhat_markers, rhat_seed, packed, packed_n_samples, maf, row_flip, row_missing,
                 row_indices, sparse_sample_indices, sparse_jxgrm_path, progress_callback, progress_every, scan_mode,
                 mmap_window_mb, rhat_rows=None):
    import math
    if int(max_iter) == 0:
        raise RuntimeError("max_iter must be > 0")
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be finite and > 0")
    if not (math.isfinite(std_eps) and std_eps > 0.0):
        raise RuntimeError("std_eps must be finite and > 0")
    if not (math.isfinite(lbd) and lbd >= 0.0):
        raise RuntimeError("lbd must be finite and >= 0")
    mode = str(scan_mode).strip().lower()
    if mode not in ("approx", "exact"):
        raise RuntimeError(f"unsupported SparseLMM scan mode: {scan_mode}")
    if mode == "approx" and int(rhat_markers) == 0:
        raise RuntimeError("rhat_markers must be > 0")
    inp = _splmm_prepare_inputs(prefix, y, x_cov, sample_indices, operator_sample_indices, site_keep, packed,
                                packed_n_samples, maf, row_flip, row_missing, row_indices, model, mmap_window_mb)
    path = sparse_jxgrm_path if sparse_jxgrm_path else _normalize_spgrm_path(_bed_prefix(prefix))
    sp_idx = inp["op_idx"] if sparse_sample_indices is None else _c(sparse_sample_indices, np.int64).ravel()
    if sp_idx is not None and sp_idx.shape[0] != inp["n"]:
        raise RuntimeError(f"sparse_sample_indices length mismatch: got {sp_idx.shape[0]}, expected {inp['n']}")
    lam = float(lbd)
    if mode == "exact":
        if inp["gm_code"] != 0:      # `exact_scan_blocks_core`, src/stats/splmm.rs:2662-2664
            raise RuntimeError("SparseLMM exact denominator mode requires additive model")
        if not lam > 0.0:
            raise RuntimeError("K + lambda I is not positive definite at lambda=0")
        out, _l10, _null = splmm_exact_scan_from_jxgrm(path, inp["y"], inp["pk"], inp["n_full"],
                                                       _expand_rows(inp["maf"], inp["rows"], inp["pk"].shape[0]),
                                                       _expand_rows(inp["flip"], inp["rows"], inp["pk"].shape[0]),
                                                       inp["x_cov"], inp["scan_idx"], inp["rows"], math.log10(lam),
                                                       grm_sample_indices=sp_idx)
        r_hat, req, used = float("nan"), 0, 0
    else:
        spm = _sparse_reml_model(path, inp["y"], inp["x_cov"], sp_idx)
        if not spm.factorizable(lam) and not (lam == 0.0 and spm.smin > 0.0):
            raise RuntimeError(f"K + lambda I is not positive definite at lambda={lam}")
        r_hat, out_t, req, used = _splmm_approx_scan(spm, lam, inp["pk"], inp["n_full"], inp["maf"], inp["flip"],
                                                     inp["rows"], inp["scan_idx"], int(rhat_markers), int(rhat_seed),
                                                     rhat_rows, gm_code=inp["gm_code"])
        out = out_t.cpu().numpy()
        req = int(rhat_markers)
    _done(progress_callback, len(inp["rows"]))
    n_all, col_ptr, _r, _v = load_spgrm(path)
    return inp, r_hat, out, req, used, int(col_ptr[-1])


def _expand_rows(values, rows, m_total):
    """Row metadata given for the selected rows -> an array indexed by payload row (what the packed entry points take)."""
    full = np.zeros(int(m_total), dtype=np.asarray(values).dtype)
    full[rows] = values
    return full


def splmm_assoc_pcg_bed(prefix, y, lbd, x_cov=None, sample_indices=None, operator_sample_indices=None, site_keep=None,
                        tol=1e-5, max_iter=200, block_rows=0, std_eps=1e-12, use_train_maf=True, threads=0, model="add",
                        rhat_markers=SPLMM_DEFAULT_RHAT_MARKERS, rhat_seed=SPLMM_DEFAULT_RHAT_SEED, packed=None,
                        packed_n_samples=0, maf=None, row_flip=None, row_missing=None, row_indices=None,
                        sparse_sample_indices=None, sparse_jxgrm_path=None, stage1_progress_callback=None,
                        scan_progress_callback=None, progress_every=0, rhat_tol=1e-3, scan_mode="exact",
                        mmap_window_mb=None, rhat_rows=None):
    """src/stats/splmm.rs:4608-4773 -> (r_hat, y_converged, y_iters, y_rel_res, x_converged_all, x_max_iters, x_max_rel_res,
    rhat_markers_requested, rhat_markers_used, stats f64 (m, 3), factor_nnz).  scan_mode "exact" = null state + score-form
    exact scan at the given lambda (`estimate_rhat_and_scan_sparse`, :3711); "approx" = the residualised GRAMMAR-gamma route
    (`estimate_residualized_approx_scan_sparse`, src/stats/splmm_approx.rs:701).  V^-1 comes from the eigendecomposition of
    the sparse K, so the solve diagnostics are those of a direct method (converged, one iteration, zero residual: what the
    reference reports for its sparse Cholesky, :3620-3645); `factor_nnz` is the number of stored entries of the sparse GRM
    (no L factor exists here).  `rhat_rows` (extension) overrides the seeded choice of the sampled markers."""
    inp, r_hat, out, req, used, nnz = _splmm_assoc(prefix, y, lbd, x_cov, sample_indices, operator_sample_indices, site_keep,
                                                   tol, max_iter, block_rows, std_eps, threads, model, rhat_markers,
                                                   rhat_seed, packed, packed_n_samples, maf, row_flip, row_missing,
                                                   row_indices, sparse_sample_indices, sparse_jxgrm_path,
                                                   scan_progress_callback, progress_every, scan_mode, mmap_window_mb,
                                                   rhat_rows)
    return (r_hat, True, 1, 0.0, True, 1, 0.0, req, used, out, nnz)


def splmm_assoc_pcg_bed_to_tsv(prefix, y, lbd, chrom, pos, snp, allele0, allele1, out_tsv, x_cov=None, sample_indices=None,
                               operator_sample_indices=None, site_keep=None, tol=1e-5, max_iter=200, block_rows=0,
                               std_eps=1e-12, use_train_maf=True, threads=0, model="add",
                               rhat_markers=SPLMM_DEFAULT_RHAT_MARKERS, rhat_seed=SPLMM_DEFAULT_RHAT_SEED, packed=None,
                               packed_n_samples=0, maf=None, row_flip=None, row_missing=None, row_indices=None,
                               sparse_sample_indices=None, sparse_jxgrm_path=None, stage1_progress_callback=None,
                               scan_progress_callback=None, progress_every=0, rhat_tol=1e-3, scan_mode="exact",
                               mmap_window_mb=None, rhat_rows=None):
    """src/stats/splmm.rs:4775-5026 -> (r_hat, y_converged, y_iters, y_rel_res, x_converged_all, x_max_iters, x_max_rel_res,
    rhat_markers_requested, rhat_markers_used, rows written, (prepare, bim, null + scan, writer wait, ...) seconds); the TSV
    has the Basic3 schema with `af` = row_maf and `miss` = the missing rate (:461-475).  Empty metadata lists: the BIM file
    of `prefix` is read for the selected rows."""
    import time
    from .tsv import write_assoc_tsv
    t0 = time.perf_counter()
    inp, r_hat, out, req, used, _nnz = _splmm_assoc(prefix, y, lbd, x_cov, sample_indices, operator_sample_indices, site_keep,
                                                    tol, max_iter, block_rows, std_eps, threads, model, rhat_markers,
                                                    rhat_seed, packed, packed_n_samples, maf, row_flip, row_missing,
                                                    row_indices, sparse_sample_indices, sparse_jxgrm_path,
                                                    scan_progress_callback, progress_every, scan_mode, mmap_window_mb,
                                                    rhat_rows)
    t1 = time.perf_counter()
    m = out.shape[0]
    if not len(chrom):
        from .bed import read_bim
        chrom, pos, snp, allele0, allele1 = read_bim(_bed_prefix(prefix)).columns(inp["rows"])
    elif not (len(chrom) == len(pos) == len(snp) == len(allele0) == len(allele1) == m):
        raise RuntimeError(f"SparseLMM TSV metadata length mismatch: rows={m}")
    t2 = time.perf_counter()
    from .pipeline import dist_info
    if dist_info()[0] == 0:        # several ranks: every rank holds the gathered table, rank 0 writes it
        written = write_assoc_tsv(out_tsv, chrom, pos, snp, allele0, allele1, inp["maf"], inp["miss"], out, resolve=False)
    else:
        written = m
    t3 = time.perf_counter()
    return (r_hat, True, 1, 0.0, True, 1, 0.0, req, used, int(written), (0.0, t2 - t1, t1 - t0, t3 - t2))


def _bed_prefix(prefix):
    """PLINK prefix with a trailing .bed / .bim / .fam removed (`normalize_plink_prefix`, src/io/gfcore.rs)."""
    t = str(prefix).strip()
    return t[:-4] if t.lower().endswith((".bed", ".bim", ".fam")) else t


def _read_bed_payload(prefix):
    """PLINK .bed payload as (m, bps) uint8 plus n_samples (src/stats/lmm.rs:1050-1061, gfcore.rs:307-323)."""
    from .bed import read_bed_payload
    return read_bed_payload(prefix)


def prepare_bed_2bit_packed(prefix, maf_threshold, max_missing_rate, het_threshold, snps_only=False):
    """src/io/gfreader.rs:7029-7110 (the packed workflow's loader + QC) ->
    (packed_keep u8 (k, bps), missing_rate f32 (k), maf f32 (k) [alt allele frequency], std_denom f32 (k),
    row_flip bool (k) [all False], site_keep bool (m), n_samples, n_snps_total).
    Row counts come from the device popcount kernel; thresholds out of range raise ValueError like the reference."""
    from . import stats as st
    from .bed import read_bed_payload, snps_only_mask
    if not (0.0 <= maf_threshold <= 0.5):
        raise ValueError("maf_threshold must be within [0, 0.5]")
    if not (0.0 <= max_missing_rate <= 1.0):
        raise ValueError("max_missing_rate must be within [0, 1.0]")
    if not (0.0 <= het_threshold <= 1.0):
        raise ValueError("het_threshold must be within [0, 1.0]")
    low = str(prefix).lower()
    if low.endswith((".bed", ".bim", ".fam")):
        prefix = str(prefix)[:-4]
    packed, n_fam, bim = read_bed_payload(prefix)
    counts = bed_row_counts(packed, n_fam, None)
    keep, miss, maf, std = st.packed_prep_row_stats(counts, n_fam, maf_threshold, max_missing_rate, het_threshold)
    if snps_only:
        keep &= snps_only_mask(bim)
    if not keep.any():
        raise RuntimeError("No SNPs left after packed BED filtering. Please relax thresholds.")
    rows = np.nonzero(keep)[0]
    return (np.ascontiguousarray(packed[rows]), miss[rows], maf[rows], std[rows], np.zeros(len(rows), dtype=bool),
            keep, int(n_fam), int(packed.shape[0]))


def grm_packed_bed_f32(prefix, method=1, maf_threshold=0.02, max_missing_rate=0.05, het_threshold=0.0,
                       snps_only=False, block_cols=65536, threads=0, progress_callback=None, progress_every=0):
    """src/stats/grm.rs:3757-3839: `prepare_bed_2bit_packed` then `grm_packed_f32` -> (f32 (n,n), eff_m, n_samples)."""
    maf_thr = min(max(float(maf_threshold), 0.0), 0.5)
    miss_thr = min(max(float(max_missing_rate), 0.0), 1.0)
    pk, _miss, maf, _std, flip, _keep, n, _tot = prepare_bed_2bit_packed(prefix, maf_thr, miss_thr,
                                                                        min(max(float(het_threshold), 0.0), 1.0),
                                                                        snps_only)
    k = grm_packed_f32(pk, n, flip, maf, None, method, block_cols, threads, progress_callback, progress_every)
    return k, int(pk.shape[0]), n


def grm_stream_bed_f32(prefix, method=1, maf_threshold=0.02, max_missing_rate=0.05, het_threshold=0.0,
                       snps_only=False, block_cols=65536, threads=0, progress_callback=None, progress_every=0,
                       mmap_window_mb=None):
    """src/stats/grm.rs:4676-4703 -> (f32 (n,n), eff_m, n_samples).  The payload is staged to HBM in windows of
    `mmap_window_mb` MiB (bed.stage_bed_payload: the reference's WindowedBedMatrix role); no host copy of it is made."""
    import torch
    from .bed import snps_only_mask, stage_bed_payload
    packed, n_samples, bim = stage_bed_payload(_bed_prefix(prefix), mmap_window_mb)
    if snps_only:
        packed = packed[torch.from_numpy(np.nonzero(snps_only_mask(bim))[0]).to(packed.device)]
    k, eff, _ = grm_stream_payload_f32(packed, n_samples, method, maf_threshold, max_missing_rate, het_threshold)
    _done(progress_callback, int(packed.shape[0]))
    return k, int(eff), int(n_samples)


def grm_stream_payload_f32(packed, n_samples, method=1, maf_threshold=0.02, max_missing_rate=0.05,
                           het_threshold=0.0):
    """In-memory form of `grm_stream_bed_f32` -> (K f32, eff_m, keep mask); `packed`: host array or device tensor."""
    n = int(n_samples)
    _pk, pk_ptr, m = _payload(packed, n)
    out = np.empty((n, n), dtype=np.float32)
    eff = np.zeros(1, dtype=np.int64)
    keep = np.zeros(m, dtype=np.uint8)
    check(lib().jx_grm_stream_payload_f32(pk_ptr, m, n, int(method), float(maf_threshold),
                                          float(max_missing_rate), float(het_threshold), _p(out), _p(eff), _p(keep)))
    return out, int(eff[0]), keep.astype(bool)


def grm_stream_bed_f32_to_npy(prefix, out_path, method=1, maf_threshold=0.02, max_missing_rate=0.05,
                              het_threshold=0.0, snps_only=False, block_cols=65536, threads=0,
                              progress_callback=None, progress_every=0, mmap_window_mb=None):
    """src/stats/grm.rs:5517-5545: writes NPY v1 f32 C-order, returns (eff_m, n_samples)."""
    k, eff, n = grm_stream_bed_f32(prefix, method, maf_threshold, max_missing_rate, het_threshold, snps_only,
                                   mmap_window_mb=mmap_window_mb)
    tmp = f"{out_path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as fh:
        np.lib.format.write_array(fh, np.ascontiguousarray(k, dtype=np.float32), version=(1, 0))
    os.replace(tmp, out_path)
    _done(progress_callback, eff)
    return eff, n


# ------------------------------------------------------------------------------------------------
# eigh  (src/math/eigh.rs)
# ------------------------------------------------------------------------------------------------

def grm_bed_f64_from_meta(prefix, row_indices, row_flip, row_maf, sample_indices=None, method=1, block_cols=65536,
                          threads=0, progress_callback=None, progress_every=0, mmap_window_mb=None):
    """src/stats/grm.rs:3639-3753 -> `build_grm_from_meta_stream` (src/stats/gblup.rs:406-652): the GRM of the BED rows
    `row_indices` over `sample_indices` with the caller's flip / allele-frequency metadata (`jx grm` after its own QC,
    python/janusx/script/grm.py:1365; `jx gs`, python/janusx/gs/workflow.py:4139) -> f64 (n, n).  method 1: centred
    additive, scaled by 1 / sum(2p(1-p)); method 2: standardised additive, scaled by 1 / m; 3 (dominance) is not built."""
    import torch
    from .bed import stage_bed_payload
    if int(method) not in (1, 2, 3):
        raise RuntimeError(f"unsupported method={method}; expected 1 (centered additive), 2 (standardized additive), or 3 "
                           "(centered dominance)")
    if int(method) == 3:
        raise RuntimeError("method=3 (centered dominance) is outside this build's scope (additive GRMs only)")
    packed, n_fam, _bim = stage_bed_payload(_bed_prefix(prefix), mmap_window_mb)
    if n_fam == 0:
        raise RuntimeError("no samples found in PLINK input")
    src = _c(row_indices, np.int64).ravel()
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if src.size == 0:
        raise RuntimeError("row_indices must not be empty")
    if flip.shape[0] != src.shape[0] or maf.shape[0] != src.shape[0]:
        raise RuntimeError(f"row meta length mismatch: row_indices={src.shape[0]}, row_flip={flip.shape[0]}, "
                           f"row_maf={maf.shape[0]}")
    if (src < 0).any():
        raise RuntimeError(f"row index must be non-negative, got {int(src[src < 0][0])}")
    if int(src.max()) >= int(packed.shape[0]):
        raise RuntimeError("row index out of range")
    if sample_indices is None:
        tr = np.arange(n_fam, dtype=np.int64)
    else:
        tr = _c(sample_indices, np.int64).ravel()
        if tr.size == 0:
            raise RuntimeError("sample_indices must not be empty")
        if tr.min() < 0 or tr.max() >= n_fam:
            raise RuntimeError("sample_indices out of range")
    rows_payload = packed[torch.from_numpy(src).to(packed.device)]
    del packed
    if int(method) == 1:
        k, _var_sum, _panel, _row_mean = _gblup_meta_grm(rows_payload, n_fam, tr, flip, maf)
        out = k.cpu().numpy()
    else:
        out = grm_packed_f64(rows_payload.cpu().numpy(), n_fam, flip, maf, None if sample_indices is None else tr, 2,
                             block_cols, threads)
    if progress_callback is not None:
        progress_callback(int(src.shape[0]), int(src.shape[0]))
    return np.ascontiguousarray(out, dtype=np.float64)


def _write_npy_f32(out_path, arr):
    tmp = f"{out_path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as fh:
        np.lib.format.write_array(fh, np.ascontiguousarray(arr, dtype=np.float32), version=(1, 0))
    os.replace(tmp, out_path)


def gblup_grm_from_meta_to_npy(prefix, out_npy_path, row_source_indices, row_flip, row_maf, sample_indices=None, method=1,
                               block_rows=65536, threads=0, progress_callback=None, progress_every=0, mmap_window_mb=None):
    """src/stats/gblup.rs:718-857: `build_grm_from_meta_stream` written as NPY v1 f32 (`jx grm` rust-meta route,
    python/janusx/script/grm.py:1459) -> (eff_m, n_samples)."""
    k = grm_bed_f64_from_meta(prefix, row_source_indices, row_flip, row_maf, sample_indices, method, block_rows, threads,
                              None, 0, mmap_window_mb)
    _write_npy_f32(out_npy_path, k)
    eff_m = int(np.asarray(row_source_indices).ravel().shape[0])
    if progress_callback is not None:
        progress_callback(eff_m, eff_m)
    return eff_m, int(k.shape[0])


_DENSE_META_GRM_CACHE = {}      # one entry: the dense GRM a sequence of row-band calls is cut from


def _dense_grm_from_meta_f32(prefix, row_source_indices, row_flip, row_maf, n_total_sites, sample_indices, method,
                             mmap_window_mb, what):
    """Dense GRM under the conventions of the sparse-GRM stream core (`grm_stream_bed_row_band_f32_fill_core`,
    src/stats/spgrm.rs:4266-4570): rows decoded with mean 2 maf (clamped) and, for method 2, 1 / sqrt(2p(1-p)) (0 below
    1e-12), missing = mean; denominator = the f64 sum of the positive finite 2p(1-p) (method 1) or m (method 2) whatever
    the sample selection.  -> (K f32 (n_use, n_use) on the host, eff_m, n_use).  The reference builds the matrix band by
    band to bound host memory; here the whole accumulator lives in HBM and consecutive band calls on the same inputs are
    cut from one cached matrix."""
    import hashlib
    import torch
    from . import pipeline as pl
    from . import stats as st
    from .bed import stage_bed_payload
    bed_prefix = _bed_prefix(prefix)
    if int(n_total_sites) <= 0:
        raise RuntimeError(f"n_total_sites must be positive for dense GRM {what} meta route.")
    if int(method) not in (1, 2):
        raise RuntimeError(f"Dense GRM part method must be 1 (centered) or 2 (standardized); got {method}")
    src = _c(row_source_indices, np.int64).ravel()
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if src.size == 0:
        raise RuntimeError("row_source_indices must not be empty")
    if (src < 0).any():
        raise RuntimeError(f"row_source_indices must be non-negative, got {int(src[src < 0][0])}")
    if flip.shape[0] != src.shape[0] or maf.shape[0] != src.shape[0]:
        raise RuntimeError(f"row meta length mismatch: row_source_indices={src.shape[0]}, row_flip={flip.shape[0]}, "
                           f"row_maf={maf.shape[0]}")
    if int(src.max()) >= int(n_total_sites):
        raise RuntimeError(f"row_source index out of range: {int(src[src >= int(n_total_sites)][0])} >= "
                           f"n_total_sites={int(n_total_sites)}")
    idx, n_sel = _opt_idx(sample_indices)
    st_bed = os.stat(bed_prefix + ".bed")
    h = hashlib.sha1()
    for a in (src, flip.astype(np.uint8), maf, idx if idx is not None else np.zeros(0, np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (os.path.abspath(bed_prefix), st_bed.st_size, st_bed.st_mtime_ns, int(method), h.hexdigest())
    hit = _DENSE_META_GRM_CACHE.get(key)
    if hit is not None:
        return hit
    _DENSE_META_GRM_CACHE.clear()
    packed, n_fam, _bim = stage_bed_payload(bed_prefix, mmap_window_mb)
    if n_fam == 0:
        raise RuntimeError("No samples found in BED input.")
    if int(src.max()) >= int(packed.shape[0]):
        raise RuntimeError(f"row_source index out of range for the BED payload: {int(src.max())} >= {int(packed.shape[0])}")
    if idx is not None and n_sel and (idx.min() < 0 or idx.max() >= n_fam):
        raise RuntimeError(f"Dense GRM part sample index out of range: {int(idx.max())} >= {n_fam}")
    n_use = n_sel if (idx is not None and n_sel) else n_fam
    m = int(src.shape[0])
    if int(method) == 1:
        v = 2.0 * maf.astype(np.float64) * (1.0 - maf.astype(np.float64))
        denom = float(np.sum(v[np.isfinite(v) & (v > 0.0)]))
        if not (np.isfinite(denom) and denom > 0.0):
            raise RuntimeError("Dense GRM part centered denominator is not positive")
    else:
        denom = float(m)
    rows_payload = packed[torch.from_numpy(src).to(packed.device)]
    del packed
    panel = pl.Panel(rows_payload, n_fam, idx if (idx is not None and n_sel) else None)
    acc = pl.grm_accumulate(panel, np.arange(m, dtype=np.int64), st.grm_lut_from_maf(maf, flip, int(method)))
    k = pl.grm_finalize(acc, n_use, denom, torch.float32).cpu().numpy()
    del acc
    out = (k, m, n_use)
    if k.nbytes <= (8 << 30):
        _DENSE_META_GRM_CACHE[key] = out
    return out


def _row_band(k, row_part_start, row_part_end):
    n_use = int(k.shape[0])
    a, b = int(row_part_start), int(row_part_end)
    if a >= b or b > n_use:
        raise RuntimeError(f"row band is invalid: start={a}, end={b}, n_samples={n_use}")
    # the band holds the LOWER triangle only (column <= global row; `spgrm_collect_batch_dense_rows`, spgrm.rs:2706-2753): the
    # caller mirrors when it assembles the parts
    return np.ascontiguousarray(np.tril(k[a:b], k=a))


def grm_bed_f32_row_band_from_meta(prefix, row_source_indices, row_flip, row_maf, n_total_sites, row_part_start,
                                   row_part_end, sample_indices=None, method=1, block_rows=0, sample_block=0, threads=0,
                                   mmap_window_mb=None, progress_callback=None, progress_every=0):
    """src/stats/spgrm.rs:5496-5642: rows [row_part_start, row_part_end) of the dense GRM of caller-prepared BED rows
    (`jx grm` part builds, python/janusx/script/grm.py:819) -> (f32 (part_rows, n_use), eff_m, n_use)."""
    k, eff_m, n_use = _dense_grm_from_meta_f32(prefix, row_source_indices, row_flip, row_maf, n_total_sites, sample_indices,
                                               method, mmap_window_mb, "part")
    band = _row_band(k, row_part_start, row_part_end)
    if progress_callback is not None:
        progress_callback(eff_m, eff_m)
    return band, eff_m, n_use


def grm_bed_f32_row_band_from_meta_to_npy(prefix, out_npy_path, row_source_indices, row_flip, row_maf, n_total_sites,
                                          row_part_start, row_part_end, sample_indices=None, method=1, block_rows=0,
                                          sample_block=0, threads=0, mmap_window_mb=None, progress_callback=None,
                                          progress_every=0):
    """src/stats/spgrm.rs:5644-5783: the same band written as NPY v1 f32 (part_rows, n_use) -> (eff_m, n_use)."""
    k, eff_m, n_use = _dense_grm_from_meta_f32(prefix, row_source_indices, row_flip, row_maf, n_total_sites, sample_indices,
                                               method, mmap_window_mb, "part")
    _write_npy_f32(out_npy_path, _row_band(k, row_part_start, row_part_end))
    if progress_callback is not None:
        progress_callback(eff_m, eff_m)
    return eff_m, n_use


def grm_bed_f32_tiled_from_meta_to_npy(prefix, out_npy_path, row_source_indices, row_flip, row_maf, n_total_sites,
                                       sample_indices=None, method=1, block_rows=0, sample_block=0, threads=0,
                                       mmap_window_mb=None, progress_callback=None, progress_every=0):
    """src/stats/spgrm.rs:5785-5922: the whole dense GRM of caller-prepared BED rows written as NPY v1 f32 (n_use, n_use)
    -> (eff_m, n_use) (`jx grm` tiled route, python/janusx/script/grm.py:985)."""
    k, eff_m, n_use = _dense_grm_from_meta_f32(prefix, row_source_indices, row_flip, row_maf, n_total_sites, sample_indices,
                                               method, mmap_window_mb, "tiled")
    _write_npy_f32(out_npy_path, k)
    if progress_callback is not None:
        progress_callback(eff_m, eff_m)
    return eff_m, n_use


def rust_eigh_from_array_f64(a, threads=0, driver=None, jobz="V", require_lapack=False, diag_shift=0.0):
    """src/math/eigh.rs:1621-1703 -> 10-tuple (evals asc, evecs (columns) or None, blas_backend, evd_backend,
    n, threads_before, threads_in_stage, threads_after, lapack_used, elapsed_s)."""
    a = _c(a, np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise RuntimeError("matrix must be square")
    n = int(a.shape[0])
    if n == 0:
        raise RuntimeError("matrix must be non-empty")
    import torch
    t0 = time.perf_counter()
    stream = torch.cuda.current_stream().cuda_stream
    d_a = torch.tensor(a, device=torch.device("cuda", torch.cuda.current_device()))       # a copy: overwritten with U^T
    d_w = torch.empty(n, dtype=torch.float64, device=d_a.device)
    check(lib().jxg_symmetrize_f64(d_a.data_ptr(), n, stream))                             # eigh.rs:179
    check(lib().jxg_eigh_f64(d_a.data_ptr(), n, float(diag_shift), d_w.data_ptr(), stream))
    evals, evecs = d_w.cpu().numpy(), None
    if str(jobz).upper() != "N":
        d_u = torch.empty_like(d_a)
        check(lib().jxg_transpose_f64(d_a.data_ptr(), d_u.data_ptr(), n, stream))          # U^T -> U (columns = vectors)
        evecs = d_u.cpu().numpy()
    # which solver ran (csrc/eigh.cpp): rocSOLVER below n = 256 or on request, else the own one- or two-stage reduction
    # + own divide and conquer (jxg_last_kernel_ms(10) = 1 after a two-stage decomposition)
    if n < 256 or os.environ.get("JXGPU_EIGH", "") == "rocsolver":
        evd = "rocsolver_dsyevd"
    elif float(lib().jxg_last_kernel_ms(10)) > 0.5:
        evd = "jxgpu_sy2sb_sb2st_stedc"
    else:
        evd = "jxgpu_sytrd_stedc"
    return (evals, evecs, "rocblas", evd, n, 0, 0, 0, True, time.perf_counter() - t0)


def rust_eigh_from_array_f64_inplace(a, threads=0, driver=None, jobz="V", require_lapack=False):
    """src/math/eigh.rs:1883-1962.  Same 10-tuple as `rust_eigh_from_array_f64`.  Despite its name the reference's function
    does NOT write into its argument: it takes `a.readonly()` (:1914), hands a row-major copy-on-write view to
    `symmetric_eigh_f64_row_major_with_driver` (:1918, :1925) and returns freshly allocated arrays (:1943-1955) -- "in place"
    there is about not copying a contiguous input on the way IN.  What it does differently from the plain entry point, and what
    this mirror reproduces: no `diag_shift` argument, an empty or non-square input is refused with its own message (:1907-1912),
    and a Fortran-ordered / strided input is accepted (read through `_c`).  The caller's array is left untouched."""
    arr = np.asarray(a)
    nrows = int(arr.shape[0]) if arr.ndim >= 1 else 0
    ncols = int(arr.shape[1]) if arr.ndim >= 2 else 0
    if arr.ndim != 2 or nrows == 0 or ncols == 0 or nrows != ncols:
        raise RuntimeError(f"rust_eigh_from_array_f64_inplace expects a non-empty square matrix; got shape=({nrows}, {ncols})")
    return rust_eigh_from_array_f64(arr, threads, driver, jobz, require_lapack, 0.0)


def rust_eigh_from_matrix_file_f64(path, threads=0, driver=None, jobz="V", require_lapack=False, diag_shift=0.0):
    """src/math/eigh.rs:1707-1786: `.npy` (f32/f64 C-order) or whitespace text matrix."""
    a = np.load(path) if str(path).endswith(".npy") else np.loadtxt(path)
    return rust_eigh_from_array_f64(np.asarray(a, dtype=np.float64), threads, driver, jobz, require_lapack, diag_shift)


def rust_eigh_from_matrix_file_subset_f64(path, subset, threads=0, driver=None, jobz="V", require_lapack=False,
                                          diag_shift=0.0):
    """src/math/eigh.rs:1788-1880."""
    a = np.load(path, mmap_mode="r") if str(path).endswith(".npy") else np.loadtxt(path)
    ix = np.asarray(subset, dtype=np.int64)
    sub = np.asarray(a[np.ix_(ix, ix)], dtype=np.float64)
    return rust_eigh_from_array_f64(sub, threads, driver, jobz, require_lapack, diag_shift)


def rust_sgemm_backend():
    return "hip-mfma-gfx950"


def rust_eigh_lapack_backend():
    return "rocsolver"


def rust_blas_get_num_threads():
    return 0


def rust_blas_set_num_threads(n):
    return None


# ------------------------------------------------------------------------------------------------
# argument front end of the association mirrors (LMM, fvLMM, LMM2, LM): each check of the reference written once, the caller
# passes its name or its message where the reference words a refusal differently
# ------------------------------------------------------------------------------------------------

def _assoc_check_bounds(low, high):
    if low >= high:
        raise RuntimeError("low must be < high")


def _assoc_check_tol(tol):
    if not (np.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be positive and finite")


def _assoc_start(init_log10_lbd, low, high):
    """Brent's start of the exact scans: a finite `init_log10_lbd` clamped to [low, high], else None (the interval midpoint)."""
    if init_log10_lbd is not None and np.isfinite(init_log10_lbd):
        return float(min(max(init_log10_lbd, low), high))
    return None


def _assoc_u_t(u_t, n, msg="u_t must be (n, n) and row-major U^T"):
    u_t = _c(u_t, np.float32)
    if u_t.shape != (n, n):
        raise RuntimeError(msg)
    return u_t


def _assoc_dense_chunk(chunk, n, msg):
    """A dense SNP-major f32 chunk (rows, n)."""
    g = _c(chunk, np.float32)
    if g.ndim != 2 or g.shape[1] != n:
        raise RuntimeError(msg)
    return g


def _assoc_chunk_args(s, xcov, y_rot, chunk, u_t, what):
    """The opening of the chunk functions: null model, the chunk `what` against n, U^T against n when the rows are still to be
    rotated (u_t None: they are rotated already).  -> (s, xcov, y, n, p, chunk f32, u_t f32 | None)."""
    s, xcov, y, n, p = _null_args(s, xcov, y_rot)
    g = _assoc_dense_chunk(chunk, n, f"{what} must be (m_chunk, n)")
    return s, xcov, y, n, p, g, None if u_t is None else _assoc_u_t(u_t, n)


def _assoc_fam_positions(fam, sample_ids, shown):
    """Sample ids -> their positions in the FAM order `fam` (int64); `shown` renders the first id that is not there."""
    pos = {sid: i for i, sid in enumerate(fam)}
    for x in sample_ids:
        if str(x) not in pos:
            raise RuntimeError(f"sample id not found in FAM: {shown(str(x))}")
    return np.array([pos[str(x)] for x in sample_ids], dtype=np.int64)


def _assoc_prepared_given(row_indices, row_flip, row_missing, row_maf):
    """Prepared row metadata arrives as all four arrays or none -> whether it is given."""
    given = [a is not None for a in (row_indices, row_flip, row_missing, row_maf)]
    if any(given) and not all(given):
        raise RuntimeError("prepared row metadata must provide all or none of: row_indices, row_flip, row_missing, row_maf")
    return all(given)


def _assoc_check_qc(maf_threshold, max_missing_rate, het_threshold):
    if not (0.0 <= maf_threshold <= 0.5):
        raise ValueError("maf_threshold must be within [0, 0.5]")
    if not (0.0 <= max_missing_rate <= 1.0):
        raise ValueError("max_missing_rate must be within [0, 1.0]")
    if not (0.0 <= het_threshold <= 1.0):
        raise ValueError("het_threshold must be within [0, 1.0]")


# ------------------------------------------------------------------------------------------------
# null model helpers  (src/stats/reml.rs)
# ------------------------------------------------------------------------------------------------

def lmm_rotate_x_y_with_ut_f64(u_t, x, y, threads=0):
    """src/stats/reml.rs:107-198 -> (f64 (n,q), f64 (n,1))."""
    y = _c(y, np.float64).ravel()
    n = int(y.shape[0])
    if n == 0:
        raise RuntimeError("y must not be empty")
    x = _c(x, np.float64)
    if x.ndim != 2:
        raise RuntimeError("x must be 2D (n, q)")
    if x.shape[0] != n:
        raise RuntimeError(f"x rows must equal len(y): rows={x.shape[0]}, len(y)={n}")
    u_t = _assoc_u_t(u_t, n, "u_t must be shape (n, n) and row-major U^T")
    q = int(x.shape[1])
    if q > 15:
        raise RuntimeError("x must have between 0 and 15 columns")
    import torch
    d_ut = torch.tensor(u_t, device=torch.device("cuda", torch.cuda.current_device()))
    d_xy = torch.from_numpy(np.concatenate([x, y[:, None]], axis=1)).to(d_ut.device)     # [X | y] side by side
    d_out = torch.empty_like(d_xy)
    check(lib().jxg_rotate_xy(d_ut.data_ptr(), n, d_xy.data_ptr(), q + 1, d_out.data_ptr(),
                              torch.cuda.current_stream().cuda_stream))
    out = d_out.cpu().numpy()
    return np.ascontiguousarray(out[:, :q]), np.ascontiguousarray(out[:, q:])


def lmm_rotate_y_with_ut_f64(u_t, y, threads=0):
    """src/stats/reml.rs:200-250 -> y_rot f64 (n): row i = <u_t[i, :], y> in f64 (what `workflow_model_packed.py:6309` calls
    per trait once X has been rotated)."""
    y = _c(y, np.float64).ravel()
    n = int(y.shape[0])
    if n == 0:
        raise RuntimeError("y must not be empty")
    u_t = _c(u_t, np.float32)
    if u_t.ndim != 2:
        raise RuntimeError("u_t must be 2D (n, n)")
    u_t = _assoc_u_t(u_t, n, "u_t must be shape (n, n) and row-major U^T")
    return lmm_rotate_x_y_with_ut_f64(u_t, np.zeros((n, 1), dtype=np.float64), y)[1].ravel()      # beside one zero column


def _null_args(s, xcov, y_rot):
    s = _c(s, np.float64).ravel()
    xcov = _c(xcov, np.float64)
    y = _c(y_rot, np.float64).ravel()
    n = int(y.shape[0])
    if xcov.ndim != 2 or xcov.shape[0] != n:
        raise RuntimeError("Xcov.n_rows must equal len(y_rot)")
    if s.shape[0] != n:
        raise RuntimeError("len(S) must equal len(y_rot)")
    return s, xcov, y, n, int(xcov.shape[1])


def lmm_reml_null_f32(s, xcov, y_rot, low, high, max_iter=50, tol=1e-2):
    """src/stats/reml.rs:570-616 -> (lbd, ml, reml)."""
    s, xcov, y, _n, _p_cov = _null_args(s, xcov, y_rot)
    _assoc_check_bounds(low, high)
    return _dense_model(s, xcov, y).reml_null(low, high, max_iter, tol)


def ml_loglike_null_f32(s, xcov, y_rot, log10_lbd):
    """src/stats/reml.rs:618-646 -> ML profile log-likelihood of the null model at log10 lambda (-1e8 on failure)."""
    return _loglike_null(s, xcov, y_rot, log10_lbd)[0]


def _loglike_null(s, xcov, y_rot, log10_lbd):
    """(ml, reml) of the null model at log10 lambda, one device launch (jxg_lmm_loglike_null)."""
    s, xcov, y, _n, _p_cov = _null_args(s, xcov, y_rot)
    return _dense_model(s, xcov, y).loglike_null(log10_lbd)


def _dense_model(s, xcov, y, u_t=None):
    """The caller's rotated null model (checked host arrays) on the current device: `pipeline.SpectralModel.rotated`; torch is
    imported here, behind every argument check."""
    import torch
    from . import pipeline as pl
    return pl.SpectralModel.rotated(s, u_t, xcov, y, torch.device("cuda", torch.cuda.current_device()))


def _scan_dense_chunk(g, s, xcov, y, u_t, mode, cols, **opts):
    """The dense-chunk scans of the mirror: `pipeline.scan_dense_rows` over the checked chunk `g` (m, n) f32 with the caller's
    rotated null model (u_t None: rows rotated already), in blocks of 4096 rows -> f64 (m, cols).  An empty chunk returns before
    the device is touched."""
    if g.shape[0] == 0:
        return np.zeros((0, cols), dtype=np.float64)
    from . import pipeline as pl
    return pl.scan_dense_rows(g, _dense_model(s, xcov, y, u_t), mode, **opts).cpu().numpy()


# ------------------------------------------------------------------------------------------------
# exact per-SNP scan  (src/stats/lmm.rs)
# ------------------------------------------------------------------------------------------------

def _chunk(s, xcov, y_rot, low, high, chunk, u_t, max_iter, tol, nullml, what):
    s, xcov, y, n, p, g, u_t = _assoc_chunk_args(s, xcov, y_rot, chunk, u_t, what)
    _assoc_check_bounds(low, high)
    return _scan_dense_chunk(g, s, xcov, y, u_t, "lmm", 4 if nullml is not None else 3, low=low, high=high, max_iter=max_iter,
                             tol=tol, nullml=nullml)


def lmm_reml_chunk_f32(s, xcov, y_rot, low, high, g_rot_chunk, max_iter=50, tol=1e-2, threads=0, nullml=None):
    """src/stats/lmm.rs:333-335 (already rotated rows) -> f64 (m, 3 or 4)."""
    return _chunk(s, xcov, y_rot, low, high, g_rot_chunk, None, max_iter, tol, nullml, "g_rot_chunk")


def lmm_reml_chunk_from_snp_f32(s, xcov, y_rot, low, high, snp_chunk, u_t, max_iter=50, tol=1e-2, threads=0,
                                nullml=None, rotate_block_rows=256):
    """src/stats/lmm.rs:1479-1630 (rotate then scan, no warm start) -> f64 (m, 3 or 4)."""
    return _chunk(s, xcov, y_rot, low, high, snp_chunk, u_t, max_iter, tol, nullml, "snp_chunk")


def _resolve_warm_start(warm_start, route_env=None):
    """`warm_start` of the exact-scan entry points -> "chain" | "none".  None = the reference's default: the chain
    (`carry_warm_start`, src/stats/lmm.rs:134-161), switched off by a truthy JX_LMM_UNIFIED_NO_WARM_START.  The reference reads
    that variable in the BED route only (:2627; its packed routes pass `true, true` unconditionally, :3244-3245, :3609-3610);
    here one setting gives every exact-scan entry point and `jx gwas -lmm` the no-chain scan."""
    from .stats import env_truthy
    if warm_start is None:
        return "none" if (route_env and env_truthy(route_env)) else "chain"
    w = str(warm_start).strip().lower()
    if w in ("chain", "carry", "on", "true", "1"):
        return "chain"
    if w in ("none", "off", "false", "0"):
        return "none"
    raise RuntimeError("warm_start must be 'chain' or 'none'")


def _assoc_packed(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, sample_indices, row_indices, mode, *,
                  low=None, high=None, max_iter=0, tol=1e-2, init_log10_lbd=None, log10_lbd=None, nullml=None,
                  progress_callback=None, progress_every=0, genetic_model="add", chain_off=None):
    """The packed scans of the mirror: mode "lmm" exact per-SNP REML on [low, high] from `init_log10_lbd` (along `chain_off`
    when given), "fvlmm" fixed lambda at `log10_lbd`, "lmm2" as "lmm" plus the ML ratio test (needs `nullml`)
    -> f64 (m, 3 | 4 with nullml | 6 for LMM2).  `pipeline.scan_rows` over a `Panel` of the (row-subsetted) payload with the
    caller's rotated null model, in blocks of 8192 rows."""
    from . import pipeline as pl
    from .stats import genetic_model_code, scan_lut_from_counts
    fixed = mode == "fvlmm"
    if fixed:           # no search: the interval's lower end carries the lambda to the kernel, which starts and stays there
        low, high, max_iter, tol = float(log10_lbd), float(log10_lbd) + 1.0, 0, 1e-2
    genetic_model_code(genetic_model)               # `PackedGeneticModel::parse` (src/decode/decode.rs:107-119)
    s, xcov, y, n, p = _null_args(s, xcov, y_rot)
    if row_indices is not None:
        ri = np.asarray(row_indices, dtype=np.int64)
        if _is_device_tensor(packed):
            import torch
            packed = packed[torch.from_numpy(ri).to(packed.device)]
        else:
            packed = np.ascontiguousarray(_c(packed, np.uint8)[ri])
    packed, _pk_ptr, m = _payload(packed, n_samples)           # host array or device tensor
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    u_t = _assoc_u_t(u_t, n)
    idx, n_sel = _opt_idx(sample_indices)
    n_eff = n_sel if idx is not None else int(n_samples)
    if n_eff != n:
        raise RuntimeError(f"selected sample count {n_eff} != len(y_rot) {n}")
    chain = chain_off is not None and mode == "lmm"
    if chain and m > 0:
        co = np.ascontiguousarray(chain_off, dtype=np.int64)
        if co.ndim != 1 or len(co) < 2:
            raise RuntimeError("chain offsets are required")
        if co[0] != 0 or co[-1] != m:
            raise RuntimeError("chain offsets must run from 0 to m")
        if np.any(np.diff(co) < 0):
            raise RuntimeError("chain offsets must ascend")
    if mode not in ("lmm", "fvlmm", "lmm2"):
        raise RuntimeError("mode must be 'lmm', 'fvlmm' or 'lmm2'")
    if mode == "lmm2" and not (nullml is not None and np.isfinite(nullml)):
        raise RuntimeError("nullml must be finite")
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if not fixed:
        _assoc_check_bounds(low, high)
        _assoc_check_tol(tol)
    if m == 0:
        return np.zeros((0, 6 if mode == "lmm2" else (4 if nullml is not None else 3)), dtype=np.float64)
    panel = _panel(packed, n_samples, idx)       # of the rows handed: its mean missing-call count picks the rotation path
    sm = pl.SpectralModel.rotated(s, u_t, xcov, y, panel.device)
    lut = scan_lut_from_counts(maf, flip, panel.counts(), n, model=genetic_model)
    out = pl.scan_rows(panel, sm, np.arange(m), lut, mode, low=float(low), high=float(high), max_iter=int(max_iter),
                       tol=float(tol), init_log10_lbd=low if fixed else _assoc_start(init_log10_lbd, low, high),
                       block_rows=8192, nullml=None if nullml is None else float(nullml), chain_off=co if chain else None,
                       progress=progress_callback, progress_every=progress_every)
    return out.cpu().numpy()


def lmm_reml_assoc_packed_f32(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, sample_indices=None,
                              row_indices=None, low=-5.0, high=5.0, max_iter=50, tol=1e-2, threads=0, model="add",
                              progress_callback=None, progress_every=0, nullml=None, init_log10_lbd=None,
                              rotate_block_rows=256, warm_start=None, warm_chain_pieces=1):
    """src/stats/lmm.rs:3040-3362 -> f64 (m, 3), or (m, 4) with `nullml` (plrt column, lmm.rs:202-330).

    Warm start (`warm_start`, None = the reference's default for this entry point = "chain"): the reference runs this scan
    with `seed_with_init_guess = carry_warm_start = true` (lmm.rs:3244-3245): inside a block of `rotate_block_rows` rows
    (blocks restart at every `progress_every` rows, :3253-3256) each SNP's Brent starts from the optimum of the valid SNP before it,
    the first one from `init_log10_lbd` or the interval midpoint (:134-161).  Here the chains run in parallel, one wave per
    chain, the rows of a chain in order -- bit-for-bit the sequential semantics.  rayon additionally cuts a block into pieces
    with a fresh state each (2 T pieces on T idle threads, more under work stealing: the reference's own output depends on
    scheduling); `warm_chain_pieces` (power of two) reproduces that halving deterministically, 1 = one chain per block.
    warm_start="none": every SNP starts from `init_log10_lbd` when given, else from the midpoint (the core-API contract,
    lmm.rs:1577-1579; what JX_LMM_UNIFIED_NO_WARM_START selects on the BED route)."""
    from .stats import warm_chain_blocks_packed, warm_chain_offsets
    _assoc_check_bounds(low, high)
    _assoc_check_tol(tol)
    chain_off = None
    if _resolve_warm_start(warm_start, "JX_LMM_UNIFIED_NO_WARM_START") == "chain":
        m_rows = int(len(row_indices)) if row_indices is not None else int(packed.shape[0])
        chain_off = warm_chain_offsets(warm_chain_blocks_packed(m_rows, rotate_block_rows, progress_every), m_rows,
                                       warm_chain_pieces)
    return _assoc_packed(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, sample_indices, row_indices, "lmm",
                         low=low, high=high, max_iter=max_iter, tol=tol, init_log10_lbd=init_log10_lbd, nullml=nullml,
                         progress_callback=progress_callback, progress_every=progress_every, genetic_model=model,
                         chain_off=chain_off)


# ------------------------------------------------------------------------------------------------
# fixed-lambda scan  (src/stats/fvlmm.rs)
# ------------------------------------------------------------------------------------------------

def _fv_chunk(s, xcov, y_rot, log10_lbd, chunk, u_t, nullml, what):
    s, xcov, y, n, p, g, u_t = _assoc_chunk_args(s, xcov, y_rot, chunk, u_t, what)
    return _scan_dense_chunk(g, s, xcov, y, u_t, "fvlmm", 4 if nullml is not None else 3, log10_lbd=float(log10_lbd),
                             nullml=nullml)


def fvlmm_assoc_chunk_f32(s, xcov, y_rot, log10_lbd, g_rot_chunk, threads=0, nullml=None):
    """src/stats/fvlmm.rs:1941-1994 -> f64 (m, 3 or 4)."""
    return _fv_chunk(s, xcov, y_rot, log10_lbd, g_rot_chunk, None, nullml, "g_rot_chunk")


def fvlmm_assoc_chunk_from_snp_f32(s, xcov, y_rot, log10_lbd, snp_chunk, u_t, threads=0, nullml=None,
                                   rotate_block_rows=512):
    """src/stats/fvlmm.rs:2114-2262 -> f64 (m, 3)."""
    return _fv_chunk(s, xcov, y_rot, log10_lbd, snp_chunk, u_t, nullml, "snp_chunk")


def _fixed_lambda_checks(s, xcov, y_rot, log10_lbd):
    """Argument checks shared by the fixed-lambda entry points (src/stats/lmm.rs:2025-2066, src/stats/fvlmm.rs:1816-1836)."""
    s_, xcov_, y_, n, p = _null_args(s, xcov, y_rot)
    if n <= p + 1:
        raise RuntimeError("n must be > p_cov+1")
    with np.errstate(over="ignore", under="ignore"):
        lbd = float(np.float64(10.0) ** np.float64(log10_lbd))     # powf semantics: inf / 0 instead of an exception
    if not (np.isfinite(lbd) and lbd > 0.0):
        raise RuntimeError("invalid log10_lbd")
    if np.any(s_ + lbd <= 0.0):
        raise RuntimeError("non-positive s[i]+lbd")
    return n, p


def lmm_assoc_chunk_f32(s, xcov, y_rot, log10_lbd, g_rot_chunk, threads=0, nullml=None):
    """src/stats/lmm.rs:2010-2224: Wald statistics of already rotated rows at ONE given lambda (the `lmm_assoc` wrapper of
    python/janusx/pyBLUP/assoc.py:1305-1345) -> f64 (m, 3 or 4).  The same sums as the fixed-lambda scan of `-fvlmm`
    (c = X'Wg, d = g'Wg, e = g'Wy with W = 1 / (s + lambda) held in f32); a row whose Schur complement is <= 1e-12 is
    (NaN, NaN, NaN) and its plrt entry keeps the 0.0 the output was allocated with (:2155-2160)."""
    _fixed_lambda_checks(s, xcov, y_rot, log10_lbd)
    out = _fv_chunk(s, xcov, y_rot, log10_lbd, g_rot_chunk, None, nullml, "g_rot_chunk")
    if nullml is not None:
        out[np.isnan(out[:, 2]), 3] = 0.0
    return out


def lmm_assoc_chunk_from_snp_f32(s, xcov, y_rot, log10_lbd, snp_chunk, u_t, threads=0, nullml=None,
                                 rotate_block_rows=512):
    """src/stats/lmm.rs:2226-2486: `lmm_assoc_chunk_f32` behind the rotation of raw SNP rows -> f64 (m, 3 or 4)."""
    _fixed_lambda_checks(s, xcov, y_rot, log10_lbd)
    out = _fv_chunk(s, xcov, y_rot, log10_lbd, snp_chunk, u_t, nullml, "snp_chunk")
    if nullml is not None:
        out[np.isnan(out[:, 2]), 3] = 0.0
    return out


class FvLmmAssocCache:
    """`FvLmmAssocCache` (src/stats/fvlmm.rs:1808-1849): the lambda-only state of the fixed-lambda scan (W, P y, W X, the
    Cholesky factor of X'WX, y'Py, df, log det V) prepared once per trait.  Here the handle keeps the host inputs; the
    device state is rebuilt per call by one small kernel (`jxg_fvlmm_prepare`)."""

    def __init__(self, s, xcov, y_rot, log10_lbd):
        self.n, self.p = _fixed_lambda_checks(s, xcov, y_rot, log10_lbd)
        self.s, self.xcov, self.y_rot = (np.array(_c(a, np.float64), copy=True) for a in (s, xcov, y_rot))
        self.log10_lbd = float(log10_lbd)
        self.lbd = float(np.float64(10.0) ** np.float64(self.log10_lbd))


def fvlmm_assoc_prepare_cache_f32(s, xcov, y_rot, log10_lbd):
    """src/stats/fvlmm.rs:1808-1849 -> cache handle for `fvlmm_assoc_chunk_with_cache_f32`."""
    return FvLmmAssocCache(s, xcov, y_rot, log10_lbd)


def fvlmm_assoc_chunk_with_cache_f32(cache, g_rot_chunk, threads=0, nullml=None):
    """src/stats/fvlmm.rs:1920-1939 -> f64 (m, 3 or 4) for already rotated rows."""
    if not isinstance(cache, FvLmmAssocCache):
        raise TypeError("cache must come from fvlmm_assoc_prepare_cache_f32")
    return _fv_chunk(cache.s, cache.xcov, cache.y_rot, cache.log10_lbd, g_rot_chunk, None, nullml, "g_rot_chunk")


def fvlmm_assoc_chunk_from_snp_with_cache_f32(cache, snp_chunk, u_t, threads=0, nullml=None, rotate_block_rows=512):
    """src/stats/fvlmm.rs:1997-2112 -> f64 (m, 3 or 4) for raw SNP rows (rotation + scan)."""
    if not isinstance(cache, FvLmmAssocCache):
        raise TypeError("cache must come from fvlmm_assoc_prepare_cache_f32")
    return _fv_chunk(cache.s, cache.xcov, cache.y_rot, cache.log10_lbd, snp_chunk, u_t, nullml, "snp_chunk")


def fvlmm_assoc_chunk_from_snp_to_tsv_f32(s, xcov, y_rot, log10_lbd, snp_chunk, u_t, chrom, pos, snp, allele0, allele1, maf,
                                          miss, threads=0, nullml=None, rotate_block_rows=512, progress_callback=None,
                                          progress_every=0):
    """src/stats/fvlmm.rs:2266-2480: rotation + fixed-lambda scan of a dense SNP chunk, the result rows already formatted
    -> (list of byte blocks of `rotate_block_rows` TSV rows each, no header; rows).  The streaming `-fvlmm` workflow writes
    the blocks to its result file (python/janusx/assoc/workflow_model_stream.py:1678)."""
    import tempfile
    from .tsv import _native_rows
    n, _p_cov = _fixed_lambda_checks(s, xcov, y_rot, log10_lbd)
    g = _assoc_dense_chunk(snp_chunk, n, "snp_chunk must be (m, n)")
    m = int(g.shape[0])
    if m == 0:
        return [], 0
    if not all(len(a) == m for a in (chrom, pos, snp, allele0, allele1, maf, miss)):
        raise RuntimeError("TSV metadata length mismatch with snp_chunk rows")
    stats = _fv_chunk(s, xcov, y_rot, log10_lbd, g, u_t, nullml, "snp_chunk")
    br = max(int(rotate_block_rows), 1)
    blocks = []
    fd, tmp = tempfile.mkstemp(prefix="jx_fvlmm_chunk_", suffix=".tsv")
    os.close(fd)
    try:
        for r0 in range(0, m, br):
            r1 = min(r0 + br, m)
            open(tmp, "wb").close()
            _native_rows(tmp, chrom[r0:r1], pos[r0:r1], snp[r0:r1], allele0[r0:r1], allele1[r0:r1], maf[r0:r1],
                         miss[r0:r1], stats[r0:r1], True, False, False)
            with open(tmp, "rb") as fh:
                blocks.append(fh.read())
            if progress_callback is not None and progress_every:
                progress_callback(r1, m)
    finally:
        try:
            os.remove(tmp)
        except OSError:
            pass
    if progress_callback is not None:
        progress_callback(m, m)
    return blocks, m


def fvlmm_assoc_packed_f32(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, log10_lbd,
                           sample_indices=None, row_indices=None, threads=0, progress_callback=None,
                           progress_every=0, rotate_block_rows=512, nullml=None):
    """Array-returning core of `fvlmm_assoc_packed_f32_to_tsv` (src/stats/fvlmm.rs:4958-5190) with a
    caller-rotated null model -> f64 (m, 3 or 4)."""
    return _assoc_packed(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, sample_indices, row_indices, "fvlmm",
                         log10_lbd=log10_lbd, nullml=nullml, progress_callback=progress_callback,
                         progress_every=progress_every)


# ------------------------------------------------------------------------------------------------
# joint SNP-pair interaction test at the null lambda  (src/stats/fvlmm2.rs; csrc/k_fvlmm2.hip)
# ------------------------------------------------------------------------------------------------

FVLMM2_MAX_PCOV = 13          # p_cov + 3 <= 16, the largest dense system the scan kernels instantiate


def _fvlmm2_null(s, xcov, y_rot, log10_lbd):
    """The null-model arguments of the joint test with the reference's checks in its order (src/stats/fvlmm2.rs:57-71, 89-100),
    shapes only: host arrays or torch CUDA tensors -> (s, xcov, y, n, p_cov, on_device)."""
    on_dev = any(_is_device_tensor(a) for a in (s, xcov, y_rot))
    if on_dev:
        import torch
        dev = next(a.device for a in (s, xcov, y_rot) if _is_device_tensor(a))

        def f64(a):
            t = a if _is_device_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
            return t.to(device=dev, dtype=torch.float64).contiguous()
        s, xcov, y = f64(s).reshape(-1), f64(xcov), f64(y_rot).reshape(-1)
        ndim = xcov.dim()
    else:
        s, xcov, y = _c(s, np.float64).ravel(), _c(xcov, np.float64), _c(y_rot, np.float64).ravel()
        ndim = xcov.ndim
    n = int(y.shape[0])
    if n == 0:
        raise RuntimeError("y_rot must not be empty")
    if ndim != 2 or int(xcov.shape[0]) != n:
        raise RuntimeError("xcov.n_rows must equal len(y_rot)")
    if int(s.shape[0]) != n:
        raise RuntimeError("len(S) must equal len(y_rot)")
    if not np.isfinite(log10_lbd):
        raise RuntimeError("log10_lbd must be finite")
    return s, xcov, y, n, int(xcov.shape[1]), on_dev


def _fvlmm2_lambda(n, p_cov, log10_lbd):
    with np.errstate(over="ignore", under="ignore"):
        lbd = float(np.float64(10.0) ** np.float64(log10_lbd))
    if not (np.isfinite(lbd) and lbd > 0.0):
        raise RuntimeError("log10_lbd must map to a finite positive lambda")
    if n <= p_cov + 3:
        raise RuntimeError(f"n must be > p_cov + 3 for the joint test, got n={n}, p_cov={p_cov}")
    if p_cov > FVLMM2_MAX_PCOV:
        raise RuntimeError(f"fvlmm2 joint test supports at most {FVLMM2_MAX_PCOV} covariate columns (p_cov + 3 <= 16), got "
                           f"p_cov={p_cov}")
    return lbd


def _fvlmm2_host_values(s, xcov, y, lbd):
    """Value checks of host arrays in the reference's order (src/stats/fvlmm2.rs:119-149); device tensors are checked by
    `jxg_fvlmm2_joint` with the same messages."""
    vv = s + lbd
    if not np.all(np.isfinite(vv) & (vv > 0.0)):
        raise RuntimeError("S + lambda must stay finite and positive for all samples")
    bad_y = ~np.isfinite(y)
    bad_x = ~np.all(np.isfinite(xcov), axis=1) if xcov.shape[1] else np.zeros(len(y), dtype=bool)
    if bad_y.any() or bad_x.any():
        i = int(np.argmax(bad_y | bad_x))                   # the first sample with either: y is looked at before its covariates
        raise RuntimeError("y_rot contains non-finite values" if bad_y[i] else "xcov contains non-finite values")


def _fvlmm2_chunk(a, n, rows, msg):
    """A (rows, n) f32 chunk, host array or torch CUDA tensor, checked against n and (where given) the row count of the first
    chunk -> (chunk, rows)."""
    if not _is_device_tensor(a):
        a = _c(a, np.float32)
    shape = tuple(int(v) for v in a.shape)
    if len(shape) != 2 or shape[1] != n or (rows is not None and shape[0] != rows):
        raise RuntimeError(msg)
    return a, shape[0]


def _fvlmm2_to_device(a, dtype, dev):
    import torch
    if not _is_device_tensor(a):
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    return a.to(device=dev, dtype=dtype).contiguous()


def fvlmm2_assoc_chunk_f32(s, xcov, y_rot, log10_lbd, snp1_chunk, snp2_chunk, combo_chunk, threads=4):
    """src/stats/fvlmm2.rs:37-290 -> f64 (rows, 9) = (beta, se, p) of snp1, snp2 and the combo term in
    y ~ xcov + snp1 + snp2 + combo at lambda = 10^log10_lbd, the rows used AS GIVEN (the reference's script hands unrotated
    rows to this function; `fvlmm2_pairs_packed` rotates them).  Host arrays or torch CUDA tensors; the result is a host array.
    p_cov <= 13 on this build."""
    s, xcov, y, n, p_cov, on_dev = _fvlmm2_null(s, xcov, y_rot, log10_lbd)
    g1, rows = _fvlmm2_chunk(snp1_chunk, n, None, "snp1_chunk.n_cols must equal len(y_rot)")
    g2, _ = _fvlmm2_chunk(snp2_chunk, n, rows, "snp2_chunk must have the same shape as snp1_chunk")
    gc, _ = _fvlmm2_chunk(combo_chunk, n, rows, "combo_chunk must have the same shape as snp1_chunk")
    lbd = _fvlmm2_lambda(n, p_cov, log10_lbd)
    if not on_dev:
        _fvlmm2_host_values(s, xcov, y, lbd)
    import torch
    from .pipeline import _ptr, _stream
    dev = s.device if on_dev else torch.device("cuda", torch.cuda.current_device())
    s, xcov, y = (_fvlmm2_to_device(a, torch.float64, dev) for a in (s, xcov, y))
    g1, g2, gc = (_fvlmm2_to_device(a, torch.float32, dev) for a in (g1, g2, gc))
    out = torch.empty((rows, 9), dtype=torch.float64, device=dev)
    check(lib().jxg_fvlmm2_joint(_ptr(g1), _ptr(g2), _ptr(gc), rows, n, n, _ptr(s), _ptr(xcov), p_cov, _ptr(y), lbd, _ptr(out),
                                 _stream()))
    return out.cpu().numpy()


def fvlmm2_pairs_packed(packed, n_samples, row_flip, row_maf, row1, row2, op, neg1, neg2, s, xcov_rot, y_rot, u_t, log10_lbd,
                        sample_indices=None, batch_size=4096):
    """Joint interaction test of SNP pairs of a packed payload (extension; the device form of `_run_trait_scan`,
    python/janusx/script/fvlmm2.py:696-739, with the rows ROTATED as the model y = X b + g1 + g2 + combo + Zu + e needs).
    row1, row2 (R): payload rows of the pairs; op: R operators of '*', '&', '|', '^' (or one for all); neg1, neg2 (R) bool: negated
    literals; s, xcov_rot, y_rot, u_t: the rotated null model (host arrays or torch CUDA tensors, u_t (n, n) f32 row-major U^T);
    row_flip, row_maf: one entry per payload row.  Per batch of `batch_size` pairs: g1, g2 and the combo row from the P32 image
    (`jxg_fvlmm2_combo_p32`), three rotations (`jxg_rotate_dense_f32`), the joint test (`jxg_fvlmm2_joint`); the buffers are
    allocated once.  -> dict: beta1, se1, p1, beta2, se2, p2, beta_combo, se_combo, p_combo (R) f64 and af1, af2, combo_af
    (R) f64 = share of the samples whose literal 1, literal 2, combo value is > 0."""
    import torch
    from . import fvlmm2 as f2
    from .pipeline import _ptr, _stream
    from .tree import _check_hbm
    s, xcov, y, n, p_cov, on_dev = _fvlmm2_null(s, xcov_rot, y_rot, log10_lbd)
    lbd = _fvlmm2_lambda(n, p_cov, log10_lbd)
    if not on_dev:
        _fvlmm2_host_values(s, xcov, y, lbd)
    r1, r2 = _c(row1, np.int64).ravel(), _c(row2, np.int64).ravel()
    npairs = int(r1.shape[0])
    ops = [str(op)] * npairs if isinstance(op, str) else [str(o) for o in op]
    ng1, ng2 = np.asarray(neg1, dtype=bool).ravel(), np.asarray(neg2, dtype=bool).ravel()
    if not (r2.shape[0] == len(ops) == ng1.shape[0] == ng2.shape[0] == npairs):
        raise RuntimeError("row1, row2, op, neg1 and neg2 must have one entry per pair")
    pk, _pk_ptr, m = _payload(packed, n_samples)
    flip, maf = np.asarray(row_flip).astype(bool).ravel(), _c(row_maf, np.float32).ravel()
    if flip.shape[0] != m or maf.shape[0] != m:
        raise RuntimeError(f"row_flip/row_maf length mismatch: got row_flip={flip.shape[0]}, row_maf={maf.shape[0]}, expected "
                           f"packed_rows={m}")
    if npairs and (min(r1.min(), r2.min()) < 0 or max(r1.max(), r2.max()) >= m):
        raise RuntimeError(f"row1/row2 out of range for {m} rows")
    idx, n_sel = _opt_idx(sample_indices)
    if (n_sel if idx is not None else int(n_samples)) != n:
        raise RuntimeError(f"selected sample count {n_sel if idx is not None else int(n_samples)} != len(y_rot) {n}")
    batch = max(1, int(batch_size))
    if int(batch) * n >= 2 ** 31:
        raise RuntimeError(f"batch_size {batch} x n {n} exceeds 2^31 elements per block; use a smaller batch")
    keys = ("beta1", "se1", "p1", "beta2", "se2", "p2", "beta_combo", "se_combo", "p_combo")
    if npairs == 0:
        return {k: np.zeros(0, dtype=np.float64) for k in keys + ("af1", "af2", "combo_af")}
    lut_all = _raw_additive_lut(maf, flip, True)
    tab, pos = f2.pair_tables(lut_all[r1], lut_all[r2], ops, ng1, ng2)      # refuses '*' with a negation before any device work
    nb = min(batch, npairs)
    _check_hbm(6.0 * nb * n * 4.0 + (0.0 if _is_device_tensor(u_t) else 4.0 * n * n) + 200.0 * nb + 16.0 * n * (p_cov + 2),
               f"fvlmm2 pair scan of {n} samples in batches of {nb}")
    panel = _panel(pk, n_samples, idx)
    dev = panel.device
    s, xcov, y = (_fvlmm2_to_device(a, torch.float64, dev) for a in (s, xcov, y))
    if _is_device_tensor(u_t):
        if tuple(u_t.shape) != (n, n):
            raise RuntimeError("u_t must be (n, n) and row-major U^T")
        ut = u_t.to(device=dev, dtype=torch.float32).contiguous()
    else:
        ut = torch.from_numpy(_assoc_u_t(u_t, n)).to(dev)
    g = torch.empty((3, nb, n), dtype=torch.float32, device=dev)
    grot = torch.empty((3, nb, n), dtype=torch.float32, device=dev)
    d_rows = torch.empty((2, nb), dtype=torch.int32, device=dev)
    d_lut = torch.empty((2, nb, 4), dtype=torch.float32, device=dev)
    d_tab = torch.empty((nb, 16), dtype=torch.float32, device=dev)
    d_pos = torch.empty(nb, dtype=torch.int32, device=dev)
    d_cnt = torch.empty((nb, 3), dtype=torch.int32, device=dev)
    d_out = torch.empty((nb, 9), dtype=torch.float64, device=dev)
    joint = np.empty((npairs, 9), dtype=np.float64)
    cnt = np.empty((npairs, 3), dtype=np.int32)
    for b0 in range(0, npairs, nb):
        nr = min(nb, npairs - b0)
        sl = slice(b0, b0 + nr)
        d_rows[:, :nr].copy_(torch.from_numpy(np.stack([r1[sl], r2[sl]]).astype(np.int32)))
        d_lut[:, :nr].copy_(torch.from_numpy(np.stack([lut_all[r1[sl]], lut_all[r2[sl]]])))
        d_tab[:nr].copy_(torch.from_numpy(tab[sl]))
        d_pos[:nr].copy_(torch.from_numpy(pos[sl].view(np.int32)))
        check(lib().jxg_fvlmm2_combo_p32(_ptr(panel.p32), panel.m, n, _ptr(d_rows[0]), _ptr(d_rows[1]), nr, _ptr(d_lut[0]),
                                         _ptr(d_lut[1]), _ptr(d_tab), _ptr(d_pos), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), n,
                                         _ptr(d_cnt), _stream()))
        for k in range(3):
            check(lib().jxg_rotate_dense_f32(_ptr(g[k]), nr, n, _ptr(ut), _ptr(grot[k]), _stream()))
        check(lib().jxg_fvlmm2_joint(_ptr(grot[0]), _ptr(grot[1]), _ptr(grot[2]), nr, n, n, _ptr(s), _ptr(xcov), p_cov, _ptr(y),
                                     lbd, _ptr(d_out), _stream()))
        joint[sl] = d_out[:nr].cpu().numpy()
        cnt[sl] = d_cnt[:nr].cpu().numpy()
    res = {k: np.ascontiguousarray(joint[:, j]) for j, k in enumerate(keys)}
    for j, k in enumerate(("af1", "af2", "combo_af")):
        res[k] = cnt[:, j].astype(np.float64) / float(n)
    return res


# ------------------------------------------------------------------------------------------------
# exhaustive SNP-pair screen on the int8 pipes  (extension; csrc/k_pairscreen.hip)
# ------------------------------------------------------------------------------------------------

PAIRSCREEN_MAX_N = 1 << 24
PAIRSCREEN_MAX_VARIANTS = 16


def _pairscreen_planes(panel, r):
    """The digit planes of the one column r over the samples of a panel (`pipeline._LmtOperand`, `jxg_lmt_prepare`)
    -> (operand, plane stride in bytes, scale = S 2^-27 as a float)."""
    import torch
    from .pipeline import _LmtOperand
    if panel.n > PAIRSCREEN_MAX_N:
        raise RuntimeError(f"pair screen: at most {PAIRSCREEN_MAX_N} samples, got {panel.n}")
    if _is_device_tensor(r):
        col = r.to(device=panel.device, dtype=torch.float64).reshape(1, -1).contiguous()
        finite = bool(torch.isfinite(col).all())
    else:
        col = _c(r, np.float64).reshape(1, -1)
        finite = bool(np.isfinite(col).all())
    if int(col.shape[1]) != panel.n:
        raise RuntimeError(f"len(r) {int(col.shape[1])} != selected sample count {panel.n}")
    if not finite:
        raise RuntimeError("r contains non-finite values")
    op = _LmtOperand(col, panel.n, panel.npad, panel.device)
    return op, int(op.planes.shape[1]) * int(op.planes.shape[2]), float(op.scale[0].item())


def _pairscreen_rows(rows, m, what):
    rows = _c(rows, np.int64).ravel()
    if rows.size and (rows.min() < 0 or rows.max() >= m):
        raise RuntimeError(f"{what} out of range for {m} rows")
    return rows


def pair_class_tables_packed(packed, n_samples, rows_i, rows_j, r, sample_indices=None):
    """Class tables of the SNP pairs (rows_i[x], rows_j[y]) of a packed payload over the selected samples (extension;
    `jxg_pairscreen_tables_p32`).  Classes of a call: hom-ref 0, het 1, hom-alt 2; a missing call belongs to none, so a pair's
    table runs over the samples called at both SNPs.  r (n) f64: a sample vector, host array or torch CUDA tensor
    -> (N (Ri, Rj, 3, 3) int32 counts, R (Ri, Rj, 3, 3) int64 sums of r in units of `scale`, scale f64 = S 2^-27 with S the
    smallest power of two >= max |r|).  Exact: r enters as its four signed radix-128 digits, what they leave (< S 2^-28 per
    sample) is dropped, and an r of multiples of S 2^-27 is summed exactly."""
    import torch
    from .pipeline import _ptr, _stream
    panel = _panel(packed, n_samples, sample_indices)
    ri, rj = _pairscreen_rows(rows_i, panel.m, "rows_i"), _pairscreen_rows(rows_j, panel.m, "rows_j")
    op, pstride, scale = _pairscreen_planes(panel, r)
    dev = panel.device
    out_n = torch.zeros((ri.size, rj.size, 3, 3), dtype=torch.int32, device=dev)
    out_r = torch.zeros((ri.size, rj.size, 3, 3), dtype=torch.int64, device=dev)
    if ri.size and rj.size:
        ti, tj = (torch.from_numpy(a.astype(np.int32)).to(dev) for a in (ri, rj))
        check(lib().jxg_pairscreen_tables_p32(_ptr(panel.p32), panel.m, panel.n, _ptr(ti), int(ri.size), _ptr(tj), int(rj.size),
                                              _ptr(op.planes), pstride, _ptr(out_n), _ptr(out_r), _stream()))
    return out_n.cpu().numpy(), out_r.cpu().numpy(), scale


def fvlmm2_screen_packed(packed, n_samples, row_flip, r, sigma2, variants, t_min, rows=None, chrom_id=None, pos=None, min_dist=0,
                         cap=1 << 22, sample_indices=None):
    """Exhaustive screen of the unordered SNP pairs of a packed payload (extension; `jxg_pairscreen_scan_p32`): for every pair
    row1 < row2 of `rows` (payload rows; None: all) and every variant the score statistic T of the combo term given the intercept
    and both literals in the linear model of r on the pair's complete samples, error variance `sigma2` (> 0).  variants: at most 16
    `fvlmm2.ScreenVariant` (`fvlmm2.screen_variants`), or their (V, 15) f64 array (`fvlmm2.variant_array`); row_flip: one entry per
    payload row, a flipped row reads its tables at class 2 - a.  A pair / variant with fewer than 5 complete samples, a literal
    that is constant or collinear with the other, or a combo inside the span of the literals is void and never a hit.
    chrom_id / pos (one entry per payload row) with min_dist > 0: a pair on one chromosome closer than min_dist is not screened.
    -> dict: row1, row2, variant, stat, n_complete (the hits with T >= t_min, sorted by stat descending, row1, row2, variant),
    pairs_screened, hits_total.  More than `cap` hits raise a RuntimeError that names the count."""
    import torch
    from .pipeline import _ptr, _stream
    from . import fvlmm2 as f2
    var = f2.variant_array(variants)
    nv = int(var.shape[0])
    if nv < 1 or nv > PAIRSCREEN_MAX_VARIANTS:
        raise RuntimeError(f"pair screen: between 1 and {PAIRSCREEN_MAX_VARIANTS} variants, got {nv}")
    if not np.isfinite(var).all():
        raise RuntimeError("pair screen: variant tables must be finite")
    sigma2, t_min, min_dist, cap = float(sigma2), float(t_min), int(min_dist), int(cap)
    if not (np.isfinite(sigma2) and sigma2 > 0.0):
        raise RuntimeError("sigma2 must be finite and positive")
    if np.isnan(t_min):
        raise RuntimeError("t_min must not be NaN")
    if min_dist < 0 or cap < 0:
        raise RuntimeError("min_dist and cap must be >= 0")
    panel = _panel(packed, n_samples, sample_indices)
    m = panel.m
    flip = np.asarray(row_flip).astype(bool).ravel()
    if flip.shape[0] != m:
        raise RuntimeError(f"row_flip length mismatch: got {flip.shape[0]}, expected packed_rows={m}")
    lst = np.arange(m, dtype=np.int64) if rows is None else np.unique(_pairscreen_rows(rows, m, "rows"))
    if min_dist > 0:
        if chrom_id is None or pos is None:
            raise RuntimeError("min_dist needs chrom_id and pos")
        cid, bp = _c(chrom_id, np.int32).ravel(), _c(pos, np.int64).ravel()
        if cid.shape[0] != m or bp.shape[0] != m:
            raise RuntimeError(f"chrom_id/pos length mismatch: expected packed_rows={m}")
    op, pstride, scale = _pairscreen_planes(panel, r)
    dev = panel.device
    nl = int(lst.size)
    rows_t = None if rows is None else torch.from_numpy(lst.astype(np.int32)).to(dev)
    flip_t = torch.from_numpy(np.ascontiguousarray(flip[lst]).astype(np.uint8)).to(dev)
    cid_t = torch.from_numpy(np.ascontiguousarray(cid[lst])).to(dev) if min_dist > 0 else None
    bp_t = torch.from_numpy(np.ascontiguousarray(bp[lst])).to(dev) if min_dist > 0 else None
    var_t = torch.from_numpy(var).to(dev)
    slots = max(1, min(cap, nl * (nl - 1) // 2 * nv))
    hit_i, hit_j, hit_v, hit_n = (torch.empty(slots, dtype=torch.int32, device=dev) for _ in range(4))
    hit_t = torch.empty(slots, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    check(lib().jxg_pairscreen_scan_p32(_ptr(panel.p32), m, panel.n, _ptr(rows_t), nl, _ptr(flip_t), _ptr(cid_t), _ptr(bp_t), min_dist,
                                        _ptr(op.planes), pstride, scale, sigma2, _ptr(var_t), nv, t_min, cap, _ptr(hit_i),
                                        _ptr(hit_j), _ptr(hit_v), _ptr(hit_n), _ptr(hit_t), _ptr(counts), _stream()))
    hits_total, pairs_screened = (int(v) for v in counts.cpu().numpy())
    if hits_total > cap:
        raise RuntimeError(f"pair screen: {hits_total} hits exceed the capacity of {cap}; raise t_min (a smaller -screen P) or cap")
    k = hits_total
    r1, r2 = lst[hit_i[:k].cpu().numpy()], lst[hit_j[:k].cpu().numpy()]
    hv, hn, ht = hit_v[:k].cpu().numpy(), hit_n[:k].cpu().numpy(), hit_t[:k].cpu().numpy()
    order = np.lexsort((hv, r2, r1, -ht))                     # stat descending, then row1, row2, variant
    return {"row1": r1[order], "row2": r2[order], "variant": hv[order].astype(np.int32), "stat": ht[order],
            "n_complete": hn[order].astype(np.int32), "pairs_screened": pairs_screened, "hits_total": hits_total}


# ------------------------------------------------------------------------------------------------
# BED -> QC -> scan -> TSV entry points (src/stats/lmm.rs:2488-2751, src/stats/fvlmm.rs:2482-2526,
# orchestration of src/stats/lmm.rs:975-1477 `run_unified_bed_scan_to_tsv_common`)
# ------------------------------------------------------------------------------------------------

def bed_row_counts(packed, n_samples, sample_indices=None):
    """(m,3) int32 (missing, het, hom_alt) over the selected samples (src/io/gfreader.rs:1378-1395)."""
    _pk, pk_ptr, m = _payload(packed, n_samples)          # host array or device tensor
    idx, n_sel = _opt_idx(sample_indices)
    out = np.zeros((m, 3), dtype=np.int32)
    check(lib().jx_row_counts(pk_ptr, m, int(n_samples), _p(idx), n_sel, _p(out)))
    return out


def _bed_scan_to_tsv(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr, genetic_model, snps_only,
                     sample_ids, row_indices, row_flip, row_missing, row_maf, mode, nullml, progress_callback,
                     progress_every=0, mmap_window_mb=None, warm_chain=None, **scan):
    # warm_chain: None, or (rotate_block_rows, pieces) -- the exact scan along the reference's warm-start chains
    # scan: the options of `mode` as `_assoc_packed` takes them (low, high, max_iter, tol, init_log10_lbd | log10_lbd)
    import torch
    from . import stats as st
    from .bed import read_fam_ids, snps_only_mask, stage_bed_payload
    from .tsv import write_assoc_tsv
    st.genetic_model_code(genetic_model)             # add / dom / rec / het (src/decode/decode.rs:100-147); anything else raises
    if nullml is not None and not np.isfinite(nullml):
        raise RuntimeError("nullml must be finite when provided")
    s_, xcov_, y_, n, p = _null_args(s, xcov, y_rot)
    if n <= p + 1:
        raise RuntimeError("n must be > p+1")
    # payload staged to HBM in windows of `mmap_window_mb` MiB (the reference's WindowedBedMatrix role); the counts, the row
    # gather and the scan below take the device tensor in place
    packed, n_fam, bim = stage_bed_payload(_bed_prefix(bed_prefix), mmap_window_mb)
    sidx = None if sample_ids is None else _assoc_fam_positions(read_fam_ids(_bed_prefix(bed_prefix)), sample_ids, repr)
    n_sel = n_fam if sidx is None else int(sidx.shape[0])
    if n_sel != n:
        raise RuntimeError(f"selected sample count {n_sel} != len(y_rot) {n}")
    m = int(packed.shape[0])
    if _assoc_prepared_given(row_indices, row_flip, row_missing, row_maf):
        rows = np.asarray(row_indices, dtype=np.int64)
        flip = np.asarray(row_flip).astype(bool)
        af = np.asarray(row_maf, dtype=np.float32)
        miss = np.asarray(row_missing, dtype=np.float32)
    else:
        counts = bed_row_counts(packed, n_fam, sidx)
        keep, af_all, miss_all = st.gwas_scan_row_stats(counts, n, maf_thr, miss_thr, het_thr)
        if snps_only:
            keep &= snps_only_mask(bim)
        rows = np.nonzero(keep)[0]
        flip = np.zeros(len(rows), dtype=bool)
        af = af_all[rows]
        miss = miss_all[rows]
    pk = packed if len(rows) == m and np.array_equal(rows, np.arange(m)) else \
        packed[torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(packed.device)]
    del packed
    chain_off = None
    if warm_chain is not None:
        from .stats import warm_chain_blocks_bed, warm_chain_offsets
        # scan units: the prepared row list, or every SNP row of the file (src/stats/lmm.rs:1103-1106, 1121-1145)
        units = np.arange(len(rows), dtype=np.int64) if row_indices is not None else rows
        n_units = len(rows) if row_indices is not None else m
        chain_off = warm_chain_offsets(warm_chain_blocks_bed(units, n_units, warm_chain[0]), len(rows), warm_chain[1])
    res = _assoc_packed(pk, n_fam, flip, af, s_, xcov_, y_, u_t, sidx, None, mode, nullml=nullml,
                        progress_callback=progress_callback, progress_every=progress_every, genetic_model=genetic_model,
                        chain_off=chain_off, **scan)
    return write_assoc_tsv(out_tsv, *bim.columns(rows), af, miss, res)


def lmm_reml_assoc_bed_to_tsv_f32(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr,
                                  genetic_model="add", snps_only=False, sample_ids=None, row_indices=None,
                                  row_flip=None, row_missing=None, row_maf=None, low=-5.0, high=5.0, max_iter=30,
                                  tol=1e-2, threads=0, nullml=None, init_log10_lbd=None, rotate_block_rows=512,
                                  progress_callback=None, progress_every=0, mmap_window_mb=None, warm_start=None,
                                  warm_chain_pieces=1):
    """src/stats/lmm.rs:2488-2751 (the default `jx gwas -lmm` kernel call) -> rows written.
    Warm start: as the reference, the chain is ON unless JX_LMM_UNIFIED_NO_WARM_START is truthy (:2627) or
    warm_start="none"; a chain is the kept rows of one chunk of `rotate_block_rows` scan units (:1121-1145), see
    `lmm_reml_assoc_packed_f32` for the semantics and `warm_chain_pieces`."""
    _assoc_check_bounds(low, high)
    _assoc_check_tol(tol)
    chain = _resolve_warm_start(warm_start, "JX_LMM_UNIFIED_NO_WARM_START") == "chain"
    return _bed_scan_to_tsv(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr, genetic_model,
                            snps_only, sample_ids, row_indices, row_flip, row_missing, row_maf, "lmm", nullml,
                            progress_callback, progress_every, mmap_window_mb,
                            warm_chain=(int(rotate_block_rows), int(warm_chain_pieces)) if chain else None,
                            low=low, high=high, max_iter=max_iter, tol=tol, init_log10_lbd=init_log10_lbd)


def lmm_reml_lmm2_chunk_from_snp_f32(s, xcov, y_rot, low, high, snp_chunk, u_t, nullml, max_iter=50, tol=1e-2,
                                     threads=0, rotate_block_rows=256):
    """src/stats/lmm.rs:1632-1760 -> f64 (m, 6) = [beta, se, pwald, lambda_reml, ml_alt, plrt] (LMM2: REML Wald test
    plus an ML likelihood-ratio test from a second Brent on `ml_loglike`, lmm.rs:202-330); no warm start."""
    s, xcov, y, n, p = _null_args(s, xcov, y_rot)
    g = _assoc_dense_chunk(snp_chunk, n, "snp_chunk must be (m_chunk, n)")
    u_t = _assoc_u_t(u_t, n)                      # required here: LMM2 has no form for rows rotated already
    _assoc_check_bounds(low, high)
    if not np.isfinite(nullml):
        raise RuntimeError("nullml must be finite")
    return _scan_dense_chunk(g, s, xcov, y, u_t, "lmm2", 6, low=low, high=high, max_iter=max_iter, tol=tol, nullml=nullml)


def lmm_reml_lmm2_assoc_bed_to_tsv_f32(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr,
                                       genetic_model="add", snps_only=False, sample_ids=None, row_indices=None,
                                       row_flip=None, row_missing=None, row_maf=None, low=-5.0, high=5.0,
                                       max_iter=30, tol=1e-2, threads=0, nullml=None, init_log10_lbd_reml=None,
                                       init_log10_lbd_ml=None, rotate_block_rows=512, progress_callback=None,
                                       progress_every=0, mmap_window_mb=None):
    """src/stats/lmm.rs:2779-3037 (`jx gwas -lmm2`) -> rows written; TSV schema Lmm2_6
    (`... pwald lambda ml plrt`, src/io/assoc2tsv.rs:54-56).  Without `nullml` the null ML is fitted first by Brent
    on -ml_loglike seeded with init_log10_lbd_ml or init_log10_lbd_reml (lmm.rs:2902-2921).  Deterministic start per
    SNP: init_log10_lbd_reml, else init_log10_lbd_ml, else the interval midpoint (see `lmm_reml_assoc_packed_f32`)."""
    _assoc_check_bounds(low, high)
    _assoc_check_tol(tol)
    if nullml is not None:
        if not np.isfinite(nullml):
            raise RuntimeError("nullml must be finite when provided")
        nullml_val = float(nullml)
    else:
        s_, xcov_, y_, _n, _p_cov = _null_args(s, xcov, y_rot)
        init = init_log10_lbd_ml if init_log10_lbd_ml is not None else init_log10_lbd_reml
        nullml_val = _dense_model(s_, xcov_, y_).null_ml(max_iter, tol, (low, high), init)[1]
    init_scan = init_log10_lbd_reml if init_log10_lbd_reml is not None else init_log10_lbd_ml
    return _bed_scan_to_tsv(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr, genetic_model,
                            snps_only, sample_ids, row_indices, row_flip, row_missing, row_maf, "lmm2", nullml_val,
                            progress_callback, progress_every, mmap_window_mb, low=low, high=high, max_iter=max_iter, tol=tol,
                            init_log10_lbd=init_scan)


def fvlmm_assoc_bed_to_tsv_f32(bed_prefix, out_tsv, s, xcov, y_rot, log10_lbd, u_t, maf_thr, miss_thr, het_thr,
                               genetic_model="add", snps_only=False, sample_ids=None, row_indices=None,
                               row_flip=None, row_missing=None, row_maf=None, threads=0, nullml=None,
                               rotate_block_rows=512, progress_callback=None, progress_every=0, mmap_window_mb=None):
    """src/stats/fvlmm.rs:2482-2526 (the default `jx gwas -fvlmm` kernel call) -> (rows, pve, log_det_v)."""
    rows = _bed_scan_to_tsv(bed_prefix, out_tsv, s, xcov, y_rot, u_t, maf_thr, miss_thr, het_thr, genetic_model,
                            snps_only, sample_ids, row_indices, row_flip, row_missing, row_maf, "fvlmm", nullml,
                            progress_callback, progress_every, mmap_window_mb, log10_lbd=float(log10_lbd))
    s_ = np.asarray(s, dtype=np.float64).ravel()
    lbd = 10.0 ** float(log10_lbd)
    vg = float(np.mean(np.clip(s_, 0.0, None)))
    pve = vg / (vg + lbd) if (vg + lbd) > 0 else float("nan")
    return rows, pve, float(np.sum(np.log(s_ + lbd)))


def lmm_reml_assoc_packed_f32_to_tsv(packed, n_samples, row_flip, row_maf, row_missing, s, xcov, y_rot, u_t,
                                     chrom, pos, snp, allele0, allele1, out_tsv, sample_indices=None,
                                     row_indices=None, low=-5.0, high=5.0, max_iter=50, tol=1e-2, threads=0,
                                     model="add", progress_callback=None, progress_every=0, nullml=None,
                                     init_log10_lbd=None, rotate_block_rows=256, bed_prefix=None, warm_start=None,
                                     warm_chain_pieces=1):
    """src/stats/lmm.rs:3364-3790 -> rows written (metadata lists empty => read the BIM via `bed_prefix`); the scan with the
    warm-start chain of `lmm_reml_assoc_packed_f32` (the reference passes `true, true` here as well, lmm.rs:3609-3610)."""
    from .tsv import write_assoc_tsv
    out = lmm_reml_assoc_packed_f32(packed, n_samples, row_flip, row_maf, s, xcov, y_rot, u_t, sample_indices,
                                    row_indices, low, high, max_iter, tol, threads, model, progress_callback,
                                    progress_every, nullml, init_log10_lbd, rotate_block_rows, warm_start, warm_chain_pieces)
    if not len(chrom):
        chrom, pos, snp, allele0, allele1 = _packed_tsv_bim_columns(bed_prefix, row_indices, out.shape[0])
    return write_assoc_tsv(out_tsv, chrom, pos, snp, allele0, allele1, np.asarray(row_maf, dtype=np.float32),
                           np.asarray(row_missing, dtype=np.float32), out, resolve=False)


def fvlmm_assoc_packed_f32_to_tsv(packed, n_samples, row_flip, row_maf, row_missing, u, s, y, x, sample_indices,
                                  low, high, max_iter, tol, tau, threads, model, chrom, pos, snp, allele0, allele1,
                                  out_tsv, progress_callback=None, progress_every=0, fixed_lbd=None, fixed_ml0=None,
                                  row_indices=None, rotate_block_rows=0, bed_prefix=None):
    """src/stats/fvlmm.rs:4958-5190 -> (lbd, ml0, reml0); writes the TSV.

    `u` (n_samples, k) f32 holds eigenvectors as columns, `s` (k) f32 their eigenvalues (caller order, the packed
    workflow passes them descending); the function adds the intercept to `x`, rotates X and y itself with the
    sample-subset of U^T (f32 widened, f64 accumulation), fits lambda by Brent on REML unless `fixed_lbd` is given,
    and scans every row at that lambda.  `fixed_ml0` switches the plrt column on."""
    import math
    from .tsv import write_assoc_tsv
    if fixed_lbd is None:
        _assoc_check_bounds(low, high)
    _assoc_check_tol(tol)
    if not (np.isfinite(tau) and tau >= 0):
        raise RuntimeError("tau must be finite and >= 0")
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    from .stats import genetic_model_code
    genetic_model_code(model)                        # add / dom / rec / het (src/decode/decode.rs:100-147); anything else raises
    packed, _pk_ptr, m_all = _payload(packed, n_samples)
    m = m_all if row_indices is None else int(len(row_indices))
    for name, arr in (("row_flip", row_flip), ("row_maf", row_maf), ("row_missing", row_missing)):
        if len(arr) != m:
            raise RuntimeError(f"{name} length mismatch: got {len(arr)}, expected {m}")
    yv = _c(y, np.float64).ravel()
    n = int(yv.shape[0])
    if n == 0:
        raise RuntimeError("y must not be empty")
    if sample_indices is not None:
        sidx = np.asarray(sample_indices, dtype=np.int64).ravel()
        if sidx.shape[0] != n:
            raise RuntimeError(f"sample_indices length mismatch: got {sidx.shape[0]}, expected {n}")
        if sidx.size and (sidx.min() < 0 or sidx.max() >= int(n_samples)):
            raise RuntimeError("sample_indices out of range")
    else:
        if n != int(n_samples):
            raise RuntimeError(f"len(y)={n} must equal n_samples={int(n_samples)} when sample_indices is not provided")
        sidx = np.arange(n, dtype=np.int64)
    u = _c(u, np.float32)
    if u.ndim != 2:
        raise RuntimeError("u must be 2D (n_samples, k)")
    if u.shape[0] != int(n_samples):
        raise RuntimeError(f"u row count mismatch: got {u.shape[0]}, expected {int(n_samples)}")
    k_full = int(u.shape[1])
    s32 = _c(s, np.float32).ravel()
    if s32.shape[0] != k_full:
        raise RuntimeError(f"s length mismatch: got {s32.shape[0]}, expected {k_full}")
    if k_full < n:
        raise RuntimeError("u must provide full-rank eigenvectors for packed fixed-lambda scan: "
                           f"got k={k_full}, expected >= n={n}")
    s_vec = s32[:n].astype(np.float64) + (float(tau) if tau != 0.0 else 0.0)
    if not np.all(np.isfinite(s_vec)):
        raise RuntimeError("invalid s/tau produced non-finite values")
    if x is not None:
        xa = _c(x, np.float64)
        if xa.ndim != 2:
            raise RuntimeError("x must be 2D (n, p0)")
        if xa.shape[0] != n:
            raise RuntimeError(f"x row count mismatch: got {xa.shape[0]}, expected {n}")
        x_full = np.concatenate([np.ones((n, 1)), xa], axis=1)
    else:
        x_full = np.ones((n, 1), dtype=np.float64)
    p = int(x_full.shape[1])
    if n <= p:
        raise RuntimeError(f"n must be > p for null model: n={n}, p={p}")
    if n <= p + 1:
        raise RuntimeError(f"n must be > p+1 for SNP tests: n={n}, p={p}")
    # u_t_sub[c, j] = u[sample_idx[j], c], c < n (fvlmm.rs:1458-1482)
    u_t = np.ascontiguousarray(u[sidx, :n].T)
    x_rot, y_rot = lmm_rotate_x_y_with_ut_f64(u_t, x_full, yv)
    y_rot = y_rot.ravel()
    with_plrt = fixed_ml0 is not None
    if with_plrt and not np.isfinite(fixed_ml0):
        raise RuntimeError("fixed_ml0 must be finite when provided")
    if fixed_lbd is not None:
        if not (np.isfinite(fixed_lbd) and fixed_lbd > 0):
            raise RuntimeError("fixed_lbd must be finite and > 0 when provided")
        lbd = float(fixed_lbd)
        ml0 = float(fixed_ml0) if with_plrt else math.nan
        reml0 = _loglike_null(s_vec, x_rot, y_rot, math.log10(lbd))[1] if with_plrt else math.nan
    else:
        lbd, _, reml0 = lmm_reml_null_f32(s_vec, x_rot, y_rot, low, high, max_iter, tol)
        ml0 = float(fixed_ml0) if with_plrt else math.nan
    if not (np.isfinite(lbd) and lbd > 0):
        raise RuntimeError("invalid fixed lambda in packed fvlmm")
    out = _assoc_packed(packed, n_samples, row_flip, row_maf, s_vec, x_rot, y_rot, u_t,
                        None if sample_indices is None else sidx, row_indices, "fvlmm", log10_lbd=math.log10(lbd),
                        nullml=float(fixed_ml0) if with_plrt else None, progress_callback=progress_callback,
                        progress_every=progress_every, genetic_model=model)
    if not len(chrom):
        chrom, pos, snp, allele0, allele1 = _packed_tsv_bim_columns(bed_prefix, row_indices, m)
    write_assoc_tsv(out_tsv, chrom, pos, snp, allele0, allele1, np.asarray(row_maf, dtype=np.float32),
                    np.asarray(row_missing, dtype=np.float32), out, resolve=False)
    return float(lbd), float(ml0), float(reml0)


# ------------------------------------------------------------------------------------------------
# LMM -> LM fallback decision (src/stats/gwas_unified.rs:54-175); O(n p^2) host arithmetic, as in the reference
# ------------------------------------------------------------------------------------------------

def gwas_lmm_lm_null_lrt_decision(y, x_cov, lmm_ml0, alpha=0.05, boundary_mixture=True):
    """-> (switch_to_lm, lrt_stat, pval, lm_ml0). `x_cov` excludes the intercept (it is prepended here)."""
    import math
    if not math.isfinite(lmm_ml0):
        raise RuntimeError("lmm_ml0 must be finite")
    if not (math.isfinite(alpha) and 0.0 < alpha < 1.0):
        raise RuntimeError("alpha must be in (0,1)")
    y = _c(y, np.float64).ravel()
    x = _c(x_cov, np.float64)
    if x.ndim != 2:
        raise RuntimeError("x_cov must be 2D")
    n, p_cov = y.shape[0], x.shape[1]
    if x.shape[0] != n:
        raise RuntimeError("x_cov rows must equal len(y)")
    if n <= p_cov + 1:
        raise RuntimeError("insufficient samples: require n > p_cov + 1")
    xd = np.concatenate([np.ones((n, 1)), x], axis=1)
    xtx = xd.T @ xd
    xty = xd.T @ y
    try:
        chol = np.linalg.cholesky(xtx)
    except np.linalg.LinAlgError:
        try:
            chol = np.linalg.cholesky(xtx + 1e-8 * np.eye(p_cov + 1))
        except np.linalg.LinAlgError:
            raise RuntimeError("failed to compute LM null log-likelihood") from None
    beta = np.linalg.solve(chol.T, np.linalg.solve(chol, xty))
    r = y - xd @ beta
    rss = float(np.dot(r, r))
    if not (math.isfinite(rss) and rss > 0.0):
        raise RuntimeError("failed to compute LM null log-likelihood")
    n_f = float(n)
    lm_ml0 = n_f * (math.log(n_f) - 1.0 - math.log(2.0 * math.pi)) / 2.0 - 0.5 * n_f * math.log(rss)
    stat = 2.0 * (float(lmm_ml0) - lm_ml0)
    if not math.isfinite(stat) or stat < 0.0:
        stat = 0.0
    pval = 1.0 if stat <= 0.0 else math.erfc(math.sqrt(0.5 * stat))
    pval = min(max(pval, 2.2250738585072014e-308), 1.0) if math.isfinite(pval) else 1.0
    if boundary_mixture:
        pval *= 0.5
    if not math.isfinite(pval):
        pval = 1.0
    pval = min(max(pval, 2.2250738585072014e-308), 1.0)
    return bool(pval >= alpha), stat, pval, lm_ml0


def lm_precompute_ixx_qr(x):
    """`_lm_precompute_ixx_qr` (python/janusx/pyBLUP/assoc.py:453-480): (X'X)^-1 of the LM design through the reduced QR,
    the Hermitian pseudo-inverse when X is rank deficient."""
    x = _c(x, np.float64)
    if x.ndim != 2:
        raise ValueError("X must be 2D for LM QR precomputation.")
    n, q = x.shape
    if n == 0 or q == 0:
        raise ValueError("X must be non-empty for LM QR precomputation.")
    _q, r = np.linalg.qr(x, mode="reduced")
    diag = np.abs(np.diag(r))
    tol = np.finfo(np.float64).eps * float(max(n, q)) * (float(diag.max()) if diag.size else 0.0)
    if int(np.sum(diag > tol)) == q:
        rinv = np.linalg.inv(r)
        return np.ascontiguousarray(rinv @ rinv.T)
    return np.ascontiguousarray(np.linalg.pinv(x.T @ x, hermitian=True))


def lm_block_assoc_packed(y, x, ixx, packed, n_samples, row_flip, row_maf, sample_indices=None, chunk_size=10000,
                          threads=0, progress_callback=None, progress_every=0):
    """src/stats/glm.rs:3550-3860 -> f64 (m, 4) = beta, se, pwald (two-sided Student t, df = n - q0 - 1), plrt.  `x` (n, q0)
    carries the intercept column (the `LM` wrapper prepends it, python/janusx/pyBLUP/assoc.py:2192-2199); `chunk_size` and
    `threads` are accepted for signature parity (the whole payload is scanned from HBM)."""
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if int(chunk_size) <= 0:
        raise RuntimeError("chunk_size must be > 0")
    y = _c(y, np.float64).ravel()
    x = _c(x, np.float64)
    ixx = _c(ixx, np.float64)
    packed, _pk_ptr, m = _payload(packed, n_samples)
    flip = _c(np.asarray(row_flip).astype(np.uint8), np.uint8).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if flip.shape[0] != m:
        raise RuntimeError(f"row_flip length mismatch: got {flip.shape[0]}, expected {m}")
    if maf.shape[0] != m:
        raise RuntimeError(f"row_maf length mismatch: got {maf.shape[0]}, expected {m}")
    idx, n_sel = _opt_idx(sample_indices)
    n = y.shape[0]
    if (n_sel if idx is not None else int(n_samples)) != n:
        raise RuntimeError(f"sample_indices length mismatch: got {n_sel if idx is not None else int(n_samples)}, "
                           f"expected len(y)={n}")
    if x.ndim != 2 or x.shape[0] != n:
        raise RuntimeError("X.n_rows must equal len(y)")
    q0 = int(x.shape[1])
    if ixx.shape != (q0, q0):
        raise RuntimeError("ixx must be (q0,q0)")
    if n <= q0 + 1:
        raise RuntimeError(f"n too small: require n > q0+1, got n={n}, q0={q0}")
    if m == 0:
        return np.zeros((0, 4), dtype=np.float64)
    from . import pipeline as pl
    out = pl.scan_rows_lm(_panel(packed, n_samples, idx), np.arange(m), maf, x, y, flip=flip, ixx=ixx,
                          progress=progress_callback, progress_every=progress_every)
    return out.cpu().numpy()


def _resolve_assoc_tsv_metadata(bed_prefix, chrom, pos, snp, allele0, allele1, row_indices, expected_len,
                                empty_msg="empty TSV metadata requires non-empty bed_prefix"):
    """`resolve_assoc_tsv_metadata` (src/io/assoc2tsv.rs:139-195): all five lists empty -> the BIM columns of `bed_prefix`
    (rows `row_indices` when given; `empty_msg` when there is no prefix); otherwise every list must have `expected_len`
    entries."""
    if not any(len(a) for a in (chrom, pos, snp, allele0, allele1)):
        prefix = str(bed_prefix or "").strip()
        if not prefix:
            raise RuntimeError(empty_msg)
        from .bed import read_bim
        bim = read_bim(_bed_prefix(prefix))
        chrom, pos, snp, allele0, allele1 = bim.columns(range(len(bim.chrom)) if row_indices is None else
                                                        [int(j) for j in row_indices])
        if len(chrom) != expected_len:
            raise RuntimeError(f"BIM metadata length mismatch: expected={expected_len}, chrom={len(chrom)}, pos={len(pos)}, "
                               f"snp={len(snp)}, allele0={len(allele0)}, allele1={len(allele1)}")
        return chrom, pos, snp, allele0, allele1
    if not all(len(a) == expected_len for a in (chrom, pos, snp, allele0, allele1)):
        raise RuntimeError(f"TSV metadata length mismatch: rows={expected_len}, chrom={len(chrom)}, pos={len(pos)}, "
                           f"snp={len(snp)}, allele0={len(allele0)}, allele1={len(allele1)}")
    return chrom, pos, snp, allele0, allele1


def _packed_tsv_bim_columns(bed_prefix, row_indices, m):
    """The empty metadata lists of the packed LMM / fvLMM `_to_tsv` routes: the BIM rows `row_indices`, else the first m."""
    sel = np.arange(m) if row_indices is None else np.asarray(row_indices, dtype=np.int64)
    return _resolve_assoc_tsv_metadata(bed_prefix, [], [], [], [], [], sel, m,
                                       "metadata lists are empty and bed_prefix is not set")


def lm_block_assoc_f32(y, x, ixx, g, chunk_size=10000, threads=0):
    """src/stats/glm.rs:4313-4497: the LM formulas of `lm_block_assoc_packed` on an already decoded SNP-major f32 block
    `g` (m, n) (the `LM.gwas` wrapper of python/janusx/pyBLUP/assoc.py:613) -> f64 (m, 4) = beta, se, pwald, plrt."""
    if int(chunk_size) <= 0:
        raise RuntimeError("chunk_size must be > 0")
    y = _c(y, np.float64).ravel()
    x = _c(x, np.float64)
    ixx = _c(ixx, np.float64)
    n = int(y.shape[0])
    if x.ndim != 2 or x.shape[0] != n:
        raise RuntimeError("X.n_rows must equal len(y)")
    q0 = int(x.shape[1])
    if ixx.shape != (q0, q0):
        raise RuntimeError("ixx must be (q0,q0)")
    g = _assoc_dense_chunk(g, n, "g must be shape (m, n)")
    if n <= q0 + 1:
        raise RuntimeError(f"n too small: require n > q0+1, got n={n}, q0={q0}")
    if g.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.float64)
    from . import pipeline as pl
    return pl.scan_rows_lm_dense(g, x, y, ixx).cpu().numpy()


def lm_block_assoc_packed_to_tsv(y, x, ixx, packed, n_samples, row_flip, row_maf, row_missing, chrom, pos, snp, allele0,
                                 allele1, out_tsv, maf_threshold=0.0, max_missing_rate=1.0, het_threshold=0.0,
                                 sample_indices=None, row_indices=None, chunk_size=10000, threads=0,
                                 progress_callback=None, progress_every=0, bed_prefix=None):
    """src/stats/glm.rs:3862-4305: `lm_block_assoc_packed` with the result table written (11 columns, `miss` as the count
    `(row_missing * n_samples) as i64` in f32 arithmetic, pwald sanitised; the thresholds are only range-checked, the rows
    arrive filtered) -> (rows written, rows scanned).  Empty metadata lists are read from `<bed_prefix>.bim`."""
    from .tsv import write_assoc_tsv_counts
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if int(chunk_size) <= 0:
        raise RuntimeError("chunk_size must be > 0")
    _assoc_check_qc(maf_threshold, max_missing_rate, het_threshold)
    packed = _c(packed, np.uint8)
    if packed.ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    if row_indices is not None:
        ri = _c(row_indices, np.int64).ravel()
        if ri.size and (ri.min() < 0 or ri.max() >= packed.shape[0]):
            raise RuntimeError("row_indices out of range")
        packed = np.ascontiguousarray(packed[ri])
    else:
        ri = None
    m = int(packed.shape[0])
    miss = _c(row_missing, np.float32).ravel()
    if np.asarray(row_flip).ravel().shape[0] != m:
        raise RuntimeError("row_flip length mismatch")
    if _c(row_maf, np.float32).ravel().shape[0] != m:
        raise RuntimeError("row_maf length mismatch")
    if miss.shape[0] != m:
        raise RuntimeError("row_missing length mismatch")
    chrom, pos, snp, allele0, allele1 = _resolve_assoc_tsv_metadata(bed_prefix, chrom, pos, snp, allele0, allele1, ri, m)
    stats = lm_block_assoc_packed(y, x, ixx, packed, n_samples, row_flip, row_maf, sample_indices, chunk_size, threads,
                                  progress_callback, progress_every)
    counts = (miss * np.float32(int(n_samples))).astype(np.int64).astype(np.float32)
    rows = write_assoc_tsv_counts(out_tsv, chrom, pos, snp, allele0, allele1, _c(row_maf, np.float32).ravel(), counts,
                                  stats[:, :3], resolve=False)
    if progress_callback is not None:
        progress_callback(m, m)
    return rows, m


def _lm_stream_checks(y, x, maf_threshold, max_missing_rate, genetic_model, het_threshold, chunk_size, mmap_window_mb):
    """Leading argument checks shared by `lm_stream_bed_to_tsv` (src/stats/glm.rs:2385-2421) and `lm2_stream_bed_to_tsv`
    (src/stats/glm2.rs:412-440), in the reference's order, before any device call.  -> (y, x)."""
    if int(chunk_size) <= 0:
        raise ValueError("chunk_size must be > 0")
    _assoc_check_qc(maf_threshold, max_missing_rate, het_threshold)
    model = str(genetic_model).strip().lower()
    if model not in ("add", "dom", "rec", "het"):
        raise ValueError("genetic_model must be one of: add, dom, rec, het")
    if model != "add":
        raise RuntimeError(f"genetic_model '{model}' is outside this build's scope (additive model only)")
    if mmap_window_mb is not None and int(mmap_window_mb) <= 0:
        raise ValueError("mmap_window_mb must be > 0")
    y = _c(y, np.float64).ravel()
    x = _c(x, np.float64)
    if x.ndim != 2 or x.shape[0] != y.shape[0]:
        raise RuntimeError("X.n_rows must equal len(y)")
    return y, x


def _lm_prepared_meta(row_indices, row_flip, row_missing, row_maf):
    """The prepared row metadata of the LM streaming routes (glm2.rs:487-510, 539-567): all four arrays or none, equal
    lengths, `row_indices` ascending.  -> (row_indices i64, row_flip bool, row_missing f32, row_maf f32) or None."""
    if not _assoc_prepared_given(row_indices, row_flip, row_missing, row_maf):
        return None
    ri = _c(row_indices, np.int64).ravel()
    fl = np.asarray(row_flip).astype(bool).ravel()
    mi = _c(row_missing, np.float32).ravel()
    mf = _c(row_maf, np.float32).ravel()
    if not (fl.shape[0] == mi.shape[0] == mf.shape[0] == ri.shape[0]):
        raise RuntimeError(f"prepared row metadata length mismatch: row_indices={ri.shape[0]}, row_flip={fl.shape[0]}, "
                           f"row_missing={mi.shape[0]}, row_maf={mf.shape[0]}")
    if ri.size > 1 and np.any(np.diff(ri) < 0):
        raise RuntimeError("prepared row_indices must be sorted in ascending BED order")
    return ri, fl, mi, mf


def _lm_stream_rows(prefix, n, sample_ids, meta, maf_threshold, max_missing_rate, snps_only, mmap_window_mb, packed,
                    packed_n_samples):
    """Payload, sample selection and kept rows of the two LM streaming routes: the panel over the selected samples, the
    kept rows in BED order with their flip, allele frequency (f32) and missing count, the BIM columns and the number of rows
    scanned.  Without prepared metadata the rows pass `lm2.row_filter` (src/stats/glm2.rs:634-717: no flip, no het filter);
    prepared rows arrive filtered, their missing count is round(row_missing) (glm2.rs:568-577)."""
    from . import bed as _bed
    from . import lm2
    bed_prefix = _bed_prefix(prefix)
    fam = _bed.read_fam_ids(bed_prefix)
    idx = None if sample_ids is None else _assoc_fam_positions(fam, sample_ids, str)
    n_sel = len(fam) if idx is None else int(idx.shape[0])
    if n_sel != n:
        raise RuntimeError(f"sample_ids length mismatch: selected n={n_sel} but len(y)={n}")
    if packed is not None or int(packed_n_samples) > 0:
        if packed is None or int(packed_n_samples) <= 0:
            raise RuntimeError("the staged payload needs both `packed` and `packed_n_samples` > 0")
        if int(packed_n_samples) != len(fam):
            raise RuntimeError(f"packed_n_samples {int(packed_n_samples)} != {len(fam)} samples of {bed_prefix}.fam")
        pk = packed
        bim = _bed.read_bim(bed_prefix)
    else:
        pk, _n_full, bim = _bed.stage_bed_payload(bed_prefix, mmap_window_mb)
    panel = _panel(pk, len(fam), idx)
    if panel.m != len(bim.snp):
        raise RuntimeError(f"payload has {panel.m} SNP rows, {bed_prefix}.bim lists {len(bim.snp)}")
    if meta is None:
        keep, af, miss = lm2.row_filter(panel.counts(), n, maf_threshold, max_missing_rate)
        rows = np.nonzero(keep)[0].astype(np.int64)
        flip, af, miss, total = np.zeros(len(rows), dtype=bool), af[rows], miss[rows].astype(np.int64), panel.m
    else:
        rows, flip, mi, af = meta
        if rows.size and (rows.min() < 0 or rows.max() >= panel.m):
            raise RuntimeError(f"row_indices out of range for n_snps={panel.m}")
        with np.errstate(invalid="ignore"):
            miss = np.where(np.isfinite(mi) & (mi >= 0), np.floor(np.abs(mi.astype(np.float64)) + 0.5), 0).astype(np.int64)
        total = int(rows.shape[0])
    if snps_only:
        ok = _bed.snps_only_mask(bim)[rows]
        rows, flip, af, miss = rows[ok], flip[ok], af[ok], miss[ok]
    return panel, rows, flip, af, miss, bim.columns(rows), total


def lm_stream_bed_to_tsv(prefix, y, x, ixx, out_tsv, sample_ids=None, row_indices=None, row_flip=None, row_missing=None,
                         row_maf=None, maf_threshold=0.0, max_missing_rate=1.0, genetic_model="add", het_threshold=0.02,
                         snps_only=False, chunk_size=10000, threads=0, progress_callback=None, progress_every=0,
                         mmap_window_mb=None, packed=None, packed_n_samples=0):
    """src/stats/glm.rs:2339 ff.: the plain LM scan of a PLINK prefix with its own row filter, written as the 11-column LM
    table (`miss` = the count of missing samples) -> (rows written, rows scanned).  `x` (n, q0) carries the intercept; `ixx` =
    (X'X)^-1 or None.  The arithmetic is that of `lm_block_assoc_packed` (`pipeline.scan_rows_lm`).  `packed` /
    `packed_n_samples`: an already staged payload of the prefix (host array or device tensor) instead of reading the .bed."""
    from . import pipeline as pl
    from .tsv import write_assoc_tsv_counts
    y, x = _lm_stream_checks(y, x, maf_threshold, max_missing_rate, genetic_model, het_threshold, chunk_size, mmap_window_mb)
    n, q0 = int(y.shape[0]), int(x.shape[1])
    if n <= q0 + 1:
        raise RuntimeError(f"n too small: require n > q0+1, got n={n}, q0={q0}")
    if ixx is not None:
        ixx = _c(ixx, np.float64)
        if ixx.shape != (q0, q0):
            raise RuntimeError("ixx must be (q0,q0)")
    meta = _lm_prepared_meta(row_indices, row_flip, row_missing, row_maf)
    panel, rows, flip, af, miss, cols, total = _lm_stream_rows(prefix, n, sample_ids, meta, maf_threshold, max_missing_rate,
                                                               snps_only, mmap_window_mb, packed, packed_n_samples)
    out = pl.scan_rows_lm(panel, rows, af, x, y, flip=flip, ixx=ixx, progress=progress_callback,
                          progress_every=progress_every)
    written = write_assoc_tsv_counts(out_tsv, *cols, af, miss.astype(np.float32), out[:, :3].cpu().numpy())
    _done(progress_callback, total)
    return written, total


def lm2_stream_bed_to_tsv(prefix, y, x, cov_all, cov_indices, out_tsv, sample_ids=None, row_indices=None, row_flip=None,
                          row_missing=None, row_maf=None, maf_threshold=0.0, max_missing_rate=1.0, genetic_model="add",
                          het_threshold=0.02, snps_only=False, chunk_size=10000, threads=0, progress_callback=None,
                          progress_every=0, mmap_window_mb=None, packed=None, packed_n_samples=0):
    """src/stats/glm2.rs:364-885: the SNP-by-covariate interaction scan y ~ X + g + g o c_1 + ... + g o c_k of a PLINK prefix,
    c = the columns `cov_indices` of `cov_all` (n, n_cov), written as the LM2 table (`tsv.write_lm2_tsv`) -> (rows written,
    rows scanned).  `x` (n, q_base) carries the intercept.  At most 8 interaction columns in this build.  `packed` /
    `packed_n_samples`: an already staged payload of the prefix (host array or device tensor) instead of reading the .bed."""
    from . import pipeline as pl
    from .lm2 import LM2_MAX_INTERACTIONS
    from .tsv import write_lm2_tsv
    y, x = _lm_stream_checks(y, x, maf_threshold, max_missing_rate, genetic_model, het_threshold, chunk_size, mmap_window_mb)
    n, q_base = int(y.shape[0]), int(x.shape[1])
    cov = _c(cov_all, np.float64)
    if cov.ndim != 2 or cov.shape[0] != n:
        raise RuntimeError("cov_all.n_rows must equal len(y)")
    n_cov = int(cov.shape[1])
    if n_cov == 0:
        raise RuntimeError("LM2 requires cov_all with at least one column")
    pick = []
    for v in _c(cov_indices, np.int64).ravel():
        if v < 0:
            raise RuntimeError("cov_indices must be >= 0")
        if v >= n_cov:
            raise RuntimeError(f"cov_indices out of range: {int(v)} >= {n_cov}")
        pick.append(int(v))
    if not pick:
        raise RuntimeError("LM2 requires at least one explicitly selected covariate column.")
    k = len(pick)
    if n <= q_base + 1 + k:
        raise RuntimeError(f"n too small: require n > q_base + 1 + n_interactions, got n={n}, q_base={q_base}, "
                           f"n_interactions={k}")
    if k > LM2_MAX_INTERACTIONS:
        raise RuntimeError(f"LM2 supports at most {LM2_MAX_INTERACTIONS} interaction covariates in this build, got {k}")
    meta = _lm_prepared_meta(row_indices, row_flip, row_missing, row_maf)
    panel, rows, flip, af, miss, cols, total = _lm_stream_rows(prefix, n, sample_ids, meta, maf_threshold, max_missing_rate,
                                                               snps_only, mmap_window_mb, packed, packed_n_samples)
    out = pl.scan_rows_lm2(panel, rows, af, x, cov[:, pick], y, flip=flip, progress=progress_callback,
                           progress_every=progress_every)
    written = write_lm2_tsv(out_tsv, *cols, af, miss, out.cpu().numpy(), pick)
    _done(progress_callback, total)
    return written, total


# ------------------------------------------------------------------------------------------------
# Multi-trait LM scan (src/stats/lm_trait.rs): many traits against one panel, one combined table
# ------------------------------------------------------------------------------------------------

def _lm_single_as_trait_stats(stats, n, q0):
    """(m, 4) beta, se, pwald, plrt of `pipeline.scan_rows_lm` -> (m, 4) beta, se, chisq = n ln(1 + t^2 / df), pwald in the
    combined table's terms: a row without a finite beta and a finite positive se has chisq NaN and p 1."""
    st = np.array(stats, dtype=np.float64, copy=True)
    df = n - q0 - 1
    with np.errstate(all="ignore"):
        ok = np.isfinite(st[:, 0]) & np.isfinite(st[:, 1]) & (st[:, 1] > 0.0)
        t = st[:, 0] / st[:, 1]
        chisq = np.where(ok, float(n) * np.log(1.0 + t * t / float(df)), np.nan)
        p = np.where(ok & np.isfinite(st[:, 2]), np.clip(st[:, 2], np.finfo(np.float64).tiny, 1.0), 1.0)
    return np.stack([st[:, 0], st[:, 1], chisq, p], axis=1)


def _lm_traits_group(writer, panel, rows, flip, af, x, y_trait_major, names, prefixes, pmax=None, on_trait=None):
    """One group of traits that share the samples of `panel`, the design and the rows, appended to the combined table trait by
    trait: two or more through `pipeline.scan_rows_lm_traits` (in calls of at most 1 GiB of dense results), one alone through
    `pipeline.scan_rows_lm`.  pmax: only the rows with pwald <= pmax are written.  on_trait(name) after each trait."""
    from . import pipeline as pl
    y = _c(y_trait_major, np.float64)
    T, m, n = int(y.shape[0]), len(rows), panel.n
    if T == 1:
        st = _lm_single_as_trait_stats(pl.scan_rows_lm(panel, rows, af, x, y[0], flip=flip).cpu().numpy(), n, int(x.shape[1]))
        if pmax is None:
            writer.put(prefixes, st, names[0])
        else:
            sel = np.nonzero(st[:, 3] <= float(pmax))[0]
            writer.put(prefixes, st[sel], names[0], sel)
        if on_trait is not None:
            on_trait(names[0])
        return
    step = T if pmax is not None else max(1, min(pl.LMT_MAX_TRAIT_BATCH, (1 << 30) // (32 * max(m, 1))))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        if pmax is None:
            dense = pl.scan_rows_lm_traits(panel, rows, af, x, y[t0:t1], flip=flip).cpu().numpy()
            for t in range(t0, t1):
                writer.put(prefixes, dense[t - t0], names[t])
                if on_trait is not None:
                    on_trait(names[t])
        else:
            hits = pl.scan_rows_lm_traits(panel, rows, af, x, y[t0:t1], flip=flip, pmax=float(pmax))
            cut = np.searchsorted(hits.trait, np.arange(t1 - t0 + 1))
            for t in range(t0, t1):
                a, b = int(cut[t - t0]), int(cut[t - t0 + 1])
                writer.put(prefixes, hits.stats[a:b], names[t], hits.row[a:b])
                if on_trait is not None:
                    on_trait(names[t])


def _lmt_rows_check(label, ri, fl, mi, mf, n_snps):
    if not (fl.shape[0] == mi.shape[0] == mf.shape[0] == ri.shape[0]):
        raise ValueError(f"{label}prepared row metadata length mismatch: row_indices={ri.shape[0]}, row_flip={fl.shape[0]}, "
                         f"row_missing={mi.shape[0]}, row_maf={mf.shape[0]}")
    if ri.size and (ri.min() < 0 or ri.max() >= n_snps):
        bad = int(ri[(ri < 0) | (ri >= n_snps)][0])
        raise ValueError(f"{label}row index {bad} out of range for n_snps={n_snps}")
    if ri.size > 1 and np.any(np.diff(ri) < 0):
        raise ValueError(f"{label}prepared row_indices must be sorted in ascending BED order")


def _lmt_same(a, b):
    """The sharing test of `jobs_support_shared_fast_path` (lm_trait.rs:192-224, without its host-memory cap): design, samples,
    rows, flips, and the bits of row_missing and row_maf."""
    return (a["x"].shape == b["x"].shape and np.array_equal(a["x"].view(np.int64), b["x"].view(np.int64))
            and np.array_equal(a["sidx"], b["sidx"]) and np.array_equal(a["ri"], b["ri"]) and np.array_equal(a["fl"], b["fl"])
            and np.array_equal(a["mi"].view(np.int32), b["mi"].view(np.int32))
            and np.array_equal(a["mf"].view(np.int32), b["mf"].view(np.int32)))


def _lmt_run(bed_prefix, n_fam, jobs, out_tsv, progress_callback, mmap_window_mb, pmax):
    """Jobs (validated) -> the combined table.  Consecutive jobs that pass `_lmt_same` form a group; a group of one goes
    through the single-trait scan."""
    from . import bed as _bed
    from .tsv import TraitTableWriter, resolve_snp_name, trait_site_prefixes
    t_start = time.perf_counter()
    pk, _n_full, bim = _bed.stage_bed_payload(bed_prefix, mmap_window_mb)
    groups = []
    for job in jobs:
        if groups and _lmt_same(groups[-1][0], job):
            groups[-1].append(job)
        else:
            groups.append([job])
    out, total = [], len(jobs)
    writer = TraitTableWriter(out_tsv)
    try:
        panel, panel_key = None, None
        for grp in groups:
            j0 = grp[0]
            if panel_key is None or not np.array_equal(panel_key, j0["sidx"]):
                panel = None                         # one image at a time
                panel, panel_key = _panel(pk, n_fam, j0["sidx"]), j0["sidx"]
            rows = j0["ri"]
            chrom, pos, snp, a0, a1 = bim.columns(rows)
            prefixes = trait_site_prefixes(chrom, pos, [resolve_snp_name(*spc) for spc in zip(snp, chrom, pos)], a0, a1,
                                           j0["mf"], j0["mi"])
            order = iter(grp)

            def on_trait(_name):
                job = next(order)
                out.append((job["name"], job["n_idv"], len(rows), len(rows), time.perf_counter() - t_start))
                if progress_callback is not None:
                    progress_callback(len(out), total, job["name"])

            _lm_traits_group(writer, panel, rows, j0["fl"], j0["mf"], j0["x"], np.stack([j["y"] for j in grp]),
                             [j["name"] for j in grp], prefixes, pmax, on_trait)
    except BaseException:
        writer.abort()
        raise
    writer.close()
    return out


def _lmt_head_checks(chunk_size, mmap_window_mb):
    if int(chunk_size) <= 0:
        raise ValueError("chunk_size must be > 0")
    if mmap_window_mb is not None and int(mmap_window_mb) <= 0:
        raise ValueError("mmap_window_mb must be > 0")


def _lmt_fam(prefix):
    from . import bed as _bed
    bed_prefix = _bed_prefix(prefix)
    try:
        fam = _bed.read_fam_ids(bed_prefix)
    except OSError as e:
        raise ValueError(str(e))
    if not fam:
        raise ValueError("no samples in PLINK FAM")
    return bed_prefix, fam


def _lmt_n_snps(bed_prefix):
    with open(f"{bed_prefix}.bim") as fh:
        return sum(1 for ln in fh if len(ln.split()) >= 6)


def lm_trait_assoc_bed_matrix_to_tsv(prefix, trait_names, y_trait_major, x, sample_indices, row_indices, row_flip, row_missing,
                                     row_maf, out_tsv, chunk_size=10000, threads=0, progress_callback=None, mmap_window_mb=None,
                                     pmax=None):
    """`lm_trait_assoc_bed_matrix_to_tsv`, src/stats/lm_trait.rs:909-1054: T traits (`y_trait_major` (T, n)) that share the
    samples `sample_indices` (positions in the FAM), the design `x` (n, q0, intercept included) and the prepared rows, scanned
    with the plain LM and written as one combined table (`tsv.HEADER_TRAITS`: all rows of trait 1, then trait 2, ...) ->
    [(name, n_idv, kept_rows, scanned_rows, elapsed_s)].  Every argument error is a ValueError raised before the payload is read.
    `progress_callback(done_traits, total_traits, name)`.  `chunk_size` / `threads` are accepted for signature parity.
    Extension: `pmax` writes only the rows with pwald <= pmax."""
    _lmt_head_checks(chunk_size, mmap_window_mb)
    names = [str(v) for v in trait_names]
    if not names:
        return []
    if any(not v.strip() for v in names):
        raise ValueError("trait_names must not contain empty values")
    y = _c(y_trait_major, np.float64)
    xx = _c(x, np.float64)
    if y.ndim != 2:
        raise ValueError("y_trait_major must be a 2D float64 array")
    if xx.ndim != 2:
        raise ValueError("x must be a 2D float64 array")
    sidx = _c(sample_indices, np.int64).ravel()
    ri = _c(row_indices, np.int64).ravel()
    fl = np.asarray(row_flip).astype(bool).ravel()
    mi = _c(row_missing, np.float32).ravel()
    mf = _c(row_maf, np.float32).ravel()
    if y.shape[0] != len(names):
        raise ValueError(f"y_trait_major rows ({y.shape[0]}) must equal len(trait_names) ({len(names)})")
    if xx.shape[1] == 0:
        raise ValueError("x must have at least one column")
    if xx.shape[0] != y.shape[1]:
        raise ValueError(f"x rows ({xx.shape[0]}) must equal y_trait_major cols ({y.shape[1]})")
    if sidx.shape[0] != y.shape[1]:
        raise ValueError(f"sample_indices length ({sidx.shape[0]}) must equal y_trait_major cols ({y.shape[1]})")
    if not (fl.shape[0] == mi.shape[0] == mf.shape[0] == ri.shape[0]):
        _lmt_rows_check("", ri, fl, mi, mf, 0)
    bed_prefix, fam = _lmt_fam(prefix)
    bad = sidx[(sidx < 0) | (sidx >= len(fam))]
    if bad.size:
        raise ValueError(f"sample index {int(bad[0])} out of range for n_samples={len(fam)}")
    _lmt_rows_check("", ri, fl, mi, mf, _lmt_n_snps(bed_prefix))
    jobs = [dict(name=names[t], n_idv=int(y.shape[1]), y=y[t], x=xx, sidx=sidx, ri=ri, fl=fl, mi=mi, mf=mf)
            for t in range(len(names))]
    return _lmt_run(bed_prefix, len(fam), jobs, out_tsv, progress_callback, mmap_window_mb, pmax)


def lm_trait_assoc_bed_to_tsv(prefix, trait_specs, out_tsv, chunk_size=10000, threads=0, progress_callback=None,
                              mmap_window_mb=None, pmax=None):
    """`lm_trait_assoc_bed_to_tsv`, src/stats/lm_trait.rs:1057-1290: one dict per trait with the keys trait_name, y, x,
    sample_indices | sample_ids, row_indices, row_flip, row_missing, row_maf and optionally n_idv.  Consecutive specs with the
    same samples, design and rows (`jobs_support_shared_fast_path`) are scanned together on the matrix pipes; the others go
    trait by trait through the single-trait LM scan into the same combined table.  Returns and raises as
    `lm_trait_assoc_bed_matrix_to_tsv`."""
    _lmt_head_checks(chunk_size, mmap_window_mb)
    if not isinstance(trait_specs, list):
        raise ValueError("trait_specs must be a list of per-trait dict objects")
    if not trait_specs:
        return []
    bed_prefix, fam = _lmt_fam(prefix)
    fam_index, n_snps, jobs = None, None, []
    for k, spec in enumerate(trait_specs):
        if not isinstance(spec, dict):
            raise ValueError(f"trait_specs[{k}] must be a dict with trait_name/y/x/(sample_indices|sample_ids)/row_* keys")

        def req(key):
            if key not in spec or spec[key] is None:
                raise ValueError(f"missing required key '{key}'")
            return spec[key]

        name = str(req("trait_name"))
        if not name.strip():
            raise ValueError(f"trait_specs[{k}].trait_name must not be empty")
        y = _c(req("y"), np.float64)
        if y.ndim != 1:
            raise ValueError(f"trait_specs[{k}].y must be a 1D float64 array")
        xx = _c(req("x"), np.float64)
        if xx.ndim != 2:
            raise ValueError(f"trait_specs[{k}].x must be a 2D float64 array")
        if xx.shape[1] == 0:
            raise ValueError(f"trait_specs[{k}].x must have at least one column")
        if xx.shape[0] != y.shape[0]:
            raise ValueError(f"trait_specs[{k}] x rows ({xx.shape[0]}) must equal len(y) ({y.shape[0]})")
        if spec.get("sample_indices") is not None:
            sidx = _c(spec["sample_indices"], np.int64).ravel()
            if sidx.shape[0] != y.shape[0]:
                raise ValueError(f"trait_specs[{k}] sample_indices length ({sidx.shape[0]}) must equal len(y) ({y.shape[0]})")
            bad = sidx[(sidx < 0) | (sidx >= len(fam))]
            if bad.size:
                raise ValueError(f"trait_specs[{k}] sample index {int(bad[0])} out of range for n_samples={len(fam)}")
        else:
            sample_ids = [str(v) for v in req("sample_ids")]
            if len(sample_ids) != y.shape[0]:
                raise ValueError(f"trait_specs[{k}] sample_ids length ({len(sample_ids)}) must equal len(y) ({y.shape[0]})")
            if fam_index is None:
                fam_index = {sid: i for i, sid in enumerate(fam)}
            for sid in sample_ids:
                if sid not in fam_index:
                    raise ValueError(f"trait_specs[{k}] sample ID '{sid}' not found in BED/FAM")
            sidx = np.array([fam_index[sid] for sid in sample_ids], dtype=np.int64)
        ri = _c(req("row_indices"), np.int64).ravel()
        fl = np.asarray(req("row_flip")).astype(bool).ravel()
        mi = _c(req("row_missing"), np.float32).ravel()
        mf = _c(req("row_maf"), np.float32).ravel()
        if n_snps is None:
            n_snps = _lmt_n_snps(bed_prefix)
        _lmt_rows_check(f"trait_specs[{k}] ", ri, fl, mi, mf, n_snps)
        n_idv = int(spec["n_idv"]) if spec.get("n_idv") is not None else int(y.shape[0])
        jobs.append(dict(name=name, n_idv=n_idv, y=y, x=xx, sidx=sidx, ri=ri, fl=fl, mi=mi, mf=mf))
    return _lmt_run(bed_prefix, len(fam), jobs, out_tsv, progress_callback, mmap_window_mb, pmax)


def lm_trait_assoc_packed(packed, n_samples, y_trait_major, x, row_flip, row_maf, sample_indices=None, row_indices=None,
                          pmax=None):
    """Extension (the reference scans files only): the multi-trait LM scan of a packed payload in memory.  `y_trait_major`
    (T, n), `x` (n, q0) with the intercept, `row_flip` / `row_maf` per scanned row (the rows `row_indices` of the payload, or all).
    -> (T, m, 4) f64 beta, se, chisq, pwald; with `pmax` the arrays (trait int32, row int32, stats (k, 4)) of the pairs with
    pwald <= pmax, ordered by (trait, row), row = position in `row_indices`."""
    from . import pipeline as pl
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    y = _c(y_trait_major, np.float64)
    xx = _c(x, np.float64)
    if y.ndim != 2 or xx.ndim != 2 or xx.shape[0] != y.shape[1]:
        raise RuntimeError("y_trait_major must be (T, n) and x (n, q0)")
    idx, n_sel = _opt_idx(sample_indices)
    if (n_sel if idx is not None else int(n_samples)) != y.shape[1]:
        raise RuntimeError(f"sample_indices length mismatch: got {n_sel if idx is not None else int(n_samples)}, "
                           f"expected y_trait_major cols={y.shape[1]}")
    panel = _panel(packed, n_samples, idx)
    rows = np.arange(panel.m, dtype=np.int64) if row_indices is None else _c(row_indices, np.int64).ravel()
    if rows.size and (rows.min() < 0 or rows.max() >= panel.m):
        raise RuntimeError(f"row_indices out of range for n_snps={panel.m}")
    fl = np.asarray(row_flip).astype(bool).ravel()
    mf = _c(row_maf, np.float32).ravel()
    if fl.shape[0] != len(rows) or mf.shape[0] != len(rows):
        raise RuntimeError(f"row_flip / row_maf length mismatch: got {fl.shape[0]} / {mf.shape[0]}, expected {len(rows)}")
    res = pl.scan_rows_lm_traits(panel, rows, mf, xx, y, flip=fl, pmax=pmax)
    return res.cpu().numpy() if pmax is None else (res.trait, res.row, res.stats)


def lmm_trait_assoc_packed(packed, n_samples, y_trait_major, x, grm, row_flip, row_maf, sample_indices=None, row_indices=None,
                           chunk_size=10000, warm_start=None, warm_chain_pieces=1, force_model=True):
    """Extension (the reference has no single native function for this route: its trait-level LMM,
    `_run_mixed_trait_packed_multi_entry`, python/janusx/assoc/workflow_model_packed.py:5932-6723, is Python around
    `lmm_rotate_y_with_ut_f64`, `lmm_reml_null_f32` and one `lmm_reml_assoc_packed_f32` per trait): T traits on the same samples
    and design, scanned together -- ONE eigendecomposition of `grm` + 1e-6 I, ONE rotation of [X | Y], a null fit per trait
    (-5, 5, 50, 1e-3) and ONE rotation of every SNP block for all traits; bounds [-5, 5], max_iter 50, tol 1e-2, start log10
    lambda0 of the trait.  `y_trait_major` (T, n), `x` (n, p) with the intercept, `grm` (n, n) of the selected samples in their
    order, or (n_samples, n_samples) of all samples when `sample_indices` selects among them; `row_flip` / `row_maf` per scanned
    row (the rows `row_indices` of the payload, or all).  Warm start as `lmm_reml_assoc_packed_f32` (None = "chain"): chains of
    `chunk_size` scanned rows cut into `warm_chain_pieces`; "none": every SNP starts from log10 lambda0.
    force_model=False: `gwas_lmm_lm_null_lrt_decision` per trait; when any trait would switch to the LM nothing is scanned.
    -> (stats (T, m, 3) f64 beta, se, p -- None when a trait would switch --, nulls: per trait (lambda0, ML0, REML0, pve)
    -- with force_model=False followed by (switch, LRT statistic, p))."""
    import torch
    from . import pipeline as pl
    from .stats import scan_lut_from_counts
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if int(chunk_size) <= 0:
        raise RuntimeError("chunk_size must be > 0")
    y = _c(y_trait_major, np.float64)
    xx = _c(x, np.float64)
    if y.ndim != 2 or xx.ndim != 2 or xx.shape[0] != y.shape[1]:
        raise RuntimeError("y_trait_major must be (T, n) and x (n, p)")
    n = int(y.shape[1])
    idx, n_sel = _opt_idx(sample_indices)
    if (n_sel if idx is not None else int(n_samples)) != n:
        raise RuntimeError(f"sample_indices length mismatch: got {n_sel if idx is not None else int(n_samples)}, "
                           f"expected y_trait_major cols={n}")
    panel = _panel(packed, n_samples, idx)
    rows = np.arange(panel.m, dtype=np.int64) if row_indices is None else _c(row_indices, np.int64).ravel()
    if rows.size and (rows.min() < 0 or rows.max() >= panel.m):
        raise RuntimeError(f"row_indices out of range for n_snps={panel.m}")
    fl = np.asarray(row_flip).astype(bool).ravel()
    mf = _c(row_maf, np.float32).ravel()
    if fl.shape[0] != len(rows) or mf.shape[0] != len(rows):
        raise RuntimeError(f"row_flip / row_maf length mismatch: got {fl.shape[0]} / {mf.shape[0]}, expected {len(rows)}")
    k = grm if _is_device_tensor(grm) else torch.from_numpy(np.ascontiguousarray(np.asarray(grm))).to(panel.device)
    if k.ndim != 2 or k.shape[0] != k.shape[1] or int(k.shape[0]) not in (n, int(n_samples)):
        raise RuntimeError(f"grm must be ({n}, {n}) or ({int(n_samples)}, {int(n_samples)})")
    sub = idx if (idx is not None and int(k.shape[0]) != n) else None
    s, ut64 = pl.eigh_from_grm(k, 1e-6, sub, f32_consumer=True)
    models = pl.SpectralModel.for_traits(s, ut64, xx, y)
    del ut64
    nulls = [(mdl.null.lbd, mdl.null.ml0, mdl.null.reml0, mdl.null.pve) for mdl in models]
    if not force_model:
        lrt = [tuple(gwas_lmm_lm_null_lrt_decision(y[ti], xx[:, 1:], nulls[ti][1])[:3]) for ti in range(len(models))]
        nulls = [nl + d for nl, d in zip(nulls, lrt)]
        if any(d[0] for d in lrt):
            return None, nulls
    lut = scan_lut_from_counts(mf, fl, panel.counts()[rows], n)
    init = np.array([float(np.log10(nl[0])) if (np.isfinite(nl[0]) and nl[0] > 0.0) else float("nan") for nl in nulls])
    chain_off = None
    if _resolve_warm_start(warm_start, "JX_LMM_UNIFIED_NO_WARM_START") == "chain":
        chain_off = pl.traits_chain_offsets(len(rows), int(chunk_size), int(warm_chain_pieces))
    out = pl.scan_rows_lmm_traits(panel, models[0], rows, lut, models[0].y_rot, init, chain_off=chain_off)
    return out.cpu().numpy(), nulls


# ------------------------------------------------------------------------------------------------
# Genotype rows as numbers and the two matrix-free products the reference's Python layer asks for beside the path
# (src/stats/packed.rs:577-760, 2060-2560): decode of selected rows, M'alpha, cross-GRM times alpha
# ------------------------------------------------------------------------------------------------

def _raw_additive_lut(maf_rows, flip_rows, clamp_low_only):
    """[0, mean, 1, 2] or flipped per row; mean = max(2 maf, 0) (`bed_packed_decode_rows_f32`, packed.rs:652) or 2 maf as it is
    (`packed_malpha_f64` / `cross_grm_times_alpha_packed_f64`, packed.rs:2470, 2240)."""
    maf = np.asarray(maf_rows, dtype=np.float32)
    mean_g = (np.float32(2.0) * maf).astype(np.float32)
    if clamp_low_only:
        mean_g = np.maximum(mean_g, np.float32(0.0))
    flip = np.asarray(flip_rows).astype(bool)
    lut = np.empty((len(maf), 4), dtype=np.float32)
    lut[:, 0] = np.where(flip, 2.0, 0.0)
    lut[:, 1] = mean_g
    lut[:, 2] = 1.0
    lut[:, 3] = np.where(flip, 0.0, 2.0)
    return lut


def _packed_host_checks(packed, n_samples):
    packed = _c(packed, np.uint8)
    if packed.ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    bps = (int(n_samples) + 3) // 4
    if packed.shape[1] != bps:
        raise RuntimeError(f"packed second dimension mismatch: got {packed.shape[1]}, expected {bps} for "
                           f"n_samples={int(n_samples)}")
    return packed


def bed_packed_decode_rows_f32(packed, n_samples, row_indices, row_flip, row_maf, sample_indices=None):
    """src/stats/packed.rs:577-672: rows `row_indices` of the 2-bit payload as f32 values over `sample_indices` (0 / 1 / 2,
    missing = max(2 maf, 0), flipped rows 2 - g) -> f32 (len(row_indices), n_out).  `row_flip` / `row_maf` are indexed by
    payload row when they have one entry per payload row, else by position in `row_indices`."""
    import torch
    from . import pipeline as pl
    packed = _packed_host_checks(packed, n_samples)
    m = int(packed.shape[0])
    rows = _c(row_indices, np.int64).ravel()
    if rows.size and (rows.min() < 0 or rows.max() >= m):
        raise RuntimeError(f"row_indices out of range for {m} rows")
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    packed_space = flip.shape[0] == m and maf.shape[0] == m
    if not (packed_space or (flip.shape[0] == rows.shape[0] and maf.shape[0] == rows.shape[0])):
        raise RuntimeError(f"row_flip/row_maf length mismatch: got row_flip={flip.shape[0]}, row_maf={maf.shape[0]}, expected "
                           f"either packed_rows={m} or selected_rows={rows.shape[0]}")
    idx, n_sel = _opt_idx(sample_indices)
    if idx is not None and n_sel and (idx.min() < 0 or idx.max() >= int(n_samples)):
        raise RuntimeError("sample_indices out of range")
    n_out = n_sel if idx is not None else int(n_samples)
    if n_out == 0 or rows.size == 0:
        return np.zeros((rows.shape[0], n_out), dtype=np.float32)
    lut = _raw_additive_lut(maf[rows] if packed_space else maf, flip[rows] if packed_space else flip, True)
    dev = torch.device("cuda", torch.cuda.current_device())
    payload = torch.from_numpy(np.ascontiguousarray(packed[rows])).to(dev)
    panel = pl.Panel(payload, int(n_samples), idx)
    out = torch.empty((rows.shape[0], n_out), dtype=torch.float32, device=dev)
    lut_t = torch.from_numpy(lut).to(dev)
    check(lib().jxg_decode_rows_p32(panel.p32.data_ptr(), panel.m, n_out, None, int(rows.shape[0]), lut_t.data_ptr(),
                                    out.data_ptr(), n_out, pl._stream()))
    return out.cpu().numpy()


def bed_decode_rows_f32_from_meta(prefix, row_indices, row_flip, row_maf, sample_indices=None, mmap_window_mb=None):
    """src/stats/packed.rs:674-760: `bed_packed_decode_rows_f32` on the rows of a BED prefix (metadata per selected row)."""
    from .bed import read_bed_payload
    packed, n_samples, _bim = read_bed_payload(_bed_prefix(prefix))
    rows = _c(row_indices, np.int64).ravel()
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if flip.shape[0] != rows.shape[0] or maf.shape[0] != rows.shape[0]:
        raise RuntimeError(f"row meta length mismatch: row_indices={rows.shape[0]}, row_flip={flip.shape[0]}, "
                           f"row_maf={maf.shape[0]}")
    if rows.size and (rows.min() < 0 or rows.max() >= packed.shape[0]):
        raise RuntimeError("row_indices out of range")
    sub = np.ascontiguousarray(packed[rows])
    return bed_packed_decode_rows_f32(sub, n_samples, np.arange(rows.shape[0], dtype=np.int64), flip, maf, sample_indices)


def _malpha_inputs(packed, n_samples, row_flip, row_maf, sample_indices):
    import torch
    from . import pipeline as pl
    packed = _packed_host_checks(packed, n_samples)
    m = int(packed.shape[0])
    if m == 0:
        raise RuntimeError("packed must contain at least one SNP row")
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if flip.shape[0] != m:
        raise RuntimeError(f"row_flip length mismatch: got {flip.shape[0]}, expected {m}")
    if maf.shape[0] != m:
        raise RuntimeError(f"row_maf length mismatch: got {maf.shape[0]}, expected {m}")
    idx = _c(sample_indices, np.int64).ravel()
    if idx.size == 0:
        raise RuntimeError("sample_indices must not be empty")
    if idx.min() < 0 or idx.max() >= int(n_samples):
        raise RuntimeError("sample_indices out of range")
    dev = torch.device("cuda", torch.cuda.current_device())
    identity = idx.shape[0] == int(n_samples) and np.array_equal(idx, np.arange(int(n_samples)))
    panel = pl.Panel(torch.from_numpy(packed).to(dev), int(n_samples), None if identity else idx)
    lut_t = torch.from_numpy(_raw_additive_lut(maf, flip, False)).to(dev)
    return panel, lut_t, m, int(idx.shape[0]), dev


def packed_malpha_f64(packed, n_samples, row_flip, row_maf, sample_indices, alpha, block_rows=4096, threads=0):
    """src/stats/packed.rs:2352-2575: m_alpha[r] = sum_j g[r, s_j] alpha[j] over the mean-imputed raw genotypes
    ([0, 2 maf, 1, 2] or flipped) of the selected samples -> f64 (m).  (`jxg_packed_tdot`: f64 sums on the device; the
    reference rounds alpha to f32 and sums in an f32 sgemm.)"""
    import torch
    from . import pipeline as pl
    panel, lut_t, m, n_out, dev = _malpha_inputs(packed, n_samples, row_flip, row_maf, sample_indices)
    a = _c(alpha, np.float64).ravel()
    if a.shape[0] != n_out:
        raise RuntimeError(f"alpha length mismatch: got {a.shape[0]}, expected {n_out} (len(sample_indices))")
    out = torch.empty(m, dtype=torch.float64, device=dev)
    a_t = torch.from_numpy(a).to(dev)
    check(lib().jxg_packed_tdot(panel.p32.data_ptr(), panel.m, n_out, None, m, lut_t.data_ptr(), a_t.data_ptr(),
                                out.data_ptr(), pl._stream()))
    return out.cpu().numpy()


def cross_grm_times_alpha_packed_f64(packed, n_samples, row_flip, row_maf, sample_indices, m_alpha, m_mean, alpha_sum,
                                     mean_sq, mean_malpha, m_var_sum, block_rows=4096, threads=0):
    """src/stats/packed.rs:2060-2350: K_cross alpha for the samples `sample_indices` without the cross GRM:
    ((M_s' m_alpha) - (M_s' m_mean) alpha_sum + mean_sq alpha_sum - mean_malpha) / m_var_sum -> f64 (n_out, 1)
    (`jxg_packed_dot`, two passes over the payload)."""
    import math
    import torch
    from . import pipeline as pl
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if not (math.isfinite(m_var_sum) and m_var_sum > 0.0):
        raise RuntimeError("m_var_sum must be finite and > 0 for compact cross-GRM prediction")
    if not (math.isfinite(alpha_sum) and math.isfinite(mean_sq) and math.isfinite(mean_malpha)):
        raise RuntimeError("alpha_sum/mean_sq/mean_malpha must be finite")
    panel, lut_t, m, n_out, dev = _malpha_inputs(packed, n_samples, row_flip, row_maf, sample_indices)
    ma = _c(m_alpha, np.float64).ravel()
    mm = _c(m_mean, np.float64).ravel()
    if ma.shape[0] != m:
        raise RuntimeError(f"m_alpha length mismatch: got {ma.shape[0]}, expected {m}")
    if mm.shape[0] != m:
        raise RuntimeError(f"m_mean length mismatch: got {mm.shape[0]}, expected {m}")
    t1 = torch.empty(n_out, dtype=torch.float64, device=dev)
    t2 = torch.empty(n_out, dtype=torch.float64, device=dev)
    for vec, dst in ((ma, t1), (mm, t2)):
        v_t = torch.from_numpy(vec).to(dev)
        check(lib().jxg_packed_dot(panel.p32.data_ptr(), panel.m, n_out, None, m, lut_t.data_ptr(), v_t.data_ptr(),
                                   dst.data_ptr(), pl._stream()))
    const_term = float(mean_sq) * float(alpha_sum) - float(mean_malpha)
    out = (t1.cpu().numpy() - t2.cpu().numpy() * float(alpha_sum) + const_term) * (1.0 / float(m_var_sum))
    return out.reshape(-1, 1)


# ------------------------------------------------------------------------------------------------
# GBLUP (`jx gs -BLUP`, n <= 15 000 branch): src/stats/gblup.rs:1242-1516 `gblup_reml_npy_grm`
# ------------------------------------------------------------------------------------------------

# ---- the argument front end the GBLUP / rrBLUP / HE mirrors below share: each check of the reference written once ----------

def _gs_check_iter_opts(max_iter, tol, std_eps):
    import math
    if int(max_iter) == 0:
        raise RuntimeError("max_iter must be > 0")
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be finite and > 0")
    if not (math.isfinite(std_eps) and std_eps > 0.0):
        raise RuntimeError("std_eps must be finite and > 0")


def _gs_check_reml_opts(g_eps, low, high, max_iter, tol):
    import math
    if not (math.isfinite(g_eps) and g_eps >= 0.0):
        raise RuntimeError("g_eps must be finite and >= 0")
    if not (math.isfinite(low) and math.isfinite(high) and low < high):
        raise RuntimeError("low/high must be finite and low < high")
    if int(max_iter) == 0:
        raise RuntimeError("max_iter must be > 0")
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be finite and > 0")


def _gs_require_stats(who, path, maf, row_flip, packed_n_samples):
    if maf is None:
        raise RuntimeError(f"{who}: {path} path requires `maf` argument.")
    if row_flip is None:
        raise RuntimeError(f"{who}: {path} path requires `row_flip` argument.")
    if int(packed_n_samples) == 0:
        raise RuntimeError(f"{who}: {path} path requires packed_n_samples > 0.")


def _gs_payload(who, prefix, packed, packed_n_samples, maf, row_flip):
    """The caller's payload with its maf / row_flip, or -- nothing of that given -- the file's payload with the loader's own
    statistics -> (payload, n_samples, maf, row_flip).  A payload that already lives in HBM is used in place (no host copy of
    50 GB)."""
    if packed is None and int(packed_n_samples) <= 0:
        pk, _miss, maf, _std, n_samples = load_bed_2bit_packed(prefix)
        return pk, n_samples, maf, bed_packed_row_flip_mask(pk, n_samples)
    if packed is None:
        raise RuntimeError(f"{who}: packed payload path requires `packed` argument.")
    _gs_require_stats(who, "packed payload", maf, row_flip, packed_n_samples)
    pk = packed if _is_device_tensor(packed) else _c(packed, np.uint8)
    if len(pk.shape) != 2:
        raise RuntimeError("packed BED payload must be 2D (m, bytes_per_snp).")
    return (pk.contiguous() if _is_device_tensor(pk) else pk), int(packed_n_samples), maf, row_flip


def _gs_check_payload_shape(pk, n_samples):
    if int(pk.shape[0]) == 0:
        raise RuntimeError("No SNP rows found in BED input.")
    if pk.shape[1] != (n_samples + 3) // 4:
        raise RuntimeError(f"packed second dimension mismatch: got {pk.shape[1]}, expected {(n_samples + 3) // 4}")


def _gs_kept_rows(m_total, maf, row_flip, site_keep):
    """-> (rows int64 or None when every row of the payload is kept, maf f32 and flip mask of the kept rows)."""
    maf_full = _c(maf, np.float32).ravel()
    if maf_full.shape[0] != m_total:
        raise RuntimeError(f"maf length mismatch: got {maf_full.shape[0]}, expected {m_total}")
    flip_full = np.asarray(row_flip).astype(bool).ravel()
    if flip_full.shape[0] != m_total:
        raise RuntimeError(f"row_flip length mismatch: got {flip_full.shape[0]}, expected {m_total}")
    if site_keep is None:
        return None, maf_full, flip_full
    mask = np.asarray(site_keep).astype(bool).ravel()
    if mask.shape[0] != m_total:
        raise RuntimeError(f"site_keep length mismatch: got {mask.shape[0]}, expected {m_total}")
    rows = np.nonzero(mask)[0].astype(np.int64)
    if rows.shape[0] == 0:
        raise RuntimeError("No SNPs remained after applying site_keep mask.")
    if rows.shape[0] == m_total:
        return None, maf_full, flip_full
    return rows, maf_full[rows], flip_full[rows]


def _gs_meta_rows(row_source_indices, row_flip, row_maf, empty_msg):
    """The metadata triple of the streaming GBLUP forms -> (rows int64, flip mask, maf f32), one entry per row."""
    src = _c(row_source_indices, np.int64).ravel()
    if src.size == 0:
        raise RuntimeError(empty_msg)
    if (src < 0).any():
        raise RuntimeError("row_source_indices must be non-negative.")
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if flip.shape[0] != src.shape[0] or maf.shape[0] != src.shape[0]:
        raise RuntimeError(f"metadata length mismatch: row_source_indices={src.shape[0]}, row_flip={flip.shape[0]}, "
                           f"row_maf={maf.shape[0]}")
    return src, flip, maf


def _gs_train_y(train_sample_indices, y_train, n_samples, min_train=1, few_msg="train_sample_indices must not be empty."):
    """-> (training sample indices int64, phenotype f64), checked in the reference's order."""
    tr = _c(train_sample_indices, np.int64).ravel()
    if tr.size and (tr.min() < 0 or tr.max() >= n_samples):
        raise RuntimeError("train_sample_indices out of range")
    if tr.shape[0] < min_train:
        raise RuntimeError(few_msg)
    y = _c(y_train, np.float64).ravel()
    if y.shape[0] != tr.shape[0]:
        raise RuntimeError(f"y_train length mismatch: got {y.shape[0]}, expected {tr.shape[0]}")
    if not np.all(np.isfinite(y)):
        raise RuntimeError("y_train contains non-finite values.")
    return tr, y


def _gs_test_idx(test_sample_indices, n_samples):
    te = np.zeros(0, dtype=np.int64) if test_sample_indices is None else _c(test_sample_indices, np.int64).ravel()
    if te.size and (te.min() < 0 or te.max() >= n_samples):
        raise RuntimeError("test_sample_indices out of range")
    return te


def _gs_pick_idx(train_pred_local_indices, n_train):
    if train_pred_local_indices is None:
        return None
    pick = _c(train_pred_local_indices, np.int64).ravel()
    if pick.size and (pick.min() < 0 or pick.max() >= n_train):
        raise RuntimeError("train_pred_local_indices out of range")
    return pick


def _gs_standardise(p, std_eps):
    """Row mean 2p and inverse standard deviation 1 / sqrt(2p(1-p)) in f32 of the (clipped) frequencies `p`, 0 where the
    variance does not exceed max(std_eps, 1e-12) -> (rm, ri, number of rows above the cut)."""
    f32 = np.float32
    rm = (f32(2.0) * p).astype(f32)
    var = np.maximum((f32(2.0) * p * (f32(1.0) - p)).astype(f32), f32(0.0))
    good = var > f32(max(float(std_eps), 1e-12))
    ri = np.zeros_like(var)
    ri[good] = (f32(1.0) / np.sqrt(var[good])).astype(f32)
    return rm, ri, int(np.count_nonzero(good))


def _rrblup_row_stats(maf_keep, rows, m_total, row_mean, row_inv_sd, std_eps):
    """`rrblup_subset_or_validate_stats` (rrblup.rs:568-625): the caller's row_mean / row_inv_sd, of the kept rows or of all
    rows of the payload, or those of the minor frequencies clipped to [0, 0.5] -> (rm, ri, m_effective)."""
    f32 = np.float32
    if (row_mean is None) != (row_inv_sd is None):
        raise RuntimeError("rrBLUP standardization requires row_mean and row_inv_sd together when overriding row stats.")
    if row_mean is None:
        return _gs_standardise(np.clip(maf_keep, f32(0.0), f32(0.5)).astype(f32), std_eps)
    rm = _c(row_mean, f32).ravel()
    ri = _c(row_inv_sd, f32).ravel()
    eff_m = int(maf_keep.shape[0])
    if rm.shape[0] == m_total and ri.shape[0] == m_total and rows is not None:
        rm, ri = rm[rows], ri[rows]
    elif rm.shape[0] != eff_m or ri.shape[0] != eff_m:
        raise RuntimeError(f"External row_mean/row_inv_sd length mismatch: mean={rm.shape[0]}, inv={ri.shape[0]}, "
                           f"expected active={eff_m} or full={m_total}.")
    return rm, ri, int(np.count_nonzero(np.isfinite(ri) & (ri > 0)))


def gblup_reml_grm(grm, train_sample_indices, y_train, test_sample_indices=None, train_pred_local_indices=None,
                   g_eps=1e-8, low=-6.0, high=6.0, max_iter=50, tol=1e-4, threads=0,
                   return_variance_components=False, estimate_only=False):
    """In-memory form of `gblup_reml_npy_grm`: `grm` (n_full, n_full) f32/f64.  Returns the reference's 12-tuple
    (pred_train (k,1), pred_test (t,1), pve, lambda, ml, reml, evd_backend, evd_elapsed, 0, sigma_g2, sigma_e2,
    effect (empty))."""
    _gs_check_reml_opts(g_eps, low, high, max_iter, tol)
    k = np.asarray(grm)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise RuntimeError("GRM must be a square matrix")
    is64 = k.dtype == np.float64
    k = _c(k, np.float64 if is64 else np.float32)
    tr = _c(train_sample_indices, np.int64).ravel()
    y = _c(y_train, np.float64).ravel()
    if y.shape[0] != tr.shape[0]:
        raise RuntimeError("y_train length must equal train_sample_indices length")
    te = np.zeros(0, dtype=np.int64) if test_sample_indices is None else _c(test_sample_indices, np.int64).ravel()
    pt = np.zeros(tr.shape[0], dtype=np.float64)
    pe = np.zeros(max(te.shape[0], 1), dtype=np.float64)
    sc = np.zeros(8, dtype=np.float64)
    t0 = time.perf_counter()
    check(lib().jx_gblup_reml_grm(_p(k), 1 if is64 else 0, int(k.shape[0]), _p(tr), int(tr.shape[0]), _p(y), _p(te),
                                  int(te.shape[0]), float(g_eps), float(low), float(high), int(max_iter), float(tol),
                                  1 if estimate_only else 0, _p(pt), _p(pe), _p(sc)))
    el = time.perf_counter() - t0
    if estimate_only:
        ptr = np.zeros((0, 1))
        pte = np.zeros((0, 1))
    else:
        if train_pred_local_indices is not None:
            pt = pt[np.asarray(train_pred_local_indices, dtype=np.int64)]
        ptr = pt.reshape(-1, 1)
        pte = pe[: te.shape[0]].reshape(-1, 1)
    sg2 = float(sc[4]) if return_variance_components else float("nan")
    se2 = float(sc[5]) if return_variance_components else float("nan")
    return (ptr, pte, float(sc[0]), float(sc[1]), float(sc[2]), float(sc[3]), "rocsolver", el, 0, sg2, se2,
            np.zeros(0, dtype=np.float64))


def _gblup_meta_lut(maf, flip, identity):
    """Centred additive decode of `decode_meta_block_f32` (src/stats/gblup.rs:239-404; bedmath.rs:1359-1441 for a sample
    subset) -> (LUT (m, 4) f32 of centred values, missing = 0; sum of the row variances; row means f64)."""
    from . import stats as st
    m = int(maf.shape[0])
    mafc = np.clip(maf, np.float32(0.0), np.float32(1.0))
    if identity:
        p64 = mafc.astype(np.float64)
        mean64 = 2.0 * p64
        var = 2.0 * p64 * (1.0 - p64)
        mean32 = mean64.astype(np.float32)
        row_mean = mean64
    else:
        mean32 = (np.float32(2.0) * mafc).astype(np.float32)
        pg = np.clip(np.float32(0.5) * mean32, np.float32(0.0), np.float32(1.0))
        var = np.maximum(np.float32(2.0) * pg * (np.float32(1.0) - pg), np.float32(0.0)).astype(np.float64)
        row_mean = mean32.astype(np.float64)
    return st.grm_lut_from_mean_scale(mean32, np.ones(m, dtype=np.float32), flip), float(np.sum(var)), row_mean


def gblup_effect_from_meta_stream(prefix, sample_indices, alpha, row_source_indices, row_flip, row_maf, mode="a",
                                  block_rows=4096, threads=0, mmap_window_mb=None):
    """src/stats/gblup.rs:2788-2895 -> `compute_effect_beta_from_meta_stream` (:930-1033): marker effects
    beta[r] = sum_j z[r, s_j] alpha[j] / sum(var) over the centred decode of the caller-prepared BED rows (the marker-effect
    output of `jx gs -BLUP`, python/janusx/gs/workflow.py:5103) -> f64 (m).  `jxg_packed_tdot` on the centred LUT."""
    import torch
    from . import pipeline as pl
    from .bed import stage_bed_payload
    mode_n = str(mode).strip().lower()
    if mode_n not in ("a", "add", "additive", "d", "dom", "dominance"):
        raise RuntimeError("mode must be one of {'a','additive','d','dominance'}")
    if mode_n in ("d", "dom", "dominance"):
        raise RuntimeError("mode 'dominance' is outside this build's scope (additive model only)")
    packed, n_fam, _bim = stage_bed_payload(_bed_prefix(prefix), mmap_window_mb)
    if n_fam == 0:
        raise RuntimeError("No samples found in BED input.")
    tr = _c(sample_indices, np.int64).ravel()
    if tr.size and (tr.min() < 0 or tr.max() >= n_fam):
        raise RuntimeError("sample_indices out of range")
    a = _c(alpha, np.float64).ravel()
    if a.shape[0] != tr.shape[0]:
        raise RuntimeError(f"alpha length mismatch: got {a.shape[0]}, expected {tr.shape[0]}")
    src, flip, maf = _gs_meta_rows(row_source_indices, row_flip, row_maf, "row_source_indices must not be empty.")
    if tr.size == 0:
        raise RuntimeError("compute_effect_beta_from_meta_stream: sample_idx must not be empty")
    if int(src.max()) >= int(packed.shape[0]):
        raise RuntimeError("row_source_indices out of range")
    identity = tr.shape[0] == n_fam and np.array_equal(tr, np.arange(n_fam))
    glut, var_sum, _row_mean = _gblup_meta_lut(maf, flip, identity)
    if not (np.isfinite(var_sum) and var_sum > 0.0):
        raise RuntimeError("compute_effect_beta_from_meta_stream: invalid denominator")
    dev = packed.device
    rows_payload = packed[torch.from_numpy(src).to(dev)]
    del packed
    panel = pl.Panel(rows_payload, n_fam, None if identity else tr)
    m = int(src.shape[0])
    out = torch.empty(m, dtype=torch.float64, device=dev)
    lut_t = torch.from_numpy(np.ascontiguousarray(glut, dtype=np.float32)).to(dev)     # named: alive until the launch is queued
    a_t = torch.from_numpy(a).to(dev)
    check(lib().jxg_packed_tdot(panel.p32.data_ptr(), panel.m, int(tr.shape[0]), None, m, lut_t.data_ptr(), a_t.data_ptr(),
                                out.data_ptr(), pl._stream()))
    return out.cpu().numpy() * (1.0 / var_sum)


def _gblup_meta_grm(rows_payload, n_samples, tr, flip, maf):
    """Centred-additive GRM of the samples `tr` over the payload rows with the caller's flip / maf metadata, the
    formulation of `build_grm_from_meta_stream` (src/stats/gblup.rs:406-652; per-row centring and variance of
    `decode_meta_block_f32` :239-404, bedmath.rs:1359-1441 for a sample subset) -> (K f64 (n_tr, n_tr) on the device,
    scaled by 1 / sum(var); sum(var); the panel; the row means in f64)."""
    import torch
    from . import pipeline as pl
    from . import stats as st
    n_tr = int(tr.shape[0])
    m = int(rows_payload.shape[0])
    identity = n_tr == n_samples and np.array_equal(tr, np.arange(n_samples))
    glut, var_sum, row_mean = _gblup_meta_lut(maf, flip, identity)
    panel = pl.Panel(rows_payload, n_samples, None if identity else tr)
    acc = pl.grm_accumulate(panel, np.arange(m, dtype=np.int64), glut)
    k = pl.grm_finalize(acc, n_tr, var_sum, torch.float64)
    del acc
    return k, var_sum, panel, row_mean


def gblup_reml_packed_bed(prefix, train_sample_indices, y_train, test_sample_indices=None,
                          train_pred_local_indices=None, site_keep=None, g_eps=1e-8, low=-6.0, high=6.0, max_iter=50,
                          tol=1e-4, block_rows=4096, threads=0, return_variance_components=False, estimate_only=False,
                          return_effect=False, row_source_indices=None, row_flip=None, row_maf=None,
                          mmap_window_mb=None):
    """src/stats/gblup.rs:1517-1958, metadata-streaming path (the one `python/janusx/gs/workflow.py:6300-6360` takes; without
    the metadata arguments the `site_keep` route :1986-2140 with the loader's row statistics, same formulation):
    GRM of the training samples straight from the BED payload, spectral REML, then marker effects
    effect_beta = (M' alpha - mean * sum(alpha)) / sum(var) and predictions alpha0 + M beta, M never materialised
    (jxg_packed_tdot / jxg_packed_dot).  Returns the reference's 12-tuple (pred_train (k,1), pred_test (t,1), pve,
    lambda, ml, reml, evd_backend, evd_elapsed, eff_m, sigma_g2, sigma_e2, effect (m) or empty)."""
    import math
    import torch
    from . import pipeline as pl
    from . import stats as st
    from .bed import read_bed_payload
    _gs_check_reml_opts(g_eps, low, high, max_iter, tol)
    packed_loaded = None
    if row_source_indices is None or row_flip is None or row_maf is None:
        # `site_keep` route (gblup.rs:1986-2140): the whole payload (or the rows of the mask) with the loader's own row
        # statistics -- alt-allele frequency over all samples (`load_bed_2bit_packed`) and the flip mask of
        # `bed_packed_row_flip_mask` -- then the same model.  The reference evaluates it in marker space when
        # n_train > m (`gblup_marker_fast_packed`) and through `grm_packed_f64_with_stats` otherwise; here both go through
        # the formulation of the metadata route below (one GRM of the training samples, spectral REML, M' alpha).
        packed_loaded, _miss, maf_all, _std, n_loaded = load_bed_2bit_packed(prefix)
        if n_loaded == 0:
            raise RuntimeError("No samples found in BED input.")
        m_total = int(packed_loaded.shape[0])
        if m_total == 0:
            raise RuntimeError("No SNP rows found in BED input.")
        flip_all = bed_packed_row_flip_mask(packed_loaded, n_loaded)
        rows, row_maf, row_flip = _gs_kept_rows(m_total, maf_all, flip_all, site_keep)
        row_source_indices = np.arange(m_total, dtype=np.int64) if rows is None else rows
    src, flip, maf = _gs_meta_rows(row_source_indices, row_flip, row_maf,
                                   "row_source_indices must not be empty for metadata streaming path.")
    if packed_loaded is not None:
        packed, n_samples = packed_loaded, int(n_loaded)
    else:
        packed, n_samples, _bim = read_bed_payload(prefix)
    if n_samples == 0:
        raise RuntimeError("No samples found in BED input.")
    if src.max() >= packed.shape[0]:
        raise RuntimeError("row_source_indices out of range")
    tr, y = _gs_train_y(train_sample_indices, y_train, n_samples)
    te = _gs_test_idx(test_sample_indices, n_samples)
    n_tr = int(tr.shape[0])
    if n_tr <= 1:
        raise RuntimeError("GBLUP REML requires at least 2 training samples.")
    pick = tr if train_pred_local_indices is None else tr[np.asarray(train_pred_local_indices, dtype=np.int64)]
    m = int(src.shape[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    rows_payload = torch.from_numpy(np.ascontiguousarray(packed[src])).to(dev)
    k, var_sum, panel, row_mean = _gblup_meta_grm(rows_payload, n_samples, tr, flip, maf)
    k.diagonal().add_(float(g_eps))
    y_mean = float(np.sum(y) / n_tr)
    yc = torch.from_numpy(y - y_mean).to(dev)
    alpha = torch.empty(n_tr, dtype=torch.float64, device=dev)
    fit = np.zeros(6, dtype=np.float64)
    t0 = time.perf_counter()
    check(lib().jxg_gblup_fit(k.data_ptr(), n_tr, 0.0, yc.data_ptr(), float(low), float(high), float(tol),
                              int(max_iter), alpha.data_ptr(), fit.ctypes.data, stream))
    evd_elapsed = time.perf_counter() - t0
    lbd, beta_rot, q, ml, reml, mean_s = [float(v) for v in fit]
    n_eff = float(n_tr - 1)
    sg2 = q / max(n_eff, 1.0)
    se2 = lbd * sg2
    var_g = sg2 * max(mean_s, 0.0)
    den = var_g + se2
    pve = var_g / den if (math.isfinite(den) and den > 0.0) else float("nan")
    beta0 = y_mean + beta_rot
    pred_tr = np.zeros((0, 1))
    pred_te = np.zeros((0, 1))
    effect = np.zeros(0, dtype=np.float64)
    if (not estimate_only) or return_effect:
        mg = np.clip(np.float32(2.0) * maf, np.float32(0.0), np.float32(2.0)).astype(np.float32)
        rlut = np.empty((m, 4), dtype=np.float32)      # mean-imputed raw genotype (bedmath.rs:983-988)
        rlut[:, 0] = np.where(flip, 2.0, 0.0)
        rlut[:, 1] = mg
        rlut[:, 2] = 1.0
        rlut[:, 3] = np.where(flip, 0.0, 2.0)
        rlut_t = torch.from_numpy(rlut).to(dev)
        m_alpha_t = torch.empty(m, dtype=torch.float64, device=dev)
        check(lib().jxg_packed_tdot(panel.p32.data_ptr(), panel.m, n_tr, None, m, rlut_t.data_ptr(), alpha.data_ptr(),
                                    m_alpha_t.data_ptr(), stream))
        m_alpha = m_alpha_t.cpu().numpy()
        alpha_sum = float(alpha.sum().item())
        mean_sq = float(np.sum(row_mean * row_mean))
        mean_malpha = float(np.sum(row_mean * m_alpha))
        inv_var = 1.0 / max(var_sum, 1e-12)
        effect = (m_alpha - row_mean * alpha_sum) * inv_var
        alpha0 = beta0 + (mean_sq * alpha_sum - mean_malpha) * inv_var
        if not estimate_only:
            beta_t = torch.from_numpy(effect).to(dev)

            def predict(idx):
                if len(idx) == 0:
                    return np.zeros((0, 1))
                pan = pl.Panel(rows_payload, n_samples, np.asarray(idx, dtype=np.int64))
                out = torch.empty(len(idx), dtype=torch.float64, device=dev)
                check(lib().jxg_packed_dot(pan.p32.data_ptr(), pan.m, len(idx), None, m, rlut_t.data_ptr(),
                                           beta_t.data_ptr(), out.data_ptr(), stream))
                return (out.cpu().numpy() + alpha0).reshape(-1, 1)

            pred_tr = predict(pick)
            pred_te = predict(te)
    sg2_o = sg2 if return_variance_components else float("nan")
    se2_o = se2 if return_variance_components else float("nan")
    return (pred_tr, pred_te, pve, lbd, ml, reml, "rocsolver", evd_elapsed, m, sg2_o, se2_o,
            effect if return_effect else np.zeros(0, dtype=np.float64))


def gblup_reml_npy_grm(grm_path, train_sample_indices, y_train, test_sample_indices=None,
                       train_pred_local_indices=None, g_eps=1e-8, low=-6.0, high=6.0, max_iter=50, tol=1e-4,
                       threads=0, return_variance_components=False, estimate_only=False):
    """src/stats/gblup.rs:1242-1516: `.npy` GRM (f32/f64 C-order) on disk."""
    k = np.load(grm_path)
    return gblup_reml_grm(k, train_sample_indices, y_train, test_sample_indices, train_pred_local_indices, g_eps, low,
                          high, max_iter, tol, threads, return_variance_components, estimate_only)


# ---- rrBLUP by PCG over the packed payload ---------------------------------------------------------

def load_bed_2bit_packed(prefix):
    """src/io/gfreader.rs:4401-4530: (packed (m, ceil(n/4)) u8, missing_rate f32, maf f32, std_denom f32, n_samples);
    the per-SNP counts come from the device, the f32 expressions are the reference's."""
    from .bed import read_bed_payload
    p = str(prefix)
    if p.lower().endswith((".bed", ".bim", ".fam")):
        p = p[:-4]
    packed, n_samples, _bim = read_bed_payload(p)
    if n_samples == 0:
        raise RuntimeError("no samples found in PLINK input")
    cnt = bed_row_counts(packed, n_samples)
    mi, he, ho = cnt[:, 0].astype(np.int64), cnt[:, 1].astype(np.int64), cnt[:, 2].astype(np.int64)
    f32 = np.float32
    miss = (mi.astype(f32) / f32(n_samples)).astype(f32)
    nm = n_samples - mi
    alt = he + 2 * ho
    ok = nm > 0
    pfreq = np.zeros(mi.shape[0], dtype=f32)
    pfreq[ok] = alt[ok].astype(f32) / (f32(2.0) * nm[ok].astype(f32))
    maf = np.where(ok, np.minimum(pfreq, f32(1.0) - pfreq), f32(0.0)).astype(f32)
    d = np.sqrt((f32(2.0) * pfreq * (f32(1.0) - pfreq)).astype(f32)).astype(f32)
    std = np.where(ok & np.isfinite(d), d, f32(0.0)).astype(f32)
    return packed, miss, maf, std, int(n_samples)


def bed_packed_row_flip_mask(packed, n_samples):
    """src/stats/packed.rs:45-121: True where the ALT frequency among non-missing calls exceeds 0.5 (f64)."""
    packed = _c(packed, np.uint8)
    if packed.ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    if packed.shape[1] != (int(n_samples) + 3) // 4:
        raise RuntimeError(f"packed second dimension mismatch: got {packed.shape[1]}, expected "
                           f"{(int(n_samples) + 3) // 4} for n_samples={int(n_samples)}")
    cnt = bed_row_counts(packed, n_samples).astype(np.int64)
    nm = int(n_samples) - cnt[:, 0]
    alt = cnt[:, 1] + 2 * cnt[:, 2]
    out = np.zeros(cnt.shape[0], dtype=bool)
    ok = nm > 0
    out[ok] = (alt[ok].astype(np.float64) / (2.0 * nm[ok].astype(np.float64))) > 0.5
    return out


class pcg_image_scope:
    """`with pcg_image_scope():` -- inside, the two images of the training payload that `he_pcg_bed` / `rrblup_pcg_bed` build
    (SNP-major and sample-major, 40 GB each at BASELINE configs[4]) stay in HBM between the calls and a second call on the same
    DEVICE payload, kept rows and training samples reuses them (`jx gs -rrBLUP -rr-solver pcg`: lambda by Haseman-Elston, then the
    solve).  The caller guarantees the payload does not change inside the scope; leaving it frees the images (`jx_pcg_image_scope`)."""

    def __enter__(self):
        check(lib().jx_pcg_image_scope(1))
        return self

    def __exit__(self, et, ev, tb):
        lib().jx_pcg_image_scope(0)
        return False


def rrblup_pcg_bed(prefix, train_sample_indices, y_train, test_sample_indices=None, train_pred_local_indices=None,
                   site_keep=None, lambda_value=10000.0, tol=1e-4, max_iter=100, block_rows=4096, std_eps=1e-12,
                   threads=0, progress_callback=None, progress_every=0, compute_trainvar=False, packed=None,
                   packed_n_samples=0, maf=None, row_flip=None, row_mean=None, row_inv_sd=None, blas_threads=0):
    """src/stats/rrblup.rs:3494-4307.  Marker effects of the standardised genotypes by Jacobi-preconditioned CG on the
    device (`jx_rrblup_pcg_packed`), the payload resident in HBM for the whole solve.  Returns the reference's tuple
    (pred_train (k,1), pred_test (t,1), pve_trainvar, converged, iters, rel_res, m_effective, pve_lambda_vc,
    k_trace_mean, beta f32 (m)).  `block_rows`, `threads`, `blas_threads` are accepted and ignored; the streaming-stats
    form (maf/row_flip with a prefix and no payload) loads the payload from the prefix."""
    import math
    from . import stats as st
    _gs_check_iter_opts(max_iter, tol, std_eps)
    if (not math.isfinite(lambda_value)) or lambda_value < 0.0:
        raise RuntimeError("lambda_value must be finite and >= 0")
    f32 = np.float32
    if packed is None and (maf is not None or row_flip is not None or int(packed_n_samples) > 0):
        _gs_require_stats("rrblup_pcg_bed", "streaming stats", maf, row_flip, packed_n_samples)
        if not str(prefix).strip():
            raise RuntimeError("rrblup_pcg_bed: streaming stats path requires non-empty prefix.")
        from .bed import read_bed_payload
        pk, n_file, _bim = read_bed_payload(str(prefix))
        n_samples = int(packed_n_samples)
        if n_file != n_samples:
            raise RuntimeError(f"packed_n_samples mismatch: got {n_samples}, BED has {n_file}")
    else:
        pk, n_samples, maf, row_flip = _gs_payload("rrblup_pcg_bed", prefix, packed, packed_n_samples, maf, row_flip)
    _gs_check_payload_shape(pk, n_samples)
    m_total = int(pk.shape[0])
    rows, maf_keep, flip_keep = _gs_kept_rows(m_total, maf, row_flip, site_keep)
    eff_m = int(maf_keep.shape[0])
    tr, y = _gs_train_y(train_sample_indices, y_train, n_samples)
    te = _gs_test_idx(test_sample_indices, n_samples)
    n_train = int(tr.shape[0])
    pick = _gs_pick_idx(train_pred_local_indices, n_train)
    lambda_use = f32(max(float(lambda_value), 1e-8))
    rm, ri, m_effective = _rrblup_row_stats(maf_keep, rows, m_total, row_mean, row_inv_sd, std_eps)
    if row_mean is not None and m_effective == 0:
        raise RuntimeError("rrBLUP standardization received zero effective markers from external row_inv_sd.")
    lut = st.grm_lut_from_mean_scale(rm, ri, flip_keep)
    need_all = pick is None
    need_train = need_all or bool(compute_trainvar) or (pick is not None and pick.size > 0)
    beta = np.zeros(eff_m, dtype=f32)
    pred_tr_full = np.zeros(n_train, dtype=np.float64) if need_train else None
    pred_te = np.zeros(te.shape[0], dtype=np.float64)
    sc = np.zeros(8, dtype=np.float64)
    from .dist import distributed_pcg, shard_range
    shard = distributed_pcg()
    pk_s, rows_s, lut_s, beta_s = pk, rows, lut, beta          # what this process solves: every kept row, or its shard of them
    if shard is not None:
        # marker-sharded solve (dist.enable_distributed_pcg): this rank's contiguous range of the kept rows; the device layer
        # all-reduces Z'p and the iteration's scalars, beta is gathered in rank (= row) order afterwards
        import torch
        import torch.distributed as tdist
        rank, world = shard
        lo, hi = shard_range(eff_m, rank, world)
        if eff_m < world:
            # the same count on every rank: all of them stop here, before any collective (a rank left alone in the first
            # all-reduce would wait for ever)
            raise RuntimeError(f"distributed rrBLUP PCG: {eff_m} kept rows cannot be dealt over {world} ranks")
        rows_all = rows if rows is not None else np.arange(m_total, dtype=np.int64)
        if _is_device_tensor(pk):
            pk_s = pk[torch.from_numpy(rows_all[lo:hi]).to(pk.device)].contiguous() if rows is not None else pk[lo:hi]
        else:
            pk_s = np.ascontiguousarray(pk[rows_all[lo:hi]])
        rows_s, lut_s, beta_s = None, np.ascontiguousarray(lut[lo:hi]), np.zeros(hi - lo, dtype=f32)
    check(lib().jx_rrblup_pcg_packed(_payload(pk_s, n_samples)[1], int(pk_s.shape[0]), n_samples, _p(rows_s), int(beta_s.shape[0]),
                                     _p(lut_s), _p(tr), n_train, _p(y), _p(te) if te.size else None, int(te.shape[0]),
                                     float(lambda_value), float(tol), int(max_iter), _p(beta_s), _p(pred_tr_full),
                                     _p(pred_te) if te.size else None, _p(sc)))
    if shard is not None:
        sizes = [shard_range(eff_m, r, world) for r in range(world)]
        width = max(b - a for a, b in sizes)
        pad = torch.zeros(width, dtype=torch.float32)
        pad[: hi - lo] = torch.from_numpy(beta_s)
        parts = [torch.zeros(width, dtype=torch.float32) for _ in range(world)]
        if tdist.get_backend() == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
            parts = [t.to(dev) for t in parts]
            tdist.all_gather(parts, pad.to(dev))
            parts = [t.cpu() for t in parts]
        else:
            tdist.all_gather(parts, pad)
        for (a, b), t in zip(sizes, parts):
            beta[a:b] = t[: b - a].numpy()
    converged, iters, rel_res, sum_ss = bool(sc[0] != 0.0), int(sc[1]), float(sc[2]), float(sc[3])
    if progress_callback is not None:
        try:
            progress_callback(iters, int(max_iter), rel_res)
        except TypeError:
            progress_callback(iters, int(max_iter))
    pve_trainvar = float("nan")
    if need_train:
        pred_train = pred_tr_full if need_all else pred_tr_full[pick]
        if compute_trainvar:
            resid = y - pred_tr_full
            if n_train > 1:
                vg = float(np.sum((pred_tr_full - pred_tr_full.mean()) ** 2) / (n_train - 1))
                ve = float(np.sum((resid - resid.mean()) ** 2) / (n_train - 1))
            else:
                vg = ve = 0.0
            den = vg + ve
            pve_trainvar = vg / den if (math.isfinite(den) and den > 0.0) else float("nan")
    else:
        pred_train = np.zeros(0, dtype=np.float64)
    k_trace_mean = sum_ss / (float(m_effective) * float(n_train)) if (n_train > 0 and m_effective > 0) else float("nan")
    pve_lambda_vc = float("nan")
    if math.isfinite(k_trace_mean) and k_trace_mean > 0.0 and m_effective > 0:
        dv = k_trace_mean + float(lambda_use) / float(m_effective)
        if math.isfinite(dv) and dv > 0.0:
            pve_lambda_vc = k_trace_mean / dv
    return (np.asarray(pred_train, dtype=np.float64).reshape(-1, 1), pred_te.reshape(-1, 1), pve_trainvar, converged,
            iters, rel_res, m_effective, pve_lambda_vc, k_trace_mean, beta)


def rrblup_exact_snp_packed(packed, n_samples, train_sample_indices, y_train, test_sample_indices=None,
                            train_pred_local_indices=None, site_keep=None, maf=None, row_flip=None, row_mean=None,
                            row_inv_sd=None, log10_lambda_low=-6.0, log10_lambda_high=6.0, reml_tol=1e-4, reml_max_iter=50,
                            sample_block=2048, std_eps=1e-12, threads=0, blas_threads=0):
    """src/stats/rrblup.rs:3157-3490.  Exact marker-space rrBLUP (the reference's route up to 15 000 markers): SNP-space
    Gram matrix of the standardised training genotypes, eigendecomposition, REML over log10 lambda by Brent on the
    spectrum, marker effects and predictions — all on the device (`jx_rrblup_exact_snp_packed`).  Returns the reference's
    tuple (pred_train (k,1), pred_test (t,1), pve_trainvar, lambda, reml, (var_g, sigma_e2), m_effective, y_mean,
    beta f32 (m), row_mean f32 (m), row_inv_sd f32 (m), eigensolver name).  `sample_block`, `threads`, `blas_threads` are
    accepted and ignored."""
    import math
    from . import stats as st
    n_samples = int(n_samples)
    if n_samples == 0:
        raise RuntimeError("n_samples must be > 0")
    if not (math.isfinite(log10_lambda_low) and math.isfinite(log10_lambda_high)):
        raise RuntimeError("rrblup_exact_snp_packed requires finite log10(lambda) bounds.")
    if not (math.isfinite(reml_tol) and reml_tol > 0.0):
        raise RuntimeError("rrblup_exact_snp_packed requires finite reml_tol > 0.")
    if int(reml_max_iter) == 0:
        raise RuntimeError("rrblup_exact_snp_packed requires reml_max_iter > 0.")
    if not (math.isfinite(std_eps) and std_eps > 0.0):
        raise RuntimeError("rrblup_exact_snp_packed requires finite std_eps > 0.")
    f32 = np.float32
    pk = _c(packed, np.uint8)
    if pk.ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp).")
    m_total = int(pk.shape[0])
    if pk.shape[1] != (n_samples + 3) // 4:
        raise RuntimeError(f"packed second dimension mismatch: got {pk.shape[1]}, expected {(n_samples + 3) // 4}")
    if maf is None:
        raise RuntimeError("rrblup_exact_snp_packed requires `maf` argument.")
    if row_flip is None:
        raise RuntimeError("rrblup_exact_snp_packed requires `row_flip` argument.")
    rows, maf_keep, flip_keep = _gs_kept_rows(m_total, maf, row_flip, site_keep)
    eff_m = int(maf_keep.shape[0])
    if eff_m == 0:
        raise RuntimeError("rrblup_exact_snp_packed received zero active markers.")
    tr, y = _gs_train_y(train_sample_indices, y_train, n_samples, 2,
                        "rrblup_exact_snp_packed requires at least two training samples.")
    n_train = int(tr.shape[0])
    te = _gs_test_idx(test_sample_indices, n_samples)
    pick = _gs_pick_idx(train_pred_local_indices, n_train)
    rm, ri, m_effective = _rrblup_row_stats(maf_keep, rows, m_total, row_mean, row_inv_sd, std_eps)
    if m_effective == 0:
        raise RuntimeError("rrblup_exact_snp_packed found zero effective markers after standardization.")
    lut = st.grm_lut_from_mean_scale(rm, ri, flip_keep)
    beta = np.zeros(eff_m, dtype=f32)
    need_train = pick is None or pick.size > 0
    pred_tr_full = np.zeros(n_train, dtype=np.float64) if need_train else None
    pred_te = np.zeros(te.shape[0], dtype=np.float64)
    sc = np.zeros(8, dtype=np.float64)
    check(lib().jx_rrblup_exact_snp_packed(_p(pk), m_total, n_samples, _p(rows), eff_m, _p(lut), _p(tr), n_train, _p(y),
                                           _p(te) if te.size else None, int(te.shape[0]), float(log10_lambda_low),
                                           float(log10_lambda_high), float(reml_tol), int(reml_max_iter), _p(beta),
                                           _p(pred_tr_full), _p(pred_te) if te.size else None, _p(sc)))
    if pick is None:
        pred_train = pred_tr_full
    elif pick.size:
        pred_train = pred_tr_full[pick]
    else:
        pred_train = np.zeros(0, dtype=np.float64)
    return (np.asarray(pred_train, dtype=np.float64).reshape(-1, 1), pred_te.reshape(-1, 1), float(sc[0]), float(sc[1]),
            float(sc[2]), (float(sc[3]), float(sc[4])), m_effective, float(sc[7]), beta, rm.astype(f32), ri.astype(f32),
            "jxgpu_eigh_f64")


def _he_solve_2x2(a00, a01, a11, b0, b1):
    """src/stats/he.rs:874-897."""
    import math
    if not all(math.isfinite(v) for v in (a00, a01, a11, b0, b1)):
        raise RuntimeError("HE 2x2 solve received non-finite inputs")
    det = a00 * a11 - a01 * a01
    det_scale = max(abs(a00) + abs(a11) + 2.0 * abs(a01), 1.0)
    det_floor = det_scale * det_scale * float(np.finfo(np.float64).eps)
    if (not math.isfinite(det)) or abs(det) <= det_floor:
        raise RuntimeError(f"HE 2x2 solve is singular/ill-conditioned: det={det}, floor={det_floor}")
    x0 = (b0 * a11 - b1 * a01) / det
    x1 = (a00 * b1 - a01 * b0) / det
    if not (math.isfinite(x0) and math.isfinite(x1)):
        raise RuntimeError("HE 2x2 solve produced non-finite outputs")
    return x0, x1


def _he_project_nnls_2x2(a00, a01, a11, b0, b1, x0u, x1u):
    """src/stats/he.rs:815-871 -> (sigma_g2, sigma_e2, projected, boundary status 0..3)."""
    import math

    def obj(x0, x1):
        r0 = a00 * x0 + a01 * x1 - b0
        r1 = a01 * x0 + a11 * x1 - b1
        return r0 * r0 + r1 * r1
    cands = [(x0u, x1u, 0)]
    c1 = a01 * a01 + a11 * a11
    if math.isfinite(c1) and c1 > 0.0:
        cands.append((0.0, max((a01 * b0 + a11 * b1) / c1, 0.0), 1))
    c0 = a00 * a00 + a01 * a01
    if math.isfinite(c0) and c0 > 0.0:
        cands.append((max((a00 * b0 + a01 * b1) / c0, 0.0), 0.0, 2))
    cands.append((0.0, 0.0, 3))
    best = (0.0, 0.0, float("inf"), 3)
    for x0, x1, stt in cands:
        if not (math.isfinite(x0) and math.isfinite(x1)) or x0 < 0.0 or x1 < 0.0:
            continue
        o = obj(x0, x1)
        if math.isfinite(o) and o < best[2]:
            best = (x0, x1, o, stt)
    if not math.isfinite(best[2]):
        return 0.0, 0.0, True, 3
    tolp = 1e-10 * max(abs(x0u), abs(x1u), 1.0)
    projected = best[3] != 0 or abs(best[0] - x0u) > tolp or abs(best[1] - x1u) > tolp
    return best[0], best[1], projected, best[3]


def he_pcg_bed(prefix, train_sample_indices, y_train, site_keep=None, trace_samples=32, trace_probe_batch=64, tol=1e-6,
               max_iter=32, block_rows=4096, std_eps=1e-12, use_train_maf=True, exact_trace_debug=False,
               exact_trace_max_n=256, threads=0, seed=20260512, packed=None, packed_n_samples=0, maf=None, row_flip=None,
               row_source_indices=None, x_cov=None, blas_threads=0, mmap_window_mb=None):
    """src/stats/he.rs:2073-2636: Haseman-Elston variance components of y = g + e, g ~ N(0, sigma_g2 K), K the standardised
    GRM of the training samples applied matrix-free on the device (`jx_he_traces_packed`: two streaming passes per
    probe), Hutchinson traces with the reference's splitmix64 probes.  Returns the reference's 12-tuple (sigma_g2,
    sigma_e2, h2, converged, iters, rel_res, m_effective, tr_k2, y_ky, y_y, lambda, tr_k2_solve).  The packed-payload
    form and the prefix form are built (the metadata-streaming form maps onto them: rows = row_source_indices)."""
    import math
    from . import stats as st
    f32 = np.float32
    if int(trace_samples) == 0:
        raise RuntimeError("trace_samples must be > 0")
    if int(trace_probe_batch) == 0:
        raise RuntimeError("trace_probe_batch must be > 0")
    _gs_check_iter_opts(max_iter, tol, std_eps)
    ext = packed is not None or int(packed_n_samples) > 0
    meta = row_source_indices is not None
    if ext and meta:
        raise RuntimeError("he_pcg_bed: provide either packed payload inputs or row_source_indices metadata streaming "
                           "inputs, not both.")
    if (not ext) and (not meta) and (maf is not None or row_flip is not None):
        raise RuntimeError("he_pcg_bed: external maf/row_flip without packed payload requires row_source_indices for "
                           "metadata streaming.")
    if meta:
        if site_keep is not None:
            raise RuntimeError("he_pcg_bed: metadata streaming path does not accept site_keep; subset rows via "
                               "row_source_indices instead.")
        if maf is None:
            raise RuntimeError("he_pcg_bed: metadata streaming path requires `maf` argument.")
        if row_flip is None:
            raise RuntimeError("he_pcg_bed: metadata streaming path requires `row_flip` argument.")
        from .bed import read_bed_payload
        pk, n_samples, _bim = read_bed_payload(str(prefix))
        rows = _c(row_source_indices, np.int64).ravel()
        if rows.size == 0:
            raise RuntimeError("row_source_indices must not be empty for metadata streaming path.")
        if rows.min() < 0:
            raise RuntimeError("row_source_indices must be non-negative.")
    else:
        pk, n_samples, maf, row_flip = _gs_payload("he_pcg_bed", prefix, packed, packed_n_samples, maf, row_flip)
    _gs_check_payload_shape(pk, n_samples)
    m_total = int(pk.shape[0])
    if meta:
        maf_keep, flip_keep = _c(maf, f32).ravel(), np.asarray(row_flip).astype(bool).ravel()
        if maf_keep.shape[0] != rows.shape[0] or flip_keep.shape[0] != rows.shape[0]:
            raise RuntimeError("metadata length mismatch between row_source_indices, maf and row_flip")
        if rows.max() >= m_total:
            raise RuntimeError("row source index out of bounds")
    else:
        rows, maf_keep, flip_keep = _gs_kept_rows(m_total, maf, row_flip, site_keep)
    eff_m = int(maf_keep.shape[0])
    tr, y = _gs_train_y(train_sample_indices, y_train, n_samples)
    n = int(tr.shape[0])
    xc, p_cov = None, 0
    if x_cov is not None:
        xa = _c(x_cov, np.float64)
        if xa.ndim != 2:
            raise RuntimeError("x_cov must be 2D (n, p_cov)")
        if xa.shape[1] == 0:
            raise RuntimeError("x_cov must have at least one column")
        if xa.shape[0] == n_samples:
            xc = np.ascontiguousarray(xa[tr])
        elif xa.shape[0] == n:
            xc = xa
        else:
            raise RuntimeError(f"x_cov rows mismatch: got {xa.shape[0]}, expected either n_samples={n_samples} or n_train={n}")
        p_cov = int(xc.shape[1])
    # row standardisation (he.rs:454-640): oriented minor frequency, or the training samples' own frequency
    if not np.all(np.isfinite(maf_keep)):
        raise RuntimeError("row_maf contains non-finite values")
    af = np.clip(maf_keep, f32(0.0), f32(1.0))
    pfr = np.where(af <= f32(0.5), af, np.where(flip_keep, f32(1.0) - af, af)).astype(f32)
    if use_train_maf:
        if rows is None:
            pk_rows = pk
        elif _is_device_tensor(pk):
            import torch
            pk_rows = pk[torch.from_numpy(rows).to(pk.device)]
        else:
            pk_rows = np.ascontiguousarray(pk[rows])
        cnt = bed_row_counts(pk_rows, n_samples, tr).astype(np.int64)
        del pk_rows
        nm = n - cnt[:, 0]
        alt = cnt[:, 1] + 2 * cnt[:, 2]
        dos = np.where(flip_keep, 2 * nm - alt, alt)
        okc = nm > 0
        pt = np.zeros_like(pfr)
        pt[okc] = dos[okc].astype(f32) / (f32(2.0) * nm[okc].astype(f32))
        pfr = np.where(okc, pt, pfr).astype(f32)
    rm, ri, m_effective = _gs_standardise(np.clip(pfr, f32(0.0), f32(1.0)), std_eps)
    if m_effective == 0:
        raise RuntimeError("No effective SNPs after std_eps filtering")
    lut = st.grm_lut_from_mean_scale(rm, ri, flip_keep)
    exact = bool(exact_trace_debug) and n <= max(int(exact_trace_max_n), 1)
    out5 = np.zeros(5, dtype=np.float64)
    check(lib().jx_he_traces_packed(_payload(pk, n_samples)[1], m_total, n_samples, _p(rows), eff_m, _p(lut), _p(tr), n, _p(y), _p(xc), p_cov,
                                    int(trace_samples), int(seed) & ((1 << 64) - 1), 1 if exact else 0,
                                    float(m_effective), _p(out5)))
    y_ky, y_y, tr_k, tr_k2, tr_p = (float(v) for v in out5)
    if not (math.isfinite(tr_k) and tr_k > 0.0):
        raise RuntimeError(f"estimated Tr(PKP) is invalid: {tr_k}. Try increasing trace_samples.")
    if not (math.isfinite(tr_k2) and tr_k2 > 0.0):
        raise RuntimeError(f"estimated Tr((PKP)^2) is invalid: {tr_k2}. Try increasing trace_samples.")
    tr_k2_solve = max(tr_k2, (tr_k * tr_k) / tr_p + tr_p * 1e-6)
    if tr_k2_solve > tr_k2 * 1.05:
        raise RuntimeError(f"Tr((PKP)^2) stochastic estimate violates PSD bound too much: raw={tr_k2}, "
                           f"adjusted={tr_k2_solve}. Increase trace_samples.")
    sg_u, se_u = _he_solve_2x2(tr_k2_solve, tr_k, tr_p, y_ky, y_y)
    sg, se, _proj, _status = _he_project_nnls_2x2(tr_k2_solve, tr_k, tr_p, y_ky, y_y, sg_u, se_u)
    r0 = tr_k2_solve * sg + tr_k * se - y_ky
    r1 = tr_k * sg + tr_p * se - y_y
    rel_res = math.sqrt(r0 * r0 + r1 * r1) / max(math.sqrt(y_ky * y_ky + y_y * y_y), 1e-20)
    converged = math.isfinite(rel_res) and rel_res <= max(float(tol), 1e-12)
    den = sg + se
    h2 = sg / den if (math.isfinite(den) and den > 0.0) else float("nan")
    lam = se / sg if (math.isfinite(sg) and sg > 0.0) else float("inf")
    return (sg, se, h2, bool(converged), 1, rel_res, min(m_effective, eff_m), tr_k2, y_ky, y_y, lam, tr_k2_solve)


# ------------------------------------------------------------------------------------------------
# Names the reference's Python layer imports unconditionally beside the hot path (python/janusx/pyBLUP/assoc.py:207-218)
# for a model this library does not replace (FastLMM, low-rank GRM): present so that the module imports, loud when called.
# ------------------------------------------------------------------------------------------------

def _out_of_scope(name, what):
    def stub(*_args, **_kwargs):
        raise RuntimeError(f"{name}: {what} is outside the mixed-model hot path this library replaces "
                           "(GRM -> eigendecomposition -> REML -> per-SNP scan); use the reference's CPU extension for it")
    stub.__name__ = name
    stub.__doc__ = f"Out of scope ({what}); raises RuntimeError."
    return stub


fastlmm_prepare_lowrank_f64 = _out_of_scope("fastlmm_prepare_lowrank_f64", "the FastLMM low-rank model")
fastlmm_assoc_from_snp_f32 = _out_of_scope("fastlmm_assoc_from_snp_f32", "the FastLMM low-rank model")
fastlmm_reml_chunk_f32 = _out_of_scope("fastlmm_reml_chunk_f32", "the FastLMM low-rank model")
fastlmm_reml_null_f32 = _out_of_scope("fastlmm_reml_null_f32", "the FastLMM low-rank model")
fastlmm_assoc_chunk_f32 = _out_of_scope("fastlmm_assoc_chunk_f32", "the FastLMM low-rank model")



# ---- randomized SVD of the packed genotypes (`jx pca -rsvd`) ------------------------------------------------------------------

def _splitmix64(z):
    """SplitMix64 finaliser on a uint64 numpy array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def rsvd_omega(seed, rows, kp):
    """The random start of both randomized SVDs: Omega (rows, kp) f64, entry (r, c) a standard normal drawn from the
    counter-based hash of (seed, r, c) alone -- u_j = (SplitMix64(s + 2 (65536 r + c) + j) >> 11 + 1) 2^-53 for j = 0, 1 with
    s = SplitMix64(seed), then Box-Muller sqrt(-2 ln u_0) cos(2 pi u_1).  Row r is the r-th SNP row of the product (kept-row index).
    The reference draws Omega from StdRng + StandardNormal (ziggurat); the PCs agree with it to within the approximation error of
    the method, not bit for bit."""
    rows, kp = int(rows), int(kp)
    if kp > 65536:
        raise RuntimeError("rsvd_omega: kp must be <= 65536")
    s = _splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0]
    ctr = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(65536) + np.arange(kp, dtype=np.uint64)[None, :])
    with np.errstate(over="ignore"):
        base = s + np.uint64(2) * ctr
        u0 = ((_splitmix64(base) >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
        u1 = ((_splitmix64(base + np.uint64(1)) >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)


def _rsvd_row_design(maf32, flip):
    """(nrows, 2) f64 (a, b) of the centred additive design: z = (flip ? 2 - g : g) - 2 maf (f32 mean, as
    `prepare_packed_block_centered_mean_scale_f32`, src/decode/decode.rs:509-532), missing calls 0."""
    mean = (np.float32(2.0) * np.asarray(maf32, dtype=np.float32)).astype(np.float64)
    flip = np.asarray(flip, dtype=bool)
    ab = np.empty((len(mean), 2), dtype=np.float64)
    ab[:, 0] = np.where(flip, 2.0 - mean, -mean)
    ab[:, 1] = np.where(flip, -1.0, 1.0)
    return ab


class _RsvdOperator:
    """Z Q and Z' W of the centred design over the rows `rows` of a Panel (`jxg_packed_mm_cols` / `jxg_packed_tmm_cols`; the
    sample-major T32 image of the rows is built once)."""

    def __init__(self, panel, rows, ab):
        import torch
        from . import pipeline as pl
        self.panel, self.dev = panel, panel.device
        self.nrows = int(ab.shape[0])
        self.rows_t = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.dev)
        self.ab = torch.from_numpy(np.ascontiguousarray(ab, dtype=np.float64)).to(self.dev)
        self.t32 = torch.empty(int(lib().jxg_t32_bytes(panel.n, self.nrows)), dtype=torch.uint8, device=self.dev)
        check(lib().jxg_p32_transpose(panel.p32.data_ptr(), panel.m, panel.n, pl._ptr(self.rows_t), self.nrows,
                                      self.t32.data_ptr(), pl._stream()))

    def zq(self, q):
        import torch
        from . import pipeline as pl
        q = q.contiguous()
        kp = int(q.shape[1])
        w = torch.empty((self.nrows, kp), dtype=torch.float64, device=self.dev)
        check(lib().jxg_packed_mm_cols(self.panel.p32.data_ptr(), self.panel.m, self.panel.n, pl._ptr(self.rows_t), self.nrows,
                                       self.ab.data_ptr(), q.data_ptr(), kp, w.data_ptr(), pl._stream()))
        return w

    def ztw(self, w):
        import torch
        from . import pipeline as pl
        w = w.contiguous()
        kp = int(w.shape[1])
        y = torch.empty((self.panel.n, kp), dtype=torch.float64, device=self.dev)
        check(lib().jxg_packed_tmm_cols(self.t32.data_ptr(), self.panel.n, self.nrows, self.ab.data_ptr(), w.data_ptr(), kp,
                                        y.data_ptr(), pl._stream()))
        return y


def _rsvd_qr(x):
    """Q of the modified Gram-Schmidt QR (`qr_normalize_mgs`, src/stats/rsvd.rs:1377-1417): Householder QR with the signs
    that make diag(R) positive; a column whose residual norm is <= 1e-12 fails like the reference."""
    import torch
    q, r = torch.linalg.qr(x, mode="reduced")
    d = torch.diagonal(r)
    bad = ~(torch.isfinite(d) & (d.abs() > 1e-12))
    if bool(bad.any()):
        j = int(torch.nonzero(bad)[0, 0])
        raise RuntimeError(f"QR normalization failed: near-dependent column at j={j}")
    return q * torch.sign(d)[None, :]


def _rsvd_lu(x, lu_eps=1e-10, cond_min_ratio=1e-8):
    """`lu_normalize_with_qr_fallback` (src/stats/rsvd.rs:1419-1546) -> (Q, used_lu)."""
    import torch
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if rows < cols:
        return _rsvd_qr(x), False
    # factor of the n x kp block alone: pivots as row swaps (no dense n x n permutation), Q = P' L by a row index
    lu, piv = torch.linalg.lu_factor(x)
    d = torch.diagonal(lu[:cols]).abs()
    ok = bool(torch.isfinite(d).all()) and bool((d > lu_eps).all())
    if ok:
        dmin, dmax = float(d.min()), float(d.max())
        ok = dmax > lu_eps and dmin > lu_eps and (dmin / dmax) >= cond_min_ratio
    if not ok:
        return _rsvd_qr(x), False
    perm = np.arange(rows)
    for jj, pj in enumerate(piv.cpu().numpy().astype(np.int64) - 1):     # LAPACK ipiv: row jj swapped with row pj, in order
        perm[jj], perm[pj] = perm[pj], perm[jj]
    l = torch.tril(lu, diagonal=-1)
    l[:cols].fill_diagonal_(1.0)
    q = torch.empty_like(l)
    q[torch.from_numpy(perm).to(x.device)] = l                      # row perm[i] of X is row i of P X = L U
    nrm = torch.linalg.vector_norm(q, dim=0)
    if not bool((torch.isfinite(nrm) & (nrm > lu_eps)).all()):
        return _rsvd_qr(x), False
    return q / nrm[None, :], True


def _rsvd_engine(op, kp, k_eff, varsum, seed, power, tol, mode):
    """Shifted subspace iteration of `rsvd_packed_subset` (mode "lu", src/stats/rsvd.rs:1589-1661) or of
    `rsvd_stream_sample_packed_impl` (mode "svd", src/stats/adamixture.rs:3590-3700) -> (eigvals f64 (k_eff), eigvecs f64
    (n, k_eff) device, power rounds done)."""
    import torch
    omega = torch.from_numpy(rsvd_omega(seed, op.nrows, kp)).to(op.dev)
    y = op.ztw(omega)
    del omega
    if mode == "lu":
        q = _rsvd_qr(y)
    else:
        q = torch.linalg.svd(y, full_matrices=False)[0]
    sk = np.zeros(kp, dtype=np.float64)
    alpha = 0.0
    q_is_qr = True
    rounds = 0
    for it in range(int(power)):
        y = op.ztw(op.zq(q)) - alpha * q
        if mode == "lu":
            if it + 1 >= power:
                q, q_is_qr = _rsvd_qr(y), True
            else:
                q, used_lu = _rsvd_lu(y)
                q_is_qr = not used_lu
            s_y = np.sort(torch.linalg.vector_norm(y, dim=0).cpu().numpy())[::-1]
        else:
            u, s, _ = torch.linalg.svd(y, full_matrices=False)
            q = u
            s_y = s.cpu().numpy()
        rounds = it + 1
        if it > 0:
            sk_now = s_y[:k_eff] + alpha
            rel = np.abs(sk_now - sk[:k_eff]) / np.maximum(sk_now, 1e-12)
            sk[:k_eff] = sk_now
            if float(rel.max()) < tol:
                if mode == "lu" and not q_is_qr:
                    q, q_is_qr = _rsvd_qr(q), True
                break
        else:
            sk[:kp] = s_y[:kp] + alpha
        tail = float(s_y[kp - 1])
        if alpha < tail:
            alpha = 0.5 * (alpha + tail)
    if mode == "lu" and not q_is_qr:
        q = _rsvd_qr(q)
    w = op.zq(q)
    gram = (w.T @ w).cpu().numpy()
    ev, v = np.linalg.eigh(0.5 * (gram + gram.T))
    order = np.argsort(-ev, kind="stable")
    ev, v = np.maximum(ev[order], 1e-12), v[:, order]
    eigvals = ev[:k_eff] / float(varsum)
    eigvecs = q @ torch.from_numpy(np.ascontiguousarray(v[:, :k_eff])).to(op.dev)
    return eigvals, eigvecs, rounds


def rsvd_packed_subset(packed, n_samples, k, sample_indices=None, seed=42, power=5, tol=1e-1):
    """src/stats/rsvd.rs:1548-1782: randomized SVD of the centred additive design of a packed payload (m, ceil(n / 4)) over the
    selected samples -> (eigvals f32 (k_eff), eigvecs f32 (n, k_eff), row_maf f32 (m), row_flip bool (m)).  Row statistics over
    all m rows without QC (`packed_subset_row_stats`, :208-258); kp = min(max(k_eff + 10, 20), m, n); the two products per
    round run on the device (`jxg_packed_mm_cols` / `jxg_packed_tmm_cols`), the small dense steps in torch.  The start block is
    `rsvd_omega` (not the reference's StdRng stream).  `packed` may be a torch CUDA uint8 tensor (used in place)."""
    return _rsvd_packed_subset(packed, n_samples, k, sample_indices, seed, power, tol)[:4]


def _rsvd_packed_subset(packed, n_samples, k, sample_indices, seed, power, tol):
    import math
    k, n_samples, power = int(k), int(n_samples), int(power)
    if k <= 0:
        raise RuntimeError("k must be > 0")
    if n_samples <= 0:
        raise RuntimeError("n_samples must be > 0")
    tol = float(np.float32(tol))
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be positive and finite")
    if sample_indices is not None:
        idx = _c(sample_indices, np.int64).ravel()
        if idx.size == 0:
            raise RuntimeError("sample_indices must not be empty")
        if idx.min() < 0 or idx.max() >= n_samples:
            raise RuntimeError("sample_indices out of range")
    panel = _panel(packed, n_samples, sample_indices)
    n, m = panel.n, panel.m
    c = panel.counts().astype(np.int64)
    nm = n - c[:, 0]
    alt = c[:, 1] + 2 * c[:, 2]
    has = nm > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(has, alt / (2.0 * np.maximum(nm, 1)), 0.0)
    flip = has & (p > 0.5)
    pmin = np.where(flip, 1.0 - p, p)
    maf32 = pmin.astype(np.float32)
    varsum = float(np.sum(np.where(has, 2.0 * pmin * (1.0 - pmin), 0.0)))
    if not (math.isfinite(varsum) and varsum > 0.0):
        raise RuntimeError("invalid scaling denominator in packed subset RSVD")
    kp = min(max(min(k, n) + 10, 20), max(m, 1), max(n, 1))
    k_eff = min(k, n, kp)
    op = _RsvdOperator(panel, None, _rsvd_row_design(maf32, flip))
    ev, vec, rounds = _rsvd_engine(op, kp, k_eff, varsum, seed, power, tol, "lu")
    return (ev.astype(np.float32), vec.to(dtype=__import__("torch").float32).cpu().numpy(), maf32, flip.astype(bool), rounds)


def admx_rsvd_stream_sample(genotype_path, k, seed=42, power=5, tol=1e-1, snps_only=True, maf=0.02, missing_rate=0.05,
                            delimiter=None, mmap_window_mb=0, memory_mb=0):
    """src/stats/adamixture.rs:2563-2700 with the packed path `rsvd_stream_sample_packed_impl` (:3527-3720): randomized SVD of the
    centred additive design of a PLINK prefix after QC (`maf` on the minor allele, `missing_rate`, `snps_only`) ->
    (eigvals f32 (k_eff), eigvecs f32 (n, k_eff), total_variance = trace(K) of the method-1 GRM over the kept SNPs).
    kp = max(k_eff + 6, 12) capped by min(m, n) (`admx_rsvd_kp`, :621-640); a thin SVD of Y in every round.  Only a PLINK
    prefix is accepted.  `delimiter`, `mmap_window_mb` and `memory_mb` are accepted and unused."""
    return _admx_rsvd(genotype_path, k, seed, power, tol, snps_only, maf, missing_rate)[:3]


def _admx_kept_rows(genotype_path, snps_only, maf, missing_rate, payload, who, what, before_panel=None):
    """The kept rows of the ADMIXTURE / FastPop paths (QC on the minor allele, `missing_rate`, `snps_only`) ->
    (Panel, counts, rows int64, row_flip bool, row_freq f32 minor-allele frequency, Bim, PLINK prefix or None).
    `before_panel(packed, n)`, when given, is called before the P32 image is built (a memory check)."""
    from . import stats as st
    from .bed import read_bed_payload, snps_only_mask
    path = None
    if payload is None:
        path = str(genotype_path)
        low = path.lower()
        if low.endswith((".vcf", ".vcf.gz", ".hmp", ".hmp.gz", ".txt", ".tsv", ".csv", ".npy")):
            raise RuntimeError(f"{who}: only a PLINK prefix is accepted on this build (got {path})")
        if low.endswith((".bed", ".bim", ".fam")):
            path = path[:-4]
        packed, n_fam, bim = read_bed_payload(path)
    else:
        packed, n_fam, bim = payload
    if before_panel is not None:
        before_panel(packed, n_fam)
    panel = _panel(packed, n_fam)
    n = panel.n
    c = panel.counts()
    keep, _miss, af, _std = st.packed_prep_row_stats(c, n, float(maf), float(missing_rate), 0.0)
    if snps_only:
        keep &= snps_only_mask(bim)
    rows = np.nonzero(keep)[0]
    if rows.size == 0:
        raise RuntimeError(f"no SNPs passed filtering in {what}")
    flip = af[rows] > np.float32(0.5)
    freq = np.where(flip, np.float32(1.0) - af[rows], af[rows]).astype(np.float32)
    return panel, c, rows, flip, freq, bim, path


def _admx_rsvd(genotype_path, k, seed, power, tol, snps_only, maf, missing_rate, payload=None):
    """`payload`: (packed (m, bps) numpy or torch CUDA uint8, n_samples, bim) already read (the CLI's staged payload)."""
    import math
    import torch
    k, power = int(k), int(power)
    if k <= 0:
        raise RuntimeError("k must be > 0")
    if not (0.0 <= float(np.float32(maf)) <= 0.5):
        raise RuntimeError("maf must be within [0, 0.5]")
    if not (0.0 <= float(np.float32(missing_rate)) <= 1.0):
        raise RuntimeError("missing_rate must be within [0, 1]")
    tol = float(np.float32(tol))
    if not (math.isfinite(tol) and tol > 0.0):
        raise RuntimeError("tol must be positive and finite")
    panel, c, rows, flip, freq, _bim, _prefix = _admx_kept_rows(genotype_path, snps_only, maf, missing_rate, payload,
                                                                "admx_rsvd_stream_sample", "streaming RSVD")
    n = panel.n
    f64 = freq.astype(np.float64)
    varsum = float(np.sum(2.0 * f64 * (1.0 - f64)))
    if not (math.isfinite(varsum) and varsum > 0.0):
        raise RuntimeError("invalid scaling denominator in streaming RSVD (varsum <= 0)")
    # trace(K) = sum over kept rows and called genotypes of z^2, from the genotype counts (f64)
    cr = c[rows].astype(np.float64)
    n0 = (n - cr[:, 0]) - cr[:, 1] - cr[:, 2]
    mean = (np.float32(2.0) * freq).astype(np.float64)
    g0, g1, g2 = np.where(flip, 2.0, 0.0) - mean, 1.0 - mean, np.where(flip, 0.0, 2.0) - mean
    total_variance = float(np.sum(n0 * g0 * g0 + cr[:, 1] * g1 * g1 + cr[:, 2] * g2 * g2)) / varsum
    if not (math.isfinite(total_variance) and total_variance > 0.0):
        raise RuntimeError("invalid total variance in streaming RSVD (trace(K) <= 0)")
    m = int(rows.size)
    kp = min(max(min(k, n) + 6, 12), max(min(m, n), 1))
    k_eff = min(k, n, kp)
    op = _RsvdOperator(panel, rows.astype(np.int32), _rsvd_row_design(freq, flip))
    ev, vec, rounds = _rsvd_engine(op, kp, k_eff, varsum, seed, power, tol, "svd")
    return ev.astype(np.float32), vec.to(torch.float32).cpu().numpy(), float(total_variance), rounds


# ---- ADMIXTURE / FastPop (`jx adamixture`): ALS start and Adam-EM on the packed genotypes -------------------------------------

ADMX_MAX_K = 64
_ADMX_EPS = 1e-5                       # clip32 (src/stats/adamixture.rs:50-60)


def _admx_clip(x):
    return x.clamp(_ADMX_EPS, 1.0 - _ADMX_EPS)


def _admx_map_q(q):
    """`map_q_rows_inplace_f32` (src/stats/adamixture.rs:4120-4137) on a torch tensor: clip, then rows / row sum; a non-finite
    or non-positive sum gives 1/K."""
    import torch
    q = _admx_clip(q)
    s = q.sum(dim=1, keepdim=True)
    bad = ~(torch.isfinite(s) & (s > 0))
    return torch.where(bad, torch.full_like(q, 1.0 / max(int(q.shape[1]), 1)), q / torch.where(bad, torch.ones_like(s), s))


def _stdrng_words(seed, count):
    """The first `count` u32 words of `_StdRngU32(seed)`, all ChaCha12 blocks at once (numpy, wrapping u32 arithmetic)."""
    key = _StdRngU32(seed).key
    nb = (int(count) + 15) // 16
    ctr = np.arange(nb, dtype=np.uint64)
    st = [np.full(nb, v, dtype=np.uint32) for v in (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)]
    st += [np.full(nb, v, dtype=np.uint32) for v in key]
    st += [(ctr & np.uint64(0xffffffff)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32),
           np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32)]
    x = [a.copy() for a in st]

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)
    with np.errstate(over="ignore"):
        for _ in range(6):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        out = np.stack([x[i] + st[i] for i in range(16)], axis=1).reshape(-1)
    return out[: int(count)]


def adam_seed_init(m, n, k, seed):
    """`adam_seed_init_rust` (src/stats/adamixture.rs:4274-4286): StdRng `random::<f32>()` ((u32 >> 8) 2^-24), P (m, k) first,
    then Q (n, k), clipped; Q rows mapped by `map_q` -> (P, Q) f32 numpy."""
    import torch
    total = (int(m) + int(n)) * int(k)
    u = _stdrng_words(seed, total)
    v = ((u >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    v = np.clip(v, np.float32(_ADMX_EPS), np.float32(1.0 - _ADMX_EPS)).astype(np.float32)
    p = v[: int(m) * int(k)].reshape(int(m), int(k)).copy()
    q = _admx_map_q(torch.from_numpy(v[int(m) * int(k):].reshape(int(n), int(k)).copy())).numpy()
    return p, q


def _admx_pinv(mat):
    """`symmetric_pinv_f32` (src/stats/adamixture.rs:3985-4014): eigendecomposition in f64, eigenvalues with |l| <= max(1e-12
    max|l|, 1e-12) dropped, result in the dtype of `mat`."""
    import torch
    m64 = mat.to(torch.float64)
    ev, vec = torch.linalg.eigh(0.5 * (m64 + m64.T))
    cutoff = max(float(ev.abs().max()) * 1e-12, 1e-12) if ev.numel() else 1e-12
    keep = torch.isfinite(ev) & (ev.abs() > cutoff)
    inv_ev = torch.where(keep, 1.0 / torch.where(keep, ev, torch.ones_like(ev)), torch.zeros_like(ev))
    return ((vec * inv_ev[None, :]) @ vec.T).to(mat.dtype)


def _admx_right_pinv(x, reg):
    """`right_multiply_pinv_f32` (:4104-4111): X (X'X + reg I)^+."""
    import torch
    k = int(x.shape[1])
    gram = x.T @ x + float(reg) * torch.eye(k, dtype=x.dtype, device=x.device)
    return x @ _admx_pinv(gram)


def _admx_q_from_p(z, v, row_freq, i_mat):
    """`compute_q_from_p_projection_f32` (:4232-4251)."""
    q = v @ (z.T @ i_mat)
    fsum = (i_mat * row_freq[:, None]).sum(dim=0)
    return _admx_map_q(0.5 * q + fsum[None, :])


def _admx_p_from_q(z, v, row_freq, i_mat):
    """`compute_p_from_q_projection_f32` (:4253-4272)."""
    p = z @ (v.T @ i_mat)
    isum = i_mat.sum(dim=0)
    return _admx_clip(0.5 * p + row_freq[:, None] * isum[None, :])


def _admx_rmse(a, b):
    d = (a - b).to(__import__("torch").float64)
    return float((d * d).mean()) ** 0.5 if d.numel() else 0.0


def admx_als_init(z, v, row_freq, p0, max_iter=1000, tol=1e-5, reg=1e-5, loglik=None):
    """`als_init_packed_session_impl` (src/stats/adamixture.rs:4288-4389) on torch tensors of any device and dtype: z = Z v
    (m, k), v (n, k), row_freq (m), the seed P0 (m, k).  Q and P are projected in turn; the loop stops on RMSE(Q, Q_prev) < tol
    and, once max |corr| of P's columns has exceeded 0.95, after 20 rounds without a new best RMSE, rolling back to the best
    state.  -> (P, Q, init_ll = loglik(P, Q) or NaN, rounds)."""
    import torch
    dt = z.dtype
    row_freq = row_freq.to(dt)
    p = p0.to(dt)
    k = int(p.shape[1])
    q = _admx_q_from_p(z, v, row_freq, _admx_right_pinv(p, reg))
    q_prev = q.clone()
    rmse_best = float("inf")
    stall = 0
    high_corr = False
    p_best = q_best = None
    last = 0
    eye = torch.eye(k, dtype=dt, device=p.device)
    for it in range(int(max_iter)):
        last = it + 1
        p = _admx_p_from_q(z, v, row_freq, _admx_right_pinv(q, reg))
        p = _admx_clip(p)
        g_p = p.T @ p
        q = _admx_q_from_p(z, v, row_freq, p @ _admx_pinv(g_p + float(reg) * eye))
        err = _admx_rmse(q, q_prev)
        if not high_corr and k > 1:
            sd = torch.sqrt(torch.clamp(torch.diagonal(g_p), min=1e-12))
            corr = (g_p / torch.clamp(sd[:, None] * sd[None, :], min=1e-10)).abs()
            corr.fill_diagonal_(0.0)
            if float(corr.max()) > 0.95:
                high_corr = True
        if high_corr:
            if err < rmse_best:
                rmse_best, p_best, q_best, stall = err, p.clone(), q.clone(), 0
            else:
                stall += 1
            if stall >= 20:
                if p_best is not None:
                    p, q = p_best, q_best
                break
        if err < tol:
            break
        q_prev = q.clone()
    init_ll = float(loglik(p, q)) if loglik is not None else float("nan")
    return p, q, init_ll, last


class _AdmxEngine:
    """The device side of one panel: P32 image, kept rows and flips, the per-sample called counts (2 x, computed once), the
    work buffer of the EM pass (per K) and the three calls `jxg_admx_called` / `jxg_admx_em_step` / `jxg_admx_loglik`."""

    def __init__(self, panel, rows, flip):
        import torch
        from . import pipeline as pl
        self.panel, self.dev = panel, panel.device
        self.m = int(len(flip))
        self.n = panel.n
        self.rows_t = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.dev)
        self.flip_t = torch.from_numpy(np.ascontiguousarray(flip, dtype=np.uint8)).to(self.dev)
        self.work, self.work_k = None, None
        self._ensure_work(1)
        self.qb = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        check(lib().jxg_admx_called(panel.p32.data_ptr(), panel.m, self.n, pl._ptr(self.rows_t), self.m, self.work.data_ptr(),
                                    int(self.work.numel()), self.qb.data_ptr(), pl._stream()))

    def _ensure_work(self, k):
        import torch
        k = int(k)
        if not 1 <= k <= ADMX_MAX_K:
            raise RuntimeError(f"K must be within [1, {ADMX_MAX_K}] on this build (got K={k})")
        if k > self.n:
            raise RuntimeError(f"K={k} exceeds the number of samples ({self.n})")
        if self.work_k == k:
            return
        nb = int(lib().jxg_admx_work_bytes(self.m, self.n, k))
        self.work = None
        _admx_need_hbm(nb + 16 * (self.m + self.n) * k, f"the EM partial sums of K={k}")
        self.work = torch.empty(max(nb, 4 * self.n), dtype=torch.uint8, device=self.dev)
        self.work_k = k

    def _pq(self, p, q):
        k = int(p.shape[1])
        if tuple(p.shape) != (self.m, k) or tuple(q.shape) != (self.n, k):
            raise RuntimeError(f"shape mismatch: expected P ({self.m}, K) and Q ({self.n}, K), got P {tuple(p.shape)}, "
                               f"Q {tuple(q.shape)}")
        self._ensure_work(k)
        return k

    def em_step(self, p, q):
        """Plain EM step -> (P_em, Q_em); P and Q unchanged."""
        import torch
        from . import pipeline as pl
        k = self._pq(p, q)
        p_em, q_em = torch.empty_like(p), torch.empty_like(q)
        check(lib().jxg_admx_em_step(self.panel.p32.data_ptr(), self.panel.m, self.n, pl._ptr(self.rows_t), self.m,
                                     self.flip_t.data_ptr(), k, p.data_ptr(), q.data_ptr(), self.qb.data_ptr(),
                                     self.work.data_ptr(), int(self.work.numel()), p_em.data_ptr(), q_em.data_ptr(),
                                     None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, pl._stream()))
        return p_em, q_em

    def adam_step(self, p, q, mom, lr, beta1, beta2, eps, m_scale, v_scale):
        """One Adam-EM iteration in place on P, Q and the moments mom = (m_P, v_P, m_Q, v_Q)."""
        from . import pipeline as pl
        k = self._pq(p, q)
        mp, vp, mq, vq = mom
        check(lib().jxg_admx_em_step(self.panel.p32.data_ptr(), self.panel.m, self.n, pl._ptr(self.rows_t), self.m,
                                     self.flip_t.data_ptr(), k, p.data_ptr(), q.data_ptr(), self.qb.data_ptr(),
                                     self.work.data_ptr(), int(self.work.numel()), None, None, mp.data_ptr(), vp.data_ptr(),
                                     mq.data_ptr(), vq.data_ptr(), float(lr), float(beta1), float(beta2), float(eps),
                                     float(m_scale), float(v_scale), pl._stream()))

    def loglik(self, p, q):
        import torch
        from . import pipeline as pl
        k = self._pq(p, q)
        out = torch.empty(1, dtype=torch.float64, device=self.dev)
        check(lib().jxg_admx_loglik(self.panel.p32.data_ptr(), self.panel.m, self.n, pl._ptr(self.rows_t), self.m,
                                    self.flip_t.data_ptr(), k, p.data_ptr(), q.data_ptr(), self.work.data_ptr(),
                                    int(self.work.numel()), out.data_ptr(), pl._stream()))
        return float(out.item())


def _admx_need_hbm(nbytes, what):
    """Fail with a message, rather than partway through, when the device lacks `nbytes` of free memory."""
    import torch
    free, _total = torch.cuda.mem_get_info()
    if int(nbytes) > int(free):
        raise RuntimeError(f"not enough free device memory for {what}: need {int(nbytes) / 2**30:.2f} GiB, "
                           f"{int(free) / 2**30:.2f} GiB free")


def _admx_adam_loop(eng, p, q, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay, min_lr, trace=None):
    """`adam_optimize_packed_inplace_impl` (src/stats/adamixture.rs:5608-5898): Adam on the EM direction with bias correction,
    the log-likelihood after every `check_every`-th iteration, stop when |ll - ll_best| < 0.1, lr x lr_decay (floor min_lr) on a
    non-improvement and stop after two in a row; the best state is kept.  The scalars follow the reference's f32 arithmetic.
    -> (P_best, Q_best, ll_best, last_iter); `trace`, a list, receives (iteration, ll) of every check."""
    import math
    import torch
    f32 = np.float32
    lr_cur, b1, b2 = f32(lr), f32(beta1), f32(beta2)
    b1p, b2p = f32(1.0), f32(1.0)
    mom = tuple(torch.zeros_like(x) for x in (p, p, q, q))
    p_best = q_best = None
    ll_best = float("-inf")
    no_improve = 0
    last = 0
    check_every = max(int(check_every), 1)
    for it in range(int(max_iter)):
        last = it + 1
        b1p, b2p = f32(b1p * b1), f32(b2p * b2)
        ms = f32(1.0) if abs(f32(1.0) - b1p) < f32(1e-8) else f32(f32(1.0) / f32(f32(1.0) - b1p))
        vs = f32(1.0) if abs(f32(1.0) - b2p) < f32(1e-8) else f32(f32(1.0) / f32(f32(1.0) - b2p))
        eng.adam_step(p, q, mom, lr_cur, b1, b2, f32(epsilon), ms, vs)
        if last % check_every != 0:
            continue
        ll = eng.loglik(p, q)
        if trace is not None:
            trace.append((last, ll))
        if abs(ll - ll_best) < 0.1:
            break
        if ll > ll_best:
            ll_best, p_best, q_best, no_improve = ll, p.clone(), q.clone(), 0
        else:
            no_improve += 1
            lr_cur = max(f32(lr_cur * f32(lr_decay)), f32(min_lr))
            if no_improve >= 2:
                break
    if not math.isfinite(ll_best):
        ll_best, p_best, q_best = eng.loglik(p, q), p, q
    return p_best, q_best, float(ll_best), last


def _admx_check_qc(maf, missing_rate):
    if not (0.0 <= float(np.float32(maf)) <= 0.5):
        raise RuntimeError("maf must be within [0, 0.5]")
    if not (0.0 <= float(np.float32(missing_rate)) <= 1.0):
        raise RuntimeError("missing_rate must be within [0, 1]")


def _admx_p32_check(packed, n):
    m = int(packed.shape[0])
    _admx_need_hbm(((int(n) + 127) // 128) * 128 // 4 * m + (0 if _is_device_tensor(packed) else int(packed.nbytes)),
                   f"the genotype image ({m} SNPs x {int(n)} samples)")


class _AdmxFit:
    """What a training session and a CV fold backend share: a P32 image with the rows `_op_rows` of it (None = all, in order),
    the flips and frequencies of those rows, the engine of the EM passes and, on first use, the operator of the randomized SVD."""

    @property
    def n_samples(self):
        return int(self._panel.n)

    @property
    def n_snps(self):
        return int(self._rows.size)

    def row_freq(self):
        return self._freq.copy()

    def row_flip(self):
        return self._flip.copy()

    def kept_rows(self):
        return self._rows.copy()

    def write_site_file(self, path):
        """`write_p_site_from_backend_impl` (src/stats/adamixture.rs:1698-1760): chrom, pos, ref, alt of the kept BIM rows, tab
        separated, alleles swapped on flipped rows."""
        b = self._bim
        with open(path, "w") as fh:
            for r, f in zip(self._rows.tolist(), self._flip.tolist()):
                ref, alt = (b.a1[r], b.a0[r]) if f else (b.a0[r], b.a1[r])
                fh.write(f"{b.chrom[r]}\t{b.pos[r]}\t{ref}\t{alt}\n")

    def _operator(self):
        if self._op is None:
            from . import pipeline as pl
            _admx_need_hbm(int(lib().jxg_t32_bytes(self._panel.n, self.n_snps)), "the sample-major image of the randomized SVD")
            self._op = _RsvdOperator(self._panel, self._op_rows, _rsvd_row_design(self._freq, self._flip))
            del pl
        return self._op

    def zq(self, v):
        """z = Z v of the centred design over the kept rows (`multiply_a_omega_packed_checked_impl`) -> (m, k) f32 tensor."""
        import torch
        return self._operator().zq(v.to(torch.float64)).to(torch.float32)

    def fit_k(self, k, seed, solver, power, tol, max_als, reg_als, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay,
              min_lr):
        """`fit_admx_bed_training_session_impl` (src/stats/adamixture.rs:4391-4484) -> (P f32 (m, k), Q f32 (n, k), ll_final,
        adam iterations, init_ll, ALS rounds)."""
        p, q, ll, it, init_ll, als_it = self._fit(k, seed, solver, power, tol, max_als, reg_als, lr, beta1, beta2, epsilon,
                                                  max_iter, check_every, lr_decay, min_lr)
        return p.cpu().numpy(), q.cpu().numpy(), ll, it, init_ll, als_it

    def _fit(self, k, seed, solver, power, tol, max_als, reg_als, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay,
             min_lr, trace=None):
        import math
        import torch
        k = int(k)
        m, n = self.n_snps, self.n_samples
        if m == 0 or n == 0 or k == 0:
            raise RuntimeError("invalid empty input for BED training session")
        if k > ADMX_MAX_K:
            raise RuntimeError(f"K must be within [1, {ADMX_MAX_K}] on this build (got K={k})")
        dev = self._panel.device
        mode = "adam" if str(solver).strip().lower() == "adam" else "adam-em"
        if mode == "adam":
            if k > n:
                raise RuntimeError(f"K={k} exceeds the number of samples ({n})")
            p0, q0 = adam_seed_init(m, n, k, seed)
            p, q = torch.from_numpy(p0).to(dev), torch.from_numpy(q0).to(dev)
            init_ll, als_it = float("nan"), 0
        else:
            op = self._operator()
            f64 = self._freq.astype(np.float64)
            varsum = float(np.sum(2.0 * f64 * (1.0 - f64)))
            if not (math.isfinite(varsum) and varsum > 0.0):
                raise RuntimeError("invalid scaling denominator in streaming RSVD (varsum <= 0)")
            kp = min(max(min(k, n) + 6, 12), max(min(m, n), 1))
            k_eff = min(k, n, kp)
            if k_eff != k:
                raise RuntimeError(f"K={k} exceeds sample-side RSVD rank {k_eff}; reduce K or use dense fallback")
            _ev, vec, _rounds = _rsvd_engine(op, kp, k_eff, varsum, seed, int(power), float(np.float32(tol)), "svd")
            v = vec.to(torch.float32)
            z = op.zq(v.to(torch.float64)).to(torch.float32)
            p0 = adam_seed_init(m, 0, k, seed)[0]              # P comes first in the stream: Q's draws are not needed
            p, q, init_ll, als_it = admx_als_init(z, v, self._freq_t, torch.from_numpy(p0).to(dev), int(max_als),
                                                  float(np.float32(tol)), float(np.float32(reg_als)),
                                                  loglik=lambda pp, qq: self._eng.loglik(pp.contiguous(), qq.contiguous()))
            p, q = p.contiguous(), q.contiguous()
        p, q, ll, it = _admx_adam_loop(self._eng, p, q, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay, min_lr,
                                       trace)
        return p, q, ll, it, init_ll, als_it


class AdmxBedTrainingSession(_AdmxFit):
    """`AdmxBedTrainingSession` (src/stats/adamixture.rs:1526, 5950-6140): the kept rows of a PLINK prefix (QC on the minor
    allele, `missing_rate`, `snps_only`) staged once as a P32 image in HBM with their flips and the per-sample called counts;
    every `fit_k` of a K scan reuses them.  `memory_mb` is accepted and unused."""

    def __init__(self, genotype_path, snps_only=True, maf=0.02, missing_rate=0.05, memory_mb=0, payload=None):
        import torch
        _admx_check_qc(maf, missing_rate)
        self.snps_only, self.maf, self.missing_rate = bool(snps_only), float(maf), float(missing_rate)
        panel, _c, rows, flip, freq, bim, prefix = _admx_kept_rows(genotype_path, snps_only, maf, missing_rate, payload,
                                                                   "AdmxBedTrainingSession", "BED training session",
                                                                   before_panel=_admx_p32_check)
        self.prefix = prefix if prefix is not None else str(genotype_path)
        self._panel, self._rows, self._flip, self._freq, self._bim = panel, rows, flip, freq, bim
        self._eng = _AdmxEngine(panel, rows, flip)
        self._freq_t = torch.from_numpy(freq).to(panel.device)
        self._op, self._op_rows = None, rows.astype(np.int32)

    def __repr__(self):
        return (f"AdmxBedTrainingSession(prefix='{self.prefix}', n_snps={self.n_snps}, n_samples={self.n_samples}, "
                f"snps_only={self.snps_only}, maf={self.maf}, missing_rate={self.missing_rate})")

    def cv_observed_fold_counts(self, folds, seed):
        """`cv_observed_fold_counts_packed_impl` (src/stats/adamixture.rs:3056-3128) -> (observed, int64 (folds)): the called
        genotypes of the kept rows per fold of `admx_cv_fold_ids`."""
        import torch
        from . import pipeline as pl
        folds = _admx_cv_check(folds)
        eng = self._eng
        counts = torch.empty(folds, dtype=torch.int64, device=eng.dev)
        check(lib().jxg_admx_cv_fold_counts(eng.panel.p32.data_ptr(), eng.panel.m, eng.n, pl._ptr(eng.rows_t), eng.m, folds,
                                            _admx_cv_seed(seed), counts.data_ptr(), pl._stream()))
        counts = counts.cpu().numpy()
        return int(counts.sum()), counts

    def make_cv_fold_backend(self, fold_id, folds, seed):
        """`make_cv_fold_backend` (src/stats/adamixture.rs:6262-6284) -> `AdmxBedFoldBackend`."""
        return AdmxBedFoldBackend(self, fold_id, folds, seed)


ADMX_CV_MAX_FOLDS = 256                # JXG_ADMX_CV_MAX_FOLDS: the fold histogram of a workgroup lives in LDS
_ADMX_CV_WORK_BYTES = 32768            # JXG_ADMX_CV_WORK_BYTES
_ADMX_CV_GOLDEN = 0x9E3779B97F4A7C15
_U64 = (1 << 64) - 1


def _admx_cv_seed(seed):
    return int(seed) & _U64


def _admx_cv_check(folds, fold_id=None):
    folds = int(folds)
    if folds < 2:
        raise RuntimeError(f"CVerror requires folds >= 2, got {folds}.")
    if folds > ADMX_CV_MAX_FOLDS:
        raise RuntimeError(f"CVerror folds must be at most {ADMX_CV_MAX_FOLDS} on this build (got {folds})")
    if fold_id is not None and not 0 <= int(fold_id) < folds:
        raise RuntimeError(f"fold_id must be within [0, {folds}), got {int(fold_id)}")
    return folds


def admx_cv_fold_ids(flat_idx, folds, seed):
    """`cv_fold_id` (src/stats/adamixture.rs:1641-1653; python/janusx/adamixture/core.py:208-223) on the host: the fold of the
    genotypes with the flat indices kept_row * n_samples + sample, a SplitMix64 step of flat ^ (seed ^ golden) in wrapping
    u64 arithmetic (the seed taken mod 2^64), mod folds -> int64 array of the shape of `flat_idx`."""
    x = np.asarray(flat_idx).astype(np.uint64) ^ np.uint64(_admx_cv_seed(seed) ^ _ADMX_CV_GOLDEN)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x % np.uint64(max(int(folds), 1))).astype(np.int64)


class _AdmxImage:
    """A P32 image that is already in HBM, with the four attributes the engine and the RSVD operator read of a Panel."""

    def __init__(self, p32, m, n):
        self.p32, self.m, self.n, self.device = p32, int(m), int(n), p32.device


class AdmxBedFoldBackend(_AdmxFit):
    """`AdmxBedFoldBackend` (src/stats/adamixture.rs:6409-6640): one CV fold of a training session.  The reference masks the
    fold's calls in every pass over the shared payload; here the kept rows are copied once into a compact P32 image with those
    calls turned missing (`jxg_admx_cv_fold_image`), and the fold's fit is the session's fit on that image: training-only
    likelihood and called counts, `row_freq()` = the training frequencies in the SVD design, the full session's flips.
    `holdout_nll_f32` scores the held-out calls on the session's own image."""

    def __init__(self, session, fold_id, folds, seed):
        import torch
        from . import pipeline as pl
        folds = _admx_cv_check(folds, fold_id)
        full = session._eng
        self.prefix, self.snps_only, self.maf, self.missing_rate = session.prefix, session.snps_only, session.maf, session.missing_rate
        self.fold_id, self.folds, self.cv_seed = int(fold_id), folds, _admx_cv_seed(seed)
        self._full, self._rows, self._flip, self._bim = full, session._rows, session._flip, session._bim
        nt = (full.n + 127) // 128
        _admx_need_hbm(32 * nt * full.m + 12 * full.m, f"the image of CV fold {self.fold_id + 1}/{folds} ({full.m} SNPs x "
                                                       f"{full.n} samples)")
        p32 = torch.empty((nt, full.m, 32), dtype=torch.uint8, device=full.dev)
        stats = torch.empty((full.m, 3), dtype=torch.int32, device=full.dev)
        check(lib().jxg_admx_cv_fold_image(full.panel.p32.data_ptr(), full.panel.m, full.n, pl._ptr(full.rows_t), full.m,
                                           full.flip_t.data_ptr(), folds, self.cv_seed, self.fold_id, p32.data_ptr(),
                                           stats.data_ptr(), pl._stream()))
        self._row_stats = stats.cpu().numpy()
        train = self._row_stats[:, 0].astype(np.float64)
        # `cv_training_row_freq_packed_impl` (:3198-3202): the f64 quotient rounded to f32, 0 for a row without training calls
        self._freq = np.where(train > 0, self._row_stats[:, 2] / (2.0 * np.maximum(train, 1.0)), 0.0).astype(np.float32)
        self.train_observed = int(self._row_stats[:, 0].sum(dtype=np.int64))
        self.holdout_observed = int(self._row_stats[:, 1].sum(dtype=np.int64))
        self._panel = _AdmxImage(p32, full.m, full.n)
        self._eng = _AdmxEngine(self._panel, None, self._flip)
        self._freq_t = torch.from_numpy(self._freq).to(full.dev)
        self._op, self._op_rows = None, None
        self._work = torch.empty(_ADMX_CV_WORK_BYTES, dtype=torch.uint8, device=full.dev)

    def close(self):
        """Release the fold image and everything built on it."""
        self._panel = self._eng = self._op = self._freq_t = self._work = None

    def __repr__(self):
        return (f"AdmxBedFoldBackend(prefix='{self.prefix}', n_snps={self.n_snps}, n_samples={self._full.n}, "
                f"fold={self.fold_id + 1}/{self.folds}, cv_seed={self.cv_seed})")

    def loglikelihood_f32(self, p, q):
        """The training-only log-likelihood (`loglikelihood_packed_train_fold_f32_impl`, :4486-4549)."""
        pt, qt = _admx_pq_host(self._eng, p, q)
        return self._eng.loglik(pt, qt)

    def _holdout(self, p, q):
        """-> (ll_sum, n_eval) of device tensors P (m, K), Q (n, K)."""
        import torch
        from . import pipeline as pl
        full = self._full
        k = full._pq(p, q)
        out_ll = torch.empty(1, dtype=torch.float64, device=full.dev)
        out_n = torch.empty(1, dtype=torch.int64, device=full.dev)
        check(lib().jxg_admx_cv_holdout_nll(full.panel.p32.data_ptr(), full.panel.m, full.n, pl._ptr(full.rows_t), full.m,
                                            full.flip_t.data_ptr(), self.folds, self.cv_seed, self.fold_id, k, p.data_ptr(),
                                            q.data_ptr(), self._work.data_ptr(), int(self._work.numel()), out_ll.data_ptr(),
                                            out_n.data_ptr(), pl._stream()))
        return float(out_ll.item()), int(out_n.item())

    def holdout_nll_f32(self, p, q):
        """`holdout_nll_f32` (:6527-6563) -> (mean_nll, deviance, n_eval) = (-ll / n, -2 ll, n) over the held-out calls, with the
        reconstruction clamped in f64 (README, Known differences); (NaN, NaN, 0) without held-out calls."""
        pt, qt = _admx_pq_host(self._full, p, q)
        ll, n_eval = self._holdout(pt.contiguous(), qt.contiguous())
        if n_eval == 0:
            return float("nan"), float("nan"), 0
        return -ll / n_eval, -2.0 * ll, n_eval


def admx_evaluate_cverror(session, k, folds, seed=42, solver="adam-em", power=5, tol=1e-5, max_als=1000, reg_als=1e-5, lr=0.005,
                          beta1=0.80, beta2=0.88, epsilon=1e-8, max_iter=500, check_every=5, lr_decay=0.5, min_lr=1e-6,
                          keep_fits=False):
    """`evaluate_adamixture_cverror_bed` (python/janusx/adamixture/core.py:1662-1794): K-fold cross-validation error of one K on
    a staged session.  Fold i holds out the called genotypes of fold i, is fitted with the seed `seed + i + 1` and scored by the
    mean binomial negative log-likelihood of its held-out calls -> dict(cverror = mean of the fold means, cverror_se =
    std(ddof=1) / sqrt(folds), cv_folds, cv_observed, fold_counts, fold_mean_nll, fold_eval_counts[, fold_p, fold_q])."""
    folds = int(folds)
    if folds < 2:
        raise ValueError(f"CVerror requires folds >= 2, got {folds}. Use -cverror N with N>=2.")
    if folds > ADMX_CV_MAX_FOLDS:
        raise ValueError(f"CVerror folds must be at most {ADMX_CV_MAX_FOLDS} on this build (got {folds})")
    n_obs, fold_counts = session.cv_observed_fold_counts(folds, seed)
    if n_obs < folds:
        raise ValueError(f"Not enough observed genotypes for CVerror: observed={n_obs}, folds={folds}.")
    if np.any(fold_counts <= 0):
        bad = [str(i + 1) for i in np.flatnonzero(fold_counts <= 0)]
        raise ValueError(f"Failed to build non-empty CV folds in BED foldmask assignment; empty folds={','.join(bad)}.")
    means, evals, fits_p, fits_q = [], [], [], []
    for i in range(folds):
        fb = session.make_cv_fold_backend(i, folds, seed)
        try:
            if fb.holdout_observed <= 0:
                raise ValueError(f"Fold {i + 1} has no held-out genotypes.")
            p, q, _ll, _it, _init_ll, _als = fb._fit(k, int(seed) + i + 1, solver, power, tol, max_als, reg_als, lr, beta1, beta2,
                                                     epsilon, max_iter, check_every, lr_decay, min_lr)
            ll, n_eval = fb._holdout(p.contiguous(), q.contiguous())
            if n_eval <= 0:
                raise ValueError(f"Fold {i + 1} produced no held-out evaluation genotypes.")
            means.append(-ll / n_eval)
            evals.append(n_eval)
            if keep_fits:
                fits_p.append(p.cpu().numpy())
                fits_q.append(q.cpu().numpy())
        finally:
            fb.close()
    arr = np.asarray(means, dtype=np.float64)
    out = {"cverror": float(np.mean(arr)), "cverror_se": float(np.std(arr, ddof=1) / np.sqrt(arr.size)), "cv_folds": folds,
           "cv_observed": int(n_obs), "fold_counts": fold_counts, "fold_mean_nll": arr,
           "fold_eval_counts": np.asarray(evals, dtype=np.int64)}
    if keep_fits:
        out["fold_p"], out["fold_q"] = fits_p, fits_q
    return out


def admx_bed_training_meta(genotype_path, snps_only=True, maf=0.02, missing_rate=0.05, memory_mb=0):
    """-> (row_freq f32 of the kept rows, n_samples) (src/stats/adamixture.rs:6761-6800)."""
    _admx_check_qc(maf, missing_rate)
    panel, _c, _rows, _flip, freq, _bim, _p = _admx_kept_rows(genotype_path, snps_only, maf, missing_rate, None,
                                                              "admx_bed_training_meta", "BED training session")
    return freq, int(panel.n)


def admx_multiply_a_omega_bed(genotype_path, omega, row_freq, snps_only=True, maf=0.02, missing_rate=0.05, delimiter=None,
                              mmap_window_mb=0, memory_mb=0):
    """Z omega of the centred design over the kept rows (src/stats/adamixture.rs:6709-6760; `_RsvdOperator.zq`) -> (m, k) f32.
    `delimiter`, `mmap_window_mb` and `memory_mb` are accepted and unused."""
    import torch
    s = AdmxBedTrainingSession(genotype_path, snps_only, maf, missing_rate, memory_mb)
    om = _c(omega, np.float32)
    if om.ndim != 2 or om.shape[0] != s.n_samples or om.shape[1] == 0:
        raise RuntimeError("omega must be a non-empty 2D matrix with shape (n_samples, k)")
    rf = _c(row_freq, np.float32).ravel()
    if rf.size != s.n_snps:
        raise RuntimeError(f"row_freq length mismatch: got {rf.size}, expected {s.n_snps}")
    return s.zq(torch.from_numpy(om).to(s._panel.device)).cpu().numpy()


def _admx_pq_host(eng, p, q):
    import torch
    p = _c(p, np.float32)
    q = _c(q, np.float32)
    if p.ndim != 2 or q.ndim != 2 or p.shape[0] != eng.m or q.shape[0] != eng.n or p.shape[1] != q.shape[1]:
        raise RuntimeError(f"shape mismatch: G=({eng.m},{eng.n}), P={tuple(p.shape)}, Q={tuple(q.shape)}")
    return torch.from_numpy(p).to(eng.dev), torch.from_numpy(q).to(eng.dev)


def admx_loglikelihood_bed_f32(genotype_path, p, q, snps_only=True, maf=0.02, missing_rate=0.05, memory_mb=0):
    s = AdmxBedTrainingSession(genotype_path, snps_only, maf, missing_rate, memory_mb)
    pt, qt = _admx_pq_host(s._eng, p, q)
    return s._eng.loglik(pt, qt)


def admx_adam_optimize_bed_f32(genotype_path, p0, q0, lr=0.005, beta1=0.80, beta2=0.88, epsilon=1e-8, max_iter=1500,
                               check_every=5, lr_decay=0.5, min_lr=1e-6, snps_only=True, maf=0.02, missing_rate=0.05,
                               memory_mb=0):
    """-> (P, Q, ll_best, iterations) (src/stats/adamixture.rs:8563-8640)."""
    s = AdmxBedTrainingSession(genotype_path, snps_only, maf, missing_rate, memory_mb)
    pt, qt = _admx_pq_host(s._eng, p0, q0)
    p, q, ll, it = _admx_adam_loop(s._eng, pt, qt, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay, min_lr)
    return p.cpu().numpy(), q.cpu().numpy(), ll, it


def _admx_dense_engine(g):
    """Engine of a dense (m, n) u8 genotype matrix (0 / 1 / 2 = minor-allele count, 3 = missing, no flip), packed to 2 bits."""
    import torch
    from .bed import pack_dosage
    g = np.asarray(g)
    if g.ndim != 2 or g.dtype != np.uint8:
        raise RuntimeError("g must be a 2D uint8 matrix (m, n) with 0/1/2 and 3 = missing")
    m, n = g.shape
    if m == 0 or n == 0:
        raise RuntimeError("invalid empty genotype matrix")
    dose = np.where(g > 2, -1, g.astype(np.int8)).astype(np.int8)
    packed = torch.from_numpy(pack_dosage(dose)).to(torch.device("cuda", torch.cuda.current_device()))
    from . import pipeline as pl
    return _AdmxEngine(pl.Panel(packed, n), None, np.zeros(m, dtype=bool))


def admx_loglikelihood_f32(g, p, q):
    eng = _admx_dense_engine(g)
    pt, qt = _admx_pq_host(eng, p, q)
    return eng.loglik(pt, qt)


def admx_em_step_inplace_f32(g, p, q, p_em, q_em, tile_cols=None):
    """One EM step of a dense u8 matrix into the caller's p_em (m, k) / q_em (n, k) f32 arrays (`tile_cols` accepted, unused)."""
    eng = _admx_dense_engine(g)
    pt, qt = _admx_pq_host(eng, p, q)
    if p_em.shape != tuple(pt.shape) or q_em.shape != tuple(qt.shape):
        raise RuntimeError("invalid packed EM output buffer size")
    pe, qe = eng.em_step(pt, qt)
    p_em[...] = pe.cpu().numpy()
    q_em[...] = qe.cpu().numpy()


def admx_adam_optimize_f32(g, p0, q0, lr=0.005, beta1=0.80, beta2=0.88, epsilon=1e-8, max_iter=1500, check_every=5,
                           lr_decay=0.5, min_lr=1e-6, tile_cols=None):
    eng = _admx_dense_engine(g)
    pt, qt = _admx_pq_host(eng, p0, q0)
    p, q, ll, it = _admx_adam_loop(eng, pt, qt, lr, beta1, beta2, epsilon, max_iter, check_every, lr_decay, min_lr)
    return p.cpu().numpy(), q.cpu().numpy(), ll, it


def admx_map_q_f32(q):
    import torch
    return _admx_map_q(torch.from_numpy(_c(q, np.float32).copy())).numpy()


def admx_map_p_f32(p):
    return np.clip(_c(p, np.float32), np.float32(_ADMX_EPS), np.float32(1.0 - _ADMX_EPS)).astype(np.float32)


def admx_rmse_f32(q1, q2):
    a, b = _c(q1, np.float32), _c(q2, np.float32)
    if a.shape != b.shape:
        raise RuntimeError("shape mismatch in admx_rmse_f32")
    if a.size == 0:
        return 0.0
    d = (a - b).astype(np.float64)
    return float(np.float32(np.float32(np.sum(d * d) / a.size) ** np.float32(0.5)))


# ---- LD pruning and LD-block r^2 on the packed genotypes (`jx gformat -prune`; csrc/k_ld.hip) ------------------------------------

LD_MASK_BUDGET_BYTES = 256 << 20   # device band mask of one SNP range (and the integer sums of one block of LD-block rows)


def _ld_row_stats(counts, n):
    """src/stats/ld.rs:469-543 from the integer row counts (missing, het, hom_alt) -> (mean, std, maf f64, has_missing bool),
    in the reference's operation order (numpy's f64 elementwise operations are the IEEE ones the reference's are)."""
    c = np.asarray(counts, dtype=np.int64)
    non_missing = int(n) - c[:, 0]
    has = non_missing > 0
    obs_n = np.where(has, non_missing, 1).astype(np.float64)
    sum_g = (c[:, 1] + 2 * c[:, 2]).astype(np.float64)
    sum_g2 = (c[:, 1] + 4 * c[:, 2]).astype(np.float64)
    denom = float(max(int(n) - 1, 1))
    p = sum_g / (2.0 * obs_n)
    maf = np.minimum(p, 1.0 - p)
    mean = sum_g / obs_n
    ss = np.maximum(sum_g2 - (sum_g * sum_g / obs_n), 0.0)
    std = np.sqrt(np.maximum(ss / denom, 1e-12))
    return (np.where(has, mean, 0.0), np.where(has, std, 1e-6), np.where(has, maf, 0.0), non_missing < int(n))


def _ld_window_ends(chrom_codes, positions, window_bp, window_variants, step_variants):
    """`jx_ld_window_ends` (host, no device): chromosome-grouped order of the rows, group offsets, window end per window start and
    band end per row, all in positions of that order."""
    cc, ps = _c(chrom_codes, np.int32).ravel(), _c(positions, np.int64).ravel()
    m = int(cc.shape[0])
    order, off = np.zeros(m, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    win_end, band_end, ng = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(1, dtype=np.int64)
    check(lib().jx_ld_window_ends(_p(cc), _p(ps), m, int(window_bp or 0), 0 if window_bp else int(window_variants or 0),
                                  int(step_variants), _p(order), _p(off), _p(ng), _p(win_end), _p(band_end)))
    return order, off[:int(ng[0]) + 1].copy(), win_end, band_end


def _ld_prune_greedy(maf, chrom_off, win_end, ws0, ws1, mask, r0, r1, first_unchecked, dropped):
    """`jx_ld_prune_greedy` (host, no device) over the windows that start in [ws0, ws1) with the band mask (r1 - r0, wpr) uint32 of
    the rows [r0, r1); `first_unchecked` (int64) and `dropped` (uint8) are updated in place."""
    mask = _c(mask, np.uint32)
    if mask.ndim != 2 or mask.shape[0] != r1 - r0:
        raise RuntimeError(f"band mask shape mismatch: got {mask.shape}, expected ({r1 - r0}, words per row)")
    check(lib().jx_ld_prune_greedy(_p(maf), int(maf.shape[0]), _p(chrom_off), int(chrom_off.shape[0]) - 1, _p(win_end), int(ws0),
                                   int(ws1), _p(mask), int(r0), int(r1), int(mask.shape[1]), _p(first_unchecked), _p(dropped)))


def _ld_ranges(win_end, band_end, budget_bytes):
    """SNP ranges whose band masks stay under `budget_bytes`: [(ws0, ws1, r1, wpr)] = the windows that start in [ws0, ws1), all of
    which end at or before r1, and the words per mask row of the rows [ws0, r1).  The ranges partition the window starts in
    order, so the greedy runs them one after the other; rows shared by two ranges get their mask rows computed twice."""
    m = int(win_end.shape[0])
    idx = np.arange(m, dtype=np.int64)
    width = np.maximum(band_end - idx - 1, 0)
    wpr_all = max(1, (int(width.max()) + 31) // 32) if m else 1
    longest = int((win_end - idx)[win_end > 0].max()) if np.any(win_end > 0) else 1
    rows_cap = min(int(budget_bytes) // (4 * wpr_all), 1 << 20)
    if rows_cap < longest:
        raise RuntimeError(f"LD prune: a band mask budget of {int(budget_bytes)} bytes holds {rows_cap} rows of {wpr_all} words, the "
                           f"longest window has {longest} rows; use a smaller window or a larger budget")
    out, a = [], 0
    while a < m:
        r1 = min(a + rows_cap, m)
        over = np.nonzero(win_end[a:r1] > r1)[0]
        ws1 = a + int(over[0]) if over.size else r1
        ends = win_end[a:ws1]
        top = int(ends.max()) if ends.size else 0
        if top > a:
            wpr = max(1, (int(width[a:top].max()) + 31) // 32)
            out.append((a, ws1, top, wpr))
        a = ws1
    return out


def _ld_prune_check_args(ndim, bps, n_samples, n_chrom, n_pos, m, window_bp, window_variants, step_variants, r2_threshold):
    """Argument checks of src/stats/ld.rs:4269-4329, in its order and with its texts."""
    import math
    if ndim != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    r2 = float(r2_threshold)
    if not (math.isfinite(r2) and r2 > 0.0 and r2 <= 1.0):
        raise RuntimeError("r2_threshold must be finite and in (0, 1]")
    if int(step_variants) <= 0:
        raise RuntimeError("step_variants must be > 0")
    if window_bp is None and window_variants is None:
        raise RuntimeError("provide one of window_bp or window_variants")
    if window_bp is not None and int(window_bp) <= 0:
        raise RuntimeError("window_bp must be > 0")
    if window_variants is not None and int(window_variants) <= 0:
        raise RuntimeError("window_variants must be > 0")
    expected = (int(n_samples) + 3) // 4
    if bps != expected:
        raise RuntimeError(f"packed second dimension mismatch: got {bps}, expected {expected} for n_samples={int(n_samples)}")
    if n_chrom != m:
        raise RuntimeError(f"chrom_codes length mismatch: got {n_chrom}, expected {m}")
    if n_pos != m:
        raise RuntimeError(f"positions length mismatch: got {n_pos}, expected {m}")


def bed_packed_ld_prune_maf_priority(packed, n_samples, chrom_codes, positions, window_bp=None, window_variants=None,
                                     step_variants=1, r2_threshold=0.2, threads=0, mask_budget_bytes=None, timings=None):
    """src/stats/ld.rs:4245-4361: LD pruning of a packed payload (m, ceil(n / 4)) with MAF priority -> bool keep mask (m).  Windows
    of `window_bp` base pairs (it wins when both are given) or `window_variants` rows, moved by `step_variants` rows, per
    chromosome code; inside a window the strict greedy of :270-402 drops, of the first pair with r^2 > r2_threshold, the row of
    the lower MAF.  The pair predicate comes from the device (`jxg_ld_band_mask_p32`: exact integer sums, r^2 in f64 in the
    reference's operation order), range by range so that the device mask stays under `mask_budget_bytes` (extension, default
    `LD_MASK_BUDGET_BYTES`); the greedy runs on the host (`jx_ld_prune_greedy`).  The keep mask equals the reference algorithm's
    bit for bit.  `threads` is accepted and unused; `packed` may be a torch CUDA uint8 tensor (used in place); `timings`
    (extension): a dict that receives `mask_s` (wall seconds of the band-mask launches with the device-to-host mask copies and
    their synchronisation), `greedy_s` (host greedy) and `ranges`."""
    shape = tuple(packed.shape) if hasattr(packed, "shape") else np.asarray(packed).shape
    cc = np.asarray(chrom_codes).ravel()
    ps = np.asarray(positions).ravel()
    m = int(shape[0]) if len(shape) >= 1 else 0
    _ld_prune_check_args(len(shape), int(shape[1]) if len(shape) == 2 else -1, n_samples, int(cc.shape[0]), int(ps.shape[0]), m,
                         window_bp, window_variants, step_variants, r2_threshold)
    if m == 0:
        return np.zeros(0, dtype=bool)
    n = int(n_samples)
    order, chrom_off, win_end, band_end = _ld_window_ends(cc, ps, window_bp, window_variants, step_variants)
    ranges = _ld_ranges(win_end, band_end, LD_MASK_BUDGET_BYTES if mask_budget_bytes is None else int(mask_budget_bytes))
    if not ranges:                                            # no window holds two rows
        return np.ones(m, dtype=bool)
    import torch
    from .pipeline import _ptr, _stream
    panel = _panel(packed, n)
    mean, std, maf, hasmiss = _ld_row_stats(panel.counts(), n)
    dev = panel.device
    identity = bool(np.array_equal(order, np.arange(m)))
    rows_t = None if identity else torch.from_numpy(order.astype(np.int32)).to(dev)
    mean_t = torch.from_numpy(np.ascontiguousarray(mean[order])).to(dev)
    std_t = torch.from_numpy(np.ascontiguousarray(std[order])).to(dev)
    miss_t = torch.from_numpy(np.ascontiguousarray(hasmiss[order].astype(np.uint8))).to(dev)
    band_t = torch.from_numpy(band_end.astype(np.int32)).to(dev)
    maf_s = np.ascontiguousarray(maf[order])
    first_unchecked = np.arange(1, m + 1, dtype=np.int64)
    dropped = np.zeros(m, dtype=np.uint8)
    words = max((r1 - a) * wpr for a, _ws1, r1, wpr in ranges)
    mask_t = torch.empty(words, dtype=torch.int32, device=dev)
    t_kernel = t_greedy = 0.0
    for a, ws1, r1, wpr in ranges:
        t0 = time.perf_counter()
        check(lib().jxg_ld_band_mask_p32(_ptr(panel.p32), m, n, _ptr(rows_t), m, a, r1, _ptr(band_t), _ptr(mean_t), _ptr(std_t),
                                         _ptr(miss_t), float(r2_threshold), wpr, _ptr(mask_t), _stream()))
        mask = mask_t[:(r1 - a) * wpr].cpu().numpy().view(np.uint32).reshape(r1 - a, wpr)
        t1 = time.perf_counter()
        _ld_prune_greedy(maf_s, chrom_off, win_end, a, ws1, mask, a, r1, first_unchecked, dropped)
        t_kernel += t1 - t0
        t_greedy += time.perf_counter() - t1
    if timings is not None:
        timings.update(mask_s=t_kernel, greedy_s=t_greedy, ranges=len(ranges))
    keep = np.ones(m, dtype=bool)
    keep[order] = dropped == 0
    return keep


def _ld_sums(panel, i0, i1, j0, j1, rows=None):
    """(6, i1 - i0, j1 - j0) int32 D, N, S_i, S_j, Q_i, Q_j of a block of row pairs of a panel (`jxg_ld_sums_p32`); with `rows`
    (record numbers of the panel) the block is one of positions of that row list."""
    import torch
    from .pipeline import _ptr, _stream
    out = torch.empty((6, i1 - i0, j1 - j0), dtype=torch.int32, device=panel.device)
    rows_t = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(panel.device)
    nrows = panel.m if rows is None else int(rows_t.shape[0])
    check(lib().jxg_ld_sums_p32(_ptr(panel.p32), panel.m, panel.n, _ptr(rows_t), nrows, int(i0), int(i1), int(j0), int(j1), _ptr(out),
                                _stream()))
    return out.cpu().numpy()


def ld_r2_matrix_packed(packed_rows, n_samples):
    """`ld_r2_matrix_from_packed_rows_blas`, src/stats/ld.rs:1095-1198: r^2 (m, m) f32 of the rows of a packed payload, each row
    centred by its mean rounded to f32 with missing calls at 0, r^2 = clamp((gram_ij / sqrt(gram_ii gram_jj))^2, 0, 1), 0 where
    the root is <= 1e-20, 1 on the diagonal.  The Gram comes from the exact integer sums of `jxg_ld_sums_p32`:
    gram_ij = D - mu_i S_j - mu_j S_i + mu_i mu_j N in f64 (the reference adds f32 products in its BLAS)."""
    shape = tuple(packed_rows.shape)
    if len(shape) != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    m, n = int(shape[0]), int(n_samples)
    if m == 0:
        return np.zeros((0, 0), dtype=np.float32)
    if m == 1:
        return np.ones((1, 1), dtype=np.float32)
    if n <= 0:
        raise RuntimeError("n_samples must be > 0")
    if shape[1] != (n + 3) // 4:
        raise RuntimeError(f"packed row length mismatch: got {m * shape[1]}, expected {m * ((n + 3) // 4)}")
    panel = _panel(packed_rows, n)
    c = panel.counts().astype(np.int64)
    mean = _ld_row_stats(c, n)[0]
    mu = mean.astype(np.float32).astype(np.float64)
    nm = (n - c[:, 0]).astype(np.float64)
    alt, sq = (c[:, 1] + 2 * c[:, 2]).astype(np.float64), (c[:, 1] + 4 * c[:, 2]).astype(np.float64)
    diag = np.maximum(sq - 2.0 * mu * alt + mu * mu * nm, 0.0)
    out = np.empty((m, m), dtype=np.float32)
    step = max(32, min(m, (LD_MASK_BUDGET_BYTES // (24 * m)) // 32 * 32))
    for i0 in range(0, m, step):
        i1 = min(m, i0 + step)
        s = _ld_sums(panel, i0, i1, 0, m).astype(np.float64)
        mi = mu[i0:i1, None]
        gram = s[0] - mi * s[3] - mu[None, :] * s[2] + (mi * mu[None, :]) * s[1]
        den = np.sqrt(diag[i0:i1, None] * diag[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            corr = np.where(den > 1e-20, gram / np.where(den > 1e-20, den, 1.0), 0.0)
            r2 = corr * corr
        r2 = np.clip(np.where(np.isfinite(r2), r2, 0.0), 0.0, 1.0)
        out[i0:i1] = r2.astype(np.float32)
    np.fill_diagonal(out, 1.0)
    return out


def _ld_chr_token(s):
    """`normalize_chr_token`, src/stats/ld.rs:621-628: trimmed, a leading `chr` (any case) stripped."""
    t = str(s).strip()
    return t[3:] if len(t) >= 3 and t[:3].lower() == "chr" else t


def _ld_select_bim(bfile, chrom_ranges, start_bp, end_bp, selected_chrom=None, selected_pos=None):
    """Row selection of `bed_ldblock_r2_rust` (src/stats/ld.rs:793-825, 871-921, 4741-4773; host only) -> (total rows, row indices,
    chromosome tokens, positions)."""
    prefix = _bed_prefix(bfile)
    if not prefix:
        raise RuntimeError("bfile must not be empty")
    chrom_ranges, start_bp, end_bp = list(chrom_ranges), [int(v) for v in start_bp], [int(v) for v in end_bp]
    if len(chrom_ranges) != len(start_bp) or len(chrom_ranges) != len(end_bp):
        raise RuntimeError(f"bimrange length mismatch: chrom_ranges={len(chrom_ranges)}, start_bp={len(start_bp)}, "
                           f"end_bp={len(end_bp)}")
    if not chrom_ranges:
        raise RuntimeError("bimrange list must not be empty")
    ranges = {}
    for i, (ch, s, e) in enumerate(zip(chrom_ranges, start_bp, end_bp)):
        if s < 0 or e < 0:
            raise RuntimeError(f"bimrange[{i}] start/end must be >= 0, got ({s}, {e})")
        if s > e:
            s, e = e, s
        ranges.setdefault(_ld_chr_token(ch), []).append((s, e))
    sites = None
    if (selected_chrom is None) != (selected_pos is None):
        raise RuntimeError("selected_chrom and selected_pos must be provided together")
    if selected_chrom is not None:
        if len(selected_chrom) != len(selected_pos):
            raise RuntimeError(f"selected_chrom/selected_pos length mismatch: {len(selected_chrom)} vs {len(selected_pos)}")
        sites = {(_ld_chr_token(ch), int(p)) for ch, p in zip(selected_chrom, selected_pos)}
    total, idx, chrom, pos = 0, [], [], []
    path = f"{prefix}.bim"
    try:
        fh = open(path)
    except OSError as e:
        raise RuntimeError(f"{path}: {e}") from None
    with fh:
        for line_no, line in enumerate(fh, 1):
            parts = line.split()
            if len(parts) < 4:
                raise RuntimeError(f"{path}:{line_no}: malformed .bim line")
            try:
                p = int(parts[3])
            except ValueError:
                raise RuntimeError(f"{path}:{line_no}: invalid position {parts[3]!r}") from None
            ch = _ld_chr_token(parts[0])
            keep = any(s <= p <= e for s, e in ranges.get(ch, ()))
            if keep and sites is not None and (ch, p) not in sites:
                keep = False
            if keep:
                idx.append(total)
                chrom.append(ch)
                pos.append(p)
            total += 1
    if total == 0:
        raise RuntimeError(f"no variant rows in {path}")
    return total, idx, chrom, pos


def bed_ldblock_r2_rust(bfile, chrom_ranges, start_bp, end_bp, selected_chrom=None, selected_pos=None, threads=0):
    """src/stats/ld.rs:4721-4811: r^2 matrix of the `.bim` rows of a PLINK prefix that lie in the inclusive ranges
    (chrom_ranges[i], start_bp[i], end_bp[i]) (a `chr` prefix is stripped, a reversed range is swapped) and, when given, in the site
    set (selected_chrom, selected_pos) -> (r2 f32 (k, k), chromosome tokens, positions).  An empty selection gives a (0, 0) array
    and two empty lists.  `threads` is accepted and unused."""
    from .bed import BED_MAGIC, read_fam_ids
    prefix = _bed_prefix(bfile)
    total, idx, chrom, pos = _ld_select_bim(bfile, chrom_ranges, start_bp, end_bp, selected_chrom, selected_pos)
    if not idx:
        return np.zeros((0, 0), dtype=np.float32), [], []
    n = len(read_fam_ids(prefix))
    if n == 0:
        raise RuntimeError("empty PLINK input (no samples in .fam)")
    bps = (n + 3) // 4
    path = f"{prefix}.bed"
    with open(path, "rb") as fh:
        if fh.read(3) != BED_MAGIC:
            raise RuntimeError(f"{path}: not a SNP-major PLINK .bed (bad magic)")
    if os.path.getsize(path) != 3 + total * bps:
        raise RuntimeError(f"{path}: size {os.path.getsize(path)} != 3 + {total}*{bps}")
    rows = np.ascontiguousarray(np.memmap(path, dtype=np.uint8, mode="r", offset=3, shape=(total, bps))[np.asarray(idx)])
    return ld_r2_matrix_packed(rows, n), chrom, pos


# ---- site / sample statistics and LD scores (`jx gstats`; src/stats/gstats.rs; csrc/k_gstats.hip, csrc/k_ld.hip) --------------------

LDSC_PARTIAL_BUDGET_BYTES = 256 << 20   # device partial sums (one f64 per row and 32-row block of partners) of one row range
_LDSC_KINDS = {"variant": 0, "variants": 0, "snp": 0, "snps": 0, "bp": 1, "b": 1, "kb": 1, "mb": 1, "cm": 2, "genetic": 2}


def _rust_f64(v):
    """A float as Rust's `{}` prints it (the reference's error texts)."""
    import math
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return str(int(v)) if v == math.floor(v) and abs(v) < 1e16 else repr(v)


def _ldsc_parse_window(kind, value):
    """`parse_ldsc_window`, src/stats/gstats.rs:824-863 -> (0 variants | 1 bp | 2 cM, integer window, cM window)."""
    import math
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise RuntimeError(f"window_value must be finite and > 0, got {_rust_f64(value)}")
    code = _LDSC_KINDS.get(str(kind).strip().lower())
    if code is None:
        raise RuntimeError(f"window_kind must be one of: variants, bp, cm; got '{kind}'")
    if code == 2:
        return 2, 0, value
    rounded = math.floor(value + 0.5)                         # f64::round of a positive value
    w = int(min(rounded, 2.0 ** 63 - 1024.0))                 # `as i64` saturates
    if code == 0:
        if abs(rounded - value) > 1e-9:
            raise RuntimeError(f"variant-count LD-score window must be an integer, got {_rust_f64(value)}")
        if w <= 0:
            raise RuntimeError(f"variant-count LD-score window must be > 0, got {w}")
    else:
        if abs(rounded - value) > 1e-6:
            raise RuntimeError(f"bp LD-score window must resolve to an integer, got {_rust_f64(value)}")
        if w <= 0:
            raise RuntimeError(f"bp LD-score window must be > 0, got {w}")
    return code, w, 0.0


def _ldsc_window_bounds(chrom_codes, positions, cm_positions, kind, w_int, w_cm):
    """`jx_ldsc_window_bounds` (host, no device): the chromosome-grouped, sorted order of the rows, the group offsets and the
    two-sided window [start, end) per position of that order."""
    cc, ps = _c(chrom_codes, np.int32).ravel(), _c(positions, np.int64).ravel()
    cm = None if cm_positions is None else _c(cm_positions, np.float64).ravel()
    m = int(cc.shape[0])
    order, off, ng = np.zeros(m, dtype=np.int64), np.zeros(m + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    start, end = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    check(lib().jx_ldsc_window_bounds(_p(cc), _p(ps), _p(cm), m, int(kind), int(w_int), float(w_cm), _p(order), _p(off), _p(ng),
                                      _p(start), _p(end)))
    return order, off[:int(ng[0]) + 1].copy(), start, end


def _ldsc_ranges(start, end, budget_bytes):
    """Row ranges [(r0, r1, npb)] of the row list whose partial sums stay under `budget_bytes`: r0 a multiple of 32, so that the
    32-row blocks of a row and of its partners, and hence the rounding of its score, do not depend on the budget; npb = the most
    32-row blocks of partners any 32-row block of the range reaches; at most 65 535 blocks per range (the grid)."""
    m = int(start.shape[0])
    edges = np.arange(0, m, 32)
    reach = (np.maximum.reduceat(end, edges) - 1) // 32 - np.minimum.reduceat(start, edges) // 32 + 1
    budget, out, a, nblk = int(budget_bytes), [], 0, int(edges.shape[0])
    while a < nblk:
        npb = int(reach[a])
        if 32 * npb * 8 > budget:
            raise RuntimeError(f"LD score: a partial-sum budget of {budget} bytes is below the {32 * npb * 8} bytes one block of 32 "
                               f"rows needs ({npb} blocks of partners); use a smaller window or a larger budget")
        b = a + 1
        while b < nblk and b - a < 65535:
            top = max(npb, int(reach[b]))
            if (b + 1 - a) * 32 * top * 8 > budget:
                break
            npb, b = top, b + 1
        out.append((32 * a, min(32 * b, m), npb))
        a = b
    return out


def ldscore_packed(packed, n_samples, chrom_codes, positions, cm_positions=None, window_kind="bp", window_value=100000,
                   partial_budget_bytes=None, timings=None):
    """LD scores of a packed payload (m, ceil(n / 4)) (extension: `compute_ldscore_core`, src/stats/gstats.rs:1002-1171, for a panel
    in memory) -> (M int64 (m), ldsc f64 (m)): per row the size of its two-sided window among the rows of its chromosome code
    (`window_kind` / `window_value` as `gstats_bed_ldscore`; `cm_positions` for a cM window) and l_i = self term + the sum of the
    clamped r^2 with the other rows of the window.  The windows come from the host (`jx_ldsc_window_bounds`), the pair values and
    their sums from the device (`jxg_ld_score_p32`: exact integer pair sums, r^2 in f64 in the reference's operation order from
    the side of the row the score belongs to), range by range so that the device partials stay under `partial_budget_bytes`
    (default `LDSC_PARTIAL_BUDGET_BYTES`); the scores do not depend on the budget.  `packed` may be a torch CUDA uint8 tensor;
    `timings`: a dict that receives `bounds_s`, `score_s` (launches and the copy of the scores) and `ranges`."""
    kind, w_int, w_cm = _ldsc_parse_window(window_kind, window_value)
    shape = tuple(packed.shape) if hasattr(packed, "shape") else np.asarray(packed).shape
    if len(shape) != 2:
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    n, m = int(n_samples), int(shape[0])
    if n <= 0:
        raise RuntimeError("n_samples must be > 0")
    if int(shape[1]) != (n + 3) // 4:
        raise RuntimeError(f"packed second dimension mismatch: got {int(shape[1])}, expected {(n + 3) // 4} for n_samples={n}")
    cc, ps = np.asarray(chrom_codes).ravel(), np.asarray(positions).ravel()
    if int(cc.shape[0]) != m:
        raise RuntimeError(f"chrom_codes length mismatch: got {int(cc.shape[0])}, expected {m}")
    if int(ps.shape[0]) != m:
        raise RuntimeError(f"positions length mismatch: got {int(ps.shape[0])}, expected {m}")
    if cm_positions is None and kind == 2:
        raise RuntimeError("a cM LD-score window needs cm_positions")
    if cm_positions is not None and int(np.asarray(cm_positions).size) != m:
        raise RuntimeError(f"cm_positions length mismatch: got {int(np.asarray(cm_positions).size)}, expected {m}")
    if m >= 1 << 31:
        raise RuntimeError("at most 2^31 - 1 rows")
    if m == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
    t0 = time.perf_counter()
    order, _off, start, end = _ldsc_window_bounds(cc, ps, cm_positions, kind, w_int, w_cm)
    t_bounds = time.perf_counter() - t0
    ranges = _ldsc_ranges(start, end, LDSC_PARTIAL_BUDGET_BYTES if partial_budget_bytes is None else int(partial_budget_bytes))
    import torch
    from .pipeline import _ptr, _stream
    panel = _panel(packed, n)
    counts = panel.counts().astype(np.int64)
    mean, std, maf, hasmiss = _ld_row_stats(counts, n)
    self_term = (((n - counts[:, 0]) > 1) & (maf > 0.0)).astype(np.float64)     # src/stats/gstats.rs:1054-1058
    dev = panel.device
    identity = bool(np.array_equal(order, np.arange(m)))
    rows_t = None if identity else torch.from_numpy(order.astype(np.int32)).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    mean_t, std_t, miss_t, self_t = up(mean[order]), up(std[order]), up(hasmiss[order].astype(np.uint8)), up(self_term[order])
    start_t, end_t = up(start.astype(np.int32)), up(end.astype(np.int32))
    part_t = torch.empty(max((r1 - r0) * npb for r0, r1, npb in ranges), dtype=torch.float64, device=dev)
    score_t = torch.empty(m, dtype=torch.float64, device=dev)
    t0 = time.perf_counter()
    for r0, r1, npb in ranges:
        check(lib().jxg_ld_score_p32(_ptr(panel.p32), m, n, _ptr(rows_t), m, r0, r1, _ptr(start_t), _ptr(end_t), _ptr(mean_t),
                                     _ptr(std_t), _ptr(miss_t), _ptr(self_t), npb, _ptr(part_t), _ptr(score_t), _stream()))
    score = score_t.cpu().numpy()
    if timings is not None:
        timings.update(bounds_s=t_bounds, score_s=time.perf_counter() - t0, ranges=len(ranges))
    m_counts, ldsc = np.empty(m, dtype=np.int64), np.empty(m, dtype=np.float64)
    m_counts[order] = end - start
    ldsc[order] = score
    return m_counts, ldsc


def _gstats_site_rates(counts, n):
    """`packed_site_rates`, src/stats/gstats.rs:158-177, in f32 from the integer row counts (missing, het, hom_alt) -> (maf, miss,
    het) f32.  numpy's float32 elementwise operations are the IEEE ones the reference's are, in its order."""
    c = np.asarray(counts, dtype=np.int64)
    missing, het_count, hom_alt = c[:, 0], c[:, 1], c[:, 2]
    non_missing = np.maximum(int(n) - missing, 0)
    called = non_missing > 0
    miss_rate = missing.astype(np.float32) / np.float32(n)
    nm32 = np.where(called, non_missing, 1).astype(np.float32)
    p_alt = (het_count + 2 * hom_alt).astype(np.float32) / (np.float32(2.0) * nm32)
    maf = np.minimum(p_alt, np.float32(1.0) - p_alt)
    het = het_count.astype(np.float32) / nm32
    zero = np.float32(0.0)
    return np.where(called, maf, zero).astype(np.float32), miss_rate.astype(np.float32), np.where(called, het, zero).astype(np.float32)


def _gstats_sample_rates(sample_counts, n_snps):
    """`finalize_individual_rates`, src/stats/gstats.rs:222-245, in f32 from the per-sample counts (2, n) (missing, het) -> (miss,
    het) f32."""
    c = np.asarray(sample_counts, dtype=np.int64)
    miss_ct, het_ct = c[0], c[1]
    nonmiss = int(n_snps) - miss_ct
    miss = miss_ct.astype(np.float32) / np.float32(n_snps)
    het = np.where(nonmiss > 0, het_ct.astype(np.float32) / np.where(nonmiss > 0, nonmiss, 1).astype(np.float32), np.float32(0.0))
    return miss.astype(np.float32), het.astype(np.float32)


def _sample_counts(panel):
    """(2, n) int32: per sample the number of rows of a panel with a missing call and with a het call (`jxg_sample_counts_p32`)."""
    import torch
    from .pipeline import _ptr, _stream
    out = torch.empty((2, panel.n), dtype=torch.int32, device=panel.device)
    check(lib().jxg_sample_counts_p32(_ptr(panel.p32), panel.m, panel.n, _ptr(out), _stream()))
    return out.cpu().numpy()


def sample_counts_packed(packed, n_samples):
    """Per-sample (missing, het) row counts (2, n) int32 of a packed payload (m, ceil(n / 4)), host array or torch CUDA tensor
    (extension: the integer half of `gstats_bed_individual_stats`)."""
    return _sample_counts(_panel(packed, n_samples))


def _gstats_open_bed(prefix):
    """`open_bed_mmap`, src/stats/gstats.rs:123-156 -> (payload (m, bps) uint8 memmap, n_samples, m)."""
    from .bed import read_fam_ids
    try:
        n = len(read_fam_ids(prefix))
    except OSError as e:
        raise RuntimeError(f"{prefix}.fam: {e}") from None
    if n == 0:
        raise RuntimeError("no samples found in PLINK input")
    path = f"{prefix}.bed"
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as fh:
            head = fh.read(3)
    except OSError as e:
        raise RuntimeError(f"{path}: {e}") from None
    if size < 3:
        raise RuntimeError(f"{path}: BED too small")
    if head != bytes([0x6C, 0x1B, 0x01]):
        raise RuntimeError(f"{path}: unsupported BED header (expect SNP-major 0x6C 0x1B 0x01)")
    bps, data_len = (n + 3) // 4, size - 3
    if data_len % bps != 0:
        raise RuntimeError(f"{path}: invalid payload length data_len={data_len}, bytes_per_snp={bps}")
    m = data_len // bps
    if m == 0:
        raise RuntimeError(f"{path}: no variant rows found")
    return np.memmap(path, dtype=np.uint8, mode="r", offset=3, shape=(m, bps)), n, m


def _gstats_bim_ldsc_meta(prefix):
    """`parse_bim_ldsc_meta`, src/stats/gstats.rs:785-822 -> (chromosome codes int32 by first appearance of the normalised token,
    positions int64, cM f64)."""
    path = f"{prefix}.bim"
    codes, cc, ps, cm = {}, [], [], []
    try:
        fh = open(path)
    except OSError as e:
        raise RuntimeError(f"{path}: {e}") from None
    with fh:
        for line_no, line in enumerate(fh, 1):
            toks = line.split()
            if len(toks) < 4:
                raise RuntimeError(f"{path}:{line_no}: malformed BIM row, expect at least 4 columns")
            try:
                if "_" in toks[2]:
                    raise ValueError
                cm.append(float(toks[2]))
            except ValueError:
                raise RuntimeError(f"{path}:{line_no}: invalid cM value '{toks[2]}': invalid float literal") from None
            try:
                if "_" in toks[3]:
                    raise ValueError
                bp = int(toks[3])
            except ValueError:
                raise RuntimeError(f"{path}:{line_no}: invalid BP value '{toks[3]}': invalid digit found in string") from None
            if not -(1 << 63) <= bp < (1 << 63):
                raise RuntimeError(f"{path}:{line_no}: invalid BP value '{toks[3]}': number too {'large' if bp > 0 else 'small'} "
                                   "to fit in target type")
            ps.append(bp)
            cc.append(codes.setdefault(_ld_chr_token(toks[0]), len(codes)))
    if not cc:
        raise RuntimeError(f"{path}: no variant rows found")
    return np.asarray(cc, dtype=np.int32), np.asarray(ps, dtype=np.int64), np.asarray(cm, dtype=np.float64)


def gstats_bed_site_stats(prefix, threads=0):
    """src/stats/gstats.rs:1173-1199: per-site MAF, missing rate and het rate of a PLINK prefix -> (maf, miss, het f32 (m),
    n_samples), the rates of `packed_site_rates` (:158-177) from the device's row counts.  `threads` is accepted and unused."""
    payload, n, _m = _gstats_open_bed(_bed_prefix(prefix))
    maf, miss, het = _gstats_site_rates(_panel(payload, n).counts(), n)
    return maf, miss, het, n


def gstats_bed_joint_stats(prefix, site_maf=True, site_miss=True, site_het=True, individual_miss=True, individual_het=True,
                           threads=0):
    """src/stats/gstats.rs:1201-1278: the requested site and sample tables of a PLINK prefix in one pass -> (maf, miss, het f32 (m),
    sample miss, sample het f32 (n), n_samples, n_snps), None where not requested.  `threads` is accepted and unused."""
    payload, n, m = _gstats_open_bed(_bed_prefix(prefix))
    panel = _panel(payload, n)
    maf, miss, het = _gstats_site_rates(panel.counts(), n)
    imiss = ihet = None
    if individual_miss or individual_het:
        imiss, ihet = _gstats_sample_rates(_sample_counts(panel), m)
    return (maf if site_maf else None, miss if site_miss else None, het if site_het else None, imiss if individual_miss else None,
            ihet if individual_het else None, n, m)


def gstats_bed_individual_stats(prefix, threads=0):
    """src/stats/gstats.rs:1331-1357: per-sample missing rate and het rate over the SNPs of a PLINK prefix -> (miss, het f32 (n),
    n_snps), `finalize_individual_rates` (:222-245) from the device's per-sample counts.  `threads` is accepted and unused."""
    payload, n, m = _gstats_open_bed(_bed_prefix(prefix))
    imiss, ihet = _gstats_sample_rates(_sample_counts(_panel(payload, n)), m)
    return imiss, ihet, m


def gstats_bed_ldscore(prefix, window_kind, window_value, threads=0):
    """src/stats/gstats.rs:1359-1403: windowed LD scores of a PLINK prefix -> (M int64 (m), ldsc f64 (m), n_samples); window kinds
    `variants` / `bp` / `cm` with their aliases (`parse_ldsc_window`, :824-863), chromosomes from the normalised `.bim` token,
    positions and cM from the `.bim`.  A NaN cM value under a cM window is refused (the reference sorts with it).  `threads` is
    accepted and unused."""
    pfx = _bed_prefix(prefix)
    _ldsc_parse_window(window_kind, window_value)
    payload, n, m = _gstats_open_bed(pfx)
    cc, ps, cm = _gstats_bim_ldsc_meta(pfx)
    if int(cc.shape[0]) != m:
        raise RuntimeError(f"BED/BIM row mismatch: bed={m}, bim={int(cc.shape[0])}")
    m_counts, ldsc = ldscore_packed(payload, n, cc, ps, cm, window_kind, window_value)
    return m_counts, ldsc, n


# ------------------------------------------------------------------------------------------------
# KING (src/math/KING.rs)
# ------------------------------------------------------------------------------------------------
# Robust kinship of Manichaikul et al. 2010 from the integer pair counts of csrc/k_king.hip (exact i32 Grams of the code
# indicators on the int8 matrix pipes), the related-pair graph and the greedy unrelated set.  The reference's early stop
# (`king_kinship_upper_bound`, :245-262) is not mirrored: the related set is the exact one (README, "Known differences").

KING_DEFAULT_KINSHIP_THRESHOLD = 0.05
KING_DEFAULT_MAX_EXACT_PAIRS = 8_000_000_000
KING_MAX_ROWS = 1 << 29
_KING_COUNT_FIELDS = ("shared_nonmissing", "ibs0", "same_hom", "both_het", "het_i_obs", "het_j_obs")


def _king_validate(packed, n_samples):
    """`validate_king_inputs`, src/math/KING.rs:96-125, on a payload (m, bytes_per_snp) or a flat byte array -> (n, m); no device
    call."""
    n = int(n_samples)
    if n <= 0:
        raise RuntimeError("KING requires n_samples > 0")
    if n > 0xFFFFFFFF:
        raise RuntimeError(f"KING adjacency uses u32 sample ids; got n_samples={n} > 4294967295")
    bps = (n + 3) // 4
    shape = tuple(int(s) for s in packed.shape)
    if len(shape) not in (1, 2):
        raise RuntimeError("packed must be 2D (m, bytes_per_snp)")
    nbytes = int(np.prod(shape, dtype=np.int64)) if shape else 0
    if nbytes == 0:
        raise RuntimeError("KING requires non-empty packed genotype data")
    if (len(shape) == 2 and shape[1] != bps) or nbytes % bps != 0:
        raise RuntimeError(f"KING packed payload length mismatch: packed_bytes={nbytes} not divisible by bytes_per_snp={bps}")
    m = nbytes // bps
    if m > KING_MAX_ROWS:
        raise RuntimeError(f"KING pair counts are exact int32 sums: at most {KING_MAX_ROWS} variant sites, got {m}")
    return n, m


def _king_payload2d(packed, n):
    return packed.reshape(-1, (n + 3) // 4) if len(packed.shape) == 1 else packed


def _king_threshold(kinship_threshold):
    t = float(kinship_threshold)
    if not np.isfinite(t):
        raise RuntimeError("KING kinship_threshold must be finite")
    return t


def _king_enforce_exact_budget(n):
    """`king_enforce_exact_budget`, src/math/KING.rs:200-215: JANUSX_KING_MAX_EXACT_PAIRS (default 8e9, 0 = no limit)."""
    raw = os.environ.get("JANUSX_KING_MAX_EXACT_PAIRS")
    limit = KING_DEFAULT_MAX_EXACT_PAIRS
    if raw is not None:
        txt = raw.strip()
        if txt.isascii() and (txt[1:] if txt[:1] == "+" else txt).isdigit() and int(txt) < (1 << 64):
            limit = int(txt)
    if limit == 0:
        return
    pairs = int(n) * max(int(n) - 1, 0) // 2
    if pairs > limit:
        raise RuntimeError(f"KING exact all-pairs budget exceeded: pairs={pairs} > limit={limit}. Set JANUSX_KING_MAX_EXACT_PAIRS=0 "
                           "to force, or raise the limit explicitly.")


def _king_counts(panel, i0, i1, j0, j1):
    import torch
    from .pipeline import _ptr, _stream
    out = torch.empty((6, i1 - i0, j1 - j0), dtype=torch.int32, device=panel.device)
    check(lib().jxg_king_counts_p32(_ptr(panel.p32), panel.m, panel.n, int(i0), int(i1), int(j0), int(j1), _ptr(out), _stream()))
    return out.cpu().numpy()


def king_pair_counts_packed(packed, n_samples, i0, i1, j0, j1):
    """(6, i1 - i0, j1 - j0) int32 pair counts of the samples [i0, i1) x [j0, j1) of a packed payload (host array or torch CUDA
    tensor), planes in the field order of `KingBitCounts` (src/math/bitwise.rs:127-135): shared_nonmissing, ibs0, same_hom,
    both_het, het_i_obs, het_j_obs (extension: the reference counts one pair per call)."""
    n, _m = _king_validate(packed, n_samples)
    i0, i1, j0, j1 = int(i0), int(i1), int(j0), int(j1)
    for name, lo, hi in (("sample_i", i0, i1), ("sample_j", j0, j1)):
        if lo < 0 or hi < lo:
            raise RuntimeError(f"KING {name} range [{lo}, {hi}) is not a range")
        if hi > n:
            raise RuntimeError(f"KING {name} out of range: {hi - 1} >= {n}")
    if i1 == i0 or j1 == j0:
        return np.zeros((6, i1 - i0, j1 - j0), dtype=np.int32)
    return _king_counts(_panel(_king_payload2d(packed, n), n), i0, i1, j0, j1)


def _king_stats_from_counts(c):
    """`king_stats_from_counts`, src/math/KING.rs:217-243, from the six counts of one pair."""
    shared, ibs0, same_hom, both_het, het_i, het_j = (int(v) for v in c)
    ibs2 = both_het + same_hom
    denom = het_i + het_j
    kin = (float(both_het) - 2.0 * float(ibs0)) / float(denom) if denom > 0 else float("nan")
    return {"shared_nonmissing": shared, "ibs0": ibs0, "ibs1": max(shared - (ibs0 + ibs2), 0), "ibs2": ibs2, "het_i_obs": het_i,
            "het_j_obs": het_j, "both_het": both_het, "kinship": kin}


def king_pair_stats(packed, n_samples, i, j):
    """`king_pair_stats`, src/math/KING.rs:410-428, of the samples i and j of a packed payload -> dict with the `KingPairStats`
    fields."""
    n, _m = _king_validate(packed, n_samples)
    i, j = int(i), int(j)
    if i < 0 or i >= n:
        raise RuntimeError(f"KING sample_i out of range: {i} >= {n}")
    if j < 0 or j >= n:
        raise RuntimeError(f"KING sample_j out of range: {j} >= {n}")
    return _king_stats_from_counts(_king_counts(_panel(_king_payload2d(packed, n), n), i, i + 1, j, j + 1)[:, 0, 0])


def _king_related_pairs(panel, threshold, max_rows=None, timings=None):
    """Sorted related-pair table of a panel: the fused launch into a buffer of `max_rows` rows (default: 4 n + 65536), run again
    with a buffer of the counted size when the count exceeds it."""
    import torch
    from .pipeline import _ptr, _stream
    n = panel.n
    cap = int(max_rows) if max_rows is not None else min(n * (n - 1) // 2, 4 * n + 65536)
    cap = max(cap, 1)
    dev = panel.device
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    launches = 0
    t0 = time.perf_counter()
    while True:
        bi, bj, b0 = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
        bk = torch.empty(cap, dtype=torch.float64, device=dev)
        check(lib().jxg_king_related_p32(_ptr(panel.p32), panel.m, n, threshold, cap, _ptr(bi), _ptr(bj), _ptr(b0), _ptr(bk), _ptr(count),
                                         _stream()))
        launches += 1
        total = int(count.item())
        if total <= cap:
            break
        del bi, bj, b0, bk
        cap = total                                   # the count is exact: the second launch fits
    t1 = time.perf_counter()
    i = bi[:total].cpu().numpy().view(np.uint32)
    j = bj[:total].cpu().numpy().view(np.uint32)
    order = np.lexsort((j, i))
    if timings is not None:
        timings.update(pairs_s=t1 - t0, launches=launches, rows=total)
    return (np.ascontiguousarray(i[order]), np.ascontiguousarray(j[order]),
            np.ascontiguousarray(b0[:total].cpu().numpy().view(np.uint32)[order]), np.ascontiguousarray(bk[:total].cpu().numpy()[order]))


def _king_check_pairs_args(packed, n_samples, kinship_threshold, max_rows=None):
    n, m = _king_validate(packed, n_samples)
    t = _king_threshold(kinship_threshold)
    if max_rows is not None and int(max_rows) < 1:
        raise RuntimeError("KING max_rows must be >= 1")
    _king_enforce_exact_budget(n)
    return n, m, t


def king_related_pairs_packed(packed, n_samples, kinship_threshold=KING_DEFAULT_KINSHIP_THRESHOLD, max_rows=None):
    """`king_related_pairs_from_packed`, src/math/KING.rs:530-538: the pairs i < j with a finite kinship >= the threshold ->
    (i uint32, j uint32, ibs0 uint32, kinship f64), ordered by (i, j).  `max_rows`: rows of the first device buffer (the launch is
    repeated with the counted size when there are more)."""
    n, _m, t = _king_check_pairs_args(packed, n_samples, kinship_threshold, max_rows)
    return _king_related_pairs(_panel(_king_payload2d(packed, n), n), t, max_rows)


def _king_graph(n, pi, pj):
    """CSR adjacency of the related pairs (ordered by (i, j)): neighbours of a sample ascending (`king_related_graph_from_bitplanes`,
    src/math/KING.rs:631-648) -> (offsets int64 (n + 1), neighbors uint32, degrees int32)."""
    src = np.concatenate([pi, pj]).astype(np.int64)
    dst = np.concatenate([pj, pi]).astype(np.uint32)
    order = np.lexsort((dst, src))
    degrees = np.bincount(src, minlength=n).astype(np.int32)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(degrees, out=offsets[1:])
    return offsets, np.ascontiguousarray(dst[order]), degrees


def king_related_graph_packed(packed, n_samples, kinship_threshold=KING_DEFAULT_KINSHIP_THRESHOLD):
    """`king_related_graph_from_packed`, src/math/KING.rs:659-667 -> (neighbors: list of n ascending uint32 arrays, degrees int32 (n),
    edge_count, n_sites)."""
    n, m, t = _king_check_pairs_args(packed, n_samples, kinship_threshold)
    pi, pj, _b0, _k = _king_related_pairs(_panel(_king_payload2d(packed, n), n), t)
    offsets, nbrs, degrees = _king_graph(n, pi, pj)
    return [nbrs[offsets[s]:offsets[s + 1]] for s in range(n)], degrees, int(pi.shape[0]), m


def king_prune_related_graph(offsets, neighbors):
    """`king_prune_related_graph`, src/math/KING.rs:669-743, on a CSR graph (`jx_king_prune`, host) -> (kept uint32 ascending, removed
    uint32 in removal order)."""
    offsets = _c(offsets, np.int64).ravel()
    neighbors = _c(neighbors, np.uint32).ravel()
    n = int(offsets.shape[0]) - 1
    if n < 0:
        raise RuntimeError("KING graph offsets must hold n + 1 entries")
    if n and (int(offsets[-1]) != int(neighbors.shape[0]) or int(offsets[0]) != 0):
        raise RuntimeError(f"KING graph offsets do not match its neighbours: offsets[n]={int(offsets[-1])} neighbors={int(neighbors.shape[0])}")
    kept, removed = np.empty(max(n, 1), dtype=np.uint32), np.empty(max(n, 1), dtype=np.uint32)
    nk, nr = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    check(lib().jx_king_prune(n, _p(offsets), _p(neighbors), _p(kept), _p(nk), _p(removed), _p(nr)))
    return kept[:int(nk[0])].copy(), removed[:int(nr[0])].copy()


def _king_unrelated_set(panel, threshold, timings=None):
    pi, pj, b0, kin = _king_related_pairs(panel, threshold, timings=timings)
    t0 = time.perf_counter()
    offsets, nbrs, _deg = _king_graph(panel.n, pi, pj)
    kept, removed = king_prune_related_graph(offsets, nbrs)
    if timings is not None:
        timings.update(prune_s=time.perf_counter() - t0)
    return kept, removed, (pi, pj, b0, kin)


def king_unrelated_set_packed(packed, n_samples, kinship_threshold=KING_DEFAULT_KINSHIP_THRESHOLD, threads=0, timings=None):
    """`king_unrelated_set_from_packed`, src/math/KING.rs:745-753 -> (kept uint32 ascending, removed uint32 in removal order,
    edge_count, n_sites).  `threads` is accepted and unused."""
    n, m, t = _king_check_pairs_args(packed, n_samples, kinship_threshold)
    kept, removed, pairs = _king_unrelated_set(_panel(_king_payload2d(packed, n), n), t, timings)
    return kept, removed, int(pairs[0].shape[0]), m


def _king_from_bed(prefix, maf_threshold, max_missing_rate, het_threshold, snps_only, kinship_threshold):
    t = _king_threshold(kinship_threshold)
    pk, _miss, _maf, _std, _flip, _keep, n, _tot = prepare_bed_2bit_packed(prefix, float(maf_threshold), float(max_missing_rate),
                                                                           float(het_threshold), snps_only)
    n, m, t = _king_check_pairs_args(pk, n, t)
    kept, removed, pairs = _king_unrelated_set(_panel(pk, n), t)
    return kept, removed, pairs, m, n


def king_unrelated_set_from_bed(prefix, maf_threshold=0.01, max_missing_rate=0.1, het_threshold=0.0, snps_only=False,
                                kinship_threshold=KING_DEFAULT_KINSHIP_THRESHOLD, threads=0):
    """`king_unrelated_set_from_bed_py`, src/math/KING.rs:794-824: `prepare_bed_2bit_packed`, the related pairs, their graph and
    the greedy prune -> (kept uint32, removed uint32, edge_count, n_sites).  `threads` is accepted and unused."""
    kept, removed, pairs, m, _n = _king_from_bed(prefix, maf_threshold, max_missing_rate, het_threshold, snps_only, kinship_threshold)
    return kept, removed, int(pairs[0].shape[0]), m


def king_format_kinship(value):
    """Kinship as the `.king.kin0` table writes it: the shortest text that reads back to the same f64 (`repr`)."""
    return repr(float(value))


def write_king_tables(out, ids, n_sites, pairs, kept, removed):
    """`{out}.king.kin0` (TSV `ID1 ID2 NSNP IBS0 KINSHIP`, the related pairs in (i, j) order, NSNP = kept sites),
    `{out}.king.unrelated.id` (kept samples, ascending) and `{out}.king.related.id` (removed samples in removal order) -> paths."""
    pi, pj, b0, kin = pairs
    paths = [f"{out}.king.kin0", f"{out}.king.unrelated.id", f"{out}.king.related.id"]
    with open(paths[0], "w", encoding="utf-8") as fh:
        fh.write("ID1\tID2\tNSNP\tIBS0\tKINSHIP\n")
        fh.writelines(f"{ids[int(a)]}\t{ids[int(b)]}\t{int(n_sites)}\t{int(z)}\t{king_format_kinship(k)}\n"
                      for a, b, z, k in zip(pi, pj, b0, kin))
    for path, sel in ((paths[1], kept), (paths[2], removed)):
        with open(path, "w", encoding="utf-8") as fh:
            fh.writelines(f"{ids[int(s)]}\n" for s in sel)
    return paths


# ------------------------------------------------------------------------------------------------
# Neighbour-joining tree (src/stats/tree.rs): `jx tree -nj`, in tree.py
# ------------------------------------------------------------------------------------------------
from .tree import (geno_chunk_to_alignment_u8, geno_chunk_to_alignment_u8_siteinfo, geno_chunk_to_alignment_u8_sites,  # noqa: E402,F401
                   nj_merge_log, nj_newick_from_alignment_u8, nj_newick_from_distance_matrix, nj_newick_from_packed,
                   tree_from_bed, tree_jc69_distance, tree_pair_counts_packed)


# ------------------------------------------------------------------------------------------------
# FarmCPU, raw route (src/stats/farmcpu.rs:4153-5510): `jx gwas -farmcpu`, host half in farmcpu.py
# ------------------------------------------------------------------------------------------------

def _farmcpu_inputs(y, x_cov, packed, n_samples, row_flip, row_maf, sample_indices, row_indices, threshold):
    if int(n_samples) <= 0:
        raise RuntimeError("n_samples must be > 0")
    y = _c(y, np.float64).ravel()
    n = int(y.shape[0])
    if n == 0:
        raise RuntimeError("empty phenotype vector")
    x_cov = np.zeros((n, 0)) if x_cov is None else _c(x_cov, np.float64)
    if x_cov.ndim != 2:
        raise RuntimeError("x_cov must be 2D (n, p_cov)")
    if x_cov.shape[0] != n:
        raise RuntimeError(f"x_cov rows mismatch: got {x_cov.shape[0]}, expected n={n}")
    pk, _ptr_unused, m_packed = _payload(packed, n_samples)
    idx, n_sel = _opt_idx(sample_indices)
    if (n_sel if idx is not None else int(n_samples)) != n:
        raise RuntimeError(f"sample_indices length mismatch: got {n_sel if idx is not None else int(n_samples)}, "
                           f"expected len(y)={n}")
    if row_indices is None:
        rows = np.arange(m_packed, dtype=np.int64)
    else:
        rows = _c(row_indices, np.int64).ravel()
        if rows.size and (rows.min() < 0 or rows.max() >= m_packed):
            raise RuntimeError("row_indices out of range")
    m = int(rows.shape[0])
    if m == 0:
        raise RuntimeError("empty packed marker matrix")
    flip = np.asarray(row_flip).astype(bool).ravel()
    maf = _c(row_maf, np.float32).ravel()
    if flip.shape[0] != m or maf.shape[0] != m:
        raise RuntimeError(f"row metadata length mismatch: row_flip={flip.shape[0]}, row_maf={maf.shape[0]}, m={m}")
    thr = 1.0 / m if threshold is None else float(threshold)
    if not (np.isfinite(thr) and thr > 0.0):
        raise RuntimeError("threshold must be finite and > 0")
    x_base = np.ascontiguousarray(np.hstack([np.ones((n, 1)), x_cov]))
    return y, x_base, pk, idx, rows, flip, maf, thr


def farmcpu_packed(y, x_cov, packed, n_samples, row_flip, row_maf, chrom, pos, sample_indices=None, row_indices=None,
                   threshold=None, max_iter=30, qtn_bound=None, nbin=5, szbin=(5e5, 5e6, 5e7), stage1_progress_callback=None):
    """In-memory form of the raw FarmCPU route (an extension: the reference only writes files): `chrom` / `pos` per marker
    (after `row_indices`), threshold None = 1 / markers.  -> `farmcpu.FarmcpuResult`: stats (m, 3) [beta, se, p] of the final
    scan, the final QTN list (marker positions), the per-iteration trace (QTN set, winning (sz, nn), scores) and the missing
    counts."""
    from . import farmcpu as fc
    y, x_base, pk, idx, rows, flip, maf, thr = _farmcpu_inputs(y, x_cov, packed, n_samples, row_flip, row_maf, sample_indices,
                                                               row_indices, threshold)
    if len(chrom) != len(rows) or len(pos) != len(rows):
        raise RuntimeError(f"chrom / pos length mismatch: chrom={len(chrom)}, pos={len(pos)}, m={len(rows)}")
    return fc.run_raw(_panel(pk, n_samples, idx), rows, maf, flip, y, x_base, chrom, pos, thr, max_iter, qtn_bound, nbin, szbin,
                      stage1_progress_callback)


def farmcpu_packed_to_tsv(y, x_cov, packed, n_samples, row_flip, row_maf, row_missing, out_tsv, sample_indices=None,
                          row_indices=None, source_row_indices=None, threshold=1e-6, max_iter=30, qtn_bound=None, nbin=5,
                          szbin=(5e5, 5e6, 5e7), threads=0, stage1_progress_callback=None, progress_callback=None,
                          pseudo_tsv=None, bed_prefix=None, raw=False, skip_main_scan=False):
    """src/stats/farmcpu.rs:4127-5510 with the reference's signature; only `raw=True` is built (`-farmcpu`), the unified route
    and `skip_main_scan` are refused.  The marker metadata comes from `<bed_prefix>.bim` (rows `source_row_indices`, else
    `row_indices`); `pseudo_tsv` takes the QTN table when QTNs exist.  `threads` is accepted for signature parity.
    -> (rows written, QTN count, QTN rows written, stage 1 seconds, stage 2 seconds)."""
    from . import farmcpu as fc
    if not raw:
        raise RuntimeError("farmcpu_packed_to_tsv: the unified route (raw=False, -frgwas) is not built; pass raw=True (-farmcpu)")
    if skip_main_scan:
        raise RuntimeError("farmcpu_packed_to_tsv: skip_main_scan=True is not built")
    y, x_base, pk, idx, rows, flip, maf, thr = _farmcpu_inputs(y, x_cov, packed, n_samples, row_flip, row_maf, sample_indices,
                                                               row_indices, threshold)
    m = len(rows)
    if _c(row_missing, np.float32).ravel().shape[0] != m:
        raise RuntimeError(f"row metadata length mismatch: row_missing={_c(row_missing, np.float32).ravel().shape[0]}, m={m}")
    if source_row_indices is not None:
        meta_rows = _c(source_row_indices, np.int64).ravel()
        if meta_rows.shape[0] != m:
            raise RuntimeError(f"source_row_indices length mismatch: got {meta_rows.shape[0]}, expected {m}")
        if meta_rows.size and meta_rows.min() < 0:
            raise RuntimeError("source_row_indices must be non-negative")
    else:
        meta_rows = rows
    chrom, pos, snp, a0, a1 = _resolve_assoc_tsv_metadata(bed_prefix, [], [], [], [], [], meta_rows, m,
                                                          "FarmCPU streaming scan requires non-empty bed_prefix")
    res = fc.run_raw(_panel(pk, n_samples, idx), rows, maf, flip, y, x_base, chrom, pos, thr, max_iter, qtn_bound, nbin, szbin,
                     stage1_progress_callback)
    t0 = time.perf_counter()
    written = fc.write_main_tsv(out_tsv, chrom, pos, snp, a0, a1, maf, res.miss, res.stats)
    qtn_rows = 0
    if pseudo_tsv and res.qtn:
        qtn_rows = fc.write_qtn_tsv(pseudo_tsv, res.qtn, chrom, pos, snp, a0, a1, maf, res.miss, res.stats, rows)
    _done(progress_callback, m)
    return written, len(res.qtn), qtn_rows, res.stage1_secs, res.stage2_secs + (time.perf_counter() - t0)


# ---- multi-kernel AI-REML (src/stats/reml.rs:703-1049) ------------------------------------------------------------------------

def _reml_probe_signs(n, probes, seed):
    """The +-1 Hutchinson probes of reml.rs:798-806 -> (probes, n) f64, probe-major then sample.  Entry k of probe i is -1 when
    `rng.random::<f64>() < 0.5`; with rand 0.9's `(next_u64 >> 11) 2^-53` that is bit 63 of the u64 clear: the top bit of the
    SECOND u32 word of the pair.  The words come from `_stdrng_words`, so this inherits the "parity unpinned" status of the StdRng
    restatement (README, "Known differences"): it pins this build's stream, not the crate's."""
    n, probes = int(n), int(probes)
    w = _stdrng_words(seed, 2 * n * probes)
    hi = w[1::2]
    return np.where((hi >> np.uint32(31)) == 0, -1.0, 1.0).reshape(probes, n)


def ai_reml_multi_f64(k_stack, xcov, y, max_iter=100, tol=1e-6, min_var=1e-12, trace_probes=8, trace_seed=42, _fitter=None):
    """`ai_reml_multi_f64` (src/stats/reml.rs:703-1049): average-information REML over q n x n kernels plus the residual
    -> (theta ndarray (q + 1), ml, reml, used_iter, converged).  Literal to the source: the argument checks and their messages
    (RuntimeError, before any device call), the start value var(y) / (q + 1), the `max(min_var)` clamp, the 24-step halving with
    acceptance `reml_cand >= reml_curr - 1e-12`, the stop on the largest relative change < tol, and every early `break`, which
    returns the last values with converged = False.  `use_exact_trace = trace_probes == 0 or n <= 768`; otherwise the probes of
    `_reml_probe_signs` (parity with the crate's StdRng stream is unpinned, see there).  Every likelihood evaluation is
    `pipeline.MultiKernelReml.profile`, every step `ai_step`: V is formed, factored and solved on the device.
    `k_stack` may be a CUDA f64 tensor (an extension: kernels already in HBM are not staged through the host); `_fitter`, a
    `MultiKernelReml` built from the same arguments, is reused instead of building one (`blup.BLUP`)."""
    if not hasattr(k_stack, "shape"):
        k_stack = np.asarray(k_stack, dtype=np.float64)
    kshape = tuple(k_stack.shape)
    if len(kshape) != 3:
        raise RuntimeError("k_stack must be 3D (q, n, n)")
    q, n = int(kshape[0]), int(kshape[1])
    if int(kshape[2]) != n:
        raise RuntimeError("k_stack must be (q, n, n)")
    if q == 0:
        raise RuntimeError("k_stack requires at least one kernel")
    y = _c(y, np.float64).reshape(-1)
    if y.shape[0] != n:
        raise RuntimeError("len(y) must equal n in k_stack")
    x = _c(xcov, np.float64)
    if x.ndim != 2:
        raise RuntimeError("xcov must be 2D (n, p)")
    if x.shape[0] != n:
        raise RuntimeError("xcov.n_rows must equal n in k_stack")
    p = int(x.shape[1])
    if p == 0:
        raise RuntimeError("xcov must have at least one column")
    if n <= p:
        raise RuntimeError("n must be > p in xcov")
    min_var = float(min_var) if np.isfinite(min_var) and min_var > 0.0 else 1e-12
    tol = float(tol) if np.isfinite(tol) and tol > 0.0 else 1e-6
    trace_probes = int(trace_probes)
    use_exact_trace = trace_probes == 0 or n <= 768
    probes = None if use_exact_trace else _reml_probe_signs(n, max(trace_probes, 1), int(trace_seed))
    if _fitter is None:
        from . import pipeline
        _fitter = pipeline.MultiKernelReml(k_stack, x, y)
    fit = _fitter

    mean = float(np.sum(y)) / float(n)
    var_y = float(np.sum((y - mean) ** 2)) / float(max(n, 2) - 1)
    if not np.isfinite(var_y) or var_y <= 0.0:
        var_y = 1.0
    m = q + 1
    theta = np.full(m, max(var_y / float(m), min_var))
    converged, used_iter = False, 0
    last_ml = last_reml = float("nan")
    for it in range(int(max_iter)):
        used_iter = it + 1
        prof = fit.profile(theta)
        if prof is None:
            break
        reml_curr, ml_curr = prof[0], prof[1]
        last_reml, last_ml = reml_curr, ml_curr
        step_out = fit.ai_step(theta, probes)
        if step_out is None:
            break
        delta = step_out[2]
        accepted, step = False, 1.0
        theta_next, reml_next, ml_next = theta.copy(), reml_curr, ml_curr
        for _ in range(24):
            cand = np.maximum(theta + step * delta, min_var)
            pc = fit.profile(cand)
            if pc is not None and np.isfinite(pc[0]) and pc[0] >= reml_curr - 1e-12:
                accepted, theta_next, reml_next, ml_next = True, cand, pc[0], pc[1]
                break
            step *= 0.5
            if step < 1e-8:
                break
        if not accepted:
            break
        rel_max = float(np.max(np.abs(theta_next - theta) / np.maximum(theta, min_var)))
        theta, last_reml, last_ml = theta_next, reml_next, ml_next
        if rel_max < tol:
            converged = True
            break
    return np.asarray(theta, dtype=np.float64), float(last_ml), float(last_reml), int(used_iter), bool(converged)
