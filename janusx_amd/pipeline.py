"""HBM-resident end-to-end mixed-model pipeline: GRM -> eigh -> null REML -> per-SNP scan.

This is the path `bench.py` times and the multi-GPU driver shards.  torch is used only as plumbing (device
buffers, streams, `torch.distributed`); every computation is a libjxgpu kernel called through the C ABI.

Mirrors the reference's call stack for `jx gwas -lmm/-fvlmm`:
  build_grm_streaming (python/janusx/assoc/workflow.py:2928) -> grm_stream_bed_f32 (src/stats/grm.rs:4690)
  _gwas_eigh_from_grm (workflow.py:5509, ridge 1e-6)      -> rust_eigh_* (src/math/eigh.rs:1422)
  LMM._initialize_from_spectral (python/janusx/pyBLUP/assoc.py:1726-1876)
  lmm_reml_assoc_bed_to_tsv_f32 / fvlmm_assoc_bed_to_tsv_f32 (src/stats/lmm.rs:2513, src/stats/fvlmm.rs:2502)
"""
from __future__ import annotations

import copy
import math
import os
import time
import warnings
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch

from . import stats as st
from ._lib import check, lib

SCALE_EXP = 10  # U^T planes are scaled by 2^10 before the fp16 split (keeps the lo plane out of subnormals)
SERIES_CAP_BYTES = 8 << 30   # chain-series storage of the exact scan: rows per super-block = this / (8 (series + 1 + columns))
LM_BLOCK_ROWS = 1 << 20      # rows per launch (and per progress report) of the plain LM scan


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@dataclass
class NullFit:
    lbd: float
    ml0: float
    reml0: float
    sigma_g2: float
    sigma_e2: float
    pve: float
    bounds: tuple


@dataclass
class StageTimes:
    t: dict = field(default_factory=dict)

    def add(self, key, dt):
        self.t[key] = self.t.get(key, 0.0) + dt


class Panel:
    """A 2-bit genotype payload resident in HBM in the internal P32 tiling."""

    def __init__(self, packed: torch.Tensor, n_samples: int, sample_idx=None, p32_buffer=None):
        # p32_buffer: a (tiles, m, 32) uint8 device tensor of a previous Panel of the same shape to re-tile into (a caller that
        # re-tiles the same payload repeatedly -- bench.py's steps -- keeps the allocation out of its loop)
        assert packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 2
        self.device = packed.device
        self.m = int(packed.shape[0])
        self.n_src = int(n_samples)
        bps = int(packed.shape[1])
        if bps != (self.n_src + 3) // 4:
            raise RuntimeError(f"packed length mismatch: got {bps} bytes per SNP, expected {(self.n_src + 3) // 4}")
        idx_t = None
        if sample_idx is not None:
            idx = np.asarray(sample_idx, dtype=np.int64)
            if idx.size == 0:
                raise RuntimeError("sample_indices must not be empty")
            bad = idx[(idx < 0) | (idx >= self.n_src)]
            if bad.size:
                raise RuntimeError(f"sample index out of range: {int(bad[0])} >= {self.n_src}")
            if not (idx.size == self.n_src and np.array_equal(idx, np.arange(self.n_src))):
                idx_t = torch.from_numpy(idx.astype(np.int32)).to(self.device)
            self.n = int(idx.size)
        else:
            self.n = self.n_src
        self.nt = lib().jxg_num_tiles(self.n)
        self.npad = self.nt * 128
        if (p32_buffer is not None and tuple(p32_buffer.shape) == (self.nt, self.m, 32) and p32_buffer.dtype == torch.uint8
                and p32_buffer.device == self.device and p32_buffer.is_contiguous()):
            self.p32 = p32_buffer
        else:
            self.p32 = torch.empty((self.nt, self.m, 32), dtype=torch.uint8, device=self.device)
        check(lib().jxg_repack_p32(_ptr(packed), bps, self.n_src, self.m, _ptr(idx_t), self.n, None, self.m,
                                   _ptr(self.p32), _stream()))
        self._counts = None
        self._mean_missing = None
        self.sharded = False            # True: this payload is one rank's SNP shard of a larger panel (`payload_sharded`)

    def mean_missing(self) -> float:
        """Mean number of missing calls per row over the rows of the payload that CAN pass a quality filter (at most n / 10
        missing calls: a few percent of mostly-missing junk rows must not push every kept row into the dense missing-call form;
        ADVICE r4), cached: the call-independent statistic behind the choice of the rotation path for rows with a few missing
        calls (`jxg_rot_miss_max`).  Under a distributed run the sum and
        the row count are added over the ranks, so that every rank of a payload-sharded scan decides from the same number (with
        a replicated payload every rank already holds the same rows)."""
        if self._mean_missing is None:
            c = self.counts()
            mi = c[:, 0].astype(np.float64) if len(c) else np.zeros(0)
            ok = mi <= self.n / 10.0
            tot = np.array([float(mi[ok].sum()), float(np.count_nonzero(ok))], dtype=np.float64)
            if self.sharded:
                from . import dist as jd
                rank, world = dist_info()
                if world > 1:
                    t = torch.from_numpy(tot)
                    if torch.distributed.get_backend() == "nccl":
                        t = t.to(self.device)
                    jd.allreduce_sum_(t)
                    tot = t.cpu().numpy()
            self._mean_missing = float(tot[0] / tot[1]) if tot[1] > 0 else 0.0
        return self._mean_missing

    def counts(self) -> np.ndarray:
        """(m,3) int32 (missing, het, hom_alt) over the selected samples (host copy, cached)."""
        if self._counts is None:
            c = torch.empty((self.m, 3), dtype=torch.int32, device=self.device)
            check(lib().jxg_row_counts_p32(_ptr(self.p32), self.m, self.n, _ptr(c), _stream()))
            self._counts = c.cpu().numpy()
        return self._counts


def grm_accumulate(panel: Panel, rows: np.ndarray, lut: np.ndarray, acc: torch.Tensor = None, kchunk=0):
    """acc (npad,npad) f64 += Z Z^T over the given SNP rows with their (len(rows),4) f32 value LUT."""
    dev = panel.device
    if acc is None:
        acc = torch.zeros((panel.npad, panel.npad), dtype=torch.float64, device=dev)
    if len(rows) == 0:
        return acc
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    lut_t = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(dev)
    check(lib().jxg_grm_accumulate(_ptr(panel.p32), panel.m, panel.n, _ptr(rows_t), _ptr(lut_t), len(rows),
                                   _ptr(acc), int(kchunk), 0, _stream()))
    return acc


def grm_finalize(acc: torch.Tensor, n: int, scale: float, dtype=torch.float32):
    out = torch.empty((n, n), dtype=dtype, device=acc.device)
    check(lib().jxg_grm_finalize(_ptr(acc), n, 1.0 / float(scale), _ptr(out), 1 if dtype == torch.float64 else 0,
                                 _stream()))
    return out


_DIST_EIGH = {}   # keeps the ctypes callback and the staging tensor alive


def dist_info():
    """(rank, world) of the initialised torch.distributed group; (0, 1) without one (or with a single rank)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init_distributed(eigh_min_n: int = 16384):
    """Call once per process after `torch.distributed.init_process_group` (one process per GPU; backend "nccl" = RCCL over
    xGMI, "gloo" in the functional tests): switches the rank-aware forms of `build_grm` / `run_trait` / `run_gwas` on (they
    look at the process group themselves) and distributes the eigendecomposition (`enable_distributed_eigh`).
    SURVEY.md 8(e): SNP ranges per rank for the GRM, one sum-reduction of the partial accumulators, eigenvectors sharded over
    the ranks, SNP-sharded scan, results gathered in BED order.  -> (rank, world)."""
    rank, world = dist_info()
    if world > 1 and os.environ.get("JXGPU_DIST_EIGH", "1") != "0":
        enable_distributed_eigh(eigh_min_n)
    return rank, world


def _my_slice(count: int, payload_sharded: bool):
    """This rank's contiguous share [lo, hi) of `count` work items (all of them when the payload itself is the rank's shard)."""
    rank, world = dist_info()
    if world == 1 or payload_sharded:
        return 0, count
    from .dist import shard_range
    return shard_range(count, rank, world)


def _allgather_rows(t: torch.Tensor) -> torch.Tensor:
    """Per-rank (rows_r, ...) tensors concatenated in rank order on every rank (= BED order of contiguous SNP shards)."""
    from .dist import gather_rows
    import torch.distributed as dist
    if dist_info()[1] == 1:
        return t
    if t.is_cuda and dist.get_backend() != "nccl":
        return gather_rows(t.cpu()).to(t.device)         # functional multi-rank mode on shared GPUs (gloo): through host memory
    return gather_rows(t)


gather_results = _allgather_rows


def _allgather_np(a: np.ndarray) -> np.ndarray:
    if dist_info()[1] == 1:
        return a
    import torch.distributed as dist
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dist.get_backend() == "nccl":
        return _allgather_rows(t.to(torch.device("cuda", torch.cuda.current_device()))).cpu().numpy()
    from .dist import gather_rows
    return gather_rows(t).numpy()


def enable_distributed_eigh(min_n: int = 0):
    """Distribute the eigendecomposition over the ranks of the initialised torch.distributed group (every rank must then
    call `eigh_from_grm` on the same matrix).  Two-stage path (n >= 10000, the default there): the reduction stages and
    the divide and conquer run replicated -- their kernels are bit-reproducible, so the replicas agree --, every rank
    back-transforms its n / world eigenvectors (two thirds of the flops) and one broadcast per rank (RCCL over xGMI with
    the nccl backend) completes U on every rank.  One-stage path (JXGPU_DIST_EIGH_ONESTAGE=1, or n below the two-stage
    threshold): per column each rank streams 1 / world of the trailing-matrix tiles of the symv and one all-reduce sums
    the partial products, from `min_n` rows (default 16384: below that a column is launch-latency-bound and the
    collective costs more than it saves)."""
    import ctypes as C
    import torch.distributed as dist
    from .dist import allreduce_sum_, broadcast_
    import os
    force_single = os.environ.get("JXGPU_DIST_EIGH_FORCE", "0") not in ("", "0")   # one-rank run of the same code path
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not force_single):
        check(lib().jxg_eigh_set_dist(0, 1, None, None, None, 0, 0))
        check(lib().jxg_eigh_set_gather(None, None))
        check(lib().jxg_eigh_set_agree(None, None))
        check(lib().jxg_eigh_set_band_dist(0, 1, None, None, None, 0, 0, 0))
        _DIST_EIGH.clear()
        return False
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda", torch.cuda.current_device())
    state = {"staging": None}

    def _cb(_user):
        try:
            allreduce_sum_(state["staging"])
            return 0
        except Exception as e:   # noqa: BLE001 - reported through the C status
            import sys
            print(f"distributed eigh: all-reduce failed on rank {rank}: {e!r}", file=sys.stderr, flush=True)
            return 1

    cb = C.CFUNCTYPE(C.c_int, C.c_void_p)(_cb)

    def _gather(_user):
        # two-stage path: every rank has back-transformed the eigenvectors [n r / world, n (r + 1) / world) (rows of the
        # row-major result); one broadcast per rank completes the matrix on every rank (RCCL over xGMI with nccl)
        try:
            a = state["out"]
            n = int(a.shape[0])
            for r in range(world):
                r0, r1 = (n * r) // world, (n * (r + 1)) // world
                if r1 > r0:
                    broadcast_(a[r0:r1], r)
            return 0
        except Exception as e:   # noqa: BLE001 - reported through the C status
            import sys
            print(f"distributed eigh: gather failed on rank {rank}: {e!r}", file=sys.stderr, flush=True)
            return 1

    gcb = C.CFUNCTYPE(C.c_int, C.c_void_p)(_gather)
    check(lib().jxg_eigh_set_gather(C.cast(gcb, C.c_void_p) if world > 1 else None, None))

    def _agree(_user, checksum):
        # the replicated stages must have produced the same bits on every rank before rows of different ranks are mixed:
        # MIN and MAX of the 64-bit checksum (as two 32-bit halves in int64 lanes) over the ranks
        try:
            cs = int(checksum) & 0xFFFFFFFFFFFFFFFF
            # test hook: this rank pretends to hold different bits (the replicated results' checksum only -- the failure flags of
            # the reduction stages, compared through the same callback, are 0 or the constant below)
            if os.environ.get("JXGPU_DIST_EIGH_TEST_DISAGREE", "") == str(rank) and cs not in (0, 0x9E3779B97F4A7C15):
                cs ^= 1
            v = torch.tensor([cs >> 32, cs & 0xFFFFFFFF], dtype=torch.int64)
            lo, hi = v.clone(), v.clone()
            if dist.get_backend() == "nccl":
                lo, hi = lo.to(dev), hi.to(dev)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            return 1 if bool((lo == hi).all()) else 0
        except Exception as e:   # noqa: BLE001 - reported through the C status
            import sys
            print(f"distributed eigh: agreement check failed on rank {rank}: {e!r}", file=sys.stderr, flush=True)
            return -1

    acb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)(_agree)
    check(lib().jxg_eigh_set_agree(C.cast(acb, C.c_void_p) if world > 1 else None, None))

    def _band(_user, count):
        # band reduction with the trailing matrix sharded over the ranks (k_sy2sb.hip): per panel the partial products Z = A22 V
        # and the gather of the next panel's block column are summed over the ranks (RCCL over xGMI with nccl, on the stream
        # the eigensolver runs on)
        try:
            t = state["band_staging"][: int(count)]
            if world > 1:
                allreduce_sum_(t)
            elif dist.get_backend() == "nccl":
                dist.all_reduce(t)      # one-rank run of the same code path (JXGPU_DIST_EIGH_FORCE): the RCCL call itself
            return 0
        except Exception as e:   # noqa: BLE001 - reported through the C status
            import sys
            print(f"distributed eigh: band all-reduce failed on rank {rank}: {e!r}", file=sys.stderr, flush=True)
            return 1

    bcb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64)(_band)
    band_on = os.environ.get("JXGPU_DIST_BAND", "1") != "0"
    band_min_n = int(os.environ.get("JXGPU_DIST_BAND_MIN_N", "8192"))
    band_block = int(os.environ.get("JXGPU_DIST_BAND_BLOCK", "2048"))

    def prepare(n):
        need = int(lib().jxg_eigh_dist_staging_doubles(int(n)))
        if state["staging"] is None or state["staging"].numel() != need:
            state["staging"] = torch.zeros(need, dtype=torch.float64, device=dev)
            check(lib().jxg_eigh_set_dist(rank, world, C.cast(cb, C.c_void_p), None, _ptr(state["staging"]), need,
                                          int(min_n)))
        if band_on and int(n) >= band_min_n:
            # block size first (it sizes the staging buffer), then the buffer itself
            check(lib().jxg_eigh_set_band_dist(rank, world, None, None, None, 0, band_min_n, band_block))
            bneed = int(lib().jxg_eigh_band_staging_doubles(int(n)))
            if state.get("band_staging") is None or state["band_staging"].numel() < bneed:
                state["band_staging"] = torch.zeros(bneed, dtype=torch.float64, device=dev)
            check(lib().jxg_eigh_set_band_dist(rank, world, C.cast(bcb, C.c_void_p), None, _ptr(state["band_staging"]),
                                               int(state["band_staging"].numel()), band_min_n, band_block))
        else:
            check(lib().jxg_eigh_set_band_dist(rank, world, None, None, None, 0, band_min_n, band_block))

    _DIST_EIGH.update(cb=cb, gcb=gcb, acb=acb, bcb=bcb, state=state, prepare=prepare)
    return True


LAST_EIGH = {"planes": 0}      # digit planes of the sliced int8 products in the last eigh_from_grm call


def eigh_from_grm(k: torch.Tensor, ridge=1e-6, subset_idx=None, f32_consumer=False):
    """K (n,n) f32/f64 on device -> (S f64 (k), U^T f64 (k,k) row j = eigenvector j).
    f32_consumer: the caller keeps the eigenvectors only as the f32 U^T of the scan (`SpectralModel`, the reference's `Dh`,
    python/janusx/pyBLUP/assoc.py:1817; src/stats/reml.rs:109-198): the sliced int8 products of the Q1 back-transformation and of
    the divide-and-conquer merges then run with 5 digit planes (15 products) instead of 6 (21) -- orthogonality of U 4e-10
    instead of 2e-12 at n = 20 000, six times below the 2.6e-9 the f32 rounding of the kept copy leaves by itself; eigenvalues unchanged
    (JXGPU_OZ_PLANES, when set, decides alone; JXGPU_EIGH_F32_PLANES=0 keeps 6)."""
    dev = k.device
    n = int(k.shape[0])
    idx = np.arange(n, dtype=np.int32) if subset_idx is None else np.asarray(subset_idx, dtype=np.int32)
    kk = int(idx.shape[0])
    idx_t = torch.from_numpy(idx).to(dev)
    a = torch.empty((kk, kk), dtype=torch.float64, device=dev)
    check(lib().jxg_gather_sub_f64(_ptr(k), 1 if k.dtype == torch.float64 else 0, n, _ptr(idx_t), kk, _ptr(a),
                                   _stream()))
    check(lib().jxg_symmetrize_f64(_ptr(a), kk, _stream()))
    w = torch.empty(kk, dtype=torch.float64, device=dev)
    if _DIST_EIGH:
        _DIST_EIGH["prepare"](kk)   # staging buffer of the per-column all-reduce (sized by n)
        _DIST_EIGH["state"]["out"] = a   # the gather callback of the two-stage path completes this tensor
    five = bool(f32_consumer) and not os.environ.get("JXGPU_OZ_PLANES") and os.environ.get("JXGPU_EIGH_F32_PLANES", "5") == "5"
    prev = lib().jxg_oz_set_planes(5) if five else 0
    try:
        LAST_EIGH["planes"] = int(lib().jxg_oz_planes())      # what bench.py prices the Q1 stage on
        check(lib().jxg_eigh_f64(_ptr(a), kk, float(ridge), _ptr(w), _stream()))
    finally:
        if five:
            lib().jxg_oz_set_planes(prev)
    return w, a


class SpectralModel:
    """Device-resident counterpart of `LMM.from_spectral` (python/janusx/pyBLUP/assoc.py:1702-1876)."""

    def __init__(self, s: torch.Tensor, ut64: torch.Tensor, x: np.ndarray, y: np.ndarray, fit_null: bool = True):
        dev = s.device
        self.n = n = int(s.shape[0])
        self.S = s
        self.ut = torch.empty((n, n), dtype=torch.float32, device=dev)  # Dh = float32(U^T)
        check(lib().jxg_cast_f64_to_f32(_ptr(ut64), _ptr(self.ut), n * n, _stream()))
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if x.ndim != 2 or x.shape[0] != n or y.shape[0] != n:
            raise RuntimeError(f"design row mismatch: got {x.shape[0]}, expected {n}")
        self.p = p = int(x.shape[1])
        xy = torch.from_numpy(np.concatenate([x, y[:, None]], axis=1)).to(dev)
        rot = torch.empty_like(xy)
        check(lib().jxg_rotate_xy(_ptr(self.ut), n, _ptr(xy), p + 1, _ptr(rot), _stream()))
        self.xcov = rot[:, :p].contiguous()
        self.y = rot[:, p].contiguous()
        self._planes = None
        self._fv = None
        if not fit_null:      # spectrum of a sparse (possibly indefinite) K: lambda comes from the sparse REML search
            self.null = None
            return
        self.null = self._profile(*self.reml_null())

    @classmethod
    def rotated(cls, s, u_t, xcov, y, device):
        """A model from what a caller has rotated already (the mirror's packed and dense-chunk entry points): s (n) f64, u_t (n, n)
        f32 row-major U^T kept as given (None: the rows to scan are rotated already), X~ (n, p) and y~ (n) f64, host arrays or torch
        tensors.  No rotation and no null fit (null = None)."""
        def dev(a, dtype):
            if a is None:
                return None
            if torch.is_tensor(a):           # parts that are on a device already
                return a.to(device=device, dtype=torch.float64 if dtype == np.float64 else torch.float32).contiguous()
            a = np.ascontiguousarray(a, dtype=dtype)
            return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)
        self = cls.__new__(cls)
        self.S, self.ut, self.xcov, self.y = dev(s, np.float64), dev(u_t, np.float32), dev(xcov, np.float64), dev(y, np.float64)
        self.n, self.p = int(self.S.shape[0]), int(self.xcov.shape[1])
        self.null = self._planes = self._fv = None
        return self

    @classmethod
    def for_traits(cls, s: torch.Tensor, ut64: torch.Tensor, x: np.ndarray, Y: np.ndarray):
        """The models of T traits on the same samples and design (trait-level LMM): ONE cast of U^T and ONE rotation of
        [X | Y] (n x (p + T)); the models share S, `ut`, `xcov` and -- through the first one, which the rotation stage is built
        from -- the planes of U^T; each has its own y~ and null fit (-5, 5, 50, 1e-3 as the constructor).  Y: (T, n).
        -> list of T models."""
        dev = s.device
        x = np.ascontiguousarray(x, dtype=np.float64)
        Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.float64)))
        n = int(s.shape[0])
        if x.ndim != 2 or x.shape[0] != n or Y.shape[1] != n:
            raise RuntimeError(f"design row mismatch: got {x.shape[0]} / {Y.shape[1]}, expected {n}")
        p, nt = int(x.shape[1]), int(Y.shape[0])
        base = cls.__new__(cls)
        base.n, base.p, base.S = n, p, s
        base.ut = torch.empty((n, n), dtype=torch.float32, device=dev)
        check(lib().jxg_cast_f64_to_f32(_ptr(ut64), _ptr(base.ut), n * n, _stream()))
        cols = np.concatenate([x, Y.T], axis=1)
        parts = []
        for c0 in range(0, p + nt, 16):                       # jxg_rotate_xy takes up to 16 columns
            xy = torch.from_numpy(np.ascontiguousarray(cols[:, c0:c0 + 16])).to(dev)
            part = torch.empty_like(xy)
            check(lib().jxg_rotate_xy(_ptr(base.ut), n, _ptr(xy), int(xy.shape[1]), _ptr(part), _stream()))
            parts.append(part)
        rot = torch.cat(parts, dim=1)
        base.xcov = rot[:, :p].contiguous()
        base.y_rot = rot[:, p:].t().contiguous()              # (T, n): every trait's y~
        base.null = base._planes = base._fv = None
        models = []
        for ti in range(nt):
            mdl = base if ti == 0 else copy.copy(base)
            mdl.y = base.y_rot[ti]
            mdl.null = mdl._profile(*mdl.reml_null())
            models.append(mdl)
        return models

    def reml_null(self, low=-5.0, high=5.0, max_iter=50, tol=1e-3):
        """-> (lambda0, ml0, reml0): Brent on -reml_loglike of the null model (`lmm_reml_null_f32`, src/stats/reml.rs:570-616)."""
        out3 = torch.empty(3, dtype=torch.float64, device=self.S.device)
        check(lib().jxg_lmm_reml_null(_ptr(self.S), _ptr(self.xcov), _ptr(self.y), self.n, self.p, float(low), float(high),
                                      int(max_iter), float(tol), _ptr(out3), _stream()))
        return tuple(float(v) for v in out3.cpu().numpy())

    def loglike_null(self, log10_lbd):
        """-> (ml, reml) of the null model at log10 lambda, -1e8 on failure (src/stats/reml.rs:255-470)."""
        out2 = torch.empty(2, dtype=torch.float64, device=self.S.device)
        check(lib().jxg_lmm_loglike_null(_ptr(self.S), _ptr(self.xcov), _ptr(self.y), self.n, self.p, float(log10_lbd),
                                         _ptr(out2), _stream()))
        return tuple(float(v) for v in out2.cpu().numpy())

    def _profile(self, lbd, ml0, reml0) -> NullFit:
        # assoc.py:907-951 `_lmm_profile_exact_vc` + :1845-1876 (host, O(n p^2))
        s = np.maximum(self.S.cpu().numpy(), 0.0)
        x = self.xcov.cpu().numpy()
        y = self.y.cpu().numpy()
        n, p = x.shape
        sg2 = se2 = float("nan")
        if math.isfinite(lbd) and lbd > 0.0 and n - p > 0:
            v_inv = 1.0 / np.maximum(s + lbd, 1e-30)
            a = (x.T * v_inv) @ x
            b = (x.T * v_inv) @ y
            try:
                beta = np.linalg.solve(a, b)
            except np.linalg.LinAlgError:
                beta = np.linalg.lstsq(a, b, rcond=None)[0]
            r = y - x @ beta
            q = float(np.dot(v_inv, r * r))
            if math.isfinite(q) and q > 0.0:
                sg2 = q / float(n - p)
                se2 = lbd * sg2
        trace_mean = float(np.sum(s) / float(max(1, n)))
        ssum = sg2 + se2
        if math.isfinite(ssum) and ssum > 0.0:
            vg = sg2 * max(trace_mean, 0.0)
            den = vg + se2
            pve = vg / den if (math.isfinite(den) and den > 0.0) else sg2 / ssum
        else:
            vg0 = float(np.mean(s))
            pve = vg0 / (vg0 + lbd) if (vg0 + lbd) > 0 else float("nan")
        if pve > 0.95 or pve < 0.05 or (not math.isfinite(lbd)) or lbd <= 0.0:
            bounds = (-5.0, 5.0)
        else:
            bounds = (math.log10(lbd) - 2.0, math.log10(lbd) + 2.0)
        return NullFit(lbd, ml0, reml0, sg2, se2, pve, bounds)

    def planes(self):
        if self._planes is None:
            nt = lib().jxg_num_tiles(self.n)
            npad = nt * 128
            hi = torch.empty((npad, npad), dtype=torch.float16, device=self.S.device)
            lo = torch.empty((npad, npad), dtype=torch.float16, device=self.S.device)
            check(lib().jxg_ut_split(_ptr(self.ut), self.n, _ptr(hi), _ptr(lo), SCALE_EXP, _stream()))
            usum = torch.empty(npad, dtype=torch.float32, device=self.S.device)   # sum_i u_t[j][i]: affine term of exact rows
            check(lib().jxg_ut_rowsum(_ptr(self.ut), self.n, _ptr(usum), _stream()))
            self._planes = (hi, lo, usum)
        return self._planes

    def qplanes(self):
        """Three int8 planes of U^T with one scale per eigenvector (jxg_ut_quant3): operands of the int8 rotation of exact
        design rows (csrc/k_rotate_i8.hip)."""
        if getattr(self, "_qplanes", None) is None:
            npad = lib().jxg_num_tiles(self.n) * 128
            q = torch.empty((3, npad, npad), dtype=torch.int8, device=self.S.device)
            umax = torch.empty(npad, dtype=torch.float32, device=self.S.device)
            check(lib().jxg_ut_quant3(_ptr(self.ut), self.n, _ptr(q), _ptr(umax), _stream()))
            self._qplanes = (q, umax)
        return self._qplanes

    def usamp(self):
        """U with one row per sample (the transpose of `ut`, f32): what the missing-call term of the rotation gathers from
        (jxg_rotate_missing_correct)."""
        if getattr(self, "_usamp", None) is None:
            us = torch.empty((self.n, self.n), dtype=torch.float32, device=self.S.device)
            check(lib().jxg_transpose_f32(_ptr(self.ut), self.n, _ptr(us), _stream()))
            self._usamp = us
        return self._usamp

    def warm_seed(self):
        """log10 lambda0 clamped into the null bounds: the start of the per-SNP searches and the null ML; None unless lambda0 > 0."""
        lo_b, hi_b = self.null.bounds
        return min(max(math.log10(self.null.lbd), lo_b), hi_b) if self.null.lbd > 0 else None

    def null_ml(self, max_iter, tol, bounds=None, init=None):
        """-> (seed, null ML of the lmm2 scan): Brent on -ml_loglike, seeded with the REML optimum (src/stats/lmm.rs:2902-2921; the
        workflow passes bounds, max_iter = 30, tol = 1e-2, init_log10_lbd_reml = log10 lambda0: workflow_model_stream.py:1499-1590).
        bounds (low, high) and init: the caller's own (a model without a null fit); default: those of the null fit."""
        o2 = torch.empty(2, dtype=torch.float64, device=self.S.device)
        if bounds is None:
            bounds, init = self.null.bounds, self.warm_seed()
        lo_b, hi_b = float(bounds[0]), float(bounds[1])
        check(lib().jxg_lmm2_null_ml(_ptr(self.S), _ptr(self.xcov), _ptr(self.y), self.n, self.p, lo_b, hi_b, int(max_iter),
                                     float(tol), 1 if init is not None else 0, float(init or 0.0), o2.data_ptr(), _stream()))
        ml0 = float(o2.cpu().numpy()[1])
        if not math.isfinite(ml0):
            raise RuntimeError("failed to optimize null ML for LMM2 unified scan")
        return init, ml0

    def fv_cache(self, log10_lbd=None):
        lbd = self.null.lbd if log10_lbd is None else 10.0 ** float(log10_lbd)
        if self._fv is None or self._fv[0] != lbd:
            dev = self.S.device
            n, p = self.n, self.p
            w = torch.empty(n, dtype=torch.float32, device=dev)
            py = torch.empty(n, dtype=torch.float32, device=dev)
            wx = torch.empty((n, p), dtype=torch.float32, device=dev)
            a = np.zeros((p, p), dtype=np.float64)
            sc = np.zeros(3, dtype=np.float64)
            torch.cuda.current_stream().synchronize()
            check(lib().jxg_fvlmm_prepare(_ptr(self.S), _ptr(self.xcov), _ptr(self.y), n, p, float(lbd), _ptr(w),
                                          _ptr(py), _ptr(wx), a.ctypes.data, sc.ctypes.data))
            self._fv = (lbd, w, py, wx, a, float(sc[0]), float(sc[1]), int(sc[2]))
        return self._fv


def _fused_fixed_lambda(p: int) -> bool:
    """The fixed-lambda scans (fvlmm, SparseLMM exact) reduce the rotated tile inside the rotation kernel's epilogue
    (`jxg_rotate_packed16x_fused` + `jxg_fvlmm_finish_dev`) instead of writing and re-reading G~ (4 m n bytes each way);
    JXGPU_FVLMM_FUSED=0 keeps the two-kernel form, more than 8 covariates always do."""
    return p <= 8 and os.environ.get("JXGPU_FVLMM_FUSED", "1").strip() != "0"


def _chain_segments(co, a, b, dev):
    """The warm-start chains (offsets `co`) that touch the rows [a, b) -> (index of the first one, their offsets relative to a,
    clipped to [0, b - a], as an int32 device tensor)."""
    nch = len(co) - 1
    c0 = min(int(np.searchsorted(co, a, side="right")) - 1, nch - 1)
    c1 = c0
    loc = []
    while c1 < nch and co[c1] < b:
        loc.append(max(int(co[c1]), a) - a)
        c1 += 1
    loc.append(min(int(co[c1]), b) - a)
    return c0, torch.from_numpy(np.asarray(loc, dtype=np.int32)).to(dev)


def _block_positions(mask, br, dev):
    """Per block of `br` rows the positions inside the block at which `mask` holds -> per block (int32 device tensor of them, a
    view of one upload, or None; their number)."""
    parts = [np.flatnonzero(mask[b0:b0 + br]).astype(np.int32) for b0 in range(0, len(mask), br)]
    t = torch.from_numpy(np.concatenate(parts)).to(dev)
    ends = np.cumsum([len(a) for a in parts]).tolist()
    return [(t[e - len(a):] if len(a) else None, len(a)) for a, e in zip(parts, ends)]


class _Fp16Rotation:
    """What the two rotation stages share: rows and LUT records of a call on the device, and the fp16 hi / lo launches over the
    `parts` (offset, nb, hi, lo, panel) of an eigenbasis -- one part for a dense basis, the diagonal blocks otherwise."""
    int8 = False
    fused_ok = True        # `fused_sums` exists: `_fixed_lambda_scan` may take the sums instead of G~

    def _upload(self, rows, lut, dev):
        self.rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        self.lut16 = torch.empty((len(rows), 16), dtype=torch.uint8, device=dev)
        return torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(dev)

    def rotate(self, grot, r0, nr, rowoff_p=None, usum_p=None):
        """G~ of the rows [r0, r0 + nr) -> grot (>= nr, n) f32: every part writes its columns."""
        rows_p, lut_p = self.rows_t[r0:].data_ptr(), self.lut16[r0:].data_ptr()
        for off, nb, hi, lo, panel in self.parts:
            check(lib().jxg_rotate_packed16x_ld(_ptr(panel.p32), panel.m, nb, rows_p, nr, lut_p, rowoff_p, usum_p, _ptr(hi), _ptr(lo),
                                                SCALE_EXP, grot[:, off:].data_ptr(), self.n, _stream()))

    def fused_sums(self, sums, r0, nr, w, py, wx, p, rowoff_p=None, usum_p=None):
        """Fused sums of the rows [r0, r0 + nr) against w, Py~, WX~ -> sums (tiles, >= nr, p + 2) f64; G~ is never written."""
        rows_p, lut_p = self.rows_t[r0:].data_ptr(), self.lut16[r0:].data_ptr()
        t0 = 0
        for off, nb, hi, lo, panel in self.parts:
            check(lib().jxg_rotate_packed16x_fused(_ptr(panel.p32), panel.m, nb, rows_p, nr, lut_p, rowoff_p, usum_p, _ptr(hi),
                                                   _ptr(lo), SCALE_EXP, w[off:].data_ptr(), py[off:].data_ptr(), wx[off:].data_ptr(),
                                                   p, _ptr(sums), p + 2, t0, _stream()))
            t0 += panel.nt


class DenseRotation(_Fp16Rotation):
    """Rotation stage of a dense eigenbasis for the SNP rows of one call in blocks of `block_rows`: what decides the kernel a row
    takes is fixed here, once; `rotate` / `fused_sums` then only launch (no allocation, no host sync), and a row gets the same bits
    whatever block, chunk or rank it lands in.  fixed_lambda: for fvlmm / SparseLMM exact; int8=False: the fp16 kernel at every n."""

    def __init__(self, panel: Panel, model: SpectralModel, rows, lut, block_rows, fixed_lambda=False, int8=True):
        dev, mk, n, br = panel.device, len(rows), model.n, int(block_rows)
        self.panel, self.n, self.br, self.tiles = panel, n, br, panel.nt
        lut_t = self._upload(rows, lut, dev)
        self.hi, self.lo, self.usum = model.planes()
        self.parts = [(0, n, self.hi, self.lo, panel)]
        # int8 planes of the eigenvectors for the exact-row tiles of full-size blocks (k_rotate_i8.hip)
        # From n = 4096 the int8 / 256-tile rotation kernels write G~ and the fixed-lambda scans read it back (10 ms per 200 000
        # SNPs at n = 20 000) instead of the fused epilogue of the 128-tile fp16 kernel: 225 vs 360 ms for the scan of `-fvlmm` at
        # BASELINE configs[2].  JXGPU_FVLMM_FUSED=2 keeps the fused form at every size.
        use_q = int8 and n >= 4096 and os.environ.get("JXGPU_ROT_I8", "1") != "0"
        if fixed_lambda and os.environ.get("JXGPU_FVLMM_FUSED", "1").strip() == "2" and _fused_fixed_lambda(model.p):
            use_q = False
        self.int8, self.qpl = use_q, (model.qplanes() if use_q else None)
        self.fused_ok = not use_q
        # fp16 hi/lo LUT records (range-checked; rows without missing calls as integer LUT + offset, see jxg_lut_split_rows)
        self.rowoff = torch.empty(mk, dtype=torch.float32, device=dev)
        # rows with a few missing calls keep the exact (int8) rotation and get their missing-call term added behind it
        # (jxg_rotate_missing_correct: d * the sum of the missing samples' rows of U); only where the int8 rotation runs
        # The limit is decided from a statistic of the PANEL (mean missing calls over all its rows, cached), never from the rows of
        # this call: a row takes the same path -- and gets the same bits -- in chunked, unchunked and rank-sharded scans (the mirror's
        # packed entry points build their panel from the rows they are handed).
        miss_max = int(lib().jxg_rot_miss_max(n, panel.mean_missing())) if use_q else 0
        rowmiss = torch.zeros(mk, dtype=torch.float32, device=dev) if miss_max > 0 else None
        check(lib().jxg_lut_split_rows_m(_ptr(panel.p32), panel.m, n, _ptr(self.rows_t), _ptr(lut_t), mk, _ptr(self.lut16),
                                         _ptr(self.rowoff), _ptr(rowmiss), miss_max, _stream()))
        self.rowmiss = rowmiss = rowmiss if (rowmiss is not None and bool((rowmiss != 0).any().item())) else None
        # the missing-call term as one more int8 product (jxg_rotate_missing_dense) when the limit is "none" (> 256: more than n / 300
        # missing calls per row on average), else as a gather per missing call over U with one row per sample
        self.miss_dense = rowmiss is not None and miss_max > 256
        self.usamp = model.usamp() if (rowmiss is not None and not self.miss_dense) else None
        # per block: positions of the rows with a missing-call term, of the exact rows (finite row offset: int8 rotation) and of
        # the others (fp16 rotation); a row's path does not depend on the blocking, so chunked scans stay bit-identical to
        # unchunked ones
        self.sel_miss = _block_positions((rowmiss != 0).cpu().numpy(), br, dev) if self.miss_dense else None
        if use_q and int(torch.isnan(self.rowoff).sum().item()) == 0:
            # every row exact (a panel without missing calls): identity lists (NULL), nothing to build
            self.sel_exact = [(None, min(br, mk - b0)) for b0 in range(0, mk, br)]
            self.sel_rest = [(None, 0)] * len(self.sel_exact)
        elif use_q:
            ex = ~np.isnan(self.rowoff.cpu().numpy())
            self.sel_exact, self.sel_rest = _block_positions(ex, br, dev), _block_positions(~ex, br, dev)

    def rotate(self, grot, r0, nr):
        panel, n = self.panel, self.n
        rows_p, lut_p, off_p = self.rows_t[r0:].data_ptr(), self.lut16[r0:].data_ptr(), self.rowoff[r0:].data_ptr()
        if not self.int8:
            return super().rotate(grot, r0, nr, off_p, _ptr(self.usum))
        bi = r0 // self.br
        (ex, ne), (rs, nx) = self.sel_exact[bi], self.sel_rest[bi]
        check(lib().jxg_rotate_packed16x_q(_ptr(panel.p32), panel.m, n, rows_p, nr, lut_p, off_p, _ptr(self.usum), _ptr(self.hi),
                                           _ptr(self.lo), SCALE_EXP, _ptr(self.qpl[0]), _ptr(self.qpl[1]), _ptr(ex), ne, _ptr(rs), nx,
                                           _ptr(grot), _stream()))
        if self.miss_dense:
            sel, nm = self.sel_miss[bi]
            if nm > 0:
                check(lib().jxg_rotate_missing_dense(_ptr(panel.p32), panel.m, n, rows_p, _ptr(sel), nm, self.rowmiss[r0:].data_ptr(),
                                                     _ptr(self.qpl[0]), _ptr(self.qpl[1]), _ptr(grot), n, _stream()))
        elif self.rowmiss is not None:
            check(lib().jxg_rotate_missing_correct(_ptr(panel.p32), panel.m, n, rows_p, nr, self.rowmiss[r0:].data_ptr(),
                                                   _ptr(self.usamp), _ptr(grot), n, _stream()))

    def fused_sums(self, sums, r0, nr, w, py, wx, p):
        super().fused_sums(sums, r0, nr, w, py, wx, p, self.rowoff[r0:].data_ptr(), _ptr(self.usum))


class BlockRotation:
    """Block-diagonal eigenbasis of a sparse GRM whose graph falls into small connected components (thresholded GRMs are
    block diagonal by family): the samples are ordered so that every diagonal block holds whole components, each block has
    its own dense eigendecomposition, and a SNP is rotated block by block with the MFMA rotation kernel writing its columns
    of the rotated row (`jxg_rotate_packed16x_ld`).  Memory and time are O(n B) / O(n B) per SNP for blocks of B samples
    instead of O(n^2): the form the SparseLMM routes take beyond the reach of one dense n x n eigenproblem
    (reference: sparse LLT of K + lambda I, src/stats/spreml.rs:384-512, src/math/cholesky.rs:776-1075)."""

    def __init__(self, packed: torch.Tensor, n_samples: int, sample_idx: np.ndarray, blocks):
        # blocks: list of (offset, nb, ut64 device tensor (nb, nb), rows = eigenvectors); sample_idx: panel sample of every
        # position of the block order
        self.n = int(sum(b[1] for b in blocks))
        self.parts = []
        dev = packed.device
        for off, nb, ut64 in blocks:
            ut32 = torch.empty((nb, nb), dtype=torch.float32, device=dev)
            check(lib().jxg_cast_f64_to_f32(_ptr(ut64), _ptr(ut32), nb * nb, _stream()))
            npad = lib().jxg_num_tiles(nb) * 128
            hi = torch.empty((npad, npad), dtype=torch.float16, device=dev)
            lo = torch.empty((npad, npad), dtype=torch.float16, device=dev)
            check(lib().jxg_ut_split(_ptr(ut32), nb, _ptr(hi), _ptr(lo), SCALE_EXP, _stream()))
            del ut32
            panel = Panel(packed, n_samples, np.asarray(sample_idx[off:off + nb], dtype=np.int64))
            self.parts.append((off, nb, hi, lo, panel))
        self.m = int(packed.shape[0])
        self.device = dev


class BlockDiagRotation(_Fp16Rotation):
    """Rotation stage of a block-diagonal eigenbasis (`BlockRotation`) for the SNP rows of one call: the general hi / lo split of
    every LUT, then per block of rows one fp16 launch per diagonal block (no row offsets, no int8 path)."""

    def __init__(self, rot: BlockRotation, rows, lut):
        self.parts, self.n = rot.parts, rot.n
        self.tiles = int(sum(panel.nt for _o, _nb, _h, _l, panel in rot.parts))
        lut_t = self._upload(rows, lut, rot.device)
        check(lib().jxg_lut_split(_ptr(lut_t), len(rows), _ptr(self.lut16), _stream()))


class DenseRowsRotation:
    """Rotation stage of DENSE SNP-major f32 rows `g` (m, n) on the host (the mirror's dense-chunk entry points): a block of
    rows is copied to the device and rotated with the exact f32 kernel (`jxg_rotate_dense_f32`) by the `parts` (offset, nb, U^T f32
    (nb, nb) on the device, sample positions of the part or None) of the eigenbasis -- one part for a dense basis, the diagonal
    blocks otherwise; no parts: the rows are rotated already.  The staging buffers are allocated here, once."""
    fused_ok = False       # G~ is always written
    tiles = 0

    def __init__(self, g: np.ndarray, parts, n: int, block_rows: int, dev):
        self.n, self.parts = int(n), list(parts)
        with warnings.catch_warnings():      # a read-only array is only ever read through this tensor
            warnings.simplefilter("ignore", UserWarning)
            self.g = torch.from_numpy(g)
        br = int(block_rows)
        self.whole = len(self.parts) == 1 and self.parts[0][3] is None and self.parts[0][1] == self.n
        self.gb = torch.empty((br, self.n), dtype=torch.float32, device=dev) if self.parts else None
        # (rows of the part's samples, their rotation) per part of a split basis
        self.sub = [] if self.whole else [tuple(torch.empty((br, nb), dtype=torch.float32, device=dev) for _ in range(2))
                                          for _off, nb, _ut, _cols in self.parts]

    def rotate(self, grot, r0, nr):
        """G~ of the rows [r0, r0 + nr) -> grot (>= nr, n) f32."""
        (self.gb if self.parts else grot)[:nr].copy_(self.g[r0:r0 + nr])
        if self.whole:
            check(lib().jxg_rotate_dense_f32(_ptr(self.gb), nr, self.n, _ptr(self.parts[0][2]), _ptr(grot), _stream()))
            return
        for (off, nb, ut32, cols), (sub, rb) in zip(self.parts, self.sub):
            if cols is None:
                sub[:nr].copy_(self.gb[:nr, off:off + nb])
            else:
                torch.index_select(self.gb[:nr], 1, cols, out=sub[:nr])
            check(lib().jxg_rotate_dense_f32(_ptr(sub), nr, nb, _ptr(ut32), _ptr(rb), _stream()))
            grot[:nr, off:off + nb] = rb[:nr]


# What `_run_blocks` drives: a rotation stage, scan(buf, r0, nr) writing the rows [r0, r0 + nr) of the table from their block
# buffer, whole_table (`on_block` gets the table once at the end) and fused = (w, py, wx, p) where that buffer holds the sums, not G~.
_Scanner = namedtuple("_Scanner", "stage scan whole_table fused", defaults=(False, None))


def _exact_scan(stage, model, out, evals, br, brent, max_iter, tol, nullml, chain_off):
    """'lmm': exact per-SNP REML.  One-off: the Chebyshev tables of the lambda-only REML sums where they exist; with `chain_off`
    the chains' carried states and, where the series form exists, the storage of one super-block of series."""
    dev, mk, n, p = out.device, int(out.shape[0]), model.n, model.p
    lo_b, hi_b, warm, init = brent
    tol, max_iter = float(tol), int(max_iter)
    with_plrt, nullml_v = (1, float(nullml)) if nullml is not None else (0, 0.0)
    s_p, x_p, y_p, tables = _ptr(model.S), _ptr(model.xcov), _ptr(model.y), None
    nbytes = int(lib().jxg_lmm_tables_bytes(n, p, lo_b, hi_b))
    if nbytes > 0:
        tables = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib().jxg_lmm_tables_build(s_p, x_p, y_p, n, p, lo_b, hi_b, _ptr(tables), _stream()))

    ev_p = (lambda r0: evals[r0:].data_ptr()) if evals is not None else (lambda r0: None)      # noqa: E731
    if chain_off is None:
        def scan(grot, r0, nr):
            if tables is not None:
                check(lib().jxg_lmm_scan_tab(_ptr(grot), nr, n, s_p, x_p, p, lo_b, hi_b, _ptr(tables), tol, max_iter, warm, init,
                                             with_plrt, nullml_v, out[r0:].data_ptr(), ev_p(r0), _stream()))
            else:
                check(lib().jxg_lmm_scan_exact(_ptr(grot), nr, n, s_p, x_p, y_p, p, lo_b, hi_b, tol, max_iter, warm, init,
                                               with_plrt, nullml_v, out[r0:].data_ptr(), ev_p(r0), _stream()))
        return _Scanner(stage, scan)
    co = np.ascontiguousarray(chain_off, dtype=np.int64)
    if co.ndim != 1 or len(co) < 2 or co[0] != 0 or co[-1] != mk or np.any(np.diff(co) < 0):
        raise RuntimeError("chain_off must ascend from 0 to len(rows)")
    carry = torch.full((len(co) - 1,), init if warm else float("nan"), dtype=torch.float64, device=dev)
    sd = int(lib().jxg_lmm_series_doubles(p, lo_b, hi_b)) if tables is not None else 0
    if sd == 0:
        # no series form (wide bounds, many covariates): the chains that touch this block, states carried across blocks
        def scan(grot, r0, nr):
            c0, loc_t = _chain_segments(co, r0, r0 + nr, dev)
            check(lib().jxg_lmm_scan_chain(_ptr(grot), nr, n, s_p, x_p, y_p, p, lo_b, hi_b, tol, max_iter, _ptr(loc_t),
                                           len(loc_t) - 1, carry[c0:].data_ptr(), with_plrt, nullml_v, out[r0:].data_ptr(),
                                           ev_p(r0), _stream()))
        return _Scanner(stage, scan)
    cap = SERIES_CAP_BYTES // (8 * (sd + 1 + out.shape[1]))
    sb_rows, sb0 = min(mk, max(br, cap // br * br)), 0     # rows per super-block; first row of the open one
    scoef = torch.empty((sb_rows, sd), dtype=torch.float64, device=dev)
    sssq = torch.empty(sb_rows, dtype=torch.float64, device=dev)

    def scan(grot, r0, nr):
        # the series of this block behind those of the open super-block; when it is full or the rows end, its Brent
        # searches: one launch over the chains that touch it
        nonlocal sb0
        check(lib().jxg_lmm_series_coef_tab(_ptr(grot), nr, n, x_p, p, lo_b, hi_b, _ptr(tables), scoef[r0 - sb0:].data_ptr(),
                                            sssq[r0 - sb0:].data_ptr(), _stream()))
        if r0 + nr - sb0 >= sb_rows or r0 + nr >= mk:
            c0, loc_t = _chain_segments(co, sb0, r0 + nr, dev)
            check(lib().jxg_lmm_series_brent_tab(r0 + nr - sb0, n, s_p, x_p, p, lo_b, hi_b, _ptr(tables), tol, max_iter, 0, 0.0,
                                                 _ptr(scoef), _ptr(sssq), _ptr(loc_t), len(loc_t) - 1, carry[c0:].data_ptr(),
                                                 with_plrt, nullml_v, out[sb0:].data_ptr(), ev_p(sb0), _stream()))
            sb0 = r0 + nr
    return _Scanner(stage, scan, whole_table=True)


def _lmm2_scan(stage, model, out, brent, max_iter, tol, nullml):
    """'lmm2': REML Wald + ML likelihood ratio against the null ML."""
    lo_b, hi_b, warm, init = brent

    def scan(grot, r0, nr):
        check(lib().jxg_lmm2_scan(_ptr(grot), nr, model.n, _ptr(model.S), _ptr(model.xcov), _ptr(model.y), model.p, lo_b, hi_b,
                                  float(tol), int(max_iter), warm, init, float(nullml), out[r0:].data_ptr(), _stream()))
    return _Scanner(stage, scan)


def _fixed_lambda_scan(stage, p, out, w, py, wx, a_chol, ypy, df, score, with_plrt=0, nullml=0.0, log_det_v=0.0):
    """'fvlmm' / 'splmm' over any rotation stage.  Where the stage has the fused form (`fused_ok`: the fp16 kernel) and
    `_fused_fixed_lambda` allows it `jxg_fvlmm_finish_dev` finishes the fused sums; else `jxg_fvlmm_scan_dev` /
    `jxg_splmm_exact_scan_dev` read G~.
    score: the SparseLMM exact scan -- score-form test with the null sigma2 = yPy / (n - p) (src/stats/splmm.rs:2567-2880)."""
    n = stage.n
    a_dev = torch.from_numpy(np.ascontiguousarray(a_chol, dtype=np.float64)).to(out.device)
    if _fused_fixed_lambda(p) and stage.fused_ok:
        def finish(sums, r0, nr):
            check(lib().jxg_fvlmm_finish_dev(_ptr(sums), stage.tiles, p + 2, nr, n, p, _ptr(a_dev), ypy, df, with_plrt, nullml,
                                             log_det_v, 1 if score else 0, out[r0:].data_ptr(), _stream()))
        return _Scanner(stage, finish, fused=(w, py, wx, p))

    def scan(grot, r0, nr):
        if score:
            check(lib().jxg_splmm_exact_scan_dev(_ptr(grot), nr, n, p, _ptr(w), _ptr(py), _ptr(wx), _ptr(a_dev), ypy, df,
                                                 out[r0:].data_ptr(), _stream()))
        else:
            check(lib().jxg_fvlmm_scan_dev(_ptr(grot), nr, n, p, _ptr(w), _ptr(py), _ptr(wx), _ptr(a_dev), ypy, df, with_plrt,
                                           nullml, log_det_v, out[r0:].data_ptr(), _stream()))
    return _Scanner(stage, scan)


def _splmm_scan(stage, p, out, fv_state):
    # null state on the K + lambda I scale, formed in f64 by the caller without the 1e-6 ridge jxg_fvlmm_prepare puts
    # on X'WX (fvlmm.rs): at the large lambda of a trait without polygenic signal that ridge is a 1e-4 relative error
    w, py, wx, a_chol, ypy = fv_state
    return _fixed_lambda_scan(stage, p, out, w, py, wx, a_chol, ypy, stage.n - p, True)


def _run_blocks(scanner, out, br, nbuf=1, times: StageTimes = None, on_block=None, progress=None, progress_every=0):
    """The block loop of the packed and the dense-row scans: rotate block b into one of `nbuf` buffers, scan it; stage times from
    events, `on_block` on a copy stream one block behind, `progress`.  Only launches, no allocation and no host sync per block (the
    chain forms upload the offsets of the chains that touch a block or super-block: `_chain_segments`; the dense-row stage uploads
    the block's rows)."""
    stage, scan, whole_table, fused = scanner
    mk = int(out.shape[0])
    rotate = stage.rotate if fused is None else (lambda buf, r0, nr: stage.fused_sums(buf, r0, nr, *fused))
    shape, dtype = ((br, stage.n), torch.float32) if fused is None else ((stage.tiles, br, fused[3] + 2), torch.float64)
    bufs = [torch.empty(shape, dtype=dtype, device=out.device) for _ in range(nbuf)]
    # per block the events around its rotation (0, 1) and around its scan (2, 3); only where stage times are asked for
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range((mk + br - 1) // br if times is not None else 0)]
    pending = None          # (i0, i1, event recorded behind the block's scan)
    copy_stream = torch.cuda.Stream(device=out.device) if on_block is not None else None
    step, last_tick = (int(progress_every) if progress_every and int(progress_every) > 0 else br), 0

    def hand_over(item):
        i0, i1, ev = item
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ev)
            host = out[i0:i1].to("cpu", non_blocking=False)
        on_block(i0, host.numpy())

    for bi, r0 in enumerate(range(0, mk, br)):
        nr = min(br, mk - r0)
        buf = bufs[bi % nbuf]
        if ev:
            ev[bi][0].record()
        rotate(buf, r0, nr)
        if ev:
            ev[bi][1].record()
            ev[bi][2].record()
        scan(buf, r0, nr)
        if ev:
            ev[bi][3].record()
        if on_block is not None and not whole_table:
            done = torch.cuda.Event()
            done.record()
            if pending is not None:
                hand_over(pending)       # the previous block, while this one runs
            pending = (r0, r0 + nr, done)
        if progress is not None and (r0 + nr >= mk or r0 + nr >= last_tick + step):
            last_tick = r0 + nr
            progress(r0 + nr, mk)
    if whole_table and on_block is not None:
        done = torch.cuda.Event()
        done.record()
        pending = (0, mk, done)
    if pending is not None:
        hand_over(pending)
    if times is not None:
        torch.cuda.synchronize()
        times.add("rotate", sum(e[0].elapsed_time(e[1]) for e in ev) * 1e-3)
        times.add("scan", sum(e[2].elapsed_time(e[3]) for e in ev) * 1e-3)


def scan_rows(panel: Panel, model: SpectralModel, rows: np.ndarray, lut: np.ndarray, mode="lmm", low=None,
              high=None, max_iter=30, tol=1e-2, init_log10_lbd=None, block_rows=None, return_evals=False,
              times: StageTimes = None, nullml=None, fv_state=None, on_block=None, chain_off=None, progress=None,
              progress_every=0):
    """Rotate + scan the given SNP rows. mode: 'lmm' (exact per-SNP REML), 'fvlmm' (fixed lambda) or 'lmm2' (REML Wald +
    ML likelihood ratio, needs `nullml`).  Returns a (len(rows), 3) f64 device tensor [beta, se, p] -- 4 columns
    [.., plrt] when `nullml` is given, 6 columns [beta, se, pwald, lambda, ml, plrt] for 'lmm2' -- (and the per-SNP
    Brent evaluation counts).
    block_rows: rows per rotation block; None = 8192, or 32768 for the exact scan beyond the LDS-resident limit.
    chain_off ('lmm' only): offsets into `rows` (int64, 0 ... len(rows), ascending; `stats.warm_chain_offsets`) of the
    reference's warm-start chains (src/stats/lmm.rs:134-161): inside a chain every SNP's Brent starts from the optimum of the
    valid SNP before it, the first one from `init_log10_lbd` or the interval midpoint.  The rotation and the per-SNP series stay
    parallel over all SNPs; the Brent searches run one wave per chain -- where the series form exists in ONE launch per
    super-block (the series of at most SERIES_CAP_BYTES / (8 (series + 1 + columns)) rows, whole blocks, at least one; a chain cut
    by a super-block continues from its carried state; `on_block` then receives the whole table at the end), block by block with
    carried states otherwise.
    progress(done, total): called after a block when `done` has advanced by `progress_every` rows (default: one block) since the
    last call, and after the last block; an exception raised there ends the scan."""
    dev, n = panel.device, model.n
    if panel.n != n:
        raise RuntimeError(f"selected sample count {panel.n} != model n {n}")
    mk = len(rows)
    with_plrt = 1 if nullml is not None else 0
    if mode == "lmm2" and nullml is None:
        raise RuntimeError("lmm2 needs the null ML (nullml)")
    out = torch.empty((mk, 6 if mode == "lmm2" else (4 if with_plrt else 3)), dtype=torch.float64, device=dev)
    evals = torch.zeros(mk, dtype=torch.int32, device=dev) if return_evals else None
    if mk == 0:
        return (out, evals) if return_evals else out
    if block_rows is None:
        # beyond the LDS-resident limit the exact scan runs its tiled form: one workgroup per CU walks a queue of SNPs in
        # lock step over LDS tiles of (s, X~, y~); longer blocks keep every wave's queue deep (8 SNPs per wave)
        block_rows = 32768 if mode == "lmm" and (8 * n * (2 + model.p) > 156 * 1024 or model.p + 1 > 4) else 8192
    br = int(min(block_rows, mk))
    stage = DenseRotation(panel, model, rows, lut, br, fixed_lambda=mode in ("fvlmm", "splmm"))
    if mode in ("lmm", "lmm2"):     # (low, high, warm, init) of the Brent searches
        brent = (*(model.null.bounds if low is None else (float(low), float(high))),
                 int(init_log10_lbd is not None), float(init_log10_lbd or 0.0))
    if mode == "lmm2":
        scanner = _lmm2_scan(stage, model, out, brent, max_iter, tol, nullml)
    elif mode == "lmm":
        scanner = _exact_scan(stage, model, out, evals, br, brent, max_iter, tol, nullml, chain_off)
    elif mode == "splmm":
        if fv_state is None:
            raise RuntimeError("the SparseLMM exact scan needs its null state (fv_state = w, py, wx, a_chol, ypy)")
        scanner = _splmm_scan(stage, model.p, out, fv_state)
    else:
        lbd, w, py, wx, a_chol, ypy, log_det_v, df = model.fv_cache(init_log10_lbd)
        scanner = _fixed_lambda_scan(stage, model.p, out, w, py, wx, a_chol, ypy, df, False, with_plrt,
                                     float(nullml) if nullml is not None else 0.0, log_det_v)
    _run_blocks(scanner, out, br, 2 if mk > br else 1, times, on_block, progress, progress_every)
    return (out, evals) if return_evals else out


TRAITS_BLOCK_BYTES = 8 << 30      # rotated-row buffer of the trait-level LMM scan (one of two): a block's chains run side by side


def scan_rows_lmm_traits(panel: Panel, shared: SpectralModel, rows: np.ndarray, lut: np.ndarray, y_rot, init, low=-5.0, high=5.0,
                         max_iter=50, tol=1e-2, chain_off=None, block_rows=None, return_evals=False, on_trait=None,
                         times: StageTimes = None):
    """The exact per-SNP REML scan of T traits that share samples and design (`_run_mixed_trait_packed_multi_entry`,
    python/janusx/assoc/workflow_model_packed.py:6473-6515): ONE rotation stage and ONE pass over the rows; every rotated block
    is scanned for all traits before the next one is rotated (the reference rotates every block once per trait).
    shared: S / U^T / X~ (any model of `SpectralModel.for_traits`); y_rot (T, n) f64: the traits' rotated phenotypes; init (T):
    log10 lambda0 per trait, NaN = none (the interval midpoint).  chain_off as `scan_rows`: the chains that touch a block are
    walked for all traits by ONE launch (`jxg_lmm_traits_chain_tab`, a workgroup per (chain, trait); per-trait carried states, so
    a chain cut by a block continues in the next); without chains `jxg_lmm_scan_tab` once per trait on the same buffer.
    block_rows: None = whole chains -- the largest multiple of the longest chain within TRAITS_BLOCK_BYTES -- or 32768 without
    chains.  on_trait(t, table (m, 3) host array): called per trait, in order, when the scan is done.  times: receives "tables"
    (host clock, synchronised) and the "rotate" / "scan" stage times of the blocks (device events).
    -> (T, m, 3) f64 device tensor [beta, se, p] (and the (T, m) evaluation counts)."""
    dev, n, p = panel.device, shared.n, shared.p
    if panel.n != n:
        raise RuntimeError(f"selected sample count {panel.n} != model n {n}")
    if not torch.is_tensor(y_rot):
        y_rot = torch.from_numpy(np.ascontiguousarray(y_rot, dtype=np.float64))
    y_rot = y_rot.to(device=dev, dtype=torch.float64).contiguous()
    if y_rot.ndim != 2 or int(y_rot.shape[1]) != n:
        raise RuntimeError(f"y_rot must be (T, {n})")
    nt, mk = int(y_rot.shape[0]), len(rows)
    init = np.asarray(init, dtype=np.float64).ravel()
    if len(init) != nt:
        raise RuntimeError("one init_log10_lbd per trait (NaN: none)")
    lo_b, hi_b, tol, max_iter = float(low), float(high), float(tol), int(max_iter)
    out = torch.empty((nt, mk, 3), dtype=torch.float64, device=dev)
    evals = torch.zeros((nt, mk), dtype=torch.int32, device=dev) if return_evals else None
    if mk == 0 or nt == 0:
        return (out, evals) if return_evals else out
    co = None
    if chain_off is not None:
        co = np.ascontiguousarray(chain_off, dtype=np.int64)
        if co.ndim != 1 or len(co) < 2 or co[0] != 0 or co[-1] != mk or np.any(np.diff(co) < 0):
            raise RuntimeError("chain_off must ascend from 0 to len(rows)")
    if block_rows is None:
        block_rows = 32768
        if co is not None:
            longest = max(1, int(np.max(np.diff(co))))
            block_rows = max(1, TRAITS_BLOCK_BYTES // (4 * n) // longest) * longest
    br = int(min(block_rows, mk))
    stage = DenseRotation(panel, shared, rows, lut, br)
    s_p, x_p = _ptr(shared.S), _ptr(shared.xcov)
    nbytes = int(lib().jxg_lmm_tables_bytes(n, p, lo_b, hi_b))
    stride = (nbytes + 15) // 16 * 16
    tables = None
    if times is not None:
        torch.cuda.synchronize()
    t_tab = time.perf_counter()
    if nbytes > 0:
        tables = torch.empty((nt, stride), dtype=torch.uint8, device=dev)
        for ti in range(nt):
            check(lib().jxg_lmm_tables_build(s_p, x_p, y_rot[ti].data_ptr(), n, p, lo_b, hi_b, tables[ti].data_ptr(), _stream()))
    if times is not None:
        torch.cuda.synchronize()
        times.add("tables", time.perf_counter() - t_tab)
    ev_p = (lambda ti, r0: evals[ti, r0:].data_ptr()) if evals is not None else (lambda ti, r0: None)      # noqa: E731
    if co is None:
        def scan(grot, r0, nr):
            for ti in range(nt):
                warm, x0 = (1, float(init[ti])) if math.isfinite(init[ti]) else (0, 0.0)
                if tables is not None:
                    check(lib().jxg_lmm_scan_tab(_ptr(grot), nr, n, s_p, x_p, p, lo_b, hi_b, tables[ti].data_ptr(), tol, max_iter,
                                                 warm, x0, 0, 0.0, out[ti, r0:].data_ptr(), ev_p(ti, r0), _stream()))
                else:
                    check(lib().jxg_lmm_scan_exact(_ptr(grot), nr, n, s_p, x_p, y_rot[ti].data_ptr(), p, lo_b, hi_b, tol, max_iter,
                                                   warm, x0, 0, 0.0, out[ti, r0:].data_ptr(), ev_p(ti, r0), _stream()))
    else:
        nch = len(co) - 1
        carry = torch.from_numpy(np.repeat(np.where(np.isfinite(init), init, np.nan)[:, None], nch, axis=1).copy()).to(dev)
        batched = tables is not None and p + 1 <= 8

        def scan(grot, r0, nr):
            c0, loc_t = _chain_segments(co, r0, r0 + nr, dev)
            if batched:
                check(lib().jxg_lmm_traits_chain_tab(_ptr(grot), nr, n, s_p, x_p, p, lo_b, hi_b, _ptr(tables), stride, nt, tol,
                                                     max_iter, _ptr(loc_t), len(loc_t) - 1, carry[0, c0:].data_ptr(), nch,
                                                     out[0, r0:].data_ptr(), mk, ev_p(0, r0), _stream()))
                return
            # eight covariates and more (or no tables): the one-wave-per-chain entry per trait, on the shared rotated block
            for ti in range(nt):
                if tables is not None:
                    check(lib().jxg_lmm_scan_chain_tab(_ptr(grot), nr, n, s_p, x_p, p, lo_b, hi_b, tables[ti].data_ptr(), tol,
                                                       max_iter, _ptr(loc_t), len(loc_t) - 1, carry[ti, c0:].data_ptr(), 0, 0.0,
                                                       out[ti, r0:].data_ptr(), ev_p(ti, r0), _stream()))
                else:
                    check(lib().jxg_lmm_scan_exact_chain(_ptr(grot), nr, n, s_p, x_p, y_rot[ti].data_ptr(), p, lo_b, hi_b, tol,
                                                         max_iter, _ptr(loc_t), len(loc_t) - 1, carry[ti, c0:].data_ptr(), 0, 0.0,
                                                         out[ti, r0:].data_ptr(), ev_p(ti, r0), _stream()))
    # `_run_blocks` sizes its loop by the first dimension of the table it is handed: one trait's rows
    _run_blocks(_Scanner(stage, scan), out[0], br, 2 if mk > br else 1, times)
    if on_trait is not None:
        for ti in range(nt):
            on_trait(ti, out[ti].cpu().numpy())
    return (out, evals) if return_evals else out


def scan_rows_splmm_blocks(rot: BlockRotation, p: int, rows: np.ndarray, lut: np.ndarray, fv_state, block_rows=8192):
    """SparseLMM exact scan (`jxg_splmm_exact_scan_dev`, src/stats/splmm.rs:2567-2880) over rows rotated by a block-diagonal
    eigenbasis: per block of SNP rows one rotation launch per diagonal block, then the score-form scan over the full
    rotated rows (fused: the finish of their sums).  Returns (len(rows), 3) f64 [beta, se, p] on the device."""
    out = torch.empty((len(rows), 3), dtype=torch.float64, device=rot.device)
    if len(rows):
        _run_blocks(_splmm_scan(BlockDiagRotation(rot, rows, lut), p, out, fv_state), out, int(min(block_rows, len(rows))))
    return out


_Dims = namedtuple("_Dims", "n p")     # what the 'splmm' scan reads of a model: its null state arrives as `fv_state`


def scan_dense_rows(g: np.ndarray, model, mode, parts=None, low=None, high=None, max_iter=30, tol=1e-2, log10_lbd=None,
                    nullml=None, fv_state=None, dev=None, block_rows=4096):
    """`scan_rows` for DENSE SNP-major f32 rows `g` (m, n) on the host (the mirror's dense-chunk entry points): the same scanners
    and block loop over a `DenseRowsRotation`.  mode: 'lmm' (exact per-SNP REML on [low, high], no chains, no warm start), 'lmm2'
    (needs `nullml`), 'fvlmm' (fixed lambda at `log10_lbd`) or 'splmm' (`fv_state` as `scan_rows`).  parts: see `DenseRowsRotation`;
    None = `model.ut` as one part, or no rotation where the model has none.  -> (m, 3 | 4 with nullml | 6 for 'lmm2') f64 on the
    device."""
    dev = model.S.device if dev is None else dev
    m, n, p = int(g.shape[0]), model.n, model.p
    if parts is None:
        parts = [] if model.ut is None else [(0, n, model.ut, None)]
    with_plrt, nullml_v = (1, float(nullml)) if nullml is not None else (0, 0.0)
    out = torch.empty((m, 6 if mode == "lmm2" else 3 + with_plrt), dtype=torch.float64, device=dev)
    br = int(max(1, min(block_rows, m)))
    stage = DenseRowsRotation(g, parts, n, br, dev)
    if mode == "lmm":
        scanner = _exact_scan(stage, model, out, None, br, (float(low), float(high), 0, 0.0), max_iter, tol, nullml, None)
    elif mode == "lmm2":
        scanner = _lmm2_scan(stage, model, out, (float(low), float(high), 0, 0.0), max_iter, tol, nullml)
    elif mode == "splmm":
        scanner = _splmm_scan(stage, p, out, fv_state)
    else:
        _lbd, w, py, wx, a_chol, ypy, log_det_v, df = model.fv_cache(log10_lbd)
        scanner = _fixed_lambda_scan(stage, p, out, w, py, wx, a_chol, ypy, df, False, with_plrt, nullml_v, log_det_v)
    _run_blocks(scanner, out, br)
    return out


def scan_rows_splmm_dense(g: np.ndarray, parts, n: int, p: int, fv_state, dev, block_rows=8192):
    """SparseLMM exact scan of DENSE f32 rows `g` (m, n) on the host (`splmm_assoc_pcg_dense_f32`, src/stats/splmm.rs:5464-5650):
    `scan_dense_rows` with the eigenbasis of the sparse K as `parts` -- one part for a dense decomposition, the diagonal blocks
    otherwise -- and `jxg_splmm_exact_scan_dev` behind it.  -> (m, 3) f64 on the device."""
    return scan_dense_rows(g, _Dims(n, p), "splmm", parts, fv_state=fv_state, dev=dev, block_rows=block_rows)


def scan_rows_splmm_factor(rows_f32, m: int, n: int, p: int, csr, diag: np.ndarray, lam: float, vinv_x: np.ndarray,
                           py: np.ndarray, a_chol: np.ndarray, ypy: float, dev, block_rows: int = 256, tol: float = 1e-11,
                           max_iter: int = 1000):
    """SparseLMM exact scan (`exact_scan_blocks_core`, src/stats/splmm.rs:2567-2880) WITHOUT a spectral form of K: the relatedness
    graph holds a connected component beyond one dense eigenproblem (`janusx._SparseFactorReml`).  The reference solves
    (K + lambda I) z = g per SNP with its sparse factor; here every block of `block_rows` decoded rows is the right-hand side
    of one multi-vector conjugate-gradient solve over the CSR image of K in HBM (`jxg_sps_solve_multi`, csrc/k_spsolve.hip),
    then g'V^-1 g, g.Py, g.(V^-1 X) in sample space (`jxg_sps_scan_sums`) and the score-form finish of the other exact scans
    (`jxg_fvlmm_finish_dev`, score_mode = 1).  rows_f32(r0, nr) -> device tensor (nr, n) f32 of the decoded rows r0 .. r0 + nr
    ([0, 2 maf, 1, 2] or flipped, missing = mean, not centred).  -> (m, 3) f64 [beta, se, p] on the device."""
    rowptr, col, val = csr
    out = torch.empty((m, 3), dtype=torch.float64, device=dev)
    if m == 0:
        return out
    br = int(max(64, min(block_rows, (m + 63) // 64 * 64)))
    ldr = int(lib().jxg_sps_ldr(br))
    dinv = torch.from_numpy(1.0 / (np.asarray(diag, dtype=np.float64) + float(lam))).to(dev)
    work = torch.empty(int(lib().jxg_sps_work_doubles(n, ldr)), dtype=torch.float64, device=dev)
    g = torch.empty((n, ldr), dtype=torch.float64, device=dev)
    z = torch.empty((n, ldr), dtype=torch.float64, device=dev)
    sums = torch.empty((br, p + 2), dtype=torch.float64, device=dev)
    py_t = torch.from_numpy(np.ascontiguousarray(py, dtype=np.float64)).to(dev)
    vx_t = torch.from_numpy(np.ascontiguousarray(vinv_x, dtype=np.float64)).to(dev)
    a_dev = torch.from_numpy(np.ascontiguousarray(a_chol, dtype=np.float64)).to(dev)
    info = np.zeros(2, dtype=np.float64)
    for r0 in range(0, m, br):
        nr = min(br, m - r0)
        rows = rows_f32(r0, nr)
        check(lib().jxg_sps_rows_to_cols_f64(_ptr(rows), nr, n, int(rows.stride(0)), _ptr(g), ldr, _stream()))
        check(lib().jxg_sps_solve_multi(n, _ptr(rowptr), _ptr(col), _ptr(val), float(lam), _ptr(dinv), _ptr(g), nr, ldr,
                                        float(tol), int(max_iter), _ptr(z), _ptr(work), info.ctypes.data, _stream()))
        check(lib().jxg_sps_scan_sums(n, _ptr(g), _ptr(z), nr, ldr, _ptr(py_t), _ptr(vx_t), p, _ptr(sums), _ptr(work), _stream()))
        check(lib().jxg_fvlmm_finish_dev(_ptr(sums), 1, p + 2, nr, n, p, _ptr(a_dev), float(ypy), n - p, 0, 0.0, 0.0, 1,
                                         out[r0:].data_ptr(), _stream()))
    return out


def rotate_rows(panel: Panel, model: SpectralModel, rows: np.ndarray, lut: np.ndarray) -> torch.Tensor:
    """G~ = G U for a (small) list of SNP rows, written out: (len(rows), n) f32 on the device (the fp16 hi / lo rotation of
    `scan_rows` without a scan behind it; used for the sampled markers of the SparseLMM gamma estimate)."""
    grot = torch.empty((len(rows), model.n), dtype=torch.float32, device=panel.device)
    DenseRotation(panel, model, rows, lut, len(rows), int8=False).rotate(grot, 0, len(rows))
    return grot


def rotate_rows_blocks(rot: BlockRotation, rows: np.ndarray, lut: np.ndarray) -> torch.Tensor:
    """`rotate_rows` for a block-diagonal eigenbasis: every diagonal block writes its columns of the rotated rows."""
    grot = torch.empty((len(rows), rot.n), dtype=torch.float32, device=rot.device)
    BlockDiagRotation(rot, rows, lut).rotate(grot, 0, len(rows))
    return grot


def scan_rows_grammar(panel: Panel, rows: np.ndarray, lut: np.ndarray, x: np.ndarray, score_vec: np.ndarray, r_hat: float,
                      block_rows=65536, on_block=None):
    """SparseLMM approximate (GRAMMAR-gamma) scan over the payload in sample space (`jxg_splmm_grammar_scan_p32`,
    src/stats/splmm.rs:2935-3316 as called by `scan_with_py_and_rhat`, :3318): no rotation, (p + 1) dots per SNP.
    x (n, p) f64 design with intercept, score_vec (n) f64; both are rounded to f32 like `pack_score_design_rhs_f32`.
    Returns (len(rows), 3) f64 [beta, se, p] on the device."""
    dev, n, mk = panel.device, panel.n, len(rows)
    p = int(x.shape[1])
    out = torch.empty((mk, 3), dtype=torch.float64, device=dev)
    if mk == 0:
        return out
    if not (np.all(np.isfinite(score_vec)) and np.all(np.isfinite(x))):
        raise RuntimeError("SparseLMM scan received non-finite dense operand")
    xr = np.concatenate([x, np.asarray(score_vec, dtype=np.float64)[:, None]], axis=1).astype(np.float32).astype(np.float64)
    xtx = np.asarray(x, dtype=np.float64).T @ np.asarray(x, dtype=np.float64)
    ixx = np.linalg.inv(xtx)
    xr_t = torch.from_numpy(np.ascontiguousarray(xr)).to(dev)
    ixx_t = torch.from_numpy(np.ascontiguousarray(ixx)).to(dev)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    lut_t = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(dev)
    br = int(min(block_rows, mk))
    work = torch.empty(br * (p + 2), dtype=torch.float64, device=dev)
    for r0 in range(0, mk, br):
        nr = min(br, mk - r0)
        check(lib().jxg_splmm_grammar_scan_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, lut_t[r0:].data_ptr(),
                                               _ptr(xr_t), p, _ptr(ixx_t), 1.0, float(r_hat), 1.0, _ptr(work),
                                               out[r0:].data_ptr(), _stream()))
        if on_block is not None:
            on_block(r0, out[r0:r0 + nr].cpu().numpy())
    return out


def _lm_residualized(x, y, ixx, dev):
    """Host half of the LM scans (`jx_lm_residualize`; `ixx` None: (X'X)^-1 from `x`) -> ([X | r_y] rounded through f32
    (n, q0 + 1) f64 and (X'X)^-1 on the device, y'M_X y)."""
    from .janusx import lm_precompute_ixx_qr
    n, q0 = x.shape
    ixx = lm_precompute_ixx_qr(x) if ixx is None else np.ascontiguousarray(ixx, dtype=np.float64)
    xr = np.empty((n, q0 + 1), dtype=np.float64)
    yy = np.zeros(1, dtype=np.float64)
    check(lib().jx_lm_residualize(y.ctypes.data, x.ctypes.data, ixx.ctypes.data, n, q0, xr.ctypes.data, yy.ctypes.data))
    return torch.from_numpy(xr).to(dev), torch.from_numpy(ixx).to(dev), float(yy[0])


def scan_rows_lm_dense(g: np.ndarray, x: np.ndarray, y: np.ndarray, ixx=None, dev=None, block_rows=None):
    """`scan_rows_lm` for DENSE SNP-major f32 rows `g` (m, n) on the host (`lm_block_assoc_f32`, src/stats/glm.rs:4313-4497): per
    block of rows an upload and `jxg_lm_scan_dense`, in the block loop of the other scans.  x (n, q0) with the intercept and
    y (n): contiguous f64.  block_rows: None = at most 1 GiB of rows.  -> (m, 4) f64 device tensor [beta, se, pwald, plrt]."""
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    (m, n), q0 = g.shape, int(x.shape[1])
    br = max(1, min(m, 2 ** 30 // (4 * n))) if block_rows is None else max(1, min(m, int(block_rows)))
    xr_t, ixx_t, yy = _lm_residualized(x, y, ixx, dev)
    out = torch.empty((m, 4), dtype=torch.float64, device=dev)
    work = torch.empty(br * (q0 + 2), dtype=torch.float64, device=dev)

    def scan(gb, r0, nr):
        check(lib().jxg_lm_scan_dense(_ptr(gb), nr, n, n, _ptr(xr_t), q0, _ptr(ixx_t), yy, _ptr(work), out[r0:].data_ptr(),
                                      _stream()))
    _run_blocks(_Scanner(DenseRowsRotation(g, [], n, br, dev), scan), out, br)       # no parts: the stage only uploads
    return out


def scan_rows_lm(panel: Panel, rows: np.ndarray, af: np.ndarray, x: np.ndarray, y: np.ndarray, on_block=None, flip=None,
                 ixx=None, progress=None, progress_every=0):
    """Plain LM scan of the given SNP rows of a resident panel (`lm_block_assoc_packed`, src/stats/glm.rs:3550-3860; the `LM`
    wrapper python/janusx/pyBLUP/assoc.py:2185-2228): mean-imputed additive decode with the rows' allele frequencies
    ([0, mean, 1, 2], or [2, mean, 1, 0] where `flip`), `x` includes the intercept, `ixx` = (X'X)^-1 (default: from `x`).
    One launch per LM_BLOCK_ROWS rows; `progress(done, total)` as in `scan_rows`.  Returns a (len(rows), 4) f64 device tensor
    [beta, se, pwald (Student t), plrt]."""
    dev = panel.device
    n = panel.n
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.float64)
    if y.shape[0] != n or x.shape[0] != n:
        raise RuntimeError(f"selected sample count {panel.n} != len(y) {y.shape[0]}")
    q0 = int(x.shape[1])
    mk = len(rows)
    out = torch.empty((mk, 4), dtype=torch.float64, device=dev)
    if mk == 0:
        return out
    xr_t, ixx_t, yy = _lm_residualized(x, y, ixx, dev)
    mean_g = np.clip(np.float32(2.0) * np.asarray(af, dtype=np.float32), np.float32(0.0), np.float32(2.0))
    fl = np.zeros(mk, dtype=bool) if flip is None else np.asarray(flip, dtype=bool)
    lut = np.zeros((mk, 4), dtype=np.float32)
    lut[:, 0], lut[:, 1], lut[:, 2], lut[:, 3] = np.where(fl, 2.0, 0.0), mean_g, 1.0, np.where(fl, 0.0, 2.0)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    lut_t = torch.from_numpy(lut).to(dev)
    br = min(LM_BLOCK_ROWS, mk)
    step, last_tick = (int(progress_every) if progress_every and int(progress_every) > 0 else br), 0
    work = torch.empty(br * (q0 + 2), dtype=torch.float64, device=dev)
    for r0 in range(0, mk, br):
        nr = min(br, mk - r0)
        check(lib().jxg_lm_scan_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, lut_t[r0:].data_ptr(), _ptr(xr_t),
                                    q0, _ptr(ixx_t), yy, _ptr(work), out[r0:].data_ptr(), _stream()))
        if progress is not None and (r0 + nr >= mk or r0 + nr >= last_tick + step):
            last_tick = r0 + nr
            progress(r0 + nr, mk)
    if on_block is not None:
        on_block(0, out[:, :3].cpu().numpy())
    return out


LMT_MAX_TRAIT_BATCH = 1024        # `resolve_trait_batch_size`, src/stats/lm_trait.rs:288-300
LMT_SCRATCH_BYTES = 256 << 20     # the sums of one row block: rows per block = this / (8 (rank + trait batch))
LMT_HIT_CAPACITY = 1 << 20        # slots of the first hit buffer
LmTraitHits = namedtuple("LmTraitHits", "trait row stats")


class _LmtOperand:
    """Digit planes of f64 columns (`jxg_lmt_prepare`): `cols` is (C, n), one column per row, a host array or a contiguous f64
    device tensor.  keep_rem: `rem` (C, n) on the device = what the four digits leave of every entry."""

    def __init__(self, cols, n: int, npad: int, dev, keep_rem=False):
        self.ncols = int(cols.shape[0])
        cpad = lib().jxg_lmt_cpad(self.ncols)
        b = cols if torch.is_tensor(cols) else torch.from_numpy(np.ascontiguousarray(cols, dtype=np.float64)).to(dev)
        self.rem = torch.empty((self.ncols, n), dtype=torch.float64, device=dev) if keep_rem else None
        self.planes = torch.empty((4, cpad, npad), dtype=torch.int8, device=dev)
        self.scale = torch.empty(cpad, dtype=torch.float64, device=dev)
        self.colsum = torch.empty(cpad, dtype=torch.int64, device=dev)
        self.sexp = torch.empty(cpad, dtype=torch.int32, device=dev)
        check(lib().jxg_lmt_prepare(_ptr(b), n, n, self.ncols, _ptr(self.planes), _ptr(self.scale), _ptr(self.colsum),
                                    _ptr(self.sexp), _ptr(self.rem), _stream()))


def lm_traits_row_d(counts: np.ndarray, n: int, mean_g: np.ndarray, flip: np.ndarray) -> np.ndarray:
    """sum_i v^2 of the mean-imputed additive rows from their (missing, het, hom_alt) counts: n_1 + 4 n_2 + n_miss mean^2 with the
    f32 mean squared in f64 (n_2 = the homozygotes of the other allele where the row is flipped)."""
    c = np.asarray(counts, dtype=np.int64)
    miss, het, hom = c[:, 0], c[:, 1], c[:, 2]
    two = np.where(flip, n - miss - het - hom, hom)
    m64 = np.asarray(mean_g, dtype=np.float32).astype(np.float64)
    return (het + 4 * two).astype(np.float64) + miss.astype(np.float64) * (m64 * m64)


def scan_rows_lm_traits(panel: Panel, rows: np.ndarray, af: np.ndarray, x: np.ndarray, Y: np.ndarray, flip=None, pmax=None,
                        trait_batch=None, hit_capacity=None, progress=None, block_rows=None):
    """Multi-trait LM scan of the given SNP rows of a resident panel: the shared-projection route of the reference
    (`lm_trait_assoc_bed_to_tsv_shared_fast`, src/stats/lm_trait.rs:481-686) for traits that share the samples, the design `x`
    (n, q0, intercept included) and the rows.  `Y` is TRAIT-MAJOR, (T, n) like the reference's `y_trait_major`; every value must be
    finite (masks are the caller's job).  Host: the f64 Gram-Schmidt basis Q of `x` (`lm2.qr_basis`), R = Y - Q Q'Y and rss0 per
    trait; device: the digit planes of [Q | R] (`jxg_lmt_prepare`; Q twice: its digits and what they leave), per row block G Q
    once and G R per batch of at most `trait_batch` (<= 1024) traits (`jxg_lmt_sums_p32`), and the statistics
    (`jxg_lmt_stats`).  Rows decode as in `scan_rows_lm`:
    [0, mean, 1, 2] with mean = clip(2 af, 0, 2) in f32, or [2, mean, 1, 0] where `flip`.
    pmax None -> a (T, len(rows), 4) f64 device tensor [beta, se, chisq, p].
    pmax = P  -> LmTraitHits(trait int32, row int32 (position in `rows`), stats (k, 4) f64) of every (trait, row) with p <= P,
    sorted by (trait, row); `hit_capacity` sizes the first device buffer, a block whose hits do not fit is run again into a larger
    one.  `progress(done_rows, total_rows)` after every row block."""
    from . import lm2
    dev, n = panel.device, panel.n
    x = np.ascontiguousarray(x, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise RuntimeError("Y must be trait-major with shape (n_traits, n_samples)")
    T = int(Y.shape[0])
    if Y.shape[1] != n or x.ndim != 2 or x.shape[0] != n:
        raise RuntimeError(f"selected sample count {n} != trait length {Y.shape[1]} / design rows {x.shape[0]}")
    if T == 0:
        raise RuntimeError("no traits given")
    bad = np.nonzero(~np.all(np.isfinite(Y), axis=1))[0]
    if bad.size:
        raise RuntimeError(f"trait {int(bad[0])} contains non-finite values")
    if pmax is not None and not (float(pmax) == float(pmax)):
        raise RuntimeError("pmax must not be NaN")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    mk = len(rows)
    if mk and (rows.min() < 0 or rows.max() >= panel.m):
        raise RuntimeError("row index out of range")
    tb = LMT_MAX_TRAIT_BATCH if trait_batch is None else int(trait_batch)
    if tb < 1:
        raise RuntimeError("trait_batch must be >= 1")
    tb = min(tb, LMT_MAX_TRAIT_BATCH, T)
    q = lm2.qr_basis(x)
    rank = int(q.shape[1])
    qty = q.T @ Y.T                                        # (rank, T)
    R = Y - (q @ qty).T
    if not np.all(np.isfinite(R)):
        raise RuntimeError("LM QR residualization produced non-finite values")
    rss0 = np.einsum("tn,tn->t", R, R)
    hits = pmax is not None
    if mk == 0:
        if hits:
            return LmTraitHits(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4)))
        return torch.empty((T, 0, 4), dtype=torch.float64, device=dev)

    mean_g = np.clip(np.float32(2.0) * np.asarray(af, dtype=np.float32), np.float32(0.0), np.float32(2.0))
    fl = np.zeros(mk, dtype=bool) if flip is None else np.asarray(flip, dtype=bool)
    if len(mean_g) != mk or len(fl) != mk:
        raise RuntimeError("af / flip length != number of rows")
    d_row = lm_traits_row_d(panel.counts()[rows], n, mean_g, fl)
    rows_t = torch.from_numpy(rows).to(dev)
    mean_t = torch.from_numpy(np.ascontiguousarray(mean_g)).to(dev)
    flip_t = torch.from_numpy(fl.astype(np.uint8)).to(dev)
    d_t = torch.from_numpy(d_row).to(dev)
    rss0_t = torch.from_numpy(np.ascontiguousarray(rss0)).to(dev)
    # Q takes eight digits, as two operands: gg = d - sum qg^2 meets an absolute threshold and needs qg to f64 accuracy
    op_q = _LmtOperand(q.T, n, panel.npad, dev, keep_rem=True) if rank else None
    op_q_lo = _LmtOperand(op_q.rem, n, panel.npad, dev) if rank else None
    op_r = [_LmtOperand(R[t0:t0 + tb], n, panel.npad, dev) for t0 in range(0, T, tb)]

    # rows per block: a fixed scratch budget (whole row tiles), or what the caller asks for
    br = int(block_rows) if block_rows else max(128, min(LMT_SCRATCH_BYTES // (8 * (rank + tb)), 1 << 22) // 128 * 128)
    br = max(1, min(br, mk))
    qg = torch.empty((br, max(rank, 1)), dtype=torch.float64, device=dev)
    qg_lo = torch.empty_like(qg)
    gy = torch.empty((br, tb), dtype=torch.float64, device=dev)
    out = None if hits else torch.empty((T, mk, 4), dtype=torch.float64, device=dev)
    if hits:
        cap = max(1, int(hit_capacity) if hit_capacity is not None else min(mk * T, LMT_HIT_CAPACITY))
        h_t = torch.empty(cap, dtype=torch.int32, device=dev)
        h_r = torch.empty(cap, dtype=torch.int32, device=dev)
        h_v = torch.empty((cap, 4), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        total = 0

    def sums(op, dst, r0, nr):
        check(lib().jxg_lmt_sums_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, mean_t[r0:].data_ptr(),
                                     flip_t[r0:].data_ptr(), _ptr(op.planes), _ptr(op.scale), _ptr(op.colsum), op.ncols,
                                     _ptr(dst), dst.shape[1], _stream()))

    def stats(r0, nr, t0, nt):
        check(lib().jxg_lmt_stats(_ptr(qg), _ptr(qg_lo) if rank else None, qg.shape[1], rank, _ptr(gy), gy.shape[1], nt,
                                  d_t[r0:].data_ptr(), nr, rss0_t[t0:].data_ptr(), n, None if hits else out[t0:, r0:].data_ptr(), mk * 4,
                                  float(pmax) if hits else 0.0, cap if hits else 0, t0, r0, _ptr(h_t) if hits else None,
                                  _ptr(h_r) if hits else None, _ptr(h_v) if hits else None, _ptr(count) if hits else None,
                                  _stream()))

    for r0 in range(0, mk, br):
        nr = min(br, mk - r0)
        if rank:
            sums(op_q, qg, r0, nr)
            sums(op_q_lo, qg_lo, r0, nr)
        for bi, t0 in enumerate(range(0, T, tb)):
            nt = min(tb, T - t0)
            sums(op_r[bi], gy, r0, nr)
            stats(r0, nr, t0, nt)
            if hits:
                seen = int(count.item())
                if seen > cap:                      # this block's hits did not fit: a larger buffer, the block's statistics again
                    cap = max(seen, 2 * cap)
                    grown = (torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                             torch.empty((cap, 4), dtype=torch.float64, device=dev))
                    for dst, src in zip(grown, (h_t, h_r, h_v)):
                        dst[:total] = src[:total]
                    h_t, h_r, h_v = grown
                    count.fill_(total)
                    stats(r0, nr, t0, nt)
                    seen = int(count.item())
                total = seen
        if progress is not None:
            progress(r0 + nr, mk)
    if not hits:
        return out
    ht, hr, hv = h_t[:total].cpu().numpy(), h_r[:total].cpu().numpy(), h_v[:total].cpu().numpy()
    order = np.lexsort((hr, ht))
    return LmTraitHits(np.ascontiguousarray(ht[order]), np.ascontiguousarray(hr[order]), np.ascontiguousarray(hv[order]))


FarmcpuFem = namedtuple("FarmcpuFem", "p qtn_min_p stats")


def farmcpu_missing_value(af: np.ndarray) -> np.ndarray:
    """Major-allele imputation of the FarmCPU routes (`farmcpu_missing_impute_value`, src/stats/farmcpu.rs:206-217): a missing call
    decodes to 2 where 2 af > 1 and to 0 otherwise (f32, the `mean` operand of `jxg_lmt_sums_p32`); a flip leaves it alone."""
    a = np.asarray(af, dtype=np.float32).astype(np.float64)
    return np.where(2.0 * a > 1.0, np.float32(2.0), np.float32(0.0)).astype(np.float32)


def _farmcpu_scan(panel: Panel, rows, af, flip, x, q_base, y, final, block_rows):
    from . import farmcpu as fc
    dev, n = panel.device, panel.n
    des = fc.design_operands(x, q_base, y)
    q, rank, kq = des.q, int(des.q.shape[1]), int(des.w.shape[0])
    if kq > lib().jxg_farmcpu_max_qtn():
        raise RuntimeError(f"FarmCPU scan: {kq} pseudo-QTN columns are above the cap of {lib().jxg_farmcpu_max_qtn()} "
                           "(lower the QTN bound)")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    mk = len(rows)
    if mk and (rows.min() < 0 or rows.max() >= panel.m):
        raise RuntimeError("row index out of range")
    out = torch.empty((mk, 3), dtype=torch.float64, device=dev)
    maxbits = torch.zeros(max(kq, 1), dtype=torch.int64, device=dev)
    if mk:
        miss_g = farmcpu_missing_value(af)
        fl = np.zeros(mk, dtype=bool) if flip is None else np.asarray(flip, dtype=bool)
        if len(miss_g) != mk or len(fl) != mk:
            raise RuntimeError("af / flip length != number of rows")
        ss_t = torch.from_numpy(lm_traits_row_d(panel.counts()[rows], n, miss_g, fl)).to(dev)
        rows_t = torch.from_numpy(rows).to(dev)
        mean_t = torch.from_numpy(miss_g).to(dev)
        flip_t = torch.from_numpy(fl.astype(np.uint8)).to(dev)
        # one operand [Q | r_y]: its digits; a second one for what the digits of Q leave (b22 meets an absolute threshold)
        op_hi = _LmtOperand(np.vstack([q.T, des.r_y[None, :]]), n, panel.npad, dev, keep_rem=True)
        op_lo = _LmtOperand(op_hi.rem[:rank], n, panel.npad, dev)
        w_t = torch.from_numpy(np.ascontiguousarray(des.w)).to(dev) if kq else None
        bgb_t = torch.from_numpy(np.ascontiguousarray(des.bg_beta[q_base:])).to(dev) if kq else None
        dixx_t = torch.from_numpy(np.diag(des.ixx)[q_base:].copy()).to(dev) if kq else None
        br = int(block_rows) if block_rows else max(128, min(LMT_SCRATCH_BYTES // (8 * (2 * rank + 1)), 1 << 22) // 128 * 128)
        br = max(1, min(br, mk))
        hi = torch.empty((br, rank + 1), dtype=torch.float64, device=dev)
        lo = torch.empty((br, rank + 1), dtype=torch.float64, device=dev)    # the kernel reads both with one leading dimension
        for r0 in range(0, mk, br):
            nr = min(br, mk - r0)
            for op, dst in ((op_hi, hi), (op_lo, lo)):
                check(lib().jxg_lmt_sums_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, mean_t[r0:].data_ptr(),
                                             flip_t[r0:].data_ptr(), _ptr(op.planes), _ptr(op.scale), _ptr(op.colsum), op.ncols,
                                             _ptr(dst), dst.shape[1], _stream()))
            gy = hi[:, rank:]
            if final:
                check(lib().jxg_farmcpu_final_stats(_ptr(hi), _ptr(lo), rank + 1, rank, gy.data_ptr(), rank + 1, ss_t[r0:].data_ptr(),
                                                    nr, des.bg_rss, des.df, out[r0:].data_ptr(), _stream()))
            else:
                check(lib().jxg_farmcpu_fem_stats(_ptr(hi), _ptr(lo), rank + 1, rank, gy.data_ptr(), rank + 1, ss_t[r0:].data_ptr(),
                                                  nr, des.bg_rss, des.df, _ptr(w_t), rank, kq, _ptr(bgb_t), _ptr(dixx_t),
                                                  out[r0:].data_ptr(), _ptr(maxbits), _stream()))
    return des, out, maxbits[:kq]


def scan_rows_farmcpu_fem(panel: Panel, rows: np.ndarray, af: np.ndarray, flip, x: np.ndarray, q_base: int, y: np.ndarray,
                          block_rows=None) -> FarmcpuFem:
    """Fixed-effect scan of FarmCPU's raw route (`scan_packed_full_matrix_reduced`, src/stats/farmcpu.rs:2629-2941) over the given
    rows of a resident panel: `x` (n, q0) = [1 | covariates | pseudo-QTN columns] with the QTN columns from `q_base` on.  Rows
    decode additively with major-allele imputation (`farmcpu_missing_value`).  Host: `farmcpu.design_operands`; device: the
    products G [Q | r_y] (`jxg_lmt_sums_p32`, Q as two operands) and `jxg_farmcpu_fem_stats` per block of rows; the bits of a row
    do not depend on `block_rows`.  -> FarmcpuFem(p: (len(rows),) f64 device tensor, void rows 1; qtn_min_p: host (q0 - q_base,)
    = per QTN slot the p of the largest t^2 of its restated coefficient over the non-void rows (1 where there is none);
    stats: (len(rows), 3) device tensor [beta, se, p], void rows (NaN, NaN, 1))."""
    from . import lm2
    des, out, maxbits = _farmcpu_scan(panel, rows, af, flip, x, q_base, y, False, block_rows)
    t2 = maxbits.cpu().numpy().view(np.float64)
    qmin = np.array([lm2.student_t_two_sided(math.sqrt(v), des.df) if v > 0.0 else 1.0 for v in t2], dtype=np.float64)
    return FarmcpuFem(out[:, 2], qmin, out)


def scan_rows_farmcpu_final(panel: Panel, rows: np.ndarray, af: np.ndarray, flip, x: np.ndarray, q_base: int, y: np.ndarray,
                            block_rows=None) -> torch.Tensor:
    """Final scan of FarmCPU's raw route against the final design (`write_farmcpu_packed_main_scan`, src/stats/farmcpu.rs:
    3613-3650; `jxg_farmcpu_final_stats`): a (len(rows), 3) f64 device tensor [beta, se, p], three NaN for a void row.  The rows
    of the QTNs themselves are the caller's (they take the background fit's coefficients)."""
    return _farmcpu_scan(panel, rows, af, flip, x, q_base, y, True, block_rows)[1]


def scan_rows_lm2(panel: Panel, rows: np.ndarray, af: np.ndarray, x: np.ndarray, cov_sel: np.ndarray, y: np.ndarray, flip=None,
                  block_rows=LM_BLOCK_ROWS, progress=None, progress_every=0):
    """SNP-by-covariate interaction scan of the given SNP rows of a resident panel (`lm2_fit_single_snp`, src/stats/glm2.rs:
    142-325): per SNP y ~ X + g + g o c_1 + ... + g o c_k with c = the columns of `cov_sel` (n, k), k <= 8; `x` (n, q_base)
    includes the intercept.  Host: the Gram-Schmidt basis of X, r_y and the weight columns (`lm2.py`), once; device: one pass
    of the moment kernel and the per-SNP algebra per `block_rows` rows (`jxg_lm2_scan_p32`); rows whose Schur complement has
    no plain inverse come back flagged and are solved here with the pseudo-inverse, from the device sums.
    Returns a (len(rows), 4 (1 + k) + 4) f64 device tensor: (beta, se, chisq, pwald) of the SNP and of each interaction, then
    chisq_int_joint, p_int_joint, chisq_joint, p_joint."""
    from . import lm2
    from .janusx import _raw_additive_lut
    dev, n = panel.device, panel.n
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    x = np.ascontiguousarray(x, dtype=np.float64)
    cov_sel = np.ascontiguousarray(cov_sel, dtype=np.float64).reshape(len(y), -1)
    if y.shape[0] != n or x.shape[0] != n:
        raise RuntimeError(f"selected sample count {panel.n} != len(y) {y.shape[0]}")
    q_base, k = int(x.shape[1]), int(cov_sel.shape[1])
    if k < 1:
        raise RuntimeError("LM2 requires at least one explicitly selected covariate column.")
    if k > lm2.LM2_MAX_INTERACTIONS:
        raise RuntimeError(f"LM2 supports at most {lm2.LM2_MAX_INTERACTIONS} interaction covariates in this build, got {k}")
    if n <= q_base + 1 + k:
        raise RuntimeError(f"n too small: require n > q_base + 1 + n_interactions, got n={n}, q_base={q_base}, "
                           f"n_interactions={k}")
    if not np.all(np.isfinite(cov_sel)):
        raise RuntimeError("LM2 interaction covariates contain non-finite values")
    mk, ncol = len(rows), 4 * (1 + k) + 4
    out = torch.empty((mk, ncol), dtype=torch.float64, device=dev)
    if mk == 0:
        return out
    q, r_y, rss0 = lm2.qr_projection(x, y)
    q_rank, df = int(q.shape[1]), n - (q_base + 1 + k)       # df counts the columns of X as given, also when some were dropped
    img, nblk, nblk_v = lm2.weight_image(*lm2.weight_columns(q, r_y, cov_sel))
    img_t = torch.from_numpy(img).to(dev)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    # [0, max(2 af, 0), 1, 2], the calls mirrored where `flip` (`decode_packed_row_model_into_f64`, src/decode/decode.rs:307-364)
    lut_t = torch.from_numpy(_raw_additive_lut(af, np.zeros(mk, dtype=bool) if flip is None else flip, True)).to(dev)
    br = int(max(1, min(block_rows, mk)))
    step, last_tick = (int(progress_every) if progress_every and int(progress_every) > 0 else br), 0
    sums = torch.empty((br, nblk * 16), dtype=torch.float64, device=dev)
    flag = torch.zeros(br, dtype=torch.int32, device=dev)
    for r0 in range(0, mk, br):
        nr = min(br, mk - r0)
        check(lib().jxg_lm2_scan_p32(_ptr(panel.p32), panel.m, n, rows_t[r0:].data_ptr(), nr, lut_t[r0:].data_ptr(), _ptr(img_t),
                                     nblk, nblk_v, q_rank, k, rss0, df, _ptr(sums), out[r0:].data_ptr(), _ptr(flag), 0, _stream()))
        # reading the flags waits for the block: nothing at the default block size, a serialisation with small `block_rows`
        bad = torch.nonzero(flag[:nr]).ravel()
        if bad.numel():
            host = sums[bad].cpu().numpy()
            fixed = np.stack([lm2.solve_from_sums(host[i], q_rank, k, nblk_v * 16, rss0, df) for i in range(len(host))])
            out[r0 + bad] = torch.from_numpy(fixed).to(dev)
        if progress is not None and (r0 + nr >= mk or r0 + nr >= last_tick + step):
            last_tick = r0 + nr
            progress(r0 + nr, mk)
    return out


@dataclass
class GwasResult:
    keep: np.ndarray        # (m,) bool, kept SNPs in BED order
    af: np.ndarray          # (m_kept,) f32
    miss: np.ndarray        # (m_kept,) f32
    stats: np.ndarray       # (m_kept, 3) f64 beta, se, p
    null: NullFit
    grm_eff_m: int
    times: dict
    model_tag: str = None   # route that produced `stats`: the requested mode, or "lm" after the null LRT fallback
    null_lrt: tuple = None  # (switch_to_lm, LRT statistic, p) of `gwas_lmm_lm_null_lrt_decision` when it was evaluated


def build_grm(packed: torch.Tensor, n_samples: int, method=1, maf=0.02, geno=0.05, panel: Panel = None,
              payload_sharded: bool = False):
    """`build_grm_streaming` -> `grm_stream_bed_f32` on an HBM-resident payload (all samples; het filter off,
    python/janusx/assoc/workflow.py:2928-3095). Returns (K f32 device tensor (n,n), eff_m, panel).
    Several ranks (torch.distributed initialised, SURVEY.md 8(e) / BASELINE north_star): every rank accumulates the partial
    Z Z' of ITS SNPs -- a contiguous share of the kept rows of a replicated payload, or all kept rows of its own payload shard
    (`payload_sharded`) --, ONE sum-reduction of the lower-triangle tiles of the f64 accumulators (RCCL over xGMI) and of the two
    scalar denominators follows, and every rank finalises the same K."""
    if panel is None:
        panel = Panel(packed, n_samples)
    panel.sharded = bool(payload_sharded)
    counts = panel.counts()
    n = panel.n
    gkeep, mean_g, scale, flip, var = st.stream_grm_row_prepare(counts, n, method, maf, geno, 0.0)
    grows = np.nonzero(gkeep)[0]
    lo, hi = _my_slice(len(grows), payload_sharded)
    grows = grows[lo:hi]
    panel.grm_rows_local = int(len(grows))          # this rank's share (bench.py prices its launch with it)
    totals = torch.tensor([float(np.sum(var[grows])), float(len(grows))], dtype=torch.float64, device=panel.device)
    world = dist_info()[1]
    if world > 1:
        from .dist import allreduce_sum_
        allreduce_sum_(totals)
    var_sum, eff = (float(v) for v in totals.cpu().numpy())
    if int(round(eff)) == 0:
        raise RuntimeError("No SNPs remained after filtering; GRM is empty.")
    denom = var_sum if method == 1 else eff
    if not (math.isfinite(denom) and denom > 0.0):
        raise RuntimeError("invalid centered GRM denominator: sum(2p(1-p)) <= 0")
    glut = st.grm_lut_from_mean_scale(mean_g[grows], scale[grows], flip[grows])
    acc = grm_accumulate(panel, grows, glut)
    if world > 1:
        from .dist import allreduce_grm_accumulator_
        allreduce_grm_accumulator_(acc)
    k32 = grm_finalize(acc, n, denom, torch.float32)
    return k32, int(round(eff)), panel


def trait_null_model(k: torch.Tensor, keep_idx, x: np.ndarray, y: np.ndarray) -> SpectralModel:
    """The spectral null model of one trait: eigh of K[keep, keep] + 1e-6 I, rotation of [X | y], REML null fit (`model.null`).
    What `run_trait` scans with and `jx fvlmm2` tests pairs with."""
    s, ut64 = eigh_from_grm(k, 1e-6, keep_idx, f32_consumer=True)     # only the f32 U^T of SpectralModel is kept
    return SpectralModel(s, ut64, x, y)


def run_trait(packed: torch.Tensor, n_samples: int, k: torch.Tensor, keep_idx, y: np.ndarray, x: np.ndarray,
              mode="lmm", maf=0.02, geno=0.05, het=1.0, max_iter=30, tol=1e-2, warm_start=False, on_rows=None,
              force_model=True, payload_sharded: bool = False, warm_chain=None):
    """One trait of `run_chunked_gwas_lmm_lm` (python/janusx/assoc/workflow_model_stream.py:464-1480):
    eigh of K[keep, keep] + 1e-6 I, spectral null model, QC on the trait's samples, rotate + scan.
    `x` includes the intercept column; `y`, `x` are already restricted to keep_idx (in that order).
    `on_rows(keep, af, miss, ncol, model_tag)` (optional) is called once the kept SNP set and the route are known and
    returns the `on_block` callback of `scan_rows` (or None): the streaming writer is opened there.
    force_model=False: the null likelihood-ratio test against the plain LM (`gwas_lmm_lm_null_lrt_decision`) runs after the
    null fit and, when it finds no polygenic variance (p >= 0.05), the trait is scanned with the LM instead
    (workflow_model_stream.py:930-963; result.model_tag == "lm", three columns beta, se, Student-t p).
    Several ranks (torch.distributed initialised; `init_distributed`): the eigendecomposition is shared out over the ranks, the
    null model is fitted on every rank (deterministic), every rank scans ITS kept SNPs -- a contiguous share of the kept rows of
    a replicated payload, or the kept rows of its own payload shard (`payload_sharded`) -- and the result rows are gathered in
    BED order on every rank; `on_rows` is called on rank 0 only, with the whole table as one block.
    warm_chain = (chunk_rows, pieces) ('lmm' only): the reference's default scan of this route (`lmm_reml_assoc_bed_to_tsv_f32`
    as workflow_model_stream.py:1449-1480 calls it: init_log10_lbd = log10 lambda0, rotate_block_rows = the CLI chunk size,
    warm-start chain on, src/stats/lmm.rs:2627): a chain is the kept rows of one chunk of `chunk_rows` SNP rows of the file
    (`stats.warm_chain_blocks_bed`), cut into `pieces` by halving.  On several ranks over a replicated payload the rows are dealt
    at chain boundaries (same table as one rank); with a payload shard per rank the chunks count from the shard's first row."""
    rank, world = dist_info()
    keep_idx = None if keep_idx is None else np.asarray(keep_idx, dtype=np.int64)
    model = trait_null_model(k, keep_idx, x, y)
    panel = Panel(packed, n_samples, keep_idx)
    panel.sharded = bool(payload_sharded)
    counts = panel.counts()
    n = panel.n
    keep, af, miss = st.gwas_scan_row_stats(counts, n, maf, geno, het)
    rows = np.nonzero(keep)[0]
    chain_off = None
    if warm_chain is not None and mode == "lmm":
        chain_off = st.warm_chain_offsets(st.warm_chain_blocks_bed(rows, panel.m, int(warm_chain[0])), len(rows), int(warm_chain[1]))
        warm_start = True            # the route passes init_log10_lbd = log10 lambda0 (workflow_model_stream.py:1436-1440)
    if world > 1:
        return _run_trait_ranks(panel, model, counts, keep, af, miss, rows, y, x, mode, max_iter, tol, warm_start, on_rows,
                                force_model, payload_sharded, chain_off)
    lut = st.scan_lut_from_counts(af[rows], np.zeros(len(rows), dtype=bool), counts[rows], n)
    lrt = None
    if not force_model:
        from .janusx import gwas_lmm_lm_null_lrt_decision
        sw, stat, pv, _ml = gwas_lmm_lm_null_lrt_decision(y, np.asarray(x)[:, 1:], model.null.ml0)
        lrt = (sw, stat, pv)
        if sw:
            # the reference's LM routes print the COUNT of missing samples in the miss column (AssocMissValue::Count,
            # src/io/assoc2tsv.rs:452-458; the streaming writer formats rint(miss) as an integer)
            miss_cnt = counts[rows, 0].astype(np.float32)
            on_block = on_rows(keep, af[rows], miss_cnt, 3, "lm") if on_rows is not None else None
            out = scan_rows_lm(panel, rows, af[rows], x, y, on_block=on_block)
            res = GwasResult(keep, af[rows], miss_cnt, out[:, :3].cpu().numpy(), model.null, 0, {})
            res.model_tag, res.null_lrt = "lm", lrt
            return res
    on_block = on_rows(keep, af[rows], miss[rows], 6 if mode == "lmm2" else 3, mode) if on_rows is not None else None
    out = _scan_trait(panel, model, rows, lut, mode, max_iter, tol, warm_start, chain_off, on_block)
    res = GwasResult(keep, af[rows], miss[rows], out.cpu().numpy(), model.null, 0, {})
    res.model_tag, res.null_lrt = mode, lrt
    return res


@dataclass
class TraitsResult:
    keep: np.ndarray        # (m,) bool, kept SNPs in BED order
    af: np.ndarray          # (m_kept,) f32
    miss: np.ndarray        # (m_kept,) f32 missing rate
    stats: np.ndarray       # (T, m_kept, 3) f64 beta, se, p -- None when `switch` is set
    nulls: list             # T NullFit
    null_lrt: list = None   # per trait (switch_to_lm, LRT statistic, p) when the decision was evaluated
    switch: int = None      # index of the first trait whose null LRT asks for the LM: nothing was scanned


def traits_chain_offsets(m_kept: int, chunk: int, pieces: int = 1):
    """Warm-start chains of the trait-level LMM route: blocks of `chunk` KEPT rows, as on the packed route
    (`lmm_reml_assoc_packed_f32` per trait, workflow_model_packed.py:6473-6493), cut into `pieces` by halving."""
    return st.warm_chain_offsets(st.warm_chain_blocks_packed(int(m_kept), int(chunk), 0), int(m_kept), int(pieces))


def run_traits_lmm(packed: torch.Tensor, n_samples: int, k: torch.Tensor, keep_idx, Y: np.ndarray, x: np.ndarray, maf=0.02,
                   geno=0.05, het=1.0, force_model=True, warm_chain=None, on_trait=None) -> TraitsResult:
    """One group of traits measured on the same samples with the same design, scanned together (trait-level LMM,
    `_run_mixed_trait_packed_multi_entry`, python/janusx/assoc/workflow_model_packed.py:5932-6723): ONE eigendecomposition of
    K[keep, keep] + 1e-6 I, ONE rotation of [X | Y], per trait the null fit (-5, 5, 50, 1e-3) and its profile, ONE QC pass and
    ONE rotation of every SNP block for all traits (`scan_rows_lmm_traits`: bounds [-5, 5], max_iter 50, tol 1e-2, start log10
    lambda0 of the trait where it is finite and positive).  Y: (T, n_keep), x with the intercept, both restricted to keep_idx.
    warm_chain = (chunk, pieces) or None (no chains).  force_model=False: `gwas_lmm_lm_null_lrt_decision` per trait; if any
    trait would switch to the LM nothing is scanned and `switch` names the first such trait (the caller runs the group trait by
    trait).  One rank only."""
    if dist_info()[1] > 1:
        raise RuntimeError("run_traits_lmm runs on one rank")
    keep_idx = None if keep_idx is None else np.asarray(keep_idx, dtype=np.int64)
    Y = np.ascontiguousarray(np.atleast_2d(np.asarray(Y, dtype=np.float64)))
    s, ut64 = eigh_from_grm(k, 1e-6, keep_idx, f32_consumer=True)
    models = SpectralModel.for_traits(s, ut64, x, Y)
    del ut64
    nulls = [mdl.null for mdl in models]
    panel = Panel(packed, n_samples, keep_idx)
    counts = panel.counts()
    n = panel.n
    keep, af, miss = st.gwas_scan_row_stats(counts, n, maf, geno, het)
    rows = np.nonzero(keep)[0]
    lrt = None
    if not force_model:
        from .janusx import gwas_lmm_lm_null_lrt_decision
        lrt = [tuple(gwas_lmm_lm_null_lrt_decision(Y[ti], np.asarray(x)[:, 1:], nulls[ti].ml0)[:3]) for ti in range(len(models))]
        sw = [ti for ti, d in enumerate(lrt) if d[0]]
        if sw:
            return TraitsResult(keep, af[rows], miss[rows], None, nulls, lrt, sw[0])
    lut = st.scan_lut_from_counts(af[rows], np.zeros(len(rows), dtype=bool), counts[rows], n)
    init = np.array([math.log10(nf.lbd) if (math.isfinite(nf.lbd) and nf.lbd > 0.0) else float("nan") for nf in nulls])
    chain_off = traits_chain_offsets(len(rows), warm_chain[0], warm_chain[1]) if warm_chain is not None else None
    out = scan_rows_lmm_traits(panel, models[0], rows, lut, models[0].y_rot, init, chain_off=chain_off, on_trait=on_trait)
    return TraitsResult(keep, af[rows], miss[rows], out.cpu().numpy(), nulls, lrt, None)


def _scan_trait(panel, model, rows, lut, mode, max_iter, tol, warm_start, chain_off, on_block=None):
    """One trait's scan with the seeds of its route: 'lmm' from log10 lambda0 when `warm_start`, 'lmm2' always, with the null ML."""
    if mode == "lmm":
        return scan_rows(panel, model, rows, lut, "lmm", max_iter=max_iter, tol=tol, on_block=on_block, chain_off=chain_off,
                         init_log10_lbd=model.warm_seed() if warm_start else None)
    if mode == "lmm2":
        init, ml0 = model.null_ml(max_iter, tol)
        return scan_rows(panel, model, rows, lut, "lmm2", max_iter=max_iter, tol=tol, init_log10_lbd=init, nullml=ml0,
                         on_block=on_block)
    return scan_rows(panel, model, rows, lut, "fvlmm", on_block=on_block)


def _run_trait_ranks(panel, model, counts, keep, af, miss, rows, y, x, mode, max_iter, tol, warm_start, on_rows, force_model,
                     payload_sharded, chain_off=None):
    """Scan stage of `run_trait` on several ranks: this rank's rows -> gather in BED order -> rank 0 hands the table on."""
    rank, world = dist_info()
    n = panel.n
    lo, hi = _my_slice(len(rows), payload_sharded)
    my_chain = None
    if chain_off is not None and mode == "lmm":
        if not payload_sharded:
            # deal whole chains: the cut nearest to the even share, so that no chain starts without its predecessor's state
            cuts = st.deal_whole_chains(chain_off, world)
            lo, hi = int(cuts[rank]), int(cuts[rank + 1])
        inside = chain_off[(chain_off >= lo) & (chain_off <= hi)] - lo
        my_chain = np.unique(np.concatenate([[0], inside, [hi - lo]])).astype(np.int64)
    mine = rows[lo:hi]
    lrt, tag, ncol = None, mode, (6 if mode == "lmm2" else 3)
    miss_col = miss[rows]
    if not force_model:
        from .janusx import gwas_lmm_lm_null_lrt_decision
        sw, stat, pv, _ml = gwas_lmm_lm_null_lrt_decision(y, np.asarray(x)[:, 1:], model.null.ml0)   # same on every rank
        lrt = (sw, stat, pv)
        if sw:
            tag, ncol = "lm", 3
            miss_col = counts[rows, 0].astype(np.float32)
    if tag == "lm":
        out = scan_rows_lm(panel, mine, af[mine], x, y)[:, :3].contiguous()
    else:
        lut = st.scan_lut_from_counts(af[mine], np.zeros(len(mine), dtype=bool), counts[mine], n)
        out = _scan_trait(panel, model, mine, lut, mode, max_iter, tol, warm_start, my_chain if len(mine) else None)
    out = _allgather_rows(out)
    keep_all, af_k, miss_k = keep, af[rows], miss_col
    if payload_sharded:       # the QC columns are per shard too: concatenate them in rank (= BED) order
        keep_all, af_k, miss_k = _allgather_np(keep), _allgather_np(af[rows]), _allgather_np(miss_col)
    stats = out.cpu().numpy()
    if on_rows is not None and rank == 0:
        on_block = on_rows(keep_all, af_k, miss_k, ncol, tag)
        if on_block is not None:
            on_block(0, stats)
    res = GwasResult(keep_all, af_k, miss_k, stats, model.null, 0, {})
    res.model_tag, res.null_lrt = tag, lrt
    return res


def run_gwas(packed: torch.Tensor, n_samples: int, y: np.ndarray, covar: np.ndarray = None, mode="lmm",
             maf=0.02, geno=0.05, het=1.0, grm_method=1, max_iter=30, tol=1e-2, timing=True,
             payload_sharded: bool = False, warm_chain=None) -> GwasResult:
    """`jx gwas -lmm/-fvlmm` on an HBM-resident payload (all samples phenotyped): GRM -> eigh -> null REML -> per-SNP scan.
    Several ranks (torch.distributed initialised; `init_distributed`): the composition of SURVEY.md 8(e) -- SNP-sharded GRM with
    one sum-reduction (`build_grm`), eigenvectors shared out over the ranks (`eigh_from_grm`), SNP-sharded scan, result rows
    gathered in BED order on every rank; `packed` is the whole payload on every rank, or this rank's contiguous SNP shard of it
    (`payload_sharded`)."""
    tm = StageTimes()

    def tick():
        if timing:
            torch.cuda.synchronize()
        return time.perf_counter()

    t0 = tick()
    panel = Panel(packed, n_samples)
    counts = panel.counts()
    n = panel.n
    t1 = tick()
    tm.add("prep", t1 - t0)
    # GRM: `grm_stream_bed_f32` defaults maf/geno from the CLI, het filter off (workflow.py:3095)
    k32, geff, _ = build_grm(packed, n_samples, grm_method, maf, geno, panel=panel, payload_sharded=payload_sharded)
    t2 = tick()
    tm.add("grm", t2 - t1)
    s, ut64 = eigh_from_grm(k32, 1e-6, f32_consumer=True)             # only the f32 U^T of SpectralModel is kept
    t3 = tick()
    tm.add("eigh", t3 - t2)
    x = np.ones((n, 1)) if covar is None else np.concatenate([np.ones((n, 1)), np.asarray(covar, dtype=np.float64)], 1)
    model = SpectralModel(s, ut64, x, y)
    del ut64
    t4 = tick()
    tm.add("null", t4 - t3)
    keep, af, miss = st.gwas_scan_row_stats(counts, n, maf, geno, het)
    rows = np.nonzero(keep)[0]
    lo, hi = _my_slice(len(rows), payload_sharded)
    mine = rows[lo:hi]
    lut = st.scan_lut_from_counts(af[mine], np.zeros(len(mine), dtype=bool), counts[mine], n)
    if mode == "lmm":
        chain_off, init = None, None
        if warm_chain is not None:       # the reference CLI's scan: chains over chunks of the file's rows, seeded with lambda0
            chain_off = st.warm_chain_offsets(st.warm_chain_blocks_bed(mine, panel.m, int(warm_chain[0])), len(mine),
                                              int(warm_chain[1]))
            init = model.warm_seed()
        out = scan_rows(panel, model, mine, lut, "lmm", max_iter=max_iter, tol=tol, init_log10_lbd=init,
                        times=tm if timing else None, chain_off=chain_off)
    else:
        out = scan_rows(panel, model, mine, lut, "fvlmm", times=tm if timing else None)
    res = _allgather_rows(out).cpu().numpy()
    af_k, miss_k = af[rows], miss[rows]
    if payload_sharded and dist_info()[1] > 1:
        keep, af_k, miss_k = _allgather_np(keep), _allgather_np(af_k), _allgather_np(miss_k)
    t5 = tick()
    tm.add("scan_total", t5 - t4)
    tm.add("total", t5 - t0)
    return GwasResult(keep, af_k, miss_k, res, model.null, geff, tm.t)


class MultiKernelReml:
    """Device-resident evaluation of the multi-kernel REML of `ai_reml_multi_f64` (src/stats/reml.rs:703-1049):
    V = sum_j theta_j K_j + theta_e I is formed, factored and solved in HBM (csrc/k_potrf.hip: `jxg_reml_combine_f64`,
    `jxg_dpotrf_lower_f64`, `jxg_dpotrs_lower_f64`); the p x p and m x m algebra is host f64 numpy.

    `k_stack` (q, n, n) numpy or CUDA f64 tensor, symmetrised as the reference does ((K + K') / 2, reml.rs:776) and kept in HBM;
    `x` (n, p) fixed-effect design, `y` (n,).  The factor and the pieces of the last `profile` are kept: asking for the same theta
    again (the accepted line-search candidate becomes the next iteration's theta) costs nothing and changes no number."""

    def __init__(self, k_stack, x, y):
        ks = k_stack if torch.is_tensor(k_stack) else torch.from_numpy(np.ascontiguousarray(k_stack, dtype=np.float64))
        if ks.dim() != 3 or ks.shape[1] != ks.shape[2] or ks.shape[0] < 1:
            raise RuntimeError("k_stack must be (q, n, n)")
        ks = ks.to(device="cuda", dtype=torch.float64)
        self.ks = ((ks + ks.transpose(1, 2)) * 0.5).contiguous()
        del ks
        self.q, self.n = int(self.ks.shape[0]), int(self.ks.shape[1])
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.n, -1)
        self.y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        self.p = int(self.x.shape[1])
        self.v = torch.empty((self.n, self.n), dtype=torch.float64, device="cuda")
        self.logdet = float("nan")
        self._fac_key = None
        self._prof_key, self._prof = None, None
        self.n_factor = 0                       # factorisations done (the timing script and the tests read it)

    # ---- device pieces --------------------------------------------------------------------------------------------------------
    @staticmethod
    def _key(theta):
        return np.ascontiguousarray(theta, dtype=np.float64).reshape(-1).tobytes()

    def _factor(self, theta):
        """The Cholesky factor of V(theta) in the lower triangle of self.v; False when a pivot fails (the reference's
        `v.cholesky()` returning None)."""
        th = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        if th.shape[0] != self.q + 1:
            raise RuntimeError(f"theta must have q + 1 = {self.q + 1} entries")
        key = th.tobytes()
        if key == self._fac_key:
            return True
        self._fac_key = None
        import ctypes as C
        info = C.c_int(0)
        ld = C.c_double(0.0)
        check(lib().jxg_reml_combine_f64(self.ks.data_ptr(), self.q, self.n, th.ctypes.data, self.v.data_ptr(), _stream()))
        check(lib().jxg_dpotrf_lower_f64(self.v.data_ptr(), self.n, self.n, C.addressof(info), _stream()))
        self.n_factor += 1
        if info.value != 0:
            return False
        check(lib().jxg_potrf_logdet_f64(self.v.data_ptr(), self.n, self.n, C.addressof(ld), _stream()))
        self.logdet = float(ld.value)
        self._fac_key = key
        return True

    def solve(self, cols):
        """V^-1 applied to the columns `cols` (n, c) numpy -> (n, c) numpy, with the current factor."""
        b = torch.from_numpy(np.ascontiguousarray(np.asarray(cols, dtype=np.float64).reshape(self.n, -1).T)).cuda()
        check(lib().jxg_dpotrs_lower_f64(self.v.data_ptr(), self.n, self.n, b.data_ptr(), int(b.shape[0]), self.n, _stream()))
        return np.ascontiguousarray(b.cpu().numpy().T)

    def _kernel_products(self, cols):
        """K_j cols for every kernel: one dgemm each -> list of q (n, c) numpy arrays."""
        r = torch.from_numpy(np.ascontiguousarray(np.asarray(cols, dtype=np.float64).T)).cuda()      # (c, n): column-major n x c
        c = int(r.shape[0])
        out = torch.empty_like(r)
        res = []
        for j in range(self.q):
            check(lib().jxg_dgemm_f64(0, 0, self.n, c, self.n, 1.0, self.ks[j].data_ptr(), self.n, r.data_ptr(), self.n, 0.0,
                                      out.data_ptr(), self.n, 0, _stream()))
            res.append(np.ascontiguousarray(out.cpu().numpy().T))
        return res

    def _traces_exact(self):
        """tr(V^-1 K_j), j < q, and tr(V^-1): V^-1 by n solves on the identity, the traces by `jxg_sym_dot_f64`."""
        vinv = torch.eye(self.n, dtype=torch.float64, device="cuda")
        check(lib().jxg_dpotrs_lower_f64(self.v.data_ptr(), self.n, self.n, vinv.data_ptr(), self.n, self.n, _stream()))
        out = torch.empty(self.q, dtype=torch.float64, device="cuda")
        for j in range(self.q):
            check(lib().jxg_sym_dot_f64(vinv.data_ptr(), self.ks[j].data_ptr(), self.n, self.n, self.n, out[j:].data_ptr(), _stream()))
        tr = list(out.cpu().numpy())
        tr.append(float(np.sum(vinv.diagonal().cpu().numpy())))
        return np.asarray(tr, dtype=np.float64)

    # ---- the two blocks of the iteration ----------------------------------------------------------------------------------------
    def profile(self, theta):
        """reml.rs:833-884 (and 966-1012 for a candidate): -> (reml, ml, pieces), or None where the reference breaks or halves the
        step: a failed Cholesky of V or of X'V^-1X, r'V^-1r not positive and finite, a value that is not finite.  One rule serves
        both uses, so a candidate whose ml alone is not finite is rejected too, where reml.rs:1013 tests only reml_cand; with
        r'V^-1r positive and finite the two differ by finite terms, so the case does not arise."""
        key = self._key(theta)
        if key == self._prof_key:
            return self._prof
        self._prof_key, self._prof = None, None
        if not self._factor(theta):
            return None
        n, p, x, y = self.n, self.p, self.x, self.y
        sol = self.solve(np.concatenate([x, y[:, None]], axis=1))
        vinv_x, vinv_y = sol[:, :p], sol[:, p]
        xt_vinv_x = x.T @ vinv_x
        try:
            lx = np.linalg.cholesky(xt_vinv_x)
        except np.linalg.LinAlgError:
            return None
        eye_p = np.eye(p)
        c_inv = np.linalg.solve(lx.T, np.linalg.solve(lx, eye_p))
        beta = np.linalg.solve(lx.T, np.linalg.solve(lx, x.T @ vinv_y))
        r = y - x @ beta
        vinv_r = self.solve(r[:, None])[:, 0]
        alpha = vinv_r - vinv_x @ (c_inv @ (x.T @ vinv_r))
        qval = float(r @ vinv_r)
        if not np.isfinite(qval) or qval <= 0.0:
            return None
        log_det_v = self.logdet
        log_det_xt = float(2.0 * np.sum(np.log(np.diag(lx))))
        nf, pf = float(n), float(p)
        reml_c = (nf - pf) * (math.log(nf - pf) - 1.0 - math.log(2.0 * math.pi)) / 2.0
        reml = reml_c - 0.5 * ((nf - pf) * math.log(qval) + log_det_v + log_det_xt)
        ml_c = nf * (math.log(nf) - 1.0 - math.log(2.0 * math.pi)) / 2.0
        ml = ml_c - 0.5 * (nf * math.log(qval) + log_det_v)
        if not np.isfinite(reml) or not np.isfinite(ml):
            return None
        pieces = {"vinv_x": vinv_x, "c_inv": c_inv, "beta": beta, "r": r, "vinv_r": vinv_r, "alpha": alpha, "qval": qval,
                  "log_det_v": log_det_v, "log_det_xt": log_det_xt}
        self._prof_key, self._prof = key, (float(reml), float(ml), pieces)
        return self._prof

    def ai_step(self, theta, probes=None):
        """reml.rs:886-952: -> (score, ai, delta) at theta, or None where the reference breaks (no factor, a singular AI matrix, a
        step that is not finite).  probes None: the exact trace through V^-1; otherwise `probes` (n_probes, n) of +-1 and the
        Hutchinson estimate with the cached V^-1 z."""
        prof = self.profile(theta)
        if prof is None:
            return None
        if not self._factor(theta):             # the factor of this theta (a failed candidate in between replaces it)
            return None
        pc = prof[2]
        n, p, q, m = self.n, self.p, self.q, self.q + 1
        alpha, vinv_x, c_inv = pc["alpha"], pc["vinv_x"], pc["c_inv"]
        cols = [alpha[:, None], vinv_x]
        if probes is not None:
            z = np.ascontiguousarray(probes, dtype=np.float64).reshape(-1, n)
            vinv_z = self.solve(z.T)
            cols.append(z.T)
            tr1 = np.zeros(m)
        else:
            tr1 = self._traces_exact()
        rmat = np.concatenate(cols, axis=1)
        prods = self._kernel_products(rmat) + [rmat]            # the residual's kernel is the identity
        score = np.zeros(m)
        ka = np.empty((n, m))
        for j in range(m):
            kr = prods[j]
            ka[:, j] = kr[:, 0]
            quad = float(alpha @ kr[:, 0])
            if probes is not None:
                kz = kr[:, 1 + p:]
                s = 0.0
                for i in range(z.shape[0]):
                    s += float(vinv_z[:, i] @ kz[:, i])
                tr1[j] = s / float(z.shape[0])
            bt_kb = vinv_x.T @ kr[:, 1:1 + p]
            tr2 = float(np.sum(c_inv * bt_kb.T))
            score[j] = -0.5 * ((tr1[j] - tr2) - quad)
        vinv_ka = self.solve(ka)
        pka = vinv_ka - vinv_x @ (c_inv @ (vinv_x.T @ ka))
        ai = np.zeros((m, m))
        for a in range(m):
            for b in range(a + 1):
                ai[a, b] = ai[b, a] = 0.5 * float(ka[:, a] @ pka[:, b])
        ai[np.diag_indices(m)] += 1e-10
        try:
            delta = np.linalg.solve(ai, score)
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(delta)):
            return None
        return score, ai, delta
