"""Neighbour-joining tree of packed genotypes: the mirrors and extensions behind `jx tree -nj` (re-exported by `janusx.py`).

Behaviour: src/stats/tree.rs and python/janusx/script/tree.py of the reference.  The pair counts (csrc/k_tree.hip, two int8 Grams
on the matrix pipes) and the whole neighbour-joining loop (row sums, argmin, merge: no host round trip per step) run on the
device; the JC69 transform - the route's only transcendental - the branch lengths and the Newick text are host numpy / Python
floats over the device's merge log, so that apart from one `ln` per pair the tree is a pure function of integer counts and IEEE
`+ - * /`.  Exact mode only; zeros that come out of a clamp are canonical +0.0 on the alignment route (README, "Known differences").
"""
from __future__ import annotations

import re
import time
import warnings

import numpy as np

from ._lib import check, lib

TREE_MAX_ROWS = 1 << 29

_NJ_MODES_EXACT = ("exact",)
# spellings `nj_newick_from_alignment_u8` accepts (src/stats/tree.rs:7340-7362) -> the mode they select
_NJ_MODES_UNBUILT = {
    "bionj": "bionj", "bio-nj": "bionj", "bio_nj": "bionj",
    "bionj-dist": "bionj-dist", "bionj_dist": "bionj-dist", "bionjdist": "bionj-dist",
    "bionj-jc": "bionj-jc", "bionj_jc": "bionj-jc", "bionjjc": "bionj-jc", "bionj-jc69": "bionj-jc", "bionj_jc69": "bionj-jc",
    "bionj-binom": "bionj-binom", "bionj_binom": "bionj-binom", "bionjbinom": "bionj-binom",
    "bionj-auto": "bionj-auto", "bionj_auto": "bionj-auto", "bionjauto": "bionj-auto",
    "top-hits": "top-hits", "tophits": "top-hits", "top_hits": "top-hits",
    "rapidnj": "rapidnj", "rapid-nj": "rapidnj", "rapid_nj": "rapidnj",
    "lt-lazyq": "lt-lazyq", "lazyq-lt": "lt-lazyq", "lazyq": "lt-lazyq", "rapid-lt": "lt-lazyq", "rapidlt": "lt-lazyq",
    "nnc-lazyq": "lt-lazyq",
    "rapid-core": "rapid-core", "rapid_core": "rapid-core", "rapidcore": "rapid-core", "lt-rapid-core": "rapid-core",
    "rapid-lt-core": "rapid-core",
}


# ------------------------------------------------------------------------------------------------
# letters
# ------------------------------------------------------------------------------------------------

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = ord("N")


def _upper(codes):
    """`ascii_upper` (tree.rs:146-152) on a uint8 array."""
    c = np.asarray(codes, dtype=np.uint8)
    return np.where((c >= ord("a")) & (c <= ord("z")), c - np.uint8(32), c).astype(np.uint8)


def first_base_code(s) -> int:
    """`first_base_code`, tree.rs:295-307: the first byte that is not ASCII white space, upper-cased; N unless A / C / G / T."""
    for b in str(s).encode("utf-8"):
        if b in (0x20, 0x09, 0x0A, 0x0C, 0x0D):
            continue
        if 0x61 <= b <= 0x7A:
            b -= 32
        return b if b in b"ACGT" else _N
    return _N


def sanitize_base_pairs(ref_codes, alt_codes):
    """`sanitize_base_pair`, tree.rs:266-292, on uint8 arrays -> (ref, alt) letters, both A / C / G / T."""
    r, a = _upper(ref_codes), _upper(alt_codes)
    r = np.where(np.isin(r, _ACGT), r, np.uint8(_N)).astype(np.uint8)
    a = np.where(np.isin(a, _ACGT), a, np.uint8(_N)).astype(np.uint8)
    rn, an = r == _N, a == _N
    out_r = np.where(rn & an, ord("A"), np.where(rn, np.where(a != ord("A"), ord("A"), ord("C")), r))
    out_a = np.where(rn & an, ord("G"), np.where(an & ~rn, np.where(r != ord("G"), ord("G"), ord("T")), a))
    return out_r.astype(np.uint8), out_a.astype(np.uint8)


_IUPAC = {frozenset(b"AC"): ord("M"), frozenset(b"AG"): ord("R"), frozenset(b"AT"): ord("W"), frozenset(b"CG"): ord("S"),
          frozenset(b"CT"): ord("Y"), frozenset(b"GT"): ord("K")}
_IUPAC_LUT = np.full((256, 256), _N, dtype=np.uint8)
for _pair, _code in _IUPAC.items():
    _x, _y = sorted(_pair)
    _IUPAC_LUT[_x, _y] = _IUPAC_LUT[_y, _x] = _code


def het_iupac(ref_letters, alt_letters):
    """`het_iupac`, tree.rs:310-323, on uint8 arrays: equal letters give that letter."""
    r, a = np.asarray(ref_letters, dtype=np.uint8), np.asarray(alt_letters, dtype=np.uint8)
    return np.where(r == a, r, _IUPAC_LUT[r, a]).astype(np.uint8)


def geno_chunk_to_alignment_u8(geno, ref_codes, alt_codes):
    """`geno_chunk_to_alignment_u8`, tree.rs:7170-7183 over `convert_geno_to_alignment_u8` :6931-7002: (m sites, n samples) f32
    values and one ref / alt byte per site -> (n, m) uint8 letters: value <= 0.5 the ref letter, >= 1.5 the alt letter, in between
    the IUPAC het code, not finite or negative N."""
    g = np.asarray(geno, dtype=np.float32)
    if g.ndim != 2:
        raise ValueError("geno chunk must be 2D float32 array: (n_sites, n_samples)")
    rc = np.asarray(ref_codes, dtype=np.uint8).ravel()
    ac = np.asarray(alt_codes, dtype=np.uint8).ravel()
    m, n = g.shape
    if rc.shape[0] != m or ac.shape[0] != m:
        raise ValueError(f"ref/alt length mismatch: expected {m}, got {rc.shape[0]}/{ac.shape[0]}")
    if m == 0 or n == 0:
        return np.zeros((n, m), dtype=np.uint8)
    r, a = sanitize_base_pairs(rc, ac)
    h = het_iupac(r, a)
    with np.errstate(invalid="ignore"):
        out = np.where(~np.isfinite(g) | (g < 0.0), np.uint8(_N),
                       np.where(g <= 0.5, r[:, None], np.where(g >= 1.5, a[:, None], h[:, None])))
    return np.ascontiguousarray(out.astype(np.uint8).T)


def geno_chunk_to_alignment_u8_sites(geno, ref_alleles, alt_alleles):
    """`geno_chunk_to_alignment_u8_sites`, tree.rs:7237-7256: allele strings, reduced by `first_base_code`."""
    ref_alleles, alt_alleles = list(ref_alleles), list(alt_alleles)
    if len(ref_alleles) != len(alt_alleles):
        raise ValueError(f"ref_alleles/alt_alleles length mismatch: {len(ref_alleles)}/{len(alt_alleles)}")
    rc = np.array([first_base_code(s) for s in ref_alleles], dtype=np.uint8)
    ac = np.array([first_base_code(s) for s in alt_alleles], dtype=np.uint8)
    return geno_chunk_to_alignment_u8(geno, rc, ac)


def geno_chunk_to_alignment_u8_siteinfo(geno, sites):
    """`geno_chunk_to_alignment_u8_siteinfo`, tree.rs:7258-7283: `sites` carry `.ref_allele` / `.alt_allele`."""
    g = np.asarray(geno, dtype=np.float32)
    sites = list(sites)
    m = int(g.shape[0]) if g.ndim == 2 else -1
    if g.ndim == 2 and len(sites) != m:
        raise ValueError(f"sites length mismatch: expected {m}, got {len(sites)}")
    return geno_chunk_to_alignment_u8_sites(g, [s.ref_allele for s in sites], [s.alt_allele for s in sites])


def packed_site_letters(ref_alleles, alt_alleles, flip):
    """Letters of the 2-bit codes of every site as the chunk loader and the conversion give them -> (l00, l10, l11) uint8 (m):
    a flipped site (alt frequency > 0.5, gfcore.rs:454-462) has its values turned round AND its allele strings swapped, which
    matters where `sanitize_base_pair` replaces a non-ACGT allele."""
    rc = np.array([first_base_code(s) for s in ref_alleles], dtype=np.uint8)
    ac = np.array([first_base_code(s) for s in alt_alleles], dtype=np.uint8)
    flip = np.asarray(flip, dtype=bool)
    r, a = sanitize_base_pairs(np.where(flip, ac, rc), np.where(flip, rc, ac))
    return np.where(flip, a, r).astype(np.uint8), het_iupac(r, a), np.where(flip, r, a).astype(np.uint8)


def _unpack_codes(packed, n):
    pk = np.asarray(packed, dtype=np.uint8)
    codes = np.stack([(pk >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(pk.shape[0], -1)
    return codes[:, :n]


def packed_to_alignment_u8(packed, n_samples, l00, l10, l11):
    """(n, m) uint8 letters of a packed payload (m, ceil(n / 4)) from the per-site letters of `packed_site_letters`; 01 -> N."""
    n = int(n_samples)
    lut = np.stack([np.asarray(l00, dtype=np.uint8), np.full(len(l00), _N, dtype=np.uint8), np.asarray(l10, dtype=np.uint8),
                    np.asarray(l11, dtype=np.uint8)], axis=1)                    # (m, 4) by code
    m = lut.shape[0]
    out = np.empty((n, m), dtype=np.uint8)
    step = max(1, (1 << 24) // max(n, 1))
    for r0 in range(0, m, step):
        codes = _unpack_codes(packed[r0:r0 + step], n)
        out[:, r0:r0 + step] = np.take_along_axis(lut[r0:r0 + step], codes.astype(np.intp), axis=1).T
    return out


# ------------------------------------------------------------------------------------------------
# Newick
# ------------------------------------------------------------------------------------------------

def quote_newick_name(name) -> str:
    """`quote_newick_name`, tree.rs:159-168: ASCII letters, digits, `_`, `.`, `-` pass; anything else is quoted, `'` -> `_`."""
    name = str(name)
    if all(ch.isascii() and (ch.isalnum() or ch in "_.-") for ch in name):
        return name
    return "'" + name.replace("'", "_") + "'"


def format_branch_length(x) -> str:
    """Rust's `{:.10}` of an f64: the correctly rounded text, `-0.0` keeps its sign."""
    return format(float(x), ".10f")


def render_newick(names, joins, root) -> str:
    """`render_newick`, tree.rs:179-193, without recursion (a caterpillar of 20 000 leaves is 20 000 deep): `joins[t]` =
    (left, right, left_len, right_len) of node len(names) + t -> `(L:len,R:len)` nested, no trailing `;`."""
    n = len(names)
    out = []
    stack = [root]
    while stack:
        x = stack.pop()
        if isinstance(x, str):
            out.append(x)
        elif x < n:
            out.append(quote_newick_name(names[x]))
        else:
            left, right, ll, rl = joins[x - n]
            stack.extend((f":{format_branch_length(rl)})", right, f":{format_branch_length(ll)},", left, "("))
    return "".join(out)


def _finite(x):
    return x - x == 0.0


def nj_branch_lengths(dij, ri, rj, m, route):
    """Branch lengths of a join of m active nodes.  route "alignment": tree.rs:7684-7701 (zeros canonical +0.0); "distance":
    tree.rs:7104-7113, followed literally."""
    dij, ri, rj = float(dij), float(ri), float(rj)
    if route == "alignment":
        delta = (ri - rj) / (float(m) - 2.0)
        li = 0.5 * (dij + delta)
        lj = dij - li
        li = li if _finite(li) and li > 0.0 else 0.0
        lj = lj if _finite(lj) and lj > 0.0 else 0.0
        return li, lj
    denom = max(float(m) - 2.0, 1.0)
    li = 0.5 * dij + (ri - rj) / (2.0 * denom)
    lj = dij - li
    if not _finite(li) or li < 0.0:
        li = 0.0
    if not _finite(lj) or lj < 0.0:
        lj = 0.0
    return li, lj


def newick_from_merge_log(names, log_ij, log_vals, last, route) -> str:
    """Newick text (with the trailing `;`) of the device's merge log: joins t = 0 .. n - 3 of (i, j, d_ij, r_i, r_j), then the
    last two nodes and their distance, each getting half of it (tree.rs:7851-7873 / :7149-7166)."""
    n = len(names)
    joins = []
    for t in range(n - 2):
        m = n - t
        dij, ri, rj = (float(v) for v in log_vals[t])
        if route == "alignment" and not _finite((float(m) - 2.0) * dij - ri - rj):
            raise ValueError("failed to build NJ tree: no valid pair found")
        li, lj = nj_branch_lengths(dij, ri, rj, m, route)
        joins.append((int(log_ij[t][0]), int(log_ij[t][1]), li, lj))
    d = float(last)
    if route == "alignment":
        d = d if _finite(d) and d > 0.0 else 0.0
    elif not _finite(d) or d < 0.0:
        d = 0.0
    joins.append((int(log_ij[n - 2][0]), int(log_ij[n - 2][1]), 0.5 * d, 0.5 * d))
    return render_newick(names, joins, n + len(joins) - 1) + ";"


# ------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------

def _check_hbm(need, what):
    import torch
    free = int(torch.cuda.mem_get_info()[0])
    if need > 0.95 * free:
        raise RuntimeError(f"{what}: the working set needs {int(need)} bytes of HBM, {free} bytes are free")


def _nj_run_device(dist, route, timings=None):
    """The NJ loop on the device over a symmetric (n, n) f64 host matrix with a zero diagonal -> (log_ij (n - 1, 2) int32,
    log_vals (n - 2, 3) f64, last f64).  timings (dict): upload_s (host clock) and nj_loop_ms (device events) are added."""
    import torch
    from .pipeline import _ptr, _stream
    n = int(dist.shape[0])
    work_bytes = int(lib().jxg_nj_work_bytes(n))
    _check_hbm(8.0 * n * n + work_bytes + 40.0 * n, f"neighbour joining of {n} samples")
    dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # a read-only host array: only read on its way to the device
        d = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    work = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device=dev)
    log_ij = torch.zeros((n - 1, 2), dtype=torch.int32, device=dev)
    log_vals = torch.zeros((max(n - 2, 1), 3), dtype=torch.float64, device=dev)
    last = torch.zeros(1, dtype=torch.float64, device=dev)
    if timings is not None:
        torch.cuda.synchronize()
        timings["upload_s"] = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib().jxg_nj_run(_ptr(d), n, 0 if route == "alignment" else 1, _ptr(log_ij), _ptr(log_vals), _ptr(last), _ptr(work),
                           _stream()))
    if timings is not None:
        e1.record()
        e1.synchronize()
        timings["nj_loop_ms"] = e0.elapsed_time(e1)
    return log_ij.cpu().numpy(), log_vals.cpu().numpy()[:n - 2], float(last.cpu().numpy()[0])


def nj_merge_log(dist, route="alignment"):
    """Merge log of the exact NJ loop on a symmetric f64 matrix with a zero diagonal (extension; see `newick_from_merge_log`).
    route: "alignment" or "distance" - which clamp the new distances take."""
    if route not in ("alignment", "distance"):
        raise ValueError("route must be 'alignment' or 'distance'")
    d = np.asarray(dist, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1] or d.shape[0] < 2:
        raise ValueError("distance matrix must be square with at least 2 samples")
    return _nj_run_device(d, route)


def _tree_validate_payload(packed, n_samples):
    n = int(n_samples)
    if n < 2:
        raise ValueError("need at least 2 samples to build a tree")
    shape = tuple(int(s) for s in packed.shape)
    if len(shape) != 2 or shape[1] != (n + 3) // 4:
        raise RuntimeError(f"packed must be 2D (m, bytes_per_snp = {(n + 3) // 4})")
    if shape[0] > TREE_MAX_ROWS:
        raise RuntimeError(f"tree pair counts are exact int32 sums: at most {TREE_MAX_ROWS} variant sites, got {shape[0]}")
    return n, shape[0]


def _tree_counts_device(packed, n, same_base):
    """-> (valid, mismatch) int32 (n, n) device tensors."""
    import torch
    from .janusx import _is_device_tensor, _panel
    from .pipeline import _ptr, _stream
    m = int(packed.shape[0])
    _check_hbm(8.0 * n * n, f"tree pair counts of {n} samples")
    dev = torch.device("cuda", torch.cuda.current_device())
    valid = torch.zeros((n, n), dtype=torch.int32, device=dev)
    mism = torch.zeros((n, n), dtype=torch.int32, device=dev)
    if same_base is None:
        parts = [(packed, 0)] if m else []
    else:
        sb = np.asarray(same_base, dtype=bool).ravel()
        if sb.shape[0] != m:
            raise RuntimeError(f"same_base length mismatch: got {sb.shape[0]}, expected {m}")
        parts = []
        for rows, mode in ((np.nonzero(~sb)[0], 0), (np.nonzero(sb)[0], 1)):
            if rows.shape[0] == m:
                parts.append((packed, mode))
            elif rows.shape[0]:
                sel = packed[torch.from_numpy(rows).to(packed.device)] if _is_device_tensor(packed) else np.ascontiguousarray(packed[rows])
                parts.append((sel, mode))
    for k, (pk, mode) in enumerate(parts):
        panel = _panel(pk, n)
        check(lib().jxg_tree_counts_p32(_ptr(panel.p32), panel.m, n, mode, 1 if k else 0, _ptr(valid), _ptr(mism), _stream()))
        del panel
    return valid, mism


def tree_pair_counts_packed(packed, n_samples, same_base=None):
    """(valid, mismatch) int32 (n, n) of a packed payload of biallelic sites (host array or torch CUDA tensor; extension): sites
    where both samples are homozygous, and where they are homozygous for different alleles - the `valid` and `valid - same` of
    `pair_mismatch_stats_bitset` (tree.rs:377-403) on the letters of the payload.  `same_base` (m bools): sites whose two letters
    are equal (an indel such as A / AT): every called sample is known there and the site adds to `valid` alone."""
    n, _m = _tree_validate_payload(packed, n_samples)
    valid, mism = _tree_counts_device(packed, n, same_base)
    return valid.cpu().numpy(), mism.cpu().numpy()


def tree_jc69_distance(valid, mismatch, min_overlap=1):
    """JC69 distances (n, n) f64, symmetric with a zero diagonal, from the pair counts (`pair_distance_bitset` tree.rs:447-453 over
    `mismatch_to_jc69_distance` :365-374; host numpy, the upper triangle transformed and mirrored): with valid >= max(min_overlap,
    1), p = mismatch / valid clamped to [0, 0.75 - 1e-12], d = -0.75 ln(max(1 - 4 p / 3, 1e-12)), floored at +0.0, 1.0 when not
    finite; otherwise 1.0."""
    v = np.asarray(valid)
    mm = np.asarray(mismatch)
    if v.ndim != 2 or v.shape[0] != v.shape[1] or mm.shape != v.shape:
        raise ValueError("valid and mismatch must be square matrices of one shape")
    n = v.shape[0]
    min_ov = max(int(min_overlap), 1)
    out = np.zeros((n, n), dtype=np.float64)
    step = max(1, (1 << 22) // max(n, 1))
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        vb = v[i0:i1, i0:].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.clip(mm[i0:i1, i0:].astype(np.float64) / vb, 0.0, 1.0)
            p = np.clip(p, 0.0, 0.75 - 1e-12)
            d = -0.75 * np.log(np.maximum(1.0 - (4.0 * p / 3.0), 1e-12))
        d = np.where(np.isfinite(d), np.where(d > 0.0, d, 0.0), 1.0)
        d = np.where(v[i0:i1, i0:] >= min_ov, d, 1.0)
        out[i0:, i0:i1] = d.T
        out[i0:i1, i0:] = d
    np.fill_diagonal(out, 0.0)
    return out


def _check_names(sample_ids, n):
    names = [str(s) for s in sample_ids]
    if len(names) != n:
        raise ValueError(f"sample_ids length mismatch: got {len(names)}, expected {n}")
    return names


def nj_newick_from_packed(packed, n_samples, sample_ids, same_base=None, min_overlap=1, max_taxa=20000, timings=None):
    """Exact NJ tree (Newick with `;`) of a packed payload of biallelic sites (extension): `tree_pair_counts_packed`,
    `tree_jc69_distance`, then the loop and lengths of `nj_newick_from_alignment_u8`.  timings (dict): the stages' seconds."""
    n, _m = _tree_validate_payload(packed, n_samples)
    names = _check_names(sample_ids, n)
    if int(max_taxa) == 0:
        raise ValueError("max_taxa must be > 0")
    if n > int(max_taxa):
        raise ValueError(f"n_samples={n} exceeds max_taxa={int(max_taxa)}; NJ in phase-1 is O(N^3)")
    import torch
    t0 = time.perf_counter()
    valid, mism = _tree_counts_device(packed, n, same_base)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    valid, mism = valid.cpu().numpy(), mism.cpu().numpy()
    t2 = time.perf_counter()
    dist = tree_jc69_distance(valid, mism, min_overlap)
    del valid, mism
    t3 = time.perf_counter()
    log = _nj_run_device(dist, "alignment", timings)
    t4 = time.perf_counter()
    text = newick_from_merge_log(names, *log, "alignment")
    if timings is not None:
        timings.update(counts_s=t1 - t0, download_s=t2 - t1, jc69_s=t3 - t2, nj_s=t4 - t3, render_s=time.perf_counter() - t4)
    return text


def normalize_distance_matrix(dist):
    """`normalize_distance_matrix_from_ndarray`, tree.rs:7004-7060: symmetrised (mean of the two finite directions, or the finite
    one), negative -> 0.0, zero diagonal; its errors, the first in its row-major walk, as ValueError."""
    d = np.asarray(dist, dtype=np.float64)
    if d.ndim != 2:
        raise ValueError("distance matrix must be 2D")
    n = d.shape[0]
    if n < 2:
        raise ValueError("need at least 2 samples to build a tree")
    if d.shape[1] != n:
        raise ValueError(f"distance matrix must be square, got {n}x{d.shape[1]}")
    a, b = d, d.T
    fa, fb = np.isfinite(a), np.isfinite(b)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.where(fa & fb, 0.5 * (a + b), np.where(fa, a, b))
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    bad = upper & ~np.isfinite(v)
    diag_bad = ~np.isfinite(np.diagonal(d))
    i_diag = int(np.argmax(diag_bad)) if diag_bad.any() else n
    bad_rows = bad.any(axis=1)
    i_pair = int(np.argmax(bad_rows)) if bad_rows.any() else n
    if i_diag < n and i_diag <= i_pair:
        raise ValueError(f"distance matrix diagonal has NaN/Inf at ({i_diag},{i_diag})")
    if i_pair < n:
        i, j = i_pair, int(np.argmax(bad[i_pair]))
        if not fa[i, j] and not fb[i, j]:
            raise ValueError(f"distance matrix has NaN/Inf in both directions at ({i}, {j}) and ({j}, {i})")
        raise ValueError(f"distance matrix has invalid value after symmetrization at ({i}, {j})")
    v = np.where(v < 0.0, 0.0, v)                                  # -0.0 stays, as `v < 0.0` leaves it
    np.fill_diagonal(v, 0.0)
    return np.ascontiguousarray(v)


def nj_newick_from_distance_matrix(dist, sample_ids, max_taxa=20000):
    """`nj_newick_from_distance_matrix`, tree.rs:7185-7235: exact NJ of a distance matrix -> Newick with `;`."""
    d = np.asarray(dist)
    if d.ndim != 2:
        raise ValueError("distance matrix must be a 2D float matrix: (n_samples, n_samples)")
    n = int(d.shape[0])
    if n < 2:
        raise ValueError("need at least 2 samples to build a tree")
    if d.shape[1] != n:
        raise ValueError(f"distance matrix must be square, got {n}x{d.shape[1]}")
    names = _check_names(sample_ids, n)
    if int(max_taxa) == 0:
        raise ValueError("max_taxa must be > 0")
    if n > int(max_taxa):
        raise ValueError(f"n_samples={n} exceeds max_taxa={int(max_taxa)}; distance-NJ is O(N^3)")
    norm = normalize_distance_matrix(d)
    return newick_from_merge_log(names, *_nj_run_device(norm, "distance"), "distance")


def alignment_to_packed(aln):
    """Biallelic (n, m) uint8 alignment -> (packed (k, ceil(n / 4)) uint8 of the k columns that hold a known base, the first base
    of a column in A < C < G < T order as 00, the second as 11, everything else (IUPAC codes, gaps, N) as 01).  A column with three
    or more distinct bases raises RuntimeError."""
    a = _upper(aln)
    n, m = a.shape
    present = np.stack([(a == b).any(axis=0) for b in _ACGT], axis=0)            # (4, m)
    count = present.sum(axis=0)
    if (count >= 3).any():
        col = int(np.argmax(count >= 3))
        raise RuntimeError(f"alignment column {col} holds {int(count[col])} distinct bases; only biallelic alignments are built "
                           "(every column at most two of A/C/G/T)")
    cols = np.nonzero(count >= 1)[0]
    first = np.argmax(present, axis=0)                                            # index into ACGT of the first base
    second = 3 - np.argmax(present[::-1], axis=0)
    codes = np.full((len(cols), ((n + 3) // 4) * 4), 1, dtype=np.uint8)
    sub = a[:, cols].T                                                            # (k, n)
    body = np.full(sub.shape, 1, dtype=np.uint8)
    body[sub == _ACGT[first[cols]][:, None]] = 0
    body[(sub == _ACGT[second[cols]][:, None]) & (count[cols] == 2)[:, None]] = 3
    codes[:, :n] = body
    codes = codes.reshape(len(cols), -1, 4)
    return (codes[:, :, 0] | (codes[:, :, 1] << 2) | (codes[:, :, 2] << 4) | (codes[:, :, 3] << 6)).astype(np.uint8)


def nj_newick_from_alignment_u8(aln, sample_ids, min_overlap=1, max_taxa=2000, threads=0, nj_approx="exact", top_hits_k=64):
    """`nj_newick_from_alignment_u8`, tree.rs:7285-7874, exact mode: arguments checked with the reference's messages before any
    device work; the approximate and BIONJ modes are valid names that this build refuses (RuntimeError); biallelic alignments
    only.  `threads` is accepted and unused."""
    a = np.asarray(aln)
    if a.ndim != 2:
        raise ValueError("alignment must be a 2D uint8 matrix: (n_samples, n_sites)")
    n, n_sites = int(a.shape[0]), int(a.shape[1])
    if n < 2:
        raise ValueError("need at least 2 samples to build a tree")
    if n_sites == 0:
        raise ValueError("alignment has zero sites")
    names = _check_names(sample_ids, n)
    if int(max_taxa) == 0:
        raise ValueError("max_taxa must be > 0")
    if n > int(max_taxa):
        raise ValueError(f"n_samples={n} exceeds max_taxa={int(max_taxa)}; NJ in phase-1 is O(N^3)")
    mode = str(nj_approx).lower()
    if mode not in _NJ_MODES_EXACT and mode not in _NJ_MODES_UNBUILT:
        raise ValueError(f"invalid nj_approx='{nj_approx}' (expected 'exact', 'bionj', 'bionj-dist', 'bionj-jc', 'bionj-binom', "
                         "'bionj-auto', 'top-hits', 'rapidnj', 'lt-lazyq', or 'rapid-core')")
    if _NJ_MODES_UNBUILT.get(mode) == "top-hits" and int(top_hits_k) == 0:
        raise ValueError("top_hits_k must be > 0 when nj_approx='top-hits'")
    if mode in _NJ_MODES_UNBUILT:
        raise RuntimeError(f"nj_approx='{_NJ_MODES_UNBUILT[mode]}' is not built on this build: exact neighbour joining only")
    packed = alignment_to_packed(a.astype(np.uint8, copy=False))
    if packed.shape[0] == 0:                                                       # no known base anywhere: every distance is 1.0
        dist = np.ones((n, n), dtype=np.float64)
        np.fill_diagonal(dist, 0.0)
    else:
        valid, mism = tree_pair_counts_packed(packed, n, None)
        dist = tree_jc69_distance(valid, mism, min_overlap)
    return newick_from_merge_log(names, *_nj_run_device(dist, "alignment"), "alignment")


# ------------------------------------------------------------------------------------------------
# files and the BED route
# ------------------------------------------------------------------------------------------------

def sanitize_phylip_names(names):
    """`_sanitize_phylip_names`, python/janusx/script/tree.py:124-139."""
    used, out = set(), []
    for raw in names:
        base = re.sub(r"\s+", "_", str(raw).strip()).replace("'", "_") or "sample"
        name, idx = base, 2
        while name in used:
            name = f"{base}_{idx}"
            idx += 1
        used.add(name)
        out.append(name)
    return out


def write_fasta(path, sample_ids, aln):
    """`_write_fasta`, tree.py:142-149: `>id`, then 80 columns per line."""
    with open(path, "w", encoding="utf-8") as fh:
        for sid, row in zip(sample_ids, aln):
            fh.write(f">{sid}\n")
            text = bytes(row).decode("ascii")
            fh.writelines(text[i:i + 80] + "\n" for i in range(0, len(text), 80))


def write_phylip(path, sample_ids, aln):
    """`_write_phylip`, tree.py:152-161."""
    names = sanitize_phylip_names(sample_ids)
    width = max((len(x) for x in names), default=0)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(f"{len(names)} {aln.shape[1] if len(names) else 0}\n")
        for name, row in zip(names, aln):
            fh.write(f"{name}{' ' * (width + 2 - len(name))}{bytes(row).decode('ascii')}\n")


def tree_from_bed(prefix, maf=0.02, geno=0.05, het=0.02, snps_only=False, out=None, write_phylip_file=False, write_fasta_file=True,
                  min_overlap=1, max_taxa=None):
    """`jx tree -bfile PREFIX -nj` (python/janusx/script/tree.py:376-440 + its NJ call): the sites the chunk loader keeps
    (`stats.chunk_loader_row_keep`), their letters, the pair counts and the NJ loop on the device -> dict(newick (with `;`),
    sample_ids, n_sites, outputs).  With `out`, `{out}.nwk` (Newick + newline), `{out}.fasta` unless `write_fasta_file` is off,
    and `{out}.phy` with `write_phylip_file`; without, nothing is written.  The alignment (n x n_sites bytes) is only built when a
    file needs it."""
    from . import stats as st
    from .bed import read_bed_payload, read_fam_ids, snps_only_mask
    from .janusx import _bed_prefix, bed_row_counts
    prefix = _bed_prefix(prefix)
    packed, n, bim = read_bed_payload(prefix)
    ids = read_fam_ids(prefix)
    if n < 2:
        raise ValueError(f"Need at least 2 samples for tree inference, got {n}.")
    max_taxa = max(2, n) if max_taxa is None else int(max_taxa)          # the command passes max(2, n): tree.py:697
    if max_taxa == 0:
        raise ValueError("max_taxa must be > 0")
    if n > max_taxa:
        raise ValueError(f"n_samples={n} exceeds max_taxa={max_taxa}; NJ in phase-1 is O(N^3)")
    m_total = int(packed.shape[0])
    keep = np.zeros(m_total, dtype=bool)
    flip = np.zeros(m_total, dtype=bool)
    if m_total:
        keep, flip = st.chunk_loader_row_keep(bed_row_counts(packed, n, None), n, maf, geno, het)
        if snps_only:
            keep &= snps_only_mask(bim)
    rows = np.nonzero(keep)[0]
    if rows.shape[0] == 0:
        raise ValueError("No variant sites passed filters; cannot build alignment/tree.")
    pk = np.ascontiguousarray(packed[rows])
    l00, l10, l11 = packed_site_letters([bim.a0[r] for r in rows], [bim.a1[r] for r in rows], flip[rows])
    newick = nj_newick_from_packed(pk, n, ids, same_base=(l00 == l11), min_overlap=min_overlap, max_taxa=max_taxa)
    outputs = []
    if out is not None:
        with open(f"{out}.nwk", "w", encoding="utf-8") as fh:
            fh.write(newick + "\n")
        outputs.append(f"{out}.nwk")
        if write_fasta_file or write_phylip_file:
            aln = packed_to_alignment_u8(pk, n, l00, l10, l11)
            if write_fasta_file:
                write_fasta(f"{out}.fasta", ids, aln)
                outputs.append(f"{out}.fasta")
            if write_phylip_file:
                write_phylip(f"{out}.phy", ids, aln)
                outputs.append(f"{out}.phy")
    return {"newick": newick, "sample_ids": ids, "n_sites": int(rows.shape[0]), "outputs": outputs}
