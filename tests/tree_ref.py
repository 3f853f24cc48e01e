"""Restatement of the reference's `jx tree -nj` (src/stats/tree.rs, src/io/gfcore.rs:408-480, python/janusx/script/tree.py) in
plain numpy and Python floats, independent of the product code: the expected value of tests/test_tree_host.py and
tests/test_gpu_tree.py.

Every sum whose order matters is a sequential one: row sums are `np.cumsum(...)[..., -1]` (never `np.sum`, which adds pairwise),
scalars are Python floats (IEEE binary64, no fusing)."""
import math

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------- sites: process_snp_row_with_precomputed_counts_impl

def row_keep_scalar(missing, het, hom, n, maf_thr, miss_thr, het_thr):
    """One row of the chunk loader's filter -> (keep, flip)."""
    maf32, miss32, het32 = F32(maf_thr), F32(miss_thr), F32(het_thr)
    if n == 0:
        return False, False
    nm = n - missing
    missing_rate = F32(1.0 - (float(nm) / float(n)))
    if missing_rate > miss32:
        return False, False
    if nm == 0:
        return (not (maf32 > F32(0.0))), False
    if het32 < F32(1.0):                                       # BedChunkReader::new, gfreader.rs:3245
        if float(het) / float(nm) > float(het32):
            return False, False
    alt_freq = float(het + 2 * hom) / (2.0 * float(nm))
    flip = alt_freq > 0.5
    maf = F32(min(alt_freq, 1.0 - alt_freq))
    if maf < maf32:
        return False, flip
    return True, flip


# ---------------------------------------------------------------- letters

def ascii_upper(b):
    return b - 32 if 0x61 <= b <= 0x7A else b


def first_base_code(s):
    for b in s.encode("utf-8"):
        if b in (0x20, 0x09, 0x0A, 0x0C, 0x0D):
            continue
        u = ascii_upper(b)
        return u if u in b"ACGT" else ord("N")
    return ord("N")


def sanitize_base_pair(r, a):
    r, a = ascii_upper(r), ascii_upper(a)
    n = ord("N")
    if r not in b"ACGT":
        r = n
    if a not in b"ACGT":
        a = n
    if r == n and a == n:
        return ord("A"), ord("G")
    if r == n:
        return (ord("A"), a) if a != ord("A") else (ord("C"), a)
    if a == n:
        return (r, ord("G")) if r != ord("G") else (r, ord("T"))
    return r, a


def het_iupac(r, a):
    if r == a:
        return r
    return {frozenset(b"AC"): ord("M"), frozenset(b"AG"): ord("R"), frozenset(b"AT"): ord("W"), frozenset(b"CG"): ord("S"),
            frozenset(b"CT"): ord("Y"), frozenset(b"GT"): ord("K")}.get(frozenset((r, a)), ord("N"))


def convert_geno_to_alignment(g, rc, ac):
    """convert_geno_to_alignment_u8 on (m, n) f32 values and per-site bytes -> (n, m) uint8."""
    g = np.asarray(g, dtype=np.float32)
    m, n = g.shape
    out = np.full((n, m), ord("N"), dtype=np.uint8)
    for i in range(m):
        r, a = sanitize_base_pair(int(rc[i]), int(ac[i]))
        h = het_iupac(r, a)
        for j in range(n):
            x = g[i, j]
            if not np.isfinite(x) or x < 0.0:
                b = ord("N")
            elif x <= 0.5:
                b = r
            elif x >= 1.5:
                b = a
            else:
                b = h
            out[j, i] = b
    return out


def unpack_values(packed, n):
    """(m, n) f32 values of a payload: 00 -> 0, 10 -> 1, 11 -> 2, 01 -> -9 (gfcore.rs:1945-1948)."""
    pk = np.asarray(packed, dtype=np.uint8)
    codes = np.stack([(pk >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(pk.shape[0], -1)[:, :n]
    return np.array([0.0, -9.0, 1.0, 2.0], dtype=np.float32)[codes]


def bed_alignment(packed, n, a0, a1, flip):
    """The alignment the command builds from kept rows: a flipped row has its values turned round and its allele strings swapped
    (gfcore.rs:454-462), then `geno_chunk_to_alignment_u8_siteinfo`."""
    g = unpack_values(packed, n)
    rc, ac = [], []
    for i in range(g.shape[0]):
        ref, alt = a0[i], a1[i]
        if flip[i]:
            g[i] = np.where(g[i] >= 0.0, 2.0 - g[i], g[i])
            ref, alt = alt, ref
        rc.append(first_base_code(ref))
        ac.append(first_base_code(alt))
    return convert_geno_to_alignment(g, rc, ac)


# ---------------------------------------------------------------- distance: build_distance_matrix

def pair_counts(aln):
    """-> (valid, mismatch) int64 (n, n): A / C / G / T known, everything else unknown."""
    a = np.asarray(aln, dtype=np.uint8)
    a = np.where((a >= 0x61) & (a <= 0x7A), a - 32, a)
    planes = [(a == b).astype(np.int64) for b in b"ACGT"]
    known = sum(planes)
    valid = known @ known.T
    same = sum(p @ p.T for p in planes)
    return valid, valid - same


def jc69_denominator(p_mismatch):
    p = min(max(p_mismatch, 0.0), 0.75 - 1e-12)
    return max(1.0 - (4.0 * p / 3.0), 1e-12)


def distance_matrix(valid, mismatch, min_overlap=1):
    """JC69 of every pair i < j, mirrored.  The logarithm is numpy's, as in the product (README, "Known differences"), taken in one
    call over a contiguous array of the denominators; everything around it is scalar."""
    n = valid.shape[0]
    min_ov = max(int(min_overlap), 1)
    pairs, denoms = [], []
    d = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(i + 1, n):
            v = int(valid[i, j])
            if v >= min_ov and v > 0:
                p = min(max(float(int(mismatch[i, j])) / float(v), 0.0), 1.0)
                pairs.append((i, j))
                denoms.append(jc69_denominator(p))
            else:
                d[i, j] = d[j, i] = 1.0
    logs = np.log(np.array(denoms, dtype=np.float64)) if denoms else []
    for (i, j), lg in zip(pairs, logs):
        x = -0.75 * float(lg)
        if math.isfinite(x):
            x = x if x > 0.0 else 0.0              # canonical +0.0
        else:
            x = 1.0
        d[i, j] = d[j, i] = x
    return d


# ---------------------------------------------------------------- normalize_distance_matrix_from_ndarray

def normalize_distance_matrix(d):
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2:
        raise ValueError("distance matrix must be 2D")
    n = d.shape[0]
    if n < 2:
        raise ValueError("need at least 2 samples to build a tree")
    if d.shape[1] != n:
        raise ValueError(f"distance matrix must be square, got {n}x{d.shape[1]}")
    out = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        if not math.isfinite(d[i, i]):
            raise ValueError(f"distance matrix diagonal has NaN/Inf at ({i},{i})")
        for j in range(i + 1, n):
            a, b = float(d[i, j]), float(d[j, i])
            if math.isfinite(a) and math.isfinite(b):
                v = 0.5 * (a + b)
            elif math.isfinite(a):
                v = a
            elif math.isfinite(b):
                v = b
            else:
                raise ValueError(f"distance matrix has NaN/Inf in both directions at ({i}, {j}) and ({j}, {i})")
            if not math.isfinite(v):
                raise ValueError(f"distance matrix has invalid value after symmetrization at ({i}, {j})")
            if v < 0.0:
                v = 0.0
            out[i, j] = out[j, i] = v
    return out


# ---------------------------------------------------------------- NJ, exact mode

def nj(dist, route):
    """Exact NJ on a symmetric matrix.  route "alignment": nj_newick_from_alignment_u8 (:7502-7873, zeros canonical +0.0);
    "distance": nj_newick_from_distance_exact (:7062-7167, literal).  -> (log_ij (n - 1, 2) int, log_vals (n - 2, 3) f64, last f64,
    joins [(left, right, left_len, right_len)])."""
    n = dist.shape[0]
    total = 2 * n - 2
    d = np.zeros((total, total), dtype=np.float64)
    d[:n, :n] = dist
    active = list(range(n))
    log_ij, log_vals, joins = [], [], []
    with np.errstate(all="ignore"):
        while len(active) > 2:
            m = len(active)
            act = np.array(active)
            sub = d[np.ix_(act, act)]
            r = np.cumsum(sub, axis=1)[:, -1]                      # sequential, ascending node id; the diagonal adds +0.0
            q = (float(m) - 2.0) * sub - r[:, None] - r[None, :]   # row = the smaller id
            q = np.where(np.triu(np.ones((m, m), dtype=bool), 1) & ~np.isnan(q), q, np.inf)
            flat = int(np.argmin(q))                               # first least element in (i, j) order
            pi, pj = divmod(flat, m)
            if not q[pi, pj] < np.inf:
                pi, pj = 0, 1
            bi, bj = active[pi], active[pj]
            dij, ri, rj = float(d[bi, bj]), float(r[pi]), float(r[pj])
            if route == "alignment":
                if not math.isfinite((float(m) - 2.0) * dij - ri - rj):
                    raise ValueError("failed to build NJ tree: no valid pair found")
                delta = (ri - rj) / (float(m) - 2.0)
                li = 0.5 * (dij + delta)
                lj = dij - li
                li = li if math.isfinite(li) and li > 0.0 else 0.0
                lj = lj if math.isfinite(lj) and lj > 0.0 else 0.0
            else:
                denom = max(float(m) - 2.0, 1.0)
                li = 0.5 * dij + (ri - rj) / (2.0 * denom)
                lj = dij - li
                if not math.isfinite(li) or li < 0.0:
                    li = 0.0
                if not math.isfinite(lj) or lj < 0.0:
                    lj = 0.0
            u = n + len(joins)
            rest = np.array([k for k in active if k != bi and k != bj])
            duk = 0.5 * (d[bi, rest] + d[bj, rest] - dij)
            if route == "alignment":
                duk = np.where(np.isfinite(duk) & (duk > 0.0), duk, 0.0)
            else:
                duk = np.where(~np.isfinite(duk) | (duk < 0.0), 0.0, duk)
            d[u, rest] = duk
            d[rest, u] = duk
            log_ij.append((bi, bj))
            log_vals.append((dij, ri, rj))
            joins.append((bi, bj, li, lj))
            active = [k for k in active if k != bi and k != bj] + [u]
    a0, a1 = active
    last = float(d[a0, a1])
    dd = last
    if route == "alignment":
        dd = dd if math.isfinite(dd) and dd > 0.0 else 0.0
    elif not math.isfinite(dd) or dd < 0.0:
        dd = 0.0
    joins.append((a0, a1, 0.5 * dd, 0.5 * dd))
    log_ij.append((a0, a1))
    return (np.array(log_ij, dtype=np.int64).reshape(-1, 2), np.array(log_vals, dtype=np.float64).reshape(-1, 3), last, joins)


# ---------------------------------------------------------------- Newick

def quote_newick_name(name):
    safe = all((b < 128 and chr(b).isalnum()) or b in b"_.-" for b in name.encode("utf-8"))
    return name if safe else "'" + name.replace("'", "_") + "'"


def render_newick(names, joins):
    """Iterative render of the last join's node; lengths as `.10f`; trailing `;`."""
    n = len(names)
    text = {}
    for x in range(n):
        text[x] = quote_newick_name(names[x])
    # children always have smaller ids than their parent: one pass in id order builds every subtree's text from pieces
    pieces = {x: [text[x]] for x in range(n)}
    for t, (left, right, ll, rl) in enumerate(joins):
        pieces[n + t] = ["(", pieces.pop(left), ":", format(ll, ".10f"), ",", pieces.pop(right), ":", format(rl, ".10f"), ")"]
    out, stack = [], [pieces[n + len(joins) - 1]]
    while stack:
        x = stack.pop()
        if isinstance(x, str):
            out.append(x)
        else:
            stack.extend(reversed(x))
    return "".join(out) + ";"


def newick(dist, names, route):
    return render_newick(names, nj(dist, route)[3])


def fasta_text(ids, aln):
    out = []
    for sid, row in zip(ids, aln):
        out.append(f">{sid}\n")
        s = bytes(row).decode("ascii")
        out.extend(s[i:i + 80] + "\n" for i in range(0, len(s), 80))
    return "".join(out)
