"""Host half of `jx gwas -farmcpu`: the raw FarmCPU route of the reference (`farmcpu_packed_to_tsv(..., raw=True)`,
src/stats/farmcpu.rs:4153-5510; the `Raw` branch :4737-5240 and the final scan :5306-5493).  The device half is
`pipeline.scan_rows_farmcpu_fem` / `scan_rows_farmcpu_final` (csrc/k_farmcpu.hip over the int8 product of csrc/k_lm_traits.hip).

Per iteration: a fixed-effect scan of every marker against the design [1 | covariates | pseudo-QTN columns] (device), the choice
of a lead set among bin size x lead count combinations by the legacy profile likelihood (`ll_score`: the lead genotypes are
decoded on the device, their SVD and the p-sized algebra run here in f64), and the merge of leads and saved QTNs (threshold,
position de-duplication, the SUPER correlation rule).  Not built: the unified route (`raw=False`), `skip_main_scan`, the local
window merge (off on the raw route) and the reference's JX_FARMCPU_* environment switches -- their defaults are what runs.
"""
from __future__ import annotations

import math
import os
import time
from collections import namedtuple

import numpy as np

from . import lm2
from .tsv import MIN_POSITIVE, fmt_e4, fmt_f4, resolve_snp_name

CHROM_BLOCK = 1_000_000_000_000
DEFAULT_SZBIN = (500_000, 5_000_000, 50_000_000)
SUPER_R = 0.7
DesignOperands = namedtuple("DesignOperands", "q r_y bg_rss w bg_beta ixx df xy")
FarmcpuResult = namedtuple("FarmcpuResult", "stats qtn trace miss stage1_secs stage2_secs")


# ---- grids and positions (farmcpu.rs:4319-4375) -------------------------------------------------------------------------------

def global_positions(chrom, pos) -> np.ndarray:
    """pos + 10^12 (rank of the chromosome NAME in sorted order)."""
    names = [str(c) for c in chrom]
    block = {c: i for i, c in enumerate(sorted(set(names)))}
    return np.asarray(pos, dtype=np.int64) + CHROM_BLOCK * np.array([block[c] for c in names], dtype=np.int64)


def qtn_bound_auto(n: int) -> int:
    if n <= 2:
        return 1
    den = math.log10(float(n))
    if not math.isfinite(den) or den <= 0.0:
        return 1
    return max(int(math.floor(math.sqrt(float(n) / den))), 1)


def nbin_values(qb: int, nbin: int):
    qb = max(int(qb), 1)
    step = max(qb // max(int(nbin), 1), 1)
    vals = list(range(step, qb + 1, step))
    return vals if vals else [qb]


def szbin_values(szbin):
    vals = [max(int(round(float(v))), 1) for v in (szbin or ()) if math.isfinite(float(v)) and float(v) > 0.0]
    return vals if vals else list(DEFAULT_SZBIN)


# ---- lead selection and merge -------------------------------------------------------------------------------------------------

def select_lead_indices(sz: int, n_lead: int, pvalue: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """`select_lead_indices` (:832-868): the best marker of every bin `pos div sz` (ties: the lower index), of those the
    `n_lead` best (ties: the lower bin), sorted by index."""
    p = np.asarray(pvalue, dtype=np.float64)
    if p.size == 0 or n_lead <= 0:
        return np.zeros(0, dtype=np.int64)
    bins = np.floor_divide(np.asarray(pos, dtype=np.int64), int(sz))
    order = np.lexsort((p, bins))                              # stable: by bin, then p, then index
    first = np.ones(order.size, dtype=bool)
    first[1:] = bins[order[1:]] != bins[order[:-1]]
    lead = order[first]
    lead = lead[np.argsort(p[lead], kind="stable")][:int(n_lead)]
    return np.sort(lead).astype(np.int64)


def prepare_seq_qtn(qtn_saved, opt_lead, femp, global_pos, threshold: float, keep_saved: bool):
    """`farmcpu_raw_prepare_seq_qtn` (:870-934): leads then saved QTNs without repeats; a marker stays when it is a saved QTN
    (`keep_saved`) or its p is finite and below the threshold; sorted by (p, index); one marker per global position."""
    union, seen = [], set()
    for idx in list(opt_lead) + list(qtn_saved):
        idx = int(idx)
        if idx not in seen:
            seen.add(idx)
            union.append(idx)
    saved = set(int(i) for i in qtn_saved) if keep_saved else set()
    enabled = math.isfinite(threshold) and threshold > 0.0
    kept = [i for i in union if (keep_saved and i in saved) or not enabled
            or (math.isfinite(femp[i]) and femp[i] < threshold)]
    kept.sort(key=lambda i: (float(femp[i]), i))
    out, pos_seen = [], set()
    for i in kept:
        gp = int(global_pos[i])
        if gp not in pos_seen:
            pos_seen.add(gp)
            out.append(i)
    return out


def fix_zero_pvalues(p: np.ndarray) -> np.ndarray:
    """`farmcpu_fix_zero_pvalues` (:936-951), in place: p <= 0 becomes 0.01 of the smallest positive p."""
    ok = np.isfinite(p) & (p > 0.0)
    if ok.any():
        repl = min(max(float(p[ok].min()) * 0.01, MIN_POSITIVE), 1.0)
        p[np.isfinite(p) & (p <= 0.0)] = repl
    return p


def super_keep(sample_major: np.ndarray, thr: float = SUPER_R) -> np.ndarray:
    """`farmcpu_super_keep_from_sample_major` (:1538-1594): column j (n, k input, in order of prior p) is dropped when its |r|
    with ANY earlier column exceeds `thr` -- an earlier column that was dropped itself still counts."""
    s = np.asarray(sample_major, dtype=np.float64)
    n, k = s.shape
    keep = np.ones(k, dtype=bool)
    if k == 0 or n == 0:
        return keep
    z = s - s.mean(axis=0)
    sd = np.sqrt((z * z).sum(axis=0) / (n - 1)) if n > 1 else np.zeros(k)
    for j in range(k):
        for i in range(j):
            den = float(n - 1) * sd[i] * sd[j]
            if den > 0.0 and math.isfinite(den):
                r = float(z[:, i] @ z[:, j]) / den
                if math.isfinite(r) and abs(r) > thr:
                    keep[j] = False
                    break
    return keep


def overlap_ratio(a, b) -> float:
    sa, sb = set(int(i) for i in a), set(int(i) for i in b)
    union = len(sa | sb)
    return 0.0 if union == 0 else len(sa & sb) / union


# ---- design -------------------------------------------------------------------------------------------------------------------

def pinv_xtx(xtx: np.ndarray) -> np.ndarray:
    """`pinv_xtx_with_rank` (:1909-1936): V S^-1 U' of the SVD, singular values <= 1e-12 max(s_max, 1) dropped."""
    a = np.asarray(xtx, dtype=np.float64)
    if a.shape[0] == 0:
        return np.zeros((0, 0))
    u, s, vt = np.linalg.svd(a)
    cutoff = 1e-12 * max(float(s.max()), 1.0)
    s_inv = np.where(np.isfinite(s) & (s > cutoff), 1.0 / np.where(s > 0.0, s, 1.0), 0.0)
    return (vt.T * s_inv) @ u.T


def orthonormal_basis(x: np.ndarray) -> np.ndarray:
    """Orthonormal basis of the columns of x (n, q0) by the rule of `lm2.qr_basis` (a column of zero norm, or whose residual
    norm^2 is <= 1e-12 max(|col|^2, 1), is dropped) with the two orthogonalisation passes as matrix-vector products against the
    basis so far: the design grows to ~70 columns and is rebuilt every round, and the column-by-column form costs 10^4 vector
    operations there.  -> Q (n, rank)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, q0 = x.shape
    if n == 0 or q0 == 0:
        raise RuntimeError("empty LM design")
    if not np.all(np.isfinite(x)):
        raise RuntimeError("LM design contains non-finite values")
    q = np.empty((n, q0), dtype=np.float64, order="F")
    r = 0
    for c in range(q0):
        v = x[:, c].copy()
        norm2_col = float(v @ v)
        if norm2_col <= 0.0:
            continue
        for _pass in range(2):
            if r:
                v -= q[:, :r] @ (q[:, :r].T @ v)
        norm2 = float(v @ v)
        if norm2 <= 1e-12 * max(norm2_col, 1.0) or not math.isfinite(norm2):
            continue
        q[:, r] = v * (1.0 / math.sqrt(norm2))
        r += 1
    if n <= r + 1:
        raise RuntimeError(f"n too small: require n > rank(X)+1, got n={n}, rank={r}")
    return np.ascontiguousarray(q[:, :r])


def design_operands(x: np.ndarray, q_base: int, y: np.ndarray) -> DesignOperands:
    """What the device scans need of a design `x` (n, q0; QTN columns from `q_base` on): the orthonormal basis Q of its columns
    (`orthonormal_basis`), r_y = y - QQ'y and bg_rss = |r_y|^2, and from the reference's ixx = pinv(X'X): bg_beta = ixx X'y and
    W = (ixx X'Q)[q_base:] whose row j maps Q'g to b21[q_base + j] (X'g = X'Q Q'g: g - QQ'g is orthogonal to every column of X).
    df = n - q0 - 1, with q0 the column count as in the reference, also for a rank-deficient design."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    n, q0 = x.shape
    if y.shape[0] != n:
        raise RuntimeError(f"design rows {n} != len(y) {y.shape[0]}")
    if not 0 <= int(q_base) <= q0:
        raise RuntimeError(f"q_base exceeds background design width: q_base={q_base}, q0={q0}")
    if n <= q0 + 1:
        raise RuntimeError(f"n too small for LM core: n={n}, q={q0}")
    q = orthonormal_basis(x)
    r_y = y - q @ (q.T @ y)
    ixx = pinv_xtx(x.T @ x)
    xy = x.T @ y
    w = (ixx @ (x.T @ q))[int(q_base):]
    return DesignOperands(q, r_y, float(r_y @ r_y), np.ascontiguousarray(w), ixx @ xy, ixx, n - q0 - 1, xy)


# ---- the legacy REM scorer (:1277-1490) ---------------------------------------------------------------------------------------

def ll_score(y: np.ndarray, x: np.ndarray, s: np.ndarray, delta_start=-5.0, delta_end=5.0, delta_step=0.1, svd_eps=1e-8,
             pinv_rcond=1e-12) -> float:
    """-2 max over the grid delta = e^{start .. end} of the profile log-likelihood of y ~ X b + S u + e, u ~ N(0, sigma^2 I),
    e ~ N(0, delta sigma^2 I), through the SVD of the lead genotypes S (n, k): singular values <= `svd_eps` are dropped, the
    inner p x p system is solved by the SVD pseudo-inverse; a constant lead column collapses the grid to e^100."""
    y = np.asarray(y, dtype=np.float64).ravel()
    x = np.asarray(x, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    n, p = x.shape
    k = s.shape[1]
    if k == 0:
        raise RuntimeError("legacy FarmCPU ll scorer received zero candidate markers")
    if n <= 1 or np.any((((s - s.mean(axis=0)) ** 2).sum(axis=0) / (n - 1)) == 0.0):
        delta_start = delta_end = 100.0
    u, sv, _vt = np.linalg.svd(s, full_matrices=False)
    keep = sv > svd_eps
    u1, d = u[:, keep], sv[keep] ** 2
    r = int(d.size)
    u1tx, u1ty = u1.T @ x, u1.T @ y                              # (r, p), (r)
    y_res = y - u1 @ u1ty
    x_res = x - u1 @ u1tx
    xrx, xry = x_res.T @ x_res, x_res.T @ y_res
    exps = []
    e = delta_start
    while e <= delta_end + 1e-12:
        exps.append(e)
        e += delta_step
    delta = np.exp(np.array(exps))
    ok = np.isfinite(delta) & (delta > 0.0)
    delta = delta[ok]
    if delta.size == 0:
        raise RuntimeError("legacy FarmCPU ll scorer failed to find a finite optimum")
    wgt = 1.0 / (d[None, :] + delta[:, None])                   # (G, r)
    part12 = np.log(d[None, :] + delta[:, None]).sum(axis=1)
    beta1 = np.einsum("ra,gr,rb->gab", u1tx, wgt, u1tx)
    beta3 = np.einsum("ra,gr,r->ga", u1tx, wgt, u1ty)
    mat = beta1 + xrx[None] / delta[:, None, None]
    rhs = beta3 + xry[None] / delta[:, None]
    uu, ss, vv = np.linalg.svd(mat)
    cut = pinv_rcond * np.maximum(ss.max(axis=1), 1.0)
    s_inv = np.where(np.isfinite(ss) & (ss > cut[:, None]), 1.0 / np.where(ss > 0.0, ss, 1.0), 0.0)
    beta = np.einsum("gba,gb,gcb,gc->ga", vv, s_inv, uu, rhs)    # V S^-1 U' rhs
    part1 = -0.5 * (n * math.log(2.0 * math.pi) + part12 + (n - r) * np.log(delta))
    res_u = u1ty[None, :] - beta @ u1tx.T                       # (G, r)
    part221 = (res_u * res_u * wgt).sum(axis=1)
    res = y_res[:, None] - x_res @ beta.T                       # (n, G)
    part222 = (res * res).sum(axis=0) / delta
    sigma = (part221 + part222) / n
    good = np.isfinite(part12) & np.isfinite(sigma) & (sigma > 0.0)
    ll = np.where(good, part1 - 0.5 * (n + n * np.log(np.where(good, sigma, 1.0))), -np.inf)
    best = float(ll.max()) if ll.size else -math.inf
    if not math.isfinite(best):
        raise RuntimeError("legacy FarmCPU ll scorer failed to find a finite optimum")
    return -2.0 * best


def best_rem_lead_set(y, x_qtn, femp, global_pos, szbin, nbin_vals, decode):
    """`farmcpu_best_rem_lead_set` (:2311-2440): every (bin size, lead count), its lead set and score (inf where the scorer
    fails); the smallest score wins, the first on ties.  `decode(indices)` -> the (n, k) genotypes of markers.
    -> (best index, [(sz, nn, score, leads)])."""
    combos = []
    pool, cols = {}, {}
    for sz in szbin:
        for nn in nbin_vals:
            combos.append((int(sz), int(nn), select_lead_indices(sz, nn, femp, global_pos)))
    need = sorted({int(i) for _sz, _nn, lead in combos for i in lead})
    if need:
        dec = decode(np.array(need, dtype=np.int64))
        cols = {i: dec[:, j] for j, i in enumerate(need)}
    out = []
    for sz, nn, lead in combos:
        key = lead.tobytes()
        if key not in pool:
            try:
                pool[key] = ll_score(y, x_qtn, np.stack([cols[int(i)] for i in lead], axis=1)) if lead.size else math.inf
            except (RuntimeError, np.linalg.LinAlgError):
                pool[key] = math.inf
        out.append((sz, nn, pool[key], lead))
    best = 0
    for i in range(1, len(out)):
        if out[i][2] < out[best][2]:
            best = i
    return best, out


# ---- the raw controller (:4737-5240) and the final scan (:5306-5493) ----------------------------------------------------------

def decode_rows(panel, rows, af, flip) -> np.ndarray:
    """(n, k) f64 genotypes of panel rows, additive with major-allele imputation (`decode_packed_rows_to_sample_major`,
    :760-830), decoded on the device."""
    import torch

    from . import pipeline as pl
    from ._lib import check, lib
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    k = len(rows)
    if k == 0:
        return np.zeros((panel.n, 0))
    fl = np.asarray(flip, dtype=bool)
    lut = np.zeros((k, 4), dtype=np.float32)
    lut[:, 0], lut[:, 1], lut[:, 2], lut[:, 3] = np.where(fl, 2.0, 0.0), pl.farmcpu_missing_value(af), 1.0, np.where(fl, 0.0, 2.0)
    out = torch.empty((k, panel.n), dtype=torch.float32, device=panel.device)
    rows_t = torch.from_numpy(rows).to(panel.device)
    lut_t = torch.from_numpy(lut).to(panel.device)
    check(lib().jxg_decode_rows_p32(panel.p32.data_ptr(), panel.m, panel.n, rows_t.data_ptr(), k, lut_t.data_ptr(), out.data_ptr(),
                                    panel.n, pl._stream()))
    return np.ascontiguousarray(out.cpu().numpy().astype(np.float64).T)


def run_raw(panel, rows, af, flip, y, x_base, chrom, pos, threshold, max_iter=30, qtn_bound=None, nbin=5,
            szbin=DEFAULT_SZBIN, on_iter=None) -> FarmcpuResult:
    """The raw FarmCPU route over the markers `rows` of a resident panel (`af`, `flip` per marker): x_base (n, q_base) carries the
    intercept and the covariates.  -> FarmcpuResult(stats (m, 3) [beta, se, p] of the final scan with the QTN rows taken from
    the background fit and a void row as (NaN, NaN, 1); qtn: marker positions of the final QTNs; trace: per iteration a dict
    with `qtn` (the set scanned in it), and from the second on `combo` (sz, nn), `scores`, `lead`, `qtn_next`; miss: missing
    calls per marker)."""
    from . import pipeline as pl
    if not (math.isfinite(threshold) and threshold > 0.0):
        raise RuntimeError("threshold must be finite and > 0")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    af = np.ascontiguousarray(af, dtype=np.float32)
    flip = np.asarray(flip, dtype=bool)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    x_base = np.ascontiguousarray(x_base, dtype=np.float64)
    n, q_base, m = panel.n, int(x_base.shape[1]), len(rows)
    if m == 0:
        raise RuntimeError("empty packed marker matrix")
    t0 = time.perf_counter()
    gpos = global_positions(chrom, pos)
    thr_eff = max(float(threshold), 0.01)
    max_iter = max(int(max_iter), 1)
    qb = max(int(qtn_bound), 1) if qtn_bound is not None else qtn_bound_auto(n)
    nbins, szb = nbin_values(qb, nbin), szbin_values(szbin)
    cache = {}

    def decode(idx):
        new = [int(i) for i in idx if int(i) not in cache]
        if new:
            dec = decode_rows(panel, rows[new], af[new], flip[new])
            for j, i in enumerate(new):
                cache[i] = dec[:, j]
        return np.stack([cache[int(i)] for i in idx], axis=1) if len(idx) else np.zeros((n, 0))

    def design(qtn):
        return np.ascontiguousarray(np.hstack([x_base, decode(qtn)])) if len(qtn) else x_base

    def fem(x, qtn):
        res = pl.scan_rows_farmcpu_fem(panel, rows, af, flip, x, q_base, y)
        prior = res.p.cpu().numpy().copy()
        for j, idx in enumerate(qtn):
            if math.isfinite(res.qtn_min_p[j]):
                prior[idx] = res.qtn_min_p[j]
        return fix_zero_pvalues(prior)

    qtn, prev, prior, x, trace = [], None, None, x_base, []
    for it in range(max_iter):
        if on_iter is not None:
            on_iter(it + 1, max_iter)
        if prior is None:
            prior = fem(x, qtn)
            trace.append({"qtn": list(qtn)})
            if it + 1 >= max_iter:
                break
            prev = list(qtn)
            continue
        best, combos = best_rem_lead_set(y, x, prior, gpos, szb, nbins, decode)
        lead = [int(i) for i in combos[best][3]] if combos else []
        finite = prior[np.isfinite(prior)]
        loop2_null = it + 1 == 2 and (float(finite.min()) if finite.size else math.inf) > thr_eff
        union = [] if loop2_null else prepare_seq_qtn(qtn, lead, prior, gpos, thr_eff, bool(qtn))
        nxt = sorted(set(i for i, k in zip(union, super_keep(decode(union))) if k)) if union else []
        trace.append({"qtn": list(qtn), "combo": (combos[best][0], combos[best][1]) if combos else None,
                      "scores": [c[2] for c in combos], "lead": lead, "union": list(union), "qtn_next": list(nxt),
                      "loop2_null": loop2_null})
        if loop2_null:
            break
        done = it + 1 >= max_iter or overlap_ratio(nxt, qtn) >= 1.0 or (prev is not None and overlap_ratio(nxt, prev) >= 1.0)
        if nxt != qtn:
            x = design(nxt)
            if not done:
                prior = fem(x, nxt)
        if done:
            qtn = nxt
            break
        prev, qtn = list(qtn), nxt
    stage1 = time.perf_counter() - t0

    t1 = time.perf_counter()
    des = design_operands(x, q_base, y)
    q0 = int(x.shape[1])
    stats = pl.scan_rows_farmcpu_final(panel, rows, af, flip, x, q_base, y).cpu().numpy()
    stats[~np.isfinite(stats[:, 2]), 2] = 1.0
    bg_df = n - q0
    bg_ve = max(des.bg_rss, 0.0) / bg_df
    for j, idx in enumerate(qtn):
        c = q_base + j
        beta, var = float(des.bg_beta[c]), float(des.ixx[c, c]) * bg_ve
        se = math.sqrt(var) if var >= 0.0 else math.nan
        p = lm2.student_t_two_sided(beta / se, bg_df) if (math.isfinite(se) and se > 0.0 and math.isfinite(beta)) else math.nan
        valid = math.isfinite(beta) and math.isfinite(se) and se > 0.0
        stats[idx] = (beta, se, min(max(p, MIN_POSITIVE), 1.0) if (valid and math.isfinite(p)) else 1.0)
    miss = panel.counts()[rows, 0].astype(np.int64)
    return FarmcpuResult(stats, [int(i) for i in qtn], trace, miss, stage1, time.perf_counter() - t1)


# ---- writers (:3687-3724) -----------------------------------------------------------------------------------------------------

QTN_HEADER = "chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\tsource_row\n"


def write_main_tsv(path, chrom, pos, snp, a0, a1, af, miss_counts, stats) -> int:
    """The `.farmcpu.tsv` table: the 11 columns of the LM routes with `miss` as a count."""
    from .tsv import write_assoc_tsv_counts
    return write_assoc_tsv_counts(path, chrom, pos, snp, a0, a1, af, np.asarray(miss_counts, dtype=np.float32), stats)


def format_qtn_row(chrom, pos, snp, a0, a1, af, miss_count, beta, se, p, source_row) -> str:
    if math.isfinite(beta) and math.isfinite(se) and se > 0.0:
        z = beta / se
        chisq, pv = z * z, (min(max(p, MIN_POSITIVE), 1.0) if math.isfinite(p) else 1.0)
    else:
        chisq, pv = math.nan, 1.0
    return (f"{chrom}\t{pos}\t{resolve_snp_name(snp, chrom, pos)}\t{a0}\t{a1}\t{fmt_f4(float(np.float32(af)))}\t{int(miss_count)}\t"
            f"{fmt_f4(beta)}\t{fmt_f4(se)}\t{fmt_e4(chisq)}\t{fmt_e4(pv)}\t{int(source_row)}\n")


def write_qtn_tsv(path, qtn, chrom, pos, snp, a0, a1, af, miss_counts, stats, source_rows) -> int:
    """The `.farmcpu.qtn` table: the main table's rows of the QTNs (in marker order) plus `source_row`."""
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "w") as fh:
        fh.write(QTN_HEADER)
        for i in sorted(int(v) for v in qtn):
            fh.write(format_qtn_row(chrom[i], pos[i], snp[i], a0[i], a1[i], af[i], miss_counts[i], float(stats[i, 0]),
                                    float(stats[i, 1]), float(stats[i, 2]), source_rows[i]))
    os.replace(tmp, path)
    return len(qtn)
