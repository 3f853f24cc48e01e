"""Host half of the SNP-by-covariate interaction scan `jx gwas -lm2` (src/stats/glm2.rs; the device half is csrc/k_lm2.hip).

Per trait: the orthonormal basis Q of the design X (`LmQrProjection::from_design`, src/stats/glm.rs:243-355), r_y = y - QQ'y,
rss0, and the two weight matrices whose columns the moment kernel sums v and v^2 against.  Per flagged SNP: the algebra of
`lm2_fit_single_snp` (glm2.rs:238-325) in f64 with `matrix_inverse_or_pinv` (glm2.rs:27-56), from the device sums.
"""
from __future__ import annotations

import math

import numpy as np

from .tsv import MIN_POSITIVE

LM2_MAX_INTERACTIONS = 8


def qr_basis(x: np.ndarray):
    """Twice-reorthogonalised modified Gram-Schmidt basis of the columns of x (n, q_base) (`LmQrProjection::from_design`,
    src/stats/glm.rs:243-355): a column of zero norm, or whose residual norm^2 is <= 1e-12 max(|col|^2, 1), is dropped.
    -> Q (n, q_rank)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, q0 = x.shape
    if n == 0:
        raise RuntimeError("empty LM design")
    if q0 == 0:
        raise RuntimeError("X has zero columns")
    if not np.all(np.isfinite(x)):
        raise RuntimeError("LM design contains non-finite values")
    cols = []
    for c in range(q0):
        v = x[:, c].copy()
        norm2_col = float(v @ v)
        if norm2_col <= 0.0:
            continue
        for _pass in range(2):
            for qv in cols:
                coeff = float(v @ qv)
                if coeff != 0.0:
                    v -= coeff * qv
        norm2 = float(v @ v)
        if norm2 <= 1e-12 * max(norm2_col, 1.0) or not math.isfinite(norm2):
            continue
        cols.append(v * (1.0 / math.sqrt(norm2)))
    rank = len(cols)
    if n <= rank + 1:
        raise RuntimeError(f"n too small: require n > rank(X)+1, got n={n}, rank={rank}")
    return np.ascontiguousarray(np.stack(cols, axis=1)) if rank else np.zeros((n, 0))


def qr_projection(x: np.ndarray, y: np.ndarray):
    """Twice-reorthogonalised modified Gram-Schmidt basis of the columns of x (n, q_base): a column of zero norm, or whose
    residual norm^2 is <= 1e-12 max(|col|^2, 1), is dropped.  -> (Q (n, q_rank), r_y (n), rss0)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    n = x.shape[0]
    if y.shape[0] != n:
        raise RuntimeError("y length mismatch")
    q = qr_basis(x)
    r_y = y - q @ (q.T @ y)
    if not np.all(np.isfinite(r_y)):
        raise RuntimeError("LM QR residualization produced non-finite values")
    rss0 = float(r_y @ r_y)
    if not math.isfinite(rss0):
        raise RuntimeError("LM QR residual RSS is not finite")
    return q, r_y, rss0


def weight_columns(q: np.ndarray, r_y: np.ndarray, cov_sel: np.ndarray):
    """The SNP-independent columns of the moments: with c_0 = 1 and c_j = cov_sel[:, j - 1],
    wv[:, a (q_rank + 1) + t] = c_a Q_t (t < q_rank), c_a r_y (t = q_rank) -- summed against v --, and
    ws[:, a (a + 1) / 2 + b] = c_a c_b (b <= a) -- summed against v^2."""
    n, qr = q.shape
    k = int(cov_sel.shape[1])
    c = np.concatenate([np.ones((n, 1)), np.asarray(cov_sel, dtype=np.float64)], axis=1)
    base = np.concatenate([q, r_y[:, None]], axis=1)
    wv = (c[:, :, None] * base[:, None, :]).reshape(n, (k + 1) * (qr + 1))
    ws = np.stack([c[:, a] * c[:, b] for a in range(k + 1) for b in range(a + 1)], axis=1)
    return np.ascontiguousarray(wv), np.ascontiguousarray(ws)


def weight_image(wv: np.ndarray, ws: np.ndarray):
    """(tiles, nblk, 32, 64) f64 operand image of `jxg_lm2_scan_p32` (include/jxgpu.h): each group of columns padded with zero
    columns to whole blocks of 16, the samples padded with zero rows to whole tiles of 128; element [tile][b][ks][lane] = column
    16 b + (lane & 15) at sample 128 tile + 4 ks + (lane >> 4).  -> (image, nblk, nblk_v)."""
    n = wv.shape[0]
    nbv, nbs = (wv.shape[1] + 15) // 16, (ws.shape[1] + 15) // 16
    nblk, nt = nbv + nbs, (n + 127) // 128
    full = np.zeros((nt * 128, nblk * 16), dtype=np.float64)
    full[:n, :wv.shape[1]] = wv
    full[:n, nbv * 16:nbv * 16 + ws.shape[1]] = ws
    # sample = 128 tile + 4 ks + fk, column = 16 b + fi, lane = 16 fk + fi
    img = full.reshape(nt, 32, 4, nblk, 16).transpose(0, 3, 1, 2, 4)
    return np.ascontiguousarray(img).reshape(nt, nblk, 32, 64), nblk, nbv


# ---- p-values (src/math/linalg.rs:20-108, src/stats/glm.rs:383-481) -------------------------------------------------------

def _gamma_q(a: float, x: float) -> float:
    if not (math.isfinite(a) and math.isfinite(x)) or a <= 0.0:
        return math.nan
    if x <= 0.0:
        return 1.0
    itmax, eps, fpmin = 200, 3e-14, 1e-300
    gln = math.lgamma(a)
    if x < a + 1.0:
        ap, delta = a, 1.0 / a
        total = delta
        for _ in range(itmax):
            ap += 1.0
            delta *= x / ap
            total += delta
            if abs(delta) <= abs(total) * eps:
                break
        return min(max(1.0 - total * math.exp(-x + a * math.log(x) - gln), 0.0), 1.0)
    b = x + 1.0 - a
    c = 1.0 / fpmin
    d = 1.0 / max(b, fpmin)
    h = d
    for i in range(1, itmax + 1):
        an = -float(i) * (float(i) - a)
        b += 2.0
        d = an * d + b
        if abs(d) < fpmin:
            d = fpmin
        c = b + an / c
        if abs(c) < fpmin:
            c = fpmin
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) <= eps:
            break
    return min(max(math.exp(-x + a * math.log(x) - gln) * h, 0.0), 1.0)


def chi2_sf(stat: float, df: float) -> float:
    """`chi2_sf` (src/math/linalg.rs:80-96): regularised incomplete gamma, the erfc form at df = 1, clamped to [MIN_POSITIVE, 1]."""
    if not math.isfinite(stat) or stat <= 0.0 or not (math.isfinite(df) and df > 0.0):
        return 1.0
    p = math.erfc(math.sqrt(0.5 * stat)) if abs(df - 1.0) <= 2.220446049250313e-16 else _gamma_q(0.5 * df, 0.5 * stat)
    return min(max(p, MIN_POSITIVE), 1.0) if math.isfinite(p) else 1.0


def _betacf(a: float, b: float, x: float) -> float:
    eps, fpmin = 3.0e-14, 1.0e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    if abs(d) < fpmin:
        d = fpmin
    d = 1.0 / d
    h = d
    for m in range(1, 201):
        fm, m2 = float(m), 2.0 * m
        for aa in (fm * (b - fm) * x / ((qam + m2) * (a + m2)), -(a + fm) * (qab + fm) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            if abs(d) < fpmin:
                d = fpmin
            c = 1.0 + aa / c
            if abs(c) < fpmin:
                c = fpmin
            d = 1.0 / d
            delta = d * c
            h *= delta
        if abs(delta - 1.0) < eps:
            break
    return h


def student_t_two_sided(t: float, df: int) -> float:
    """`student_t_p_two_sided` (src/stats/glm.rs:383-481), the statement csrc/lm_pvalue.h evaluates on the device."""
    if df <= 0:
        return math.nan
    if not math.isfinite(t):
        return math.nan if t != t else MIN_POSITIVE
    v = float(df)
    a, b, x = 0.5 * v, 0.5, v / (v + t * t)
    ln_beta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    if x == 0.0:
        p = 0.0
    elif x == 1.0:
        p = 1.0
    elif x < (a + 1.0) / (a + b + 2.0):
        p = math.exp(a * math.log(x) + b * math.log(1.0 - x) - ln_beta) / a * _betacf(a, b, x)
    else:
        p = 1.0 - math.exp(b * math.log(1.0 - x) + a * math.log(x) - ln_beta) / b * _betacf(b, a, 1.0 - x)
    if not math.isfinite(p):
        p = 1.0
    return min(max(p, MIN_POSITIVE), 1.0)


def inverse_or_pinv(a: np.ndarray) -> np.ndarray:
    """`matrix_inverse_or_pinv` (glm2.rs:27-56): the plain inverse unless elimination meets an exactly zero (or non-finite)
    pivot, then the SVD pseudo-inverse with the cut-off 1e-12 max(s_max, 1), here without rounding noise in exactly zero rows."""
    a = np.asarray(a, dtype=np.float64)
    # an index whose row and column are exactly zero (an all-zero SNP, an all-zero interaction column) carries a zero singular
    # value and nothing else: its row and column of the pseudo-inverse are exactly zero, the rest is that of the other indices
    live = [i for i in range(a.shape[0]) if np.any(a[i, :] != 0.0) or np.any(a[:, i] != 0.0)]
    if len(live) < a.shape[0]:
        out = np.zeros_like(a)
        if live:
            out[np.ix_(live, live)] = inverse_or_pinv(a[np.ix_(live, live)])
        return out
    try:
        inv = np.linalg.inv(a)
        if np.all(np.isfinite(inv)):
            return inv
    except np.linalg.LinAlgError:
        pass
    u, s, vt = np.linalg.svd(a)
    cutoff = 1e-12 * max(float(s.max()) if s.size else 0.0, 1.0)
    s_inv = np.array([1.0 / v if (math.isfinite(v) and v > cutoff) else 0.0 for v in s])
    return (vt.T * s_inv) @ u.T


def solve_from_moments(e: np.ndarray, c: np.ndarray, d: np.ndarray, rss0: float, df: int) -> np.ndarray:
    """One SNP of `lm2_fit_single_snp` (glm2.rs:238-325) from its moments e (m), c (q_rank, m), d (m, m) ->
    (beta, se, chisq, pwald) per coefficient, then chisq_int_joint, p_int_joint, chisq_joint, p_joint."""
    m = int(e.shape[0])
    k = m - 1
    out = np.empty(4 * m + 4, dtype=np.float64)
    s_inv = inverse_or_pinv(d - c.T @ c)
    beta = s_inv @ e
    eb = float(e @ beta)
    sigma2 = max(rss0 - eb, 0.0) / float(df)
    for a in range(m):
        b, var = float(beta[a]), sigma2 * float(s_inv[a, a])
        se = math.sqrt(var) if (math.isfinite(var) and var > 0.0) else math.nan
        chisq, pw = math.nan, 1.0
        if math.isfinite(b) and math.isfinite(se) and se > 0.0:
            t = b / se
            chisq = t * t
            pw = student_t_two_sided(t, df)
            pw = min(max(pw, MIN_POSITIVE), 1.0) if math.isfinite(pw) else 1.0
        out[4 * a:4 * a + 4] = (b, se, chisq, pw)
    s2ok = math.isfinite(sigma2) and sigma2 > 0.0
    ci, pi, cj, pj = math.nan, 1.0, math.nan, 1.0
    if k > 0 and s2ok:
        b_int = beta[1:]
        ci = max(float(b_int @ inverse_or_pinv(s_inv[1:, 1:]) @ b_int) / sigma2, 0.0)
        pi = chi2_sf(ci, float(k))
    if s2ok:
        cj = max(eb / sigma2, 0.0)
        pj = chi2_sf(cj, float(m))
    out[4 * m:] = (ci, pi, cj, pj)
    return out


def solve_from_sums(sums: np.ndarray, q_rank: int, k: int, sq0: int, rss0: float, df: int) -> np.ndarray:
    """`solve_from_moments` on one row of the device sums (column layout of `weight_columns`, v^2 group from column sq0)."""
    m = 1 + k
    u = np.asarray(sums, dtype=np.float64)
    cv = u[:m * (q_rank + 1)].reshape(m, q_rank + 1)
    d = np.empty((m, m), dtype=np.float64)
    for a in range(m):
        for b in range(a + 1):
            d[a, b] = d[b, a] = u[sq0 + a * (a + 1) // 2 + b]
    return solve_from_moments(cv[:, q_rank].copy(), np.ascontiguousarray(cv[:, :q_rank].T), d, rss0, df)


def row_filter(counts: np.ndarray, n: int, maf_threshold: float, max_missing_rate: float):
    """Row filter of the LM / LM2 streaming routes when no prepared metadata is given (glm2.rs:634-717), on counts (m, 3) =
    (missing, het, hom_alt) over the n selected samples: a row is dropped when missing / n > max_missing_rate, when it has no
    call at all, or when min(alt_freq, 1 - alt_freq) < maf_threshold, all in f32.  -> (keep, alt_freq f32, missing count)."""
    f32 = np.float32
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    missing, het, hom = counts[:, 0], counts[:, 1], counts[:, 2]
    nm = np.maximum(n - missing, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        miss_rate = (missing.astype(f32) / f32(n)) if n > 0 else np.ones(len(missing), dtype=f32)
        alt_freq = (het + 2 * hom).astype(f32) / (f32(2.0) * nm.astype(f32))
        maf = np.minimum(alt_freq, f32(1.0) - alt_freq)
    keep = ~(miss_rate > f32(max_missing_rate)) & (nm > 0)
    keep &= ~(maf < f32(maf_threshold))
    return keep, np.where(nm > 0, alt_freq, f32(0.0)).astype(f32), missing
