"""Restatement in f64 numpy of the shared-projection route of the reference's trait-level LM scan
(`lm_trait_assoc_bed_to_tsv_shared_fast`, src/stats/lm_trait.rs:481-686): one two-pass modified Gram-Schmidt basis of the design
(`LmQrProjection::from_design`, src/stats/glm.rs:243-355), G Q and G R, and the per-(SNP, trait) rule of
`lm_assoc_from_shared_projection` (:303-335) followed by `sanitize_assoc_pvalue` (src/math/linalg.rs:99-108).  Everything is f64;
gy is the residualised sum g'r.  A helper of tests/test_lm_traits_host.py and tests/test_gpu_lm_traits.py."""
import math

import numpy as np

MIN_POSITIVE = 2.2250738585072014e-308


def mgs_basis(x):
    """Two-pass modified Gram-Schmidt: an all-zero column is dropped, and so is a column whose orthogonalised squared norm is
    <= 1e-12 max(col_norm^2, 1).  -> Q (n, rank)."""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    for c in range(x.shape[1]):
        v = x[:, c].copy()
        col2 = float(v @ v)
        if col2 <= 0.0:
            continue
        for _ in range(2):
            for qv in cols:
                v = v - float(v @ qv) * qv
        n2 = float(v @ v)
        if not math.isfinite(n2) or n2 <= 1e-12 * max(col2, 1.0):
            continue
        cols.append(v / math.sqrt(n2))
    return np.stack(cols, axis=1) if cols else np.zeros((x.shape[0], 0))


def decode_rows(g, af, flip):
    """(m, n) dosages (negative = missing) -> mean-imputed additive values in f64: [0, mean, 1, 2] or [2, mean, 1, 0] where flip,
    mean = clip(2 af, 0, 2) in f32."""
    g = np.asarray(g)
    mean = np.clip(np.float32(2.0) * np.asarray(af, dtype=np.float32), np.float32(0.0), np.float32(2.0)).astype(np.float64)
    fl = np.asarray(flip, dtype=bool)[:, None]
    v = np.where(fl, 2.0 - g, g).astype(np.float64)
    return np.where(g < 0, mean[:, None], v)


def student_t_two_sided(t, df):
    """Two-sided Student t tail, clamped to [f64::MIN_POSITIVE, 1] (src/stats/glm.rs:458-481); vectorised through scipy."""
    from scipy import stats as sst
    p = 2.0 * sst.t.sf(np.abs(t), df)
    p = np.where(np.isfinite(p), p, 1.0)
    p = np.where(np.isinf(t), MIN_POSITIVE, p)
    return np.clip(p, MIN_POSITIVE, 1.0)


def lm_traits_restatement(v, x, y_trait_major):
    """v (m, n) decoded rows, x (n, q0) design with intercept, y_trait_major (T, n) -> ((T, m, 4) beta, se, chisq, p; rank)."""
    v = np.asarray(v, dtype=np.float64)
    y = np.asarray(y_trait_major, dtype=np.float64)
    n = v.shape[1]
    q = mgs_basis(x)
    rank = q.shape[1]
    df = n - rank - 1
    r = y - (q @ (q.T @ y.T)).T
    rss0 = np.einsum("tn,tn->t", r, r)
    qg = v @ q                                              # (m, rank)
    gg = np.einsum("mn,mn->m", v, v) - np.einsum("mk,mk->m", qg, qg)
    gy = v @ r.T                                            # (m, T)
    out = np.full((y.shape[0], v.shape[0], 4), np.nan)
    out[:, :, 3] = 1.0
    ok_row = np.isfinite(gg) & (gg > 1e-8) & (df > 0)
    with np.errstate(all="ignore"):
        beta = gy / gg[:, None]
        rss1 = np.maximum(rss0[None, :] - gy * beta, 0.0)
        ve = rss1 / df
        se = np.sqrt(ve / gg[:, None])
        ok = ok_row[:, None] & np.isfinite(beta) & np.isfinite(ve) & (ve > 0.0) & np.isfinite(se) & (se > 0.0)
        t = beta / se
        chisq = n * np.log(1.0 + t * t / df)
        p = student_t_two_sided(np.where(ok, t, 0.0), max(df, 1))
    for k, a in enumerate((beta, se, chisq, p)):
        out[:, :, k] = np.where(ok, a, out[:, :, k].T).T
    return out, rank
