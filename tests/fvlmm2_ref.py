"""f64 numpy restatement of the joint SNP-pair test of `jx fvlmm2` and of its literal, combo and af rules, written from the
reference's text (src/stats/fvlmm2.rs:37-290; python/janusx/script/fvlmm2.py:306-385, 719-725; src/math/linalg.rs:2-4,
314-335; src/stats/reml.rs:46-66).  Sample by sample and row by row, no device, nothing shared with the package."""
import math

import numpy as np

MIN_POSITIVE = 2.2250738585072014e-308


def normal_sf(z):
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def cholesky_inplace(a, dim):
    """Lower factor in place; False when a pivot is <= 1e-18."""
    for i in range(dim):
        for j in range(i + 1):
            acc = a[i, j]
            for k in range(j):
                acc -= a[i, k] * a[j, k]
            if i == j:
                if acc <= 1e-18:
                    return False
                a[i, j] = math.sqrt(acc) if acc == acc else float("nan")
            else:
                a[i, j] = acc / a[j, j]
        a[i, i + 1:] = 0.0
    return True


def cholesky_solve(l, dim, b):
    y = np.zeros(dim)
    for i in range(dim):
        acc = b[i]
        for k in range(i):
            acc -= l[i, k] * y[k]
        y[i] = acc / l[i, i]
    x = np.zeros(dim)
    for i in range(dim - 1, -1, -1):
        acc = y[i]
        for k in range(i + 1, dim):
            acc -= l[k, i] * x[k]
        x[i] = acc / l[i, i]
    return x


def joint_rows(s, xcov, y, log10_lbd, g1, g2, gc):
    """-> (rows, 9) f64: (beta, se, p) of g1, g2, gc in y ~ xcov + g1 + g2 + gc, weights 1 / (s + lambda), ridge 1e-6."""
    s = np.asarray(s, dtype=np.float64)
    xcov = np.asarray(xcov, dtype=np.float64).reshape(len(s), -1)
    y = np.asarray(y, dtype=np.float64)
    n, p = xcov.shape
    dim = p + 3
    lbd = 10.0 ** float(log10_lbd)
    vinv = 1.0 / (s + lbd)
    rows = g1.shape[0]
    out = np.full((rows, 9), np.nan)
    for r in range(rows):
        z = np.concatenate([xcov, np.stack([g1[r], g2[r], gc[r]], axis=1).astype(np.float64)], axis=1)
        if not np.all(np.isfinite(z[:, p:])):
            continue
        a = (z.T * vinv) @ z
        b = (z.T * vinv) @ y
        a[np.arange(dim), np.arange(dim)] += 1e-6
        if not cholesky_inplace(a, dim):
            continue
        beta = cholesky_solve(a, dim, b)
        res = y - z @ beta
        rr = float(np.sum(vinv * res * res))
        df = float(n - dim)
        if not (math.isfinite(rr) and rr > 0.0 and df > 0.0):
            continue
        sigma2 = rr / df
        if not (math.isfinite(sigma2) and sigma2 > 0.0):
            continue
        for t, ci in enumerate((p, p + 1, p + 2)):
            e = np.zeros(dim)
            e[ci] = 1.0
            var = sigma2 * cholesky_solve(a, dim, e)[ci]
            if not (math.isfinite(var) and var > 0.0):
                break                      # the earlier coefficients stay written
            se = math.sqrt(var)
            zz = beta[ci] / se
            pv = min(max(2.0 * normal_sf(abs(zz)), MIN_POSITIVE), 1.0) if math.isfinite(zz) else float("nan")
            out[r, 3 * t:3 * t + 3] = (beta[ci], se, pv)
    return out


def decode_rows(packed, n_samples, rows, flip, maf, sample_idx=None):
    """Rows of a PLINK 2-bit payload as f32: 0 / 1 / 2 copies of the counted allele (flipped rows 2 - g), missing = 2 maf."""
    packed = np.asarray(packed, dtype=np.uint8)
    codes = ((packed[np.asarray(rows)][:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(len(rows), -1)
    codes = codes[:, :n_samples]
    if sample_idx is not None:
        codes = codes[:, np.asarray(sample_idx)]
    out = np.empty(codes.shape, dtype=np.float32)
    for k, r in enumerate(rows):
        f = bool(flip[r])
        lut = np.array([2.0 if f else 0.0, np.float32(2.0) * np.float32(maf[r]), 1.0, 0.0 if f else 2.0], dtype=np.float32)
        out[k] = lut[codes[k]]
    return out


def literalize(g, neg):
    """rint(clip(g, 0, 2)), half to even; 2 - hit where the row is negated."""
    hit = np.rint(np.clip(np.asarray(g, dtype=np.float32), 0.0, 2.0)).astype(np.float32)
    neg = np.asarray(neg, dtype=bool).reshape(-1, 1)
    return np.where(neg, np.float32(2.0) - hit, hit).astype(np.float32)


def xor_dual(a, b):
    out = np.empty(a.shape, dtype=np.float32)
    for idx in np.ndindex(a.shape):
        x, w = float(a[idx]), float(b[idx])
        if x == w:
            out[idx] = 1.0 if x == 1.0 else 0.0
        else:
            out[idx] = 1.0 if (x == 1.0 or w == 1.0) else 2.0
    return out


def combo_rows(g1, g2, ops, neg1, neg2):
    """-> (combo f32 (R, n), af1, af2, combo_af f64 (R)) of decoded rows g1, g2."""
    l1, l2 = literalize(g1, neg1), literalize(g2, neg2)
    out = np.empty(g1.shape, dtype=np.float32)
    for i, op in enumerate(ops):
        if op == "*":
            assert not (neg1[i] or neg2[i])
            out[i] = (g1[i] * g2[i]).astype(np.float32)
        elif op == "&":
            out[i] = np.minimum(l1[i], l2[i])
        elif op == "|":
            out[i] = np.maximum(l1[i], l2[i])
        elif op == "^":
            out[i] = xor_dual(l1[i], l2[i])
        else:
            raise ValueError(op)
    return out, np.mean(l1 > 0.0, axis=1), np.mean(l2 > 0.0, axis=1), np.mean(out > 0.0, axis=1)


def errors(got, ref):
    """The project's norms on a (rows, 9) table against the restatement: beta against max(|beta|, se), se relative, p in the norm
    |dp| / p / max(1, z^2) -> (beta_err, se_err, p_err) maxima over all rows and the three terms.  The NaN patterns must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    be = se_e = pe = 0.0
    for t in range(3):
        b, s, p = (ref[:, 3 * t + k] for k in range(3))
        ok = ~np.isnan(b)
        if not ok.any():
            continue
        gb, gs, gp = (got[ok, 3 * t + k] for k in range(3))
        b, s, p = b[ok], s[ok], p[ok]
        z2 = (b / s) ** 2
        be = max(be, float(np.max(np.abs(gb - b) / np.maximum(np.abs(b), s))))
        se_e = max(se_e, float(np.max(np.abs(gs - s) / s)))
        pe = max(pe, float(np.max(np.abs(gp - p) / p / np.maximum(1.0, z2))))
    return be, se_e, pe


def bh(p, n_tests=None):
    """Benjamini-Hochberg of the finite non-negative entries, one hypothesis at a time; NaN elsewhere."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    idx = [i for i in range(len(p)) if math.isfinite(p[i]) and p[i] >= 0.0]
    m = max(len(idx), int(n_tests)) if n_tests is not None else len(idx)
    idx.sort(key=lambda i: min(p[i], 1.0))          # stable: ties keep their order
    best = 1.0
    for rank in range(len(idx), 0, -1):
        i = idx[rank - 1]
        pi = min(p[i], 1.0)
        best = min(best, pi * (float(m) / rank))
        out[i] = min(max(best, pi), 1.0)
    return out


def sci4(v):
    if not math.isfinite(v):
        return "NA"
    mant, exp = ("%.4e" % v).split("e")
    mant = mant.rstrip("0").rstrip(".")
    if mant in ("", "-0", "+0"):
        mant = "0"
    return "%se%d" % (mant, int(exp))


def fixed4(v):
    return "%.4f" % v if math.isfinite(v) else "NA"


HEADER = "chrom\tpos\tcombo_id\tcombo_af\tunit_name\tbeta_combo_joint\tse_combo_joint\tp_combo_joint\tp_combo_joint_fdr\tp_lit1_joint\tp_lit2_joint"


def render_rows(chrom, pos, combo_id, combo_af, joint, fdr):
    return ["\t".join([str(chrom[r]), str(int(round(float(pos[r])))), str(combo_id[r]), fixed4(combo_af[r]), ".", fixed4(joint[r, 6]),
                       fixed4(joint[r, 7]), sci4(joint[r, 8]), sci4(fdr[r]), sci4(joint[r, 2]), sci4(joint[r, 5])])
            for r in range(joint.shape[0])]
