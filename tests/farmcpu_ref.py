"""Plain numpy f64 restatement of the reference's raw FarmCPU route (`farmcpu_packed_to_tsv(..., raw=True)`,
src/stats/farmcpu.rs), written from the source and literal to it: the raw design X with ixx = pinv(X'X) by SVD (:1909-1936), the
fixed-effect scan with one p per (marker, QTN slot) and a running minimum (:2629-2941), the lead selection (:832-868), the legacy
profile-likelihood scorer through the SVD of the lead genotypes with one pseudo-inverse per grid point (:1277-1490), the merge
(:870-934, :1538-1594, :4966-5020), the controller (:4737-5240) and the final scan (:3384-3403, :3613-3724).  The Rust was not
run; nothing here calls janusx_amd."""
import math

import numpy as np

MIN_POSITIVE = 2.2250738585072014e-308


# ---- p-values (src/stats/glm.rs:383-481), over arrays --------------------------------------------------------------------------

def _betacf(a, b, x):
    """a, b scalars; x array."""
    eps, fpmin = 3.0e-14, 1.0e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = np.where(np.abs(d) < fpmin, fpmin, d)
    d = 1.0 / d
    h = d.copy()
    live = np.ones(x.shape, dtype=bool)
    for m in range(1, 201):
        fm, m2 = float(m), 2.0 * m
        for aa in (fm * (b - fm) * x / ((qam + m2) * (a + m2)), -(a + fm) * (qab + fm) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = np.where(np.abs(d) < fpmin, fpmin, d)
            c = 1.0 + aa / c
            c = np.where(np.abs(c) < fpmin, fpmin, c)
            d = 1.0 / d
            delta = d * c
            h = np.where(live, h * delta, h)
        live &= ~(np.abs(delta - 1.0) < eps)
        if not live.any():
            break
    return h


def student_t_two_sided(t, df):
    """Two-sided Student t p of an array of t at one df; NaN t -> NaN, infinite t -> the smallest positive double."""
    t = np.asarray(t, dtype=np.float64)
    out = np.full(t.shape, np.nan)
    if df <= 0:
        return out
    v = float(df)
    a, b = 0.5 * v, 0.5
    ln_beta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    fin = np.isfinite(t)
    out[np.isinf(t)] = MIN_POSITIVE
    x = v / (v + t[fin] * t[fin])
    p = np.empty_like(x)
    lo = x < (a + 1.0) / (a + b + 2.0)
    with np.errstate(all="ignore"):
        xs = x[lo]
        p[lo] = np.exp(a * np.log(xs) + b * np.log(1.0 - xs) - ln_beta) / a * _betacf(a, b, xs)
        xs = x[~lo]
        p[~lo] = 1.0 - np.exp(b * np.log(1.0 - xs) + a * np.log(xs) - ln_beta) / b * _betacf(b, a, 1.0 - xs)
    p[x == 0.0] = 0.0
    p[x == 1.0] = 1.0
    p[~np.isfinite(p)] = 1.0
    out[fin] = np.minimum(np.maximum(p, MIN_POSITIVE), 1.0)
    return out


def sanitize_p(beta, se, p):
    """`sanitize_assoc_pvalue` (src/math/linalg.rs:99-108)."""
    ok = np.isfinite(beta) & np.isfinite(se) & (se > 0.0)
    return np.where(ok & np.isfinite(p), np.clip(np.where(np.isfinite(p), p, 1.0), MIN_POSITIVE, 1.0), 1.0)


# ---- decode (:760-830) ---------------------------------------------------------------------------------------------------------

def decode(g, af, flip):
    """g (m, n) int8 dosages of A1 copies... as stored (0, 1, 2, negative = missing) -> f64 (m, n): a missing call is 2 when
    2 af > 1 and 0 otherwise, a called value of a flipped row is 2 - g, the missing value is not flipped."""
    g = np.asarray(g)
    miss = np.where(2.0 * np.asarray(af, dtype=np.float32).astype(np.float64) > 1.0, 2.0, 0.0)[:, None]
    called = np.where(np.asarray(flip, dtype=bool)[:, None], 2.0 - g, g.astype(np.float64))
    return np.where(g < 0, miss, called)


# ---- design and scans ----------------------------------------------------------------------------------------------------------

def pinv_xtx(xtx):
    u, s, vt = np.linalg.svd(np.asarray(xtx, dtype=np.float64))
    cutoff = 1e-12 * max(float(s.max()), 1.0)
    s_inv = np.array([1.0 / v if (math.isfinite(v) and v > cutoff) else 0.0 for v in s])
    return vt.T @ np.diag(s_inv) @ u.T


def fem_scan(gd, x, q_base, y):
    """`scan_packed_full_matrix_reduced` on decoded rows gd (m, n) -> (beta, se, p (m), qtn_min_p (k_qtn), void (m) bool)."""
    n, q0 = x.shape
    m = gd.shape[0]
    k_qtn = q0 - q_base
    ixx = pinv_xtx(x.T @ x)
    xy = x.T @ y
    yy = float(y @ y)
    bg_df = n - q0
    bg_beta = ixx @ xy
    bg_rhs = float(bg_beta @ xy)
    df = bg_df - 1
    xs = gd @ x
    b21 = xs @ ixx
    ss = (gd * gd).sum(axis=1)
    sy = gd @ y
    b22 = ss - (b21 * xs).sum(axis=1)
    beta = np.full(m, np.nan)
    se = np.full(m, np.nan)
    p = np.ones(m)
    qmin = np.ones(k_qtn)
    live = (df > 0) & np.isfinite(b22) & (b22 > 1e-8)
    with np.errstate(all="ignore"):
        sy_adj = sy - xs @ bg_beta
        bm = sy_adj / b22
        ve = (yy - (bg_rhs + sy_adj * bm)) / df
        live &= np.isfinite(bm) & np.isfinite(ve) & ~(ve < 0.0)
        sm = np.sqrt(ve / b22)
        okp = live & np.isfinite(sm) & (sm > 0.0)
        praw = np.ones(m)
        praw[okp] = student_t_two_sided(bm[okp] / sm[okp], df)
        p[live] = sanitize_p(bm[live], sm[live], praw[live])
        beta[live], se[live] = bm[live], sm[live]
        for slot in range(k_qtn):
            bq = bg_beta[q_base + slot] - b21[:, q_base + slot] * bm
            sq = np.sqrt((ixx[q_base + slot, q_base + slot] + b21[:, q_base + slot] ** 2 / b22) * ve)
            ok = live & np.isfinite(bq) & np.isfinite(sq) & (sq > 0.0)
            if ok.any():
                pq = student_t_two_sided(bq[ok] / sq[ok], df)
                for v in pq:                                       # the running minimum
                    if math.isfinite(v) and v < qmin[slot]:
                        qmin[slot] = v
    return beta, se, p, qmin, ~live


def fix_zero_pvalues(p):
    ok = [v for v in p if math.isfinite(v) and v > 0.0]
    if not ok:
        return p
    repl = min(max(min(ok) * 0.01, MIN_POSITIVE), 1.0)
    for i in range(len(p)):
        if math.isfinite(p[i]) and p[i] <= 0.0:
            p[i] = repl
    return p


def prior_from_model(gd, x, q_base, y, qtn):
    _b, _s, p, qmin, _v = fem_scan(gd, x, q_base, y)
    p = p.copy()
    for j, idx in enumerate(qtn):
        if math.isfinite(qmin[j]):
            p[idx] = qmin[j]
    return fix_zero_pvalues(p)


def final_scan(gd, x, q_base, y, qtn):
    """The final table's (beta, se, p) per marker: markers by the final-scan rule (void -> NaN, NaN, 1), QTN rows from the
    background fit."""
    n, q0 = x.shape
    m = gd.shape[0]
    ixx = pinv_xtx(x.T @ x)
    xy = x.T @ y
    bg_df = n - q0
    bg_beta = ixx @ xy
    bg_rss = max(float(y @ y) - float(bg_beta @ xy), 0.0)
    bg_ve = bg_rss / bg_df
    y_res = y - x @ bg_beta
    df = bg_df - 1
    xs = gd @ x
    b21 = xs @ ixx
    b22 = (gd * gd).sum(axis=1) - (b21 * xs).sum(axis=1)
    sy = gd @ y_res
    out = np.full((m, 3), np.nan)
    with np.errstate(all="ignore"):
        live = (df > 0) & np.isfinite(b22) & (b22 > 1e-8)
        beta = sy / b22
        rss = np.maximum(bg_rss - sy * sy / b22, 0.0)
        se = np.sqrt(rss / df / b22)
        live &= np.isfinite(beta) & np.isfinite(se) & (se > 0.0)
        out[live, 0], out[live, 1] = beta[live], se[live]
        out[live, 2] = student_t_two_sided(beta[live] / se[live], df)
    out[~np.isfinite(out[:, 2]), 2] = 1.0
    for j, idx in enumerate(qtn):
        c = q_base + j
        b = float(bg_beta[c])
        with np.errstate(all="ignore"):
            s = float(np.sqrt(ixx[c, c] * bg_ve))
        pw = float(student_t_two_sided(np.array([b / s]), bg_df)[0]) if (math.isfinite(s) and s > 0.0 and math.isfinite(b)) \
            else math.nan
        out[idx] = (b, s, float(sanitize_p(np.array(b), np.array(s), np.array(pw))))
    return out


# ---- lead selection, scorer, merge -----------------------------------------------------------------------------------------------

def global_positions(chrom, pos):
    rank = {c: i for i, c in enumerate(sorted(set(str(c) for c in chrom)))}
    return np.array([int(p) + 1_000_000_000_000 * rank[str(c)] for c, p in zip(chrom, pos)], dtype=np.int64)


def grids(n, nbin=5, qtn_bound=None):
    qb = qtn_bound if qtn_bound is not None else max(int(math.floor(math.sqrt(n / math.log10(n)))), 1)
    step = max(qb // max(nbin, 1), 1)
    return qb, list(range(step, qb + 1, step)) or [qb]


def select_lead_indices(sz, n_lead, p, pos):
    m = len(p)
    if m == 0 or n_lead == 0:
        return []
    order = sorted(range(m), key=lambda i: (int(pos[i]) // sz, float(p[i])))      # sorted() is stable, like sort_by
    lead, last = [], None
    for i in order:
        b = int(pos[i]) // sz
        if last is None or b != last:
            lead.append(i)
            last = b
    lead.sort(key=lambda i: float(p[i]))
    return sorted(lead[:n_lead])


def ll_score(y, x, s, start=-5.0, end=5.0, step=0.1, svd_eps=1e-8, rcond=1e-12):
    n, p = x.shape
    k = s.shape[1]
    if n <= 1:
        start = end = 100.0
    else:
        for c in range(k):
            z = s[:, c] - s[:, c].sum() / n
            if (z * z).sum() / (n - 1) == 0.0:
                start = end = 100.0
                break
    u, sv, _ = np.linalg.svd(s, full_matrices=False)
    keep = [i for i, v in enumerate(sv) if v > svd_eps]
    r = len(keep)
    d = np.array([sv[i] * sv[i] for i in keep])
    u1 = u[:, keep]
    u1tx, u1ty = u1.T @ x, u1.T @ y
    y_res, x_res = y - u1 @ u1ty, x - u1 @ u1tx
    xrx, xry = x_res.T @ x_res, x_res.T @ y_res
    best = -math.inf
    e = start
    while e <= end + 1e-12:
        delta = math.exp(e)
        if math.isfinite(delta) and delta > 0.0:
            w = 1.0 / (d + delta)
            part12 = float(np.log(d + delta).sum())
            beta1 = (u1tx.T * w) @ u1tx
            beta3 = (u1tx.T * w) @ u1ty
            if math.isfinite(part12):
                mat = beta1 + xrx / delta
                rhs = beta3 + xry / delta
                uu, ss, vt = np.linalg.svd(mat)
                cut = rcond * max(float(ss.max()), 1.0)
                s_inv = np.array([1.0 / v if (math.isfinite(v) and v > cut) else 0.0 for v in ss])
                beta = (vt.T @ np.diag(s_inv) @ uu.T) @ rhs
                part1 = -0.5 * (n * math.log(2.0 * math.pi) + part12 + (n - r) * math.log(delta))
                ru = u1ty - u1tx @ beta
                part221 = float((ru * ru * w).sum())
                ri = y_res - x_res @ beta
                part222 = float(ri @ ri) / delta
                sigma = (part221 + part222) / n
                if math.isfinite(sigma) and sigma > 0.0:
                    ll = part1 - 0.5 * (n + n * math.log(sigma))
                    if ll > best:
                        best = ll
        e += step
    if not math.isfinite(best):
        return math.inf
    return -2.0 * best


def prepare_seq_qtn(saved, lead, femp, gpos, thr, keep_saved):
    union = []
    for i in list(lead) + list(saved):
        if i not in union:
            union.append(i)
    kept = []
    for i in union:
        if keep_saved and i in saved:
            kept.append(i)
        elif not (math.isfinite(thr) and thr > 0.0):
            kept.append(i)
        elif math.isfinite(femp[i]) and femp[i] < thr:
            kept.append(i)
    kept.sort(key=lambda i: (float(femp[i]), i))
    out, seen = [], set()
    for i in kept:
        if int(gpos[i]) not in seen:
            seen.add(int(gpos[i]))
            out.append(i)
    return out


def super_keep(s, thr=0.7):
    n, k = s.shape
    keep = [True] * k
    z = s - s.sum(axis=0) / n
    sd = np.sqrt((z * z).sum(axis=0) / (n - 1))
    for j in range(k):
        for i in range(j):
            den = (n - 1) * sd[i] * sd[j]
            if den > 0.0 and math.isfinite(den):
                c = float(z[:, i] @ z[:, j]) / den
                if math.isfinite(c) and abs(c) > thr:
                    keep[j] = False
                    break
    return keep


def overlap(a, b):
    u = len(set(a) | set(b))
    return 0.0 if u == 0 else len(set(a) & set(b)) / u


# ---- controller ------------------------------------------------------------------------------------------------------------------

def run_raw(gd, y, x_base, chrom, pos, threshold, max_iter=30, nbin=5, szbin=(500_000, 5_000_000, 50_000_000), qtn_bound=None):
    """gd (m, n): decoded markers.  -> dict(stats (m, 3), qtn, trace): trace[i] as `janusx_amd.farmcpu.run_raw` records it, plus
    the counts the fixture conditions are stated on."""
    m, n = gd.shape
    q_base = x_base.shape[1]
    gpos = global_positions(chrom, pos)
    thr = max(threshold, 0.01)
    _qb, nbins = grids(n, nbin, qtn_bound)

    def design(q):
        return np.hstack([x_base, gd[q].T]) if q else x_base

    qtn, prev, prior, x, trace = [], None, None, x_base, []
    for it in range(max(max_iter, 1)):
        if prior is None:
            prior = prior_from_model(gd, x, q_base, y, qtn)
            trace.append({"qtn": list(qtn)})
            if it + 1 >= max_iter:
                break
            prev = list(qtn)
            continue
        combos = []
        for sz in szbin:
            for nn in nbins:
                lead = select_lead_indices(int(sz), nn, prior, gpos)
                combos.append((int(sz), nn, ll_score(y, x, gd[lead].T) if lead else math.inf, lead))
        best = 0
        for i in range(1, len(combos)):
            if combos[i][2] < combos[best][2]:
                best = i
        lead = combos[best][3]
        finite = [v for v in prior if math.isfinite(v)]
        loop2_null = it + 1 == 2 and (min(finite) if finite else math.inf) > thr
        union = [] if loop2_null else prepare_seq_qtn(qtn, lead, prior, gpos, thr, bool(qtn))
        keep = super_keep(gd[union].T) if union else []
        nxt = sorted(set(i for i, k in zip(union, keep) if k))
        raw_union = []
        for i in list(lead) + list(qtn):
            if i not in raw_union:
                raw_union.append(i)
        passed = [i for i in raw_union if (bool(qtn) and i in qtn) or (math.isfinite(prior[i]) and prior[i] < thr)]
        trace.append({"qtn": list(qtn), "combo": (combos[best][0], combos[best][1]), "scores": [c[2] for c in combos],
                      "lead": list(lead), "union": list(union), "qtn_next": list(nxt), "loop2_null": loop2_null,
                      "lead_failed_threshold": [i for i in lead if not (math.isfinite(prior[i]) and prior[i] < thr)],
                      "dropped_by_position": 0 if loop2_null else len(passed) - len(union),
                      "dropped_by_super": len(union) - len(nxt), "prior": prior.copy(), "gpos": gpos})
        if loop2_null:
            break
        done = it + 1 >= max_iter or overlap(nxt, qtn) >= 1.0 or (prev is not None and overlap(nxt, prev) >= 1.0)
        if nxt != qtn:
            x = design(nxt)
            prior = prior_from_model(gd, x, q_base, y, nxt)
        if done:
            qtn = nxt
            break
        prev, qtn = list(qtn), nxt
    return {"stats": final_scan(gd, x, q_base, y, qtn), "qtn": list(qtn), "trace": trace, "x": x}


# ---- rendering (:3687-3724) ------------------------------------------------------------------------------------------------------

def _e4(v):
    if v != v:
        return "NaN"
    mant, ex = f"{v:.4e}".split("e")
    return f"{mant}e{int(ex)}"


def _f4(v):
    return "NaN" if v != v else f"{v:.4f}"


def render_row(chrom, pos, snp, a0, a1, af, miss, beta, se, p, source_row=None):
    ok = math.isfinite(beta) and math.isfinite(se) and se > 0.0
    chisq = (beta / se) ** 2 if ok else math.nan
    row = f"{chrom}\t{pos}\t{snp}\t{a0}\t{a1}\t{_f4(float(np.float32(af)))}\t{int(miss)}\t{_f4(beta)}\t{_f4(se)}\t{_e4(chisq)}\t{_e4(p)}"
    return row + (f"\t{int(source_row)}\n" if source_row is not None else "\n")


HEADER = "chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald"


def render_tables(stats, qtn, chrom, pos, snp, a0, a1, af, miss, source_rows):
    main = HEADER + "\n" + "".join(render_row(chrom[i], pos[i], snp[i], a0[i], a1[i], af[i], miss[i], *stats[i])
                                   for i in range(len(stats)))
    q = HEADER + "\tsource_row\n" + "".join(render_row(chrom[i], pos[i], snp[i], a0[i], a1[i], af[i], miss[i], *stats[i],
                                                      source_row=source_rows[i]) for i in sorted(qtn))
    return main, q


# ---- the whole-procedure fixture -------------------------------------------------------------------------------------------------

FIXTURE_SEED = 3


def _genotype_from_latent(z, freq):
    """Two thresholds on a standard-normal latent: P(g >= 1) and P(g = 2) of a Hardy-Weinberg site of allele frequency freq."""
    q = np.sort(z)
    n = len(z)
    t1 = q[min(int(round(n * (1.0 - freq) ** 2)), n - 1)]
    t2 = q[min(int(round(n * (1.0 - freq * freq))), n - 1)]
    return (z >= t1).astype(np.int8) + (z >= t2).astype(np.int8)


def make_fixture(seed=FIXTURE_SEED, n=400, m=3000):
    """n samples x m markers on the chromosomes "1", "10", "2" (name order differs from numeric order), positions over 120 Mb per
    chromosome (240 / 24 / 3 bins of the three default sizes), 2 % missing calls, and a phenotype with planted effects:
      * five plain causal markers;
      * a masked pair: b and d are correlated and carry opposite effects, so that b is weak until d is in the model, and a marker a
        AT THE POSITION OF b (a second record of a multi-allelic site), correlated with b and not with d, that beats b marginally:
        a enters first, b replaces it later and a leaves by the position rule;
      * a near copy of a causal marker in another bin: both are leads, the SUPER rule drops the later one.
    -> dict(g (m, n) int8 with -9 = missing, flip, af (f32, of the stored allele before the flip is applied), chrom, pos, y, x_base)."""
    rng = np.random.default_rng(seed)
    per = m // 3
    chrom = np.repeat(np.array(["1", "10", "2"]), per)
    pos = np.concatenate([np.sort(rng.choice(np.arange(1, 120_000_000), size=per, replace=False)) for _ in range(3)]).astype(np.int64)
    # a sparse last 50 Mb bin on chromosome "10": its best of five markers is a lead that fails the threshold
    pos[per:2 * per] = np.sort(np.concatenate([rng.choice(np.arange(1, 100_000_000), size=per - 5, replace=False),
                                               rng.choice(np.arange(100_000_000, 120_000_000), size=5, replace=False)]))
    freq = rng.uniform(0.1, 0.5, size=m)
    g = rng.binomial(2, freq[:, None], size=(m, n)).astype(np.int8)
    causal = [150, 700, 1300, 1900, 2600]
    ib, ia, idd, ic, icopy = 2200, 2201, 420, causal[1], 2850
    zb = rng.standard_normal(n)
    zd = 0.75 * zb + math.sqrt(1.0 - 0.75 ** 2) * rng.standard_normal(n)
    za = (zb - 0.75 * zd) / math.sqrt(1.0 - 0.75 ** 2) * 0.85 + math.sqrt(1.0 - 0.85 ** 2) * rng.standard_normal(n)
    g[ib], g[idd], g[ia] = _genotype_from_latent(zb, 0.4), _genotype_from_latent(zd, 0.4), _genotype_from_latent(za, 0.4)
    pos[ia] = pos[ib]
    copy = g[ic].copy()
    swap = rng.random(n) < 0.08
    copy[swap] = rng.binomial(2, freq[ic], size=int(swap.sum()))
    g[icopy] = copy
    full = g.astype(np.float64)
    eff = np.zeros(m)
    eff[causal] = [0.9, -0.8, 0.85, -0.9, 0.8]
    eff[ib], eff[idd] = 1.6, -2.08
    cov = rng.standard_normal((n, 2))
    y = full.T @ eff + cov @ np.array([0.5, -0.3]) + rng.standard_normal(n) * 1.6
    g[rng.random(g.shape) < 0.02] = -9
    called = (g >= 0).sum(axis=1)
    af = (np.where(g < 0, 0, g).sum(axis=1) / np.maximum(2 * called, 1)).astype(np.float32)
    flip = af > np.float32(0.5)
    x_base = np.hstack([np.ones((n, 1)), cov])
    return {"g": g, "flip": flip, "af": np.where(flip, np.float32(1.0) - af, af).astype(np.float32), "raw_af": af, "chrom": chrom,
            "pos": pos, "y": y, "x_base": x_base, "special": {"a": ia, "b": ib, "d": idd, "c": ic, "copy": icopy}}


def fixture_decoded(fx):
    """The decoded markers of a fixture, as the scans see them."""
    return decode(fx["g"], fx["af"], fx["flip"])
