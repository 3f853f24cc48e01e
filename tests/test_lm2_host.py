"""Host tests of `jx gwas -lm / -lm2` (plain LM and the SNP-by-covariate interaction scan), no GPU: a numpy restatement of the
reference's LM2 (src/stats/glm2.rs, src/stats/glm.rs:243-355, src/math/linalg.rs:20-108), the selector parser, the table, the
row filter and the refusals of the mirror functions that come before any device call.

The restatement below is the one `tests/test_gpu_lm2.py` compares the device results with.  No reference binary can pin it, so it
is pinned by reading (file:line in the docstrings) and guarded twice: against textbook OLS (`numpy.linalg.lstsq` on [X, g, g o c],
scipy's t and chi-square tails, the joint Wald statistics from the full covariance matrix), and against itself under reordering
of the sample sums (forwards -- the reference's order --, backwards, BLAS) on every panel of the GPU tests, where it moves by
less than 1e-10 while cond(S) stays below 1e6 -- which is what leaves the GPU tests' 1e-9 three decades of room."""
import math
import os

import numpy as np
import pytest

from janusx_amd import cli
from janusx_amd import janusx as jx
from janusx_amd import lm2, tsv
from oracle import jx_oracle as O

MIN_POSITIVE = 2.2250738585072014e-308

# name -> (n, m, q_base, k, missing rate): the panels of tests/test_gpu_lm2.py.  n straddles the 128-sample record; (q_base, k)
# = (1, 1), (3, 2), (5, 3), (12, 8) give 7, 18, 34 and 162 weight columns
PANELS = {
    "n127": (127, 70, 3, 2, 0.05), "n128": (128, 70, 3, 2, 0.0), "n129": (129, 70, 3, 2, 0.05), "n300": (300, 257, 3, 2, 0.05),
    "q1k1": (300, 70, 1, 1, 0.0), "q5k3": (300, 70, 5, 3, 0.05), "q12k8": (300, 70, 12, 8, 0.05),
}


def lm2_panel(name):
    """-> (g (m, n) int8 dosage with -9 = missing, x (n, q_base) with intercept, cov_all (n, k + 1), cov_indices, y): allele
    frequency 0.1 - 0.5, continuous covariates with means 0 .. 10, a phenotype with SNP, covariate and interaction effects."""
    n, m, q_base, k, missing = PANELS[name]
    rng = np.random.default_rng(20261018 + sum(map(ord, name)))
    p = rng.uniform(0.1, 0.5, size=m)
    g = rng.binomial(2, p[:, None], size=(m, n)).astype(np.int8)
    if missing > 0:
        g[rng.random((m, n)) < missing] = -9
    x = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, q_base - 1))], axis=1)
    cov_all = rng.normal(size=(n, k + 1)) + np.linspace(0.0, 10.0, k + 1)[None, :]
    cov_indices = [int(j) for j in rng.permutation(k + 1)[:k]]
    gc = np.where(g[0] < 0, 0, g[0]).astype(np.float64)
    y = x @ rng.normal(size=q_base) + 0.3 * gc + 0.1 * gc * cov_all[:, cov_indices[0]] + rng.normal(size=n)
    return g, x, cov_all, cov_indices, y


# ---- restatement -----------------------------------------------------------------------------------------------------------------

def _seq(a, axis=0):
    """Sum along `axis` one term after the other, like a Rust loop (numpy's own reductions add pairwise)."""
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def ref_qr(x, y):
    """`LmQrProjection::from_design` (src/stats/glm.rs:243-355): modified Gram-Schmidt with a second pass, a column dropped when
    its norm is zero or its residual norm^2 <= 1e-12 max(|col|^2, 1).  -> (Q (n, rank), r_y, rss0)."""
    n, q0 = x.shape
    cols = []
    for c in range(q0):
        v = x[:, c].astype(np.float64).copy()
        col_norm2 = float(_seq(v * v))
        if col_norm2 <= 0.0:
            continue
        for _ in range(2):
            for qv in cols:
                coeff = float(_seq(v * qv))
                if coeff != 0.0:
                    v = v - coeff * qv
        norm2 = float(_seq(v * v))
        if norm2 <= 1e-12 * max(col_norm2, 1.0) or not math.isfinite(norm2):
            continue
        cols.append(v * (1.0 / math.sqrt(norm2)))
    q = np.stack(cols, axis=1)
    qty = _seq(q * y[:, None])
    r_y = y - _seq(q * qty[None, :], axis=1)
    return q, r_y, float(_seq(r_y * r_y))


def ref_decode(g_row, af32, flip=False):
    """`decode_packed_row_model_into_f64` (src/decode/decode.rs:307-364), additive: a missing call takes max(2 af, 0) with the f32
    frequency widened to f64; the calls (not the missing value) are mirrored to 2 - v where the row is flipped."""
    v = g_row.astype(np.float64)
    if flip:
        v = 2.0 - v
    return np.where(g_row < 0, max(2.0 * float(np.float32(af32)), 0.0), v)


def ref_gamma_q(a, x):
    """src/math/linalg.rs:20-77: series below a + 1, Lentz continued fraction above; ITMAX 200, EPS 3e-14."""
    if not (math.isfinite(a) and math.isfinite(x)) or a <= 0.0:
        return math.nan
    if x <= 0.0:
        return 1.0
    if math.isinf(x):
        return 0.0
    gln = math.lgamma(a)
    if x < a + 1.0:
        ap, de = a, 1.0 / a
        s = de
        for _ in range(200):
            ap += 1.0
            de *= x / ap
            s += de
            if abs(de) <= abs(s) * 3e-14:
                break
        return min(max(1.0 - s * math.exp(-x + a * math.log(x) - gln), 0.0), 1.0)
    b, c = x + 1.0 - a, 1.0 / 1e-300
    d = 1.0 / max(b, 1e-300)
    h = d
    for i in range(1, 201):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = 1e-300 if abs(d) < 1e-300 else d
        c = b + an / c
        c = 1e-300 if abs(c) < 1e-300 else c
        d = 1.0 / d
        h *= d * c
        if abs(d * c - 1.0) <= 3e-14:
            break
    return min(max(math.exp(-x + a * math.log(x) - gln) * h, 0.0), 1.0)


def ref_chi2_sf(stat, df):
    """src/math/linalg.rs:80-96."""
    if not math.isfinite(stat) or stat <= 0.0 or not (math.isfinite(df) and df > 0.0):
        return 1.0
    p = math.erfc(math.sqrt(0.5 * stat)) if abs(df - 1.0) <= np.finfo(np.float64).eps else ref_gamma_q(0.5 * df, 0.5 * stat)
    return min(max(p, MIN_POSITIVE), 1.0) if math.isfinite(p) else 1.0


def ref_inverse_or_pinv(a):
    """`matrix_inverse_or_pinv` (glm2.rs:27-56): the plain inverse unless a pivot (or the determinant) is exactly zero, then the
    SVD pseudo-inverse with the cut-off 1e-12 max(s_max, 1)."""
    try:
        inv = np.linalg.inv(a)
        if np.isfinite(inv).all():
            return inv
    except np.linalg.LinAlgError:
        pass
    u, s, vt = np.linalg.svd(a)
    cut = 1e-12 * max(float(s.max()), 1.0)
    return vt.T @ np.diag([1.0 / v if (math.isfinite(v) and v > cut) else 0.0 for v in s]) @ u.T


def ref_moments(v, csel, q, r_y, order="forward"):
    """glm2.rs:211-236: e, C (rank, m), D (m, m) with z_0 = v, z_j = v c_j; `order` = how the sample sums are taken."""
    z = np.concatenate([v[:, None], v[:, None] * csel], axis=1)
    if order == "blas":
        return z.T @ r_y, q.T @ z, z.T @ z
    sl = slice(None) if order == "forward" else slice(None, None, -1)
    return _seq((z * r_y[:, None])[sl]), _seq((q[:, :, None] * z[:, None, :])[sl]), _seq((z[:, :, None] * z[:, None, :])[sl])


def ref_solve(e, c, d, rss0, df):
    """glm2.rs:238-325 -> ((beta, se, chisq, pwald) per coefficient, chisq_int_joint, p_int_joint, chisq_joint, p_joint), S."""
    m = len(e)
    k = m - 1
    s = d - c.T @ c
    s_inv = ref_inverse_or_pinv(s)
    beta = s_inv @ e
    eb = float(_seq(e * beta))
    sigma2 = max(rss0 - eb, 0.0) / float(df)
    out = []
    for a in range(m):
        var = sigma2 * s_inv[a, a]
        se = math.sqrt(var) if (math.isfinite(var) and var > 0.0) else math.nan
        ok = math.isfinite(beta[a]) and math.isfinite(se) and se > 0.0
        chisq = (beta[a] / se) ** 2 if ok else math.nan
        pw = 1.0
        if ok:
            pw = O.student_t_p_two_sided(beta[a] / se, df)
            pw = min(max(pw, MIN_POSITIVE), 1.0) if math.isfinite(pw) else 1.0
        out += [float(beta[a]), se, chisq, pw]
    s2ok = math.isfinite(sigma2) and sigma2 > 0.0
    if k > 0 and s2ok:
        bi = beta[1:]
        ci = max(float(bi @ ref_inverse_or_pinv(s_inv[1:, 1:]) @ bi) / sigma2, 0.0)
        out += [ci, ref_chi2_sf(ci, float(k))]
    else:
        out += [math.nan, 1.0]
    if s2ok:
        cj = max(eb / sigma2, 0.0)
        out += [cj, ref_chi2_sf(cj, float(m))]
    else:
        out += [math.nan, 1.0]
    return np.array(out, dtype=np.float64), s


def ref_alt_freq(g):
    """f32 ALT frequency over the called samples and the count of missing calls per row (glm2.rs:661-679)."""
    called = g >= 0
    nm = called.sum(axis=1)
    alt = np.where(called, g, 0).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = alt.astype(np.float32) / (np.float32(2.0) * nm.astype(np.float32))
    return af.astype(np.float32), (g.shape[1] - nm).astype(np.int64)


def ref_lm2_scan(g, af32, flip, x, csel, y, order="forward", with_s=False):
    """The LM2 table of the rows of g: df = n - (q_base + 1 + k) with q_base = the columns of x as given (glm2.rs:149-162)."""
    n, q_base = x.shape
    k = csel.shape[1]
    q, r_y, rss0 = ref_qr(x, y)
    df = n - (q_base + 1 + k)
    rows, ss = [], []
    for r in range(g.shape[0]):
        v = ref_decode(g[r], af32[r], bool(flip[r]) if flip is not None else False)
        st, s = ref_solve(*ref_moments(v, csel, q, r_y, order), rss0, df)
        rows.append(st)
        ss.append(s)
    return (np.stack(rows), ss) if with_s else np.stack(rows)


def lm2_errors(got, want, k):
    """The norms of the bar: beta and se relative to max(|beta|, se), every chisq relative to max(1, stat), every p relative and
    over max(1, stat).  -> (beta, se, chisq, p) maxima; NaN patterns must agree."""
    m = 1 + k
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs"
    eb = es = ec = ep = 0.0
    for a in range(m):
        b, se, ch, pw = (want[:, 4 * a + j] for j in range(4))
        ok = np.isfinite(se)
        scale = np.maximum(np.abs(b[ok]), se[ok])
        eb = max(eb, float(np.max(np.abs(got[ok, 4 * a] - b[ok]) / scale, initial=0.0)))
        es = max(es, float(np.max(np.abs(got[ok, 4 * a + 1] - se[ok]) / scale, initial=0.0)))
        ec = max(ec, float(np.max(np.abs(got[ok, 4 * a + 2] - ch[ok]) / np.maximum(1.0, ch[ok]), initial=0.0)))
        ep = max(ep, float(np.max(np.abs(got[ok, 4 * a + 3] - pw[ok]) / pw[ok] / np.maximum(1.0, ch[ok]), initial=0.0)))
        assert np.array_equal(got[~ok, 4 * a + 3], pw[~ok])
    for t in (4 * m, 4 * m + 2):
        ch, pv = want[:, t], want[:, t + 1]
        ok = np.isfinite(ch)
        ec = max(ec, float(np.max(np.abs(got[ok, t] - ch[ok]) / np.maximum(1.0, ch[ok]), initial=0.0)))
        ep = max(ep, float(np.max(np.abs(got[ok, t + 1] - pv[ok]) / pv[ok] / np.maximum(1.0, ch[ok]), initial=0.0)))
    return eb, es, ec, ep


# ---- the restatement against textbook OLS ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n129", "q5k3"])
def test_restatement_is_textbook_ols(name):
    from scipy import stats as sst
    g, x, cov_all, idx, y = lm2_panel(name)
    g = g[:40]
    n, q_base = x.shape
    k = len(idx)
    csel = cov_all[:, idx]
    af, _ = ref_alt_freq(g)
    got = ref_lm2_scan(g, af, None, x, csel, y)
    df = n - q_base - 1 - k
    worst = [0.0, 0.0, 0.0]
    for r in range(g.shape[0]):
        v = ref_decode(g[r], af[r])
        a = np.concatenate([x, v[:, None], v[:, None] * csel], axis=1)
        coef, *_ = np.linalg.lstsq(a, y, rcond=None)
        res = y - a @ coef
        cov = float(res @ res) / df * np.linalg.inv(a.T @ a)
        beta, se = coef[q_base:], np.sqrt(np.diag(cov)[q_base:])
        row = got[r]
        for j in range(1 + k):
            scale = max(abs(beta[j]), se[j])
            t2 = (beta[j] / se[j]) ** 2
            p = 2.0 * sst.t.sf(abs(beta[j] / se[j]), df)
            worst[0] = max(worst[0], abs(row[4 * j] - beta[j]) / scale, abs(row[4 * j + 1] - se[j]) / scale)
            worst[1] = max(worst[1], abs(row[4 * j + 2] - t2) / max(1.0, t2))
            worst[2] = max(worst[2], abs(row[4 * j + 3] - p) / p / max(1.0, t2))
        bi = beta[1:]
        w_int = float(bi @ np.linalg.inv(cov[q_base + 1:, q_base + 1:]) @ bi)
        w_all = float(beta @ np.linalg.inv(cov[q_base:, q_base:]) @ beta)
        for t, stat, dof in ((4 * (1 + k), w_int, k), (4 * (1 + k) + 2, w_all, 1 + k)):
            p = sst.chi2.sf(stat, dof)
            worst[1] = max(worst[1], abs(row[t] - stat) / max(1.0, stat))
            worst[2] = max(worst[2], abs(row[t + 1] - p) / p / max(1.0, stat))
    print(f"{name}: restatement against lstsq: beta / se {worst[0]:.2e}, statistics {worst[1]:.2e}, p {worst[2]:.2e}")
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8 and worst[2] <= 1e-8, worst


# ---- the restatement under reordering --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PANELS))
def test_restatement_moves_little_under_reordering(name):
    g, x, cov_all, idx, y = lm2_panel(name)
    k = len(idx)
    csel = cov_all[:, idx]
    af, _ = ref_alt_freq(g)
    flip = (np.arange(g.shape[0]) % 2).astype(bool)
    fwd, ss = ref_lm2_scan(g, af, flip, x, csel, y, "forward", with_s=True)
    cond = max(float(np.linalg.cond(s)) for s in ss)
    worst = 0.0
    for order in ("backward", "blas"):
        eb, es, ec, _ep = lm2_errors(ref_lm2_scan(g, af, flip, x, csel, y, order), fwd, k)
        worst = max(worst, eb, es, ec)
    print(f"{name}: worst reorder difference {worst:.2e}, worst cond(S) {cond:.2e}")
    assert cond <= 1e6, cond
    assert worst <= 1e-10, worst


def test_package_host_algebra_is_the_restatement():
    """`lm2.qr_projection` / `solve_from_moments` (the host recompute of flagged rows) against the restatement, and exact on the
    degenerate rows it is there for: an all-zero SNP, and an all-zero interaction column, whose coefficient is 0 without a standard
    error while the others are those of the fit without the column."""
    g, x, cov_all, idx, y = lm2_panel("q5k3")
    csel = cov_all[:, idx]
    g = g[:12].copy()
    g[3] = 0
    af, _ = ref_alt_freq(g)
    q, r_y, rss0 = ref_qr(x, y)
    q2, r2, rss2 = lm2.qr_projection(x, y)
    assert q2.shape == q.shape and np.allclose(q2, q, rtol=0, atol=1e-12) and abs(rss2 - rss0) <= 1e-10 * rss0
    df = x.shape[0] - x.shape[1] - 1 - csel.shape[1]
    for r in range(g.shape[0]):
        if r == 3:
            continue
        e, c, d = ref_moments(ref_decode(g[r], af[r]), csel, q, r_y)
        want, _s = ref_solve(e, c, d, rss0, df)
        assert np.allclose(lm2.solve_from_moments(e, c, d, rss0, df), want, rtol=1e-11, atol=0), r
    zero = lm2.solve_from_moments(*ref_moments(ref_decode(g[3], af[3]), csel, q, r_y), rss0, df)
    for a in range(4):
        assert zero[4 * a] == 0.0 and math.isnan(zero[4 * a + 1]) and math.isnan(zero[4 * a + 2]) and zero[4 * a + 3] == 1.0
    assert zero[-4] == 0.0 and zero[-3] == 1.0 and zero[-2] == 0.0 and zero[-1] == 1.0
    cz = csel.copy()
    cz[:, 1] = 0.0
    less, _s = ref_solve(*ref_moments(ref_decode(g[0], af[0]), np.delete(csel, 1, axis=1), q, r_y), rss0, df)
    got = lm2.solve_from_moments(*ref_moments(ref_decode(g[0], af[0]), cz, q, r_y), rss0, df)
    assert got[8] == 0.0 and math.isnan(got[9]) and math.isnan(got[10]) and got[11] == 1.0
    assert np.allclose(got[[0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]], less[:12], rtol=1e-9, atol=0)      # same df handed to both
    assert abs(got[16] - less[12]) <= 1e-9 * max(1.0, less[12]) and abs(got[17] - ref_chi2_sf(got[16], 3.0)) <= 1e-12 * got[17]


def test_weight_image_layout():
    """Element [tile][b][ks][lane] = column 16 b + (lane & 15) at sample 128 tile + 4 ks + (lane >> 4); the v^2 group starts at a
    whole block; zero beyond n and beyond the columns."""
    rng = np.random.default_rng(5)
    n, qr, k = 130, 4, 3
    q, r_y, csel = rng.normal(size=(n, qr)), rng.normal(size=n), rng.normal(size=(n, k))
    wv, ws = lm2.weight_columns(q, r_y, csel)
    assert wv.shape == (n, (k + 1) * (qr + 1)) and ws.shape == (n, (k + 1) * (k + 2) // 2)
    assert np.array_equal(wv[:, 0 * (qr + 1) + 2], q[:, 2]) and np.array_equal(wv[:, 2 * (qr + 1) + qr], csel[:, 1] * r_y)
    assert np.array_equal(ws[:, 0], np.ones(n)) and np.array_equal(ws[:, 3 * 4 // 2 + 1], csel[:, 2] * csel[:, 0])
    img, nblk, nbv = lm2.weight_image(wv, ws)
    assert (nblk, nbv) == (3, 2) and img.shape == (2, 3, 32, 64)
    for tile, b, ks, lane in ((0, 0, 0, 0), (0, 1, 31, 63), (1, 0, 0, 17), (1, 2, 0, 21), (1, 2, 0, 37), (1, 1, 5, 3)):
        i, col = 128 * tile + 4 * ks + (lane >> 4), 16 * b + (lane & 15)
        want = 0.0
        if i < n and col < wv.shape[1]:
            want = wv[i, col]
        elif i < n and 32 <= col < 32 + ws.shape[1]:
            want = ws[i, col - 32]
        assert img[tile, b, ks, lane] == want, (tile, b, ks, lane)


# ---- selectors -------------------------------------------------------------------------------------------------------------------

def test_selector_forms():
    p = cli._parse_lm2_covariate_selector
    assert p(None) == [] and p("") == [] and p("__SELF__") == []
    assert p("0") == [0] and p("0:3") == [0, 1, 2, 3] and p(":2") == [0, 1, 2] and p("0,3") == [0, 3]
    assert p("3:1") == [3, 2, 1] and p("2,0:2, 2") == [2, 0, 1] and p(" 1 , ,4") == [1, 4] and p("+2") == [2]


@pytest.mark.parametrize("text,msg", [
    ("1:", "-lm2/--lm2: open-ended covariate range '1:' is not supported; provide an explicit end."),
    (":", "-lm2/--lm2: invalid empty covariate range ':'."),
    ("a:2", "-lm2/--lm2: invalid covariate range start 'a'."),
    ("1:b", "-lm2/--lm2: invalid covariate range end 'b'."),
    ("x", "-lm2/--lm2: invalid covariate selector 'x'. Use 0-based indices/ranges like 0, 0:3, :2, 0,3."),
    ("-1", "-lm2/--lm2: covariate column indices must be >= 0, got -1."),
    ("1:-1", "-lm2/--lm2: covariate column indices must be >= 0, got -1."),
])
def test_selector_refusals(text, msg):
    with pytest.raises(ValueError) as e:
        cli._parse_lm2_covariate_selector(text)
    assert str(e.value) == msg


def test_selector_resolution():
    cov = np.zeros((5, 3))
    assert cli._resolve_lm2_covariate_indices(cov, [2, 0]).tolist() == [2, 0]
    assert cli._resolve_lm2_covariate_indices(cov, []).size == 0
    with pytest.raises(ValueError) as e:
        cli._resolve_lm2_covariate_indices(cov, [0, 3])
    assert str(e.value) == "-lm2/--lm2: covariate column index out of range: 3. valid=[0..2]"
    with pytest.raises(ValueError, match="at least one covariate column from -c"):
        cli._resolve_lm2_covariate_indices(np.zeros((5, 0)), [0])
    with pytest.raises(ValueError, match="2D merged covariate matrix"):
        cli._resolve_lm2_covariate_indices(np.zeros(5), [0])


# ---- the table -------------------------------------------------------------------------------------------------------------------

def test_header_names_columns_by_their_index():
    assert tsv.lm2_header([2, 0]) == ("chrom\tpos\tsnp\tallele0\tallele1\taf\tmiss\tbeta\tse\tchisq\tpwald\tbeta_i2\tse_i2\tpwald_i2\t"
                                      "beta_i0\tse_i0\tpwald_i0\tchisq_int_joint\tp_int_joint\tchisq_joint\tp_joint\n")


def test_row_rendering():
    st = [0.123449, 0.05, 6.0956, 3.21e-5, math.nan, math.nan, math.nan, 1.0, math.inf, 1e-300, 12.34567, 0.002]
    row = tsv.format_lm2_row("1", 1000, "rs1", "A", "G", np.float32(0.25), 3, st)
    assert row == "1\t1000\trs1\tA\tG\t0.2500\t3\t0.1234\t0.0500\t6.0956e0\t3.2100e-5\tNaN\tNaN\t1.0000e0\tinf\t1.0000e-300\t1.2346e1\t2.0000e-3\n"
    nan_row = tsv.format_lm2_row("2", 5, "2_5", "A", "C", np.float32(0.0), 0, [0.0, math.nan, math.nan, 1.0, 0.0, math.nan, math.nan, 1.0,
                                                                             0.0, 1.0, 0.0, 1.0])
    assert nan_row == "2\t5\t2_5\tA\tC\t0.0000\t0\t0.0000\tNaN\tNaN\t1.0000e0\t0.0000\tNaN\t1.0000e0\t0.0000e0\t1.0000e0\t0.0000e0\t1.0000e0\n"


def test_writer_renames_and_resolves_names(tmp_path):
    path = str(tmp_path / "t.lm2.tsv")
    stats = np.arange(24, dtype=np.float64).reshape(2, 12) / 7.0
    assert tsv.write_lm2_tsv(path, ["1", "1"], [10, 20], [".", "rs2"], ["A", "A"], ["G", "T"], np.float32([0.1, 0.2]), [0, 4], stats,
                             [1]) == 2
    lines = open(path).read().split("\n")
    assert lines[0] == tsv.lm2_header([1]).rstrip("\n") and lines[1].split("\t")[:7] == ["1", "10", "1_10", "A", "G", "0.1000", "0"]
    assert lines[2].split("\t")[2] == "rs2" and lines[3] == "" and os.listdir(tmp_path) == ["t.lm2.tsv"]
    with pytest.raises(RuntimeError):
        tsv.write_lm2_tsv(path, [], [], [], [], [], [], [], np.zeros((0, 12)), [1, 2])


# ---- the df quirk ----------------------------------------------------------------------------------------------------------------

def test_df_counts_the_columns_of_x_as_given():
    g, x, cov_all, idx, y = lm2_panel("q5k3")
    g = g[:6]
    csel = cov_all[:, idx]
    af, _ = ref_alt_freq(g)
    xd = np.concatenate([x, x[:, 2:3]], axis=1)                  # a duplicated column: q_rank = q_base - 1
    q, _r, _rss = ref_qr(xd, y)
    assert q.shape[1] == x.shape[1] == xd.shape[1] - 1
    assert lm2.qr_projection(xd, y)[0].shape[1] == x.shape[1]
    full, dup = ref_lm2_scan(g, af, None, x, csel, y), ref_lm2_scan(g, af, None, xd, csel, y)
    n, k = x.shape[0], len(idx)
    df_full, df_dup = n - x.shape[1] - 1 - k, n - xd.shape[1] - 1 - k
    assert np.allclose(dup[:, 0], full[:, 0], rtol=1e-9)                                         # same fit ...
    assert np.allclose(dup[:, 1], full[:, 1] * math.sqrt(df_full / df_dup), rtol=1e-9)           # ... one degree of freedom fewer


# ---- refusals before any device call ---------------------------------------------------------------------------------------------

def _lm2_call(**kw):
    n = kw.pop("n", 20)
    args = dict(prefix="/nonexistent/prefix", y=np.zeros(n), x=np.ones((n, 2)), cov_all=np.ones((n, 3)), cov_indices=[0, 2],
                out_tsv="/nonexistent/out.tsv")
    args.update(kw)
    return jx.lm2_stream_bed_to_tsv(**args)


def _lm_call(**kw):
    n = kw.pop("n", 20)
    args = dict(prefix="/nonexistent/prefix", y=np.zeros(n), x=np.ones((n, 2)), ixx=None, out_tsv="/nonexistent/out.tsv")
    args.update(kw)
    return jx.lm_stream_bed_to_tsv(**args)


@pytest.mark.parametrize("call", [_lm2_call, _lm_call])
def test_shared_refusals(call):
    for kw, exc, msg in (
            (dict(chunk_size=0), ValueError, "chunk_size must be > 0"),
            (dict(maf_threshold=0.6), ValueError, "maf_threshold must be within [0, 0.5]"),
            (dict(maf_threshold=-0.1), ValueError, "maf_threshold must be within [0, 0.5]"),
            (dict(max_missing_rate=1.5), ValueError, "max_missing_rate must be within [0, 1.0]"),
            (dict(het_threshold=-1.0), ValueError, "het_threshold must be within [0, 1.0]"),
            (dict(genetic_model="mult"), ValueError, "genetic_model must be one of: add, dom, rec, het"),
            (dict(genetic_model="dom"), RuntimeError, "genetic_model 'dom' is outside this build's scope (additive model only)"),
            (dict(mmap_window_mb=0), ValueError, "mmap_window_mb must be > 0"),
            (dict(x=np.ones((19, 2))), RuntimeError, "X.n_rows must equal len(y)"),
            (dict(row_indices=[0, 1], row_flip=[False, False], row_missing=[0.0, 0.0]), RuntimeError,
             "prepared row metadata must provide all or none of: row_indices, row_flip, row_missing, row_maf"),
            (dict(row_indices=[3, 1], row_flip=[False, False], row_missing=[0.0, 0.0], row_maf=[0.1, 0.2]), RuntimeError,
             "prepared row_indices must be sorted in ascending BED order"),
            (dict(row_indices=[1, 3], row_flip=[False], row_missing=[0.0, 0.0], row_maf=[0.1, 0.2]), RuntimeError,
             "prepared row metadata length mismatch: row_indices=2, row_flip=1, row_missing=2, row_maf=2")):
        with pytest.raises(exc) as e:
            call(**kw)
        assert str(e.value) == msg, kw


def test_lm2_refusals():
    for kw, msg in (
            (dict(n=5), "n too small: require n > q_base + 1 + n_interactions, got n=5, q_base=2, n_interactions=2"),
            (dict(cov_indices=[]), "LM2 requires at least one explicitly selected covariate column."),
            (dict(cov_indices=[0, 3]), "cov_indices out of range: 3 >= 3"),
            (dict(cov_indices=[-1]), "cov_indices must be >= 0"),
            (dict(cov_all=np.ones((19, 3))), "cov_all.n_rows must equal len(y)"),
            (dict(cov_all=np.ones((20, 0))), "LM2 requires cov_all with at least one column"),
            (dict(cov_all=np.ones((40, 12)), cov_indices=list(range(9)), n=40, x=np.ones((40, 2))),
             "LM2 supports at most 8 interaction covariates in this build, got 9")):
        with pytest.raises(RuntimeError) as e:
            _lm2_call(**kw)
        assert str(e.value) == msg, kw


def test_lm_refusals():
    with pytest.raises(RuntimeError) as e:
        _lm_call(n=3)
    assert str(e.value) == "n too small: require n > q0+1, got n=3, q0=2"
    with pytest.raises(RuntimeError) as e:
        _lm_call(ixx=np.eye(3))
    assert str(e.value) == "ixx must be (q0,q0)"


def test_cli_names_the_new_flags(tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["gwas", "-bfile", str(tmp_path / "none"), "-p", str(tmp_path / "none.tsv")])
    assert str(e.value) == "select at least one model: -lm, -lm2, -lmm, -lmm2, -fvlmm, -splmm and/or -splmm-exact"
    with pytest.raises(SystemExit) as e:
        cli.main(["gwas", "-bfile", str(tmp_path / "none"), "-p", str(tmp_path / "none.tsv"), "-lm2", "2:"])
    assert "open-ended covariate range" in str(e.value)


# ---- the row filter --------------------------------------------------------------------------------------------------------------

def test_row_filter_against_hand_counts():
    n = 10
    # (missing, het, hom_alt): a common SNP; one missing call; 3 of 10 missing; rare; no call at all; monomorphic ALT; folded
    counts = np.array([[0, 4, 1], [1, 3, 0], [3, 2, 2], [0, 1, 0], [10, 0, 0], [0, 0, 10], [0, 2, 7]])
    keep, af, miss = lm2.row_filter(counts, n, 0.0, 1.0)
    assert keep.tolist() == [True, True, True, True, False, True, True]
    assert af.dtype == np.float32 and miss.tolist() == [0, 1, 3, 0, 10, 0, 0]
    want = np.float32([6 / 20, 3 / 18, 6 / 14, 1 / 20, 0.0, 1.0, 16 / 20])
    assert np.array_equal(af, np.float32([np.float32(6) / np.float32(20), np.float32(3) / np.float32(18), np.float32(6) / np.float32(14),
                                          np.float32(1) / np.float32(20), 0.0, 1.0, np.float32(16) / np.float32(20)]))
    assert np.allclose(af, want)
    keep, _af, _miss = lm2.row_filter(counts, n, 0.1, 0.25)
    # 3 / 10 missing > 0.25; maf 0.05 and 0.0 < 0.1; the folded row has maf 0.2 and its af column stays 0.8
    assert keep.tolist() == [True, True, False, False, False, False, True]
    keep, _af, _miss = lm2.row_filter(counts, n, 0.0, 0.1)
    assert keep.tolist() == [True, True, False, True, False, True, True]      # 1 / 10 is not > 0.1 in f32
    g, *_ = lm2_panel("n129")
    af_ref, miss_ref = ref_alt_freq(g)
    cnt = np.stack([(g < 0).sum(1), (g == 1).sum(1), (g == 2).sum(1)], axis=1)
    keep, af, miss = lm2.row_filter(cnt, g.shape[1], 0.0, 1.0)
    assert keep.all() and np.array_equal(af, af_ref) and np.array_equal(miss, miss_ref)
