"""Plain numpy / scipy f64 restatement of the reference's multi-kernel variance-component route, written from the source and
literal to it: `ai_reml_multi_f64` (src/stats/reml.rs:703-1049), `REML()` (python/janusx/pyBLUP/blup.py:158-229) and the dense
`BLUP._fit` / `predict` (blup.py:683-1004) with their helpers (`_testX` :231, `_normalize_G` :313, `_onehotZ` :360).  The probe
matrix is an argument: the StdRng stream of reml.rs:798-806 is not part of this file.  The Rust was not run; nothing here calls
janusx_amd."""
import math
from types import SimpleNamespace

import numpy as np
from scipy.linalg import cho_solve
from scipy.optimize import minimize

OBJ_PENALTY = 1e30          # blup.py:24
TRUE_VAR = (0.5, 0.3, 0.4)  # simulated variances of the kernels of make_case, then 0.3 for the residual
RESID_VAR = 0.3


# ---- designs -------------------------------------------------------------------------------------------------------------------

def _make(n, q, seed):
    """-> (k_stack (q, n, n), x (n, 2), y (n,), theta_true (q + 1,), the one-hot factor or None).  K1: centred binomial genotypes, 3 n markers, G G' / 3 n;
    K2: Z Z' of a one-hot factor with max(4, n // 12) levels; K3: a Wishart kernel scaled to mean diagonal 1; X = [1 | N(0, 1)];
    y simulated with variances (0.5, 0.3, 0.4 | 0.3)."""
    rng = np.random.default_rng(1000 + seed)
    z = None
    m = 3 * n
    frq = rng.uniform(0.1, 0.5, size=m)
    g = rng.binomial(2, frq[None, :], size=(n, m)).astype(np.float64)
    g -= g.mean(axis=0, keepdims=True)
    kernels = [g @ g.T / float(m)]
    if q >= 2:
        lev = max(4, n // 12)
        codes = rng.integers(0, lev, size=n)
        codes[:min(lev, n)] = np.arange(min(lev, n))        # every level occurs
        z = np.zeros((n, lev))
        z[np.arange(n), codes] = 1.0
        kernels.append(z @ z.T)
    if q >= 3:
        w = rng.standard_normal((n, n + 8))
        k3 = w @ w.T
        kernels.append(k3 / np.mean(np.diag(k3)))
    assert 1 <= q <= 3
    k_stack = np.stack(kernels[:q], axis=0)
    x = np.column_stack([np.ones(n), rng.standard_normal(n)])
    theta = np.array(list(TRUE_VAR[:q]) + [RESID_VAR])
    v = theta[-1] * np.eye(n)
    for j in range(q):
        v += theta[j] * k_stack[j]
    y = x @ np.array([1.0, 0.5]) + np.linalg.cholesky(v) @ rng.standard_normal(n)
    return k_stack, x, y, theta, z


def make_case(n, q, seed):
    """The designs of the tests, see `_make`."""
    return _make(n, q, seed)[:4]


def make_blup_case(n, seed):
    """make_case(n, 3, seed) as `BLUP` takes it: -> (y, covariate column, Z one-hot, [G1, G3]); G1 is handed over at twice its
    scale, so that the normalisation has something to undo."""
    k_stack, x, y, _theta, z = _make(n, 3, seed)
    return y, x[:, 1].copy(), z, [2.0 * k_stack[0], k_stack[2]]


def case_v(n, seed):
    """The covariance matrix of make_case(n, min(3, ..), seed) at the truth: the SPD test matrix of the factor and solve tests."""
    k_stack, _x, _y, theta = make_case(n, 3 if n >= 4 else 1, seed)
    v = theta[-1] * np.eye(n)
    for j in range(k_stack.shape[0]):
        v += theta[j] * k_stack[j]
    return (v + v.T) * 0.5


# ---- reml.rs:703-1049 ----------------------------------------------------------------------------------------------------------

def _trace_ab(a, b):
    """reml.rs:691-701: sum_rc a[r, c] b[c, r]."""
    return float(np.sum(a * b.T))


def _sym(k_stack):
    ks = np.asarray(k_stack, dtype=np.float64)
    return [(ks[j] + ks[j].T) * 0.5 for j in range(ks.shape[0])]          # reml.rs:776


def profile(kmats, x, y, theta):
    """reml.rs:833-884 (the same lines as 966-1012 for a candidate) -> (reml, ml, pieces) or None where the source breaks / halves."""
    n, p = x.shape
    q = len(kmats)
    v = np.eye(n) * theta[q]                                             # :834
    for j in range(q):
        v = v + kmats[j] * theta[j]                                       # :836
    try:
        lv = np.linalg.cholesky(v)                                        # :838
    except np.linalg.LinAlgError:
        return None
    vinv_x = cho_solve((lv, True), x)                                     # :842
    xt_vinv_x = x.T @ vinv_x
    try:
        lx = np.linalg.cholesky(xt_vinv_x)                                # :844
    except np.linalg.LinAlgError:
        return None
    c_inv = cho_solve((lx, True), np.eye(p))                              # :847
    vinv_y = cho_solve((lv, True), y)                                     # :849
    beta = cho_solve((lx, True), x.T @ vinv_y)                            # :851
    r = y - x @ beta                                                      # :853
    vinv_r = cho_solve((lv, True), r)                                     # :854
    alpha = vinv_r - vinv_x @ (c_inv @ (x.T @ vinv_r))                    # :855-856
    qval = float(r @ vinv_r)                                              # :857
    if not np.isfinite(qval) or qval <= 0.0:
        return None
    log_det_v = float(np.sum(2.0 * np.log(np.diag(lv))))                  # :862-866
    log_det_xt = float(np.sum(2.0 * np.log(np.diag(lx))))                 # :867-871
    nf, pf = float(n), float(p)
    reml_c = (nf - pf) * (math.log(nf - pf) - 1.0 - math.log(2.0 * math.pi)) / 2.0
    reml = reml_c - 0.5 * ((nf - pf) * math.log(qval) + log_det_v + log_det_xt)     # :874-876
    ml_c = nf * (math.log(nf) - 1.0 - math.log(2.0 * math.pi)) / 2.0
    ml = ml_c - 0.5 * (nf * math.log(qval) + log_det_v)                   # :877-879
    if not np.isfinite(reml) or not np.isfinite(ml):
        return None
    return reml, ml, {"lv": lv, "vinv_x": vinv_x, "c_inv": c_inv, "beta": beta, "r": r, "vinv_r": vinv_r, "alpha": alpha,
                      "qval": qval, "log_det_v": log_det_v, "log_det_xt": log_det_xt}


def ai_step(kmats, x, pieces, probes=None, detail=None):
    """reml.rs:886-952 -> (score, ai, delta) or None.  probes None: exact trace (:890-894, 910-911); else (n_probes, n).
    `detail`, a dict, receives the terms of the score (tr1, tr2, quad per component) and the vectors behind the AI matrix."""
    n, p = x.shape
    q = len(kmats)
    m = q + 1
    lv, vinv_x, c_inv, alpha = pieces["lv"], pieces["vinv_x"], pieces["c_inv"], pieces["alpha"]
    eye = np.eye(n)
    vinv_exact = cho_solve((lv, True), eye) if probes is None else None   # :890-894
    vinv_probe = None if probes is None else [cho_solve((lv, True), z) for z in probes]     # :896-901
    score = np.zeros(m)
    ka_list, pka_list = [], []
    for j in range(m):
        kj = kmats[j] if j < q else eye                                   # :904
        ka = kj @ alpha
        quad = float(alpha @ ka)
        ka_list.append(ka)
        if vinv_exact is not None:
            tr1 = _trace_ab(vinv_exact, kj)                               # :911
        else:
            s = 0.0
            for z, vz in zip(probes, vinv_probe):                         # :915-918
                s += float(vz @ (kj @ z))
            tr1 = s / float(len(probes))
        kb = kj @ vinv_x                                                  # :924
        tr2 = _trace_ab(c_inv, vinv_x.T @ kb)                             # :925-926
        score[j] = -0.5 * ((tr1 - tr2) - quad)                            # :927-928
        if detail is not None:
            detail.setdefault("terms", []).append((tr1, tr2, quad))
        vinv_ka = cho_solve((lv, True), ka)                               # :930
        pka_list.append(vinv_ka - vinv_x @ (c_inv @ (vinv_x.T @ ka)))     # :931
    if detail is not None:
        detail["ka"], detail["pka"] = ka_list, pka_list
    ai = np.zeros((m, m))
    for a in range(m):
        for b in range(a + 1):
            ai[a, b] = ai[b, a] = 0.5 * float(ka_list[a] @ pka_list[b])   # :936-942
    for d in range(m):
        ai[d, d] += 1e-10                                                 # :943-945
    try:
        delta = np.linalg.solve(ai, score)                                # :947
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(delta)):
        return None
    return score, ai, delta


def ai_reml_multi_f64(k_stack, xcov, y, max_iter=100, tol=1e-6, min_var=1e-12, trace_probes=8, probes=None, log=None):
    """reml.rs:703-1049 -> (theta, ml, reml, used_iter, converged).  `probes` (n_probes, n) is used when the source would draw
    them (trace_probes != 0 and n > 768).  `log`, a list, receives one dict per iteration: the halvings, the margin of every
    acceptance test (reml_cand - reml_curr + 1e-12) and the stopping quantity rel_max."""
    ks = np.asarray(k_stack, dtype=np.float64)
    if ks.ndim != 3:
        raise RuntimeError("k_stack must be 3D (q, n, n)")
    q, n = ks.shape[0], ks.shape[1]
    if ks.shape[2] != n:
        raise RuntimeError("k_stack must be (q, n, n)")
    if q == 0:
        raise RuntimeError("k_stack requires at least one kernel")
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if y.shape[0] != n:
        raise RuntimeError("len(y) must equal n in k_stack")
    x = np.asarray(xcov, dtype=np.float64)
    if x.shape[0] != n:
        raise RuntimeError("xcov.n_rows must equal n in k_stack")
    p = x.shape[1]
    if p == 0:
        raise RuntimeError("xcov must have at least one column")
    if n <= p:
        raise RuntimeError("n must be > p in xcov")
    if not (np.isfinite(min_var) and min_var > 0.0):
        min_var = 1e-12
    if not (np.isfinite(tol) and tol > 0.0):
        tol = 1e-6
    kmats = _sym(ks)
    use_exact = trace_probes == 0 or n <= 768                             # :794
    if not use_exact and probes is None:
        raise ValueError("the probe route needs the probe matrix")
    pr = None if use_exact else np.asarray(probes, dtype=np.float64)
    mean = float(np.sum(y)) / float(n)
    var_y = float(np.sum((y - mean) ** 2)) / float(max(n, 2) - 1)         # :809-817
    if not np.isfinite(var_y) or var_y <= 0.0:
        var_y = 1.0
    m = q + 1
    theta = np.full(m, max(var_y / float(m), min_var))                    # :823
    converged, used_iter = False, 0
    last_ml = last_reml = float("nan")
    for it in range(int(max_iter)):
        used_iter = it + 1
        prof = profile(kmats, x, y, theta)
        if prof is None:
            break
        reml_curr, ml_curr, pieces = prof
        last_reml, last_ml = reml_curr, ml_curr
        step_out = ai_step(kmats, x, pieces, pr)
        if step_out is None:
            break
        delta = step_out[2]
        accepted, step = False, 1.0
        theta_next, reml_next, ml_next = theta.copy(), reml_curr, ml_curr
        rec = {"it": used_iter, "halvings": 0, "margins": [], "rel_max": None, "reml": reml_curr}
        for _ in range(24):                                               # :960
            cand = np.maximum(theta + step * delta, min_var)              # :961-964
            pc = profile(kmats, x, y, cand)
            if pc is not None:
                rec["margins"].append(pc[0] - (reml_curr - 1e-12))
            if pc is not None and pc[0] >= reml_curr - 1e-12:             # :1013
                accepted, theta_next, reml_next, ml_next = True, cand, pc[0], pc[1]
                break
            step *= 0.5
            rec["halvings"] += 1
            if step < 1e-8:
                break
        if log is not None:
            log.append(rec)
        if not accepted:
            break
        rel_max = float(np.max(np.abs(theta_next - theta) / np.maximum(theta, min_var)))       # :1030-1036
        rec["rel_max"] = rel_max
        theta, last_reml, last_ml = theta_next, reml_next, ml_next
        if rel_max < tol:
            converged = True
            break
    return theta, last_ml, last_reml, used_iter, converged


class MultiKernelRemlRef:
    """The two blocks above behind the interface of `pipeline.MultiKernelReml` (profile / ai_step at a given theta)."""

    def __init__(self, k_stack, x, y):
        self.kmats = _sym(k_stack)
        self.q, self.n = len(self.kmats), self.kmats[0].shape[0]
        self.x = np.asarray(x, dtype=np.float64).reshape(self.n, -1)
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.p = self.x.shape[1]

    def profile(self, theta):
        return profile(self.kmats, self.x, self.y, np.asarray(theta, dtype=np.float64).reshape(-1))

    def ai_step(self, theta, probes=None, detail=None):
        prof = self.profile(theta)
        if prof is None:
            return None
        return ai_step(self.kmats, self.x, prof[2], None if probes is None else np.asarray(probes, dtype=np.float64), detail)


# ---- blup.py -------------------------------------------------------------------------------------------------------------------

def REML(theta, y, X, Klist):
    """blup.py:158-229, the objective of the L-BFGS-B fallback (lower is better)."""
    theta = np.asarray(theta, dtype=float).reshape(-1)
    if theta.size != len(Klist) + 1 or not np.all(np.isfinite(theta)) or np.any(theta <= 0.0):
        return OBJ_PENALTY
    n, p = X.shape
    V = theta[-1] * np.eye(n)
    for num, K in enumerate(Klist):
        V += theta[num] * np.asarray(K, dtype=float)
    try:
        L = np.linalg.cholesky(V)
    except np.linalg.LinAlgError:
        return OBJ_PENALTY
    VinvX = cho_solve((L, True), X)
    Vinvy = cho_solve((L, True), y)
    XTV_invX = X.T @ VinvX
    beta, _res, rank, _sv = np.linalg.lstsq(XTV_invX, X.T @ Vinvy, rcond=None)
    if int(rank) < int(p):
        return OBJ_PENALTY
    r = y - X @ beta
    Vinvr = cho_solve((L, True), r)
    rTV_invr = float((r.T @ Vinvr)[0, 0])
    if not np.isfinite(rTV_invr) or rTV_invr <= 0.0:
        return OBJ_PENALTY
    log_detV = float(2.0 * np.sum(np.log(np.diag(L))))
    sign, log_detX = np.linalg.slogdet(XTV_invX)
    if sign <= 0 or not np.isfinite(log_detX):
        return OBJ_PENALTY
    total_log = (n - p) * np.log(rTV_invr) + log_detV + float(log_detX)
    c = (n - p) * (np.log(n - p) - 1 - np.log(2 * np.pi)) / 2.0
    out = float(total_log / 2.0 - c)
    return out if np.isfinite(out) else OBJ_PENALTY


def onehot_info(Z_list, ridge=1e-8):
    """blup.py:360-389, dense inputs."""
    info = []
    for z in Z_list:
        zz = np.asarray(z, dtype=float)
        if bool(np.isin(zz, [0, 1]).all() and (zz.sum(axis=1) > 0).all()):
            info.append((1, 0.0, 1.0))
        else:
            info.append((float(zz.shape[1]), zz.mean(axis=0), zz.std(axis=0) + ridge))
    return info


def normalize_G(G_list, ridge=1e-8):
    """blup.py:313-330."""
    out, scales = [], []
    for g in G_list:
        gs = np.asarray(g, dtype=float)
        gs = (gs + gs.T) / 2.0
        s = float(np.mean(np.diag(gs))) + float(ridge)
        out.append(gs / s)
        scales.append(s)
    return out, scales


def blup_fit(y, X=None, Z=None, G=None, maxiter=100, probes=None, force_fallback=False, theta0_scale=1.0):
    """The dense route of `BLUP._fit` (blup.py:786-901) -> namespace(theta, var, beta, u, g_by_G, g, fitted, residuals, route,
    sigma2, cov_beta).  `force_fallback`: skip AI-REML (what a non-converged run does, blup.py:542-543, 807-830);
    `theta0_scale` multiplies the fallback's start value (the tests measure the optimiser's own spread with it)."""
    y = np.asarray(y, dtype=float).reshape(-1, 1)
    n = y.shape[0]
    X = np.ones((n, 1)) if X is None else np.concatenate([np.ones((n, 1)), np.asarray(X, dtype=float).reshape(n, -1)], axis=1)
    Z_list = [] if Z is None else ([np.asarray(Z, dtype=float)] if isinstance(Z, np.ndarray) else [np.asarray(z, dtype=float) for z in Z])
    G_list = [] if G is None else ([np.asarray(G, dtype=float)] if isinstance(G, np.ndarray) else [np.asarray(g, dtype=float) for g in G])
    info = onehot_info(Z_list)
    Zst = [(z - info[i][1]) / info[i][2] / np.sqrt(info[i][0]) for i, z in enumerate(Z_list)]         # :786-793
    Gnorm, g_scales = normalize_G(G_list)
    Klist = [z @ z.T for z in Zst] + Gnorm                                                           # :795
    theta, route = None, None
    if not force_fallback:
        k_stack = np.stack([(k + k.T) / 2.0 for k in Klist], axis=0)
        tp = 0 if n <= 768 else (16 if n <= 2048 else 12)                                            # :521-526
        th, _ml, _reml, _nit, conv = ai_reml_multi_f64(k_stack, X, y.reshape(-1), max_iter=int(maxiter), tol=1e-6, min_var=1e-12,
                                                       trace_probes=tp, probes=probes)
        if conv and np.all(np.isfinite(th)) and not np.any(th <= 0.0):                                # :540-543
            theta, route = np.asarray(th, dtype=float), "aireml"
    if theta is None:
        theta0 = np.ones(len(Klist) + 1) * float(theta0_scale)                                       # :808
        res = minimize(REML, theta0, args=(y, X, Klist), method="L-BFGS-B", bounds=[(1e-12, None)] * len(theta0),
                       options={"maxiter": int(maxiter), "ftol": 1e-12, "gtol": 1e-8})                 # :819-827
        theta, route = np.asarray(res.x, dtype=float), "lbfgsb"
    V = theta[-1] * np.eye(n)
    for num, K in enumerate(Klist):
        V += theta[num] * K
    L = np.linalg.cholesky(V)
    VinvX = cho_solve((L, True), X)
    Vinvy = cho_solve((L, True), y)
    beta, _res, _rank, _sv = np.linalg.lstsq(X.T @ VinvX, X.T @ Vinvy, rcond=None)                    # :840-844
    r = y - X @ beta
    Vinvr = cho_solve((L, True), r)
    nz = len(Zst)
    if nz:
        Zall = np.concatenate(Zst, axis=1)
        Gall = np.concatenate([theta[i] * np.ones(z.shape[1]) for i, z in enumerate(Zst)])
        u = (Zall.T @ Vinvr) * Gall[:, None]                                                          # :863
        z_fitted = Zall @ u
    else:
        u, z_fitted = None, np.zeros((n, 1))
    g_by_G, g_total = [], np.zeros((n, 1))
    for idx, gk in enumerate(Gnorm):
        gi = theta[nz + idx] * (gk @ Vinvr)                                                           # :874
        g_by_G.append(gi)
        g_total += gi
    fitted = X @ beta + z_fitted + g_total
    sigma2 = float((r.T @ Vinvr)[0, 0]) / max(1, n - X.shape[1])                                      # :879
    var = np.array([theta[i] * np.diag(Klist[i]).mean() for i in range(len(Klist))] + [theta[-1]])    # :884-887
    return SimpleNamespace(theta=theta, var=var, beta=beta, u=u, g_by_G=g_by_G, g=g_total, fitted=fitted, residuals=y - fitted,
                           route=route, sigma2=sigma2, cov_beta=np.linalg.pinv(X.T @ VinvX) * sigma2, z_fitted=z_fitted,
                           g_scales=g_scales, Klist=Klist, X=X)
