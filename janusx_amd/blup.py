"""`BLUP`: best linear unbiased prediction with several random effects, the dense multi-kernel route of the reference's class
(python/janusx/pyBLUP/blup.py:610-1004).  Every Z (a design matrix) and every G (an n x n relationship matrix) gets one variance
component; the components are estimated by `janusx.ai_reml_multi_f64` (AI-REML on the device) and, when that does not converge,
by scipy L-BFGS-B over the profiled REML (blup.py:807-830) whose every evaluation is `pipeline.MultiKernelReml.profile`: the
n x n matrix V is formed, factored and solved in HBM on both routes.

Not built, and refused with a message: sparse-matrix inputs, and the sparse one-hot fast path (`_can_use_sparse_z_reml`, a
Rust cache object): with only one-hot Z and no G at n >= 800 the dense route runs instead.
Extension: `exact_trace=True` asks AI-REML for the exact trace (trace_probes = 0) at every n; the reference switches to
Hutchinson probes above n = 768 (blup.py:521-526)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import janusx as jxrs

_OBJ_PENALTY = 1e30          # blup.py:24


def _refuse_sparse(a, what):
    if hasattr(a, "tocsr") or hasattr(a, "toarray"):
        raise TypeError(f"BLUP: sparse {what} is not supported on this build; pass a dense numpy array")


def _test_x(X, n):
    """blup.py:231-251: the intercept is always added."""
    if X is None:
        return np.ones((n, 1))
    _refuse_sparse(X, "X")
    X = np.asarray(X, dtype=float)
    if X.size == n:
        return np.concatenate([np.ones((n, 1)), X.reshape(-1, 1)], axis=1)
    if X.shape[0] == n:
        return np.concatenate([np.ones((n, 1)), X], axis=1)
    raise ValueError(f"Row number of X is not equal to {n} in y. (X.shape={X.shape}, n={n})")


def _test_z(Z, n):
    """blup.py:265-288."""
    if Z is None:
        return []
    _refuse_sparse(Z, "Z")
    z_list = [Z] if isinstance(Z, np.ndarray) else list(Z)
    for idx, z in enumerate(z_list):
        _refuse_sparse(z, f"Z{idx}")
        if not isinstance(z, np.ndarray):
            raise TypeError(f"Type of Z{idx} is {type(z)}")
        if int(z.shape[0]) == int(n):
            z_list[idx] = np.asarray(z, dtype=float).reshape(n, -1)
        elif z.size == n:
            z_list[idx] = np.asarray(z, dtype=float).reshape(-1, 1)
        else:
            raise ValueError(f"Row number of Z{idx} is not equal to {n} in y. (Z{idx}.shape={z.shape}, n={n})")
    return z_list


def _test_g(G, n):
    """blup.py:290-311."""
    if G is None:
        return []
    _refuse_sparse(G, "G")
    g_list = [G] if isinstance(G, np.ndarray) else list(G)
    for idx, g in enumerate(g_list):
        _refuse_sparse(g, f"G{idx}")
        g = np.asarray(g, dtype=float)
        g_list[idx] = g
        if g.ndim != 2:
            raise ValueError(f"G{idx} must be 2D. (G{idx}.shape={g.shape})")
        if g.shape[0] != n or g.shape[1] != n:
            raise ValueError(f"G{idx} must be square (n,n). (G{idx}.shape={g.shape}, n={n})")
    return g_list


def _test_g_predict(G, n_pred, n_train):
    """blup.py:332-358."""
    if G is None:
        return []
    g_list = [G] if isinstance(G, np.ndarray) else list(G)
    checked = []
    for idx, g in enumerate(g_list):
        g = np.asarray(g, dtype=float)
        if g.ndim != 2:
            raise ValueError(f"G[{idx}] must be 2D. (shape={g.shape})")
        if g.shape == (n_pred, n_train) or (g.shape == (n_train, n_train) and n_pred == n_train):
            checked.append(g)
        else:
            raise ValueError(f"G[{idx}] shape mismatch: expected ({n_pred},{n_train}) or ({n_train},{n_train}) for in-sample, "
                             f"got {g.shape}")
    return checked


def _onehot_z(z_list, ridge=1e-8):
    """blup.py:360-389 (dense): (q, mean, std) of the standardisation, (1, 0, 1) for a one-hot design."""
    info = []
    for z in z_list:
        zz = np.asarray(z, dtype=float)
        if bool(np.isin(zz, [0, 1]).all() and (zz.sum(axis=1) > 0).all()):
            info.append((1, 0.0, 1.0))
        else:
            info.append((float(zz.shape[1]), zz.mean(axis=0), zz.std(axis=0) + ridge))
    return info


def _normalize_g(g_list, ridge=1e-8):
    """blup.py:313-330: symmetrise, divide by the mean diagonal + 1e-8."""
    out, scales = [], []
    for idx, g in enumerate(g_list):
        gs = np.asarray(g, dtype=float)
        gs = (gs + gs.T) / 2.0
        dmean = float(np.mean(np.diag(gs)))
        if not np.isfinite(dmean) or dmean <= 0.0:
            raise ValueError(f"G{idx} has invalid mean diagonal ({dmean}); cannot normalize.")
        s = dmean + float(ridge)
        out.append(gs / s)
        scales.append(s)
    return out, scales


def trace_probes_for(n, exact_trace=False):
    """The reference's probe dispatch (blup.py:521-526); `exact_trace` (an extension) asks for the exact trace at every n."""
    if exact_trace or n <= 768:
        return 0
    return 16 if n <= 2048 else 12


class BLUP:
    """`BLUP(y, X=None, Z=None, G=None, maxiter=100, progress=True)` (blup.py:610-681).  Attributes as in the reference: `beta`
    (p + 1, 1), `u`, `u_by_Z`, `g`, `g_by_G`, `theta`, `var` (theta_j x mean diag K_j, residual last), `fitted`, `residuals`,
    `result` (`message` names the route: "ai_reml" or scipy's), `route` ("aireml" / "aireml-exact" / "lbfgsb"; ours).
    `progress` is accepted; no bar is drawn."""

    def __init__(self, y, X=None, Z=None, G=None, maxiter=100, progress=True, exact_trace=False):
        y = np.asarray(y, dtype=float).reshape(-1, 1)
        n = y.shape[0]
        X = _test_x(X, n)
        self.Z_list = _test_z(Z, n)
        self.G_list = _test_g(G, n)
        self.onehot_info = _onehot_z(self.Z_list)
        self.z_cols = [z.shape[1] for z in self.Z_list]
        self.g_count = len(self.G_list)
        self.y, self.X, self.n, self.p = y, X, n, X.shape[1]
        self.maxiter, self.progress, self.exact_trace = maxiter, progress, bool(exact_trace)
        self.route = None
        self._fit()

    def _fit_lm(self):
        """blup.py:684-727: no random effect, ordinary least squares."""
        self.theta = self.V = None
        beta, _res, rank, _sv = np.linalg.lstsq(self.X, self.y, rcond=None)
        if int(rank) < int(self.X.shape[1]):
            raise np.linalg.LinAlgError(f"Fixed-effect design is rank deficient: rank={int(rank)}, columns={int(self.X.shape[1])}.")
        self.beta = np.asarray(beta, dtype=float)
        self.u = self.u_by_Z = self.g = None
        self.g_by_G, self._g_scales = [], []
        self._Vinvr = self._z_theta = self._g_theta = self._z_fitted = None
        self._z_standardized = False
        fitted = self.X @ self.beta
        residuals = self.y - fitted
        self._cov_beta = np.linalg.pinv(self.X.T @ self.X) * (float((residuals.T @ residuals)[0, 0]) / max(1, self.n - self.p))
        self.fitted, self.residuals, self.result, self.route = fitted, residuals, None, "lm"

    def _fit(self):
        if len(self.Z_list) == 0 and len(self.G_list) == 0:
            self._fit_lm()
            return
        from . import pipeline
        n = self.n
        zst = [np.asarray((z - self.onehot_info[i][1]) / self.onehot_info[i][2] / np.sqrt(self.onehot_info[i][0]))
               for i, z in enumerate(self.Z_list)]                                             # blup.py:786-793
        gnorm, g_scales = _normalize_g(self.G_list)
        klist = [np.asarray(z @ z.T, dtype=float) for z in zst] + gnorm                          # :795
        kdiag = [float(np.diag(k).mean()) for k in klist]
        k_stack = np.stack(klist, axis=0)
        del klist
        fitter = pipeline.MultiKernelReml(k_stack, self.X, self.y.reshape(-1))
        tp = trace_probes_for(n, self.exact_trace)
        theta, result = None, None
        th, ml, reml, nit, converged = jxrs.ai_reml_multi_f64(k_stack, self.X, self.y.reshape(-1), max_iter=int(self.maxiter),
                                                               tol=1e-6, min_var=1e-12, trace_probes=tp, trace_seed=42,
                                                               _fitter=fitter)
        th = np.asarray(th, dtype=float).reshape(-1)
        if th.size == len(kdiag) + 1 and np.all(np.isfinite(th)) and not np.any(th <= 0.0) and bool(converged):   # :537-543
            theta = th
            result = SimpleNamespace(x=th.copy(), success=True, nit=int(nit), message="ai_reml", fun=float(-reml), ml=float(ml),
                                     reml=float(reml), lbd=float(th[-1] / max(1e-12, th[0])))
            self.route = "aireml-exact" if (tp == 0 and n > 768) else "aireml"
        else:
            from scipy.optimize import minimize

            def objective(t):
                t = np.asarray(t, dtype=float).reshape(-1)
                if t.size != len(kdiag) + 1 or not np.all(np.isfinite(t)) or np.any(t <= 0.0):   # :186-191
                    return _OBJ_PENALTY
                prof = fitter.profile(t)
                return _OBJ_PENALTY if prof is None else float(-prof[0])

            theta0 = np.ones(len(kdiag) + 1, dtype=float)                                        # :808
            result = minimize(objective, theta0, method="L-BFGS-B", bounds=[(1e-12, None)] * len(theta0),
                              options={"maxiter": self.maxiter, "ftol": 1e-12, "gtol": 1e-8})      # :819-827
            theta = np.asarray(result.x, dtype=float)
            self.route = "lbfgsb"
        prof = fitter.profile(theta)                                                             # the GLS solve of :834-851
        if prof is None:
            raise RuntimeError("REML optimization failed to produce theta.")
        pc = prof[2]
        beta_hat = np.asarray(pc["beta"], dtype=float).reshape(-1, 1)
        r = np.asarray(pc["r"], dtype=float).reshape(-1, 1)
        vinv_r = np.asarray(pc["vinv_r"], dtype=float).reshape(-1, 1)
        nz, ng = len(zst), len(gnorm)
        z_theta, g_theta = theta[:nz], theta[nz:nz + ng]
        if nz > 0:
            zall = np.concatenate(zst, axis=1)
            gall = np.concatenate([z_theta[i] * np.ones(z.shape[1]) for i, z in enumerate(zst)])
            u_hat = (zall.T @ vinv_r) * gall[:, None]                                            # :863
            z_fitted = zall @ u_hat
            u_by_z, start = [], 0
            for z in zst:
                u_by_z.append(u_hat[start:start + z.shape[1]])
                start += z.shape[1]
        else:
            u_hat, z_fitted, u_by_z = None, np.zeros((n, 1)), []
        g_by_g, g_total = [], np.zeros((n, 1))
        for idx, gk in enumerate(gnorm):
            gi = g_theta[idx] * (gk @ vinv_r)                                                    # :874
            g_by_g.append(gi)
            g_total += gi
        fitted = self.X @ beta_hat + z_fitted + g_total
        sigma2 = float((r.T @ vinv_r)[0, 0]) / max(1, n - self.p)                                # :879
        self._cov_beta = np.asarray(pc["c_inv"], dtype=float) * sigma2                           # :880 (X'V^-1X has full rank here)
        self._z_standardized = True
        self.theta = theta
        self.var = np.array([theta[i] * kdiag[i] for i in range(len(kdiag))] + [theta[-1]])      # :884-887
        self.beta, self.u, self.u_by_Z, self.g, self.g_by_G = beta_hat, u_hat, u_by_z, g_total, g_by_g
        self._Vinvr, self._z_theta, self._g_theta, self._g_scales, self._z_fitted = vinv_r, z_theta, g_theta, g_scales, z_fitted
        self.sigma2, self.reml, self.ml = sigma2, float(prof[0]), float(prof[1])
        self.fitted, self.residuals, self.result = fitted, self.y - fitted, result

    def predict(self, X=None, Z=None, G=None):
        """blup.py:903-1004: X without the intercept column, Z the designs of the training effects, G in-sample (n, n) or the
        cross-kernel (n_pred, n_train) -> (n, 1)."""
        if X is not None:
            n = X.shape[0]
        elif Z is not None:
            if isinstance(Z, np.ndarray):
                n = Z.shape[0]
            elif isinstance(Z, list):
                n = Z[0].shape[0]
            else:
                raise TypeError("Type error of Z matrix")
        elif G is not None:
            if isinstance(G, np.ndarray):
                n = G.shape[0]
            elif isinstance(G, list):
                n = G[0].shape[0]
            else:
                raise TypeError("Type error of G matrix")
        else:
            raise ValueError("Input X or Z for prediction")
        X = _test_x(X, n)
        z_list = _test_z(Z, n) if Z is not None else []
        y_hat = X @ self.beta
        if len(self.Z_list) == 0 and len(self.G_list) == 0:
            return y_hat
        if len(self.Z_list) > 0:
            if len(z_list) > 0:
                if self._z_standardized:
                    z_list = [(z - self.onehot_info[i][1]) / self.onehot_info[i][2] / np.sqrt(self.onehot_info[i][0])
                              for i, z in enumerate(z_list)]
                if len(z_list) != len(self.z_cols):
                    raise ValueError(f"Z count mismatch: expected {len(self.z_cols)}, got {len(z_list)}")
                for idx, (z, expected) in enumerate(zip(z_list, self.z_cols)):
                    if z.shape[1] != expected:
                        raise ValueError(f"Z[{idx}] columns mismatch: expected {expected}, got {z.shape[1]}")
                y_hat = y_hat + np.concatenate(z_list, axis=1) @ self.u
            elif n == self.n and self._z_fitted is not None:
                y_hat = y_hat + self._z_fitted
        if len(self.G_list) > 0:
            if G is None:
                if n == self.n and self.g is not None:
                    y_hat = y_hat + self.g
                else:
                    raise ValueError("G is required for out-of-sample prediction when model has G terms. "
                                     "Provide cross-kernel matrix with shape (n_pred, n_train).")
            else:
                g_pred = _test_g_predict(G, n, self.n)
                if len(g_pred) != self.g_count:
                    raise ValueError(f"G count mismatch: expected {self.g_count}, got {len(g_pred)}")
                g_eff = np.zeros((n, 1))
                for idx, gmat in enumerate(g_pred):
                    g_eff += self._g_theta[idx] * ((np.asarray(gmat, dtype=float) / self._g_scales[idx]) @ self._Vinvr)
                y_hat = y_hat + g_eff
        return y_hat
