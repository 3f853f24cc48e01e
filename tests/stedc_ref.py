"""Designed symmetric tridiagonal matrices for the divide and conquer (csrc/k_stedc.hip) and the checks that go with them.

Every design yields (d, e): the diagonal (n) and the off-diagonal (n - 1).  They are the classical hard cases of Cuppen's method,
none of which a dense `Q diag(s) Q'` with a random Q can put in front of the merges:

    toeplitz    d = 2, e = -1: lambda_k = 2 - 2 cos(k pi / (n + 1)); nothing deflates (K = n at every merge), every tear negative
    clement     d = 0, e_k = sqrt(k (n - k)): lambda = -(n - 1), -(n - 3), .., n - 1
    wilkinson   d_i = |i - (n - 1) / 2|, e = 1 (W+ for odd n): the top pairs agree to machine precision, so the close-pair
                rotations act across the two halves (the side buffer)
    glued       copies of W+_m joined by a small off-diagonal entry
    graded      d_i = 10^(-16 i / n), e_i = 0.1 sqrt(d_i d_(i+1))
    ones_tiny   d = 1, e = 1e-10: close-pair deflation everywhere
    two_roots   d sorted uniform(0.5, 2), e = 0 but for e[n/2 - 1] = 0.3: both halves diagonal, K = 2 at the top merge
    one_root    d = 0 .. n-1, e = 0 but for e[k - 1] = 0.25 at k = n / 2 with d[k - 1] = d[k] = 5.25: after the tear the two poles
                are equal, they rotate together and K = 1
    zero_tears  d, e normal; e[n/2 - 1] = 0, e[n/4 - 1] = 1e-300, e[3 (n/4)] = -1e-18: tears that vanish at several levels
    negative    d normal, e = -|normal|

A case is (design, size argument(s), k): the design multiplied by 2^k (exact in f64).

Scale of every bar: ||T|| := max|d| + 2 max|e| (a bound of the spectral radius).  The three measured quantities of a solution
(w, Z), Z row-major with one eigenvector per row:
    ev    max|w - lambda_ref| / ||T||
    orth  max|Z Z' - I|
    res   max|T Z' - Z' diag(w)| / ||T||
Hard bars (those of test_eigh_own_divide_and_conquer with ||T|| instead of max(1, .) as the scale): ev < 1e-12 sqrt(n),
orth < 1e-11, res < 1e-11.  lambda_ref is the closed form for toeplitz and clement, LAPACK's bisection (dstebz) otherwise.
"""
import functools

import numpy as np

EPS = 2.220446049250313e-16
EV_BAR, ORTH_BAR, RES_BAR = 1e-12, 1e-11, 1e-11
REL_FACTOR = 16.0              # over LAPACK's own value for the same T (floored at 8 eps), at the sizes that stay on the f64 GEMM
REL_FLOOR = 8.0 * EPS
SIZES_F64 = (129, 130, 254, 256, 611, 1023)     # leaves 64 + 65, 65 + 65, 127 + 127, 128 + 128; every merge on the f64 GEMM
SIZE_OZ = 2100                                  # halves of 1050: the top merge can take the sliced int8 product
SCALE_EXPONENTS = (-40, -200, 40)


def toeplitz(n):
    return np.full(n, 2.0), np.full(n - 1, -1.0)


def toeplitz_eigenvalues(n):
    return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


def clement(n):
    k = np.arange(1, n, dtype=np.float64)
    return np.zeros(n), np.sqrt(k * (n - k))


def clement_eigenvalues(n):
    return np.arange(-(n - 1), n, 2, dtype=np.float64)


def wilkinson(n):
    return np.abs(np.arange(n, dtype=np.float64) - (n - 1) / 2.0), np.ones(n - 1)


def glued(m, copies, glue):
    d1, e1 = wilkinson(m)
    d = np.tile(d1, copies)
    e = np.tile(np.concatenate([e1, [glue]]), copies)[:-1]
    return d, e


def graded(n):
    d = 10.0 ** (-16.0 * np.arange(n) / n)
    return d, 0.1 * np.sqrt(d[:-1] * d[1:])


def ones_tiny(n):
    return np.ones(n), np.full(n - 1, 1e-10)


def two_roots(n):
    d = np.sort(np.random.default_rng(7100 + n).uniform(0.5, 2.0, n))
    e = np.zeros(n - 1)
    e[n // 2 - 1] = 0.3
    return d, e


def one_root(n):
    k = n // 2
    d = np.arange(n, dtype=np.float64)
    e = np.zeros(n - 1)
    e[k - 1] = 0.25
    d[k - 1] = d[k] = 5.25
    return d, e


def zero_tears(n):
    rng = np.random.default_rng(7200 + n)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    e[n // 2 - 1] = 0.0
    e[n // 4 - 1] = 1e-300
    e[3 * (n // 4)] = -1e-18
    return d, e


def negative(n):
    rng = np.random.default_rng(7300 + n)
    return rng.standard_normal(n), -np.abs(rng.standard_normal(n - 1))


DESIGNS = {"toeplitz": toeplitz, "clement": clement, "wilkinson": wilkinson, "glued": glued, "graded": graded,
           "ones_tiny": ones_tiny, "two_roots": two_roots, "one_root": one_root, "zero_tears": zero_tears, "negative": negative}
CLOSED_FORM = {"toeplitz": toeplitz_eigenvalues, "clement": clement_eigenvalues}


def _cases():
    out = []
    for name in ("toeplitz", "clement", "zero_tears"):
        out += [(name, (n,), 0) for n in SIZES_F64 + (SIZE_OZ,)]
    for name in ("graded", "ones_tiny", "two_roots", "one_root", "negative"):
        out += [(name, (n,), 0) for n in SIZES_F64]
    out += [("wilkinson", (257,), 0), ("wilkinson", (2049,), 0)]
    out += [("glued", (21, 100, 1e-8), 0), ("glued", (21, 100, 1e-14), 0), ("glued", (257, 8, 1e-10), 0)]
    for k in SCALE_EXPONENTS:
        out += [("toeplitz", (611,), k), ("toeplitz", (SIZE_OZ,), k), ("wilkinson", (257,), k), ("wilkinson", (2049,), k),
                ("negative", (611,), k), ("negative", (SIZE_OZ,), k)]
    return out


CASES = _cases()


def case_id(case):
    name, args, k = case
    tag = name + "-" + "x".join(f"{a:g}" for a in args)
    return tag if k == 0 else f"{tag}*2^{k}"


def matrix(case):
    """(d, e) of a case, fresh arrays"""
    name, args, k = case
    d, e = DESIGNS[name](*args)
    return np.ldexp(d, k), np.ldexp(e, k)


def tnorm(d, e):
    return float(np.max(np.abs(d)) + 2.0 * np.max(np.abs(e)))


def dense(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


@functools.lru_cache(maxsize=None)
def _reference_eigenvalues_unscaled(name, args):
    if name in CLOSED_FORM:
        return CLOSED_FORM[name](*args)
    from scipy.linalg import eigvalsh_tridiagonal
    d, e = DESIGNS[name](*args)
    return eigvalsh_tridiagonal(d, e, lapack_driver="stebz")


def reference_eigenvalues(case):
    """Closed form or bisection for the unscaled design, times 2^k (exact: the eigenvalues of 2^k T are 2^k times those of T)."""
    name, args, k = case
    return np.ldexp(_reference_eigenvalues_unscaled(name, args), k)


def measure(d, e, w, z, lam_ref):
    """(ev, orth, res) of the solution (w, Z row-major) of T = tridiag(d, e), in the units of the module docstring"""
    n = len(d)
    t = tnorm(d, e)
    ev = float(np.max(np.abs(w - lam_ref))) / t
    orth = float(np.max(np.abs(z @ z.T - np.eye(n))))
    # row r of Z T = (T z_r)': tridiagonal, formed without a dense T
    tz = z * d
    tz[:, :-1] += z[:, 1:] * e
    tz[:, 1:] += z[:, :-1] * e
    res = float(np.max(np.abs(tz - z * w[:, None]))) / t
    return ev, orth, res


def hard_bars(n):
    return EV_BAR * n ** 0.5, ORTH_BAR, RES_BAR


@functools.lru_cache(maxsize=None)
def lapack_measures(case):
    """(ev, orth, res) of numpy.linalg.eigh (LAPACK dsyevd) on the dense T of the case"""
    d, e = matrix(case)
    w, v = np.linalg.eigh(dense(d, e))
    return measure(d, e, w, np.ascontiguousarray(v.T), reference_eigenvalues(case))
