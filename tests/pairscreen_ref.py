"""numpy / Fraction restatement of the SNP-pair screen (`jx fvlmm2 -screen`; csrc/k_pairscreen.hip, janusx.fvlmm2_screen_packed),
written from the definition, not from the kernel:

  * the digit split of r: S = 2^e the smallest power of two >= max |r|, q1 = rint(64 r / S), q2 = rint(128 (64 r / S - q1)), ... four
    signed radix-128 digits, |q| <= 64; a sample's integer is ((q1 128 + q2) 128 + q3) 128 + q4, in units of scale = S 2^-27;
  * the class tables of a pair by direct counting over decoded codes (00 -> 0, 10 -> 1, 11 -> 2; 01 belongs to no class):
    N_ab counts, R_ab sums of the samples' integers;
  * the score statistic of the combo term given intercept and both literals, evaluated in f64 in the written order (a major, b
    minor) and exactly with `fractions.Fraction` from the integer tables;
  * hit selection and the sort (stat descending, row1, row2, variant).

STAT_F64_ERR is the largest difference between the f64 and the exact evaluation that tests/test_fvlmm2_screen_host.py finds on
random small tables, in the norm |T64 - T| / max(T, 1) (see `stat_error`); the device sums in another but fixed order, so the GPU
tests allow 8 times that."""
import math
from fractions import Fraction

import numpy as np

MIN_COMPLETE = 5
DEN_REL = 1e-10
STAT_F64_ERR = 2.3e-14    # measured: 2.298e-14 (test_fvlmm2_screen_host.py::test_f64_restatement_against_the_rational_one)
STAT_TOL_FACTOR = 8.0


def decode_classes(packed, n, sample_indices=None):
    """(m, ceil(n / 4)) uint8 payload -> (m, n_sel) int8 classes, -1 at a missing call."""
    packed = np.asarray(packed, dtype=np.uint8)
    codes = np.stack([(packed >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(packed.shape[0], -1)[:, :n]
    cls = np.array([0, -1, 1, 2], dtype=np.int8)[codes]
    return cls if sample_indices is None else cls[:, np.asarray(sample_indices, dtype=np.int64)]


def digit_split(r):
    """-> (digits (4, n) int64, scale = S 2^-27, units (n) int64 = the integer every sample enters the sums with)."""
    r = np.asarray(r, dtype=np.float64)
    mx = float(np.max(np.abs(r))) if r.size else 0.0
    e = 0
    if mx > 0.0 and math.isfinite(mx):
        f, e = math.frexp(mx)
        if f == 0.5:
            e -= 1
    a = np.ldexp(r, 6 - e)
    digits = np.empty((4, r.shape[0]), dtype=np.int64)
    for p in range(4):
        q = np.rint(a)
        digits[p] = q.astype(np.int64)
        a = (a - q) * 128.0
    assert np.abs(digits).max(initial=0) <= 64
    units = ((digits[0] * 128 + digits[1]) * 128 + digits[2]) * 128 + digits[3]
    return digits, math.ldexp(1.0, e - 27), units


def class_tables(cls_i, cls_j, units):
    """cls_i (Ri, n), cls_j (Rj, n) classes, units (n) int64 -> N (Ri, Rj, 3, 3) int32, R (Ri, Rj, 3, 3) int64."""
    ri, rj = cls_i.shape[0], cls_j.shape[0]
    out_n = np.zeros((ri, rj, 3, 3), dtype=np.int32)
    out_r = np.zeros((ri, rj, 3, 3), dtype=np.int64)
    u = np.asarray(units, dtype=np.int64)
    for a in range(3):
        ia = (cls_i == a)
        for b in range(3):
            jb = (cls_j == b)
            out_n[:, :, a, b] = ia.astype(np.int64) @ jb.astype(np.int64).T
            out_r[:, :, a, b] = (ia * u[None, :]).astype(np.int64) @ jb.astype(np.int64).T
    return out_n, out_r


def _moments(nt, rt, var, fi, fj):
    """The fourteen sums in the written order (a major, b minor); works on floats, ints and Fractions alike."""
    zero = nt[0][0] * 0
    n = s1 = s2 = s11 = s12 = s22 = c0 = c1 = c2 = cc = zero
    r0 = r1 = r2 = cr = rt[0][0] * 0
    for a in range(3):
        pa = 2 - a if fi else a
        x1 = var[9 + pa]
        for b in range(3):
            pb = 2 - b if fj else b
            x2, xc = var[12 + pb], var[3 * pa + pb]
            w, rr = nt[a][b], rt[a][b]
            n = n + w
            s1 = s1 + w * x1
            s2 = s2 + w * x2
            s11 = s11 + w * (x1 * x1)
            s12 = s12 + w * (x1 * x2)
            s22 = s22 + w * (x2 * x2)
            c0 = c0 + w * xc
            c1 = c1 + w * (x1 * xc)
            c2 = c2 + w * (x2 * xc)
            cc = cc + w * (xc * xc)
            r0 = r0 + rr
            r1 = r1 + rr * x1
            r2 = r2 + rr * x2
            cr = cr + rr * xc
    return n, s1, s2, s11, s12, s22, c0, c1, c2, cc, r0, r1, r2, cr


def _solve(mom, sigma2, den_rel, div):
    n, s1, s2, s11, s12, s22, c0, c1, c2, cc, r0, r1, r2, cr = mom
    if not n >= MIN_COMPLETE:
        return None
    d11, d12, d22 = n * s11 - s1 * s1, n * s12 - s1 * s2, n * s22 - s2 * s2
    if not d11 > 0:
        return None
    det = d11 * d22 - d12 * d12
    if not det > 0:
        return None
    e1, e2, f1, f2 = n * c1 - s1 * c0, n * c2 - s2 * c0, n * r1 - s1 * r0, n * r2 - s2 * r0
    ecc, ecr = n * cc - c0 * c0, n * cr - c0 * r0
    b1, b2 = div(e1 * d22 - e2 * d12, det), div(e2 * d11 - e1 * d12, det)
    den, num = div(ecc - b1 * e1 - b2 * e2, n), div(ecr - b1 * f1 - b2 * f2, n)
    if not den > den_rel * cc:
        return None
    return div(num * num, sigma2 * den)


def stat_f64(n_tab, r_tab, scale, var, fi, fj, sigma2):
    """f64 in the written order; NaN where void.  n_tab, r_tab (3, 3) integers; var (15) f64: combo (9), lit1 (3), lit2 (3)."""
    nt = [[float(n_tab[a][b]) for b in range(3)] for a in range(3)]
    rt = [[float(int(r_tab[a][b])) * float(scale) for b in range(3)] for a in range(3)]
    t = _solve(_moments(nt, rt, [float(x) for x in var], fi, fj), float(sigma2), DEN_REL, lambda x, y: x / y)
    return math.nan if t is None else t


def stat_exact(n_tab, r_tab, scale, var, fi, fj, sigma2):
    """The same statistic as a Fraction from the integer tables; None where void."""
    nt = [[int(n_tab[a][b]) for b in range(3)] for a in range(3)]
    rt = [[int(r_tab[a][b]) * Fraction(float(scale)) for b in range(3)] for a in range(3)]
    vals = [Fraction(float(x)) for x in var]
    vals = [int(x) if x.denominator == 1 else x for x in vals]
    return _solve(_moments(nt, rt, vals, fi, fj), Fraction(float(sigma2)), Fraction(DEN_REL), lambda x, y: Fraction(x) / Fraction(y))


def stat_error(got, exact):
    """|got - exact| / max(exact, 1): relative where the statistic is large, absolute below 1.  T = num^2 / (sigma2 den) with num a
    difference of sums much larger than itself: its rounding error is absolute, e K with K the size of the sums, so the error of T
    is ~ 2 sqrt(T) e K / sqrt(sigma2 den): bounded relative to T for T >= 1 and absolutely for T < 1, unbounded relative to a T -> 0."""
    return abs(float(got) - float(exact)) / max(float(exact), 1.0)


def screen(classes, flip, units, scale, sigma2, variants, t_min, rows=None, chrom_id=None, pos=None, min_dist=0, exact=True):
    """All pairs row1 < row2 of `rows` -> (dense dict {(row1, row2, v): T float or None}, sorted hit list of (row1, row2, v, T, n_complete),
    pairs_screened).  T from the exact evaluation (exact=True) or the f64 one."""
    m = classes.shape[0]
    lst = np.arange(m) if rows is None else np.unique(np.asarray(rows, dtype=np.int64))
    n_tab, r_tab = class_tables(classes[lst], classes[lst], units)
    dense, hits, screened = {}, [], 0
    for x in range(len(lst)):
        for y in range(x + 1, len(lst)):
            i, j = int(lst[x]), int(lst[y])
            if min_dist > 0 and chrom_id[i] == chrom_id[j] and abs(int(pos[i]) - int(pos[j])) < min_dist:
                continue
            screened += 1
            nc = int(n_tab[x, y].sum())
            for v, var in enumerate(variants):
                if exact:
                    t = stat_exact(n_tab[x, y], r_tab[x, y], scale, var, bool(flip[i]), bool(flip[j]), sigma2)
                    t = None if t is None else float(t)
                else:
                    t = stat_f64(n_tab[x, y], r_tab[x, y], scale, var, bool(flip[i]), bool(flip[j]), sigma2)
                    t = None if math.isnan(t) else t
                dense[(i, j, v)] = t
                if t is not None and t >= t_min:
                    hits.append((i, j, v, t, nc))
    hits.sort(key=lambda h: (-h[3], h[0], h[1], h[2]))
    return dense, hits, screened


STAT_TOL = STAT_TOL_FACTOR * STAT_F64_ERR        # 1.84e-13: the GPU statistic against the rational one
