"""`jx adamixture` / `jx fastpop` on the host: the -k grammar, the CLI's refusals and range checks, the StdRng seed start and
the torch ALS start (run on the CPU) against a float64 numpy restatement of `als_init_packed_session_impl`."""

import argparse

import numpy as np
import pytest
import torch

from janusx_amd import cli
from janusx_amd import janusx as jx


def _args(*argv):
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli._add_admixture_parser(sub, "adamixture")
    cli._add_admixture_parser(sub, "fastpop")
    return ap.parse_args(list(argv))


@pytest.mark.parametrize("spec,want", [
    ("8", [8]), ("1..4", [1, 2, 3, 4]), ("1:4", [1, 2, 3, 4]), ("1..10..3", [1, 4, 7, 10]), ("1:10:3", [1, 4, 7, 10]),
    ("1..10:3", [1, 4, 7, 10]), ("1,5,8", [1, 5, 8]), ("1..10:3,5,8", [1, 4, 7, 10, 5, 8]), ("4..2", [4, 3, 2]),
    (" 3 , 3,2 ", [3, 2]), ("2..2", [2]), ("10:1:4", [10, 6, 2]),
])
def test_k_spec(spec, want):
    assert cli.parse_k_spec(spec) == want


@pytest.mark.parametrize("spec", ["", "  ", "1;2", "0", "1..", "1..2..3..4", "a", "1:2:0", "0..3", ",", "1:2:3:4"])
def test_k_spec_errors(spec):
    with pytest.raises(ValueError):
        cli.parse_k_spec(spec)


def test_cv_parsing():
    assert _args("adamixture", "-bfile", "x", "-k", "2", "-cv", "0").cv == 0
    assert _args("fastpop", "-bfile", "x", "-k", "2").cv is None
    assert cli._admx_check_args(_args("adamixture", "-bfile", "x", "-k", "2..3", "-cv", "0")) == [2, 3]
    with pytest.raises(SystemExit, match="-cv 5"):
        cli._admx_check_args(_args("adamixture", "-bfile", "x", "-k", "2", "-cv", "5"))
    with pytest.raises(SystemExit, match="-cv 2"):
        cli._admx_check_args(_args("fastpop", "-bfile", "x", "-k", "2", "-cv", "2"))


def test_cli_defaults():
    a = _args("adamixture", "-bfile", "x", "-k", "3")
    assert (a.maf, a.geno, a.seed, a.solver, a.max_iter, a.check, a.tol, a.snps_only) == (0.02, 0.05, 42, "adam-em", 500, 5,
                                                                                           1e-5, False)
    assert _args("adamixture", "-bfile", "x", "-k", "3", "-snps-only").snps_only
    b = _args("fastpop", "-bfile", "x", "-k", "3", "--no-plot", "-tag", "a,b", "-t", "4", "-mem", "8")
    assert cli._admx_check_args(b) == [3]


@pytest.mark.parametrize("argv,msg", [
    (("-vcf", "a.vcf", "-k", "2"), "-vcf"), (("-hmp", "a.hmp", "-k", "2"), "-hmp"), (("-file", "a.txt", "-k", "2"), "-file"),
    (("-k", "2"), "-bfile"), (("-bfile", "x", "-k", "2", "-maf", "0.6"), "-maf"), (("-bfile", "x", "-k", "2", "-maf", "-0.1"), "-maf"),
    (("-bfile", "x", "-k", "2", "-geno", "1.5"), "-geno"), (("-bfile", "x", "-k", "2", "-tol", "0"), "-tol"),
    (("-bfile", "x", "-k", "2", "-max-iter", "0"), "-max-iter"), (("-bfile", "x", "-k", "2", "-check", "0"), "-check"),
    (("-bfile", "x", "-k", "2", "-t", "0"), "-t"), (("-bfile", "x", "-k", "65"), "K=65"), (("-bfile", "x", "-k", "2..70"), "K=65"),
    (("-bfile", "x", "-k", "0"), "K must be >= 1"), (("-bfile", "x", "-k", "1;2"), "Semicolon"),
])
def test_cli_refusals(argv, msg):
    with pytest.raises(SystemExit, match=msg):
        cli._admx_check_args(_args("adamixture", *argv))


def test_cli_refuses_ranks(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU"):
        cli._admx_check_args(_args("fastpop", "-bfile", "x", "-k", "2"))


def test_adam_seed_init_matches_stdrng():
    m, n, k, seed = 7, 5, 3, 42
    rng = jx._StdRngU32(seed)
    u = np.array([rng.next_u32() for _ in range((m + n) * k)], dtype=np.uint64)
    v = np.clip((u >> 8).astype(np.float32) * np.float32(2.0 ** -24), np.float32(1e-5), np.float32(1 - 1e-5))
    p, q = jx.adam_seed_init(m, n, k, seed)
    assert p.dtype == np.float32 and q.dtype == np.float32
    assert np.array_equal(p, v[: m * k].reshape(m, k))
    q0 = v[m * k:].reshape(n, k).astype(np.float32)
    assert np.array_equal(q, q0 / q0.sum(1, keepdims=True, dtype=np.float32))
    assert np.array_equal(jx.adam_seed_init(m, 0, k, seed)[0], p)
    assert not np.array_equal(jx.adam_seed_init(m, n, k, seed + 1)[0], p)


def test_map_helpers():
    q = np.array([[0.2, 0.0, 3.0], [np.nan, 1.0, 1.0], [-1.0, -2.0, -3.0]], dtype=np.float32)
    mq = jx.admx_map_q_f32(q)
    e = np.float32(1e-5)
    r0 = np.clip(q[0], e, 1 - e)
    assert np.allclose(mq[0], r0 / r0.sum())
    assert np.allclose(mq[1], 1.0 / 3.0) and np.allclose(mq[2], 1.0 / 3.0)
    assert np.array_equal(jx.admx_map_p_f32(np.array([[-1.0, 0.5, 2.0]], np.float32)), np.array([[e, 0.5, 1 - e]], np.float32))
    a, b = np.zeros((2, 2), np.float32), np.full((2, 2), 0.5, np.float32)
    assert jx.admx_rmse_f32(a, b) == pytest.approx(0.5)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        jx.admx_rmse_f32(a, np.zeros((3, 2), np.float32))


# ---- ALS start: float64 numpy restatement of `als_init_packed_session_impl` (src/stats/adamixture.rs:4288-4389) ----

def _clip(x):
    return np.clip(x, 1e-5, 1 - 1e-5)


def _map_q(q):
    q = _clip(q)
    s = q.sum(1, keepdims=True)
    bad = ~(np.isfinite(s) & (s > 0))
    return np.where(bad, 1.0 / q.shape[1], q / np.where(bad, 1.0, s))


def _pinv(a):
    ev, v = np.linalg.eigh(a)
    cut = max(np.abs(ev).max() * 1e-12, 1e-12)
    inv = np.where(np.abs(ev) > cut, 1.0 / np.where(np.abs(ev) > cut, ev, 1.0), 0.0)
    return (v * inv) @ v.T


def _rpinv(x, reg):
    return x @ _pinv(x.T @ x + reg * np.eye(x.shape[1]))


def _q_from_p(z, v, f, i_mat):
    return _map_q(0.5 * (v @ (z.T @ i_mat)) + (i_mat * f[:, None]).sum(0))


def _als_ref(z, v, f, p0, max_iter, tol, reg):
    p = p0.copy()
    q = _q_from_p(z, v, f, _rpinv(p, reg))
    q_prev = q.copy()
    best, stall, hc, pb, qb, last = np.inf, 0, False, None, None, 0
    for it in range(max_iter):
        last = it + 1
        iq = _rpinv(q, reg)
        p = _clip(0.5 * (z @ (v.T @ iq)) + f[:, None] * iq.sum(0)[None, :])
        g = p.T @ p
        q = _q_from_p(z, v, f, p @ _pinv(g + reg * np.eye(g.shape[0])))
        err = np.sqrt(np.mean((q - q_prev) ** 2))
        if not hc:
            sd = np.sqrt(np.maximum(np.diag(g), 1e-12))
            c = np.abs(g / np.maximum(np.outer(sd, sd), 1e-10))
            np.fill_diagonal(c, 0.0)
            hc = c.max() > 0.95
        if hc:
            if err < best:
                best, pb, qb, stall = err, p.copy(), q.copy(), 0
            else:
                stall += 1
            if stall >= 20:
                p, q = pb, qb
                break
        if err < tol:
            break
        q_prev = q.copy()
    return p, q, last


def _als_problem(m, n, k, seed, collinear=False):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, m)
    lab = rng.integers(0, k, n)
    pt = np.clip(f[:, None] + rng.normal(0, 0.15, (m, k)), 0.01, 0.99)
    g = rng.binomial(2, pt[:, lab]).astype(np.float64)
    zc = g - 2.0 * f[:, None]
    u, s, vt = np.linalg.svd(zc, full_matrices=False)
    v = vt[:k].T
    z = zc @ v
    if collinear:
        z *= 1e-3            # a weak structure: P's columns lean on row_freq alone, max |corr| > 0.95
    return z, v, f, jx.adam_seed_init(m, 0, k, 42)[0].astype(np.float64)


def test_als_converges_like_restatement():
    z, v, f, p0 = _als_problem(300, 120, 3, 1)
    tol = 1e-4
    pr, qr, itr = _als_ref(z, v, f, p0, 1000, tol, 1e-5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    calls = []
    p, q, ll, it = jx.admx_als_init(t(z), t(v), t(f), t(p0), 1000, tol, 1e-5, loglik=lambda a, b: calls.append(1) or -1.0)
    assert it == itr and it < 1000
    assert ll == -1.0 and calls == [1]
    assert np.allclose(p.numpy(), pr, atol=1e-9) and np.allclose(q.numpy(), qr, atol=1e-9)
    assert np.allclose(q.numpy().sum(1), 1.0)


def test_als_stall_rolls_back_like_restatement():
    z, v, f, p0 = _als_problem(300, 120, 3, 1, collinear=True)
    pr, qr, itr = _als_ref(z, v, f, p0, 400, 0.0, 1e-5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    p, q, ll, it = jx.admx_als_init(t(z), t(v), t(f), t(p0), 400, 0.0, 1e-5)
    assert np.isnan(ll)
    assert itr < 400 and it < 400                      # the stall branch ended both loops, not max_iter
    assert it == itr
    assert np.allclose(p.numpy(), pr, atol=1e-9) and np.allclose(q.numpy(), qr, atol=1e-9)


# ---- the slicing of the EM pass and its work buffer (`ax_grid`, `ax_work_bytes`, csrc/k_admx.hip), restated ----

AX_CAP = 8 << 30


def _ax_grid(nrows, n, k):
    """`ax_grid` of csrc/k_admx.hip restated (tests/test_gpu_admx.py imports this copy)
    -> (s1, s2, gps, tps): SNP slices, sample slices, groups of 32 rows per slice, 128-sample tiles per slice."""
    ngroups, ntiles = (nrows + 31) // 32, (n + 127) // 128
    s1 = min(ngroups, 256)
    s2 = max(1, min(2048 // max(s1, 1), ntiles))
    s1 = max(s1, 1)
    while True:
        pa, pt = 8 * k * s2 * nrows, 4 * k * s1 * n
        if pa + pt <= AX_CAP or (s1 == 1 and s2 == 1):
            break
        if (pt >= pa and s1 > 1) or s2 == 1:
            s1 = (s1 + 1) // 2
        else:
            s2 = (s2 + 1) // 2
    gps = (ngroups + s1 - 1) // s1
    tps = (ntiles + s2 - 1) // s2
    return max((ngroups + gps - 1) // gps, 1), (ntiles + tps - 1) // tps, gps, tps


def _ax_work_bytes(nrows, n, k):
    if not (1 <= k <= 64 and n >= 1 and nrows >= 1):
        return 0
    s1, s2, _gps, _tps = _ax_grid(nrows, n, k)
    al = lambda b: (b + 255) & ~255
    return 2 * al(4 * k * s2 * nrows) + al(4 * k * s1 * n) + al(4 * k * n) + al(8 * s1 * s2) + al(4 * n)


_AX_SHAPES = [(1, 1), (31, 100), (32, 128), (33, 129), (64, 256), (420, 300), (8200, 1100), (8192, 32768), (65536, 300),
              (10 ** 6, 200_000), (10 ** 6, 2_000_000), (3 * 10 ** 7, 5000), (5 * 10 ** 7, 1 << 23), (100, 1 << 23),
              (4 * 10 ** 6, 1_000_000), (250_000, 4_000_000)]
_AX_K = [1, 2, 3, 4, 5, 8, 10, 16, 17, 32, 33, 63, 64]


def test_work_bytes_match_the_restated_grid():
    from janusx_amd._lib import lib
    capped = 0
    for nrows, n in _AX_SHAPES:
        for k in _AX_K:
            if k > n:
                continue
            assert lib().jxg_admx_work_bytes(nrows, n, k) == _ax_work_bytes(nrows, n, k), (nrows, n, k)
            s1, s2, gps, tps = _ax_grid(nrows, n, k)
            ngroups, ntiles = (nrows + 31) // 32, (n + 127) // 128
            # the slices cover every group and tile, and none is empty
            assert s1 * gps >= ngroups > (s1 - 1) * gps and s2 * tps >= ntiles > (s2 - 1) * tps, (nrows, n, k)
            part = 4 * k * (2 * s2 * nrows + s1 * n)
            assert part <= AX_CAP or (s1 == 1 and s2 == 1), (nrows, n, k, part)
            full = 4 * k * (2 * min(ntiles, max(1, 2048 // min(ngroups, 256))) * nrows + min(ngroups, 256) * n)
            capped += full > AX_CAP
    assert 10 <= capped < len(_AX_SHAPES) * len(_AX_K) - 10         # shapes on both sides of the cap
    for bad in ((100, 100, 0), (100, 100, 65), (100, 0, 4), (0, 100, 4), (100, 100, -1), (-5, 100, 4)):
        assert lib().jxg_admx_work_bytes(*bad) == 0 == _ax_work_bytes(*bad), bad


def test_design_figures_of_the_partial_memory():
    """configs[4] (n = 200 000, 10^6 rows) takes 1.08 / 2.69 / 4.30 GB at K = 4 / 10 / 16, and the partial sums stay
    within 8 GiB at K = 64 (where the slices are halved to fit)."""
    from janusx_amd._lib import lib
    n, m = 200_000, 10 ** 6
    for k, gb in ((4, "1.08"), (10, "2.69"), (16, "4.30")):
        assert f"{lib().jxg_admx_work_bytes(m, n, k) / 1e9:.2f}" == gb
        assert _ax_grid(m, n, k)[:2] == (255, 8)
    s1, s2, _gps, _tps = _ax_grid(m, n, 64)
    assert (s1, s2) != (255, 8) and 4 * 64 * (2 * s2 * m + s1 * n) <= AX_CAP
    assert 2048 >= s1 * s2 >= 256                                  # still hundreds of workgroups after the halving
