"""`jx pca` and the randomized SVD of packed genotypes (`rsvd_packed_subset`, `admx_rsvd_stream_sample`, the two skinny
products `jxg_packed_mm_cols` / `jxg_packed_tmm_cols`) against float64 numpy restatements in this file."""

import numpy as np
import pytest

from janusx_amd import bed

pytestmark = pytest.mark.gpu

N, M = 2000, 20000


def _panel_dosage(n=N, m=M, miss=0.01, seed=7):
    """Four subpopulations with distinct allele frequencies (three leading eigenvalues clear of the bulk), `miss` missing."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 0.9, m)
    pops = np.clip(base[None, :] + rng.normal(0.0, 0.15, (4, m)), 0.05, 0.95)
    lab = np.arange(n) % 4
    g = rng.binomial(2, pops[lab].T).astype(np.int8)            # (m, n)
    if miss > 0:
        g[rng.random(g.shape) < miss] = -1
    return g


_CACHE = {}


def _data():
    if "g" not in _CACHE:
        g = _panel_dosage()
        _CACHE["g"] = g
        _CACHE["packed"] = bed.pack_dosage(g)
    return _CACHE["g"], _CACHE["packed"]


def _design(g):
    """Centred design of `packed_subset_row_stats` + `prepare_packed_block_centered_mean_scale_f32` (missing -> 0):
    -> Z (m, n) f64, maf f32, flip, varsum."""
    called = g >= 0
    nm = called.sum(1)
    alt = np.where(called, g, 0).sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(nm > 0, alt / (2.0 * np.maximum(nm, 1)), 0.0)
    flip = (nm > 0) & (p > 0.5)
    pm = np.where(flip, 1.0 - p, p)
    maf = pm.astype(np.float32)
    mean = (np.float32(2.0) * maf).astype(np.float64)
    gg = np.where(flip[:, None], 2.0 - g, g.astype(np.float64))
    z = np.where(called, gg - mean[:, None], 0.0)
    varsum = float(np.sum(np.where(nm > 0, 2.0 * pm * (1.0 - pm), 0.0)))
    return z, maf, flip, varsum


def _mgs(x):
    q = np.zeros_like(x)
    for j in range(x.shape[1]):
        v = x[:, j].copy()
        for i in range(j):
            v -= (q[:, i] @ v) * q[:, i]
        nrm = np.sqrt(v @ v)
        assert nrm > 1e-12
        q[:, j] = v / nrm
    return q


def _lu(x, eps=1e-10, ratio=1e-8):
    rows, cols = x.shape
    if rows < cols:
        return _mgs(x), False
    a = x.copy()
    piv = np.arange(rows)
    d = []
    for j in range(cols):
        pr = j + int(np.argmax(np.abs(a[j:, j])))
        if not abs(a[pr, j]) > eps:
            return _mgs(x), False
        if pr != j:
            a[[j, pr]] = a[[pr, j]]
            piv[[j, pr]] = piv[[pr, j]]
        d.append(abs(a[j, j]))
        a[j + 1:, j] /= a[j, j]
        a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j, j + 1:])
    if min(d) / max(d) < ratio:
        return _mgs(x), False
    lo = np.tril(a[:, :cols], -1)
    lo[np.arange(cols), np.arange(cols)] = 1.0
    q = np.empty_like(lo)
    q[piv] = lo
    return q / np.linalg.norm(q, axis=0)[None, :], True


def _rsvd_ref(z, varsum, k, seed, power, tol, mode, kp):
    """float64 restatement of rsvd.rs:1548-1661 (mode "lu") / adamixture.rs:3527-3720 (mode "svd") with the product's Omega."""
    from janusx_amd.janusx import rsvd_omega
    n = z.shape[1]
    k_eff = min(k, n, kp)
    y = z.T @ rsvd_omega(seed, z.shape[0], kp)
    q = _mgs(y) if mode == "lu" else np.linalg.svd(y, full_matrices=False)[0]
    sk = np.zeros(kp)
    alpha, q_is_qr, rounds = 0.0, True, 0
    for it in range(power):
        y = z.T @ (z @ q) - alpha * q
        if mode == "lu":
            if it + 1 >= power:
                q, q_is_qr = _mgs(y), True
            else:
                q, used = _lu(y)
                q_is_qr = not used
            s_y = np.sort(np.linalg.norm(y, axis=0))[::-1]
        else:
            u, s_y, _ = np.linalg.svd(y, full_matrices=False)
            q = u
        rounds = it + 1
        if it > 0:
            now = s_y[:k_eff] + alpha
            rel = np.abs(now - sk[:k_eff]) / np.maximum(now, 1e-12)
            sk[:k_eff] = now
            if rel.max() < tol:
                if mode == "lu" and not q_is_qr:
                    q, q_is_qr = _mgs(q), True
                break
        else:
            sk[:] = s_y + alpha
        if alpha < s_y[kp - 1]:
            alpha = 0.5 * (alpha + s_y[kp - 1])
    if mode == "lu" and not q_is_qr:
        q = _mgs(q)
    w = z @ q
    ev, v = np.linalg.eigh(w.T @ w)
    o = np.argsort(-ev)
    ev, v = np.maximum(ev[o], 1e-12), v[:, o]
    return ev[:k_eff] / varsum, q @ v[:, :k_eff], rounds


def _align(a, b):
    """b's columns sign-aligned to a's."""
    s = np.sign(np.sum(a * b, axis=0))
    s[s == 0] = 1.0
    return b * s[None, :]


def _exact(z, varsum, k):
    kk = z.T @ z / varsum
    ev, v = np.linalg.eigh(kk)
    return ev[::-1][:k], v[:, ::-1][:, :k], float(np.trace(kk))


def test_products_match_numpy_for_several_widths():
    import torch
    from janusx_amd import pipeline as pl
    from janusx_amd._lib import check, lib
    from janusx_amd.janusx import _rsvd_row_design
    rng = np.random.default_rng(3)
    n, m = 700, 900
    g = _panel_dosage(n, m, 0.02, seed=11)
    g[5] = 0
    g[6] = -1                                                     # monomorphic and all-missing rows
    z, maf, flip, _ = _design(g)
    dev = torch.device("cuda", 0)
    panel = pl.Panel(torch.from_numpy(bed.pack_dosage(g)).to(dev), n)
    rows = rng.permutation(m)[:777].astype(np.int32)
    ab = torch.from_numpy(_rsvd_row_design(maf[rows], flip[rows])).to(dev)
    rows_t = torch.from_numpy(rows).to(dev)
    zr = z[rows]
    t32 = torch.empty(int(lib().jxg_t32_bytes(n, len(rows))), dtype=torch.uint8, device=dev)
    check(lib().jxg_p32_transpose(panel.p32.data_ptr(), m, n, rows_t.data_ptr(), len(rows), t32.data_ptr(), pl._stream()))
    for kp in (1, 5, 16, 33, 64):
        q = rng.standard_normal((n, kp)) * np.logspace(0, 3, kp)[None, :]
        w = torch.empty((len(rows), kp), dtype=torch.float64, device=dev)
        check(lib().jxg_packed_mm_cols(panel.p32.data_ptr(), m, n, rows_t.data_ptr(), len(rows), ab.data_ptr(),
                                       torch.from_numpy(q).to(dev).data_ptr(), kp, w.data_ptr(), pl._stream()))
        ref = zr @ q
        err = np.abs(w.cpu().numpy() - ref) / np.abs(ref).max(axis=0)[None, :]
        assert err.max() <= 1e-6, kp
        wt = rng.standard_normal((len(rows), kp))
        y = torch.empty((n, kp), dtype=torch.float64, device=dev)
        check(lib().jxg_packed_tmm_cols(t32.data_ptr(), n, len(rows), ab.data_ptr(), torch.from_numpy(wt).to(dev).data_ptr(),
                                        kp, y.data_ptr(), pl._stream()))
        ref = zr.T @ wt
        err = np.abs(y.cpu().numpy() - ref) / np.abs(ref).max(axis=0)[None, :]
        assert err.max() <= 1e-6, kp


def test_rsvd_packed_subset_parity_with_restatement():
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    z, maf, flip, varsum = _design(g)
    ev, vec, maf_o, flip_o, rounds = jxrs._rsvd_packed_subset(packed, N, 5, None, 42, 5, 0.1)
    np.testing.assert_array_equal(maf_o, maf)
    np.testing.assert_array_equal(flip_o, flip)
    rev, rvec, rr = _rsvd_ref(z, varsum, 5, 42, 5, np.float32(0.1), "lu", 20)
    assert rounds == rr
    assert np.max(np.abs(ev - rev) / rev) < 1e-5
    assert np.abs(_align(rvec, vec) - rvec).max() < 1e-4


def test_admx_rsvd_parity_with_restatement(tmp_path):
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    g = g.copy()
    g[:50] = np.where(g[:50] >= 0, 0, g[:50])                     # rare rows that the maf filter drops
    prefix = str(tmp_path / "p")
    m = g.shape[0]
    bim = bed.Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * (m - 7) + ["AT"] * 7, ["G"] * m)
    bed.write_bed(prefix, bed.pack_dosage(g), [f"s{i}" for i in range(N)], bim)
    ev, vec, tv, rounds = jxrs._admx_rsvd(prefix, 4, 42, 5, 0.1, True, 0.02, 0.05)
    called = g >= 0
    miss = 1.0 - called.mean(1)
    alt = np.where(called, g, 0).sum(1) / (2.0 * np.maximum(called.sum(1), 1))
    keep = (np.minimum(alt, 1 - alt) >= 0.02) & (miss <= 0.05)
    keep[m - 7:] = False
    z, _maf, _flip, _ = _design(g[keep])
    f = _maf.astype(np.float64)
    varsum = float(np.sum(2.0 * f * (1.0 - f)))
    rev, rvec, rr = _rsvd_ref(z, varsum, 4, 42, 5, np.float32(0.1), "svd", 12)
    assert rounds == rr
    assert np.max(np.abs(ev - rev) / rev) < 1e-5
    assert np.abs(_align(rvec, vec) - rvec).max() < 1e-4
    assert abs(tv - float(np.sum(z * z)) / varsum) < 1e-9 * tv


def test_converged_accuracy_and_defaults():
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    z, _maf, _flip, varsum = _design(g)
    eev, evec, _tr = _exact(z, varsum, 5)
    ev, vec, *_ = jxrs.rsvd_packed_subset(packed, N, 5, seed=42, power=30, tol=1e-7)
    # components 4 and 5 sit in the bulk (1.62, 1.61: not separated); the shift alpha of the method moves towards the tail of the
    # spectrum, where the centring null vector (eigenvalue 0) competes with the bulk edge, so only the three separated
    # components converge to the exact eigenpairs -- the restatement above (same control flow) reaches the same values
    assert np.max(np.abs(ev[:3] - eev[:3]) / eev[:3]) < 1e-5
    cos = np.abs(np.sum(vec.astype(np.float64) * evec, axis=0)) / np.linalg.norm(vec.astype(np.float64), axis=0)
    assert np.all(cos[:3] >= 1 - 1e-6), cos
    ev3, vec3, *_ = jxrs.rsvd_packed_subset(packed, N, 3, seed=42, power=3, tol=0.1)
    qa = np.linalg.qr(vec3.astype(np.float64))[0]
    sv = np.linalg.svd(qa.T @ evec[:, :3], compute_uv=False)
    assert sv.min() >= 0.999, sv
    assert np.max(np.abs(ev3 - eev[:3]) / eev[:3]) < 0.01


def test_invariances():
    import torch
    from janusx_amd import janusx as jxrs
    g, packed = _data()
    a = jxrs.rsvd_packed_subset(packed, N, 5)
    b = jxrs.rsvd_packed_subset(packed, N, 5)
    c = jxrs.rsvd_packed_subset(torch.from_numpy(packed).cuda(), N, 5)
    for x, y in ((a, b), (a, c)):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    idx = np.random.default_rng(5).permutation(N)[:1500]
    s1 = jxrs.rsvd_packed_subset(packed, N, 4, sample_indices=idx)
    s2 = jxrs.rsvd_packed_subset(bed.pack_dosage(g[:, idx]), len(idx), 4)
    for u, v in zip(s1, s2):
        np.testing.assert_array_equal(u, v)
    gf = g.copy()
    rows = np.arange(0, M, 97)
    gf[rows] = np.where(gf[rows] >= 0, 2 - gf[rows], -1)
    # converged runs: a row with p = 0.5 exactly keeps flip = False either way, so its sign (and the start block's product) changes
    a = jxrs.rsvd_packed_subset(packed, N, 3, power=30, tol=1e-7)
    f = jxrs.rsvd_packed_subset(bed.pack_dosage(gf), N, 3, power=30, tol=1e-7)
    assert np.max(np.abs(f[0] - a[0]) / a[0]) < 1e-6
    assert np.abs(_align(a[1], f[1]) - a[1]).max() < 1e-6


def test_edge_cases():
    from janusx_amd import janusx as jxrs
    g = _panel_dosage(40, 15, 0.01, seed=2)
    ev, vec, _maf, _flip = jxrs.rsvd_packed_subset(bed.pack_dosage(g), 40, 60)      # k >= n, kp capped by m
    assert vec.shape == (40, 15) and ev.shape == (15,)
    z, _m, _f, varsum = _design(g)
    eev = np.linalg.eigvalsh(z.T @ z / varsum)[::-1]
    assert np.max(np.abs(ev[:10] - eev[:10]) / eev[:10]) < 1e-5
    g = _panel_dosage(300, 400, 0.01, seed=4)
    g[3] = 2
    g[4] = -1                                                                      # monomorphic and all-missing rows
    ev, vec, maf, flip = jxrs.rsvd_packed_subset(bed.pack_dosage(g), 300, 3, power=30, tol=1e-7)
    assert maf[3] == 0.0 and flip[3] and maf[4] == 0.0 and not flip[4]
    z, _m, _f, varsum = _design(g)
    eev = np.linalg.eigvalsh(z.T @ z / varsum)[::-1]
    assert np.max(np.abs(ev - eev[:3]) / eev[:3]) < 1e-5


def _write_panel(tmp_path):
    g, packed = _data()
    prefix = str(tmp_path / "cohort")
    bim = bed.Bim(["1"] * M, [f"rs{j}" for j in range(M)], list(range(1, M + 1)), ["A"] * M, ["G"] * M)
    bed.write_bed(prefix, packed, [f"s{i}" for i in range(N)], bim)
    called = g >= 0
    alt = np.where(called, g, 0).sum(1) / (2.0 * np.maximum(called.sum(1), 1))
    keep = (np.minimum(alt, 1 - alt) >= 0.02) & (1.0 - called.mean(1) <= 0.05)
    z, _maf, _flip, varsum = _design(g[keep])
    return prefix, z, varsum


def _read_vec(path):
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows])


def test_cli_pca_routes(tmp_path):
    from janusx_amd import cli
    prefix, z, varsum = _write_panel(tmp_path)
    kk = z.T @ z / varsum
    eev, evec = np.linalg.eigh(kk)
    eev, evec = eev[::-1], evec[:, ::-1]
    out = str(tmp_path / "a")
    assert cli.main(["pca", "-bfile", prefix, "-o", out]) == 0
    ids, vec = _read_vec(out + ".eigenvec")
    assert ids == [f"s{i}" for i in range(N)] and vec.shape == (N, 3)
    lines = open(out + ".eigenvec").read().splitlines()
    assert all(len(f.split(".")[1]) == 6 for f in lines[0].split("\t")[1:])
    tab = np.loadtxt(out + ".eigenval")
    assert tab.shape == (N, 2)
    top = slice(0, 3)
    assert np.max(np.abs(tab[top, 0] - eev[top]) / eev[top]) < 1e-6
    np.testing.assert_allclose(tab[:, 1], tab[:, 0] / tab[:, 0].sum(), atol=2e-8)
    assert np.abs(_align(evec[:, top], vec) - evec[:, top]).max() <= 2e-6
    # -k on the GRM written by `jx grm`
    gout = str(tmp_path / "g")
    assert cli.main(["grm", "-bfile", prefix, "-o", gout]) == 0
    out2 = str(tmp_path / "b")
    assert cli.main(["pca", "-k", gout, "-o", out2]) == 0
    _, vec2 = _read_vec(out2 + ".eigenvec")
    assert np.abs(_align(vec, vec2) - vec).max() <= 2e-6
    tab2 = np.loadtxt(out2 + ".eigenval")
    assert np.max(np.abs(tab2[top, 0] - tab[top, 0]) / tab[top, 0]) < 1e-6
    assert cli.main(["pca", "-k", gout + ".cGRM.npy", "-o", out2]) == 0
    # -rsvd: k_eff rows, ratio over trace(K)
    out3 = str(tmp_path / "c")
    assert cli.main(["pca", "-bfile", prefix, "-rsvd", "3", "0.1", "-dim", "5", "-o", out3]) == 0
    t3 = np.loadtxt(out3 + ".eigenval")
    assert t3.shape == (5, 2)
    np.testing.assert_allclose(t3[:, 1], t3[:, 0] / np.trace(kk), rtol=1e-5, atol=1e-8)
    _, v3 = _read_vec(out3 + ".eigenvec")
    assert v3.shape == (N, 5)


def test_lu_rounds_hold_no_n_by_n_object():
    """The LU normalisation works on the n x kp block alone: at n = 60 000 a dense permutation (or any n x n object) would take
    28.8 GB of device memory."""
    import torch
    from janusx_amd import janusx as jxrs
    n = 60000
    g = _panel_dosage(n, 1500, 0.01, seed=9)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev, vec, _maf, _flip, rounds = jxrs._rsvd_packed_subset(bed.pack_dosage(g), n, 3, None, 42, 5, 1e-7)
    torch.cuda.synchronize()
    assert rounds >= 2 and vec.shape == (n, 3) and np.all(ev > 0)          # rounds before the last normalise by LU
    assert torch.cuda.max_memory_allocated() - base < (1 << 30)
