"""`jx adamixture` on the GPU: the EM pass, its finalise, the log-likelihood and the Adam-EM loop (`jxg_admx_*`,
csrc/k_admx.hip) against float64 numpy restatements of the reference (src/stats/adamixture.rs:2957-3005, 5434-5898) kept in
this file, a simulated admixture, the refusals and the CLI."""

import os

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import janusx as jx

pytestmark = pytest.mark.gpu

N, M = 300, 420            # n not a multiple of 128


def _dosage(n=N, m=M, seed=11):
    """1 % missing calls, rows with an allele frequency above 0.5 (flipped), and sample 7 with every call missing."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.95, m)
    g = rng.binomial(2, np.repeat(af[:, None], n, 1)).astype(np.int8)
    g[rng.random(g.shape) < 0.01] = -1
    g[:, 7] = -1
    return g


def _write(tmp, g, name="p"):
    prefix = os.path.join(str(tmp), name)
    m, n = g.shape
    b = bed.Bim(["1"] * m, [f"s{j}" for j in range(m)], list(range(100, 100 + m)), ["A"] * m, ["G"] * m)
    bed.write_bed(prefix, bed.pack_dosage(g), [f"i{i}" for i in range(n)], b)
    return prefix


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    g = _dosage()
    prefix = _write(tmp_path_factory.mktemp("admx"), g)
    s = jx.AdmxBedTrainingSession(prefix, snps_only=True, maf=0.02, missing_rate=0.05)
    rows, flip = s.kept_rows(), s.row_flip()
    gk = g[rows].astype(np.float64)
    gk = np.where(g[rows] < 0, np.nan, np.where(flip[:, None], 2.0 - gk, gk))     # minor-allele counts of the kept rows
    assert flip.any() and (~flip).any() and rows.size > 300
    return s, gk, prefix


def _pq(m, n, k, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, (m, k)).astype(np.float32)
    q = rng.uniform(0.05, 1.0, (n, k)).astype(np.float32)
    return p, (q / q.sum(1, keepdims=True)).astype(np.float32)


def _clip(x):
    return np.clip(x, 1e-5, 1 - 1e-5)


def _em_ref(g, p, q):
    """The plain EM step in float64: -> (P_em, Q_em, a, b, t)."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    called = ~np.isnan(g)
    gg = np.where(called, g, 0.0)
    rec = np.clip(p @ q.T, 1e-6, 1 - 1e-6)
    aa = np.where(called, gg / rec, 0.0)
    bb = np.where(called, (2.0 - gg) / (1.0 - rec), 0.0)
    a, b = aa @ q, bb @ q
    t = (aa - bb).T @ p + bb.sum(0)[:, None]
    qb = 2.0 * called.sum(0)
    den = p * (a - b) + b
    pem = np.where(np.abs(den) < 1e-8, p, a * p / np.where(den == 0, 1.0, den))
    qe = np.where(qb[:, None] > 0, _clip(q * t / np.maximum(qb, 1.0)[:, None]), _clip(q))
    s = qe.sum(1, keepdims=True)
    return _clip(pem), qe / s, pem


def _ll_ref(g, p, q):
    called = ~np.isnan(g)
    rec = np.clip(p.astype(np.float64) @ q.astype(np.float64).T, 1e-6, 1 - 1e-6)
    gg = np.where(called, g, 0.0)
    return float(np.sum(np.where(called, gg * np.log(rec) + (2.0 - gg) * np.log(1.0 - rec), 0.0)))


def _dense_u8(g):
    return np.where(np.isnan(g), 3, g).astype(np.uint8)


def _rel(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1e-30)))


@pytest.mark.parametrize("k", [1, 2, 5, 16, 33, 64])
def test_em_step(panel, k):
    s, g, _ = panel
    p, q = _pq(s.n_snps, s.n_samples, k, 100 + k)
    p_ref, q_ref, _ = _em_ref(g, p, q)
    pe, qe = s._eng.em_step(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    assert _rel(pe.cpu().numpy(), p_ref) < 1e-5
    assert _rel(qe.cpu().numpy(), q_ref) < 1e-5
    pd, qd = np.zeros_like(p), np.zeros_like(q)
    jx.admx_em_step_inplace_f32(_dense_u8(g), p, q, pd, qd)
    assert _rel(pd, p_ref) < 1e-5 and _rel(qd, q_ref) < 1e-5
    pe2, qe2 = s._eng.em_step(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    assert torch.equal(pe, pe2) and torch.equal(qe, qe2)


@pytest.mark.parametrize("k", [3, 17])
def test_loglikelihood(panel, k):
    s, g, prefix = panel
    p, q = _pq(s.n_snps, s.n_samples, k, 7 + k)
    ref = _ll_ref(g, p, q)
    pt, qt = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    a, b = s._eng.loglik(pt, qt), s._eng.loglik(pt, qt)
    assert a == b
    assert abs(a - ref) <= 1e-6 * abs(ref)
    assert abs(jx.admx_loglikelihood_f32(_dense_u8(g), p, q) - ref) <= 1e-6 * abs(ref)
    assert abs(jx.admx_loglikelihood_bed_f32(prefix, p, q) - ref) <= 1e-6 * abs(ref)


def _adam_ref(g, p, q, iters, check, lr=0.005, b1=0.8, b2=0.88, eps=1e-8, decay=0.5, min_lr=1e-6):
    p, q = p.astype(np.float64), q.astype(np.float64)
    mp, vp, mq, vq = (np.zeros_like(x) for x in (p, p, q, q))
    best, pb, qb, bad, last, trace = -np.inf, None, None, 0, 0, []
    b1p = b2p = 1.0
    for it in range(iters):
        last = it + 1
        b1p, b2p = b1p * b1, b2p * b2
        _, qe, pem = _em_ref(g, p, q)
        for x, target, m_, v_ in ((p, pem, mp, vp), (q, qe, mq, vq)):
            d = target - x
            m_[...] = b1 * m_ + (1 - b1) * d
            v_[...] = b2 * v_ + (1 - b2) * d * d
            x[...] = _clip(x + lr * (m_ / (1 - b1p)) / (np.sqrt(v_ / (1 - b2p)) + eps))
        q /= q.sum(1, keepdims=True)
        if last % check:
            continue
        ll = _ll_ref(g, p, q)
        trace.append((last, ll))
        if abs(ll - best) < 0.1:
            break
        if ll > best:
            best, pb, qb, bad = ll, p.copy(), q.copy(), 0
        else:
            bad += 1
            lr = max(lr * decay, min_lr)
            if bad >= 2:
                break
    return pb, qb, best, last, trace


def test_adam_em_loop(panel):
    s, g, _ = panel
    k = 4
    p0, q0 = _pq(s.n_snps, s.n_samples, k, 5)
    pr, qr, llr, itr, trr = _adam_ref(g, p0, q0, 10, 5)
    tr = []
    p, q, ll, it = jx._admx_adam_loop(s._eng, torch.from_numpy(p0).cuda(), torch.from_numpy(q0).cuda(), 0.005, 0.8, 0.88,
                                      1e-8, 10, 5, 0.5, 1e-6, trace=tr)
    assert it == itr and len(tr) == len(trr)
    for (i1, l1), (i2, l2) in zip(tr, trr):
        assert i1 == i2 and abs(l1 - l2) <= 1e-6 * abs(l2)
    assert abs(ll - llr) <= 1e-6 * abs(llr)
    assert np.max(np.abs(p.cpu().numpy() - pr)) <= 1e-4
    # A row whose EM target equals the row itself (the all-missing sample: qb = 0, q_em = q) has an Adam delta of rounding
    # noise alone, and Adam's normalised step lr m / sqrt(v) moves it by about +-lr whatever the noise's size, so its sign
    # decides the path.  Those rows are held to the step bound; every other row to 1e-4.
    _pe, qe0, _ = _em_ref(g, p0, q0)
    noise = np.all(np.abs(qe0 - q0) < 1e-6, axis=1)
    assert np.array_equal(np.nonzero(noise)[0], [7])
    dq = np.abs(q.cpu().numpy() - qr)
    assert np.max(dq[~noise]) <= 1e-4
    assert np.max(dq[noise]) <= 2 * 10 * 0.005
    p2, q2, ll2, it2 = jx.admx_adam_optimize_f32(_dense_u8(g), p0, q0, max_iter=10, check_every=5)
    assert it2 == it and abs(ll2 - ll) <= 1e-6 * abs(ll)


def test_k1_closed_form(panel):
    s, g, _ = panel
    p, q = _pq(s.n_snps, s.n_samples, 1, 3)
    q[:] = 1.0
    pe, qe = s._eng.em_step(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    called = ~np.isnan(g)
    maf = np.nansum(g, 1) / (2.0 * called.sum(1))
    assert _rel(pe.cpu().numpy()[:, 0], _clip(maf)) < 1e-6
    assert torch.all(qe == 1.0)
    _p, qf, ll, it, init_ll, als = s.fit_k(1, 42, "adam-em", 5, 1e-5, 1000, 1e-5, 0.005, 0.8, 0.88, 1e-8, 50, 5, 0.5, 1e-6)
    assert np.all(qf == 1.0) and np.isfinite(ll) and np.isfinite(init_ll)


def _simulate(n=1500, m=12000, k=3, seed=2026):
    rng = np.random.default_rng(seed)
    q = rng.dirichlet(np.full(k, 0.5), n)
    base = rng.uniform(0.1, 0.9, m)
    p = np.clip(base[:, None] + rng.normal(0.0, 0.25, (m, k)), 0.02, 0.98)
    g = rng.binomial(2, p @ q.T).astype(np.int8)
    return g, p, q


def test_simulated_admixture(tmp_path):
    import itertools
    g, p_true, q_true = _simulate()
    prefix = _write(tmp_path, g, "sim")
    s = jx.AdmxBedTrainingSession(prefix)
    args = (3, 42, "adam-em", 5, 1e-5, 1000, 1e-5, 0.005, 0.8, 0.88, 1e-8, 500, 5, 0.5, 1e-6)
    p, q, ll, it, init_ll, als = s.fit_k(*args)
    best = min(np.sqrt(np.mean((q[:, list(pm)] - q_true) ** 2)) for pm in itertools.permutations(range(3)))
    assert best <= 0.03
    rows, flip = s.kept_rows(), s.row_flip()
    gk = np.where(flip[:, None], 2.0 - g[rows], g[rows]).astype(np.float64)
    pt = np.where(flip[:, None], 1.0 - p_true[rows], p_true[rows])
    assert ll >= _ll_ref(gk, pt, q_true)
    assert np.max(np.abs(q.sum(1) - 1.0)) <= 1e-5
    assert p.dtype == np.float32 and p.min() >= np.float32(1e-5) and p.max() <= np.float32(1 - 1e-5)
    # Q is clipped to [1e-5, 1 - 1e-5] after its Adam step and then row-normalised, as the reference: a clipped entry ends at
    # 1e-5 / s, where the row sum s of the stepped row is at most 1 + K lr (each entry moves by at most lr)
    assert q.dtype == np.float32 and q.min() >= np.float32(1e-5 / (1 + 3 * 0.005)) and q.max() <= np.float32(1 - 1e-5)
    p2, q2, ll2, it2, init2, als2 = s.fit_k(*args)
    assert np.array_equal(p, p2) and np.array_equal(q, q2) and ll == ll2 and it == it2 and init_ll == init2 and als == als2


def test_refusals(panel, tmp_path):
    s, _g, _ = panel
    args = (42, "adam", 5, 1e-5, 1000, 1e-5, 0.005, 0.8, 0.88, 1e-8, 5, 5, 0.5, 1e-6)
    with pytest.raises(RuntimeError, match="K must be within"):
        s.fit_k(65, *args)
    p, q = _pq(s.n_snps, s.n_samples, 65, 1)
    with pytest.raises(RuntimeError, match="K must be within"):
        s._eng.em_step(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    small = jx.AdmxBedTrainingSession(_write(tmp_path, _dosage(n=10, m=200, seed=3)[:, :10], "small"), maf=0.0, missing_rate=1.0)
    with pytest.raises(RuntimeError, match="exceeds the number of samples"):
        small.fit_k(12, *args)
    with pytest.raises(RuntimeError, match="exceeds sample-side RSVD rank"):
        small.fit_k(12, 42, "adam-em", *args[2:])
    from janusx_amd._lib import lib
    with pytest.raises(RuntimeError, match=r"K must be within \[1, 64\]"):
        from janusx_amd._lib import check
        check(lib().jxg_admx_loglik(None, 0, 300, None, 10, None, 65, None, None, None, 0, None, None))


def test_cli_end_to_end(panel, tmp_path):
    from janusx_amd import cli
    s, _g, prefix = panel
    ids = bed.read_fam_ids(prefix)
    for cmd in ("adamixture", "fastpop"):
        out = tmp_path / cmd
        assert cli.main([cmd, "-bfile", prefix, "-k", "2..3", "-o", str(out), "-max-iter", "30"]) == 0
        for k in (2, 3):
            base = out / f"p.{k}"
            lines = (out / f"p.{k}.Q.txt").read_text().splitlines()
            assert len(lines) == len(ids)
            for sid, line in zip(ids, lines):
                parts = line.split("\t")
                assert parts[0] == sid and len(parts) == k + 1
                assert all(len(v.split(".")[1]) == 8 for v in parts[1:])
            pn = np.load(f"{base}.P.npy")
            assert pn.dtype == np.float32 and pn.shape == (s.n_snps, k)
            site = (out / f"p.{k}.P.site").read_text().splitlines()
            assert len(site) == s.n_snps
            for line, r, f in zip(site, s.kept_rows(), s.row_flip()):
                assert line == (f"1\t{100 + r}\tG\tA" if f else f"1\t{100 + r}\tA\tG")
            assert (out / f"p.{k}.fastpop.log").exists()
        assert "K\tll_final" in (out / "p.fastpop.summary.log").read_text()
