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


def _em_ref(g, p, q, rec=None):
    """The plain EM step in float64: -> (P_em, Q_em, unclipped p_em); `rec` replaces the float64 clamped P Q' (`_rec32`)."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    called = ~np.isnan(g)
    gg = np.where(called, g, 0.0)
    rec = np.clip(p @ q.T, 1e-6, 1 - 1e-6) if rec is None else rec
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


def _ll_ref(g, p, q, rec=None):
    called = ~np.isnan(g)
    if rec is None:
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


# ---- the kernels through their slices, tails, clamps and the Adam branch, on engines built from a Panel directly ----

from test_admx_host import _ax_grid, _ax_work_bytes      # noqa: E402  (the one restatement of `ax_grid` / `ax_work_bytes`)

AX_K = [1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64]
# name -> (n, rows of the payload, listed rows, seed)
AX_PANELS = {
    "sliced": (1100, 8300, 8200, 61),   # two groups and two tiles per slice, ragged last slices (`test_sliced_panel_grid`)
    "few_rows": (300, 40, 20, 62),      # fewer than the 32 rows of a group
    "k_eq_n": (64, 200, 150, 63),       # n < 128, K up to n
    "n128": (128, 100, 64, 64),         # one full tile, two full groups
    "n256": (256, 150, 100, 65),        # two full tiles
}
_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines (P32 images, work buffers, host genotypes) live for this module only."""
    yield
    _ENGINES.clear()


def _minor_counts(g, rows, flip):
    gr = g[rows].astype(np.float64)
    return np.where(g[rows] < 0, np.nan, np.where(flip[:, None], 2.0 - gr, gr))


def _make_engine(g, rows, flip):
    from janusx_amd import pipeline as pl
    panel = pl.Panel(torch.from_numpy(bed.pack_dosage(g)).cuda(), g.shape[1])
    return jx._AdmxEngine(panel, rows.astype(np.int32), flip), _minor_counts(g, rows, flip)


def _engine(name):
    """-> (engine, minor-allele counts of the listed rows with NaN for a missing call).  Sample 7 has no call at all, listed
    row 3 is all missing (the QC of a session would drop it) and listed row 2 monomorphic; the row list is descending and
    shorter than the payload."""
    if name not in _ENGINES:
        n, m, nrows, seed = AX_PANELS[name]
        g = _dosage(n, m, seed=seed)
        rows = np.arange(m - 1, -1, -1)[:nrows]
        g[rows[3]] = -1
        g[rows[2]] = np.where(g[rows[2]] < 0, -1, 0)
        called = g[rows] >= 0
        af = np.where(called, g[rows], 0).sum(1) / np.maximum(2.0 * called.sum(1), 1.0)
        _ENGINES[name] = _make_engine(g, rows, af > 0.5)
    return _ENGINES[name]


def _rec32(p, q):
    """rec as the kernels document it: the float32 dot product in k order (separately rounded multiply and add: the library is
    built without contraction), clamped at the float32 constants 1e-6f and 1.0f - 1e-6f; -> float64."""
    rec = np.zeros((p.shape[0], q.shape[0]), dtype=np.float32)
    for kk in range(p.shape[1]):
        rec = rec + p[:, kk:kk + 1] * q[:, kk][None, :]
    assert rec.dtype == np.float32
    return np.clip(rec, np.float32(1e-6), np.float32(1.0) - np.float32(1e-6)).astype(np.float64)


def _ll_sharp(eng, g, p, q, k):
    """-> (reference, bar).  With rec from `_rec32` the kernel and this sum differ only in the order of the additions and in the
    last bits of `log`.  Every term is <= 0, so sum |term| = |sum|.  The kernel adds a lane's terms in sequence (32 gps tps
    calls; counted twice here, for the addition inside a term as well), then 7 levels of the lane tree, then the S1 S2 partials
    in sequence: L over-counts the longest chain, and a chain of L additions costs at most L 2^-53 sum |term|.  The logarithms: 2 ulp for the device's, 1 ulp for numpy's, 3 x 2^-52 relative on every
    term.  The reference is summed in extended precision."""
    called = ~np.isnan(g)
    rec = _rec32(p, q)
    gg = np.where(called, g, 0.0)
    terms = np.where(called, gg * np.log(rec) + (2.0 - gg) * np.log(1.0 - rec), 0.0)
    ref = float(np.sum(terms.astype(np.longdouble)))
    s1, s2, gps, tps = _ax_grid(eng.m, eng.n, k)
    chain = 2 * 32 * gps * tps + 7 + s1 * s2 + 1                 # + 1: the addition inside a term of this reference
    return ref, (chain * 2.0 ** -53 + 3 * 2.0 ** -52) * float(np.sum(np.abs(terms)))


def test_sliced_panel_grid():
    """The large panel is there for the slice loops: if the launch arithmetic changes, this fails instead of emptying the rest."""
    from janusx_amd._lib import lib
    n, _m, nrows, _seed = AX_PANELS["sliced"]
    for k in AX_K:
        s1, s2, gps, tps = _ax_grid(nrows, n, k)
        assert (s1, s2, gps, tps) == (129, 5, 2, 2)
        assert nrows - (s1 - 1) * gps * 32 == 8                   # the last SNP slice: one group of 8 rows
        assert n - (s2 - 1) * tps * 128 == 76                     # the last sample slice: one tile of 76 samples
        assert lib().jxg_admx_work_bytes(nrows, n, k) == _ax_work_bytes(nrows, n, k)   # the library's grid is the restated one
    for name in ("few_rows", "k_eq_n", "n128", "n256"):
        n, _m, nrows, _seed = AX_PANELS[name]
        assert _ax_grid(nrows, n, 4)[2:] == (1, 1)


@pytest.mark.parametrize("name", list(AX_PANELS))
def test_called_counts(name):
    eng, g = _engine(name)
    qb = eng.qb.cpu().numpy()
    assert np.array_equal(qb, 2.0 * (~np.isnan(g)).sum(0)) and qb[7] == 0


@pytest.mark.parametrize("k", AX_K)
@pytest.mark.parametrize("name", list(AX_PANELS))
def test_em_step_slices_and_tails(name, k):
    eng, g = _engine(name)
    p, q = _pq(eng.m, eng.n, k, 300 + k)
    p_ref, q_ref, _ = _em_ref(g, p, q)
    pt, qt = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    pe, qe = eng.em_step(pt, qt)
    pe2, qe2 = eng.em_step(pt, qt)
    assert torch.equal(pe, pe2) and torch.equal(qe, qe2)
    assert _rel(pe.cpu().numpy(), p_ref) < 1e-5
    assert _rel(qe.cpu().numpy(), q_ref) < 1e-5
    assert np.array_equal(pe.cpu().numpy()[3], p[3])              # the all-missing row: A = B = 0, p_em = p


@pytest.mark.parametrize("k", AX_K)
@pytest.mark.parametrize("name", list(AX_PANELS))
def test_loglik_slices_and_tails(name, k):
    eng, g = _engine(name)
    p, q = _pq(eng.m, eng.n, k, 500 + k)
    pt, qt = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    a, b = eng.loglik(pt, qt), eng.loglik(pt, qt)
    assert a == b
    ref = _ll_ref(g, p, q)
    assert abs(a - ref) <= 1e-6 * abs(ref)
    sharp, bar = _ll_sharp(eng, g, p, q, k)
    assert abs(a - sharp) <= bar, (abs(a - sharp), bar)


@pytest.mark.parametrize("k", AX_K)
@pytest.mark.parametrize("name", list(AX_PANELS))
def test_adam_step_from_live_moments(name, k):
    """One Adam-EM iteration from non-zero moments (sqrt(v) is a number, not rounding noise) against float64, at the 1e-5 of
    the EM step.  Every output is a sum that can cancel (delta = target - x in the moments, x + step in P and Q: a step of
    lr m / sqrt(v) is as large as a small Q entry), so 1e-5 is taken of the sum of the magnitudes of its terms:
    beta1 |m| + (1 - beta1) (|target| + |x|),  beta2 v + (1 - beta2) (|target| + |x|)^2  and  |x| + |step|.
    Q is divided by its row sum s afterwards: an entry within e_k before gives |dq_k| <= (e_k + q_k sum_j e_j) / s."""
    eng, g = _engine(name)
    lr, b1, b2, eps = 0.005, 0.8, 0.88, 1e-8
    ms, vs = 1.0 / (1.0 - b1 ** 3), 1.0 / (1.0 - b2 ** 3)
    p, q = _pq(eng.m, eng.n, k, 700 + k)
    rng = np.random.default_rng(900 + k)
    mom = [rng.uniform(-0.1, 0.1, p.shape), rng.uniform(0.01, 0.1, p.shape), rng.uniform(-0.1, 0.1, q.shape),
           rng.uniform(0.01, 0.1, q.shape)]
    mom = [x.astype(np.float32) for x in mom]
    _pe, qe_ref, pem_ref = _em_ref(g, p, q)
    out, tol = [], []
    for x, target, m0, v0 in ((p, pem_ref, mom[0], mom[1]), (q, qe_ref, mom[2], mom[3])):
        x, m0, v0 = x.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
        d = target - x
        m1 = b1 * m0 + (1 - b1) * d
        v1 = b2 * v0 + (1 - b2) * d * d
        step = lr * (m1 * np.float32(ms)) / (np.sqrt(v1 * np.float32(vs)) + eps)
        out += [_clip(x + step), m1, v1]
        mag = np.abs(target) + np.abs(x)
        tol += [b1 * np.abs(m0) + (1 - b1) * mag, b2 * v0 + (1 - b2) * mag * mag, np.abs(x) + np.abs(step)]
    p_ref, mp_ref, vp_ref, q_ref, mq_ref, vq_ref = out
    qs = q_ref.sum(1, keepdims=True)
    q_ref = q_ref / qs
    tol[5] = (tol[5] + q_ref * tol[5].sum(1, keepdims=True)) / qs
    dev = [torch.from_numpy(x.copy()).cuda() for x in (p, q, *mom)]
    eng.adam_step(dev[0], dev[1], tuple(dev[2:]), lr, b1, b2, eps, ms, vs)
    got = [x.cpu().numpy().astype(np.float64) for x in dev]
    # as in test_adam_em_loop: the all-missing sample's EM target is its own row, its delta rounding noise;
    # it is held to the step bound, every other row to the bars above
    noise = np.isnan(g).all(0)
    assert np.array_equal(np.nonzero(noise)[0], [7])
    if k > 1:                                                     # at K = 1 every row is 1 and its target is 1
        assert np.array_equal(noise, np.all(np.abs(qe_ref - q) < 1e-6, axis=1))
    assert np.all(np.abs(got[0] - p_ref) <= 1e-5 * tol[2])
    assert np.all(np.abs(got[1] - q_ref)[~noise] <= 1e-5 * tol[5][~noise])
    assert np.max(np.abs(got[1][noise] - q_ref[noise])) <= 2 * lr
    assert np.all(np.abs(got[2] - mp_ref) <= 1e-5 * tol[0]) and np.all(np.abs(got[3] - vp_ref) <= 1e-5 * tol[1])
    assert np.all(np.abs(got[4] - mq_ref)[~noise] <= 1e-5 * tol[3][~noise])
    assert np.all(np.abs(got[5] - vq_ref)[~noise] <= 1e-5 * tol[4][~noise])
    assert np.max(np.abs(got[1].sum(1) - 1.0)) <= 1e-5


def _cancellation_bars(g, p, q, rec, q_ref):
    """Relative bars of P_em and Q_em where the float32 forms of the reference, which the kernel keeps, cancel:
        denom = p (a - b) + b        per (row, k), a = sum_i aa q, b = sum_i bb q
        t    += p (aa - bb) + bb     per call and k
    With u = 2^-24, forming aa - bb, the product and the sum costs at most 4 u (p |aa - bb| + bb) per term (three roundings,
    and the last bits of aa and bb themselves), 4 u (p |a - b| + b) for denom.  Where bb is 1e6 against aa of 1 (rec at the upper
    clamp, calls below 2) that is the whole error; elsewhere it adds 2e-7 to the 1e-5 of the EM step.  Q_em is divided by its row
    sum: a relative error e_k before gives e_k + sum_j q_j e_j after.  -> (bar of P_em, bar of Q_em), both relative."""
    u = 2.0 ** -24
    p, q = p.astype(np.float64), q.astype(np.float64)
    called = ~np.isnan(g)
    gg = np.where(called, g, 0.0)
    aa = np.where(called, gg / rec, 0.0)
    bb = np.where(called, (2.0 - gg) / (1.0 - rec), 0.0)
    a, b = aa @ q, bb @ q
    den = np.abs(p * (a - b) + b)
    pbar = 1e-5 + 4 * u * (p * np.abs(a - b) + b) / np.where(den < 1e-8, np.inf, den)
    t = (aa - bb).T @ p + bb.sum(0)[:, None]
    extra = 4 * u * (np.abs(aa - bb).T @ p + bb.sum(0)[:, None]) / np.where(t > 0, t, np.inf)
    return pbar, 1e-5 + extra + (q_ref * extra).sum(1, keepdims=True)


@pytest.mark.parametrize("k", [2, 5, 33])
@pytest.mark.parametrize("calls", ["fixed", "every kind"])
def test_rec_clamps_and_clipped_inputs(calls, k):
    """P rows at 0, 1e-5, 1 and 1 - 1e-5 and Q rows with one entry at 1 - (K - 1) 1e-5: rec reaches both clamps and comes within
    1e-4 of 1 without being clamped, where 1 - rec carries the float32 rounding of rec that no float64 product shares, so the
    restatement takes rec from `_rec32`.  The rows at 0 and 1e-5 have calls of every kind.  The rows at 1 and 1 - 1e-5 come twice:
    "fixed" for the allele (every call 2, as where a fit drives P to the upper clip; 2 - g = 0 there, so this half sees the upper
    clamp only through aa and log(rec)), held to the plain 1e-5; and with calls of "every kind", where bb = (2 - g) / (1 - rec)
    reaches 1e6 and log(1 - rec) enters the likelihood.  The log-likelihood is held to 1e-6 and to the sharp bar in both; the EM
    step of the second, where the float32 forms of the reference cancel 1e6 against 1e6, to the bars of `_cancellation_bars`
    (wide on exactly those rows and on Q: what an EM step can show there is a wrong bb, not its last percent)."""
    n, m = 256, 120
    g = _dosage(n, m, seed=77)
    rows = np.arange(m - 1, 19, -1)
    called = g[rows] >= 0
    flip = np.where(called, g[rows], 0).sum(1) / np.maximum(2.0 * called.sum(1), 1.0) > 0.5
    if calls == "fixed":
        g[rows[2]] = np.where(g[rows[2]] < 0, -1, 2)
        g[rows[3]] = np.where(g[rows[3]] < 0, -1, 0)              # stored 0, flipped: minor-allele count 2
        flip[2], flip[3] = False, True
    g[rows[4]] = -1
    flip[4] = False
    eng, gk = _make_engine(g, rows, flip)
    assert np.isnan(gk[4]).all()
    p, q = _pq(len(rows), n, k, 40 + k)
    p[0], p[1], p[2], p[3] = 0.0, 1e-5, 1.0, 1.0 - 1e-5
    q[10:20] = np.float32(1e-5)
    q[np.arange(10, 20), np.arange(10) % k] = np.float32(1.0 - (k - 1) * 1e-5)
    rec = _rec32(p, q)
    lo, hi = float(np.float32(1e-6)), float(np.float32(1.0) - np.float32(1e-6))
    near = (rec < hi) & (rec > 1.0 - 1e-4)
    assert (rec == lo).any() and (rec == hi).any() and near.any()
    if calls == "fixed":
        assert np.all(np.nan_to_num(gk[2:4], nan=2.0) == 2.0)
    else:
        assert ((rec == hi) & (gk < 2)).any() and (near & (gk < 2)).any()      # 1 - rec reaches bb and log(1 - rec)
    pt, qt = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
    p_ref, q_ref, _ = _em_ref(gk, p, q, rec=rec)
    pe, qe = (x.cpu().numpy().astype(np.float64) for x in eng.em_step(pt, qt))
    if calls == "fixed":
        assert _rel(pe, p_ref) < 1e-5
        assert _rel(qe, q_ref) < 1e-5
    else:
        pbar, qbar = _cancellation_bars(gk, p, q, rec, q_ref)
        usual = np.ones(len(rows), dtype=bool)
        usual[2:4] = False
        assert _rel(pe[usual], p_ref[usual]) < 1e-5               # a row's P_em sees no other row: the plain bar
        assert np.all(np.abs(pe - p_ref)[2:4] <= (pbar * p_ref)[2:4])
        assert np.all(np.abs(qe - q_ref) <= qbar * q_ref)         # every sample meets rows 2 and 3
    assert np.array_equal(pe[4], p[4].astype(np.float64))         # |denom| < 1e-8: p_em = p
    a = eng.loglik(pt, qt)
    ref = _ll_ref(gk, p, q, rec=rec)
    assert abs(a - ref) <= 1e-6 * abs(ref)
    sharp, bar = _ll_sharp(eng, gk, p, q, k)
    assert abs(a - sharp) <= bar, (abs(a - sharp), bar)
