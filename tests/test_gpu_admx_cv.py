"""`jx adamixture -cverror` on the GPU: the three passes of csrc/k_admx_cv.hip (`jxg_admx_cv_fold_counts`, `_fold_image`,
`_holdout_nll`), the fold backend, `admx_evaluate_cverror` and the command, against numpy restatements of the reference
(src/stats/adamixture.rs:1641-1661, 3056-3214, 4486-4631; python/janusx/adamixture/core.py:1662-1794) kept in this file."""

import os

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import janusx as jx

pytestmark = pytest.mark.gpu

N, M = 300, 420            # n not a multiple of 128 or of 4
SEEDS = [42, (1 << 63) + 5]
FIT = ("adam-em", 5, 1e-5, 1000, 1e-5, 0.005, 0.8, 0.88, 1e-8, 200, 5, 0.5, 1e-6)    # the CLI's settings at -max-iter 200


def _dosage(n=N, m=M, seed=11):
    """The panel of tests/test_gpu_admx.py: 1 % missing calls, rows with an allele frequency above 0.5 (flipped), and sample 7
    with every call missing."""
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


def _fold_ids(m, n, folds, seed):
    """`cv_fold_id` of every (kept row, sample): SplitMix64 of (row n + sample) ^ (seed ^ golden), wrapping u64, mod folds."""
    flat = np.arange(m, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
    x = flat ^ np.uint64((int(seed) & ((1 << 64) - 1)) ^ 0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x % np.uint64(folds)).astype(np.int64)


def _minor(g, s):
    """Minor-allele counts of the session's kept rows, NaN for a missing call."""
    rows, flip = s.kept_rows(), s.row_flip()
    gk = g[rows].astype(np.float64)
    return np.where(g[rows] < 0, np.nan, np.where(flip[:, None], 2.0 - gk, gk))


def _codes(p32):
    """(tiles, rows, 32) bytes of a P32 image -> (rows, tiles x 128) 2-bit codes (sample 4 b + c of a tile: bits 2c of byte b)."""
    a = p32.cpu().numpy()
    c = (a[..., None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3
    return c.reshape(a.shape[0], a.shape[1], 128).transpose(1, 0, 2).reshape(a.shape[1], -1)


def _pq(m, n, k, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, (m, k)).astype(np.float32)
    q = rng.uniform(0.05, 1.0, (n, k)).astype(np.float32)
    return p, (q / q.sum(1, keepdims=True)).astype(np.float32)


def _ll_ref(g, p, q, mask):
    """Training log-likelihood over the calls of `mask` (float64, clamp 1e-6 as `loglikelihood_packed_train_fold_f32_impl`)."""
    rec = np.clip(p.astype(np.float64) @ q.astype(np.float64).T, 1e-6, 1 - 1e-6)
    gg = np.where(mask, g, 0.0)
    return float(np.sum(np.where(mask, gg * np.log(rec) + (2.0 - gg) * np.log(1.0 - rec), 0.0)))


def _holdout_ref(g, p, q, mask, rec=None):
    """-> (ll_sum, count) of the calls of `mask`: [g == 1] ln 2 + g ln rec + (2 - g) ln(1 - rec), rec clipped in float64 to
    [1e-8, 1 - 1e-8] (python/janusx/adamixture/core.py:365)."""
    if rec is None:
        rec = p.astype(np.float64) @ q.astype(np.float64).T
    rec = np.clip(rec, 1e-8, 1.0 - 1e-8)
    gg = np.where(mask, g, 0.0)
    t = np.where(gg == 1.0, np.log(2.0), 0.0) + gg * np.log(rec) + (2.0 - gg) * np.log(1.0 - rec)
    return float(np.sum(np.where(mask, t, 0.0))), int(mask.sum())


class _Case:
    def __init__(self, tmp, g, name, **qc):
        self.g = g
        self.prefix = _write(tmp, g, name)
        self.s = jx.AdmxBedTrainingSession(self.prefix, **qc)
        self.gk = _minor(g, self.s)
        self.called = ~np.isnan(self.gk)
        self.m, self.n = self.gk.shape
        self._folds = {}

    def folds(self, folds, seed):
        if (folds, seed) not in self._folds:
            self._folds[(folds, seed)] = _fold_ids(self.m, self.n, folds, seed)
        return self._folds[(folds, seed)]


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    c = _Case(tmp_path_factory.mktemp("admxcv"), _dosage(), "p", snps_only=True, maf=0.02, missing_rate=0.05)
    flip = c.s.row_flip()
    assert flip.any() and (~flip).any() and c.m > 300 and not c.called[:, 7].any()
    return c


@pytest.fixture(scope="module")
def sliced(tmp_path_factory):
    """n = 1100, 8300 rows: the count and image passes walk 3 tiles per slice in 3 slices, the hold-out pass 2 groups of rows
    and 2 tiles per slice, with ragged last slices (9 tiles, the last of 76 samples)."""
    c = _Case(tmp_path_factory.mktemp("admxcv_sliced"), _dosage(1100, 8300, seed=61), "sliced")
    assert c.m > 8192 + 32 and c.m % 16 != 0 and c.n == 1100
    return c


def _check_counts(c, folds, seed):
    obs, counts = c.s.cv_observed_fold_counts(folds, seed)
    want = np.bincount(c.folds(folds, seed)[c.called], minlength=folds)
    assert counts.dtype == np.int64 and np.array_equal(counts, want)
    assert obs == int(c.called.sum()) == int(counts.sum())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("folds", [2, 3, 5, 256])
def test_fold_counts(panel, folds, seed):
    _check_counts(panel, folds, seed)


def _check_fold_image(c, fold_id, folds, seed):
    s = c.s
    fb = s.make_cv_fold_backend(fold_id, folds, seed)
    held = c.called & (c.folds(folds, seed) == fold_id)
    train = c.called & ~held
    st = fb._row_stats
    assert st.dtype == np.int32
    assert np.array_equal(st[:, 0], train.sum(1)) and np.array_equal(st[:, 1], held.sum(1))
    assert np.array_equal(st[:, 2], np.where(train, c.gk, 0.0).sum(1).astype(np.int64))
    tr = train.sum(1).astype(np.float64)
    freq = np.where(tr > 0, np.where(train, c.gk, 0.0).sum(1) / (2.0 * np.maximum(tr, 1.0)), 0.0).astype(np.float32)
    assert fb.row_freq().dtype == np.float32 and np.array_equal(fb.row_freq(), freq)
    assert fb.train_observed == int(train.sum()) and fb.holdout_observed == int(held.sum())
    assert fb.train_observed + fb.holdout_observed == int(c.called.sum())
    assert (fb.fold_id, fb.folds, fb.cv_seed) == (fold_id, folds, seed & ((1 << 64) - 1))
    assert np.array_equal(fb.row_flip(), s.row_flip()) and np.array_equal(fb.kept_rows(), s.kept_rows())
    assert (fb.n_snps, fb.n_samples) == (c.m, c.n)
    # the image: the source rows in list order with exactly the fold's calls turned into 01, padding untouched
    src = _codes(s._panel.p32)[s.kept_rows()]
    want = src.copy()
    want[:, :c.n][held] = 1
    got = _codes(fb._panel.p32)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.all(got[:, c.n:] == 1) and np.array_equal(src[:, :c.n] != 1, c.called)
    return fb, train, held


@pytest.mark.parametrize("fold_id", [0, 1, 2])
def test_fold_image(panel, fold_id):
    fb, train, _held = _check_fold_image(panel, fold_id, 3, 42)
    # read back through the engine: training-only likelihood and called counts
    p, q = _pq(panel.m, panel.n, 3, 20 + fold_id)
    ref = _ll_ref(panel.gk, p, q, train)
    got = fb._eng.loglik(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    assert abs(got - ref) <= 1e-6 * abs(ref)
    assert abs(fb.loglikelihood_f32(p, q) - ref) <= 1e-6 * abs(ref)
    assert np.array_equal(fb._eng.qb.cpu().numpy(), 2.0 * train.sum(0))
    fb.close()
    assert fb._panel is None and fb._eng is None


def test_fold_image_large_seed(panel):
    _check_fold_image(panel, 4, 5, SEEDS[1])[0].close()


def test_row_without_training_calls(tmp_path):
    """A row with three calls that all fall into one of two folds (seed searched on the host): as that fold is held out the row
    has no training call, its frequency is 0 and nothing is NaN."""
    n, m, bed_row = 40, 60, 9
    g = _dosage(n, m, seed=5)
    g[bed_row] = -1
    g[bed_row, [3, 17, 30]] = [1, 0, 1]
    c = _Case(tmp_path, g, "edge", maf=0.0, missing_rate=1.0)
    row = int(np.nonzero(c.s.kept_rows() == bed_row)[0][0])
    assert not c.s.row_flip()[row] and c.called[row].sum() == 3
    for seed in range(200):
        ids = c.folds(2, seed)[row][c.called[row]]
        if np.all(ids == ids[0]):
            break
    else:
        raise AssertionError("no seed puts the row's three calls into one fold")
    fold_id = int(ids[0])
    fb, train, held = _check_fold_image(c, fold_id, 2, seed)
    assert tuple(fb._row_stats[row]) == (0, 3, 0) and fb.row_freq()[row] == 0.0
    assert np.all(np.isfinite(fb.row_freq()))
    p, q = _pq(c.m, n, 2, 1)
    ll = fb._eng.loglik(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    assert np.isfinite(ll) and abs(ll - _ll_ref(c.gk, p, q, train)) <= 1e-6 * abs(ll)
    mean_nll, dev, n_eval = fb.holdout_nll_f32(p, q)
    ref, cnt = _holdout_ref(c.gk, p, q, held)
    assert n_eval == cnt and np.isfinite(mean_nll) and abs(-mean_nll * n_eval - ref) <= 1e-6 * abs(ref)
    pe, qe = fb._eng.em_step(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda())
    assert bool(torch.isfinite(pe).all()) and bool(torch.isfinite(qe).all())
    assert np.array_equal(pe.cpu().numpy()[row], p[row])             # no training call: A = B = 0, p_em = p
    fb.close()
    other = c.s.make_cv_fold_backend(1 - fold_id, 2, seed)
    assert tuple(other._row_stats[row]) == (3, 0, 2) and other.row_freq()[row] == np.float32(2.0 / 6.0)
    other.close()


@pytest.mark.parametrize("k", [3, 17])
def test_holdout_nll(panel, k):
    p, q = _pq(panel.m, panel.n, k, 7 + k)
    total_ll, total_n = 0.0, 0
    for fold_id in range(3):
        fb = panel.s.make_cv_fold_backend(fold_id, 3, 42)
        held = panel.called & (panel.folds(3, 42) == fold_id)
        ref, cnt = _holdout_ref(panel.gk, p, q, held)
        a, b = fb.holdout_nll_f32(p, q), fb.holdout_nll_f32(p, q)
        assert a == b                                               # equal bits
        mean_nll, dev, n_eval = a
        assert n_eval == cnt == fb.holdout_observed
        ll = -0.5 * dev
        assert abs(ll - ref) <= 1e-6 * abs(ref)
        assert mean_nll == -ll / n_eval
        total_ll += ll
        total_n += n_eval
        fb.close()
    # the folds partition the called genotypes: their hold-out sums add up to the all-called value, count for count
    ref_all, cnt_all = _holdout_ref(panel.gk, p, q, panel.called)
    assert total_n == cnt_all and abs(total_ll - ref_all) <= 1e-6 * abs(ref_all)


@pytest.mark.parametrize("k", [1, 64])
def test_holdout_nll_k_edges(panel, k):
    p, q = _pq(panel.m, panel.n, k, 90 + k)
    fb = panel.s.make_cv_fold_backend(1, 2, 42)
    held = panel.called & (panel.folds(2, 42) == 1)
    ref, cnt = _holdout_ref(panel.gk, p, q, held)
    mean_nll, dev, n_eval = fb.holdout_nll_f32(p, q)
    assert n_eval == cnt and abs(-0.5 * dev - ref) <= 1e-6 * abs(ref)
    fb.close()


def test_holdout_nll_clamps_in_float64(panel):
    """P rows of exact zeros and exact ones against one-hot Q rows: rec is exactly 0 or 1 under any rounding, and calls of every
    kind meet both.  An f32 clamp at 1 - 1e-8 = 1 would leave ln(1 - rec) = ln 0; the f64 clamp keeps every term finite."""
    k = 3
    p = np.zeros((panel.m, k), dtype=np.float32)
    p[1::2] = 1.0
    q = np.zeros((panel.n, k), dtype=np.float32)
    q[np.arange(panel.n), np.arange(panel.n) % k] = 1.0
    rec = np.repeat(p[:, :1].astype(np.float64), panel.n, 1)
    fb = panel.s.make_cv_fold_backend(0, 2, 42)
    held = panel.called & (panel.folds(2, 42) == 0)
    for gv in (0.0, 1.0, 2.0):
        assert (held & (panel.gk == gv))[0::2].any() and (held & (panel.gk == gv))[1::2].any()
    ref, cnt = _holdout_ref(panel.gk, p, q, held, rec=rec)
    mean_nll, dev, n_eval = fb.holdout_nll_f32(p, q)
    assert n_eval == cnt and np.isfinite(mean_nll) and np.isfinite(dev)
    assert abs(-0.5 * dev - ref) <= 1e-12 * abs(ref)
    fb.close()


def test_sliced_panel(sliced):
    """Every loop of the three kernels takes more than one turn (see the fixture)."""
    c = sliced
    _check_counts(c, 5, 42)
    fb, _train, held = _check_fold_image(c, 1, 3, SEEDS[1])
    p, q = _pq(c.m, c.n, 5, 8)
    ref, cnt = _holdout_ref(c.gk, p, q, held)
    a, b = fb.holdout_nll_f32(p, q), fb.holdout_nll_f32(p, q)
    assert a == b and a[2] == cnt and abs(-0.5 * a[1] - ref) <= 1e-6 * abs(ref)
    fb.close()


def test_refusals(panel):
    s = panel.s
    with pytest.raises(RuntimeError, match="CVerror requires folds >= 2, got 1"):
        s.cv_observed_fold_counts(1, 42)
    with pytest.raises(RuntimeError, match="CVerror requires folds >= 2, got 1"):
        s.make_cv_fold_backend(0, 1, 42)
    with pytest.raises(RuntimeError, match=r"fold_id must be within \[0, 3\), got 3"):
        s.make_cv_fold_backend(3, 3, 42)
    with pytest.raises(RuntimeError, match="at most 256"):
        s.cv_observed_fold_counts(257, 42)
    with pytest.raises(RuntimeError, match="at most 256"):
        s.make_cv_fold_backend(0, 257, 42)
    with pytest.raises(ValueError, match="CVerror requires folds >= 2, got 1"):
        jx.admx_evaluate_cverror(s, 2, 1, 42, *FIT)
    # the library refuses by itself, before any launch
    from janusx_amd._lib import check, lib
    with pytest.raises(RuntimeError, match="folds must be at most 256"):
        check(lib().jxg_admx_cv_fold_counts(None, 0, 300, None, 10, 257, 0, None, None))
    with pytest.raises(RuntimeError, match=r"fold_id must be within \[0, 4\), got 4"):
        check(lib().jxg_admx_cv_fold_image(None, 0, 300, None, 10, None, 4, 0, 4, None, None, None))
    with pytest.raises(RuntimeError, match=r"K must be within \[1, 64\]"):
        check(lib().jxg_admx_cv_holdout_nll(None, 0, 300, None, 10, None, 4, 0, 1, 65, None, None, None, 0, None, None, None))
    fb = s.make_cv_fold_backend(0, 2, 42)
    p, q = _pq(panel.m + 1, panel.n, 2, 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        fb.holdout_nll_f32(p, q)
    fb.close()


def test_evaluate_cverror(panel):
    s, folds, seed, k = panel.s, 3, 42, 3
    fit = FIT[:9] + (30,) + FIT[10:]
    r = jx.admx_evaluate_cverror(s, k, folds, seed, *fit, keep_fits=True)
    ids = panel.folds(folds, seed)
    assert r["cv_folds"] == folds and r["cv_observed"] == int(panel.called.sum())
    assert np.array_equal(r["fold_counts"], np.bincount(ids[panel.called], minlength=folds))
    assert np.array_equal(r["fold_eval_counts"], r["fold_counts"])
    for i in range(folds):
        p, q = r["fold_p"][i], r["fold_q"][i]
        assert p.shape == (panel.m, k) and q.shape == (panel.n, k) and p.dtype == q.dtype == np.float32
        ref, cnt = _holdout_ref(panel.gk, p, q, panel.called & (ids == i))
        assert abs(r["fold_mean_nll"][i] - (-ref / cnt)) <= 1e-6 * abs(ref / cnt)
    means = np.asarray(r["fold_mean_nll"], dtype=np.float64)
    assert r["cverror"] == float(np.mean(means))
    assert r["cverror_se"] == float(np.std(means, ddof=1) / np.sqrt(folds))
    # fold i is fitted with the seed `seed + i + 1`
    fb = s.make_cv_fold_backend(1, folds, seed)
    p1, q1 = fb.fit_k(k, seed + 2, *fit)[:2]
    assert np.array_equal(p1, r["fold_p"][1]) and np.array_equal(q1, r["fold_q"][1])
    fb.close()
    r2 = jx.admx_evaluate_cverror(s, k, folds, seed, *fit, keep_fits=True)
    assert r2["cverror"] == r["cverror"] and r2["cverror_se"] == r["cverror_se"]
    assert np.array_equal(r2["fold_mean_nll"], r["fold_mean_nll"])
    for i in range(folds):
        assert np.array_equal(r2["fold_p"][i], r["fold_p"][i]) and np.array_equal(r2["fold_q"][i], r["fold_q"][i])
    assert "fold_p" not in jx.admx_evaluate_cverror(s, 1, 2, seed, *fit)


def _structured(n=N, m=M, k=3, seed=2027):
    """Three populations with independent uniform(0.05, 0.95) frequencies, 30 % of the samples admixed by a Dirichlet draw,
    1 % missing calls."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, (m, k))
    q = np.zeros((n, k))
    q[np.arange(n), rng.integers(0, k, n)] = 1.0
    mixed = rng.random(n) < 0.3
    q[mixed] = rng.dirichlet(np.ones(k), int(mixed.sum()))
    g = rng.binomial(2, p @ q.T).astype(np.int8)
    g[rng.random(g.shape) < 0.01] = -1
    return g


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """The simulation, its session, and the CV error and the plain fit of K = 1, 2, 3 (3 folds, seed 42), computed once."""
    c = _Case(tmp_path_factory.mktemp("admxcv_sim"), _structured(), "sim")
    cv = {k: jx.admx_evaluate_cverror(c.s, k, 3, 42, *FIT) for k in (1, 2, 3)}
    fits = {k: c.s.fit_k(k, 42, *FIT) for k in (1, 2, 3)}
    return c, cv, fits


def test_structured_simulation_prefers_the_true_k(sim):
    _c, cv, _fits = sim
    print("CVerror K=1, 2, 3:", [(cv[k]["cverror"], cv[k]["cverror_se"]) for k in (1, 2, 3)])
    assert cv[3]["cverror"] < cv[2]["cverror"] < cv[1]["cverror"]


def _untimed(text):
    return [ln for ln in text.splitlines() if not ln.startswith(("time:", "total seconds:", "CV time:"))]


def test_cli(sim, tmp_path):
    from janusx_amd import cli
    c, cv, fits = sim
    with_cv, plain = tmp_path / "cv", tmp_path / "plain"
    assert cli.main(["adamixture", "-bfile", c.prefix, "-k", "1..3", "-o", str(with_cv), "-max-iter", "200", "-cverror", "3"]) == 0
    assert cli.main(["adamixture", "-bfile", c.prefix, "-k", "1..3", "-o", str(plain), "-max-iter", "200"]) == 0
    lines = (with_cv / "sim.fastpop.cverror.summary.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["K", "CVerror", "CVerror_SE", "CV_folds", "WallTime_sec", "Q_output", "P_npy_output",
                                    "P_site_output", "Structure_plot", "Log_file"]
    assert len(lines) == 4
    for line, k in zip(lines[1:], (1, 2, 3)):
        f = line.split("\t")
        base = str(with_cv / f"sim.{k}")
        assert f[0] == str(k) and f[1] == f"{cv[k]['cverror']:.6f}" and f[2] == f"{cv[k]['cverror_se']:.6f}" and f[3] == "3"
        assert float(f[4]) > 0 and f[5:] == [base + ".Q.txt", base + ".P.npy", base + ".P.site", "", base + ".fastpop.log"]
        log = (with_cv / f"sim.{k}.fastpop.log").read_text().splitlines()
        assert f"CVerror: {cv[k]['cverror']:.6f} (SE={cv[k]['cverror_se']:.6f}, folds=3)" in log
        assert "CV fold sizes: " + ", ".join(f"F{i + 1}={int(v)}" for i, v in enumerate(cv[k]["fold_counts"])) in log
        assert "CV eval counts: " + ", ".join(f"F{i + 1}={int(v)}" for i, v in enumerate(cv[k]["fold_eval_counts"])) in log
    best = min((1, 2, 3), key=lambda k: cv[k]["cverror"])
    assert f"Best K by CVerror: K={best} " in (with_cv / "sim.fastpop.summary.log").read_text()
    # without the switch: no table, and every file is what the command wrote before the switch existed
    assert sorted(os.listdir(plain)) == sorted([f"sim.{k}.{e}" for k in (1, 2, 3) for e in ("Q.txt", "P.npy", "P.site", "fastpop.log")]
                                               + ["sim.fastpop.summary.log"])
    for k in (1, 2, 3):
        p, q, ll, it, init_ll, als_it = fits[k]
        base = str(plain / f"sim.{k}")
        for ext in ("Q.txt", "P.npy", "P.site"):
            assert (plain / f"sim.{k}.{ext}").read_bytes() == (with_cv / f"sim.{k}.{ext}").read_bytes()
        assert np.array_equal(np.load(base + ".P.npy"), p)
        assert _untimed((plain / f"sim.{k}.fastpop.log").read_text()) == [
            "command: adamixture", f"genotype: {c.prefix}", f"K scan progress: {k}/3 (K={k}, spec=1..3)", f"samples: {c.n}",
            f"kept SNPs: {c.m} (maf >= 0.02, missing rate <= 0.05, snps-only off)",
            "solver: adam-em  seed: 42  tol: 1e-05  max-iter: 200  check: 5",
            f"ALS rounds: {als_it}  init log-likelihood: {init_ll:.6f}",
            f"Adam-EM iterations: {it}  final log-likelihood: {ll:.6f}",
            "structure plot: not drawn (plots are not built)", f"outputs: {base}.Q.txt {base}.P.npy {base}.P.site"]
        assert _untimed((with_cv / f"sim.{k}.fastpop.log").read_text())[:8] == _untimed((plain / f"sim.{k}.fastpop.log").read_text())[:8]
    summary = _untimed((plain / "sim.fastpop.summary.log").read_text())
    assert summary[:5] == [f"genotype: {c.prefix}", f"samples: {c.n}", f"kept SNPs: {c.m}", "K spec: 1..3",
                           "K\tll_final\tinit_ll\tadam_iter\tals_iter\tseconds"]
    assert [ln.rsplit("\t", 1)[0] for ln in summary[5:]] == [
        f"{k}\t{fits[k][2]:.6f}\t{fits[k][4]:.6f}\t{fits[k][3]}\t{fits[k][5]}" for k in (1, 2, 3)]
