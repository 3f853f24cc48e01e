"""Host tests of `jx reml` (no GPU): the numpy restatement (tests/aireml_ref.py) against its own first-order conditions, the probe
signs, the refusals of `janusx.ai_reml_multi_f64`, the host logic of `blup.BLUP` with the device fitter replaced by the
restatement, the command's refusals and the C ABI table."""
import os
import re

import numpy as np
import pytest

import aireml_ref as R

from janusx_amd import _lib, blup, cli
from janusx_amd import janusx as jx
from janusx_amd import pipeline


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fit64():
    ks, x, y, _th = R.make_case(64, 2, 2)
    log = []
    out = R.ai_reml_multi_f64(ks, x, y, trace_probes=0, log=log)
    return ks, x, y, out, log


def test_restatement_stationary_and_scale_free(fit64):
    """At the theta the restatement returns for (64, 2, 2): the central-difference gradient of REML() along the q log-ratio
    directions is zero to the accuracy of the differences, and the objective is flat along theta -> c theta.  Step h = 1e-4 in
    log theta: the truncation error is h^2 f''' / 6 ~ 1e-8 x O(n), the rounding error eps |f| / h ~ 1e-10; the iteration stops at
    a relative change of 1e-6, which leaves a gradient of ~ 1e-6 x curvature (O(n)).  Bound: 1e-3, i.e. 1e-5 n with n = 64
    rounded up; a wrong score (a sign, a factor 2) leaves a gradient of order 1 - 10."""
    ks, x, y, (theta, _ml, reml, _it, conv), _log = fit64
    assert conv
    klist = [ks[0], ks[1]]
    yc = y.reshape(-1, 1)
    f0 = R.REML(theta, yc, x, klist)
    assert abs(f0 + reml) <= 1e-9 * max(1.0, abs(reml))         # REML() is minus the reported value (blup.py:222-226)
    h = 1e-4
    for j in range(2):
        up, dn = theta.copy(), theta.copy()
        up[j] *= np.exp(h)
        dn[j] *= np.exp(-h)
        grad = (R.REML(up, yc, x, klist) - R.REML(dn, yc, x, klist)) / (2.0 * h)
        assert abs(grad) <= 1e-3, (j, grad)
    for c in (0.5, 3.0, 100.0):
        assert abs(R.REML(c * theta, yc, x, klist) - f0) <= 1e-9 * max(1.0, abs(f0))


def test_restatement_margins_are_reported(fit64):
    """The log of acceptance and stopping margins the GPU tests rely on: no halving in this case, the stop two steps apart."""
    *_rest, out, log = fit64
    assert out[4] and out[3] == len(log)
    assert sum(r["halvings"] for r in log) == 0
    assert log[-1]["rel_max"] < 1e-6 < log[-2]["rel_max"]


# ---- probes ----------------------------------------------------------------------------------------------------------------------

# the first 8 entries of probes 0 and 1 at n = 8, seed 42, as this build's ChaCha12 restatement gives them: they pin
# `_stdrng_words`' stream and the bit rule, not the rand crate (oracle/jx_oracle.py:805-811 -- parity unpinned)
PINNED_SIGNS = [[1, 1, 1, -1, -1, -1, 1, 1], [-1, -1, 1, 1, -1, -1, 1, -1]]


def test_probe_signs_rule_and_pin():
    n, probes = 8, 2
    s = jx._reml_probe_signs(n, probes, 42)
    assert s.shape == (probes, n) and s.dtype == np.float64
    w = jx._stdrng_words(42, 2 * n * probes).astype(np.uint64)
    u64 = w[0::2] | (w[1::2] << np.uint64(32))                  # next_u64 of a block generator: low word first
    u = (u64 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert np.array_equal(s.reshape(-1), np.where(u < 0.5, -1.0, 1.0))
    assert s.astype(int).tolist() == PINNED_SIGNS
    big = jx._reml_probe_signs(769, 3, 42)                      # probe-major, then sample: a prefix of the stream is a prefix
    assert np.array_equal(big.reshape(-1)[:16], jx._reml_probe_signs(16, 1, 42).reshape(-1))
    assert set(np.unique(big)) == {-1.0, 1.0}


# ---- refusals of the mirror -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k_shape,x_shape,y_len,msg", [
    ((4, 4), (4, 1), 4, "k_stack must be 3D (q, n, n)"),
    ((1, 4, 5), (4, 1), 4, "k_stack must be (q, n, n)"),
    ((0, 4, 4), (4, 1), 4, "k_stack requires at least one kernel"),
    ((1, 4, 4), (4, 1), 5, "len(y) must equal n in k_stack"),
    ((1, 4, 4), (3, 1), 4, "xcov.n_rows must equal n in k_stack"),
    ((1, 4, 4), (4, 0), 4, "xcov must have at least one column"),
    ((1, 4, 4), (4, 4), 4, "n must be > p in xcov"),
])
def test_ai_reml_refusals(monkeypatch, k_shape, x_shape, y_len, msg):
    def no_device(*a, **k):
        raise AssertionError("a refused call reached the device layer")
    monkeypatch.setattr(pipeline, "MultiKernelReml", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        jx.ai_reml_multi_f64(np.zeros(k_shape), np.zeros(x_shape), np.zeros(y_len))


# ---- BLUP host logic --------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def host_fitter(monkeypatch):
    monkeypatch.setattr(pipeline, "MultiKernelReml", R.MultiKernelRemlRef)


@pytest.fixture(scope="module")
def blup_case():
    return R.make_blup_case(96, 6)


def test_blup_matches_restatement_on_host(host_fitter, blup_case):
    y, xc, z, gs = blup_case
    b = blup.BLUP(y, X=xc, Z=z, G=gs, progress=False)
    r = R.blup_fit(y, X=xc, Z=z, G=gs)
    assert b.route == "aireml" and r.route == "aireml" and b.result.message == "ai_reml"
    assert b._g_scales == pytest.approx([np.mean(np.diag(g)) + 1e-8 for g in gs], rel=1e-15)      # normalisation scales
    assert b.onehot_info == [(1, 0.0, 1.0)]                                                       # one-hot detected
    np.testing.assert_allclose(b.theta, r.theta, rtol=1e-9)
    np.testing.assert_allclose(b.var, r.var, rtol=1e-9)
    gn, _ = R.normalize_G(gs)
    expect_var = [b.theta[0] * np.mean(np.diag(z @ z.T))] + [b.theta[1 + i] * np.mean(np.diag(gn[i])) for i in range(2)] + [b.theta[3]]
    np.testing.assert_allclose(b.var, expect_var, rtol=1e-12)
    for mine, ref in ((b.beta, r.beta), (b.u, r.u), (b.g, r.g), (b.fitted, r.fitted), (b.residuals, r.residuals),
                      (b._cov_beta, r.cov_beta)):
        np.testing.assert_allclose(mine, ref, rtol=1e-7, atol=1e-9)
    assert b.beta.shape == (2, 1) and len(b.g_by_G) == 2 and b.u_by_Z[0].shape == (z.shape[1], 1)


def test_blup_standardises_a_dense_z(host_fitter, blup_case):
    y, xc, _z, gs = blup_case
    zd = np.random.default_rng(5).standard_normal((len(y), 7))
    b = blup.BLUP(y, X=xc, Z=zd, G=gs[0], progress=False)
    q, mean, std = b.onehot_info[0]
    assert q == 7.0
    np.testing.assert_allclose(mean, zd.mean(axis=0))
    np.testing.assert_allclose(std, zd.std(axis=0) + 1e-8)
    r = R.blup_fit(y, X=xc, Z=zd, G=gs[0])
    np.testing.assert_allclose(b.fitted, r.fitted, rtol=1e-7, atol=1e-9)


def test_blup_fallback_when_not_converged(host_fitter, blup_case, monkeypatch):
    y, xc, z, gs = blup_case
    calls = []
    real = jx.ai_reml_multi_f64

    def not_converged(*a, **k):
        calls.append(k.get("trace_probes"))
        th, ml, reml, nit, _conv = real(*a, **k)
        return th, ml, reml, nit, False
    monkeypatch.setattr(jx, "ai_reml_multi_f64", not_converged)
    b = blup.BLUP(y, X=xc, Z=z, G=gs, progress=False)
    assert calls == [0] and b.route == "lbfgsb" and hasattr(b.result, "nit") and b.result.message != "ai_reml"
    r = R.blup_fit(y, X=xc, Z=z, G=gs, force_fallback=True)
    np.testing.assert_allclose(b.theta / b.theta[-1], r.theta / r.theta[-1], rtol=1e-3)
    np.testing.assert_allclose(b.fitted, r.fitted, rtol=1e-3, atol=1e-4)


def test_blup_probe_dispatch():
    assert [blup.trace_probes_for(n) for n in (10, 768, 769, 2048, 2049)] == [0, 0, 16, 16, 12]
    assert [blup.trace_probes_for(n, exact_trace=True) for n in (768, 769, 5000)] == [0, 0, 0]


def test_blup_predict_shapes_and_no_random_effect(host_fitter, blup_case):
    y, xc, z, gs = blup_case
    n = len(y)
    b = blup.BLUP(y, X=xc, Z=z, G=gs, progress=False)
    np.testing.assert_allclose(b.predict(X=xc, Z=z, G=gs), b.fitted, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b.predict(X=xc), b.fitted, rtol=1e-10, atol=1e-12)                  # in-sample, stored effects
    out = b.predict(X=xc[:5], Z=z[:5], G=[g[:5] for g in gs])
    assert out.shape == (5, 1)
    np.testing.assert_allclose(out, b.fitted[:5], rtol=1e-10, atol=1e-12)
    with pytest.raises(ValueError, match="G is required for out-of-sample prediction"):
        b.predict(X=xc[:5], Z=z[:5])
    with pytest.raises(ValueError, match="G count mismatch"):
        b.predict(X=xc[:5], Z=z[:5], G=gs[0][:5])
    with pytest.raises(ValueError, match="columns mismatch"):
        b.predict(X=xc[:5], Z=z[:5, :-1], G=[g[:5] for g in gs])
    lm = blup.BLUP(y, X=xc, progress=False)                                                       # plain least squares
    x1 = np.column_stack([np.ones(n), xc])
    np.testing.assert_allclose(lm.beta[:, 0], np.linalg.lstsq(x1, y, rcond=None)[0], rtol=1e-10)
    assert lm.theta is None and lm.route == "lm" and lm.predict(X=xc[:4]).shape == (4, 1)


def test_blup_refused_inputs(host_fitter, blup_case):
    from scipy import sparse
    y, xc, z, gs = blup_case
    n = len(y)
    with pytest.raises(TypeError, match="sparse Z"):
        blup.BLUP(y, X=xc, Z=sparse.csr_matrix(z), progress=False)
    with pytest.raises(TypeError, match="sparse"):
        blup.BLUP(y, X=sparse.csr_matrix(xc.reshape(-1, 1)), G=gs[0], progress=False)
    with pytest.raises(ValueError, match="Row number of X"):
        blup.BLUP(y, X=np.zeros((n + 1, 2)), G=gs[0], progress=False)
    with pytest.raises(ValueError, match="Row number of Z0"):
        blup.BLUP(y, Z=np.zeros((n + 1, 2)), progress=False)
    with pytest.raises(ValueError, match=r"must be square \(n,n\)"):
        blup.BLUP(y, G=np.zeros((n, n + 1)), progress=False)
    with pytest.raises(ValueError, match="invalid mean diagonal"):
        blup.BLUP(y, G=-np.eye(n), progress=False)


# ---- command ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,msg", [
    (["-gxe"], "-gxe is not built"),
    (["-gxc", "env"], "-gxc is not built"),
    (["-spk", "x.npz"], "-spk is not built"),
    (["--spk-mode", "lowrank"], "--spk-mode is not built"),
    (["-c", "age:sex"], "interaction term 'age:sex'"),
    (["-rc", "block:year"], "interaction term 'block:year'"),
])
def test_cli_refusals_touch_no_file(monkeypatch, tmp_path, extra, msg):
    import builtins

    def no_open(*a, **k):
        raise AssertionError(f"a refused command opened {a[0]!r}")
    argv = ["reml", "-p", str(tmp_path / "absent.tsv"), "-n", "y", "-k", str(tmp_path / "absent.npy"), "-o", str(tmp_path / "o" / "out")]
    monkeypatch.setattr(builtins, "open", no_open)
    monkeypatch.setattr(np, "load", no_open)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + extra)
    assert msg in str(e.value)
    monkeypatch.undo()
    assert not os.path.exists(tmp_path / "o")


def test_cli_refuses_repeated_ids_and_text_covariates(tmp_path, monkeypatch):
    monkeypatch.setattr(cli, "_dist_setup", lambda: (0, 1))
    ph = tmp_path / "p.tsv"
    ph.write_text("id\ty\tsex\tblock\ns1\t1.0\tF\ta\ns2\t2.0\tM\tb\ns1\t3.0\tF\ta\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["reml", "-p", str(ph), "-n", "y", "-rc", "block", "-o", str(tmp_path / "out")])
    assert "occurs more than once" in str(e.value) and "line x environment" in str(e.value)
    ph.write_text("id\ty\tsex\tblock\ns1\t1.0\tF\ta\ns2\t2.0\tM\tb\ns3\t3.0\tF\ta\n")
    with pytest.raises(SystemExit) as e:
        cli.main(["reml", "-p", str(ph), "-n", "y", "-c", "sex", "-rc", "block", "-o", str(tmp_path / "out")])
    assert "is not numeric" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["reml", "-p", str(ph), "-n", "y", "-o", str(tmp_path / "out")])
    assert "at least one random term" in str(e.value)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_abi_names_and_header():
    names = ["jxg_potrf_block", "jxg_dpotrf_lower_f64", "jxg_dpotrs_lower_f64", "jxg_reml_combine_f64", "jxg_sym_dot_f64",
             "jxg_potrf_logdet_f64"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jxgpu.h")).read()
    for nm in names:
        assert nm in _lib.SIGNATURES
        proto = re.search(r"\bint " + nm + r"\(([^;]*)\);", header)
        assert proto, nm
        args = [a for a in proto.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[nm]), nm
