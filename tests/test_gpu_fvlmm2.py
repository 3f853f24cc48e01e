"""`jx fvlmm2` on the device (csrc/k_fvlmm2.hip, janusx.fvlmm2_assoc_chunk_f32 / fvlmm2_pairs_packed, cli.cmd_fvlmm2) against the
f64 restatement of tests/fvlmm2_ref.py.

Bar: the project's 1e-5 (beta against max(|beta|, se), se relative, p in the norm p / max(1, z^2)) on every row; the joint kernel on
given rows is expected near 1e-12 (same f32 rows on both sides, f64 sums in another order) and its measured maximum is printed.

The early-return pattern of src/stats/fvlmm2.rs:257-281 (a later coefficient's variance not finite and positive after an earlier one
was written) is covered by reading: with the 1e-6 ridge every diagonal element of the inverse of a factorised matrix is positive, and
no designed input reached the branch in the restatement."""
import os

import numpy as np
import pytest

import fvlmm2_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _null(n, p, seed):
    rng = np.random.default_rng(seed)
    s = rng.gamma(1.0, 1.0, size=n)
    xcov = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, max(p - 1, 0)))], axis=1)[:, :p]
    y = rng.normal(size=n)
    return s, np.ascontiguousarray(xcov), y, float(rng.uniform(-0.5, 0.5))


def _rows(n, rows, seed):
    rng = np.random.default_rng(seed + 1)
    g1 = rng.integers(0, 3, size=(rows, n)).astype(np.float32)
    g2 = rng.integers(0, 3, size=(rows, n)).astype(np.float32)
    return g1, g2, (g1 * g2).astype(np.float32)


_CASES = [(n, p) for n in (13, 63, 64, 65, 129, 257) for p in (0, 1, 3, 13) if n >= p + 3 + 8]


@pytest.mark.parametrize("n,p", _CASES)
def test_joint_kernel_is_the_restatement(n, p):
    import janusx_amd.janusx as jx
    s, xcov, y, l10 = _null(n, p, 100 * n + p)
    g1, g2, gc = _rows(n, 65, 100 * n + p)
    y = y + 0.4 * gc[0]                                   # one row with a signal
    ref = R.joint_rows(s, xcov, y, l10, g1, g2, gc)
    worst = 0.0
    for rows in (1, 5, 65):
        got = jx.fvlmm2_assoc_chunk_f32(s, xcov, y, l10, g1[:rows], g2[:rows], gc[:rows])
        assert got.shape == (rows, 9) and got.dtype == np.float64
        be, se, pe = R.errors(got, ref[:rows])
        worst = max(worst, be, se, pe)
        assert max(be, se, pe) < TOL, (n, p, rows, be, se, pe)
    print(f"fvlmm2 joint kernel n={n} p_cov={p}: max error {worst:.3e}")
    assert np.isfinite(ref).all()


def test_joint_kernel_takes_device_tensors_and_refuses_14_covariates():
    import torch
    import janusx_amd.janusx as jx
    n, p = 65, 3
    s, xcov, y, l10 = _null(n, p, 5)
    g1, g2, gc = _rows(n, 5, 5)
    host = jx.fvlmm2_assoc_chunk_f32(s, xcov, y, l10, g1, g2, gc)
    dev = jx.fvlmm2_assoc_chunk_f32(*(torch.from_numpy(a).cuda() for a in (s, xcov, y)), l10,
                                    *(torch.from_numpy(a).cuda() for a in (g1, g2, gc)))
    assert np.array_equal(host, dev)
    bad = torch.from_numpy(s.copy()).cuda()
    bad[7] = -10.0
    with pytest.raises(RuntimeError, match="S \\+ lambda must stay finite and positive for all samples"):
        jx.fvlmm2_assoc_chunk_f32(bad, torch.from_numpy(xcov).cuda(), torch.from_numpy(y).cuda(), l10, g1, g2, gc)
    # y[7] and x[3] both non-finite: sample 3 is met first, so the covariates are named, from host arrays and from device tensors
    yb, xb = y.copy(), xcov.copy()
    yb[7], xb[3, 1] = np.inf, np.nan
    for conv in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        with pytest.raises(RuntimeError, match="xcov contains non-finite values"):
            jx.fvlmm2_assoc_chunk_f32(conv(s), conv(xb), conv(yb), l10, g1, g2, gc)
        with pytest.raises(RuntimeError, match="y_rot contains non-finite values"):
            jx.fvlmm2_assoc_chunk_f32(conv(s), conv(xcov), conv(yb), l10, g1, g2, gc)
    s2, x14, y2, _ = _null(40, 14, 6)
    a1, a2, ac = _rows(40, 2, 6)
    with pytest.raises(RuntimeError, match="at most 13 covariate columns"):
        jx.fvlmm2_assoc_chunk_f32(s2, x14, y2, 0.0, a1, a2, ac)
    from janusx_amd._lib import lib
    t = [torch.from_numpy(a).cuda() for a in (a1, a2, ac, s2, x14, y2)]
    out = torch.zeros((2, 9), dtype=torch.float64, device="cuda")
    rc = lib().jxg_fvlmm2_joint(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 2, 40, 40, t[3].data_ptr(), t[4].data_ptr(), 14,
                                t[5].data_ptr(), 1.0, out.data_ptr(), None)
    assert rc != 0 and b"at most 13" in lib().jx_last_error()


def test_joint_kernel_designed_rows():
    import janusx_amd.janusx as jx
    n, p = 64, 2
    s, xcov, y, l10 = _null(n, p, 9)
    g1, g2, gc = _rows(n, 4, 9)
    g2[1, 17] = np.nan                                    # a NaN in g2: nine NaN
    gc[2, :] = 0.0                                        # an all-zero combo row: the ridge keeps the factorisation alive
    g1[3, 63] = np.inf
    with pytest.raises(RuntimeError, match="S \\+ lambda must stay finite and positive for all samples"):
        jx.fvlmm2_assoc_chunk_f32(np.where(np.arange(n) == 3, -100.0, s), xcov, y, l10, g1, g2, gc)
    got = jx.fvlmm2_assoc_chunk_f32(s, xcov, y, l10, g1, g2, gc)
    ref = R.joint_rows(s, xcov, y, l10, g1, g2, gc)
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all() and np.isfinite(got[0]).all()
    assert max(R.errors(got, ref)) < TOL
    # the zero row: beta_c = 0, se_c = sqrt(sigma^2 1e6), p_c = 1, the six other columns finite
    z = np.concatenate([xcov, g1[2][:, None], g2[2][:, None], gc[2][:, None]], axis=1).astype(np.float64)
    w = 1.0 / (s + 10.0 ** l10)
    a = (z.T * w) @ z + 1e-6 * np.eye(p + 3)
    res = y - z @ np.linalg.solve(a, (z.T * w) @ y)
    sigma2 = float(np.sum(w * res * res)) / (n - p - 3)
    assert got[2, 6] == 0.0 and got[2, 8] == 1.0 and np.isfinite(got[2, :6]).all()
    assert abs(got[2, 7] - np.sqrt(sigma2 * 1e6)) <= TOL * np.sqrt(sigma2 * 1e6)


# ---- combo kernel -------------------------------------------------------------------------------------------------------

def _panel_case(n, m, seed, missing=0.05):
    from janusx_amd import bed
    packed, g = bed.synth_panel_numpy(n, m, seed=seed, missing_rate=missing)
    rng = np.random.default_rng(seed)
    flip = rng.random(m) < 0.4
    maf = rng.uniform(0.0, 0.5, size=m).astype(np.float32)
    maf[:4] = np.array([0.25, 0.75, 1.25e-8, 0.125], dtype=np.float32)        # means 0.5, 1.5, 2.5e-8: the half-to-even ties
    return packed, g, flip, maf


@pytest.mark.parametrize("n", [127, 128, 129, 257])
@pytest.mark.parametrize("subset", [False, True])
def test_combo_kernel_bit_for_bit(n, subset):
    import torch
    import janusx_amd.janusx as jx
    from janusx_amd import fvlmm2 as f2
    from janusx_amd import pipeline as pl
    from janusx_amd._lib import check, lib
    m = 24
    packed, _g, flip, maf = _panel_case(n, m, 40 + n)
    rng = np.random.default_rng(n)
    sidx = np.sort(rng.choice(n, size=n - 30, replace=False)) if subset else None
    n_out = n if sidx is None else len(sidx)
    ops, neg1, neg2, r1, r2 = [], [], [], [], []
    for k, op in enumerate("*&|^" * 5):
        a, b = (k * 5) % m, (k * 7 + 3) % m
        ops.append(op)
        neg1.append(op != "*" and k % 3 == 1)
        neg2.append(op != "*" and k % 5 >= 3)
        r1.append(a)
        r2.append(b)
    r1, r2, neg1, neg2 = np.array(r1), np.array(r2), np.array(neg1), np.array(neg2)
    assert neg1.any() and neg2.any() and flip[r1].any() and not flip[r1].all()
    lut = jx._raw_additive_lut(maf, flip, True)
    tab, pos = f2.pair_tables(lut[r1], lut[r2], ops, neg1, neg2)
    panel = pl.Panel(torch.from_numpy(packed).cuda(), n, sidx)
    dev = panel.device
    nr = len(ops)
    for ld in (n_out, ((n_out + 3) // 4) * 4 + 4):         # rows of pitch n (the rotation's layout) and a padded pitch
        outs = [torch.full((nr, ld), -7.0, dtype=torch.float32, device=dev) for _ in range(3)]
        cnt = torch.zeros((nr, 3), dtype=torch.int32, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        t = [up(r1.astype(np.int32)), up(r2.astype(np.int32)), up(lut[r1]), up(lut[r2]), up(tab), up(pos.view(np.int32))]
        check(lib().jxg_fvlmm2_combo_p32(panel.p32.data_ptr(), panel.m, n_out, t[0].data_ptr(), t[1].data_ptr(), nr, t[2].data_ptr(),
                                         t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                         outs[2].data_ptr(), ld, cnt.data_ptr(), None))
        g1, g2, gc = (o.cpu().numpy() for o in outs)
        e1 = R.decode_rows(packed, n, r1, flip, maf, sidx)
        e2 = R.decode_rows(packed, n, r2, flip, maf, sidx)
        ec, af1, af2, afc = R.combo_rows(e1, e2, ops, neg1, neg2)
        for got, exp in ((g1, e1), (g2, e2), (gc, ec)):
            assert got[:, :n_out].tobytes() == exp.tobytes()
            assert (got[:, n_out:] == -7.0).all()                          # nothing is written beyond n
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:, 0], np.rint(af1 * n_out).astype(np.int64))
        assert np.array_equal(c[:, 1], np.rint(af2 * n_out).astype(np.int64))
        assert np.array_equal(c[:, 2], np.rint(afc * n_out).astype(np.int64))
        assert np.array_equal(c[:, 0], (R.literalize(e1, neg1) > 0).sum(axis=1))


# ---- pairs over a packed payload ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pairs_case():
    import torch
    from janusx_amd import bed
    from janusx_amd import pipeline as pl
    n, m = 257, 300
    packed, g = bed.synth_panel_numpy(n, m, seed=77, missing_rate=0.01, maf_low=0.2, maf_high=0.45)
    rng = np.random.default_rng(77)
    r1 = np.array([3, 10, 21, 40, 77, 150, 299])
    r2 = np.array([5, 11, 200, 41, 78, 151, 0])
    ops = ["*", "&", "|", "^", "*", "&", "*"]
    neg1 = np.array([False, True, False, False, False, False, False])
    neg2 = np.array([False, False, True, True, False, False, False])
    ga, gb = (np.where(g[r] < 0, 1, g[r]).astype(np.float64) for r in (3, 5))
    y = 0.9 * ga * gb + rng.normal(size=n)                              # planted g_a g_b effect on pair 0
    x = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 1))], axis=1)
    pk = torch.from_numpy(packed).cuda()
    k, _eff, _ = pl.build_grm(pk, n, 1, 0.02, 0.05)
    model = pl.trait_null_model(k, None, x, y)
    counts = pl.Panel(pk, n).counts()
    maf = ((counts[:, 1] + 2.0 * counts[:, 2]) / (2.0 * np.maximum(n - counts[:, 0], 1))).astype(np.float32)
    flip = np.zeros(m, dtype=bool)
    flip[[10, 200, 299]] = True
    return dict(n=n, packed=packed, r1=r1, r2=r2, ops=ops, neg1=neg1, neg2=neg2, model=model, maf=maf, flip=flip)


def _pairs_reference(c):
    m = c["model"]
    ut = m.ut.cpu().numpy().astype(np.float64)
    e1 = R.decode_rows(c["packed"], c["n"], c["r1"], c["flip"], c["maf"])
    e2 = R.decode_rows(c["packed"], c["n"], c["r2"], c["flip"], c["maf"])
    ec, af1, af2, afc = R.combo_rows(e1, e2, c["ops"], c["neg1"], c["neg2"])
    rot = [a.astype(np.float64) @ ut.T for a in (e1, e2, ec)]            # f64 rotation with the same U^T
    ref = R.joint_rows(m.S.cpu().numpy(), m.xcov.cpu().numpy(), m.y.cpu().numpy(), np.log10(m.null.lbd), *rot)
    return ref, af1, af2, afc


def test_pairs_packed_against_rotated_restatement(pairs_case):
    import janusx_amd.janusx as jx
    c = pairs_case
    m = c["model"]
    res = jx.fvlmm2_pairs_packed(c["packed"], c["n"], c["flip"], c["maf"], c["r1"], c["r2"], c["ops"], c["neg1"], c["neg2"], m.S, m.xcov,
                                 m.y, m.ut, float(np.log10(m.null.lbd)), batch_size=3)
    ref, af1, af2, afc = _pairs_reference(c)
    got = np.stack([res[k] for k in ("beta1", "se1", "p1", "beta2", "se2", "p2", "beta_combo", "se_combo", "p_combo")], axis=1)
    be, se, pe = R.errors(got, ref)
    z2 = (ref[:, 0::3] / ref[:, 1::3]) ** 2
    raw = np.abs(got[:, 2::3] - ref[:, 2::3]) / ref[:, 2::3]
    print(f"fvlmm2_pairs_packed: beta {be:.3e} se {se:.3e} p/max(1,z2) {pe:.3e} raw p (z2<=10) {raw[z2 <= 10].max():.3e}")
    assert int((z2[:, 2] > 10).sum()) >= 1 and int((z2[:, 2] <= 10).sum()) >= 3, z2[:, 2]
    assert max(be, se, pe) < TOL, (be, se, pe)
    assert raw[z2 <= 10].max() < TOL
    for key, exp in (("af1", af1), ("af2", af2), ("combo_af", afc)):
        assert np.array_equal(res[key], exp), key
    # one batch or many: the same rows
    one = jx.fvlmm2_pairs_packed(c["packed"], c["n"], c["flip"], c["maf"], c["r1"], c["r2"], c["ops"], c["neg1"], c["neg2"], m.S, m.xcov,
                                 m.y, m.ut, float(np.log10(m.null.lbd)), batch_size=4096)
    assert all(np.array_equal(one[k], res[k], equal_nan=True) for k in res)
    with pytest.raises(ValueError, match="Negated literals are not supported"):
        jx.fvlmm2_pairs_packed(c["packed"], c["n"], c["flip"], c["maf"], [1], [2], "*", [True], [False], m.S, m.xcov, m.y, m.ut, 0.0)


def test_rotation_is_what_differs_from_the_literal_mirror():
    """The documented difference: the command rotates the pair rows; the mirror function, like the reference's script, uses the rows it
    is given.  With a dense V = K + lambda I at n = 64 the rotated route is the GLS solve (Z'V^-1 Z + 1e-6 I)^-1, the unrotated
    one is not."""
    import torch
    import janusx_amd.janusx as jx
    from janusx_amd import bed
    from janusx_amd import pipeline as pl
    n, m = 64, 200
    packed, g = bed.synth_panel_numpy(n, m, seed=5, maf_low=0.2, maf_high=0.45)
    rng = np.random.default_rng(5)
    y = rng.normal(size=n) + 0.5 * g[7]
    x = np.ones((n, 1))
    pk = torch.from_numpy(packed).cuda()
    k, _eff, _ = pl.build_grm(pk, n, 1, 0.02, 0.05)
    model = pl.trait_null_model(k, None, x, y)
    lbd = float(model.null.lbd)
    r1, r2 = np.array([7, 20, 33]), np.array([9, 21, 150])
    maf = (g.mean(axis=1) / 2.0).astype(np.float32)
    flip = np.zeros(m, dtype=bool)
    res = jx.fvlmm2_pairs_packed(packed, n, flip, maf, r1, r2, "*", [False] * 3, [False] * 3, model.S, model.xcov, model.y, model.ut,
                                 np.log10(lbd))
    e1, e2 = R.decode_rows(packed, n, r1, flip, maf), R.decode_rows(packed, n, r2, flip, maf)
    ec = (e1 * e2).astype(np.float32)
    literal = jx.fvlmm2_assoc_chunk_f32(model.S, model.xcov, model.y, np.log10(lbd), e1, e2, ec)
    # dense GLS with V = U (S + lambda) U'
    ut = model.ut.cpu().numpy().astype(np.float64)
    vinv = ut.T @ np.diag(1.0 / (model.S.cpu().numpy() + lbd)) @ ut
    for r in range(3):
        z = np.concatenate([x, e1[r][:, None], e2[r][:, None], ec[r][:, None]], axis=1).astype(np.float64)
        ainv = np.linalg.inv(z.T @ vinv @ z + 1e-6 * np.eye(4))
        beta = ainv @ (z.T @ vinv @ y)
        rr = y - z @ beta
        se = np.sqrt(float(rr @ vinv @ rr) / (n - 4) * np.diag(ainv))
        for t, (bk, sk) in enumerate((("beta1", "se1"), ("beta2", "se2"), ("beta_combo", "se_combo"))):
            eb = abs(res[bk][r] - beta[1 + t]) / max(abs(beta[1 + t]), se[1 + t])
            es = abs(res[sk][r] - se[1 + t]) / se[1 + t]
            print(f"fvlmm2 rotated route against dense GLS, pair {r} {bk}: beta {eb:.3e} se {es:.3e}")
            assert eb <= TOL and es <= TOL, (r, bk, eb, es)        # the project's bar: both sides use the same f32 U^T
        assert abs(literal[r, 7] - se[3]) > 1e-2 * se[3] or abs(literal[r, 6] - beta[3]) > 1e-2 * se[3]


# ---- end to end -----------------------------------------------------------------------------------------------------------

def _tsv_close(got_lines, exp_lines):
    """Text against the restatement's rendering: a row may differ by a flip of the last printed digit of a 4-decimal field (bounded in
    count) and, in the 4-digit scientific fields, by what 1e-5 on beta / se allows (p moves by z^2 1e-5 relative)."""
    assert len(got_lines) == len(exp_lines)
    flips = 0
    for got, exp in zip(got_lines, exp_lines):
        if got == exp:
            continue
        fg, fe = got.split("\t"), exp.split("\t")
        assert len(fg) == len(fe) == 11 and fg[:3] == fe[:3] and fg[4] == fe[4], (got, exp)
        for col in (3, 5, 6):
            if fg[col] != fe[col]:
                assert abs(float(fg[col]) - float(fe[col])) <= 1.0001e-4, (col, got, exp)
                flips += 1
        for col in (7, 8, 9, 10):
            if fg[col] != fe[col]:
                a, b = float(fg[col]), float(fe[col])
                assert abs(a - b) <= 2.1e-4 * abs(b), (col, got, exp)   # half a unit of the 5th digit on each side + the bar
    assert flips <= max(2, len(got_lines) // 20), flips


def test_cli_end_to_end(tmp_path, capsys):
    import torch
    import janusx_amd.janusx as jx
    from janusx_amd import bed, cli
    from janusx_amd import pipeline as pl
    n, m = 257, 300
    packed, g = bed.synth_panel_numpy(n, m, seed=91, missing_rate=0.01, maf_low=0.1, maf_high=0.45)
    g_mono = np.zeros(n, dtype=np.int8)
    packed[50] = bed.pack_dosage(g_mono[None, :])[0]                     # a monomorphic site: filtered, so its name does not resolve
    ids = [f"s{i}" for i in range(n)]
    bim = bed.Bim([str(1 + j // 150) for j in range(m)], [f"rs{j}" if j != 12 else "." for j in range(m)], [1000 + 10 * j for j in range(m)],
                  ["A"] * m, ["G"] * m)
    prefix = str(tmp_path / "panel")
    bed.write_bed(prefix, packed, ids, bim)
    rng = np.random.default_rng(91)
    gq = np.where(g < 0, 1, g).astype(np.float64)
    y = 0.8 * gq[3] * gq[5] + rng.normal(size=n)
    y[[4, 100]] = np.nan
    with open(tmp_path / "ph.tsv", "w") as fh:
        fh.write("id\tT1\n" + "".join(f"{ids[i]}\t{'NA' if np.isnan(y[i]) else repr(float(y[i]))}\n" for i in range(n)))
    with open(tmp_path / "pairs.txt", "w") as fh:
        fh.write("# pairs\nrs3*rs5 note\n\n!rs10&rs11\nrs20|!!rs21\n1_1120^!rs40\nrs50*rs51\n!rs1*rs2\nrs7+rs8\nnope&rs1\nrs77*rs78\n")
    out = str(tmp_path / "res")
    assert cli.main(["fvlmm2", "-bfile", prefix, "-p", str(tmp_path / "ph.tsv"), "-i", str(tmp_path / "pairs.txt"), "-o", out,
                     "--batch-size", "2"]) == 0
    skip = open(out + ".fvlmm2.skip").read().splitlines()
    assert skip == ["line\texpr\treason",
                    "7\trs50*rs51\t\"\"\"SNP token 'rs50' was not found among active filtered variants.\"\"\"",
                    "8\t!rs1*rs2\tnegated_literals_not_supported_for_multiplicative_interaction",
                    "9\trs7+rs8\tinvalid_expression",
                    "10\tnope&rs1\t\"\"\"SNP token 'nope' was not found among active filtered variants.\"\"\""]
    lines = open(out + ".T1.fvlmm2.tsv").read().splitlines()
    assert lines[0] == R.HEADER and len(lines) == 6
    # the restatement on the same active set, null model and f64 rotation
    pk_k, _miss, maf, _std, flip, keep, _n, _tot = jx.prepare_bed_2bit_packed(prefix, 0.02, 0.05, 1.0)
    active = np.nonzero(keep)[0]
    assert 50 not in active
    loc = {int(a): i for i, a in enumerate(active)}
    keep_idx = np.array([i for i in range(n) if np.isfinite(y[i])])
    pk = torch.from_numpy(np.ascontiguousarray(pk_k)).cuda()
    k, _eff, _ = pl.build_grm(pk, n, 1, 0.02, 0.05)
    model = pl.trait_null_model(k, keep_idx, np.ones((len(keep_idx), 1)), y[keep_idx])
    specs = [(3, "*", 5, False, False, "rs3*rs5"), (10, "&", 11, True, False, "!rs10&rs11"), (20, "|", 21, False, False, "rs20|rs21"),
             (12, "^", 40, False, True, "1_1120^!rs40"), (77, "*", 78, False, False, "rs77*rs78")]
    r1 = np.array([loc[s[0]] for s in specs])
    r2 = np.array([loc[s[2]] for s in specs])
    e1 = R.decode_rows(pk_k, n, r1, flip, maf, keep_idx)
    e2 = R.decode_rows(pk_k, n, r2, flip, maf, keep_idx)
    ec, _a1, _a2, afc = R.combo_rows(e1, e2, [s[1] for s in specs], [s[3] for s in specs], [s[4] for s in specs])
    ut = model.ut.cpu().numpy().astype(np.float64)
    ref = R.joint_rows(model.S.cpu().numpy(), model.xcov.cpu().numpy(), model.y.cpu().numpy(), np.log10(model.null.lbd),
                       *(a.astype(np.float64) @ ut.T for a in (e1, e2, ec)))
    exp = R.render_rows([bim.chrom[s[0]] for s in specs], [bim.pos[s[0]] for s in specs], [s[5] for s in specs], afc, ref, R.bh(ref[:, 8]))
    _tsv_close(lines[1:], exp)
    # -among: 4 names -> 6 rows in ascending active-row order, after the rows of -i; -pmax keeps the FDR of the unfiltered run
    with open(tmp_path / "among.txt", "w") as fh:
        fh.write("rs30\nrs3\nrs5\nrs9\n")
    with open(tmp_path / "one.txt", "w") as fh:
        fh.write("rs77*rs78\n")
    out2 = str(tmp_path / "res2")
    assert cli.main(["fvlmm2", "-bfile", prefix, "-p", str(tmp_path / "ph.tsv"), "-i", str(tmp_path / "one.txt"), "-among",
                     str(tmp_path / "among.txt"), "--op", "*", "-o", out2, "--n-tests", "40"]) == 0
    full = [ln.split("\t") for ln in open(out2 + ".T1.fvlmm2.tsv").read().splitlines()[1:]]
    assert [f[2] for f in full] == ["rs77*rs78", "rs3*rs5", "rs3*rs9", "rs3*rs30", "rs5*rs9", "rs5*rs30", "rs9*rs30"]
    assert not os.path.exists(out2 + ".fvlmm2.skip")
    assert full[1][5:8] == lines[1].split("\t")[5:8]                       # the same pair gives the same statistics
    out3 = str(tmp_path / "res3")
    assert cli.main(["fvlmm2", "-bfile", prefix, "-p", str(tmp_path / "ph.tsv"), "-i", str(tmp_path / "one.txt"), "-among",
                     str(tmp_path / "among.txt"), "-o", out3, "--n-tests", "40", "-pmax", "0.05"]) == 0
    part = [ln.split("\t") for ln in open(out3 + ".T1.fvlmm2.tsv").read().splitlines()[1:]]
    want = [f for f in full if float(f[7]) <= 0.05]
    assert 1 <= len(part) < len(full) and part == want
    capsys.readouterr()
