"""Trait-level LMM (`jx gwas -lmm -trait-level-lmm`): the trait-batched, workgroup-cooperative chain kernel
(`jxg_lmm_traits_chain_tab`, csrc/k_scan_fast.hip) on synthetic rotated rows, then `pipeline.scan_rows_lmm_traits`,
`pipeline.run_traits_lmm`, the mirror `lmm_trait_assoc_packed` and the command line.  Norms and bars of tests/test_gpu_parity.py
(beta / SE / Wald p within 1e-5 of the oracle, NaN pattern identical); Brent trajectories as
`test_warm_start_chain_device_pipeline_matches_trajectories` (evaluation counts equal on > 99.5 % of the rows)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOW, HIGH, MAX_ITER, TOL_BRENT = -5.0, 5.0, 50, 1e-2
M_ROWS, T_MAX = 1500, 5


def _parity():
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import test_gpu_parity as P
    return P


def _dev():
    import torch
    return torch.device("cuda", 0)


def _chains():
    """An empty chain, a one-row chain, four blocks of 256 rows cut into 4 pieces each, one long chain for the rest."""
    co = [0, 0, 1]
    for b in range(4):
        co += [1 + 256 * b + 64 * (q + 1) for q in range(4)]
    co.append(M_ROWS)
    return np.asarray(co, dtype=np.int64)


ZERO_ROWS = (65, 129, 130, 400, 401, 1025, 1300, 1301)     # heads of chains (65, 129, 1025) and two in a row in mid-chain


@functools.lru_cache(maxsize=None)
def _case(n, p):
    """Random positive S, X~ (intercept-like column + p - 1 others), five y~, m = 1500 f32 rows with all-zero rows; per trait the
    oracle's table and evaluation counts along the chains from the carried states `carry0` (NaN for the even chains, the
    trait's own start for the odd ones).  Built once per (n, p) and left unchanged."""
    from oracle import jx_oracle_c as OC
    OC.build()
    rng = np.random.default_rng(1000 * n + p)
    s = np.sort(rng.gamma(0.7, 1.5, size=n))[::-1].copy() + 1e-6
    x = rng.normal(size=(n, p))
    x[:, 0] = rng.normal(1.0, 0.3, size=n)
    g = rng.normal(size=(M_ROWS, n)).astype(np.float32)
    g[list(ZERO_ROWS)] = 0.0
    # every trait clearly polygenic (variance c^2 s + 1 along the eigenvectors: lambda0 = 1 / c^2 between 1 / 8 and 1.4).  A trait
    # without polygenic variance has its optimum at the upper bound, where the objective is flat to rounding and the
    # comparisons of Brent's search are decided by rounding noise in ANY evaluation order (measured on such a trait at n = 150:
    # the existing one-wave entry and this kernel left the oracle's trajectory on the same 7 rows, beta off by 2.4e-5 on both)
    csq = (1.0, 2.0, 4.0, 8.0, 0.7)
    Y = np.stack([np.sqrt(csq[t] * s) * rng.normal(size=n) + rng.normal(size=n) + 0.3 * g[7 + t] for t in range(T_MAX)])
    co = _chains()
    nch = len(co) - 1
    init = np.array([-1.5, 0.0, 0.7, 2.0, -3.0])
    carry0 = np.full((T_MAX, nch), np.nan)
    carry0[:, 1::2] = init[:, None]
    ref = np.zeros((T_MAX, M_ROWS, 3))
    ev = np.zeros((T_MAX, M_ROWS), dtype=np.int32)
    for t in range(T_MAX):
        for c in range(nch):
            a, b = int(co[c]), int(co[c + 1])
            if b > a:
                ref[t, a:b], ev[t, a:b] = OC.lmm_scan_rotated_block(g[a:b], s, x, Y[t], LOW, HIGH, MAX_ITER, TOL_BRENT, warm=2,
                                                                   init=float(carry0[t, c]), return_evals=True)
    for a in (ref, ev, carry0, g, s, x, Y, co):
        a.setflags(write=False)
    return dict(n=n, p=p, s=s, x=x, Y=Y, g=g, co=co, carry0=carry0, ref=ref, ev=ev)


class _Device:
    """The shared inputs of a case on the device and the traits' table workspaces."""

    def __init__(self, c, traits):
        import torch
        from janusx_amd._lib import check, lib
        dev = _dev()
        self.c, self.traits, self.nt = c, list(traits), len(traits)
        n, p = c["n"], c["p"]
        self.s = torch.from_numpy(c["s"].copy()).to(dev)
        self.x = torch.from_numpy(c["x"].copy()).to(dev)
        self.g = torch.from_numpy(c["g"].copy()).to(dev)
        self.y = torch.from_numpy(np.ascontiguousarray(c["Y"][self.traits])).to(dev)
        nbytes = int(lib().jxg_lmm_tables_bytes(n, p, LOW, HIGH))
        assert nbytes > 0 and int(lib().jxg_lmm_series_doubles(p, LOW, HIGH)) == 0      # tables, but no series form
        self.stride = (nbytes + 15) // 16 * 16
        self.tab = torch.empty((self.nt, self.stride), dtype=torch.uint8, device=dev)
        for i in range(self.nt):
            check(lib().jxg_lmm_tables_build(self.s.data_ptr(), self.x.data_ptr(), self.y[i].data_ptr(), n, p, LOW, HIGH,
                                             self.tab[i].data_ptr(), None))

    def carry(self):
        import torch
        return torch.from_numpy(np.ascontiguousarray(self.c["carry0"][self.traits])).to(_dev())

    def launch(self, block=None):
        """All rows in calls of `block` rows (None: one call), states carried -> table (T, m, 3), counts (T, m), final states."""
        import torch
        from janusx_amd import pipeline
        from janusx_amd._lib import check, lib
        c, dev = self.c, _dev()
        n, p, co = c["n"], c["p"], c["co"]
        nch = len(co) - 1
        out = torch.full((self.nt, M_ROWS, 3), -7.0, dtype=torch.float64, device=dev)
        ev = torch.full((self.nt, M_ROWS), -7, dtype=torch.int32, device=dev)
        carry = self.carry()
        for r0 in range(0, M_ROWS, block or M_ROWS):
            nr = min(block or M_ROWS, M_ROWS - r0)
            if block is None:         # the chain list as it is, the empty chain included
                c0, loc = 0, torch.from_numpy(co.astype(np.int32)).to(dev)
            else:
                c0, loc = pipeline._chain_segments(co, r0, r0 + nr, dev)
            check(lib().jxg_lmm_traits_chain_tab(self.g[r0:].data_ptr(), nr, n, self.s.data_ptr(), self.x.data_ptr(), p, LOW, HIGH,
                                                 self.tab.data_ptr(), self.stride, self.nt, TOL_BRENT, MAX_ITER, loc.data_ptr(),
                                                 len(loc) - 1, carry[0, c0:].data_ptr(), nch, out[0, r0:].data_ptr(), M_ROWS,
                                                 ev[0, r0:].data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy(), ev.cpu().numpy(), carry.cpu().numpy()

    def one_wave(self, i):
        """Trait i of this batch through the existing one-wave-per-chain entry on the same tables."""
        import torch
        from janusx_amd._lib import check, lib
        c, dev = self.c, _dev()
        co = torch.from_numpy(c["co"].astype(np.int32)).to(dev)
        out = torch.empty((M_ROWS, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(M_ROWS, dtype=torch.int32, device=dev)
        carry = self.carry()[i].contiguous()
        check(lib().jxg_lmm_scan_chain_tab(self.g.data_ptr(), M_ROWS, c["n"], self.s.data_ptr(), self.x.data_ptr(), c["p"], LOW,
                                           HIGH, self.tab[i].data_ptr(), TOL_BRENT, MAX_ITER, co.data_ptr(), len(co) - 1,
                                           carry.data_ptr(), 0, 0.0, out.data_ptr(), ev.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy(), ev.cpu().numpy()


@pytest.mark.parametrize("nt", [1, 2, 5])
@pytest.mark.parametrize("p", [1, 2, 5])
@pytest.mark.parametrize("n", [150, 601, 1027])
def test_kernel_matches_the_oracle_along_chains(n, p, nt):
    """n = 150 leaves waves without a sample; 601 and 1027 are no multiple of 4 or 64; p = 1 / 2 / 5 are the three instantiations."""
    P = _parity()
    c = _case(n, p)
    out, ev, _carry = _Device(c, range(nt)).launch()
    for t in range(nt):
        be, se, pe = P._assoc_err(out[t], c["ref"][t], tag=f"n{n}p{p}T{nt}t{t}")      # asserts the NaN pattern too
        same = float(np.mean(ev[t] == c["ev"][t]))
        print(f"n={n} p={p} T={nt} trait {t}: beta {be:.2e} se {se:.2e} p {pe:.2e}, equal evaluation counts {same:.4f}")
        assert np.array_equal(np.isnan(out[t, :, 0]), np.isnan(c["ref"][t][:, 0]))
        assert np.all(ev[t][list(ZERO_ROWS)] == 0) and np.all(np.isnan(out[t, list(ZERO_ROWS), 0]))
        assert max(be, se, pe) < P.TOL, (n, p, nt, t, be, se, pe)
        assert same > 0.995, f"only {same:.4f} of the rows of trait {t} took the oracle's number of Brent evaluations"


@pytest.mark.parametrize("n,p", [(601, 2), (1027, 5), (150, 1)])
def test_blocks_of_700_rows_with_carried_states_give_the_same_bits(n, p):
    d = _Device(_case(n, p), range(3))
    one, ev1, c1 = d.launch()
    cut, ev2, c2 = d.launch(block=700)
    assert np.array_equal(one, cut, equal_nan=True) and np.array_equal(ev1, ev2)
    assert np.array_equal(c1, c2, equal_nan=True)


@pytest.mark.parametrize("n,p", [(601, 1), (1027, 2), (150, 5)])
def test_a_trait_has_the_same_bits_alone_in_any_batch_and_twice(n, p):
    c = _case(n, p)
    allt, ev, carry = _Device(c, range(T_MAX)).launch()
    again, ev_b, carry_b = _Device(c, range(T_MAX)).launch()
    assert np.array_equal(allt, again, equal_nan=True) and np.array_equal(ev, ev_b) and np.array_equal(carry, carry_b, equal_nan=True)
    for t in range(T_MAX):
        alone, ev_a, carry_a = _Device(c, [t]).launch()
        assert np.array_equal(alone[0], allt[t], equal_nan=True) and np.array_equal(ev_a[0], ev[t])
        assert np.array_equal(carry_a[0], carry[t], equal_nan=True)
    assert not np.array_equal(allt[0], allt[1], equal_nan=True)
    # the empty chain keeps its state; every other chain ends on a finite one
    assert np.array_equal(carry[:, 0], c["carry0"][:, 0], equal_nan=True) and np.all(np.isfinite(carry[:, 1:]))


@pytest.mark.parametrize("n,p", [(601, 1), (1027, 2), (601, 5)])
def test_kernel_against_the_one_wave_entry(n, p):
    """Same tables, same chains, another summation order: the trajectories agree (evaluation counts equal on > 99.5 % of the
    rows) and, where they do, beta / SE within 1e-8 of max(|beta|, SE) -- the bound `test_exact_scan_with_covariates_block_form`
    asserts between two forms of this scan."""
    d = _Device(_case(n, p), range(3))
    out, ev, _ = d.launch()
    for i in range(3):
        ref, ev_ref = d.one_wave(i)
        assert np.array_equal(np.isnan(out[i, :, 0]), np.isnan(ref[:, 0]))
        eq = ev[i] == ev_ref
        ok = eq & ~np.isnan(ref[:, 0])
        scale = np.maximum(np.abs(ref[ok, 0]), ref[ok, 1])
        db = float(np.max(np.abs(out[i, ok, 0] - ref[ok, 0]) / scale))
        ds = float(np.max(np.abs(out[i, ok, 1] - ref[ok, 1]) / scale))
        print(f"n={n} p={p} trait {i}: equal counts {eq.mean():.4f}, beta {db:.2e}, se {ds:.2e}")
        assert eq.mean() > 0.995, eq.mean()
        assert db < 1e-8 and ds < 1e-8, (db, ds)


# ---- pipeline and routes -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain_case3(oracle):
    """`chain_case` of tests/test_gpu_round6.py (n = 600, m = 3000, 1 % missing calls, intercept + one covariate) with three
    polygenic traits; spectral inputs from the oracle."""
    from janusx_amd import bed
    n, m = 600, 3000
    packed, g = bed.synth_panel_numpy(n, m, seed=71, missing_rate=0.01)
    Y = np.stack([bed.synth_phenotype(g, n_causal=25, pve=pve, seed=sd) for pve, sd in ((0.5, 71), (0.3, 72), (0.7, 73))])
    k, _eff, _keep = oracle.grm_stream_bed(packed, n, 1, 0.02, 0.05, 0.0)
    s, u = oracle.gwas_eigh_from_grm(k)
    x = np.concatenate([np.ones((n, 1)), np.random.default_rng(8).normal(size=(n, 1))], axis=1)
    nm = oracle.spectral_null_model(Y[0], x, s, u)
    mi, he, ho = oracle.row_counts(packed, n)
    keep, maf, miss, flip = oracle.gwas_scan_row_stats(mi, he, ho, n, 0.02, 0.05, 1.0)
    kept = np.nonzero(keep)[0]
    grot = oracle.rotate_block_f32(oracle.decode_centered_block_f32(packed, n, flip, maf, rows=kept), nm.Dh)
    return dict(n=n, packed=packed, nm=nm, kept=kept, maf=maf, grot=grot, Y=Y, x=x)


def test_shared_models_of_many_traits_equal_the_single_trait_models():
    """17 traits beside two design columns (more than one rotation call takes): S / U^T / X~ shared, y~ and the null fit of every
    trait those of the single-trait constructor."""
    import torch
    from janusx_amd import pipeline
    n, nt = 200, 17
    rng = np.random.default_rng(4)
    a = rng.normal(size=(n, 3 * n))
    k = torch.from_numpy(a @ a.T / (3 * n)).to(_dev())
    s, ut64 = pipeline.eigh_from_grm(k, 1e-6)
    x = np.concatenate([np.ones((n, 1)), rng.normal(size=(n, 1))], axis=1)
    Y = rng.normal(size=(nt, n)) + rng.normal(size=(nt, 1)) * (a[:, :5] @ rng.normal(size=5))
    models = pipeline.SpectralModel.for_traits(s, ut64, x, Y)
    assert len(models) == nt and tuple(models[0].y_rot.shape) == (nt, n)
    for t, mdl in enumerate(models):
        one = pipeline.SpectralModel(s, ut64, x, Y[t])
        assert mdl.S is models[0].S and mdl.ut is models[0].ut and mdl.xcov is models[0].xcov
        assert np.array_equal(mdl.ut.cpu().numpy(), one.ut.cpu().numpy())
        scale = float(np.abs(one.y.cpu().numpy()).max())
        assert np.max(np.abs(mdl.xcov.cpu().numpy() - one.xcov.cpu().numpy())) < 1e-12 * scale
        assert np.max(np.abs(mdl.y.cpu().numpy() - one.y.cpu().numpy())) < 1e-12 * scale
        assert abs(mdl.null.lbd - one.null.lbd) < 1e-9 * one.null.lbd and abs(mdl.null.ml0 - one.null.ml0) < 1e-9 * abs(one.null.ml0)
        assert mdl.null.bounds == pytest.approx(one.null.bounds, rel=1e-9)


def test_scan_rows_lmm_traits(oracle_c, chain_case3):
    import torch
    from janusx_amd import pipeline
    from janusx_amd import stats as st
    P = _parity()
    c = chain_case3
    n, nm, kept = c["n"], c["nm"], c["kept"]
    dev = _dev()
    panel = pipeline.Panel(torch.from_numpy(c["packed"]).to(dev), n)
    models = pipeline.SpectralModel.for_traits(torch.from_numpy(nm.S).to(dev), torch.from_numpy(nm.Dh.astype(np.float64)).to(dev),
                                               c["x"], c["Y"])
    shared = models[0]
    lut = st.scan_lut_from_counts(c["maf"][kept], np.zeros(len(kept), bool), panel.counts()[kept], n)
    init = np.array([math.log10(mdl.null.lbd) for mdl in models])
    assert np.all(np.isfinite(init))
    # without chains: the bits of the single-trait scan at the same blocking
    for br in (700, 8192):
        got = pipeline.scan_rows_lmm_traits(panel, shared, kept, lut, shared.y_rot, init, block_rows=br).cpu().numpy()
        for t, mdl in enumerate(models):
            one = pipeline.scan_rows(panel, mdl, kept, lut, "lmm", low=LOW, high=HIGH, max_iter=MAX_ITER, tol=TOL_BRENT,
                                     init_log10_lbd=float(init[t]), block_rows=br).cpu().numpy()
            assert np.array_equal(got[t], one, equal_nan=True), (br, t)
    # with chains: the oracle's chains, for blocks that cut them and for the default blocking
    co = pipeline.traits_chain_offsets(len(kept), 500, 2)
    assert len(co) > 8
    sh, xh = shared.S.cpu().numpy(), shared.xcov.cpu().numpy()
    refs = [oracle_c.lmm_scan_rotated_chains(c["grot"], sh, xh, mdl.y.cpu().numpy(), LOW, HIGH, MAX_ITER, TOL_BRENT, co,
                                             init=float(init[t]), return_evals=True) for t, mdl in enumerate(models)]
    tables = []
    for br in (700, None):
        got, ev = pipeline.scan_rows_lmm_traits(panel, shared, kept, lut, shared.y_rot, init, chain_off=co, block_rows=br,
                                                return_evals=True)
        got, ev = got.cpu().numpy(), ev.cpu().numpy()
        tables.append(got)
        for t, (ref, ev_ref) in enumerate(refs):
            be, se, pe = P._assoc_err(got[t], ref, tag=f"br{br}t{t}")
            same = float(np.mean(ev[t] == ev_ref))
            print(f"block_rows {br} trait {t}: beta {be:.2e} se {se:.2e} p {pe:.2e}, equal evaluation counts {same:.4f}")
            assert max(be, se, pe) < P.TOL, (br, t, be, se, pe)
            assert same > 0.995, (br, t, same)
    assert np.array_equal(tables[0], tables[1], equal_nan=True)


def test_run_traits_lmm_end_to_end(oracle, oracle_c, monkeypatch):
    import torch
    from janusx_amd import bed, pipeline
    P = _parity()
    n, m = 400, 2000
    packed, g = bed.synth_panel_numpy(n, m, seed=33, missing_rate=0.01, family=True)
    Y = np.stack([bed.synth_phenotype(g, n_causal=30, pve=pve, seed=sd) for pve, sd in ((0.5, 33), (0.35, 34), (0.65, 35))])
    x = np.concatenate([np.ones((n, 1)), np.random.default_rng(5).normal(size=(n, 1))], axis=1)
    dev = _dev()
    payload = torch.from_numpy(packed).to(dev)
    k_ref, _eff, _ = oracle.grm_stream_bed(packed, n, 1, 0.02, 0.05, 0.0)
    k = torch.from_numpy(k_ref).to(dev)
    calls = []
    real = pipeline.eigh_from_grm
    monkeypatch.setattr(pipeline, "eigh_from_grm", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    res = pipeline.run_traits_lmm(payload, n, k, None, Y, x, warm_chain=(500, 1))
    assert len(calls) == 1 and res.switch is None and res.stats.shape[0] == 3
    # the oracle end to end: its own eigh, per-trait null, rotation and chains
    s, u = oracle.gwas_eigh_from_grm(k_ref)
    mi, he, ho = oracle.row_counts(packed, n)
    keep, maf, miss, flip = oracle.gwas_scan_row_stats(mi, he, ho, n, 0.02, 0.05, 1.0)
    assert np.array_equal(keep, res.keep)
    rows = np.nonzero(keep)[0]
    assert np.array_equal(res.af, maf[rows]) and np.array_equal(res.miss, miss[rows])
    co = pipeline.traits_chain_offsets(len(rows), 500, 1)
    grot = None
    for t in range(3):
        nm = oracle.spectral_null_model(Y[t], x, s, u)
        if grot is None:
            grot = oracle.rotate_block_f32(oracle.decode_centered_block_f32(packed, n, flip, maf, rows=rows), nm.Dh)
        nf = res.nulls[t]
        assert abs(nf.lbd - nm.lbd_null) < 1e-5 * nm.lbd_null, (nf.lbd, nm.lbd_null)
        assert abs(nf.ml0 - nm.ML0) < 1e-6 * abs(nm.ML0) and abs(nf.reml0 - nm.LL0) < 1e-6 * abs(nm.LL0)
        assert abs(nf.pve - nm.pve) < 1e-5
        ref = oracle_c.lmm_scan_rotated_chains(grot, nm.S, nm.Xcov, nm.y, LOW, HIGH, MAX_ITER, TOL_BRENT, co,
                                               init=math.log10(nm.lbd_null))
        be, se, pe = P._assoc_err(res.stats[t], ref, tag=f"t{t}")
        print(f"end to end trait {t}: beta {be:.2e} se {se:.2e} p {pe:.2e}")
        assert max(be, se, pe) < P.TOL, (t, be, se, pe)
    # one decomposition per sample mask
    del calls[:]
    keep_a = np.arange(n, dtype=np.int64)
    keep_b = np.arange(5, n, dtype=np.int64)
    for idx, members in ((keep_a, [0, 2]), (keep_b, [1])):
        pipeline.run_traits_lmm(payload, n, k, idx, Y[members][:, idx], x[idx], warm_chain=(500, 1))
    assert len(calls) == 2


N_CLI, M_CLI = 240, 600


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    """240 samples x 600 SNPs, a covariate table and the polygenic traits t1, t3 (same samples) and t2 (15 more missing), plus
    `noise`, pure noise on the samples of t1."""
    from janusx_amd import bed
    d = tmp_path_factory.mktemp("lmmtcli")
    rng = np.random.default_rng(37)
    packed, g = bed.synth_panel_numpy(N_CLI, M_CLI, seed=37, missing_rate=0.01, family=True)
    ids = [f"s{i}" for i in range(N_CLI)]
    bim = bed.Bim(["1"] * M_CLI, [f"rs{j}" if j % 7 else "." for j in range(M_CLI)], [1000 + 10 * j for j in range(M_CLI)],
                  ["A"] * M_CLI, ["G"] * M_CLI)
    pre = str(d / "panel")
    bed.write_bed(pre, packed, ids, bim)
    cov = rng.normal(size=(N_CLI, 1))
    y = np.stack([bed.synth_phenotype(g, n_causal=20, pve=0.6, seed=40 + t) for t in range(3)] + [rng.normal(size=N_CLI)])
    y[:3] += 0.3 * cov[:, 0]
    gone = rng.permutation(N_CLI)
    y[:, gone[:9]] = np.nan
    y[1, gone[9:24]] = np.nan
    with open(pre + ".pheno.tsv", "w") as fh:
        fh.write("id\tt1\tt2\tt3\tnoise\n")
        for i in range(N_CLI):
            fh.write(ids[i] + "\t" + "\t".join("NA" if np.isnan(v) else repr(float(v)) for v in y[:, i]) + "\n")
    with open(pre + ".cov.tsv", "w") as fh:
        fh.write("id\tc0\n")
        for i in range(N_CLI):
            fh.write(f"{ids[i]}\t{float(cov[i, 0])!r}\n")
    return pre, packed, ids, bim, cov, y


def _read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:-1]]


def test_cli_writes_the_combined_table(prefix, tmp_path, capsys):
    import torch
    from janusx_amd import cli, pipeline
    from janusx_amd import janusx as jxrs
    from janusx_amd import stats as st
    from janusx_amd.tsv import HEADER_TRAITS, assoc_trait_stats, format_trait_rows, resolve_snp_name, trait_site_prefixes
    pre, packed, ids, bim, cov, y = prefix
    base = ["gwas", "-bfile", pre, "-p", pre + ".pheno.tsv", "-c", pre + ".cov.tsv", "-n", "t1", "-n", "t2", "-n", "t3", "-lmm",
            "-chunksize", "200"]
    plain, comb, cut = str(tmp_path / "plain"), str(tmp_path / "comb"), str(tmp_path / "cut")
    assert cli.main(base + ["-force-model", "-o", plain]) == 0
    assert cli.main(base + ["-force-model", "-trait-level-lmm", "-o", comb]) == 0
    said = capsys.readouterr().out
    assert "-lmm -trait-level-lmm: 3 traits" in said and "traits=2" in said and "traits=1" in said
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("comb")) == ["comb.lmm.tsv"]
    text = open(comb + ".lmm.tsv").read()
    head, body = _read_tsv(comb + ".lmm.tsv")
    assert "\t".join(head) + "\n" == HEADER_TRAITS
    names = [b[11] for b in body]
    assert [nm for i, nm in enumerate(names) if i == 0 or names[i - 1] != nm] == ["t1", "t3", "t2"]
    for name in ("t1", "t2", "t3"):
        _ph, pbody = _read_tsv(f"{plain}.{name}.lmm.tsv")
        mine = [b for b in body if b[11] == name]
        assert len(mine) == len(pbody) and 0 < len(pbody) < M_CLI
        assert [a[:7] for a in mine] == [b[:7] for b in pbody]            # site columns, af, miss as a rate
    # the whole text from the mirror's numbers
    dev = _dev()
    payload = torch.from_numpy(packed).to(dev)
    k, _eff, _ = pipeline.build_grm(payload, N_CLI, 1, 0.02, 0.05)
    want = HEADER_TRAITS
    for members in ((0, 2), (1,)):
        idx = np.nonzero(np.isfinite(y[members[0]]))[0].astype(np.int64)
        panel = pipeline.Panel(payload, N_CLI, idx)
        counts = panel.counts()
        keep, af, miss = st.gwas_scan_row_stats(counts, len(idx), 0.02, 0.05, 1.0)
        rows = np.nonzero(keep)[0]
        x = np.concatenate([np.ones((len(idx), 1)), cov[idx]], axis=1)
        stats, nulls = jxrs.lmm_trait_assoc_packed(payload, N_CLI, y[list(members)][:, idx], x, k, np.zeros(len(rows), bool), af[rows],
                                                   sample_indices=idx, row_indices=rows, chunk_size=200)
        assert stats.shape == (len(members), len(rows), 3) and len(nulls) == len(members) and all(nl[0] > 0 for nl in nulls)
        pf = trait_site_prefixes(["1"] * len(rows), [bim.pos[j] for j in rows],
                                 [resolve_snp_name(bim.snp[j], "1", bim.pos[j]) for j in rows], ["A"] * len(rows), ["G"] * len(rows),
                                 af[rows], miss[rows], as_rate=True)
        for i, t in enumerate(members):
            want += format_trait_rows(pf, assoc_trait_stats(stats[i]), ("t1", "t2", "t3")[t])
    assert text == want
    # -trait-pmax: exactly the qualifying lines (the cut is made on the unrounded p: a printed 1.0000e-2 may sit on either side)
    assert cli.main(base + ["-force-model", "-trait-level-lmm", "-trait-pmax", "0.01", "-o", cut]) == 0
    _h, cbody = _read_tsv(cut + ".lmm.tsv")
    assert [c for c in cbody if c[10] != "1.0000e-2"] == [b for b in body if float(b[10]) <= 0.01 and b[10] != "1.0000e-2"]
    assert all(c in body for c in cbody) and 0 < len(cbody) < len(body) // 5


def test_cli_leaves_a_group_with_a_noise_trait_to_the_trait_by_trait_route(prefix, tmp_path, capsys):
    from janusx_amd import cli
    pre = prefix[0]
    base = ["gwas", "-bfile", pre, "-p", pre + ".pheno.tsv", "-c", pre + ".cov.tsv", "-n", "t1", "-n", "t2", "-n", "noise", "-lmm",
            "-chunksize", "200"]
    plain, comb = str(tmp_path / "plain"), str(tmp_path / "comb")
    assert cli.main(base + ["-o", plain]) == 0
    capsys.readouterr()
    assert cli.main(base + ["-trait-level-lmm", "-o", comb]) == 0
    said = capsys.readouterr().out
    assert "Warning: -trait-level-lmm: trait noise would switch to LM (null LRT stat=" in said and "this group goes trait by trait" in said
    # the group (t1, noise) as without the switch: t1 as an LMM table, noise as an LM table; t2 alone in the combined table
    made = sorted(f for f in os.listdir(tmp_path) if f.startswith("comb"))
    assert made == ["comb.lmm.tsv", "comb.noise.lm.tsv", "comb.t1.lmm.tsv"]
    for f in ("t1.lmm.tsv", "noise.lm.tsv"):
        assert open(f"{comb}.{f}").read() == open(f"{plain}.{f}").read()
    _h, body = _read_tsv(comb + ".lmm.tsv")
    assert body and {b[11] for b in body} == {"t2"}
    _h2, pbody = _read_tsv(plain + ".t2.lmm.tsv")
    assert [b[:7] for b in body] == [b[:7] for b in pbody]
