"""GPU tests of `jx gwas -farmcpu` (csrc/k_farmcpu.hip, `pipeline.scan_rows_farmcpu_fem` / `_final`, janusx_amd/farmcpu.py) against
the f64 restatement of the reference's raw route (tests/farmcpu_ref.py): the statistics kernel at its edges, exactness of the
sums behind it, the REM scorer on device-decoded leads, the whole procedure on the fixture whose conditions
tests/test_farmcpu_host.py asserts, and the command line."""
import math
import os

import numpy as np
import pytest

import farmcpu_ref as R

pytestmark = pytest.mark.gpu

N_SRC, M_SRC = 320, 300
BAR = 1e-5            # README, "The bar, stated once": beta against max(|beta|, se), se, p / max(1, t^2) and -log10 p
# Largest relative disagreement of `farmcpu.ll_score` (batched over the delta grid) with the restatement's (one pseudo-inverse per
# grid point) over the lead sets and combo grids of the tests below: measured 4.3e-16 (three units in the last place of a score
# near 800); asserted at 10 x that, the margin for BLAS reduction order.
SCORE_REL = 4.3e-15


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


@pytest.fixture(scope="module")
def source():
    """320 samples x 300 SNPs with 3 % missing calls, built as in test_gpu_lm_traits.py: row 0 has no call at all, row 1 is
    monomorphic, row 2 all heterozygous."""
    rng = np.random.default_rng(20)
    p = rng.uniform(0.05, 0.5, size=M_SRC)
    g = rng.binomial(2, p[:, None], size=(M_SRC, N_SRC)).astype(np.int8)
    g[rng.random(g.shape) < 0.03] = -9
    g[0] = -9
    g[1] = 0
    g[2] = 1
    flip = rng.random(M_SRC) < 0.4
    flip[:3] = [True, False, True]
    called = (g >= 0).sum(1)
    af = (np.where(g < 0, 0, g).sum(1) / np.maximum(2 * called, 1)).astype(np.float32)
    af[7] = np.float32(0.8)                                       # a row whose missing calls decode to 2
    return g, flip, af


@pytest.fixture(scope="module")
def panel(source):
    torch = _torch()
    from janusx_amd import bed
    from janusx_amd.pipeline import Panel
    return Panel(torch.from_numpy(bed.pack_dosage(source[0])).cuda(), N_SRC)


@pytest.fixture(scope="module")
def decoded(source):
    g, flip, af = source
    return R.decode(g, af, flip)


def _design(decoded, p_cov, k_qtn, dup_cov=False, seed=5):
    """x = [1 | p_cov covariates | k_qtn decoded marker rows], y with effects on two of the QTNs, and the QTN markers."""
    rng = np.random.default_rng(seed)
    cov = rng.standard_normal((N_SRC, p_cov))
    qtn = list(rng.choice(np.arange(3, M_SRC), size=k_qtn, replace=False)) if k_qtn else []
    if dup_cov:
        cov[:, 0] = decoded[qtn[0]]                               # the first QTN column repeats a covariate: rank deficient
    x = np.hstack([np.ones((N_SRC, 1)), cov, decoded[qtn].T]) if qtn else np.hstack([np.ones((N_SRC, 1)), cov])
    y = rng.standard_normal(N_SRC) + 0.5 * decoded[40] - 0.4 * decoded[90]
    if qtn:
        y = y + 0.6 * decoded[qtn[0]]
    return np.ascontiguousarray(x), 1 + p_cov, y, [int(i) for i in qtn]


def _check_fem(panel, source, decoded, x, q_base, y, rows, block_rows=None):
    from janusx_amd import pipeline as pl
    g, flip, af = source
    got = pl.scan_rows_farmcpu_fem(panel, rows, af[rows], flip[rows], x, q_base, y, block_rows=block_rows)
    st = got.stats.cpu().numpy()
    beta, se, p, qmin, void = R.fem_scan(decoded[rows], x, q_base, y)
    assert np.array_equal(np.isnan(st[:, 0]), void) and np.array_equal(np.isnan(st[:, 1]), void)      # the void pattern
    assert np.all(st[void, 2] == 1.0) and np.array_equal(got.p.cpu().numpy(), st[:, 2])
    ok = ~void
    if ok.any():
        t2 = (beta[ok] / se[ok]) ** 2
        eb = np.max(np.abs(st[ok, 0] - beta[ok]) / np.maximum(np.abs(beta[ok]), se[ok]))
        es = np.max(np.abs(st[ok, 1] - se[ok]) / se[ok])
        ep = np.max(np.abs(st[ok, 2] - p[ok]) / p[ok] / np.maximum(1.0, t2))
        el = np.max(np.abs(np.log10(st[ok, 2]) - np.log10(p[ok])) / np.maximum(1.0, -np.log10(p[ok])))
        print(f"fem q0={x.shape[1]} q_base={q_base} rows={len(rows)}: beta {eb:.2e} se {es:.2e} p {ep:.2e} log10p {el:.2e}")
        assert eb <= BAR and es <= BAR and ep <= BAR and el <= BAR, (eb, es, ep, el)
    assert got.qtn_min_p.shape == qmin.shape
    if qmin.size:
        eq = np.max(np.abs(np.log10(got.qtn_min_p) - np.log10(qmin)) / np.maximum(1.0, -np.log10(qmin)))
        print(f"    per-slot min p: log10 {eq:.2e}")
        assert eq <= BAR, (eq, got.qtn_min_p, qmin)
    return got, st


@pytest.mark.parametrize("p_cov", [0, 3])
@pytest.mark.parametrize("k_qtn", [0, 1, 31, 33])
def test_fem_statistics_at_the_kernel_edges(panel, source, decoded, p_cov, k_qtn):
    """All 300 rows (the all-missing, monomorphic and all-heterozygous rows and the QTNs' own markers are void or near it);
    31 and 33 QTN columns put q0 on either side of the 32-column tile of the product."""
    x, q_base, y, qtn = _design(decoded, p_cov, k_qtn)
    _got, st = _check_fem(panel, source, decoded, x, q_base, y, np.arange(M_SRC))
    assert np.isnan(st[:3, 0]).all()
    for j in qtn:                                                 # a row equal to a QTN column: b22 = 0
        assert np.isnan(st[j, 0]) and st[j, 2] == 1.0


def test_fem_statistics_on_a_rank_deficient_design(panel, source, decoded):
    x, q_base, y, _qtn = _design(decoded, 3, 4, dup_cov=True)
    _check_fem(panel, source, decoded, x, q_base, y, np.arange(M_SRC))


@pytest.mark.parametrize("nrows", [1, 127, 129, 300])
def test_fem_statistics_at_every_row_count(panel, source, decoded, nrows):
    x, q_base, y, _qtn = _design(decoded, 3, 31)
    rows = np.arange(M_SRC - 1, -1, -1)[:nrows] if nrows < M_SRC else np.arange(M_SRC)
    _check_fem(panel, source, decoded, x, q_base, y, rows)


@pytest.mark.parametrize("k_qtn", [0, 33])
def test_blocked_and_unblocked_bits_are_equal(panel, source, decoded, k_qtn):
    from janusx_amd import pipeline as pl
    g, flip, af = source
    x, q_base, y, _qtn = _design(decoded, 3, k_qtn)
    rows = np.arange(M_SRC)
    whole = pl.scan_rows_farmcpu_fem(panel, rows, af, flip, x, q_base, y)
    fwhole = pl.scan_rows_farmcpu_final(panel, rows, af, flip, x, q_base, y).cpu().numpy()
    for br in (128, 77, 1):
        if br == 1 and k_qtn:
            continue
        part = pl.scan_rows_farmcpu_fem(panel, rows, af, flip, x, q_base, y, block_rows=br)
        assert np.array_equal(part.stats.cpu().numpy().view(np.int64), whole.stats.cpu().numpy().view(np.int64)), br
        assert np.array_equal(part.qtn_min_p.view(np.int64), whole.qtn_min_p.view(np.int64)), br
        fpart = pl.scan_rows_farmcpu_final(panel, rows, af, flip, x, q_base, y, block_rows=br).cpu().numpy()
        assert np.array_equal(fpart.view(np.int64), fwhole.view(np.int64)), br


def test_final_statistics(panel, source, decoded):
    from janusx_amd import pipeline as pl
    g, flip, af = source
    x, q_base, y, qtn = _design(decoded, 3, 5)
    got = pl.scan_rows_farmcpu_final(panel, np.arange(M_SRC), af, flip, x, q_base, y).cpu().numpy()
    want = R.final_scan(decoded, x, q_base, y, [])
    void = np.isnan(want[:, 0])
    assert np.array_equal(np.isnan(got[:, 0]), void) and np.isnan(got[void]).all()
    ok = ~void
    t2 = (want[ok, 0] / want[ok, 1]) ** 2
    assert np.max(np.abs(got[ok, 0] - want[ok, 0]) / np.maximum(np.abs(want[ok, 0]), want[ok, 1])) <= BAR
    assert np.max(np.abs(got[ok, 1] - want[ok, 1]) / want[ok, 1]) <= BAR
    assert np.max(np.abs(got[ok, 2] - want[ok, 2]) / want[ok, 2] / np.maximum(1.0, t2)) <= BAR
    assert np.max(np.abs(np.log10(got[ok, 2]) - np.log10(want[ok, 2])) / np.maximum(1.0, -np.log10(want[ok, 2]))) <= BAR


def test_fem_statistics_across_the_slot_batch(panel, source, decoded):
    """129 QTN columns: one more than a workgroup's 128 slot accumulators, so the second slot batch holds one slot."""
    x, q_base, y, _qtn = _design(decoded, 0, 129)
    _check_fem(panel, source, decoded, x, q_base, y, np.arange(M_SRC))


def test_the_kernel_refuses_more_qtn_columns_than_its_cap():
    torch = _torch()
    from janusx_amd._lib import check, lib
    cap = lib().jxg_farmcpu_max_qtn()
    assert cap == 512
    t = torch.zeros(4096, dtype=torch.float64, device="cuda")
    bits = torch.zeros(1024, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    with pytest.raises(RuntimeError, match="above the cap of 512"):        # refused before anything is launched
        check(lib().jxg_farmcpu_fem_stats(p, p, 2, 1, p, 1, p, 4, 1.0, 10, p, 1, cap + 1, p, p, p, bits.data_ptr(), None))
    with pytest.raises(RuntimeError, match="rank of the design"):
        check(lib().jxg_farmcpu_final_stats(p, p, 600, 513, p, 1, p, 4, 1.0, 10, p, None))


def test_sums_behind_the_statistics_are_exact_on_a_dyadic_design(panel, source):
    """xs = X'g, sy = g'y and ss = g'g recovered from the device sums equal integer arithmetic bit for bit when the columns are
    integers times a power of two (major-allele imputation: the missing value is 0 or 2, so everything is an integer)."""
    torch = _torch()
    from janusx_amd import pipeline as pl
    from janusx_amd._lib import check, lib
    g, flip, af = source
    rng = np.random.default_rng(8)
    ncols = 37
    k = rng.integers(-(1 << 20), (1 << 20) + 1, size=(ncols, N_SRC), dtype=np.int64)
    k[0] = 1 << 10                                                # the intercept, as a dyadic column
    e = (np.arange(ncols) % 7) - 3
    cols = k.astype(np.float64) * np.ldexp(1.0, e)[:, None]
    rows = np.arange(M_SRC, dtype=np.int32)
    miss_v = pl.farmcpu_missing_value(af)
    op = pl._LmtOperand(cols, N_SRC, panel.npad, panel.device)
    out = torch.empty((M_SRC, ncols), dtype=torch.float64, device=panel.device)
    rows_t, mean_t = torch.from_numpy(rows).cuda(), torch.from_numpy(miss_v).cuda()
    flip_t = torch.from_numpy(flip.astype(np.uint8)).cuda()
    check(lib().jxg_lmt_sums_p32(pl._ptr(panel.p32), panel.m, N_SRC, pl._ptr(rows_t), M_SRC, pl._ptr(mean_t), pl._ptr(flip_t),
                                 pl._ptr(op.planes), pl._ptr(op.scale), pl._ptr(op.colsum), ncols, pl._ptr(out), ncols,
                                 pl._stream()))
    gi = R.decode(g, af, flip).astype(np.int64)                   # integers 0, 1, 2
    want = (gi @ k.T).astype(np.float64) * np.ldexp(1.0, e)[None, :]
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    ss = pl.lm_traits_row_d(panel.counts()[rows], N_SRC, miss_v, flip)
    assert np.array_equal(ss, (gi * gi).sum(axis=1).astype(np.float64))


# ---- the REM scorer ---------------------------------------------------------------------------------------------------------------

def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("leads", [[40], [40, 90], list(range(10, 130, 10)), [40, 90, 40], [40, 1, 90]],
                         ids=["k1", "k2", "k12", "two_identical_columns", "constant_column"])
def test_scorer_on_device_decoded_leads(panel, source, decoded, leads):
    from janusx_amd import farmcpu as fc
    g, flip, af = source
    x, _q_base, y, _qtn = _design(decoded, 3, 2)
    s = fc.decode_rows(panel, np.array(leads), af[leads], flip[leads])
    assert np.array_equal(s, decoded[leads].T)                    # the device decode is the restatement's, exactly
    got, want = fc.ll_score(y, x, s), R.ll_score(y, x, decoded[leads].T)
    print(f"score {leads[:3]}..: {got:.12f} vs {want:.12f}, rel {_rel(got, want):.2e}")
    assert _rel(got, want) <= SCORE_REL


def test_scorer_argmin_over_a_grid_of_combos(panel, source, decoded):
    """3 bin sizes x 6 lead counts on the prior of a FEM scan: the same lead sets, scores within the bound, the same winner."""
    from janusx_amd import farmcpu as fc
    from janusx_amd import pipeline as pl
    g, flip, af = source
    x, q_base, y, _qtn = _design(decoded, 3, 2)
    rows = np.arange(M_SRC)
    prior = R.prior_from_model(decoded, x, q_base, y, _qtn)
    gpos = R.global_positions([str(1 + i // 100) for i in rows], [1000 + 7919 * (i % 100) * 113 for i in rows])
    szbin, nbins = [50_000, 5_000_000, 50_000_000], [2, 4, 6, 8, 10, 12]
    best, combos = fc.best_rem_lead_set(y, x, prior, gpos, szbin, nbins, lambda idx: fc.decode_rows(panel, idx, af[idx], flip[idx]))
    want = []
    for sz in szbin:
        for nn in nbins:
            lead = R.select_lead_indices(sz, nn, prior, gpos)
            want.append((lead, R.ll_score(y, x, decoded[lead].T)))
    assert len(combos) == 18 and len({tuple(w[0]) for w in want}) >= 6
    for (sz, nn, score, lead), (wlead, wscore) in zip(combos, want):
        assert list(lead) == wlead
        assert _rel(score, wscore) <= SCORE_REL, (sz, nn, score, wscore)
    assert best == int(np.argmin([w[1] for w in want]))


# ---- the whole procedure ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def whole():
    """The fixture of tests/farmcpu_ref.py, its restatement run (computed once) and the packed payload."""
    from janusx_amd import bed
    fx = R.make_fixture()
    gd = R.fixture_decoded(fx)
    ref = R.run_raw(gd, fx["y"], fx["x_base"], fx["chrom"], fx["pos"], 1.0 / len(gd))
    return fx, gd, ref, bed.pack_dosage(fx["g"])


def _table_errors(got, want):
    void = np.isnan(want[:, 0])
    assert np.array_equal(np.isnan(got[:, 0]), void) and np.all(got[void, 2] == 1.0)
    ok = ~void
    t2 = (want[ok, 0] / want[ok, 1]) ** 2
    return (np.max(np.abs(got[ok, 0] - want[ok, 0]) / np.maximum(np.abs(want[ok, 0]), want[ok, 1])),
            np.max(np.abs(got[ok, 1] - want[ok, 1]) / want[ok, 1]),
            np.max(np.abs(got[ok, 2] - want[ok, 2]) / want[ok, 2] / np.maximum(1.0, t2)),
            np.max(np.abs(np.log10(got[ok, 2]) - np.log10(want[ok, 2])) / np.maximum(1.0, -np.log10(want[ok, 2]))))


def test_whole_procedure_follows_the_restatement(whole):
    _torch()
    from janusx_amd import janusx as jx
    fx, gd, ref, packed = whole
    res = jx.farmcpu_packed(fx["y"], fx["x_base"][:, 1:], packed, gd.shape[1], fx["flip"], fx["af"], list(fx["chrom"]),
                            list(fx["pos"]))
    assert len(res.trace) == len(ref["trace"])                    # the iteration count
    for it, (a, b) in enumerate(zip(res.trace, ref["trace"])):
        assert a["qtn"] == b["qtn"], it                           # the QTN set of every iteration
        if "combo" in b:
            assert a["combo"] == b["combo"] and a["lead"] == b["lead"] and a["qtn_next"] == b["qtn_next"], it
            for sa, sb in zip(a["scores"], b["scores"]):
                assert _rel(sa, sb) <= SCORE_REL, (it, sa, sb)
    assert res.qtn == ref["qtn"] and len(res.qtn) >= 3
    errs = _table_errors(res.stats, ref["stats"])
    print("whole procedure: beta %.2e se %.2e p %.2e log10p %.2e" % errs)
    assert max(errs) <= BAR, errs
    assert np.array_equal(res.miss, (fx["g"] < 0).sum(axis=1))


def _last_digit_apart(a, b):
    if a == b:
        return True
    if "NaN" in (a, b):
        return False
    return abs(float(a) - float(b)) <= 1.0001e-4


def _bim_of(fx):
    from janusx_amd import bed
    m = len(fx["pos"])
    return bed.Bim([str(c) for c in fx["chrom"]], [("." if j % 7 == 0 else f"rs{j}") for j in range(m)],
                   [int(p) for p in fx["pos"]], ["A"] * m, ["G"] * m)


def test_written_tables_equal_the_restatements_rendering(whole, tmp_path):
    _torch()
    from janusx_amd import bed
    from janusx_amd import janusx as jx
    fx, gd, ref, packed = whole
    m, n = gd.shape
    prefix = str(tmp_path / "panel")
    bim = _bim_of(fx)
    bed.write_bed(prefix, packed, [f"s{i}" for i in range(n)], bim)
    out, qout = str(tmp_path / "r.farmcpu.tsv"), str(tmp_path / "r.farmcpu.qtn")
    miss = (fx["g"] < 0).sum(axis=1)
    with pytest.raises(RuntimeError, match="unified route"):
        jx.farmcpu_packed_to_tsv(fx["y"], fx["x_base"][:, 1:], packed, n, fx["flip"], fx["af"], miss / np.float32(n), out,
                                 bed_prefix=prefix)
    with pytest.raises(RuntimeError, match="skip_main_scan"):
        jx.farmcpu_packed_to_tsv(fx["y"], fx["x_base"][:, 1:], packed, n, fx["flip"], fx["af"], miss / np.float32(n), out,
                                 bed_prefix=prefix, raw=True, skip_main_scan=True)
    rows, nq, qrows, s1, s2 = jx.farmcpu_packed_to_tsv(fx["y"], fx["x_base"][:, 1:], packed, n, fx["flip"], fx["af"],
                                                       miss / np.float32(n), out, threshold=1.0 / m, pseudo_tsv=qout,
                                                       bed_prefix=prefix, raw=True)
    assert (rows, nq, qrows) == (m, len(ref["qtn"]), len(ref["qtn"])) and s1 > 0.0 and s2 > 0.0
    names = [s if s != "." else f"{c}_{p}" for s, c, p in zip(bim.snp, bim.chrom, bim.pos)]
    main, qtn = R.render_tables(ref["stats"], ref["qtn"], bim.chrom, bim.pos, names, bim.a0, bim.a1, fx["af"], miss, np.arange(m))
    for path, text in ((out, main), (qout, qtn)):
        got, want = open(path).read().splitlines(), text.splitlines()
        assert got[0] == want[0] and len(got) == len(want)
        moved = 0
        for a, b in zip(got[1:], want[1:]):
            if a == b:
                continue
            fa, fb = a.split("\t"), b.split("\t")
            assert fa[:7] == fb[:7] and fa[11:] == fb[11:], (a, b)                # site columns, af, miss count, source_row
            assert _last_digit_apart(fa[7], fb[7]) and _last_digit_apart(fa[8], fb[8]), (a, b)
            moved += fa[7:9] != fb[7:9]
            # chisq and pwald print five digits: they move by what 1e-5 on t allows (bounded in size, not in count)
            t2 = float(fb[9]) if fb[9] != "NaN" else 0.0
            assert (fa[9] == "NaN") == (fb[9] == "NaN")
            if fb[9] != "NaN":
                assert abs(float(fa[9]) - t2) <= 1.0001e-4 * t2 + 4e-5 * (math.sqrt(t2) + t2), (a, b)
            assert abs(float(fa[10]) - float(fb[10])) <= (1.0001e-4 + 1e-5 * max(1.0, t2)) * float(fb[10]), (a, b)
        assert moved <= 0.03 * (len(got) - 1), (path, moved)


def test_command_line(whole, tmp_path, capsys):
    _torch()
    from janusx_amd import bed, cli
    fx, gd, _ref, packed = whole
    m, n = gd.shape
    prefix = str(tmp_path / "panel")
    ids = [f"s{i}" for i in range(n)]
    bed.write_bed(prefix, packed, ids, _bim_of(fx))
    with open(prefix + ".pheno.tsv", "w") as fh:
        fh.write("id\tt1\n")
        fh.writelines(f"{s}\t{float(v)!r}\n" for s, v in zip(ids, fx["y"]))
    base = ["gwas", "-bfile", prefix, "-p", prefix + ".pheno.tsv", "-maf", "0.02", "-geno", "0.1"]
    plain, both = str(tmp_path / "plain"), str(tmp_path / "both")
    assert cli.main(base + ["-lm", "-o", plain]) == 0
    assert cli.main(base + ["-lm", "-farmcpu", "-q", "2", "-o", both]) == 0
    said = capsys.readouterr().out
    assert "-farmcpu: n=400" in said and "qtn=" in said
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("both")) == ["both.t1.farmcpu.qtn", "both.t1.farmcpu.tsv",
                                                                                "both.t1.lm.tsv"]
    # -farmcpu beside -lm leaves the LM table as it is with -q 2 alone
    alone = str(tmp_path / "alone")
    assert cli.main(base + ["-lm", "-q", "2", "-o", alone]) == 0
    assert open(both + ".t1.lm.tsv").read() == open(alone + ".t1.lm.tsv").read()
    head = open(both + ".t1.farmcpu.tsv").readline().rstrip("\n").split("\t")
    assert head == ["chrom", "pos", "snp", "allele0", "allele1", "af", "miss", "beta", "se", "chisq", "pwald"]
    lm_rows = sum(1 for _ in open(plain + ".t1.lm.tsv"))
    assert sum(1 for _ in open(both + ".t1.farmcpu.tsv")) == lm_rows
    qlines = open(both + ".t1.farmcpu.qtn").read().splitlines()
    assert qlines[0].split("\t")[-1] == "source_row" and len(qlines) >= 4
    for bad in (["-frgwas"], ["-algwas"], ["-lm", "-trait-level"]):
        with pytest.raises(SystemExit):
            cli.main(base + ["-farmcpu"] + bad + ["-o", str(tmp_path / "bad")])
