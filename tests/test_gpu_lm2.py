"""GPU tests of `jx gwas -lm / -lm2` (csrc/k_lm2.hip `jxg_lm2_scan_p32`, `pipeline.scan_rows_lm2`, the mirror functions and the
command line) against the numpy restatement of the reference in tests/test_lm2_host.py.

The bar: beta and se within 1e-9 of max(|beta|, se), every chisq within 1e-9 max(1, stat), every p within 1e-9 max(1, stat)
relatively.  The restatement alone moves by at most 1e-12 when its sample sums are reordered on these panels and cond(S) stays
below 1e5 (test_lm2_host.py::test_restatement_moves_little_under_reordering), so 1e-9 leaves three decades of room and still
fails an f32 operand (6e-8 x cond).  The tests print the measured maxima.

Row-count edges: the moment kernel gives a wave 16 SNPs (L2_SNPS) and a workgroup 64 (L2_ROWS), the algebra kernel 64 threads;
15, 16, 17 and 63, 64, 65 straddle them, 129 and 257 are several workgroups with a ragged last one."""
import math
import os

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx
from janusx_amd import pipeline as pl

from test_lm2_host import (PANELS, lm2_errors, lm2_panel, ref_alt_freq, ref_chi2_sf, ref_lm2_scan)   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def cases():
    """name -> (g, x, csel, y, af, reference table) of every panel, computed once."""
    out = {}
    for name in PANELS:
        g, x, cov_all, idx, y = lm2_panel(name)
        csel = np.ascontiguousarray(cov_all[:, idx])
        af, _miss = ref_alt_freq(g)
        out[name] = (g, x, csel, y, af, ref_lm2_scan(g, af, None, x, csel, y))
    return out


def _panel(g, sample_idx=None):
    return pl.Panel(torch.from_numpy(bed.pack_dosage(g)).cuda(), g.shape[1], sample_idx)


def _scan(g, x, csel, y, af, rows=None, flip=None, sample_idx=None, **kw):
    rows = np.arange(g.shape[0]) if rows is None else np.asarray(rows)
    out = pl.scan_rows_lm2(_panel(g, sample_idx), rows, af[rows], x, csel, y, flip=flip, **kw)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(rows), 4 * (1 + csel.shape[1]) + 4)
    return out.cpu().numpy()


def _check(got, want, k, what):
    eb, es, ec, ep = lm2_errors(got, want, k)
    print(f"{what}: max error beta {eb:.2e}, se {es:.2e}, chisq {ec:.2e}, p {ep:.2e}")
    assert eb <= TOL and es <= TOL and ec <= TOL and ep <= TOL, (what, eb, es, ec, ep)


@pytest.mark.parametrize("name", ["n127", "n128", "n129", "n300"])
def test_sample_tile_edges(cases, name):
    g, x, csel, y, af, want = cases[name]
    _check(_scan(g, x, csel, y, af), want, csel.shape[1], name)


@pytest.mark.parametrize("name", ["q1k1", "n300", "q5k3", "q12k8"])
def test_column_count_edges(cases, name):
    """7, 18, 34 and 162 weight columns: under one block of 16, across 16, across 32, and three passes of four blocks."""
    g, x, csel, y, af, want = cases[name]
    _check(_scan(g[:70], x, csel, y, af), want[:70], csel.shape[1], name)


@pytest.mark.parametrize("nrows", [1, 15, 16, 17, 63, 64, 65, 129, 257])
def test_row_count_edges(cases, nrows):
    g, x, csel, y, af, want = cases["n300"]
    _check(_scan(g, x, csel, y, af, rows=np.arange(nrows)), want[:nrows], csel.shape[1], f"{nrows} rows")


def test_strided_rows(cases):
    g, x, csel, y, af, want = cases["n300"]
    rows = np.arange(2, g.shape[0], 3)
    _check(_scan(g, x, csel, y, af, rows=rows), want[rows], csel.shape[1], "every third row")


def test_flipped_rows(cases):
    g, x, csel, y, af, _want = cases["n129"]
    flip = (np.arange(g.shape[0]) % 2).astype(bool)
    _check(_scan(g, x, csel, y, af, flip=flip), ref_lm2_scan(g, af, flip, x, csel, y), csel.shape[1], "half the rows flipped")


def test_sample_subset(cases):
    g, x, csel, y, _af, _want = cases["n300"]
    idx = np.random.default_rng(3).permutation(g.shape[1])[:203]
    gs = g[:70][:, idx]
    af, _ = ref_alt_freq(gs)
    want = ref_lm2_scan(gs, af, None, x[idx], csel[idx], y[idx])
    _check(_scan(g[:70], x[idx], csel[idx], y[idx], af, sample_idx=idx), want, csel.shape[1], "203 of 300 samples, permuted")


def test_rank_deficient_design(cases):
    g, x, csel, y, af, want_full = cases["q5k3"]
    xd = np.concatenate([x, x[:, 2:3]], axis=1)
    want = ref_lm2_scan(g, af, None, xd, csel, y)
    assert not np.allclose(want[:, 1], want_full[:, 1], rtol=1e-6)           # df = n - (q_base + 1 + k) with the column counted
    _check(_scan(g, xd, csel, y, af), want, csel.shape[1], "duplicated column in X")


def test_blocking_and_reruns_give_the_same_bits(cases):
    g, x, csel, y, af, _want = cases["n300"]
    panel = _panel(g)
    rows = np.arange(g.shape[0])
    one = pl.scan_rows_lm2(panel, rows, af, x, csel, y)
    again = pl.scan_rows_lm2(panel, rows, af, x, csel, y)
    blocks = pl.scan_rows_lm2(panel, rows, af, x, csel, y, block_rows=100)
    assert torch.equal(one.view(torch.int64), again.view(torch.int64))
    assert torch.equal(one.view(torch.int64), blocks.view(torch.int64))


def test_all_zero_snp_is_exact(cases):
    g, x, csel, y, af, want = cases["n129"]
    g = g[:20].copy()
    g[7] = 0
    af = af[:20].copy()
    af[7] = 0.0
    got = _scan(g, x, csel, y, af)
    k = csel.shape[1]
    row = got[7]
    for a in range(1 + k):
        assert row[4 * a] == 0.0 and math.isnan(row[4 * a + 1]) and math.isnan(row[4 * a + 2]) and row[4 * a + 3] == 1.0
    assert row[-4] == 0.0 and row[-3] == 1.0 and row[-2] == 0.0 and row[-1] == 1.0
    keep = np.arange(20) != 7
    _check(got[keep], want[:20][keep], k, "the rows beside the all-zero SNP")


def test_all_zero_interaction_column(cases):
    """c_2 = 0: its coefficient is 0 with no standard error, the other coefficients are those of the fit without the column (the
    standard errors up to the one degree of freedom the column still counts), and the interaction test keeps k degrees."""
    g, x, csel, y, af, _want = cases["q5k3"]
    g = g[:40]
    k = csel.shape[1]
    cz = csel.copy()
    cz[:, 1] = 0.0
    got = _scan(g, x, cz, y, af)
    less = ref_lm2_scan(g, af, None, x, np.delete(csel, 1, axis=1), y)
    n, q_base = x.shape
    df, df_less = n - (q_base + 1 + k), n - (q_base + k)
    assert np.all(got[:, 8] == 0.0) and np.isnan(got[:, 9]).all() and np.isnan(got[:, 10]).all() and np.all(got[:, 11] == 1.0)
    worst = 0.0
    for a_got, a_less in ((0, 0), (1, 1), (3, 2)):
        b, se = less[:, 4 * a_less], less[:, 4 * a_less + 1] * math.sqrt(df_less / df)
        scale = np.maximum(np.abs(b), se)
        worst = max(worst, float(np.max(np.abs(got[:, 4 * a_got] - b) / scale)), float(np.max(np.abs(got[:, 4 * a_got + 1] - se) / scale)))
    print(f"zero interaction column: other coefficients against the fit without it {worst:.2e}")
    assert worst <= TOL
    t = 4 * (1 + k)
    for r in range(g.shape[0]):
        stat = less[r, 4 * k] * df / df_less                 # the smaller model's interaction statistic on this model's sigma^2
        assert abs(got[r, t] - stat) <= TOL * max(1.0, stat)
        p = ref_chi2_sf(got[r, t], float(k))
        assert abs(got[r, t + 1] - p) <= TOL * max(1.0, stat) * p


# ---- mirror function and command line --------------------------------------------------------------------------------------------

N_CLI, M_CLI = 300, 400


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    """A PLINK prefix of 300 samples x 400 SNPs (rare and badly called rows among them), a phenotype table with 12 samples
    unphenotyped and a 3-column covariate table."""
    d = tmp_path_factory.mktemp("lm2cli")
    rng = np.random.default_rng(77)
    p = rng.uniform(0.1, 0.5, size=M_CLI)
    p[::17] = 0.004
    g = rng.binomial(2, p[:, None], size=(M_CLI, N_CLI)).astype(np.int8)
    miss = np.full(M_CLI, 0.02)
    miss[5::23] = 0.2
    g[rng.random((M_CLI, N_CLI)) < miss[:, None]] = -9
    ids = [f"s{i}" for i in range(N_CLI)]
    bim = bed.Bim(["1"] * M_CLI, [f"rs{j}" for j in range(M_CLI)], [1000 + 10 * j for j in range(M_CLI)], ["A"] * M_CLI, ["G"] * M_CLI)
    pre = str(d / "panel")
    bed.write_bed(pre, bed.pack_dosage(g), ids, bim)
    cov = rng.normal(size=(N_CLI, 3)) + np.array([0.0, 5.0, 10.0])
    gc = np.where(g[1] < 0, 0, g[1]).astype(np.float64)
    y = 0.4 * gc + 0.2 * gc * (cov[:, 2] - 10.0) + cov @ np.array([0.3, -0.2, 0.1]) + rng.normal(size=N_CLI)
    y[rng.permutation(N_CLI)[:12]] = np.nan
    with open(pre + ".pheno.tsv", "w") as fh:
        fh.write("id\ttrait\n")
        for i in range(N_CLI):
            fh.write(f"{ids[i]}\t{'NA' if np.isnan(y[i]) else repr(float(y[i]))}\n")
    with open(pre + ".cov.tsv", "w") as fh:
        fh.write("id\tc0\tc1\tc2\n")
        for i in range(N_CLI):
            fh.write(ids[i] + "\t" + "\t".join(repr(float(v)) for v in cov[i]) + "\n")
    return pre, g, ids, bim, cov, y


def _kept(g, sel):
    """The rows `jx gwas` keeps at its defaults (-maf 0.02, -geno 0.05) over the samples `sel`, in f32 like the filter."""
    gs = g[:, sel]
    af, miss = ref_alt_freq(gs)
    rate = miss.astype(np.float32) / np.float32(len(sel))
    keep = ~(rate > np.float32(0.05)) & ~(np.minimum(af, np.float32(1.0) - af) < np.float32(0.02))
    return np.nonzero(keep)[0], af, miss


def _read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:-1]]


def test_cli_writes_both_tables(prefix, tmp_path, capsys):
    pre, g, ids, bim, cov, y = prefix
    out = str(tmp_path / "run")
    assert cli.main(["gwas", "-bfile", pre, "-p", pre + ".pheno.tsv", "-c", pre + ".cov.tsv", "-lm", "-lm2", "0,2", "-o", out]) == 0
    said = capsys.readouterr().out
    assert "GRM" not in said and "-lm2:" in said and "-lm:" in said
    lm_path, lm2_path = out + ".trait.lm.tsv", out + ".trait.lm2.tsv"
    assert os.path.exists(lm_path) and os.path.exists(lm2_path)
    sel = np.nonzero(np.isfinite(y))[0]
    rows, af, miss = _kept(g, sel)
    assert 0 < len(rows) < M_CLI
    x = np.concatenate([np.ones((len(sel), 1)), cov[sel]], axis=1)
    want = ref_lm2_scan(g[rows][:, sel], af[rows], None, x, cov[sel][:, [0, 2]], y[sel])
    head, body = _read_tsv(lm2_path)
    assert head == ["chrom", "pos", "snp", "allele0", "allele1", "af", "miss", "beta", "se", "chisq", "pwald", "beta_i0", "se_i0",
                    "pwald_i0", "beta_i2", "se_i2", "pwald_i2", "chisq_int_joint", "p_int_joint", "chisq_joint", "p_joint"]
    assert [b[2] for b in body] == [bim.snp[j] for j in rows]                  # the kept SNPs, in BED order
    fixed = lambda txt, v: abs(float(txt) - v) <= 0.5001e-4 + 1e-9 * abs(v)               # noqa: E731  `{:.4}`
    sci = lambda txt, v, stat=1.0: abs(float(txt) - v) <= (0.5001e-4 + 1e-9 * max(1.0, stat)) * abs(v)   # noqa: E731  `{:.4e}`
    for i, b in enumerate(body):
        w = want[i]
        assert b[:2] == ["1", str(bim.pos[rows[i]])] and b[3:5] == ["A", "G"]
        assert b[5] == f"{float(af[rows[i]]):.4f}" and b[6] == str(int(miss[rows[i]]))
        assert fixed(b[7], w[0]) and fixed(b[8], w[1]) and sci(b[9], w[2]) and sci(b[10], w[3], w[2]), (i, b, w)
        for j in (1, 2):
            c = b[8 + 3 * j:11 + 3 * j]
            assert fixed(c[0], w[4 * j]) and fixed(c[1], w[4 * j + 1]) and sci(c[2], w[4 * j + 3], w[4 * j + 2]), (i, j, c, w)
        assert sci(b[17], w[12]) and sci(b[18], w[13], w[12]) and sci(b[19], w[14]) and sci(b[20], w[15], w[14]), (i, b, w)
    # the LM table is the one `lm_block_assoc_packed_to_tsv` writes for the same rows
    twin = str(tmp_path / "twin.lm.tsv")
    packed = bed.pack_dosage(g)
    jx.lm_block_assoc_packed_to_tsv(y[sel], x, jx.lm_precompute_ixx_qr(x), packed[rows], N_CLI, np.zeros(len(rows), dtype=bool),
                                    af[rows], (miss[rows] + 0.5).astype(np.float32) / np.float32(N_CLI),
                                    [bim.chrom[j] for j in rows], [bim.pos[j] for j in rows], [bim.snp[j] for j in rows],
                                    [bim.a0[j] for j in rows], [bim.a1[j] for j in rows], twin, sample_indices=sel)
    assert open(lm_path, "rb").read() == open(twin, "rb").read()


def test_cli_lm2_without_covariates_runs_lm(prefix, tmp_path, capsys):
    pre = prefix[0]
    out = str(tmp_path / "nocov")
    assert cli.main(["gwas", "-bfile", pre, "-p", pre + ".pheno.tsv", "-lm2", "0", "-o", out]) == 0
    assert "LM2 received no external covariates from -c; falling back to LM." in capsys.readouterr().out
    assert os.path.exists(out + ".trait.lm.tsv") and not os.path.exists(out + ".trait.lm2.tsv")


def test_mirror_functions_on_a_sample_subset(prefix, tmp_path):
    """`lm2_stream_bed_to_tsv` with `sample_ids` in an order of their own and its own row filter (no call at all drops a row), then
    with prepared row metadata and flipped rows; `lm_stream_bed_to_tsv` writes the LM table of the same rows."""
    pre, g, ids, bim, cov, y = prefix
    sel = np.nonzero(np.isfinite(y))[0][::-1][:150].copy()
    x = np.concatenate([np.ones((len(sel), 1)), cov[sel][:, :1]], axis=1)
    gs = g[:, sel]
    af, miss = ref_alt_freq(gs)
    rate = miss.astype(np.float32) / np.float32(len(sel))
    rows = np.nonzero(~(rate > np.float32(0.1)) & ~(np.minimum(af, np.float32(1.0) - af) < np.float32(0.05)))[0]
    path = str(tmp_path / "m.lm2.tsv")
    wrote, scanned = jx.lm2_stream_bed_to_tsv(pre, y[sel], x, cov[sel], [1], path, sample_ids=[ids[i] for i in sel], maf_threshold=0.05,
                                              max_missing_rate=0.1)
    assert (wrote, scanned) == (len(rows), M_CLI)
    head, body = _read_tsv(path)
    assert head[11:14] == ["beta_i1", "se_i1", "pwald_i1"] and [b[2] for b in body] == [bim.snp[j] for j in rows]
    want = ref_lm2_scan(gs[rows], af[rows], None, x, cov[sel][:, [1]], y[sel])
    for i, b in enumerate(body):
        assert b[6] == str(int(miss[rows[i]]))
        assert abs(float(b[7]) - want[i, 0]) <= 0.5001e-4 + 1e-9 * abs(want[i, 0]) and abs(float(b[11]) - want[i, 4]) <= 0.5001e-4 + 1e-9 * abs(want[i, 4])
    # prepared metadata: a strided choice of rows, every other one flipped
    pick = rows[::3]
    flip = (np.arange(len(pick)) % 2).astype(bool)
    wrote, scanned = jx.lm2_stream_bed_to_tsv(pre, y[sel], x, cov[sel], [1], path, sample_ids=[ids[i] for i in sel], row_indices=pick,
                                              row_flip=flip, row_missing=miss[pick].astype(np.float32), row_maf=af[pick])
    assert (wrote, scanned) == (len(pick), len(pick))
    _head, body = _read_tsv(path)
    want = ref_lm2_scan(gs[pick], af[pick], flip, x, cov[sel][:, [1]], y[sel])
    for i, b in enumerate(body):
        assert b[2] == bim.snp[pick[i]] and b[6] == str(int(miss[pick[i]]))
        assert abs(float(b[7]) - want[i, 0]) <= 0.5001e-4 + 1e-9 * abs(want[i, 0])
    lm_path, twin = str(tmp_path / "m.lm.tsv"), str(tmp_path / "m.twin.tsv")
    assert jx.lm_stream_bed_to_tsv(pre, y[sel], x, None, lm_path, sample_ids=[ids[i] for i in sel], maf_threshold=0.05,
                                   max_missing_rate=0.1) == (len(rows), M_CLI)
    jx.lm_block_assoc_packed_to_tsv(y[sel], x, jx.lm_precompute_ixx_qr(x), bed.pack_dosage(g)[rows], N_CLI,
                                    np.zeros(len(rows), dtype=bool), af[rows], (miss[rows] + 0.5).astype(np.float32) / np.float32(N_CLI),
                                    [bim.chrom[j] for j in rows], [bim.pos[j] for j in rows], [bim.snp[j] for j in rows],
                                    [bim.a0[j] for j in rows], [bim.a1[j] for j in rows], twin, sample_indices=sel)
    assert open(lm_path, "rb").read() == open(twin, "rb").read()
