"""GPU tests of `jx gstats` (csrc/k_ld.hip `jxg_ld_score_p32`, csrc/k_gstats.hip `jxg_sample_counts_p32`) against the numpy
restatement of the reference in tests/test_gstats_host.py.

LD scores: the pair values are bit-identical to the restatement's (integer sums, the same f64 expressions, no contraction); only
the order in which at most M_i non-negative terms are added differs.  Each order lies within (M_i - 1) 2^-53 of the true sum,
relatively, so |l - l_ref| <= 4 M_i 2^-53 l_ref is the sum of both with a factor two of room: a failure is a bug, not noise.  The
sample counts are integers and the f32 rates are the reference's expressions: both are compared exactly."""
import os

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx
from janusx_amd._lib import lib

from test_ld_host import LdRef   # noqa: E402
from test_gstats_host import (M, _write_prefix, gstats_panel, ref_ldscore, ref_sample_counts, ref_sample_rates,   # noqa: E402
                              ref_site_rates, render_table)

pytestmark = pytest.mark.gpu

# variants 1, 31, 32, 33 straddle the 32-row block, 2000 > m is the whole group; cM = position / 1e5
WINDOWS = [("variants", 1), ("variants", 31), ("variants", 32), ("variants", 33), ("variants", 100), ("variants", 2000), ("bp", 1),
           ("bp", 50000), ("cm", 0.5)]


@pytest.fixture(scope="module")
def panels():
    out = {}
    for name in ("complete", "missing"):
        g, pos, cm = gstats_panel(name)
        out[name] = (g, pos, cm, bed.pack_dosage(g), LdRef(g, 1.0))
    return out


def _check_scores(m_got, l_got, m_want, l_want, what):
    assert m_got.dtype == np.int64 and l_got.dtype == np.float64 and m_got.shape == m_want.shape and l_got.shape == l_want.shape
    assert np.array_equal(m_got, m_want), what
    bound = 4.0 * m_want * 2.0 ** -53 * l_want
    err = np.abs(l_got - l_want)
    worst = int(np.argmax(err - bound))
    print(f"{what}: mean score {l_want.mean():.3f}, max |l - l_ref| {err.max():.2e}, worst row {worst}: {err[worst]:.2e} against a "
          f"bound of {bound[worst]:.2e}; bit-identical rows {int((l_got == l_want).sum())} / {len(l_want)}")
    assert (err <= bound).all(), (what, worst, float(l_got[worst]), float(l_want[worst]))


@pytest.mark.parametrize("panel", ["complete", "missing"])
def test_ld_scores_are_the_restatements(panels, panel):
    g, pos, cm, packed, ref = panels[panel]
    n = g.shape[1]
    chrom = np.zeros(M, dtype=np.int32)
    share = float(ref.st["has_missing"].mean())
    if panel == "complete":
        assert share == 0.0
    else:
        assert 0.4 <= share <= 0.6, share                     # both formulas and both launch forms run
    for kind, w in WINDOWS:
        m_want, l_want = ref_ldscore(g, chrom, pos, cm, kind, w, ref)
        if panel == "complete" and (kind, w) in (("variants", 1), ("variants", 32)):
            assert l_want.mean() > (2.0 if w == 1 else 4.5), l_want.mean()    # the panel has LD to find (2.4 and 5.06)
        m_got, l_got = jx.ldscore_packed(packed, n, chrom, pos, cm, kind, w)
        _check_scores(m_got, l_got, m_want, l_want, f"{panel} {kind} {w}")


def test_ld_score_edges(panels, tmp_path):
    """A row with every call missing, a row with two calls, monomorphic rows (complete and with missing calls), identical rows,
    a chromosome boundary inside a 32-row block, interleaved codes, positions permuted inside a chromosome, and `chr1` / `1`
    tokens through the BED route."""
    g, pos, cm, _packed, _ref = panels["missing"]
    g, pos = g.copy(), pos.copy()
    g[100] = -9                                               # every call missing
    g[101] = -9
    g[101, :2] = [1, 2]                                       # two calls: pairs with N <= 1 or no variance
    g[200] = 0                                                # monomorphic, complete
    g[201] = np.where(g[201] >= 0, 2, -9)                     # monomorphic with missing calls
    g[300] = g[299]                                           # identical rows
    n = g.shape[1]
    packed, ref = bed.pack_dosage(g), LdRef(g, 1.0)
    chrom = np.zeros(M, dtype=np.int32)
    chrom[500:] = 1                                           # 500 = 15 * 32 + 20
    rng = np.random.default_rng(3)
    perm = pos.copy()
    perm[:500] = rng.permutation(pos[:500])                   # positions permuted inside a chromosome
    for cc, ps, kind, w in ((chrom, pos, "variants", 40), (chrom, pos, "bp", 30000), (chrom, perm, "bp", 30000),
                            (chrom, perm, "cm", 0.3), ((np.arange(M) % 2).astype(np.int32), pos, "variants", 40),
                            ((np.arange(M) % 2).astype(np.int32), perm, "bp", 40000)):
        cmv = ps / 1.0e5
        m_want, l_want = ref_ldscore(g, cc, ps, cmv, kind, w, ref)
        m_got, l_got = jx.ldscore_packed(packed, n, cc, ps, cmv, kind, w)
        _check_scores(m_got, l_got, m_want, l_want, f"edges {kind} {w}")
        if np.array_equal(ps, pos) and cc is chrom:
            assert l_got[100] == 0.0 and l_got[200] == 0.0 and l_got[201] == 0.0          # self term 0, every pair value 0
            assert l_got[300] >= 2.0 and l_got[299] >= 2.0                                    # self + the identical row
    # the all-missing row adds 0 to every other row: over the whole group the scores are those of the panel without it
    keep = np.arange(M) != 100
    one = np.zeros(M, dtype=np.int32)
    m_with, l_with = jx.ldscore_packed(packed, n, one, pos, None, "variants", 2000)
    m_wo, l_wo = jx.ldscore_packed(bed.pack_dosage(g[keep]), n, one[keep], pos[keep], None, "variants", 2000)
    assert (m_with == M).all() and (m_wo == M - 1).all() and l_with[100] == 0.0
    assert np.max(np.abs(l_with[keep] - l_wo) / l_wo.clip(1.0)) <= 4.0 * M * 2.0 ** -53
    # chr1 / 1 tokens through the BED route are one chromosome; a second chromosome comes back later in the file
    tokens = ["chr1"] * 300 + ["2"] * 200 + ["1"] * (M - 500)
    codes = np.array([0] * 300 + [1] * 200 + [0] * (M - 500), dtype=np.int32)
    prefix = _write_prefix(tmp_path, "edges", g, tokens, perm, perm / 1.0e5)
    for kind, w in (("snp", 40.0), ("kb", 30000.0), ("genetic", 0.3)):
        m_want, l_want = ref_ldscore(g, codes, perm, perm / 1.0e5, {"snp": "variants", "kb": "bp", "genetic": "cm"}[kind],
                                     int(w) if kind != "genetic" else w, ref)
        m_got, l_got, n_got = jx.gstats_bed_ldscore(prefix + ".bed", kind, w, threads=3)
        assert n_got == n
        _check_scores(m_got, l_got, m_want, l_want, f"BED route {kind} {w}")


def test_ld_score_budget_and_determinism(panels):
    g, pos, cm, packed, _ref = panels["missing"]
    n = g.shape[1]
    chrom = np.zeros(M, dtype=np.int32)
    chrom[500:] = 1
    dev = torch.from_numpy(packed).cuda()
    for kind, w, budget in (("variants", 100, 32 * 9 * 8 * 3), ("bp", 50000, 32 * 8 * 8 * 2), ("variants", 2000, 32 * 32 * 8 * 2)):
        t0, t1 = {}, {}
        m_a, l_a = jx.ldscore_packed(packed, n, chrom, pos, cm, kind, w, timings=t0)
        m_b, l_b = jx.ldscore_packed(dev, n, chrom, pos, cm, kind, w)
        assert np.array_equal(m_a, m_b) and np.array_equal(l_a, l_b)              # two calls: bit-identical
        m_c, l_c = jx.ldscore_packed(dev, n, chrom, pos, cm, kind, w, partial_budget_bytes=budget, timings=t1)
        assert t0["ranges"] == 1 and t1["ranges"] >= 8, (t0, t1)
        assert np.array_equal(m_a, m_c) and np.array_equal(l_a, l_c), (kind, w)   # the budget does not change a bit
    with pytest.raises(RuntimeError, match=r"budget of 64 bytes is below the \d+ bytes"):
        jx.ldscore_packed(dev, n, chrom, pos, cm, "variants", 100, partial_budget_bytes=64)


def test_sample_counts_are_numpys(panels):
    chunk = lib().jxg_sample_counts_chunk()                   # SC_CHUNK of csrc/k_gstats.hip: SNP rows per workgroup
    assert chunk == 7680
    rng = np.random.default_rng(9)

    def check(g, device=False):
        n = g.shape[1]
        packed = bed.pack_dosage(g)
        got = jx.sample_counts_packed(torch.from_numpy(packed).cuda() if device else packed, n)
        assert got.dtype == np.int32 and got.shape == (2, n)                      # no slot for the pad samples of the last tile
        assert np.array_equal(got, ref_sample_counts(g)), g.shape

    for n in (1, 127, 128, 129):
        for m in (1, 1003):
            g = rng.choice(np.array([0, 1, 2, -9], dtype=np.int8), size=(m, n), p=[0.4, 0.3, 0.2, 0.1])
            if m > 1:
                g[7] = -9                                     # a row with all calls missing
            check(g)
    g601 = panels["missing"][0].copy()
    g601[7] = -9
    check(g601)
    check(g601[:1])
    check(g601, device=True)
    m_long = 2 * chunk + 777                                  # two full SNP chunks and an odd remainder
    g = rng.choice(np.array([0, 1, 2, -9], dtype=np.int8), size=(m_long, 129), p=[0.3, 0.3, 0.2, 0.2])
    g[:, 3] = -9                                              # a sample without a call: count = m
    g[:, 128] = 1                                             # the one sample of the last tile: het everywhere
    check(g)
    check(g, device=True)


def test_mirror_tuples_and_cli(panels, tmp_path, capsys):
    g, pos, _cm, _packed, _ref = panels["missing"]
    m = 300
    g, pos = g[:m].copy(), pos[:m]
    g[5] = -9
    g[:, 11] = -9
    n = g.shape[1]
    tokens = ["chr1"] * 120 + ["X"] * 100 + ["1"] * 80
    codes = np.array([0] * 120 + [1] * 100 + [0] * 80, dtype=np.int32)
    cm = np.round(pos / 1.0e5, 3)
    prefix = _write_prefix(tmp_path, "in", g, tokens, pos, cm)
    maf, lmiss, lhet = ref_site_rates(g)
    imiss, ihet = ref_sample_rates(g)
    # the mirror tuples
    got = jx.gstats_bed_site_stats(prefix, threads=2)
    assert got[3] == n and all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(got[:3], (maf, lmiss, lhet)))
    got = jx.gstats_bed_individual_stats(prefix + ".bim")
    assert got[2] == m and all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(got[:2], (imiss, ihet)))
    got = jx.gstats_bed_joint_stats(prefix)
    assert got[5:] == (n, m) and all(np.array_equal(a, b) for a, b in zip(got[:5], (maf, lmiss, lhet, imiss, ihet)))
    got = jx.gstats_bed_joint_stats(prefix, False, True, False, False, True)
    assert got[0] is None and got[2] is None and got[3] is None and np.array_equal(got[1], lmiss) and np.array_equal(got[4], ihet)
    got = jx.gstats_bed_joint_stats(prefix, site_miss=False, individual_miss=False, individual_het=False)
    assert got[1] is None and got[3] is None and got[4] is None and np.array_equal(got[0], maf) and got[5:] == (n, m)
    # the command line
    out = str(tmp_path / "res" / "stats")
    assert cli.main(["gstats", "-bfile", prefix, "-freq", "-miss", "-het", "-ldsc", "50", "-o", out, "-t", "4"]) == 0
    text = capsys.readouterr().out
    assert text.count("not written") == 1 and "PDF" in text
    sites = [(c, str(int(p))) for c, p in zip(tokens, pos)]
    fam = [(f"id{i}", f"id{i}") for i in range(n)]
    for suffix, header, leads, name, values in (("freq", "chr\tpos", sites, "freq", maf), ("lmiss", "chr\tpos", sites, "miss", lmiss),
                                                ("lhet", "chr\tpos", sites, "het", lhet), ("imiss", "fid\tiid", fam, "miss", imiss),
                                                ("ihet", "fid\tiid", fam, "het", ihet)):
        assert open(f"{out}.{suffix}").read() == render_table(header, leads, name, values), suffix
    assert not [f for f in os.listdir(os.path.dirname(out)) if f.endswith((".pdf", ".log"))]

    def check_ldsc(path, kind, w):
        m_want, l_want = ref_ldscore(g, codes, pos, cm, kind, w)
        lines = open(path).read().splitlines()
        assert lines[0] == "chr\tpos\tM\tldsc" and len(lines) == m + 1
        for (c, p), mw, lw, line in zip(sites, m_want, l_want, lines[1:]):
            f = line.split("\t")
            assert f[:3] == [c, p, str(int(mw))] and len(f[3].split(".")[1]) == 6, line
            assert abs(float(f[3]) - lw) <= 1e-6, (line, lw)  # half a unit of the printed digit, and a last-digit flip

    check_ldsc(f"{out}.{n}.50snp.ldsc", "variants", 50)
    outdir = str(tmp_path / "dir") + os.sep
    assert cli.main(["gstats", "-bfile", prefix + ".bed", "-ldsc", "0.5cm", "-o", outdir, "-prefix", "p2"]) == 0
    check_ldsc(os.path.join(outdir, f"p2.{n}.0.5cm.ldsc"), "cm", 0.5)
    assert sorted(os.listdir(outdir)) == [f"p2.{n}.0.5cm.ldsc"]                 # only what was asked for
    assert cli.main(["gstats", "-bfile", prefix, "-freq", "-o", outdir, "-prefix", "p3"]) == 0
    assert open(os.path.join(outdir, "p3.freq")).read() == render_table("chr\tpos", sites, "freq", maf)
    assert cli.main(["gstats", "-bfile", prefix, "-ldsc", "-o", outdir, "-prefix", "p4"]) == 0
    check_ldsc(os.path.join(outdir, f"p4.{n}.100kb.ldsc"), "bp", 100000)
