"""GPU tests of KING (`jx grm -king`; csrc/k_king.hip) against the numpy restatement in tests/test_king_host.py.

Everything is compared exactly.  The pair counts are integer sums; the kinship is one f64 subtraction of exact integers and one
correctly rounded f64 division in the restatement's order, so the device's value has the restatement's bits; the graph and the
prune are integer algorithms.  Shapes: n = 2 (one pair), 81 (two 64-tiles, inside one 128-record), 129 / 257 (one sample past one /
two 128-tiles), 301 (a tail that is no multiple of 16); m around the kernel's 64-row step (1, 63, 65, 129) and 333."""
import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx

from test_king_host import (king_panel, ref_counts, ref_graph, ref_kinship, ref_pairs, ref_prune, ref_site_keep,   # noqa: E402
                            render_king)

pytestmark = pytest.mark.gpu

BK = 64                                                       # KING_BK of csrc/k_king.hip
NS = [2, 81, 129, 257, 301]
MS = [1, BK - 1, BK + 1, 2 * BK + 1, 333]
MISS = [0.0, 0.1]
FORMS = ["64", "128"]                                         # JXGPU_KING_TILE: every launch form of the fused kernel
EVERY_FINITE = -1e300


@pytest.fixture(scope="module")
def panels():
    """(n, miss) -> dosages (333, n); the cases with fewer rows take the first m rows."""
    out = {}
    for n in NS:
        for miss in MISS:
            if n == 2:
                out[n, miss] = np.ascontiguousarray(king_panel(1, 333, miss, seed=3)[:, [0, 4]])    # a sample and its duplicate
            else:
                out[n, miss] = king_panel((n - 1) // 4, 333, miss, seed=n)
            assert out[n, miss].shape == (333, n)
    return out


@pytest.fixture(scope="module")
def refs(panels):
    """(n, miss, m) -> (6, n, n) int64 counts of the restatement, computed once."""
    return {(n, miss, m): ref_counts(g[:m]) for (n, miss), g in panels.items() for m in MS}


def _panel(g):
    return jx._panel(torch.from_numpy(bed.pack_dosage(g)).cuda(), g.shape[1])


def _rectangles(n):
    """(i0, i1, j0, j1): inside one 16-sample group, across a group, across the 64-tile and the 128-record edge, the tail, one row."""
    if n == 2:
        return [(0, 1, 1, 2), (1, 2, 0, 2)]
    r = [(3, 13, 18, 30), (17, 18, 0, n), (60, 70, 5, 66), (0, n, 63, 65), (n - 7, n, 1, n - 1), (70, 81, 70, 81)]
    if n > 128:
        r += [(120, n, 60, 129), (127, 129, 127, 129)]
    if n > 256:
        r += [(250, n, 0, 3), (1, 2, 255, n)]
    return r


def _same_table(got, want):
    assert [a.dtype for a in got] == [np.uint32, np.uint32, np.uint32, np.float64]
    assert all(a.shape == b.shape for a, b in zip(got, want)), (got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "pair set"
    assert np.array_equal(got[2], want[2]), "ibs0"
    assert got[3].tobytes() == want[3].astype(np.float64).tobytes(), "kinship bits"


@pytest.mark.parametrize("n", NS)
def test_pair_counts_are_the_restatements(panels, refs, n):
    for miss in MISS:
        for m in MS:
            g, want = panels[n, miss][:m], refs[n, miss, m]
            panel = _panel(g)
            got = jx._king_counts(panel, 0, n, 0, n)
            assert got.dtype == np.int32 and got.shape == (6, n, n)
            for p in range(6):
                assert np.array_equal(got[p], want[p]), (n, miss, m, p)
            if m in (1, 333):
                for i0, i1, j0, j1 in _rectangles(n):
                    got = jx._king_counts(panel, i0, i1, j0, j1)
                    assert got.shape == (6, i1 - i0, j1 - j0)
                    assert np.array_equal(got, want[:, i0:i1, j0:j1]), (n, miss, m, i0, i1, j0, j1)
    g = panels[n, 0.1]
    got = jx.king_pair_counts_packed(bed.pack_dosage(g), n, 1, n, 0, n - 1)                     # a host payload, the public entry
    assert np.array_equal(got, refs[n, 0.1, 333][:, 1:n, 0:n - 1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", NS)
def test_fused_path_finds_every_finite_pair(panels, refs, monkeypatch, n, form):
    monkeypatch.setenv("JXGPU_KING_TILE", form)
    for miss in MISS:
        for m in MS:
            c = refs[n, miss, m]
            want = ref_pairs(c, EVERY_FINITE)
            got = jx._king_related_pairs(_panel(panels[n, miss][:m]), EVERY_FINITE)
            _same_table(got, want)
            n_nan = int(np.isnan(ref_kinship(c)[np.triu_indices(n, 1)]).sum())
            assert got[0].shape[0] == n * (n - 1) // 2 - n_nan
            if n > 2:
                assert n_nan >= n - 1                         # the pairs of the all-missing sample are absent


@pytest.mark.parametrize("form", ["default"] + FORMS)
def test_thresholds(panels, refs, monkeypatch, form):
    if form != "default":
        monkeypatch.setenv("JXGPU_KING_TILE", form)
    n, m = 81, 333
    g, c = panels[n, 0.0], refs[n, 0.0, m]
    kin = ref_kinship(c)[np.triu_indices(n, 1)]
    assert int((kin == 0.25).sum()) >= 1                      # 0.25 is attained: tests >= against >
    packed = bed.pack_dosage(g)
    for thr in (0.05, 0.177, 0.25):
        above, below, nan = int((kin >= thr).sum()), int((kin < thr).sum()), int(np.isnan(kin).sum())
        print(f"threshold {thr}: {above} pairs at or above, {below} below, {nan} without a kinship")
        assert above >= 50 and below >= 1000 and nan >= 1
        want = ref_pairs(c, thr)
        assert want[0].shape[0] == above
        _same_table(jx.king_related_pairs_packed(packed, n, thr), want)


def test_capacity_retry_gives_the_identical_table(panels, refs):
    n, m = 129, 333
    panel = _panel(panels[n, 0.1])
    want = ref_pairs(refs[n, 0.1, m], 0.05)
    assert want[0].shape[0] > 16
    t_small, t_large = {}, {}
    _same_table(jx._king_related_pairs(panel, 0.05, 16, t_small), want)
    _same_table(jx._king_related_pairs(panel, 0.05, None, t_large), want)
    assert (t_small["launches"], t_large["launches"]) == (2, 1) and t_small["rows"] == want[0].shape[0]
    _same_table(jx.king_related_pairs_packed(bed.pack_dosage(panels[n, 0.1]), n, 0.05, max_rows=16), want)
    _same_table(jx._king_related_pairs(panel, EVERY_FINITE, 16), ref_pairs(refs[n, 0.1, m], EVERY_FINITE))


def _bed_case(tmp_path):
    g = king_panel(20, 333, 0.02, seed=5).copy()
    g[7] = 0                                                  # monomorphic: fails every MAF filter
    g[8, :] = np.where(np.arange(g.shape[1]) < 3, 1, 0)       # minor allele frequency 3 / 162: 0.01 <= . < 0.02
    g[9, 10:40] = -9                                          # 31 of 81 calls missing: fails every missing filter
    g[11] = np.where(g[11] < 0, 0, g[11])
    g[11, 10:18] = -9                                         # 8 of 81 calls missing: passes 0.1, fails 0.05
    m, n = g.shape
    prefix = str(tmp_path / "fam")
    ids = [f"s{i}" for i in range(n)]
    bed.write_bed(prefix, bed.pack_dosage(g), ids, bed.Bim(["1"] * m, [f"rs{i}" for i in range(m)], list(range(1, m + 1)), ["A"] * m,
                                                           ["G"] * m))
    return g, prefix, ids


def _ref_unrelated(g, threshold):
    n = g.shape[1]
    pairs = ref_pairs(ref_counts(g), threshold)
    nbrs = ref_graph(n, pairs[0], pairs[1])
    kept, removed = ref_prune(nbrs)
    return pairs, nbrs, kept, removed


def test_graph_prune_and_bed_route(tmp_path):
    g, prefix, _ids = _bed_case(tmp_path)
    n = g.shape[1]
    keep = ref_site_keep(g, 0.01, 0.1)
    assert not keep[7] and keep[8] and not keep[9] and keep[11] and int(keep.sum()) < g.shape[0]
    gk = g[keep]
    pairs, nbrs, kept_want, removed_want = _ref_unrelated(gk, 0.05)
    assert len(removed_want) >= 20 and len(kept_want) >= 20
    kept, removed, edges, sites = jx.king_unrelated_set_from_bed(prefix + ".bed", threads=2)
    assert kept.dtype == np.uint32 and removed.dtype == np.uint32
    assert (kept.tolist(), removed.tolist(), edges, sites) == (kept_want, removed_want, int(pairs[0].shape[0]), int(keep.sum()))
    kept, removed, edges, sites = jx.king_unrelated_set_packed(bed.pack_dosage(gk), n)
    assert (kept.tolist(), removed.tolist(), edges, sites) == (kept_want, removed_want, int(pairs[0].shape[0]), int(keep.sum()))
    got_nbrs, degrees, edges, sites = jx.king_related_graph_packed(torch.from_numpy(bed.pack_dosage(gk)).cuda(), n)
    assert [v.tolist() for v in got_nbrs] == nbrs and degrees.tolist() == [len(v) for v in nbrs] and degrees.dtype == np.int32
    assert edges == int(pairs[0].shape[0]) and sites == int(keep.sum())
    # another threshold, another filter
    keep2 = ref_site_keep(g, 0.02, 0.05)
    assert not keep2[8] and not keep2[11]
    pairs2, _nb2, kept2, removed2 = _ref_unrelated(g[keep2], 0.177)
    got = jx.king_unrelated_set_from_bed(prefix, 0.02, 0.05, 0.0, False, 0.177)
    assert (got[0].tolist(), got[1].tolist(), got[2], got[3]) == (kept2, removed2, int(pairs2[0].shape[0]), int(keep2.sum()))


def test_cli_end_to_end(tmp_path, capsys):
    g, prefix, ids = _bed_case(tmp_path)
    keep = ref_site_keep(g, 0.02, 0.05)                       # the command's own -maf / -geno defaults
    pairs, _nbrs, kept, removed = _ref_unrelated(g[keep], 0.05)
    out = str(tmp_path / "res")
    assert cli.main(["grm", "-bfile", prefix, "-king", "-o", out]) == 0
    text = capsys.readouterr().out
    assert f"n={g.shape[1]} sites={int(keep.sum())} edges={int(pairs[0].shape[0])} kept={len(kept)} removed={len(removed)}" in text
    want = render_king(ids, int(keep.sum()), pairs, kept, removed)
    for suffix, body in zip((".king.kin0", ".king.unrelated.id", ".king.related.id"), want):
        assert open(out + suffix, "rb").read() == body.encode(), suffix
    # an explicit threshold and filter
    keep = ref_site_keep(g, 0.01, 0.1)
    pairs, _nbrs, kept, removed = _ref_unrelated(g[keep], 0.25)
    assert cli.main(["grm", "-bfile", prefix, "-king", "0.25", "-maf", "0.01", "-geno", "0.1", "-o", out]) == 0
    want = render_king(ids, int(keep.sum()), pairs, kept, removed)
    for suffix, body in zip((".king.kin0", ".king.unrelated.id", ".king.related.id"), want):
        assert open(out + suffix, "rb").read() == body.encode(), suffix


def test_pair_stats_of_a_duplicate(panels, refs):
    n = 81
    g = panels[n, 0.0]
    packed = bed.pack_dosage(g)
    st = jx.king_pair_stats(packed, n, 0, n - 1)
    assert st["ibs0"] == 0 and st["kinship"] == 0.5 and st["ibs1"] == 0 and st["ibs2"] == st["shared_nonmissing"] == 333
    assert st["het_i_obs"] == st["het_j_obs"] == st["both_het"]
    c = refs[n, 0.0, 333]
    st = jx.king_pair_stats(packed, n, 9, 2)                  # i > j: the het counts keep their sides
    assert (st["shared_nonmissing"], st["ibs0"], st["both_het"], st["het_i_obs"], st["het_j_obs"]) == tuple(
        int(c[p][9, 2]) for p in (0, 1, 3, 4, 5))
    assert st["ibs2"] == int(c[3][9, 2] + c[2][9, 2]) and st["ibs1"] == int(c[0][9, 2] - c[1][9, 2] - c[2][9, 2] - c[3][9, 2])
    assert st["kinship"] == ref_kinship(c)[9, 2]
    st = jx.king_pair_stats(packed, n, 5, 2)                  # the all-missing sample
    assert st["shared_nonmissing"] == 0 and np.isnan(st["kinship"])


def test_two_runs_give_the_same_table(panels):
    panel = _panel(panels[301, 0.1])
    a = jx._king_related_pairs(panel, 0.0)
    b = jx._king_related_pairs(panel, 0.0)
    assert a[0].shape[0] > 1000
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
