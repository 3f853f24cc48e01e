"""GPU tests of LD pruning and the LD-block r^2 matrix on the packed genotypes (csrc/k_ld.hip): the keep mask of
`bed_packed_ld_prune_maf_priority` must equal the numpy restatement of the reference algorithm (tests/test_ld_host.py) bit for bit
-- the pair sums are integers and the f64 expression order is the reference's, so a mismatch is a bug, never noise --, the six
integer sums of `jxg_ld_sums_p32` must equal numpy's exactly, and the f32 LD-block matrix must lie within 2e-7 of the f64
restatement (the f32 rounding of an r^2 in [0, 1], 6e-8, with a factor three of room)."""
import os

import numpy as np
import pytest
import torch

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx

from test_ld_host import (PANELS, PARAM_SETS, check_ref_conditions, ld_panel, ref_ld_matrix, ref_prune_panel,   # noqa: E402
                          ref_six_sums)

pytestmark = pytest.mark.gpu

M = 4000


@pytest.fixture(scope="module")
def panels():
    out = {}
    for name, (n, missing) in PANELS.items():
        g, pos = ld_panel(n, M, 11 if missing else 7, missing)
        out[name] = (g, pos, bed.pack_dosage(g))
    return out


_REF = {}


def _ref(panels, name, params):
    """The restatement's keep mask and counters on a whole panel with one chromosome (computed once per module)."""
    key = (name,) + tuple(params)
    if key not in _REF:
        g, pos, _ = panels[name]
        _REF[key] = ref_prune_panel(g, np.zeros(M, dtype=np.int32), pos, *params)
    return _REF[key]


def _prune(packed, n, chrom, pos, window_bp, window_variants, step, r2, **kw):
    return jx.bed_packed_ld_prune_maf_priority(packed, n, chrom, pos, window_bp=window_bp, window_variants=window_variants,
                                               step_variants=step, r2_threshold=r2, **kw)


@pytest.mark.parametrize("panel", ["complete", "missing"])
@pytest.mark.parametrize("params", PARAM_SETS + [(None, 50, 5, 1.0)])
def test_prune_keep_mask_is_the_restatements(panels, panel, params):
    g, pos, packed = panels[panel]
    chrom = np.zeros(M, dtype=np.int32)
    wbp, wv, step, r2 = params
    want, ref = _ref(panels, panel, params)
    print(f"{panel} {params}: restatement keeps {int(want.sum())} / {M}, in-LD pairs by formula {ref.hits}, "
          f"closest pair to the threshold {ref.min_margin:.3e} (relative), {ref.asked} pairs asked")
    if r2 < 1.0:
        check_ref_conditions(want, ref)
        assert ref.hits["clean"] > 0
        assert (ref.hits["pairwise"] > 0) == (panel == "missing")
    else:
        assert want.all()                                            # nothing is pruned at r2 = 1
    got = _prune(packed, g.shape[1], chrom, pos, wbp, wv, step, r2)
    assert got.dtype == bool and got.shape == (M,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} rows differ, first at {int(np.nonzero(got != want)[0][0])}"


@pytest.mark.parametrize("params,budget", [((50000, None, 10, 0.2), 4096), ((None, 200, 1, 0.5), 16384), ((None, 50, 5, 0.2), 1024)])
def test_prune_over_several_budget_ranges(panels, params, budget):
    """A band of several 32-row tiles, cut into many SNP ranges by a small mask budget (the function's own argument); a device
    tensor payload."""
    g, pos, packed = panels["missing"]
    chrom = np.zeros(M, dtype=np.int32)
    wbp, wv, step, r2 = params
    want, _ = _ref(panels, "missing", params)
    t = {}
    got = _prune(torch.from_numpy(packed).cuda(), g.shape[1], chrom, pos, wbp, wv, step, r2, mask_budget_bytes=budget, timings=t)
    assert t["ranges"] >= 8, t
    assert np.array_equal(got, want)
    with pytest.raises(RuntimeError, match="longest window"):
        _prune(packed, g.shape[1], chrom, pos, wbp, wv, step, r2, mask_budget_bytes=64)


def test_prune_edges(panels):
    """m not a multiple of the 32-row tile, a chromosome boundary inside a tile, interleaved chromosome codes, a row with every
    call missing, a monomorphic row, and ties in MAF (identical neighbours)."""
    g, pos, _ = panels["missing"]
    m = 1003
    g, pos = g[:m].copy(), pos[:m].copy()
    g[100] = -9                                                      # every call missing
    g[101] = -9
    g[101, :2] = [1, 2]                                              # two calls: pairs with N <= 1 or no variance
    g[200] = 0                                                       # monomorphic, complete
    g[201] = np.where(g[201] >= 0, 2, -9)                            # monomorphic with missing calls
    g[300] = g[299]                                                  # identical rows: r2 = 1, equal MAF
    chrom = np.zeros(m, dtype=np.int32)
    chrom[500:] = 1                                                  # 500 = 15 * 32 + 20
    packed = bed.pack_dosage(g)
    n = g.shape[1]
    for wbp, wv, step, r2 in ((None, 50, 5, 0.2), (30000, None, 3, 0.3), (None, 40, 7, 1.0)):
        want, _ = ref_prune_panel(g, chrom, pos, wbp, wv, step, r2)
        assert np.array_equal(_prune(packed, n, chrom, pos, wbp, wv, step, r2), want), (wbp, wv, step, r2)
    inter = (np.arange(m) % 2).astype(np.int32)
    for wbp, wv in ((None, 30), (40000, None)):
        want, _ = ref_prune_panel(g, inter, pos, wbp, wv, 3, 0.2)
        assert np.array_equal(_prune(packed, n, inter, pos, wbp, wv, 3, 0.2, mask_budget_bytes=2048), want)
    # both window kinds given: the base-pair window wins
    want, _ = ref_prune_panel(g, chrom, pos, 30000, None, 3, 0.3)
    assert np.array_equal(_prune(packed, n, chrom, pos, 30000, 5, 3, 0.3), want)


def test_six_sums_are_exact(panels):
    g, _, packed = panels["missing"]
    g = g[:900].copy()
    g[50] = -9
    n = g.shape[1]
    panel = jx._panel(bed.pack_dosage(g), n)
    for i0, i1, j0, j1 in ((37, 337, 101, 401), (0, 300, 0, 300), (600, 900, 0, 33), (899, 900, 0, 900)):
        got = jx._ld_sums(panel, i0, i1, j0, j1)
        want = ref_six_sums(g, np.arange(i0, i1), np.arange(j0, j1))
        assert got.dtype == np.int32 and got.shape == want.shape
        for p, name in enumerate(("D", "N", "S_i", "S_j", "Q_i", "Q_j")):
            assert np.array_equal(got[p], want[p]), (name, i0, i1, j0, j1)


def test_ld_block_matrix(panels, tmp_path):
    g, pos, _ = panels["missing"]
    g, pos = g[1000:1301].copy(), pos[1000:1301]
    g[7] = -9                                                        # every call missing: r2 = 0 off the diagonal
    g[8] = 1                                                         # monomorphic
    n = g.shape[1]
    want = ref_ld_matrix(g)
    got = jx.ld_r2_matrix_packed(bed.pack_dosage(g), n)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"ld_r2_matrix_packed: max abs error {err:.3e} (bar 2e-7)")
    assert err <= 2e-7
    assert (got[7, :7] == 0).all() and (got[8, 9:] == 0).all() and (np.diag(got) == 1).all()
    assert jx.ld_r2_matrix_packed(np.zeros((0, (n + 3) // 4), np.uint8), n).shape == (0, 0)
    assert jx.ld_r2_matrix_packed(bed.pack_dosage(g[:1]), n).tolist() == [[1.0]]
    # through a PLINK prefix: two chromosomes, a range of the second and a site set
    m = g.shape[0]
    chroms = ["chr1"] * 100 + ["2"] * (m - 100)
    prefix = str(tmp_path / "blk")
    bed.write_bed(prefix, bed.pack_dosage(g), [f"s{i}" for i in range(n)],
                  bed.Bim(chroms, [f"rs{i}" for i in range(m)], pos.tolist(), ["A"] * m, ["G"] * m))
    lo, hi = int(pos[120]), int(pos[260])
    r2, ch, ps = jx.bed_ldblock_r2_rust(prefix, ["chr2"], [hi], [lo])
    assert ch == ["2"] * 141 and ps == pos[120:261].tolist()
    assert float(np.max(np.abs(r2.astype(np.float64) - ref_ld_matrix(g[120:261])))) <= 2e-7
    sel = [3, 50, 99, 130, 131, 300]
    r2, ch, ps = jx.bed_ldblock_r2_rust(prefix, ["1", "2"], [0, 0], [int(pos[-1])] * 2, selected_chrom=["1"] * 3 + ["chr2"] * 3,
                                        selected_pos=pos[sel].tolist())
    assert ps == pos[sel].tolist() and ch == ["1"] * 3 + ["2"] * 3
    assert float(np.max(np.abs(r2.astype(np.float64) - ref_ld_matrix(g[sel])))) <= 2e-7


def test_cli_gformat_prune(panels, tmp_path, capsys):
    g, pos, _ = panels["missing"]
    m = 1200
    g, pos = g[:m], pos[:m]
    n = g.shape[1]
    chroms = ["1"] * 500 + ["chrX"] * 300 + ["1"] * 400              # the first chromosome comes back
    prefix = str(tmp_path / "in")
    bed.write_bed(prefix, bed.pack_dosage(g), [f"id{i}" for i in range(n)],
                  bed.Bim(chroms, [f"rs{i}" for i in range(m)], pos.tolist(), ["A"] * m, ["C"] * m))
    codes = np.array([0] * 500 + [1] * 300 + [0] * 400, dtype=np.int32)
    want, _ = ref_prune_panel(g, codes, pos, None, 50, 5, 0.2)
    assert 0.05 * m <= want.sum() <= 0.5 * m
    out = str(tmp_path / "res" / "pruned")
    assert cli.main(["gformat", "-bfile", prefix, "-prune", "50", "5", "0.2", "-o", out]) == 0
    assert f"kept {int(want.sum())} / {m} variants" in capsys.readouterr().out
    raw = open(prefix + ".bed", "rb").read()
    bps = (n + 3) // 4
    rows = np.frombuffer(raw, dtype=np.uint8, offset=3).reshape(m, bps)
    assert open(out + ".bed", "rb").read() == raw[:3] + rows[want].tobytes()
    lines = open(prefix + ".bim").read().splitlines(keepends=True)
    assert open(out + ".bim").read() == "".join(ln for ln, k in zip(lines, want) if k)
    assert open(out + ".fam").read() == open(prefix + ".fam").read()
    # a physical window, into a directory with -prefix
    want, _ = ref_prune_panel(g, codes, pos, 20000, None, 2, 0.4)
    outdir = str(tmp_path / "dir") + os.sep
    assert cli.main(["gformat", "-bfile", prefix + ".bed", "-prune", "20kb", "2", "0.4", "-o", outdir, "-prefix", "p2"]) == 0
    assert open(os.path.join(outdir, "p2.bed"), "rb").read() == raw[:3] + rows[want].tobytes()
