"""`jx tree -nj` on the GPU against tests/tree_ref.py: the pair counts exactly, the merge log of the NJ loop bit for bit (ids equal;
d_ij, r_i, r_j the same f64 bits), the Newick text byte for byte for both branch-length formulas, and the command end to end.

Sizes of the count kernel (csrc/k_tree.hip) the shapes straddle: 64-sample tiles (n = 63 / 64 / 65), 128-sample P32 records
(127 / 128 / 129), 64-row k-steps (m = 63 / 64 / 65, 129 = two steps and one row) and the 32-deep MFMA inside a step (31 / 32 / 33).
The NJ loop has no size threshold; its row sums take 64 rows per round and 64 columns per workgroup (every m from n down to 3 occurs in a run as the tree shrinks,
63 / 64 / 65 and 127 / 128 / 129 included)
and its argmin rows 256 columns per pass (n = 300 goes beyond one pass)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tree_ref as R   # noqa: E402
from janusx_amd import bed, cli   # noqa: E402
from janusx_amd import janusx as jx   # noqa: E402
from janusx_amd import tree as T   # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- counts

def _count_panel(n, m, seed, same_every=5):
    """Codes with all four values, missing calls, and every `same_every`-th row an equal-letter site (A / AT)."""
    rng = np.random.default_rng(seed)
    g = rng.choice([0, 1, 2, -1], size=(m, n), p=[0.45, 0.15, 0.3, 0.1])
    if n * m >= 4:
        g.flat[:4] = [0, 1, 2, -1]
    same = (np.arange(m) % same_every == same_every - 1) if same_every else np.zeros(m, dtype=bool)
    a0 = ["A"] * m
    a1 = ["AT" if s else "G" for s in same]
    return bed.pack_dosage(g), same, a0, a1


def _ref_counts(packed, n, a0, a1):
    aln = R.bed_alignment(packed, n, a0, a1, np.zeros(len(a0), dtype=bool))
    return R.pair_counts(aln)


COUNT_SHAPES = [(n, m) for n in (2, 127, 128, 129, 300) for m in (1, 63, 64, 65, 200)] + [(63, 33), (64, 32), (65, 31), (65, 129)]


@pytest.mark.parametrize("n,m", COUNT_SHAPES)
def test_pair_counts_equal_the_integer_restatement(n, m):
    packed, same, a0, a1 = _count_panel(n, m, 1000 * n + m)
    valid, mism = jx.tree_pair_counts_packed(packed, n, same)
    rv, rm = _ref_counts(packed, n, a0, a1)
    assert valid.dtype == np.int32 and valid.shape == (n, n)
    assert np.array_equal(valid, rv) and np.array_equal(mism, rm)


def test_pair_counts_modes_and_king():
    n, m = 129, 200
    packed, _same, a0, _a1 = _count_panel(n, m, 77, same_every=0)
    valid, mism = jx.tree_pair_counts_packed(packed, n)
    rv, rm = _ref_counts(packed, n, a0, ["G"] * m)
    assert np.array_equal(valid, rv) and np.array_equal(mism, rm)
    king = jx.king_pair_counts_packed(packed, n, 0, n, 0, n)               # shared, ibs0, same_hom, ...
    assert np.array_equal(valid, king[1] + king[2]) and np.array_equal(mism, king[1])
    # every row an equal-letter site: one image, valid = called x called, no mismatch
    v1, m1 = jx.tree_pair_counts_packed(packed, n, np.ones(m, dtype=bool))
    r1v, r1m = _ref_counts(packed, n, a0, ["AT"] * m)
    assert np.array_equal(v1, r1v) and np.array_equal(v1, king[0]) and not m1.any() and not r1m.any()
    # a device payload gives the same counts
    import torch
    v2, m2 = jx.tree_pair_counts_packed(torch.from_numpy(packed).cuda(), n)
    assert np.array_equal(v2, valid) and np.array_equal(m2, mism)


# ---------------------------------------------------------------- NJ loop

def _sym(x):
    d = x + x.T
    np.fill_diagonal(d, 0.0)
    return d


def _jc_matrix(n, m, seed):
    rng = np.random.default_rng(seed)
    g = rng.choice([0, 2, 1, -1], size=(m, n), p=[0.55, 0.35, 0.05, 0.05])
    aln = R.bed_alignment(bed.pack_dosage(g), n, ["A"] * m, ["G"] * m, np.zeros(m, dtype=bool))
    return R.distance_matrix(*R.pair_counts(aln))


def _balanced(n):
    """Additive distances of a balanced binary tree with every branch 0.25 long: d = 0.5 x (height of the common ancestor)."""
    i = np.arange(n)
    x = i[:, None] ^ i[None, :]
    return 0.5 * np.ceil(np.log2(x + 1.0))


NJ_NAMES = ([f"random_n{n}" for n in (2, 3, 4, 5)] + [f"nonmetric_n{n}" for n in (63, 64, 65, 129)] +
            ["ties_jc_m8_n100", "balanced_dyadic_n64", "all_zero_n20", "jc_panel_n300"])
_NJ_CASES, _NJ_REF = {}, {}


def _nj_case(name):
    """The matrix of a case, built once (and only when a GPU test asks for it)."""
    if name not in _NJ_CASES:
        n = int(name.rsplit("_n", 1)[1])
        rng = np.random.default_rng(4200 + n)
        if name.startswith("random"):
            d = _sym(rng.random((n, n)))
        elif name.startswith("nonmetric"):
            d = _sym(rng.random((n, n)) ** 6 * 10.0)
        elif name.startswith("ties"):
            d = _jc_matrix(n, 8, 5)
        elif name.startswith("balanced"):
            d = _balanced(n)
        elif name.startswith("all_zero"):
            d = np.zeros((n, n))
        else:
            d = _jc_matrix(n, 400, 6)
        d.setflags(write=False)
        _NJ_CASES[name] = d
    return _NJ_CASES[name]


def _nj_ref(name, route):
    if (name, route) not in _NJ_REF:
        _NJ_REF[(name, route)] = R.nj(_nj_case(name), route)
    return _NJ_REF[(name, route)]


@pytest.mark.parametrize("route", ["alignment", "distance"])
@pytest.mark.parametrize("name", NJ_NAMES)
def test_nj_merge_log_and_newick(name, route):
    dist = _nj_case(name)
    n = dist.shape[0]
    ref_ij, ref_vals, ref_last, ref_joins = _nj_ref(name, route)
    log_ij, log_vals, last = jx.nj_merge_log(dist, route)
    assert np.array_equal(log_ij, ref_ij), name
    assert log_vals.tobytes() == ref_vals.tobytes(), name                  # d_ij, r_i, r_j: the same bits
    assert np.float64(last).tobytes() == np.float64(ref_last).tobytes()
    names = [f"t{i}" for i in range(n)]
    assert T.newick_from_merge_log(names, log_ij, log_vals, last, route) == R.render_newick(names, ref_joins)


def test_nj_cases_exercise_what_they_are_for():
    # the non-metric matrices drive new distances and branch lengths into the clamps
    for n in (63, 64, 65, 129):
        joins = _nj_ref(f"nonmetric_n{n}", "alignment")[3]
        assert sum(1 for _l, _r, a, b in joins if a == 0.0 or b == 0.0) >= 3
    # m = 8 sites give few distinct distances: many exact ties of q
    assert len(np.unique(_nj_case("ties_jc_m8_n100"))) <= 40
    # balanced dyadic tree: the sums are exact and at the first step all 32 cherries tie exactly: the first in (i, j) order is joined,
    # and so on down the first half of the leaves, then the cherries of the new nodes
    ij = _nj_ref("balanced_dyadic_n64", "alignment")[0]
    assert ij[:16].tolist() == [[2 * k, 2 * k + 1] for k in range(16)]
    assert ij[16:24].tolist() == [[64 + 2 * k, 65 + 2 * k] for k in range(8)]
    # all zero: every q ties at 0, the first pair in (i, j) order is joined every time
    ij = _nj_ref("all_zero_n20", "distance")[0]
    assert ij[0].tolist() == [0, 1] and ij[1].tolist() == [2, 3]


def test_distance_matrix_mirror_symmetrises_an_asymmetric_input():
    rng = np.random.default_rng(9)
    n = 40
    d = rng.random((n, n)) * 2.0 - 0.2                                     # asymmetric, some negative entries
    d[3, 7] = np.nan                                                      # one direction missing: the other is taken
    d[11, 2] = np.inf
    np.fill_diagonal(d, 0.3)                                              # a finite diagonal is ignored
    names = [f"s {i}" if i == 5 else f"s{i}" for i in range(n)]
    want = R.render_newick(names, R.nj(R.normalize_distance_matrix(d), "distance")[3])
    assert jx.nj_newick_from_distance_matrix(d, names) == want


def test_alignment_mirror():
    rng = np.random.default_rng(13)
    n, m = 70, 90
    first = rng.choice(list(b"ACGT"), size=m)
    second = np.array([rng.choice([b for b in b"ACGT" if b != f]) for f in first])
    pick = rng.random((n, m))
    aln = np.where(pick < 0.5, first[None, :], np.where(pick < 0.85, second[None, :], rng.choice(list(b"NRY-acgt"), size=(n, m))))
    aln = aln.astype(np.uint8)
    low = (aln >= 0x61)                                                   # lower-case letters must agree with the column's two bases
    up = np.where(low, aln - 32, aln)
    ok = (up == first[None, :]) | (up == second[None, :]) | ~np.isin(up, list(b"ACGT"))
    aln = np.where(ok, aln, ord("N")).astype(np.uint8)
    aln[:, 10] = ord("N")                                                 # a column without a known base
    aln[:, 11] = ord("C")                                                 # a constant column
    names = [f"a{i}" for i in range(n)]
    for min_overlap in (1, 60):
        want = R.render_newick(names, R.nj(R.distance_matrix(*R.pair_counts(aln), min_overlap), "alignment")[3])
        assert jx.nj_newick_from_alignment_u8(aln, names, min_overlap=min_overlap) == want


# ---------------------------------------------------------------- end to end

def _write_panel(tmp_path):
    rng = np.random.default_rng(2026)
    n, m = 150, 400
    p = rng.uniform(0.05, 0.95, m)
    g = np.where(rng.random((m, n)) < p[:, None], 2, 0)                    # inbred lines: homozygous calls
    g = np.where(rng.random((m, n)) < 0.004, 1, g)                         # a few hets
    g = np.where(rng.random((m, n)) < 0.01, -1, g)                         # missing calls
    g[0] = -1                                                              # all missing
    g[1, :20] = -1                                                         # missing rate 0.13 > 0.05
    g[2] = 0
    g[2, :2] = 2                                                           # MAF 2 / 150 < 0.02
    g[3, :30] = 1                                                          # het rate 0.2 > 0.02
    g[4] = np.where(np.arange(n) < 120, 2, 0)                              # alt frequency 0.8: flipped
    a0 = [str(rng.choice(list("ACGT"))) for _ in range(m)]
    a1 = [str(rng.choice([c for c in "ACGT" if c != a])) for a in a0]
    a0[4], a1[4] = "A", "*"                                                # a non-ACGT allele on a flipped row: letters C / A
    a0[5], a1[5] = "A", "AT"                                               # an indel pair with equal first bases
    a0[6], a1[6] = "<INS>", "g"
    ids = [f"line{i}" for i in range(n)]
    ids[3] = "line:3"
    prefix = str(tmp_path / "panel")
    bed.write_bed(prefix, bed.pack_dosage(g), ids, bed.Bim(["1"] * m, [f"rs{i}" for i in range(m)], list(range(1, m + 1)), a0, a1))
    return prefix, g, a0, a1, ids


def _reference_run(g, a0, a1, ids, snps_only=False):
    n = g.shape[1]
    counts = np.stack([(g < 0).sum(axis=1), (g == 1).sum(axis=1), (g == 2).sum(axis=1)], axis=1)
    kf = [R.row_keep_scalar(int(a), int(b), int(c), n, 0.02, 0.05, 0.02) for a, b, c in counts]
    keep = np.array([k for k, _ in kf])
    if snps_only:
        keep &= np.array([len(x) == 1 and len(y) == 1 and x in "ACGTacgt" and y in "ACGTacgt" for x, y in zip(a0, a1)])
    rows = np.nonzero(keep)[0]
    aln = R.bed_alignment(bed.pack_dosage(g[rows]), n, [a0[r] for r in rows], [a1[r] for r in rows], [kf[r][1] for r in rows])
    text = R.newick(R.distance_matrix(*R.pair_counts(aln)), ids, "alignment")
    return keep, aln, text


@pytest.fixture(scope="module")
def panel(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tree")
    prefix, g, a0, a1, ids = _write_panel(tmp)
    return {"tmp": tmp, "prefix": prefix, "g": g, "a0": a0, "a1": a1, "ids": ids, "ref": _reference_run(g, a0, a1, ids)}


def test_tree_from_bed_end_to_end(panel):
    keep, aln, text = panel["ref"]
    assert not keep[:4].any() and keep[4] and keep[5] and keep[6] and 300 <= keep.sum() < 400
    assert bytes(aln[:, 0]) == b"C" * 120 + b"A" * 30                      # row 4, the first kept row: letters C / A after the flip
    out = str(panel["tmp"] / "out" / "tree")
    os.makedirs(os.path.dirname(out))
    res = jx.tree_from_bed(panel["prefix"], out=out, write_phylip_file=True)
    assert res["n_sites"] == int(keep.sum()) and res["sample_ids"] == panel["ids"] and res["newick"] == text
    assert res["outputs"] == [f"{out}.nwk", f"{out}.fasta", f"{out}.phy"]
    with open(f"{out}.nwk", "rb") as fh:
        assert fh.read() == (text + "\n").encode()
    with open(f"{out}.fasta", "rb") as fh:
        assert fh.read() == R.fasta_text(panel["ids"], aln).encode()
    with open(f"{out}.phy", encoding="utf-8") as fh:
        lines = fh.read().split("\n")
    assert lines[0] == f"150 {int(keep.sum())}" and lines[1] == "line0    " + bytes(aln[0]).decode() and lines[4].startswith("line:3   " + chr(aln[3, 0]))
    assert "'line:3'" in text


def test_cli_tree_no_fasta(panel, capsys):
    keep, _aln, text = _reference_run(panel["g"], panel["a0"], panel["a1"], panel["ids"], snps_only=True)
    assert keep.sum() == panel["ref"][0].sum() - 3                         # the rows 4, 5 and 6 are no SNPs
    outdir = str(panel["tmp"] / "cli") + os.sep
    assert cli.main(["tree", "-bfile", panel["prefix"], "-nj", "exact", "-snps-only", "-o", outdir, "-prefix", "t", "--no-fasta"]) == 0
    with open(os.path.join(outdir, "t.nwk"), "rb") as fh:
        assert fh.read() == (text + "\n").encode()
    assert not os.path.exists(os.path.join(outdir, "t.fasta")) and not os.path.exists(os.path.join(outdir, "t.phy"))
    printed = capsys.readouterr().out
    assert f"sites={int(keep.sum())}" in printed and "not written" in printed


def test_refuses_a_matrix_that_does_not_fit(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 1 << 30))
    with pytest.raises(RuntimeError, match=r"needs 8\d+ bytes of HBM, 1048576 bytes are free"):
        jx.nj_merge_log(np.zeros((1000, 1000)), "distance")
