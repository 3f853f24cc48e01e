"""Host half of KING (`jx grm -king`): the greedy prune (`jx_king_prune`) against a Python restatement, the refusals of the public
functions (raised before any device call: this file runs without a GPU), the `-king` argument handling and the table writers.

The numpy restatement of the definitions (indicator matrices and integer matrix products, include/jxgpu.h "KING") lives here and
is shared with tests/test_gpu_king.py."""
import heapq

import numpy as np
import pytest

from janusx_amd import bed
from janusx_amd import cli
from janusx_amd import janusx as jx
from janusx_amd._lib import lib, SIGNATURES


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def king_panel(n_fam, m, miss=0.0, seed=7, all_missing=5):
    """(m, n = 4 n_fam + 1) int8 dosages, -9 = missing: families of two founders and two children from per-site allele
    frequencies U(0.1, 0.9), sample n - 1 a duplicate of sample 0 (made before the missing calls are drawn), and sample
    `all_missing` with every call missing (its pairs have no kinship)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, m)

    def hap():
        return (rng.random(m) < p).astype(np.int8)

    people = []
    for _ in range(n_fam):
        a, b = (hap(), hap()), (hap(), hap())

        def child():
            return (np.where(rng.random(m) < 0.5, a[0], a[1]), np.where(rng.random(m) < 0.5, b[0], b[1]))
        people += [a, b, child(), child()]
    people.append(people[0])
    g = np.stack([h[0] + h[1] for h in people], 1).astype(np.int8)
    g[rng.random(g.shape) < miss] = -9
    if all_missing is not None and all_missing < g.shape[1]:
        g[:, all_missing] = -9
    return g


def ref_counts(g):
    """(6, n, n) int64 in the field order of the pair counts: shared, ibs0, same_hom, both_het, het_i_obs, het_j_obs."""
    z, h, a = ((g == v).astype(np.float64) for v in (0, 1, 2))   # f64 products of 0 / 1 and sums below 2^53: exact integers
    nn = z + h + a
    return np.stack([nn.T @ nn, z.T @ a + a.T @ z, z.T @ z + a.T @ a, h.T @ h, h.T @ nn, nn.T @ h]).astype(np.int64)


def ref_kinship(c):
    """(both_het - 2 ibs0) / (het_i_obs + het_j_obs) in f64 in that order, NaN where the denominator is 0."""
    den = (c[4] + c[5]).astype(np.float64)
    num = c[3].astype(np.float64) - 2.0 * c[1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def ref_pairs(c, threshold):
    """(i, j, ibs0, kinship) of the pairs i < j with a finite kinship >= threshold, ordered by (i, j)."""
    n = c.shape[1]
    iu, ju = np.triu_indices(n, 1)
    kin = ref_kinship(c)[iu, ju]
    keep = np.isfinite(kin) & (kin >= threshold)
    return iu[keep].astype(np.uint32), ju[keep].astype(np.uint32), c[1][iu, ju][keep].astype(np.uint32), kin[keep]


def ref_graph(n, pi, pj):
    nbrs = [[] for _ in range(n)]
    for a, b in zip(pi.tolist(), pj.tolist()):
        nbrs[a].append(b)
        nbrs[b].append(a)
    return [sorted(v) for v in nbrs]


def ref_prune(nbrs):
    """Max-heap of (degree, id) with lazy deletion: heapq on (-degree, -id), so that ties go to the larger id."""
    n = len(nbrs)
    live = [len(v) for v in nbrs]
    active = [True] * n
    heap = [(-live[i], -i) for i in range(n)]
    heapq.heapify(heap)
    removed = []
    while heap:
        d, i = heapq.heappop(heap)
        d, i = -d, -i
        if not active[i] or d != live[i]:
            continue
        if d <= 0:
            break
        active[i] = False
        live[i] = 0
        removed.append(i)
        for nb in nbrs[i]:
            if active[nb]:
                live[nb] -= 1
                heapq.heappush(heap, (-live[nb], -nb))
    return [i for i in range(n) if active[i]], removed


def ref_site_keep(g, maf_thr, miss_thr):
    """The site filter of `prepare_bed_2bit_packed` with het threshold 0: f32 missing rate <= miss_thr and f32 minor allele
    frequency >= maf_thr (a site without calls passes only maf_thr <= 0)."""
    f32 = np.float32
    n = g.shape[1]
    called = (g >= 0).sum(1)
    alt = np.where(g >= 0, g, 0).astype(np.int64).sum(1)
    miss = (n - called).astype(np.float32) / f32(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        af = np.where(called > 0, alt.astype(np.float32) / (f32(2.0) * called.astype(np.float32)), f32(0.0)).astype(np.float32)
    keep = np.where(called > 0, np.minimum(af, f32(1.0) - af) >= f32(maf_thr), f32(maf_thr) <= f32(0.0))
    return keep & ~(miss > f32(miss_thr))


def render_king(ids, n_sites, pairs, kept, removed):
    """The three files of `jx grm -king` as text."""
    pi, pj, b0, kin = pairs
    kin0 = "ID1\tID2\tNSNP\tIBS0\tKINSHIP\n" + "".join(f"{ids[a]}\t{ids[b]}\t{n_sites}\t{z}\t{float(k)!r}\n"
                                                       for a, b, z, k in zip(pi.tolist(), pj.tolist(), b0.tolist(), kin.tolist()))
    return kin0, "".join(f"{ids[s]}\n" for s in kept), "".join(f"{ids[s]}\n" for s in removed)


def csr(nbrs):
    offsets = np.zeros(len(nbrs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(v) for v in nbrs])
    flat = np.asarray([x for v in nbrs for x in v], dtype=np.uint32)
    return offsets, flat


# ---- prune -------------------------------------------------------------------------------------------------------------------------

def _random_graph(rng, kind):
    n = int(rng.integers(1, 40))
    edges = set()
    if kind == "empty":
        pass
    elif kind == "clique":
        k = int(rng.integers(2, n + 1)) if n >= 2 else 0
        members = rng.permutation(n)[:k].tolist()
        edges = {(min(a, b), max(a, b)) for a in members for b in members if a != b}
    elif kind == "star":
        hub = int(rng.integers(0, n))
        edges = {(min(hub, b), max(hub, b)) for b in range(n) if b != hub and rng.random() < 0.7}
    elif kind == "ties":                                      # disjoint edges and paths: many equal degrees
        order = rng.permutation(n).tolist()
        step = int(rng.integers(2, 4))
        for s in range(0, n - 1, step):
            for a, b in zip(order[s:s + step - 1], order[s + 1:s + step]):
                edges.add((min(a, b), max(a, b)))
    else:
        dens = float(rng.choice([0.02, 0.1, 0.3, 0.8]))
        edges = {(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < dens}
    nbrs = [[] for _ in range(n)]
    for a, b in edges:
        nbrs[a].append(b)
        nbrs[b].append(a)
    return [sorted(v) for v in nbrs]


def test_prune_matches_the_restatement_on_random_graphs():
    rng = np.random.default_rng(11)
    seen_removed = 0
    for trial in range(400):
        nbrs = _random_graph(rng, ("empty", "clique", "star", "ties", "random", "random", "random", "random")[trial % 8])
        kept_want, removed_want = ref_prune(nbrs)
        kept, removed = jx.king_prune_related_graph(*csr(nbrs))
        assert kept.dtype == np.uint32 and removed.dtype == np.uint32
        assert kept.tolist() == kept_want and removed.tolist() == removed_want, (trial, nbrs)
        # the kept set is independent, and every removed sample had a kept or removed neighbour
        ks = set(kept_want)
        assert all(b not in ks for a in kept_want for b in nbrs[a])
        seen_removed += len(removed_want)
    assert seen_removed > 1000


def test_prune_hand_case_and_trivial_graphs():
    kept, removed = jx.king_prune_related_graph(*csr([[1, 2], [0], [0, 3], [2]]))
    assert kept.tolist() == [0, 3] and removed.tolist() == [2, 1]
    kept, removed = jx.king_prune_related_graph(*csr([[], [], []]))
    assert kept.tolist() == [0, 1, 2] and removed.tolist() == []
    kept, removed = jx.king_prune_related_graph(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32))
    assert kept.tolist() == [] and removed.tolist() == []
    # a triangle: equal degrees, the larger id goes first
    kept, removed = jx.king_prune_related_graph(*csr([[1, 2], [0, 2], [0, 1]]))
    assert kept.tolist() == [0] and removed.tolist() == [2, 1]


def test_prune_refuses_a_neighbour_out_of_range():
    offsets, flat = csr([[1], [0, 4], [], []])
    with pytest.raises(RuntimeError, match=r"KING neighbor index out of range: neighbors\[1\] contains 4 >= 4"):
        jx.king_prune_related_graph(offsets, flat)
    with pytest.raises(RuntimeError, match="offsets do not match"):
        jx.king_prune_related_graph(np.array([0, 1, 3], dtype=np.int64), np.array([1, 0], dtype=np.uint32))
    with pytest.raises(RuntimeError, match="offsets must not decrease"):
        jx.king_prune_related_graph(np.array([0, 2, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.uint32))


def test_abi_lists_the_king_entries():
    for name in ("jxg_king_related_p32", "jxg_king_counts_p32", "jx_king_prune"):
        assert name in SIGNATURES and hasattr(lib(), name)


# ---- refusals, before any device call --------------------------------------------------------------------------------------------------

def _all_entry_points(packed, n, threshold=0.05):
    return [lambda: jx.king_pair_counts_packed(packed, n, 0, 1, 0, 1), lambda: jx.king_pair_stats(packed, n, 0, 1),
            lambda: jx.king_related_pairs_packed(packed, n, threshold), lambda: jx.king_related_graph_packed(packed, n, threshold),
            lambda: jx.king_unrelated_set_packed(packed, n, threshold)]


def test_refusals_come_before_the_device(monkeypatch):
    g = (np.arange(40 * 9).reshape(40, 9) % 3).astype(np.int8)
    m, n = g.shape
    packed = bed.pack_dosage(g)
    for call in _all_entry_points(packed, 0):
        with pytest.raises(RuntimeError, match="KING requires n_samples > 0"):
            call()
    for call in _all_entry_points(packed[:0], n):
        with pytest.raises(RuntimeError, match="KING requires non-empty packed genotype data"):
            call()
    for call in _all_entry_points(packed, 13):                # 3 bytes per SNP in the payload, 4 expected
        with pytest.raises(RuntimeError, match=f"KING packed payload length mismatch: packed_bytes={m * 3} not divisible by bytes_per_snp=4"):
            call()
    for call in _all_entry_points(packed.ravel()[:-1], n):    # a flat payload as the reference takes it
        with pytest.raises(RuntimeError, match=f"KING packed payload length mismatch: packed_bytes={m * 3 - 1} not divisible"):
            call()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for call in _all_entry_points(packed, n, bad)[2:]:
            with pytest.raises(RuntimeError, match="KING kinship_threshold must be finite"):
                call()
    with pytest.raises(RuntimeError, match="KING sample_i out of range: 9 >= 9"):
        jx.king_pair_stats(packed, n, 9, 0)
    with pytest.raises(RuntimeError, match="KING sample_j out of range: 12 >= 9"):
        jx.king_pair_stats(packed, n, 0, 12)
    with pytest.raises(RuntimeError, match="KING sample_i out of range: -1 >= 9"):
        jx.king_pair_stats(packed, n, -1, 0)
    with pytest.raises(RuntimeError, match="KING sample_j out of range: 9 >= 9"):
        jx.king_pair_counts_packed(packed, n, 0, 2, 3, 10)
    with pytest.raises(RuntimeError, match="KING sample_i range"):
        jx.king_pair_counts_packed(packed, n, 3, 2, 0, 1)
    with pytest.raises(RuntimeError, match="KING max_rows must be >= 1"):
        jx.king_related_pairs_packed(packed, n, 0.05, max_rows=0)
    # the pair budget: 9 samples are 36 pairs
    monkeypatch.setenv("JANUSX_KING_MAX_EXACT_PAIRS", "35")
    for call in _all_entry_points(packed, n)[2:]:
        with pytest.raises(RuntimeError, match=r"KING exact all-pairs budget exceeded: pairs=36 > limit=35\. Set "
                                               r"JANUSX_KING_MAX_EXACT_PAIRS=0 to force, or raise the limit explicitly\."):
            call()
    monkeypatch.delenv("JANUSX_KING_MAX_EXACT_PAIRS")
    jx._king_enforce_exact_budget(126_491)                    # 7 999 923 295 pairs
    with pytest.raises(RuntimeError, match="pairs=8000049786 > limit=8000000000"):
        jx._king_enforce_exact_budget(126_492)
    monkeypatch.setenv("JANUSX_KING_MAX_EXACT_PAIRS", "0")
    jx._king_enforce_exact_budget(10_000_000)
    monkeypatch.setenv("JANUSX_KING_MAX_EXACT_PAIRS", "many")   # unparsable: the default
    with pytest.raises(RuntimeError, match="limit=8000000000"):
        jx._king_enforce_exact_budget(126_492)


def test_bed_route_refusals(tmp_path):
    with pytest.raises(RuntimeError, match="KING kinship_threshold must be finite"):
        jx.king_unrelated_set_from_bed(str(tmp_path / "absent"), kinship_threshold=float("nan"))
    with pytest.raises(ValueError, match="maf_threshold must be within"):
        jx.king_unrelated_set_from_bed(str(tmp_path / "absent"), maf_threshold=0.7)


def test_pair_stats_from_counts():
    # two samples over four sites: (0, 2), (1, 1), (2, 0), (0, 1)
    g = np.array([[0, 2], [1, 1], [2, 0], [0, 1]], dtype=np.int8)
    c = ref_counts(g)
    st = jx._king_stats_from_counts(c[:, 0, 1])
    assert st == {"shared_nonmissing": 4, "ibs0": 2, "ibs1": 1, "ibs2": 1, "het_i_obs": 1, "het_j_obs": 2, "both_het": 1, "kinship": -1.0}
    assert np.isnan(jx._king_stats_from_counts([3, 1, 2, 0, 0, 0])["kinship"])
    assert ref_kinship(c)[0, 1] == -1.0


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def test_king_flag_parsing_and_refused_combinations(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "_cmd_grm_king", lambda args: seen.append(args) or 0)
    assert cli.main(["grm", "-bfile", "p", "-king"]) == 0
    assert cli.main(["grm", "-bfile", "p", "-king", "0.177", "-maf", "0.1", "-snps-only"]) == 0
    assert cli.main(["grm", "-bfile", "p", "--king", "-0.5"]) == 0
    assert [a.king for a in seen] == [0.05, 0.177, -0.5]
    assert (seen[0].maf, seen[0].geno, seen[0].snps_only) == (0.02, 0.05, False)      # the command's own filter defaults
    assert (seen[1].maf, seen[1].snps_only) == (0.1, True)
    monkeypatch.undo()
    for extra, flag in ((["-sparse"], "-sparse"), (["-sparse", "0.1"], "-sparse"), (["-txt"], "-txt"), (["-grm", "k.npy"], "-grm")):
        with pytest.raises(SystemExit, match=f"-king cannot be combined with {flag}"):
            cli.main(["grm", "-bfile", "p", "-king"] + extra)
    with pytest.raises(SystemExit, match="KING kinship_threshold must be finite"):
        cli.main(["grm", "-bfile", "p", "-king", "nan"])
    with pytest.raises(SystemExit, match="-bfile"):
        cli.main(["grm", "-king"])


# ---- the writers -----------------------------------------------------------------------------------------------------------------------

def test_king_tables_on_a_fixed_table(tmp_path):
    ids = ["a", "b", "c", "d", "e"]
    kin = np.array([0.25, 1.0 / 3.0, 0.05, 0.1 + 0.2], dtype=np.float64)
    pairs = (np.array([0, 0, 1, 3], dtype=np.uint32), np.array([1, 4, 2, 4], dtype=np.uint32), np.array([0, 7, 12, 3], dtype=np.uint32), kin)
    kept, removed = np.array([1, 3], dtype=np.uint32), np.array([4, 0, 2], dtype=np.uint32)
    out = str(tmp_path / "t")
    paths = jx.write_king_tables(out, ids, 333, pairs, kept, removed)
    assert paths == [out + ".king.kin0", out + ".king.unrelated.id", out + ".king.related.id"]
    text = open(paths[0]).read()
    assert text == ("ID1\tID2\tNSNP\tIBS0\tKINSHIP\n" "a\tb\t333\t0\t0.25\n" "a\te\t333\t7\t0.3333333333333333\n" "b\tc\t333\t12\t0.05\n"
                    "d\te\t333\t3\t0.30000000000000004\n")
    assert open(paths[1]).read() == "b\nd\n" and open(paths[2]).read() == "e\na\nc\n"
    # the kinship column reads back to the same bits
    back = np.array([float(ln.split("\t")[4]) for ln in text.splitlines()[1:]])
    assert back.tobytes() == kin.tobytes()
    assert (text, open(paths[1]).read(), open(paths[2]).read()) == render_king(ids, 333, pairs, kept.tolist(), removed.tolist())


def test_restatement_cases_are_not_vacuous():
    """The thresholds test of tests/test_gpu_king.py relies on these properties of its panel (n = 81, m = 333, complete calls)."""
    g = king_panel(20, 333, 0.0)
    assert g.shape == (333, 81)
    c = ref_counts(g)
    iu, ju = np.triu_indices(81, 1)
    kin = ref_kinship(c)[iu, ju]
    assert int(np.isnan(kin).sum()) == 80                      # the pairs of the all-missing sample
    for thr in (0.05, 0.177, 0.25):
        assert int((kin >= thr).sum()) >= 50 and int((kin < thr).sum()) >= 1000, thr
    assert int((kin == 0.25).sum()) >= 1                       # the threshold 0.25 is attained: >= against >
    dup = ref_kinship(c)[0, 80]
    assert dup == 0.5 and c[1][0, 80] == 0
