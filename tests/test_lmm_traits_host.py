"""Host side of the trait-level LMM route (`jx gwas -lmm -trait-level-lmm`): the text of the combined table, the argument rules
and the warm-start chains of a group.  No GPU."""
import numpy as np
import pytest


def test_combined_line_is_the_single_trait_line_plus_the_phenotype(tmp_path):
    """For (beta, se, p) with NaN / p = 1 rows, a zero and a negative se, p outside (0, 1] and tiny p: the line of the combined
    table is the line the single-trait `.lmm.tsv` writers (the native one and its Python statement) print, followed by the name."""
    from janusx_amd.tsv import (HEADER3, assoc_trait_stats, format_row, format_trait_rows, resolve_snp_name, trait_site_prefixes,
                                write_assoc_tsv)
    nan = float("nan")
    betas = [0.0, 1.23456, -0.000049, 12345.678, -3.5e-7, nan, 0.5]
    ses = [1.0, 0.33333, 2.5e-5, 1e-9, 0.0, -1.0, nan, float("inf")]
    ps = [1.0, 0.05, 1.23456e-5, 3e-300, 1e-320, 0.0, 1.5, nan, -0.1]
    grid = np.array([(b, s, p) for b in betas for s in ses for p in ps], dtype=np.float64)
    k = len(grid)
    rng = np.random.default_rng(2)
    chrom = [str(1 + i % 3) for i in range(k)]
    pos = [100 + 7 * i for i in range(k)]
    snp = [("." if i % 5 == 0 else ("" if i % 11 == 0 else f"rs{i}")) for i in range(k)]
    a0, a1 = ["A"] * k, ["G"] * k
    af = rng.uniform(0, 0.5, size=k).astype(np.float32)
    miss = (rng.integers(0, 50, size=k) / np.float32(977.0)).astype(np.float32)
    path = str(tmp_path / "single.lmm.tsv")
    assert write_assoc_tsv(path, chrom, pos, snp, a0, a1, af, miss, grid) == k
    lines = open(path).read().split("\n")
    assert lines[0] + "\n" == HEADER3 and lines[-1] == "" and len(lines) == k + 2
    single = lines[1:-1]
    assert single == [format_row(chrom[i], pos[i], snp[i], a0[i], a1[i], af[i], miss[i], *grid[i]).rstrip("\n") for i in range(k)]
    pf = trait_site_prefixes(chrom, pos, [resolve_snp_name(snp[i], chrom[i], pos[i]) for i in range(k)], a0, a1, af, miss, as_rate=True)
    comb = format_trait_rows(pf, assoc_trait_stats(grid), "height cm").split("\n")
    assert comb[-1] == "" and comb[:-1] == [ln + "\theight cm" for ln in single]
    # a selection of rows (-trait-pmax) prints the same lines
    st4 = assoc_trait_stats(grid)
    hit = np.nonzero(st4[:, 3] <= 0.01)[0]
    assert 0 < len(hit) < k
    assert format_trait_rows(pf, st4[hit], "t", hit).split("\n")[:-1] == [single[i] + "\tt" for i in hit]


@pytest.fixture()
def tiny(tmp_path):
    from janusx_amd import bed
    n, m = 12, 6
    g = np.random.default_rng(0).integers(0, 3, size=(m, n)).astype(np.int8)
    pre = str(tmp_path / "tiny")
    bed.write_bed(pre, bed.pack_dosage(g), [f"s{i}" for i in range(n)],
                  bed.Bim(["1"] * m, [f"rs{j}" for j in range(m)], list(range(1, m + 1)), ["A"] * m, ["G"] * m))
    ph = str(tmp_path / "ph.tsv")
    with open(ph, "w") as fh:
        fh.write("id\tt1\tt2\n")
        for i in range(n):
            fh.write(f"s{i}\t{i * 0.5}\t{i % 3}\n")
    return pre, ph


def test_argument_rules_stop_the_run_before_it_starts(tiny, monkeypatch):
    from janusx_amd import cli
    monkeypatch.setattr(cli, "_dist_setup", lambda: pytest.fail("the run started"))
    pre, ph = tiny
    base = ["gwas", "-bfile", pre, "-p", ph]
    with pytest.raises(SystemExit, match="LMM trait-level route requires -lmm"):
        cli.main(base + ["-lm", "-trait-level-lmm"])
    with pytest.raises(SystemExit, match="LMM trait-level route requires -lmm"):
        cli.main(base + ["-fvlmm", "-trait-level-lmm"])
    with pytest.raises(SystemExit, match="LMM trait-level route requires at least 2 traits."):
        cli.main(base + ["-lmm", "-trait-level-lmm", "-n", "t2"])
    # -lmm -trait-level without -lm keeps failing, and now names the switch of this route
    with pytest.raises(SystemExit, match=r"the LM trait-level route requires -lm \(.*-trait-level-lmm\)"):
        cli.main(base + ["-lmm", "-trait-level"])
    with pytest.raises(SystemExit, match="-trait-pmax belongs to -trait-level"):
        cli.main(base + ["-lmm", "-trait-pmax", "0.01"])
    with pytest.raises(SystemExit, match=r"-trait-pmax must be within \[0, 1\]"):
        cli.main(base + ["-lmm", "-trait-level-lmm", "-trait-pmax", "2"])


def test_trait_pmax_is_accepted_with_either_switch(tiny, monkeypatch):
    from janusx_amd import cli

    class Started(Exception):
        pass

    def started():
        raise Started()

    monkeypatch.setattr(cli, "_dist_setup", started)
    pre, ph = tiny
    for flags in (["-lmm", "-trait-level-lmm"], ["-lm", "-trait-level"], ["-lm", "-lmm", "-trait-level", "-trait-level-lmm"]):
        with pytest.raises(Started):
            cli.main(["gwas", "-bfile", pre, "-p", ph] + flags + ["-trait-pmax", "0.01"])


@pytest.mark.parametrize("m_kept,chunk,pieces", [(3000, 500, 1), (3000, 500, 4), (2950, 512, 1), (2950, 512, 2), (7, 10000, 1),
                                                  (10001, 10000, 1)])
def test_group_chains_are_the_packed_route_chains_of_the_kept_rows(m_kept, chunk, pieces):
    from janusx_amd import pipeline
    from janusx_amd import stats as st
    co = pipeline.traits_chain_offsets(m_kept, chunk, pieces)
    assert np.array_equal(co, st.warm_chain_offsets(st.warm_chain_blocks_packed(m_kept, chunk, 0), m_kept, pieces))
    assert co.dtype == np.int64 and co[0] == 0 and co[-1] == m_kept and np.all(np.diff(co) > 0)
    # blocks of `chunk` KEPT rows (not chunks of the file), each cut into `pieces` by halving
    starts = np.arange(0, m_kept, chunk)
    assert np.all(np.isin(starts, co))
    if pieces == 1:
        assert np.array_equal(co, np.append(starts, m_kept))
    else:
        assert len(co) - 1 == pieces * len(starts) and np.max(np.diff(co)) <= -(-chunk // pieces)
