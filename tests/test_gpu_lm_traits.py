"""GPU tests of the multi-trait LM scan (`jx gwas -lm -trait-level`; csrc/k_lm_traits.hip, `pipeline.scan_rows_lm_traits`): the int8
plane product bit for bit on dyadic operands at its tiling edges, parity of the statistics with the f64 restatement of the
reference's shared-projection route (tests/lm_traits_ref.py), chunked = unchunked bits, the hits form, and the command line."""
import math
import os

import numpy as np
import pytest

from lm_traits_ref import decode_rows, lm_traits_restatement

pytestmark = pytest.mark.gpu

N_SRC, M_SRC = 320, 300


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    return torch


@pytest.fixture(scope="module")
def source():
    """320 samples x 300 SNPs with 3 % missing calls; row 0 has no call at all, row 1 is monomorphic, row 2 all heterozygous."""
    rng = np.random.default_rng(20)
    p = rng.uniform(0.05, 0.5, size=M_SRC)
    g = rng.binomial(2, p[:, None], size=(M_SRC, N_SRC)).astype(np.int8)
    g[rng.random(g.shape) < 0.03] = -9
    g[0] = -9
    g[1] = 0
    g[2] = 1
    flip = rng.random(M_SRC) < 0.4
    flip[:3] = [True, False, True]
    return g, flip


_PANELS = {}


def _panel(g, idx):
    """Panel over the samples `idx` of the source (cached per sample list) and the rows' allele frequencies over them."""
    torch = _torch()
    from janusx_amd import bed
    from janusx_amd.pipeline import Panel
    key = idx.tobytes()
    if key not in _PANELS:
        packed = torch.from_numpy(bed.pack_dosage(g)).cuda()
        panel = Panel(packed, N_SRC, sample_idx=idx)
        gs = g[:, idx]
        called = (gs >= 0).sum(1)
        af = (np.where(gs < 0, 0, gs).sum(1) / np.maximum(2 * called, 1)).astype(np.float32)
        _PANELS[key] = (panel, gs, af)
    return _PANELS[key]


# ---- exactness on dyadic operands ---------------------------------------------------------------------------------------------

def _dyadic_columns(n, ncols, seed):
    """Integer columns K (ncols, n), |K| <= 2^27, times a power of two per column.  The first entries of every column hold the
    largest and smallest digit of each of the four radix-128 planes (+-64 2^(7 j)), sums of them, and values whose leading digits
    round up so that the next plane goes negative (a carry between planes)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(1 << 27), (1 << 27) + 1, size=(ncols, n), dtype=np.int64)
    special = []
    for j in (21, 14, 7, 0):
        special += [64 << j, -(64 << j), 63 << j, -(63 << j)]
    special += [(1 << 27), -(1 << 27), (5 << 21) + (1 << 20) + 3, -((5 << 21) + (1 << 20) + 3), (1 << 20) + (1 << 13) + (1 << 6),
                (7 << 21) + (127 << 14) + (127 << 7) + 127, (1 << 21) - 1, -(1 << 14) + 1, 1, -1, 0]
    special = np.array(special, dtype=np.int64)
    k[:, :min(n, len(special))] = special[:n]
    k[0, :] = k[0, :] >> 9                                      # a column that does not reach the top digit
    if ncols > 2:
        k[2, :] = 0                                             # a zero column
    e = (np.arange(ncols) % 9) - 4
    return k, e


def _device_sums(panel, rows, mean, flip, cols):
    torch = _torch()
    from janusx_amd._lib import check, lib
    from janusx_amd.pipeline import _LmtOperand, _ptr, _stream
    op = _LmtOperand(cols, panel.n, panel.npad, panel.device)
    nrows = len(rows)
    out = torch.full((nrows, op.ncols + 3), -7.0, dtype=torch.float64, device=panel.device)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    mean_t = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float32)).cuda()
    flip_t = torch.from_numpy(np.asarray(flip).astype(np.uint8)).cuda()
    check(lib().jxg_lmt_sums_p32(_ptr(panel.p32), panel.m, panel.n, _ptr(rows_t), nrows, _ptr(mean_t), _ptr(flip_t), _ptr(op.planes),
                                 _ptr(op.scale), _ptr(op.colsum), op.ncols, _ptr(out), out.shape[1], _stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, op.ncols:] == -7.0)                      # nothing beyond the operand's columns is written
    return o[:, :op.ncols]


def _integer_sums(gs, rows, mean, flip, k, e):
    """The same sums in integer arithmetic: called part and missing part exact, then the epilogue's three f64 roundings."""
    gr = gs[rows].astype(np.int64)
    fl = np.asarray(flip, dtype=bool)[:, None]
    called = np.where(gr < 0, 0, np.where(fl, 2 - gr, gr))
    n_called = called @ k.T                                     # (rows, ncols) int64, exact
    n_miss = (gr < 0).astype(np.int64) @ k.T
    s = np.ldexp(1.0, e)[None, :]
    mean64 = np.asarray(mean, dtype=np.float32).astype(np.float64)[:, None]
    return n_called.astype(np.float64) * s + mean64 * (n_miss.astype(np.float64) * s)


def _check_exact(source, idx, rows, ncols, seed=1):
    g, flip = source
    panel, gs, af = _panel(g, idx)
    mean = np.clip(np.float32(2.0) * af[rows], np.float32(0.0), np.float32(2.0))
    k, e = _dyadic_columns(len(idx), ncols, seed)
    got = _device_sums(panel, rows, mean, flip[rows], k.astype(np.float64) * np.ldexp(1.0, e)[:, None])
    want = _integer_sums(gs, rows, mean, flip[rows], k, e)
    assert got.shape == want.shape
    bad = np.nonzero(got.view(np.int64) != want.view(np.int64))
    assert bad[0].size == 0, (len(idx), len(rows), ncols, bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("n", [127, 128, 129, 300])
def test_sums_are_exact_at_every_sample_count(source, n):
    _check_exact(source, np.arange(n), np.arange(257), 65)


@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 127, 128, 129, 257])
def test_sums_are_exact_at_every_row_count(source, nrows):
    _check_exact(source, np.arange(300), np.arange(nrows), 65)


@pytest.mark.parametrize("ncols", [1, 2, 15, 16, 17, 63, 64, 65, 130])
def test_sums_are_exact_at_every_column_count(source, ncols):
    _check_exact(source, np.arange(300), np.arange(257), ncols)


def test_sums_are_exact_on_a_strided_row_list_and_a_sample_subset(source):
    _check_exact(source, np.arange(300), np.arange(M_SRC - 1, -1, -3), 65)
    sub = np.sort(np.random.default_rng(4).permutation(N_SRC)[:211])
    _check_exact(source, sub, np.arange(2, 259), 65, seed=2)


def test_the_planes_carry_the_documented_digits():
    """`jxg_lmt_prepare`: the scale is the smallest power of two >= max |b|, the digits are the balanced radix-128 ones, pad
    samples and pad columns are zero and the k order inside a 16-sample group is byte 4 q + b = sample 4 b + q."""
    torch = _torch()
    from janusx_amd.pipeline import _LmtOperand
    n = 130
    k, e = _dyadic_columns(n, 3, 5)
    cols = k.astype(np.float64) * np.ldexp(1.0, e)[:, None]
    op = _LmtOperand(cols, n, 256, torch.device("cuda"))
    planes = op.planes.cpu().numpy().astype(np.int64)
    assert planes.shape == (4, 32, 256) and np.abs(planes).max() <= 64
    assert not planes[:, 3:].any()
    pos = np.arange(256)
    sample = (pos // 16) * 16 + 4 * (pos % 4) + (pos % 16) // 4      # sample held by byte `pos`
    value = ((planes[0] * 128 + planes[1]) * 128 + planes[2]) * 128 + planes[3]
    by_sample = np.zeros((32, 256), dtype=np.int64)
    by_sample[:, sample] = value
    assert not by_sample[:, n:].any()
    scale = op.scale.cpu().numpy()
    sexp = op.sexp.cpu().numpy()
    for c in range(3):
        mx = np.abs(cols[c]).max()
        assert scale[c] == np.ldexp(1.0, int(sexp[c]) - 27)
        assert (mx == 0 and sexp[c] == 0) or (np.ldexp(1.0, int(sexp[c]) - 1) < mx <= np.ldexp(1.0, int(sexp[c])))
        assert np.array_equal(by_sample[c, :n].astype(np.float64) * scale[c], cols[c])
    assert np.array_equal(op.colsum.cpu().numpy()[:3], by_sample[:3].sum(1))


# ---- parity with the restatement ------------------------------------------------------------------------------------------------

N_PAR, M_PAR, T_PAR = 300, 257, 65


def _design(q, rng):
    """(n, q) design with intercept; from 7 columns on one column repeats another and one is zero: rank = q - 2."""
    x = np.concatenate([np.ones((N_PAR, 1)), rng.normal(size=(N_PAR, q - 1)) + np.arange(q - 1) * 3.0], axis=1)
    if q >= 7:
        x[:, 4] = x[:, 2] * 2.0
        x[:, 5] = 0.0
    return x


def _traits(gs, rng):
    y = rng.normal(size=(T_PAR, N_PAR))
    for t in range(0, 12, 2):
        y[t] += 0.5 * np.where(gs[10 + t] < 0, 0, gs[10 + t])        # some signal
    y[5] = 0.0                                                       # a constant trait: every row void
    y[6] = 1.0e4 + rng.normal(size=N_PAR)                            # mean 10^4 standard deviations
    y[7] *= 1.0e-12
    y[8] *= 1.0e12
    return y


def _errors(got, want, n, df):
    """Maxima in the project's norms: beta / max(|beta|, se), se relative, p over max(1, t^2), -log10 p."""
    void = np.isnan(want[..., 0])
    assert np.array_equal(np.isnan(got[..., 0]), void) and np.array_equal(np.isnan(got[..., 1]), void)
    assert np.array_equal(np.isnan(got[..., 2]), void)
    assert np.all(got[..., 3][void] == 1.0) and np.all(want[..., 3][void] == 1.0)
    ok = ~void
    b, s, c, p = (got[..., k][ok] for k in range(4))
    wb, ws, _wc, wp = (want[..., k][ok] for k in range(4))
    t2 = (wb / ws) ** 2
    e_beta = np.max(np.abs(b - wb) / np.maximum(np.abs(wb), ws))
    e_se = np.max(np.abs(s - ws) / ws)
    e_p = max(np.max(np.abs(p - wp) / wp / np.maximum(1.0, t2)),
              np.max(np.abs(np.log10(p) - np.log10(wp)) / np.maximum(1.0, -np.log10(wp))))
    chi = n * np.log(1.0 + (b / s) ** 2 / df)
    chi_ok = np.all(np.abs(c - chi) <= 1e-9 * np.abs(chi) + 1e-12 * n)
    return e_beta, e_se, e_p, chi_ok, int(ok.sum())


@pytest.mark.parametrize("q", [1, 3, 7, 12])
def test_statistics_match_the_restatement(source, q):
    """n = 300, m = 257, T = 65: beta within 1e-5 of max(|beta|, SE), SE within 1e-5, p within 1e-5 in both norms, chisq against
    n ln(1 + t^2 / df) of the device's own beta and SE, the void pattern equal.  Rows: no call at all, monomorphic, all
    heterozygous, flipped, 3 % missing calls; traits: constant, mean 10^4 sd, scaled by 1e-12 and by 1e12."""
    from janusx_amd.pipeline import scan_rows_lm_traits
    g, flip = source
    idx = np.arange(N_PAR)
    panel, gs, af = _panel(g, idx)
    rows = np.arange(M_PAR)
    rng = np.random.default_rng(100 + q)
    x, y = _design(q, rng), _traits(gs, rng)
    got = scan_rows_lm_traits(panel, rows, af[rows], x, y, flip=flip[rows]).cpu().numpy()
    want, rank = lm_traits_restatement(decode_rows(gs[rows], af[rows], flip[rows]), x, y)
    assert rank == (q if q < 7 else q - 2)
    assert got.shape == want.shape == (T_PAR, M_PAR, 4)
    assert np.isnan(want[5, :, 0]).all() and np.isnan(want[:, :3, 0]).all()     # the constant trait; rows 0, 1 and 2
    assert not np.isnan(want[0, 3:, 0]).any()
    e_beta, e_se, e_p, chi_ok, count = _errors(got, want, N_PAR, N_PAR - rank - 1)
    print(f"lm-traits parity q={q} rank={rank} cells={count}: beta {e_beta:.3e} se {e_se:.3e} p {e_p:.3e}")
    assert chi_ok
    assert e_beta < 1e-5 and e_se < 1e-5 and e_p < 1e-5, (e_beta, e_se, e_p)


# ---- same bits ---------------------------------------------------------------------------------------------------------------

def test_blocks_batches_and_column_positions_give_the_same_bits(source):
    from janusx_amd.pipeline import scan_rows_lm_traits
    g, flip = source
    panel, gs, af = _panel(g, np.arange(N_PAR))
    rows = np.arange(M_PAR)
    rng = np.random.default_rng(9)
    x, y = _design(3, rng), _traits(gs, rng)
    run = lambda yy, **kw: scan_rows_lm_traits(panel, rows, af[rows], x, yy, flip=flip[rows], **kw).cpu().numpy().view(np.int64)  # noqa: E731
    base = run(y)
    assert np.array_equal(run(y), base)                                          # a second run
    assert np.array_equal(run(y, block_rows=32), base)                           # row blocks of 32 against 257
    assert np.array_equal(run(y, trait_batch=16), base)                          # trait batches of 16 against 65
    assert np.array_equal(run(y, block_rows=32, trait_batch=16), base)
    perm = np.random.default_rng(3).permutation(T_PAR)
    assert np.array_equal(run(y[perm], trait_batch=16), base[perm])              # traits at other column positions
    assert np.array_equal(run(y[40:41]), base[40:41])                            # a trait alone


# ---- hits ----------------------------------------------------------------------------------------------------------------------

def test_hits_are_the_dense_selection(source):
    from janusx_amd.pipeline import scan_rows_lm_traits
    g, flip = source
    panel, gs, af = _panel(g, np.arange(N_PAR))
    rows = np.arange(M_SRC)
    rng = np.random.default_rng(12)
    x, y = _design(3, rng), _traits(gs, rng)[:20]
    kw = dict(flip=flip[rows])
    dense = scan_rows_lm_traits(panel, rows, af[rows], x, y, **kw).cpu().numpy()
    for pmax, cap in ((0.05, None), (0.05, 64), (0.0, None), (1.0, 64)):
        h = scan_rows_lm_traits(panel, rows, af[rows], x, y, pmax=pmax, hit_capacity=cap, trait_batch=8, block_rows=128, **kw)
        tt, rr = np.nonzero(dense[:, :, 3] <= pmax)                              # (trait, row) order
        assert np.array_equal(h.trait, tt.astype(np.int32)) and np.array_equal(h.row, rr.astype(np.int32)), (pmax, cap)
        assert np.array_equal(h.stats.view(np.int64), dense[tt, rr].view(np.int64))
        if pmax == 0.0:
            assert len(h.trait) == 0
        if pmax == 1.0:
            assert len(h.trait) == 20 * M_SRC and np.isnan(h.stats[:, 0]).any()
        if pmax == 0.05:
            assert len(h.trait) > 64


# ---- command line and mirrors on a small PLINK prefix -------------------------------------------------------------------------

N_CLI, M_CLI = 240, 330


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    """240 samples x 330 SNPs (rare and badly called rows among them), a covariate table and three traits: t1 and t3 share their
    samples, t2 lacks 15 more."""
    from janusx_amd import bed
    d = tmp_path_factory.mktemp("lmtcli")
    rng = np.random.default_rng(31)
    p = rng.uniform(0.1, 0.5, size=M_CLI)
    p[::19] = 0.004
    g = rng.binomial(2, p[:, None], size=(M_CLI, N_CLI)).astype(np.int8)
    miss = np.full(M_CLI, 0.02)
    miss[5::23] = 0.2
    g[rng.random((M_CLI, N_CLI)) < miss[:, None]] = -9
    ids = [f"s{i}" for i in range(N_CLI)]
    bim = bed.Bim(["1"] * M_CLI, [f"rs{j}" for j in range(M_CLI)], [1000 + 10 * j for j in range(M_CLI)], ["A"] * M_CLI, ["G"] * M_CLI)
    pre = str(d / "panel")
    bed.write_bed(pre, bed.pack_dosage(g), ids, bim)
    cov = rng.normal(size=(N_CLI, 2)) + np.array([0.0, 5.0])
    y = rng.normal(size=(3, N_CLI)) + cov @ np.array([0.3, -0.2])
    for t, j in enumerate((1, 40, 41)):
        y[t] += 0.6 * np.where(g[j] < 0, 0, g[j])
    gone = rng.permutation(N_CLI)
    y[:, gone[:9]] = np.nan
    y[1, gone[9:24]] = np.nan
    with open(pre + ".pheno.tsv", "w") as fh:
        fh.write("id\tt1\tt2\tt3\n")
        for i in range(N_CLI):
            fh.write(ids[i] + "\t" + "\t".join("NA" if np.isnan(v) else repr(float(v)) for v in y[:, i]) + "\n")
    with open(pre + ".cov.tsv", "w") as fh:
        fh.write("id\tc0\tc1\n")
        for i in range(N_CLI):
            fh.write(ids[i] + "\t" + "\t".join(repr(float(v)) for v in cov[i]) + "\n")
    return pre, g, ids, bim, cov, y


def _read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:-1]]


def _last_digit_apart(a, b):
    """Two printed numbers that differ by one unit of their last printed digit at most."""
    if a == b:
        return True
    ma, mb = a.split("e")[0], b.split("e")[0]
    if len(a.split("e")) != len(b.split("e")) or (len(a.split("e")) == 2 and a.split("e")[1] != b.split("e")[1]):
        return abs(float(a) - float(b)) <= 1.0001e-4 * abs(float(b))
    return abs(float(ma) - float(mb)) <= 1.0001e-4


def test_cli_writes_the_combined_table(prefix, tmp_path, capsys):
    from janusx_amd import cli
    pre, g, ids, bim, cov, y = prefix
    base = ["gwas", "-bfile", pre, "-p", pre + ".pheno.tsv", "-c", pre + ".cov.tsv", "-lm"]
    plain, comb, cut = str(tmp_path / "plain"), str(tmp_path / "comb"), str(tmp_path / "cut")
    assert cli.main(base + ["-o", plain]) == 0
    assert cli.main(base + ["-trait-level", "-o", comb]) == 0
    said = capsys.readouterr().out
    assert "-lm -trait-level: 3 traits" in said and "traits=2" in said and "traits=1" in said
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("comb")) == ["comb.lm.tsv"]
    head, body = _read_tsv(comb + ".lm.tsv")
    assert head == ["chrom", "pos", "snp", "allele0", "allele1", "af", "miss", "beta", "se", "chisq", "pwald", "phenotype"]
    # groups in the order of their first trait, traits of a group in selection order: t1, t3 (same samples), then t2
    names = [b[11] for b in body]
    assert [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n] == ["t1", "t3", "t2"]
    for t, name in enumerate(("t1", "t2", "t3")):
        phead, pbody = _read_tsv(f"{plain}.{name}.lm.tsv")
        mine = [b for b in body if b[11] == name]
        assert len(mine) == len(pbody) and 0 < len(pbody) < M_CLI
        n = int(np.isfinite(y[t]).sum())
        df = n - 3 - 1
        moved = 0
        for a, b in zip(mine, pbody):
            assert a[:7] == b[:7]                                                 # site columns, af, miss count
            assert _last_digit_apart(a[7], b[7]) and _last_digit_apart(a[8], b[8]), (a, b)
            moved += a[7:9] != b[7:9]                                             # a flip of the last digit of beta or se
            # pwald prints five digits: it moves in many rows, by what 1e-5 on t allows (bounded in size, not in count)
            t2 = float(b[9]) if b[9] != "NaN" else 0.0
            assert abs(float(a[10]) - float(b[10])) <= (1.0001e-4 + 1e-5 * max(1.0, t2)) * float(b[10]), (a, b)
            if b[9] != "NaN":
                assert abs(float(a[9]) - n * math.log1p(float(b[9]) / df)) <= 2.5e-4 * float(a[9]) + 1e-12, (a, b)
            else:
                assert a[9] == "NaN" and a[10] == "1.0000e0"
        assert moved <= 0.03 * len(mine), (name, moved, len(mine))
    # -trait-pmax: the qualifying rows only, the same text
    assert cli.main(base + ["-trait-level", "-trait-pmax", "0.01", "-o", cut]) == 0
    _h, cbody = _read_tsv(cut + ".lm.tsv")
    # (the cut is made on the unrounded p: a printed 1.0000e-2 may sit on either side)
    assert [c for c in cbody if c[10] != "1.0000e-2"] == [b for b in body if float(b[10]) <= 0.01 and b[10] != "1.0000e-2"]
    assert all(c in body for c in cbody)
    assert 0 < len(cbody) < len(body) // 10 and {c[11] for c in cbody} == {"t1", "t2", "t3"}


def test_mirrors_on_a_sample_subset(prefix, tmp_path):
    """`lm_trait_assoc_bed_matrix_to_tsv` and `lm_trait_assoc_bed_to_tsv` with prepared rows (some flipped) over 150 samples in an
    order of their own: the reference's tuples, the same table from both, and the table of the in-memory scan's numbers."""
    from janusx_amd import bed
    from janusx_amd import janusx as jx
    from janusx_amd import tsv
    pre, g, ids, bim, cov, y = prefix
    full = np.nonzero(np.isfinite(y).all(0))[0]
    sel = full[::-1][:150].copy()
    gs = g[:, sel]
    called = (gs >= 0).sum(1)
    af = (np.where(gs < 0, 0, gs).sum(1) / np.maximum(2 * called, 1)).astype(np.float32)
    miss = (gs < 0).sum(1)
    rows = np.nonzero((miss <= 0.1 * len(sel)) & (np.minimum(af, 1 - af) >= 0.05))[0]
    flip = (rows % 3 == 0)
    maf = np.where(flip, np.float32(1.0) - af[rows], af[rows]).astype(np.float32)
    rate = (miss[rows] / np.float32(len(sel))).astype(np.float32)
    x = np.concatenate([np.ones((len(sel), 1)), cov[sel]], axis=1)
    yt = np.ascontiguousarray(y[:, sel])
    seen = []
    p1, p2 = str(tmp_path / "m1.tsv"), str(tmp_path / "m2.tsv")
    res = jx.lm_trait_assoc_bed_matrix_to_tsv(pre, ["t1", "t2", "t3"], yt, x, sel, rows, flip, rate, maf, p1,
                                              progress_callback=lambda d, t, name: seen.append((d, t, name)))
    assert [(r[0], r[1], r[2], r[3]) for r in res] == [(nm, 150, len(rows), len(rows)) for nm in ("t1", "t2", "t3")]
    assert all(isinstance(r[4], float) and r[4] >= 0.0 for r in res) and seen == [(1, 3, "t1"), (2, 3, "t2"), (3, 3, "t3")]
    specs = [dict(trait_name=nm, y=yt[t], x=x, sample_ids=[ids[i] for i in sel], row_indices=rows, row_flip=flip, row_missing=rate,
                  row_maf=maf, n_idv=150 + t) for t, nm in enumerate(("t1", "t2", "t3"))]
    specs[2]["x"] = x[:, :2].copy()                          # another design: this trait goes alone
    res2 = jx.lm_trait_assoc_bed_to_tsv(pre, specs, p2)
    assert [(r[0], r[1], r[2], r[3]) for r in res2] == [(nm, 150 + t, len(rows), len(rows)) for t, nm in enumerate(("t1", "t2", "t3"))]
    t1 = open(p1).read().split("\n")
    t2 = open(p2).read().split("\n")
    k = 1 + 2 * len(rows)
    assert t1[:k] == t2[:k] and len(t1) == len(t2) == 2 + 3 * len(rows)
    assert t1[k:] != t2[k:]                                  # t3 without the second covariate
    dense = jx.lm_trait_assoc_packed(bed.pack_dosage(g), N_CLI, yt, x, flip, maf, sample_indices=sel, row_indices=rows)
    assert dense.shape == (3, len(rows), 4)
    want, _rank = lm_traits_restatement(decode_rows(gs[rows], maf, flip), x, yt)
    e_beta, e_se, e_p, chi_ok, _count = _errors(dense, want, len(sel), len(sel) - 3 - 1)
    assert chi_ok and e_beta < 1e-5 and e_se < 1e-5 and e_p < 1e-5
    pre_txt = tsv.trait_site_prefixes(["1"] * len(rows), [bim.pos[j] for j in rows], [bim.snp[j] for j in rows], ["A"] * len(rows),
                                      ["G"] * len(rows), maf, rate)
    assert "".join(tsv.format_trait_rows(pre_txt, dense[t], nm) for t, nm in enumerate(("t1", "t2", "t3"))) == "\n".join(t1[1:])
    ht, hr, hv = jx.lm_trait_assoc_packed(bed.pack_dosage(g), N_CLI, yt, x, flip, maf, sample_indices=sel, row_indices=rows, pmax=0.01)
    tt, rr = np.nonzero(dense[:, :, 3] <= 0.01)
    assert np.array_equal(ht, tt) and np.array_equal(hr, rr) and np.array_equal(hv.view(np.int64), dense[tt, rr].view(np.int64))
