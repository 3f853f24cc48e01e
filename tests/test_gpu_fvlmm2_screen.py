"""`jx fvlmm2 -screen` on the device (csrc/k_pairscreen.hip, janusx.pair_class_tables_packed / fvlmm2_screen_packed, cli.cmd_fvlmm2)
against the restatement of tests/pairscreen_ref.py: the integer class tables bit for bit, the statistic against the rational
evaluation within `pairscreen_ref.STAT_TOL` (8 x the f64 restatement's own error, 1.84e-13 in the norm |dT| / max(T, 1)), the void
pattern, the hit list, the exclusions and the command.

Statistics that are equal in exact arithmetic: max(a, b) = a + b - min(a, b) and min(2 - a, 2 - b) = 2 - max(a, b), so given the
intercept and both literals the combos a&b, a|b, !a&!b and !a|!b differ by a member of the span and share one T; a class that a pair
does not show merges more.  Their f64 values differ in the last bits, so inside such a group the order of a sorted list follows the
rounding: the list is compared with the f64 restatement (the same operations in the same order), and with the rational one up to the
order inside groups of equal exact T."""
import math

import numpy as np
import pytest

import pairscreen_ref as P

pytestmark = pytest.mark.gpu


def _payload(n_src, m, seed, missing, special):
    from janusx_amd import bed
    packed, g = bed.synth_panel_numpy(n_src, m, seed=seed, missing_rate=missing, maf_low=0.1, maf_high=0.5)
    if special:
        g = g.copy()
        g[11] = -9                                             # an all-missing row
        g[29] = 1                                              # a monomorphic row
        packed = bed.pack_dosage(g)
    return packed


def _dyadic(rng, n):
    r = np.ldexp(rng.integers(-2 ** 27, 2 ** 27 + 1, size=n).astype(np.float64), -27)
    r[0] = 0.75                                                # S = 1 whatever the draw
    return r


@pytest.mark.parametrize("n", [65, 129, 200])
@pytest.mark.parametrize("kind", ["clean", "missing3", "special"])
def test_tables_bit_for_bit(n, kind):
    """N and R of 45 x 33 rows out of 80 equal direct counting, and the scale is equal: n at the 64-sample step edge, the
    128-sample record edge and a ragged tail; lists that are no multiple of 16 and cross the block edges 16 and 32; r random and
    dyadic; with and without a sample selection; host and device payload."""
    import torch
    import janusx_amd.janusx as jx
    rng = np.random.default_rng(1000 + n)
    m, n_src = 80, n + 37
    rows_i, rows_j = rng.choice(m, size=45, replace=False), rng.choice(m, size=33, replace=False)
    if kind == "special":
        rows_i[[0, 17]], rows_j[[5, 32]] = [11, 29], [29, 11]
    for dyadic, select, device in ((False, False, False), (True, False, True), (False, True, True), (True, True, False)):
        nn = n_src if select else n
        packed = _payload(nn, m, 77 + n, 0.03 if kind == "missing3" else 0.0, kind == "special")
        idx = rng.permutation(n_src)[:n] if select else None
        r = _dyadic(rng, n) if dyadic else rng.normal(size=n) * 3.7
        cls = P.decode_classes(packed, nn, idx)
        _digits, scale, units = P.digit_split(r)
        if dyadic:
            assert np.array_equal(units.astype(np.float64) * scale, r)
        exp_n, exp_r = P.class_tables(cls[rows_i], cls[rows_j], units)
        if kind == "missing3":
            assert (cls < 0).any()
        if kind == "special":
            assert exp_n[0].sum() == 0 and exp_n[17][:, [0, 2], :].sum() == 0 and exp_n[17].sum() > 0
        pk = torch.from_numpy(packed).cuda() if device else packed
        got_n, got_r, got_scale = jx.pair_class_tables_packed(pk, nn, rows_i, rows_j, r, sample_indices=idx)
        assert got_n.dtype == np.int32 and got_r.dtype == np.int64 and got_n.shape == got_r.shape == (45, 33, 3, 3)
        assert got_scale == scale, (dyadic, select, device)
        assert np.array_equal(got_n, exp_n), (dyadic, select, device)
        assert np.array_equal(got_r, exp_r), (dyadic, select, device)
        if idx is None and not device:                         # r as a device tensor gives the same planes
            again = jx.pair_class_tables_packed(pk, nn, rows_i[:3], rows_j[:2], torch.from_numpy(r).cuda())
            assert np.array_equal(again[0], exp_n[:3, :2]) and np.array_equal(again[1], exp_r[:3, :2]) and again[2] == scale


# ---- the statistic and the hits on one panel -------------------------------------------------------------------------------------

N_STAT, M_STAT = 129, 48
_CACHE = {}


def _panel():
    """n = 129, m = 48, 3 % missing, flipped rows, row 5 = row 4 (identical rows), row 7 monomorphic; the restatement's dense
    statistics (rational and f64), computed once."""
    if _CACHE:
        return _CACHE
    from janusx_amd import bed
    from janusx_amd import fvlmm2 as f2
    rng = np.random.default_rng(4242)
    _packed, g = bed.synth_panel_numpy(N_STAT, M_STAT, seed=4242, missing_rate=0.03, maf_low=0.1, maf_high=0.5)
    g = g.copy()
    g[5] = g[4]
    g[7] = np.where(g[7] < 0, -9, 0)
    packed = bed.pack_dosage(g)
    flip = rng.random(M_STAT) < 0.4
    flip[4], flip[5] = False, False
    r = rng.normal(size=N_STAT)
    variants = f2.screen_variants()
    var = f2.variant_array(variants)
    cls = P.decode_classes(packed, N_STAT)
    _d, scale, units = P.digit_split(r)
    sigma2 = float(r @ r) / (N_STAT - 1)
    exact, _h, screened = P.screen(cls, flip, units, scale, sigma2, var, 0.0, exact=True)
    f64, _h, _s = P.screen(cls, flip, units, scale, sigma2, var, 0.0, exact=False)
    assert screened == M_STAT * (M_STAT - 1) // 2
    assert all((exact[k] is None) == (f64[k] is None) for k in exact)      # no pair sits at a void threshold
    n_tab, _r_tab = P.class_tables(cls, cls, units)
    _CACHE.update(packed=packed, flip=flip, r=r, var=var, variants=variants, cls=cls, scale=scale, units=units, sigma2=sigma2,
                  exact=exact, f64=f64, n_complete=n_tab.sum(axis=(2, 3)))
    return _CACHE


def _ref_hits(c, dense, t_min, keep=lambda i, j: True):
    hits = [(i, j, v, t, int(c["n_complete"][i, j])) for (i, j, v), t in dense.items() if t is not None and t >= t_min and keep(i, j)]
    hits.sort(key=lambda h: (-h[3], h[0], h[1], h[2]))
    return hits


def _got_hits(res):
    return list(zip(res["row1"].tolist(), res["row2"].tolist(), res["variant"].tolist(), res["stat"].tolist(), res["n_complete"].tolist()))


def _same_up_to_exact_ties(got, ref_exact):
    """The same (row1, row2, variant, n_complete) entries, every stat within the tolerance, and an order that differs from the
    rational one only inside groups of statistics within the tolerance of one another."""
    assert sorted(h[:3] + h[4:] for h in got) == sorted(h[:3] + h[4:] for h in ref_exact)
    exact = {h[:3]: h[3] for h in ref_exact}
    for h in got:
        assert P.stat_error(h[3], exact[h[:3]]) <= P.STAT_TOL, h
    for a, b in zip(got, got[1:]):
        ta, tb = exact[a[:3]], exact[b[:3]]
        assert ta >= tb or P.stat_error(ta, tb) <= 2 * P.STAT_TOL, (a, b)
        assert (-a[3], a[0], a[1], a[2]) < (-b[3], b[0], b[1], b[2])        # sorted by its own keys


def _t_min(c, rank):
    """Between the rank-th and the next largest distinct exact statistic; no statistic within 1e-9 relative of it."""
    vals = sorted({t for t in c["exact"].values() if t is not None}, reverse=True)
    k = rank
    while vals[k] - vals[k + 1] < 1e-6 * vals[k]:
        k += 1
    t_min = 0.5 * (vals[k] + vals[k + 1])
    for dense in (c["exact"], c["f64"]):
        assert all(abs(t - t_min) > 1e-9 * t_min for t in dense.values() if t is not None)
    return t_min


def test_statistic_of_every_pair_and_variant():
    """t_min = 0 returns every statistic that is not void (T >= 0): the void pattern is the rational one's, every T lies within
    STAT_TOL of the rational value; identical rows (4, 5) and every pair with the monomorphic row 7 are void in every variant."""
    import janusx_amd.janusx as jx
    c = _panel()
    res = jx.fvlmm2_screen_packed(c["packed"], N_STAT, c["flip"], c["r"], c["sigma2"], c["variants"], 0.0)
    got = {h[:3]: h for h in _got_hits(res)}
    live = {k for k, t in c["exact"].items() if t is not None}
    assert res["pairs_screened"] == M_STAT * (M_STAT - 1) // 2 and res["hits_total"] == len(live) == len(got)
    assert set(got) == live
    nv = len(c["variants"])
    assert all((4, 5, v) not in got for v in range(nv))
    assert all((min(7, j), max(7, j), v) not in got for j in range(M_STAT) if j != 7 for v in range(nv))
    assert len(live) > 0.8 * nv * (M_STAT - 2) * (M_STAT - 3) // 2
    worst = max(P.stat_error(h[3], c["exact"][k]) for k, h in got.items())
    same = sum(h[3] == c["f64"][k] for k, h in got.items())
    print(f"screen statistic: {len(got)} values, largest error against the rational value {worst:.3e} (allowed {P.STAT_TOL:.3e}); "
          f"{same} equal the f64 restatement bit for bit")
    assert worst <= P.STAT_TOL
    assert all(h[4] == c["n_complete"][k[0], k[1]] for k, h in got.items())


def test_hit_list_counts_and_sort():
    import janusx_amd.janusx as jx
    c = _panel()
    t_min = _t_min(c, 60)
    res = jx.fvlmm2_screen_packed(c["packed"], N_STAT, c["flip"], c["r"], c["sigma2"], c["var"], t_min)
    ref_exact, ref_f64 = _ref_hits(c, c["exact"], t_min), _ref_hits(c, c["f64"], t_min)
    assert res["pairs_screened"] == M_STAT * (M_STAT - 1) // 2
    assert res["hits_total"] == len(ref_exact) == len(ref_f64) >= 60
    got = _got_hits(res)
    _same_up_to_exact_ties(got, ref_exact)
    assert [h[:3] + h[4:] for h in got] == [h[:3] + h[4:] for h in ref_f64]       # the same operations in the same order
    assert res["variant"].dtype == np.int32 and res["n_complete"].dtype == np.int32 and res["stat"].dtype == np.float64


def test_min_dist_rows_and_cap():
    import torch
    import janusx_amd.janusx as jx
    c = _panel()
    t_min = _t_min(c, 200)
    chrom = (np.arange(M_STAT) // 24).astype(np.int32)
    pos = 1000 * np.arange(M_STAT, dtype=np.int64)

    def far(i, j):
        return chrom[i] != chrom[j] or abs(int(pos[i]) - int(pos[j])) >= 3500
    res = jx.fvlmm2_screen_packed(torch.from_numpy(c["packed"]).cuda(), N_STAT, c["flip"], c["r"], c["sigma2"], c["var"], t_min,
                                  chrom_id=chrom, pos=pos, min_dist=3500)
    ref = _ref_hits(c, c["exact"], t_min, far)
    n_far = sum(far(i, j) for i in range(M_STAT) for j in range(i + 1, M_STAT))
    assert n_far == M_STAT * (M_STAT - 1) // 2 - 2 * (23 + 22 + 21)
    assert res["pairs_screened"] == n_far and res["hits_total"] == len(ref) < len(_ref_hits(c, c["exact"], t_min))
    _same_up_to_exact_ties(_got_hits(res), ref)
    # rows= restricts the pairs (given unsorted and twice: the pairs of the distinct rows, row1 < row2)
    rows = np.array([40, 3, 17, 4, 5, 9, 33, 3, 21, 46, 0, 12, 13, 30, 31, 32, 2, 25, 44, 19, 8])
    inside = set(rows.tolist())
    res = jx.fvlmm2_screen_packed(c["packed"], N_STAT, c["flip"], c["r"], c["sigma2"], c["var"], t_min, rows=rows)
    ref = _ref_hits(c, c["exact"], t_min, lambda i, j: i in inside and j in inside)
    assert res["pairs_screened"] == 20 * 19 // 2 and res["hits_total"] == len(ref) > 0
    _same_up_to_exact_ties(_got_hits(res), ref)
    # a capacity below the count raises and names it; nothing is truncated silently
    total = len(_ref_hits(c, c["exact"], t_min))
    with pytest.raises(RuntimeError, match=rf"{total} hits exceed the capacity of 7; raise t_min"):
        jx.fvlmm2_screen_packed(c["packed"], N_STAT, c["flip"], c["r"], c["sigma2"], c["var"], t_min, cap=7)
    full = jx.fvlmm2_screen_packed(c["packed"], N_STAT, c["flip"], c["r"], c["sigma2"], c["var"], t_min, cap=total)
    assert full["hits_total"] == total == len(full["stat"])


def test_entry_point_refusals():
    import torch
    from janusx_amd._lib import lib
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    L = lib()
    assert L.jxg_pairscreen_max_variants() == 16

    def scan(n=64, nrows=4, nv=1, sigma2=1.0, t_min=1.0, min_dist=0, stride=128):
        st = L.jxg_pairscreen_scan_p32(p, 4, n, None, nrows, p, None, None, min_dist, p, stride, 1.0, sigma2, p, nv, t_min, 4, p, p, p, p, p,
                                       p, None)
        return st, L.jx_last_error().decode()
    assert scan(n=0) == (1, "jxg_pairscreen_scan_p32: n must be > 0")
    assert scan(n=(1 << 24) + 1, stride=1 << 25)[1].startswith("jxg_pairscreen_scan_p32: at most 16 777 216 samples")
    assert scan(nv=17)[1] == "jxg_pairscreen_scan_p32: between 1 and 16 variants, got 17"
    assert scan(sigma2=0.0)[1] == "jxg_pairscreen_scan_p32: sigma2 must be finite and positive"
    assert scan(t_min=math.nan)[1] == "jxg_pairscreen_scan_p32: t_min is NaN"
    assert scan(min_dist=5)[1] == "jxg_pairscreen_scan_p32: min_dist needs chromosome ids and positions"
    assert scan(stride=64)[1].startswith("jxg_pairscreen_scan_p32: the digit planes of r are missing or shorter")
    st = L.jxg_pairscreen_tables_p32(p, 4, 64, None, 2, p, 2, p, 128, p, p, None)
    assert st == 1 and L.jx_last_error().decode() == "jxg_pairscreen_tables_p32: row lists or outputs missing"


def test_command_screen_end_to_end(tmp_path, capsys):
    """n = 160, m = 60, y = 2 min(g_20, g_41) + noise with the literals' own effects projected out: the planted pair leads the
    screen table, its `&` line stands in the leading group of equal statistics (a&b, a|b, !a&!b, !a|!b share one T, see the module
    text), the pair reaches the joint table in the existing layout, and the BH count is pairs screened x variants."""
    from janusx_amd import bed, cli
    from janusx_amd import fvlmm2 as f2
    n, m, a, b = 160, 60, 20, 41
    packed, g = bed.synth_panel_numpy(n, m, seed=314, missing_rate=0.0, maf_low=0.3, maf_high=0.5)
    ids = [f"s{i}" for i in range(n)]
    bim = bed.Bim([str(1 + j // 30) for j in range(m)], [f"rs{j}" for j in range(m)], [1000 + 100 * j for j in range(m)], ["A"] * m, ["G"] * m)
    prefix = str(tmp_path / "panel")
    bed.write_bed(prefix, packed, ids, bim)
    rng = np.random.default_rng(314)
    combo = np.minimum(g[a], g[b]).astype(np.float64)
    z = np.column_stack([np.ones(n), g[a], g[b]]).astype(np.float64)
    combo -= z @ np.linalg.lstsq(z, combo, rcond=None)[0]               # no main effects: what the literals explain is taken out
    y = 2.0 * combo + 0.5 * rng.normal(size=n)
    with open(tmp_path / "ph.tsv", "w") as fh:
        fh.write("id\tT1\n" + "".join(f"{ids[i]}\t{float(y[i])!r}\n" for i in range(n)))
    out = str(tmp_path / "res")
    assert cli.main(["fvlmm2", "-bfile", prefix, "-p", str(tmp_path / "ph.tsv"), "-screen", "1e-4", "-screen-top", "8", "-o", out]) == 0
    text = capsys.readouterr().out
    lines = [ln.split("\t") for ln in open(out + ".T1.fvlmm2.screen.tsv").read().splitlines()]
    assert tuple(lines[0]) == f2.SCREEN_COLUMNS and len(lines) > 4
    assert lines[1][:2] == [f"rs{a}", f"rs{b}"] and lines[1][3] == str(n)
    lead = [ln[2] for ln in lines[1:] if ln[4] == lines[1][4] and ln[:2] == lines[1][:2]]
    assert sorted(lead) == sorted([f"rs{a}&rs{b}", f"rs{a}|rs{b}", f"!rs{a}&!rs{b}", f"!rs{a}|!rs{b}"]) and lead == [ln[2] for ln in lines[1:5]]
    stats = [float(ln[4]) for ln in lines[1:]]
    assert stats == sorted(stats, reverse=True) and stats[-1] >= f2.chi2_1_quantile(1e-4) - 5e-5
    for ln in lines[1:]:                                               # the tail of the printed statistic: dp / p = dT / 2
        pv = f2.chi2_1_pvalue(float(ln[4]))
        assert abs(float(ln[5]) - pv) <= 1e-3 * pv and float(ln[5]) <= 1.001e-4, ln
    # every combo_id reads back through the interaction parser
    names, index = f2.build_name_map([str(1 + j // 30) for j in range(m)], [1000 + 100 * j for j in range(m)], [f"rs{j}" for j in range(m)])
    assert all(isinstance(f2._resolve_expression(ln[2], index), f2.PairSpec) for ln in lines[1:])
    joint = [ln.split("\t") for ln in open(out + ".T1.fvlmm2.tsv").read().splitlines()]
    assert tuple(joint[0]) == f2.OUTPUT_COLUMNS and len(joint) == 1 + min(8, len(lines) - 1)
    assert [ln[2] for ln in joint[1:]] == [ln[2] for ln in lines[1:len(joint)]]
    planted = next(ln for ln in joint[1:] if ln[2] == f"rs{a}&rs{b}")
    assert planted[0] == "1" and planted[1] == str(1000 + 100 * a) and float(planted[7]) < 1e-8
    # the default BH count: pairs screened x variants (every site passes the filters: 60 active rows)
    n_tests = m * (m - 1) // 2 * 10
    assert f"BH hypothesis count: {n_tests} (pairs screened x variants)" in text
    p = np.array([float(ln[7]) for ln in joint[1:]])
    exp = f2.bh_adjust(p, n_tests=n_tests)
    assert all(abs(float(ln[8]) - e) <= 2.1e-4 * e for ln, e in zip(joint[1:], exp))
    # --n-tests still overrides
    out2 = str(tmp_path / "res2")
    assert cli.main(["fvlmm2", "-bfile", prefix, "-p", str(tmp_path / "ph.tsv"), "-screen", "1e-4", "-screen-top", "8", "-o", out2,
                     "--n-tests", "50", "-screen-ops", "&,*", "-screen-min-dist", "250"]) == 0
    assert "BH hypothesis count" not in capsys.readouterr().out
    joint2 = [ln.split("\t") for ln in open(out2 + ".T1.fvlmm2.tsv").read().splitlines()]
    p2 = np.array([float(ln[7]) for ln in joint2[1:]])
    assert all(abs(float(ln[8]) - e) <= 2.1e-4 * e for ln, e in zip(joint2[1:], f2.bh_adjust(p2, n_tests=50)))
