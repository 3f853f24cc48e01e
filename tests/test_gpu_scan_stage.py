"""The callback contract of `pipeline.scan_rows`: which blocks `on_block` is handed and when `progress` is called, whatever
scan runs behind the rotation stage.  n = 320 samples (three column tiles, the last one ragged), 600 SNP rows with 1 % missing
calls in blocks of 256 (two full blocks and a remainder of 88)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from janusx_amd import bed  # noqa: E402


@pytest.fixture(scope="module")
def stage_case():
    """Synthetic eigenbasis (QR of a seeded normal matrix, seeded positive spectrum): no eigendecomposition needed."""
    import torch
    from janusx_amd import pipeline, stats
    n, m = 320, 600
    dev = torch.device("cuda", 0)
    packed, _g = bed.synth_panel_numpy(n, m, seed=93, missing_rate=0.01)
    panel = pipeline.Panel(torch.from_numpy(packed).to(dev), n)
    counts = panel.counts()
    _keep, af, _miss = stats.gwas_scan_row_stats(counts, n, 0.02, 0.05, 1.0)
    rows = np.arange(m, dtype=np.int32)
    lut = stats.scan_lut_from_counts(af, np.zeros(m, bool), counts, n)
    rng = np.random.default_rng(93)
    u = np.linalg.qr(rng.standard_normal((n, n)))[0]
    s = np.sort(rng.gamma(2.0, 0.5, n)) + 1e-3
    y = u @ (np.sqrt(s) * rng.standard_normal(n)) + rng.standard_normal(n)
    x = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, 1))], axis=1)
    model = pipeline.SpectralModel(torch.from_numpy(s).to(dev), torch.from_numpy(np.ascontiguousarray(u.T)).to(dev), x, y)
    return panel, model, rows, lut


def _scan_with_callbacks(case, mode, **kw):
    from janusx_amd import pipeline
    panel, model, rows, lut = case
    blocks, ticks = [], []
    out = pipeline.scan_rows(panel, model, rows, lut, mode, block_rows=256, progress_every=300,
                             on_block=lambda i0, blk: blocks.append((i0, np.array(blk))),
                             progress=lambda done, total: ticks.append((done, total)), **kw)
    return out.cpu().numpy(), blocks, ticks


@pytest.mark.parametrize("mode", ["fvlmm", "lmm"])
def test_scan_rows_hands_over_every_block_in_order(stage_case, mode):
    """`on_block` gets the blocks of `block_rows` rows as they finish, in order, with the bytes of the returned table;
    `progress` is called when `progress_every` rows have passed since its last call (after the second block: 512 >= 300; not
    after the first) and after the last block."""
    out, blocks, ticks = _scan_with_callbacks(stage_case, mode)
    assert out.shape == (600, 3) and np.isfinite(out).any()
    assert [(i0, len(blk)) for i0, blk in blocks] == [(0, 256), (256, 256), (512, 88)]
    assert np.concatenate([blk for _i0, blk in blocks]).tobytes() == out.tobytes()
    assert ticks == [(512, 600), (600, 600)]


def test_scan_rows_chain_series_hands_over_the_whole_table_once(stage_case):
    """With warm-start chains in the series form the Brent searches of a super-block run behind its last block, so `on_block`
    gets the whole table once, at the end; `progress` still follows the blocks."""
    from janusx_amd._lib import lib
    model = stage_case[1]
    lo, hi = model.null.bounds
    assert int(lib().jxg_lmm_series_doubles(model.p, lo, hi)) > 0          # the series form
    co = np.array([0, 150, 300, 450, 600], dtype=np.int64)
    out, blocks, ticks = _scan_with_callbacks(stage_case, "lmm", chain_off=co,
                                              init_log10_lbd=min(max(math.log10(model.null.lbd), lo), hi))
    assert np.isfinite(out).any()
    assert len(blocks) == 1 and blocks[0][0] == 0 and blocks[0][1].tobytes() == out.tobytes()
    assert ticks == [(512, 600), (600, 600)]


def test_scan_rows_exception_in_progress_ends_the_scan(stage_case):
    """An exception raised in `progress` propagates out of `scan_rows`; no block behind the one it was raised after is handed
    over."""
    from janusx_amd import pipeline
    panel, model, rows, lut = stage_case
    seen = []

    def stop(done, total):
        raise RuntimeError(f"stopped at {done} of {total}")

    with pytest.raises(RuntimeError, match="stopped at 512 of 600"):
        pipeline.scan_rows(panel, model, rows, lut, "fvlmm", block_rows=256, progress_every=300,
                           on_block=lambda i0, blk: seen.append(i0), progress=stop)
    assert seen == [0]
