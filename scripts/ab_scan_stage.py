"""A/B of the packed scan routes through the public names of `janusx_amd.pipeline` only, so that the same file runs against
two checkouts: seeded inputs, one process, one line `route=<name> digest=<sha256[:16]> finite=<count>` per route.  The digest
covers the returned table (and the Brent evaluation counts where asked for), every (i0, block) handed to `on_block` in order and
the (done, total) sequence of `progress`.  Shapes: n = 320 / m = 600 (three column tiles, the last one ragged; fp16 rotation
only) and n = 4224 / m = 1500 (first size on the int8 rotation, 33 tiles) at the missing rates 0 (identity lists), 0.002 (gather
form of the missing-call term) and 0.01 (dense form); block_rows 100 and 256.
usage: ab_scan_stage.py [out.json]   (from the checkout to test; two outputs must be equal line by line)"""
import hashlib, json, math, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from janusx_amd import pipeline as pl, stats as st
from janusx_amd._lib import lib

dev = torch.device("cuda", 0)
LINES = {}


def digest_route(name, call, **kw):
    """call(**kw, on_block=..., progress=...) when `kw` asks for callbacks; -> one output line"""
    h = hashlib.sha256()
    if kw.pop("callbacks", False):
        kw["on_block"] = lambda i0, blk: (h.update(np.int64(i0).tobytes()), h.update(np.ascontiguousarray(blk).tobytes()))
        kw["progress"] = lambda done, total: h.update(np.asarray([done, total], dtype=np.int64).tobytes())
    res = call(**kw)
    finite = 0
    for t in (res if isinstance(res, tuple) else (res,)):
        a = t.cpu().numpy()
        h.update(a.tobytes())
        finite += int(np.isfinite(a).sum()) if a.dtype.kind == "f" else 0
    LINES[name] = {"digest": h.hexdigest()[:16], "finite": finite}
    print(f"route={name} digest={h.hexdigest()[:16]} finite={finite}", flush=True)


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def orthonormal(nb, rng):
    return np.linalg.qr(rng.standard_normal((nb, nb)))[0]


def make_model(n, p, seed):
    """Synthetic eigenbasis: U^T from the QR of a seeded normal matrix, a seeded positive spectrum, a trait with a polygenic
    part on that spectrum; intercept + (p - 1) seeded covariates."""
    rng = np.random.default_rng(seed)
    u = orthonormal(n, rng)
    s = np.sort(rng.gamma(2.0, 0.5, n)) + 1e-3
    y = u @ (np.sqrt(s) * rng.standard_normal(n)) + rng.standard_normal(n)
    x = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, p - 1))], axis=1)
    return pl.SpectralModel(torch.from_numpy(s).to(dev), torch.from_numpy(np.ascontiguousarray(u.T)).to(dev), x, y), x, y


def splmm_state(s, xr, yr, lam):
    """Null state of the SparseLMM exact scan on the K + lambda I scale from rotated X~, y~ (f64 on the host)."""
    d = s + lam
    wx = xr / d[:, None]
    a_chol = np.linalg.cholesky(xr.T @ wx)
    b0 = np.linalg.solve(a_chol.T, np.linalg.solve(a_chol, wx.T @ yr))
    py = (yr - xr @ b0) / d
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    return f32(1.0 / d), f32(py), f32(wx), a_chol, float(yr @ py)


def panel_rows(n, m, missing):
    packed, _ = bench.synth_panel_gpu(n, m, 20260609, dev, missing_rate=missing)
    panel = pl.Panel(packed, n)
    counts = panel.counts()
    _keep, af, _ms = st.gwas_scan_row_stats(counts, n, 0.02, 0.05, 1.0)
    rows = np.arange(m, dtype=np.int32)                   # every row: the row count is part of the blocking under test
    lut = st.scan_lut_from_counts(af[rows], np.zeros(len(rows), bool), counts[rows], n)
    raw = np.zeros((len(rows), 4), dtype=np.float32)      # the SparseLMM decode: [0, 2 maf, 1, 2], not centred
    raw[:, 1], raw[:, 2], raw[:, 3] = np.clip(2.0 * af[rows], 0.0, 2.0), 1.0, 2.0
    return packed, panel, rows, lut, raw


def dense_routes(tag, n, panel, rows, lut, raw, models, br):
    model = models[2]
    mk = len(rows)
    lo, hi = model.null.bounds
    init = min(max(math.log10(model.null.lbd), lo), hi)
    base = dict(block_rows=br)

    def scan(mode, mdl=model, l=lut, **kw):
        return lambda **cb: pl.scan_rows(panel, mdl, rows, l, mode, **{**base, **kw, **cb})
    t = f"{tag}/br{br}/"
    digest_route(t + "lmm", scan("lmm", return_evals=True))
    digest_route(t + "lmm_init", scan("lmm", init_log10_lbd=init, return_evals=True))
    digest_route(t + "lmm_nullml", scan("lmm", nullml=model.null.ml0))
    co = np.unique(np.concatenate([np.arange(0, mk, 150), [mk]])).astype(np.int64)
    chain = dict(init_log10_lbd=init, chain_off=co, return_evals=True, nullml=model.null.ml0)
    sd = int(lib().jxg_lmm_series_doubles(model.p, lo, hi))
    assert sd > 0 and 2 * br < mk and not np.isin(2 * br, co)      # the series form; the cut lies inside a chain
    digest_route(t + "lmm_chain_series", scan("lmm", **chain))
    cap = pl.SERIES_CAP_BYTES
    pl.SERIES_CAP_BYTES = 2 * br * 8 * (sd + 1 + 4)
    try:
        digest_route(t + "lmm_chain_series_superblocks", scan("lmm", **chain))
    finally:
        pl.SERIES_CAP_BYTES = cap
    assert int(lib().jxg_lmm_series_doubles(model.p, -5.0, 5.0)) == 0
    digest_route(t + "lmm_chain_block_wide_bounds", scan("lmm", low=-5.0, high=5.0, **chain))
    if 6 in models:      # six design columns: the block form of the objective (k_scan_fast.hip), chains in both forms
        m6 = models[6]
        l6, h6 = m6.null.bounds
        kw6 = dict(mdl=m6, chain_off=co, return_evals=True, init_log10_lbd=min(max(math.log10(m6.null.lbd), l6), h6))
        digest_route(t + "lmm_chain_p6", scan("lmm", **kw6))
        digest_route(t + "lmm_chain_block_p6_wide_bounds", scan("lmm", low=-5.0, high=5.0, **kw6))
    with env(JXGPU_SCAN_EXACT="1"):
        assert int(lib().jxg_lmm_tables_bytes(n, model.p, lo, hi)) == 0
        digest_route(t + "lmm_no_tables", scan("lmm", return_evals=True))
    digest_route(t + "lmm2", scan("lmm2", nullml=model.null.ml0, init_log10_lbd=init))
    for f in ("1", "0") + (("2",) if n >= 4096 else ()):
        with env(JXGPU_FVLMM_FUSED=f):
            digest_route(t + f"fvlmm_fused{f}", scan("fvlmm"))
            digest_route(t + f"splmm_fused{f}", scan("splmm", l=raw, fv_state=splmm_state(
                model.S.cpu().numpy(), model.xcov.cpu().numpy(), model.y.cpu().numpy(), model.null.lbd)))
    digest_route(t + "fvlmm_nullml", scan("fvlmm", nullml=model.null.ml0))
    if 9 in models:
        digest_route(t + "fvlmm_p9", scan("fvlmm", mdl=models[9]))
    digest_route(t + "lmm_callbacks", scan("lmm", progress_every=300), callbacks=True)
    digest_route(t + "lmm_chain_series_callbacks", scan("lmm", progress_every=300, **chain), callbacks=True)
    digest_route(t + "fvlmm_callbacks", scan("fvlmm", progress_every=300), callbacks=True)


def block_routes(n, packed, rows, raw, x, y, sizes=(129, 48, 1, 142)):
    """The block-diagonal basis: an orthonormal basis per diagonal block, the samples in a seeded order."""
    rng = np.random.default_rng(5)
    perm = rng.permutation(n).astype(np.int64)
    ut = np.zeros((n, n))
    blocks, off = [], 0
    for nb in sizes:
        q = orthonormal(nb, rng)
        ut[off:off + nb, off:off + nb] = q.T
        blocks.append((off, nb, torch.from_numpy(np.ascontiguousarray(q.T)).to(dev)))
        off += nb
    assert off == n
    s = rng.gamma(2.0, 0.5, n) + 1e-3
    rot = pl.BlockRotation(packed, n, perm, blocks)
    state = splmm_state(s, ut @ x[perm], ut @ y[perm], 0.7)
    digest_route("n320/rotate_rows_blocks", lambda: pl.rotate_rows_blocks(rot, rows[:200], raw[:200]))
    for br in (100, 256, 8192):
        for f in ("1", "0"):
            with env(JXGPU_FVLMM_FUSED=f):
                digest_route(f"n320/br{br}/splmm_blocks_fused{f}",
                             lambda: pl.scan_rows_splmm_blocks(rot, x.shape[1], rows, raw, state, block_rows=br))


def main():
    for k in ("JXGPU_ROT_I8", "JXGPU_FVLMM_FUSED", "JXGPU_ROT_MISS_MAX", "JXGPU_ROT_MISS_DENSE", "JXGPU_SCAN_EXACT"):
        os.environ.pop(k, None)
    n, m = 320, 600
    models, xs, ys = {}, {}, {}
    for p in (2, 6, 9):
        models[p], xs[p], ys[p] = make_model(n, p, 100 + p)
    packed, panel, rows, lut, raw = panel_rows(n, m, 0.01)
    for br in (100, 256):
        dense_routes("n320", n, panel, rows, lut, raw, models, br)
    digest_route("n320/rotate_rows", lambda: pl.rotate_rows(panel, models[2], rows[:200], lut[:200]))
    block_routes(n, packed, rows, raw, xs[2], ys[2])
    n, m = 4224, 1500
    model, _x, _y = make_model(n, 2, 4224)
    for missing in (0.0, 0.002, 0.01):
        packed, panel, rows, lut, raw = panel_rows(n, m, missing)
        for br in (100, 256):
            dense_routes(f"n4224_miss{missing:g}", n, panel, rows, lut, raw, {2: model}, br)
        digest_route(f"n4224_miss{missing:g}/rotate_rows", lambda: pl.rotate_rows(panel, model, rows[:300], lut[:300]))
    torch.cuda.synchronize()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(LINES, f, indent=1)


main()
