"""Q1 back-transformation: the reflector blocks prepared beside the last panels of the band reduction (JXGPU_Q1_TAIL_NT, csrc/eigh.cpp
and csrc/k_ormtr.hip, behind src/math/eigh.rs:1422-1528) against the same blocks prepared in line in front of the Q1 products.  Every
kernel of a block sees the arguments of the in-line form -- the chunked launches cover disjoint rows with the K split of the whole
call -- so eigenvalues and eigenvectors must be the same bits.  The switch is read per call: the forms run in one process."""
import os

import pytest


def _grm_like(n, seed):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    z = torch.randn((n, n + 64), generator=g, device=dev, dtype=torch.float32)
    k = (z @ z.T / (n + 64)).to(torch.float64)
    return 0.5 * (k + k.T)


def _block_diagonal(n, seed):
    """families of 7, as a thresholded sparse GRM looks, and one pair of relatives 100 samples apart at the end.  The families
    alone lie inside the band (half bandwidth 64): every panel is in the reduced form [R; 0] already and passes without a flag.
    The pair puts one entry under the band of column n - 101, so its panel has a single non-zero column beside the corner of R:
    exactly rank-deficient and not reduced, which the band reduction flags."""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    k = torch.zeros((n, n), device=dev, dtype=torch.float64)
    for b0 in range(0, n, 7):
        b1 = min(n, b0 + 7)
        z = torch.randn((b1 - b0, 20), generator=g, device=dev, dtype=torch.float64)
        k[b0:b1, b0:b1] = z @ z.T / 20
    k[n - 1, n - 101] = k[n - 101, n - 1] = 0.25      # inside the last 192 rows, which the one-stage reduction finishes in one workgroup
    return 0.5 * (k + k.T)


def _eigh_with(k, tail_nt):
    from janusx_amd import pipeline
    old = os.environ.get("JXGPU_Q1_TAIL_NT")
    try:
        if tail_nt is None:
            os.environ.pop("JXGPU_Q1_TAIL_NT", None)
        else:
            os.environ["JXGPU_Q1_TAIL_NT"] = tail_nt
        return pipeline.eigh_from_grm(k, 1e-6)
    finally:
        if old is None:
            os.environ.pop("JXGPU_Q1_TAIL_NT", None)
        else:
            os.environ["JXGPU_Q1_TAIL_NT"] = old


def _check_invariants(k, s, ut):
    import torch
    n = k.shape[0]
    kk = k.clone()
    kk.diagonal().add_(1e-6)
    smax = float(s.abs().max())
    assert bool((s[1:] >= s[:-1]).all())
    assert float((ut @ kk - s[:, None] * ut).abs().max()) < 1e-11 * smax
    assert float((ut @ ut.T - torch.eye(n, device=k.device, dtype=torch.float64)).abs().max()) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3200, 1700])
def test_q1_blocks_prepared_beside_the_band_reduction_give_the_same_bits(n):
    """n = 3200: Q1 on the int8 pipes, 1024-reflector blocks of 3135 reflectors (three full blocks and a ragged one of 63; the last is
    always prepared in line).  n = 1700: Q1 on the f64 GEMM (below JXGPU_OZ_MIN_N), blocks of 1024 and 611 -- V T of the first is
    issued in row chunks with a K split of 2.  In line (0), the default, and a threshold (1500) that is reached after the first
    blocks are complete: w and U bit for bit."""
    import torch
    from janusx_amd._lib import lib
    k = _grm_like(n, n)
    out = {}
    for nt in ("0", None, "1500"):
        out[nt] = _eigh_with(k, nt)
        assert float(lib().jxg_last_kernel_ms(10)) == 1.0      # the two-stage path, not its fallback
    for nt in (None, "1500"):
        assert torch.equal(out[nt][0], out["0"][0]), nt
        assert torch.equal(out[nt][1], out["0"][1]), nt
    _check_invariants(k, *out[None])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [700, 2200])
def test_q1_blocks_prepared_for_a_flagged_band_reduction_are_discarded(n, monkeypatch):
    """A block-diagonal matrix: the band reduction flags a rank-deficient panel, the plan is dropped and the one-stage fallback gives
    what it gives with everything in line.  700 rows (two-stage forced): one block, nothing prepared ahead; 2200 rows: two
    1024-reflector blocks were prepared beside the band reduction when the flag is read."""
    import torch
    from janusx_amd._lib import lib
    if n < 1500:
        monkeypatch.setenv("JXGPU_EIGH", "twostage")
    k = _block_diagonal(n, 11)
    s1, u1 = _eigh_with(k, None)
    assert float(lib().jxg_last_kernel_ms(10)) == 0.0          # the fallback was taken
    s0, u0 = _eigh_with(k, "0")
    assert torch.equal(s1, s0) and torch.equal(u1, u0)
    _check_invariants(k, s1, u1)
