"""The 16-byte forms of the f64 GEMM family (csrc/k_dgemm.hip: wide steady-state operand loader of `dgemm_kernel`, wide operand and
C accesses of `dsyr2k_pipe_kernel<true>`) against the 8-byte forms (JXGPU_DGEMM_WIDE=0), inside one process through the C-ABI
entries.  The wide forms change how bytes travel, never which products are summed in which order: every comparison is bit for bit.
Where a torch f64 product is also compared, the bar is the one of tests/test_gpu_parity.py::test_f64_gemm_family (1e-13 of the
largest reference element).

Buffers are column-major; a torch tensor of shape (cols, ld) is the matrix with leading dimension ld.  The wide forms need 16-byte
aligned bases and even leading dimensions, so matrices with an odd row count are stored with ld = rows + 1 where the wide form is
meant to run, and with ld = rows (or a base moved by one double) where the fallback is."""
import contextlib
import os

import pytest

pytestmark = pytest.mark.gpu
PARITY = 1e-13


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _both(run):
    """run() under JXGPU_DGEMM_WIDE=0 and under the default; returns (narrow, wide)."""
    import torch
    outs = []
    for form in ("0", None):
        with _env(JXGPU_DGEMM_WIDE=form):
            outs.append(run())
            torch.cuda.synchronize()
    return outs


def _ctx(seed):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, generator=g, device=dev, dtype=torch.float64)   # noqa: E731
    return dev, torch.cuda.current_stream().cuda_stream, rnd


def _even(x):
    return x + (x & 1)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("m,n,k", [(130, 66, 50), (257, 129, 1040), (64, 64, 272)])
def test_dgemm_wide_loader_same_bits(m, n, k):
    """NN / TN / NT / TT, automatic split and ksplit = 1, beta = 0 and beta != 0: ragged M and N, a K tail, the three tile
    instantiations, K long enough for runs of the stream loader.  Even leading dimensions: the wide form runs, also at odd m."""
    from janusx_amd._lib import check, lib
    dev, st, rnd = _ctx(1000 * m + k)
    L = lib()
    for ta in (0, 1):
        for tb in (0, 1):
            ra, ca = (k, m) if ta else (m, k)            # stored A: ra x ca
            rb, cb = (n, k) if tb else (k, n)
            lda, ldb, ldc = _even(ra), _even(rb), _even(m)
            a, b, c0 = rnd(ca, lda), rnd(cb, ldb), rnd(n, ldc)
            # the tensor (cols, ld) is the stored matrix transposed: op(A) (m x k) and op(B) (k x n)
            prod = (a[:, :ra] if ta else a[:, :ra].T) @ (b[:, :rb] if tb else b[:, :rb].T)
            for ksplit in (0, 1):
                for beta in (0.0, 0.75):
                    def run():
                        c = c0.clone()
                        check(L.jxg_dgemm_f64(ta, tb, m, n, k, -0.5, a.data_ptr(), lda, b.data_ptr(), ldb, beta, c.data_ptr(), ldc,
                                              ksplit, st))
                        return c
                    narrow, wide = _both(run)
                    assert bool(wide.equal(narrow)), (ta, tb, ksplit, beta)
                    ref = -0.5 * prod + beta * c0[:, :m].T
                    assert _rel(wide[:, :m].T, ref) < PARITY, (ta, tb, ksplit, beta)
                    assert bool(wide[:, m:].equal(c0[:, m:]))                 # the padding rows of C are not written


def _symm_case(rnd, dev, m, n, ld, shift=0):
    """Lower-stored symmetric A (the strict upper triangle poisoned), B, C with leading dimension ld, every base moved by `shift`
    doubles from its allocation."""
    import torch
    def buf(cols):                                                              # noqa: E306
        flat = rnd(cols * ld + shift)
        return flat[shift:].view(cols, ld)
    a, b, c0 = buf(m), buf(n), buf(n)
    at = a[:, :m]                                                               # at[j, i] = A[i][j]
    full = torch.tril(at.T) + torch.tril(at.T, -1).T
    at.T.masked_fill_(torch.triu(torch.ones((m, m), device=dev, dtype=torch.bool), 1), 1e300)
    ref = 0.7 * (full @ b[:, :m].T) + 0.3 * c0[:, :m].T
    return a, b, c0, ref


def _symm_run(a, b, c0, m, n, ld, st):
    from janusx_amd._lib import check, lib
    def run():                                                                  # noqa: E306
        c = c0.clone()
        check(lib().jxg_dsymm_lower_f64(m, n, 0.7, a.data_ptr(), ld, b.data_ptr(), ld, 0.3, c.data_ptr(), ld, st))
        return c
    return run


@pytest.mark.parametrize("m", [400, 1300])
@pytest.mark.parametrize("n", [16, 64, 96])
def test_dsymm_wide_loader_same_bits(m, n):
    """Tiles left of, right of and across the diagonal (x-fast, k-fast and general steps), both tile widths, a K split."""
    dev, st, rnd = _ctx(7 * m + n)
    a, b, c0, ref = _symm_case(rnd, dev, m, n, m)
    narrow, wide = _both(_symm_run(a, b, c0, m, n, m, st))
    assert bool(wide.equal(narrow))
    assert _rel(wide.T, ref) < PARITY


def _syr2k_case(m, k, seed):
    import torch
    dev, st, rnd = _ctx(seed)
    a, b, c0 = rnd(k, m), rnd(k, m), rnd(m, m)
    # the tensor's [j, i] is C[i][j]: the strict upper triangle of C is the strict lower triangle of the tensor
    upper = torch.tril(torch.ones((m, m), device=dev, dtype=torch.bool), -1)
    c0.masked_fill_(upper, 1e300)
    return st, a, b, c0, upper


@pytest.mark.parametrize("m,wgs", [(3600, "64"), (3650, "64"), (300, None)])
def test_dsyr2k_wide_forms_same_bits(m, wgs):
    """K = 128.  m = 3600 and 3650 (ragged last tile) on 64 workgroups: 435 tiles are fewer than two per workgroup of the default
    grid (7 / 8 of the CUs), which would select the one-tile-per-workgroup form -- JXGPU_SYR2K_PIPE_WGS=64 gives the persistent
    kernel six to seven tiles each.  m = 300: the general form.  The strict upper triangle holds a sentinel and is not touched;
    the lower triangle also agrees with the one-tile-per-workgroup form (JXGPU_SYR2K_PIPE=0, 8-byte accesses: the row-pair
    relabelling of the persistent kernel changes no sum) and with torch."""
    from janusx_amd._lib import check, lib
    k = 128
    st, a, b, c0, upper = _syr2k_case(m, k, m)
    def run():                                                                  # noqa: E306
        c = c0.clone()
        check(lib().jxg_dsyr2k_lower_nt_f64(m, k, -1.0, a.data_ptr(), m, b.data_ptr(), m, 1.0, c.data_ptr(), m, st))
        return c
    with _env(JXGPU_SYR2K_PIPE_WGS=wgs):
        narrow, wide = _both(run)
        with _env(JXGPU_SYR2K_PIPE="0", JXGPU_DGEMM_WIDE="0"):
            plain = run()
    assert bool(wide.equal(narrow))
    assert bool(wide.equal(plain))
    assert bool(wide[upper].equal(c0[upper]))
    ref = c0 - b.T @ a                                                          # C^T = C0^T - B A'
    assert float((wide - ref)[~upper].abs().max() / ref[~upper].abs().max()) < PARITY


@pytest.mark.parametrize("ld,shift", [(1301, 0), (1302, 1)])
def test_misaligned_inputs_take_the_narrow_form(ld, shift):
    """m = 1301 stored with an odd leading dimension, and with every base pointer one double off a 16-byte boundary: no 16-byte
    access is possible, both settings run the 8-byte form, agree with each other and with torch."""
    m, n = 1301, 64
    dev, st, rnd = _ctx(ld + shift)
    a, b, c0, ref = _symm_case(rnd, dev, m, n, ld, shift)
    assert a.data_ptr() % 16 == 8 * shift
    narrow, wide = _both(_symm_run(a, b, c0, m, n, ld, st))
    assert bool(wide.equal(narrow))
    assert _rel(wide[:, :m].T, ref) < PARITY
    assert _rel(narrow[:, :m].T, ref) < PARITY


def test_odd_m_with_even_ld_takes_the_wide_form():
    """m = 1301 stored with ld = 1302 on aligned bases is eligible: the ragged last tile row keeps 8-byte loads for its x-fast
    steps, everything else is wide -- bit for bit the 8-byte result, and the padding row of C is not written."""
    m, n, ld = 1301, 64, 1302
    dev, st, rnd = _ctx(5)
    a, b, c0, ref = _symm_case(rnd, dev, m, n, ld)
    assert a.data_ptr() % 16 == 0
    narrow, wide = _both(_symm_run(a, b, c0, m, n, ld, st))
    assert bool(wide.equal(narrow))
    assert _rel(wide[:, :m].T, ref) < PARITY
    assert bool(wide[:, m:].equal(c0[:, m:]))


@pytest.mark.parametrize("n", [1700, 1701])
def test_eigh_same_bits(n):
    """`jxg_eigh_f64` on the two-stage path: n = 1700 (even ld: wide forms in the band reduction and the back-transformation's
    products), n = 1701 (odd ld: fallback).  Eigenvalues and eigenvectors are the same bits under both settings."""
    import torch
    from janusx_amd._lib import check, lib
    dev, st, rnd = _ctx(n)
    x = rnd(n, n + 40)
    k = x @ x.T / (n + 40)
    def run():                                                                  # noqa: E306
        a = k.clone()
        w = torch.empty(n, device=dev, dtype=torch.float64)
        check(lib().jxg_eigh_f64(a.data_ptr(), n, 0.0, w.data_ptr(), st))
        return torch.cat([w, a.reshape(-1)])
    narrow, wide = _both(run)
    assert bool(wide.equal(narrow))
    w = wide[:n]
    assert _rel(w.sort().values, torch.linalg.eigvalsh(k)) < 1e-12
