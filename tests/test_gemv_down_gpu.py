"""The straight-line form of the one-row decode GEMV at K = 14336 (csrc/llm_k.hip gemv_stream_kernel; down_proj of the decode step)
against gemv_kernel (usdm_gemv_args.resident = -1) and against an exact integer reference.  Every comparison is == on the raw bf16 /
f32 bits.  resident = 1 selects the form at any N: 16 = one workgroup, 40 = a ragged last workgroup (8 of its 16 rows), 272 = 17
workgroups; N = 4096 is the 7B's shape under the launcher's own choice.  The row stride is K and K + 8 (the gap holds values that
would show), every output is followed by a sentinel-filled gap."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K = 14336
NS = (16, 40, 272)
LDWS = (K, K + 8)
PAD = 64
FILL = float("nan")     # no output is NaN (finite operands), so an element that still holds it was not written


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _launch(W, x, n, ldw, resident, res=None, rbf=True, inplace=False, y32_only=False, skip=None):
    """-> (y16 or None, y32), each n outputs and PAD sentinels; inplace: y16 starts as the residual and is passed as both"""
    from usdm_amd import ops
    dev = W.device
    y16 = None if y32_only else torch.full((n + PAD,), FILL, dtype=BF, device=dev)
    y32 = torch.full((n + PAD,), FILL, device=dev)
    if inplace:
        y16[:n] = res
        res = y16
    ops.gemv(W, x, N=n, K=K, ldw=ldw, round_bf16=rbf, residual=res, y16=y16, y32=y32, skip=skip, resident=resident)
    torch.cuda.synchronize()
    for y in (y16, y32):
        assert y is None or bool(y[n:].isnan().all()), "written beyond N"
    return y16, y32


def _same(a, b):
    return all(p is None and q is None or torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def random_cases(dev):
    """{(N, ldw): (W, x, residual)}, made once and never changed"""
    gen = torch.Generator().manual_seed(14336)
    out = {}
    for n in NS:
        for ldw in LDWS:
            W = torch.full((n, ldw), 7.0)
            W[:, :K] = torch.randn((n, K), generator=gen) * K ** -0.5
            out[n, ldw] = (W.to(BF).to(dev), torch.randn(K, generator=gen).to(BF).to(dev), torch.randn(n, generator=gen).to(BF).to(dev))
    return out


@pytest.mark.parametrize("ldw", LDWS)
@pytest.mark.parametrize("n", NS)
def test_stream_equals_gemv_kernel(dev, random_cases, n, ldw):
    W, x, res = random_cases[n, ldw]
    skip = torch.ones(1, dtype=torch.int32, device=dev)
    variants = [dict(), dict(res=res), dict(res=res, rbf=False), dict(rbf=False), dict(res=res, y32_only=True), dict(y32_only=True)]
    for kw in variants:
        a, b = _launch(W, x, n, ldw, -1, **kw), _launch(W, x, n, ldw, 1, **kw)
        assert _same(a, b), (n, ldw, kw)
        assert not bool(a[1][:n].isnan().any()) and float(a[1][:n].abs().max()) > 0
        y16, y32 = _launch(W, x, n, ldw, 1, skip=skip, **kw)
        assert bool(y32.isnan().all()) and (y16 is None or bool(y16.isnan().all())), (n, ldw, kw, "written although *skip = 1")
    # the in-place form of the step: residual and y16 are one array
    a = _launch(W, x, n, ldw, -1, res=res)
    for r in (-1, 1):
        assert _same(a, _launch(W, x, n, ldw, r, res=res, inplace=True)), (n, ldw, r)
    y16, y32 = _launch(W, x, n, ldw, 1, res=res, inplace=True, skip=skip)
    assert torch.equal(_bits(y16[:n]), _bits(res)) and bool(y32.isnan().all())


def _integer_case(n, ldw, seed, dev):
    """W in {-1, 0, 1} (about K / 16 random entries per row, the rest placed so that row o sums to t(o) in +-[1, 127], a value that
    depends on o), x in +-{1, 2}, a residual of integers in [-8, 8]: every partial sum is an integer below 2^24, exact in f32 in any
    order, and t(o) + residual is exact in bf16.  A lost or repeated K iteration, a row of another workgroup or a piece of x staged
    at the wrong offset changes the integer."""
    gen = torch.Generator().manual_seed(seed)
    sgn = torch.randint(0, 2, (K,), generator=gen).double() * 2 - 1
    mag = torch.randint(1, 3, (K,), generator=gen).double()
    xp = sgn * mag
    o = torch.arange(n)
    target = ((o * 37) % 127 + 1).double() * (1 - 2 * ((o // 2) % 2)).double()
    ones = (mag == 1).nonzero().flatten()
    W = (torch.rand((n, K), generator=gen) < 1 / 16).double() * (torch.randint(0, 2, (n, K), generator=gen).double() * 2 - 1)
    for r in range(n):
        d = int(target[r] - W[r] @ xp)
        free = ones[W[r, ones] == 0]
        at = free[torch.randperm(free.numel(), generator=gen)[:abs(d)]]
        assert at.numel() == abs(d)
        W[r, at] = sgn[at] * (1 if d > 0 else -1)           # each adds +-1 to the row's sum
    assert torch.equal(W @ xp, target)
    Wp = torch.full((n, ldw), 7.0, dtype=torch.float64)
    Wp[:, :K] = W
    res = torch.randint(-8, 9, (n,), generator=gen).double()
    return Wp.to(BF).to(dev), xp.to(BF).to(dev), res.to(BF).to(dev), target, res


@pytest.mark.parametrize("n", NS)
def test_stream_exact_integers(dev, n):
    for ldw in LDWS:
        W, x, res, target, resd = _integer_case(n, ldw, 500 + n, dev)
        for r in (-1, 1):
            for rbf in (False, True):
                y16, y32 = _launch(W, x, n, ldw, r, rbf=rbf)
                assert torch.equal(y32[:n].cpu().double(), target) and torch.equal(y16[:n].cpu().double(), target), (n, ldw, r, rbf)
                y16, y32 = _launch(W, x, n, ldw, r, res=res, rbf=rbf)
                assert torch.equal(y32[:n].cpu().double(), target + resd) and torch.equal(y16[:n].cpu().double(), target + resd), (n, ldw, r, rbf)
            y16, y32 = _launch(W, x, n, ldw, r, res=res, inplace=True)
            assert torch.equal(y16[:n].cpu().double(), target + resd) and torch.equal(y32[:n].cpu().double(), target + resd), (n, ldw, r)


def test_stream_default_on_the_7b_shape(dev):
    """down_proj of the 7B, the launcher's own choice against gemv_kernel; random weights made on the device, no residual"""
    from usdm_amd import _lib, ops
    n = 4096
    gen = torch.Generator(device=dev).manual_seed(7)
    W = (torch.randn((n, K), generator=gen, device=dev) * K ** -0.5).to(BF)
    x = torch.randn(K, generator=gen, device=dev).to(BF)
    args = lambda r: ops.gemv(W, x, N=n, K=K, y32=torch.empty(1, device=dev), only_args=True, resident=r)
    assert _lib.lib.usdm_gemv_streams(ctypes.byref(args(0))) == 1 and _lib.lib.usdm_gemv_streams(ctypes.byref(args(-1))) == 0
    a = _launch(W, x, n, K, -1)
    for r in (0, 1):
        assert _same(a, _launch(W, x, n, K, r)), r
    assert float(a[1][:n].abs().max()) > 0 and not bool(a[1][:n].isnan().any())
