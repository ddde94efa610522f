"""The decode GEMV over the lossless 13-bit weight image (usdm_gemv_packed; csrc/llm_k.hip gemv_stream_wpack_kernel, down_proj of
the decode step) against the same call without the image - the straight-line bf16 form (resident = 1) and gemv_kernel
(resident = -1) - and against an exact integer reference.  Every comparison is == on the raw bf16 / f32 bits.
N = 16: one workgroup; 40: a ragged last workgroup; 272: 17 workgroups (the shapes of tests/test_gemv_down_gpu.py).  Rows with a
zero weight are planted so that both paths of the kernel run in one launch - a workgroup whose waves take different paths, a
workgroup of marked rows only, the last row; the flag array (and its copy as bits in the kernel argument) says that every other
row streamed the image."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K = 14336
LDWS = (K, K + 8)
PAD = 64
FILL = float("nan")
MARKED = {16: (3,), 40: (0, 17, 39), 272: (5,) + tuple(range(16, 32)) + (271,)}


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _launch(W, x, n, ldw, resident, wp=None, res=None, rbf=True, inplace=False, y32_only=False, skip=None):
    """-> (y16 or None, y32), each n outputs and PAD sentinels; inplace: y16 starts as the residual and is passed as both"""
    from usdm_amd import ops
    dev = W.device
    y16 = None if y32_only else torch.full((n + PAD,), FILL, dtype=BF, device=dev)
    y32 = torch.full((n + PAD,), FILL, device=dev)
    if inplace:
        y16[:n] = res
        res = y16
    ops.gemv(W, x, N=n, K=K, ldw=ldw, round_bf16=rbf, residual=res, y16=y16, y32=y32, skip=skip, resident=resident, wpack=wp)
    torch.cuda.synchronize()
    for y in (y16, y32):
        assert y is None or bool(y[n:].isnan().all()), "written beyond N"
    return y16, y32


def _same(a, b):
    return all(p is None and q is None or torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _pack(W, n):
    from usdm_amd import _lib, ops, wpack
    p = wpack.PackedWeight.from_matrix(W[:, :K].contiguous())
    assert p.marked_rows == sorted(MARKED[n]), "the flag array: exactly the planted rows stream bf16, every other row the image"
    bits = list(p.args().marked)
    assert [r for r in range(32 * len(bits)) if bits[r >> 5] >> (r & 31) & 1] == sorted(MARKED[n])
    a = ops.gemv(W, W[0], N=n, K=K, ldw=W.shape[1], y32=torch.empty(1, device=W.device), only_args=True, resident=1)
    assert _lib.lib.usdm_gemv_packs(ctypes.byref(a)) == 1        # the launch really takes the packed form
    return p


@pytest.fixture(scope="module")
def random_cases(dev):
    """{(N, ldw): (W, x, residual)}, made once and never changed"""
    gen = torch.Generator().manual_seed(13)
    out = {}
    for n in MARKED:
        for ldw in LDWS:
            W = torch.full((n, ldw), 7.0)
            W[:, :K] = torch.randn((n, K), generator=gen) * K ** -0.5
            W = W.to(BF)
            W[W.abs() < 2.0 ** -20] = 2.0 ** -9       # (the draw's own zeros and tiny weights: only the planted rows are marked)
            for i, r in enumerate(MARKED[n]):
                W[r, (997 * i + 511 * r) % K] = 0.0 if i % 2 else -0.0
            out[n, ldw] = (W.to(dev), torch.randn(K, generator=gen).to(BF).to(dev), torch.randn(n, generator=gen).to(BF).to(dev))
    return out


@pytest.mark.parametrize("ldw", LDWS)
@pytest.mark.parametrize("n", sorted(MARKED))
def test_packed_equals_the_bf16_forms(dev, random_cases, n, ldw):
    W, x, res = random_cases[n, ldw]
    wp = _pack(W, n)
    skip = torch.ones(1, dtype=torch.int32, device=dev)
    variants = [dict(), dict(res=res), dict(res=res, rbf=False), dict(rbf=False), dict(res=res, y32_only=True), dict(y32_only=True)]
    for kw in variants:
        p = _launch(W, x, n, ldw, 1, wp, **kw)
        for r in (1, -1):
            assert _same(_launch(W, x, n, ldw, r, **kw), p), (n, ldw, kw, r)
        assert not bool(p[1][:n].isnan().any()) and float(p[1][:n].abs().max()) > 0
        y16, y32 = _launch(W, x, n, ldw, 1, wp, skip=skip, **kw)
        assert bool(y32.isnan().all()) and (y16 is None or bool(y16.isnan().all())), (n, ldw, kw, "written although *skip = 1")
    # the in-place form of the step: residual and y16 are one array
    a = _launch(W, x, n, ldw, -1, res=res)
    assert _same(a, _launch(W, x, n, ldw, 1, wp, res=res, inplace=True)), (n, ldw)
    y16, y32 = _launch(W, x, n, ldw, 1, wp, res=res, inplace=True, skip=skip)
    assert torch.equal(_bits(y16[:n]), _bits(res)) and bool(y32.isnan().all())
    # a call without a packed form (gemv_kernel asked for) is usdm_gemv itself
    assert _same(a, _launch(W, x, n, ldw, -1, wp, res=res))


def _integer_case(n, seed, dev):
    """x in +-{1, 2} with period K / 2; W in +-{1, 2} (no zero: zeros are outside the window) with W[o][k + K/2] = -W[o][k], so a
    row sums to 0, then |t(o)| pairs at places where |x| = 1 are set to (2 s, -s) in units of x's sign, s = sign t(o): each adds s,
    the row sums to t(o) in +-[1, 127], a value that depends on o.  Every partial sum is an integer below 2^24, exact in f32 in any
    order, and t(o) + residual (integers in [-8, 8]) is exact in bf16.  The marked rows get zeros in both halves of some pairs
    (x K/2 apart is equal, so the sum stays).  A lost or repeated K iteration, a nibble, sign or low byte taken from another
    weight, or a row of another workgroup changes the integer."""
    gen = torch.Generator().manual_seed(seed)
    h = K // 2
    sgn = torch.randint(0, 2, (h,), generator=gen).double() * 2 - 1
    mag = torch.randint(1, 3, (h,), generator=gen).double()
    xp = (sgn * mag).repeat(2)
    o = torch.arange(n)
    target = ((o * 37) % 127 + 1).double() * (1 - 2 * ((o // 2) % 2)).double()
    ones = (mag == 1).nonzero().flatten()
    half = (torch.randint(0, 2, (n, h), generator=gen).double() * 2 - 1) * torch.randint(1, 3, (n, h), generator=gen).double()
    W = torch.cat((half, -half), dim=1)
    for r in range(n):
        t = int(target[r])
        perm = ones[torch.randperm(ones.numel(), generator=gen)]
        at, zero = perm[:abs(t)], perm[abs(t):abs(t) + 3]
        s = 1.0 if t > 0 else -1.0
        W[r, at] = 2 * s * sgn[at]
        W[r, at + h] = -s * sgn[at]
        if r in MARKED[n]:
            W[r, zero] = 0.0
            W[r, zero + h] = 0.0
    assert torch.equal(W @ xp, target)
    res = torch.randint(-8, 9, (n,), generator=gen).double()
    return W.to(BF).to(dev), xp.to(BF).to(dev), res.to(BF).to(dev), target, res


@pytest.mark.parametrize("n", sorted(MARKED))
def test_packed_exact_integers(dev, n):
    W, x, res, target, resd = _integer_case(n, 900 + n, dev)
    wp = _pack(W, n)
    for rbf in (False, True):
        y16, y32 = _launch(W, x, n, K, 1, wp, rbf=rbf)
        assert torch.equal(y32[:n].cpu().double(), target) and torch.equal(y16[:n].cpu().double(), target), (n, rbf)
        y16, y32 = _launch(W, x, n, K, 1, wp, res=res, rbf=rbf)
        assert torch.equal(y32[:n].cpu().double(), target + resd) and torch.equal(y16[:n].cpu().double(), target + resd), (n, rbf)
    y16, y32 = _launch(W, x, n, K, 1, wp, res=res, inplace=True)
    assert torch.equal(y16[:n].cpu().double(), target + resd) and torch.equal(y32[:n].cpu().double(), target + resd), n


def test_packed_default_on_the_7b_shape(dev):
    """down_proj of the 7B under the launcher's own choice, random weights made on the device (whatever rows the draw marks)"""
    from usdm_amd import wpack
    n = 4096
    gen = torch.Generator(device=dev).manual_seed(7)
    W = (torch.randn((n, K), generator=gen, device=dev) * K ** -0.5).to(BF)
    x = torch.randn(K, generator=gen, device=dev).to(BF)
    res = torch.randn(n, generator=gen, device=dev).to(BF)
    wp = wpack.PackedWeight.from_matrix(W)
    print(f"marked rows of the random 4096 x 14336 matrix: {wp.marked_rows}; image {wp.nbytes} bytes against {2 * n * K}")
    assert len(wp.marked_rows) < 64 and wp.planes.shape == (n, 7 * 3328)
    a = _launch(W, x, n, K, -1, res=res)
    assert _same(a, _launch(W, x, n, K, 0, wp, res=res)) and _same(a, _launch(W, x, n, K, 0, res=res))
    assert float(a[1][:n].abs().max()) > 0 and not bool(a[1][:n].isnan().any())
