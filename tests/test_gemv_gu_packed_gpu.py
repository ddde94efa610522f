"""The gate/up decode GEMV over the lossless 13-bit weight image (usdm_gemv_packed_glu; csrc/llm_k.hip gemv_resident_wpack_kernel)
against the same call without the image - the straight-line resident bf16 form (resident = the cap) and the one-tile form
(resident = -1) - and against an exact integer reference.  Every comparison is == on the raw bf16 / f32 bits; outputs carry
sentinel padding.

The packed form exists where the bf16 launcher runs its straight-line instantiation: K = 4096 and two tiles (of 14 outputs) on
every workgroup.  The smallest such shapes are those of tests/test_gemv_resident_gpu.py: 112 outputs on 4 workgroups and 224 on 8
(workgroup b owns the tiles b and b + grid; wave w of a tile owns its outputs 2 w and 2 w + 1).  80 outputs on 3 workgroups is
the same form with a ragged last tile (rows past N are re-read, never stored).  Zeros are planted so that one launch holds both
paths of the kernel: an output marked through its gate row only (output 0: a wave marked in tile 0 only), one through its up row
only (the last output: a wave marked in tile 1 only), and a workgroup - number 1 - whose seven waves are all marked, through
either tile in turn; every other wave streams the image."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K = 4096
EPS = 1e-5
PAD = 64
FILL = float("nan")
CAP = {112: 4, 224: 8, 80: 3}


def _planted(nout):
    """{output: up?}: output 0 through its gate row, the last through its up row, workgroup 1 whole (tiles 1 and 1 + grid)"""
    grid = CAP[nout]
    m = {0: False, nout - 1: True}
    for w in range(7):
        o = 14 * (1 + grid * (w % 2)) + 2 * w + (w % 2)      # even waves in the first tile, odd waves in the second
        m[o] = bool(w % 3 == 0)
    return m


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return all(p is None and q is None or torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _launch(W, x, g, nout, resident, wp=None, outs="both", rbf=True, skip=None, k=K):
    """-> (y16 or None, y32 or None), each nout outputs and PAD sentinels"""
    from usdm_amd import ops
    dev = W.device
    y16 = torch.full((nout + PAD,), FILL, dtype=BF, device=dev) if outs in ("both", "y16") else None
    y32 = torch.full((nout + PAD,), FILL, device=dev) if outs in ("both", "y32") else None
    ops.gemv(W, x, N=2 * nout, K=k, ldw=W.shape[1], norm_w=g, eps=EPS, act=3, round_bf16=rbf, y16=y16, y32=y32, skip=skip,
             resident=resident, wpack=wp)
    torch.cuda.synchronize()
    for y in (y16, y32):
        assert y is None or bool(y[nout:].isnan().all()), "written beyond the outputs"
    return y16, y32


def _packs(W, nout, resident, k=K, **kw):
    from usdm_amd import _lib, ops
    a = ops.gemv(W, W[0], N=2 * nout, K=k, ldw=W.shape[1], act=3, y32=torch.empty(1, device=W.device), only_args=True,
                 resident=resident, **kw)
    return _lib.lib.usdm_gemv_packs_glu(ctypes.byref(a))


def _pack(W, nout):
    """the image; its bitmap is exactly the planted outputs and the launch really takes the packed form"""
    from usdm_amd import wpack
    p = wpack.PackedWeight.from_matrix(W[:, :K].contiguous(), glu=True)
    want = _planted(nout)
    assert p.marked_rows == sorted(wpack.glu_row(o, up) for o, up in want.items())
    bits = list(p.args().marked)
    assert [o for o in range(32 * len(bits)) if bits[o >> 5] >> (o & 31) & 1] == sorted(want) == p.marked_outputs
    assert _packs(W, nout, CAP[nout]) == 1
    return p


def _plant(W, nout):
    from usdm_amd import wpack
    for i, (o, up) in enumerate(sorted(_planted(nout).items())):
        W[wpack.glu_row(o, up), (997 * i + 511 * o) % K] = 0.0 if i % 2 else -0.0
    return W


@pytest.fixture(scope="module")
def random_cases(dev):
    """{nout: (W, x, norm_w)}, made once and never changed"""
    from usdm_amd.llm import _pack_gate_up
    gen = torch.Generator().manual_seed(29)
    out = {}
    for nout in CAP:
        Wg, Wu = ((torch.randn((nout, K), generator=gen) * K ** -0.5).to(BF) for _ in range(2))
        W = _pack_gate_up(Wg, Wu)
        W[W.abs() < 2.0 ** -20] = 2.0 ** -9       # (the draw's own zeros and tiny weights: only the planted rows are marked)
        x = torch.randn(K, generator=gen).to(BF)
        g = 1.0 + 0.1 * torch.randn(K, generator=gen)
        out[nout] = (_plant(W, nout).to(dev), x.to(dev), g.to(dev))
    return out


@pytest.mark.parametrize("nout", sorted(CAP))
def test_packed_equals_the_bf16_forms(dev, random_cases, nout):
    W, x, g = random_cases[nout]
    wp = _pack(W, nout)
    skip = torch.ones(1, dtype=torch.int32, device=dev)
    for norm in (g, None):
        for outs in ("both", "y16", "y32"):
            for rbf in (True, False):
                kw = dict(outs=outs, rbf=rbf)
                p = _launch(W, x, norm, nout, CAP[nout], wp, **kw)
                for r in (CAP[nout], -1):
                    assert _same(_launch(W, x, norm, nout, r, **kw), p), (nout, norm is not None, kw, r)
                y = next(v for v in p if v is not None)[:nout].float()
                assert not bool(y.isnan().any()) and float(y.abs().max()) > 0
                s16, s32 = _launch(W, x, norm, nout, CAP[nout], wp, skip=skip, **kw)
                assert all(v is None or bool(v.isnan().all()) for v in (s16, s32)), (nout, kw, "written although *skip = 1")


def test_calls_without_a_packed_form_are_usdm_gemv(dev, random_cases):
    W, x, g = random_cases[112]
    wp = _pack(W, 112)
    # the one-tile form asked for; a cap that is not half the tiles (generic resident form; every tile resident)
    for res in (-1, 3, 5, 8):
        assert _packs(W, 112, res) == 0
        assert _same(_launch(W, x, g, 112, res, wp), _launch(W, x, g, 112, res)), res
    assert _packs(W, 112, 4, x_delta=torch.zeros(K, device=dev), x_out=torch.empty(K, dtype=BF, device=dev)) == 0
    # 80 outputs = 6 tiles: no packed form on 4 or 8 workgroups
    W80, x80, g80 = random_cases[80]
    wp80 = _pack(W80, 80)
    for res in (4, 8, -1):
        assert _packs(W80, 80, res) == 0
        assert _same(_launch(W80, x80, g80, 80, res, wp80), _launch(W80, x80, g80, 80, res)), res
    # K = 512: one K iteration, never the straight-line form (the image of another K is not looked at)
    assert _packs(W, 112, 4, k=512) == 0
    assert _same(_launch(W, x[:512], g[:512], 112, 4, wp, k=512), _launch(W, x[:512], g[:512], 112, 4, k=512))


def _integer_case(nout, seed, dev):
    """x = +-2 and eps = 1e-5 give bf16(x rstd) = +-1, so the normalised input is xp = +-norm_w with norm_w in {1, 2}, of period
    K / 2.  W in +-{1, 2} (no zero: zeros are outside the window) with W[r][k + K/2] = -W[r][k], so a row sums to 0; then |t|
    pairs at places where |xp| = 1 are set to (2 s, -s) in units of xp's sign, s = sign t: each adds s.  Gate row o sums to 32 or
    64 (silu(g) = g in f32), up row o to u(o) in +-[1, 127], a value that depends on o; every partial sum is an integer below 2^24
    and the output g u(o) <= 64 x 127 is exact in bf16.  The planted rows get zeros in both halves of three pairs (the sum stays).
    A unit, nibble, sign or low byte taken from another weight, row or tile changes the integer."""
    from usdm_amd import wpack
    from usdm_amd.llm import _pack_gate_up
    gen = torch.Generator().manual_seed(seed)
    h = K // 2
    sgn = torch.randint(0, 2, (h,), generator=gen).double() * 2 - 1
    nw = torch.randint(1, 3, (h,), generator=gen).double()
    xp = (sgn * nw).repeat(2)
    o = torch.arange(nout)
    tg = 32.0 * (1 + (o % 2)).double()
    tu = ((o * 37) % 127 + 1).double() * (1 - 2 * ((o // 2) % 2)).double()
    ones = (nw == 1).nonzero().flatten()
    zero_rows = {wpack.glu_row(oo, up): None for oo, up in _planted(nout).items()}

    def rows(target, up):
        half = (torch.randint(0, 2, (nout, h), generator=gen).double() * 2 - 1) * torch.randint(1, 3, (nout, h), generator=gen).double()
        W = torch.cat((half, -half), dim=1)
        for r in range(nout):
            t = int(target[r])
            perm = ones[torch.randperm(ones.numel(), generator=gen)]
            at, zero = perm[:abs(t)], perm[abs(t):abs(t) + 3]
            s = 1.0 if t > 0 else -1.0
            W[r, at] = 2 * s * sgn[at]
            W[r, at + h] = -s * sgn[at]
            if wpack.glu_row(r, up) in zero_rows:
                W[r, zero] = 0.0
                W[r, zero + h] = 0.0
        assert torch.equal(W @ xp, target)
        return W.to(BF)

    Wp = _pack_gate_up(rows(tg, False), rows(tu, True))
    return Wp.to(dev), (2 * sgn).repeat(2).to(BF).to(dev), nw.repeat(2).float().to(dev), tg * tu


@pytest.mark.parametrize("nout", sorted(CAP))
def test_packed_exact_integers(dev, nout):
    W, x, g, ref = _integer_case(nout, 700 + nout, dev)
    wp = _pack(W, nout)
    for res, p in ((CAP[nout], wp), (CAP[nout], None), (-1, None)):
        y16, y32 = _launch(W, x, g, nout, res, p)
        assert torch.equal(y32[:nout].cpu().double(), ref) and torch.equal(y16[:nout].cpu().double(), ref), (nout, res, p is not None)


def test_packed_default_on_the_7b_shape(dev):
    """gate/up of the 7B under the launcher's own choice, random weights made on the device (whatever outputs the draw marks)"""
    from usdm_amd import wpack
    nout = 14336
    gen = torch.Generator(device=dev).manual_seed(7)
    W = (torch.randn((2 * nout, K), generator=gen, device=dev) * K ** -0.5).to(BF)
    x = torch.randn(K, generator=gen, device=dev).to(BF)
    g = 1.0 + 0.1 * torch.randn(K, generator=gen, device=dev)
    wp = wpack.PackedWeight.from_matrix(W, glu=True)
    print(f"marked outputs of the random 28672 x 4096 matrix: {len(wp.marked_outputs)} of {nout} ({len(wp.marked_rows)} rows); "
          f"image {wp.nbytes} bytes against {4 * nout * K}")
    assert len(wp.marked_outputs) < 256 and wp.planes.shape == (2 * nout, 2 * 3328)
    assert _packs(W, nout, 0) == 1
    a = _launch(W, x, g, nout, -1)
    assert _same(a, _launch(W, x, g, nout, 0, wp)) and _same(a, _launch(W, x, g, nout, 0))
    assert float(a[1][:nout].abs().max()) > 0 and not bool(a[1][:nout].isnan().any())
