"""The resident multi-tile form of the SwiGLU decode GEMV (csrc/llm_k.hip gemv_resident_kernel; usdm_gemv_args.resident) against
the one-tile form and against an exact integer reference.  Every comparison is == on the raw bf16 / f32 bits.

A tile is 14 outputs (7 waves x 2).  usdm_gemv requires N % 32 == 0 under SwiGLU (the packed layout has whole blocks of 16 gate +
16 up rows), so the number of outputs is a multiple of 16 and never 14, 28, 42, 70 or 73: the shapes here are the multiples of 16
that give the same situations - 16, 32, 48, 80 outputs = 2, 3, 4, 6 tiles whose last one is ragged (2, 4, 6, 10 outputs), 112 and
224 outputs = 8 and 16 whole tiles.  The grid caps 1, 2, 3, 4, 5, 8 give workgroups with 1, 2, 3 and more tiles, workgroups with
one tile more than others (3 tiles on 2, 4 on 3, 6 on 4 or 5, 8 on 3 or 5, 16 on 3 or 5), and - K = 4096, tiles = 2 x grid - the
straight-line instantiation the 7B's gate/up runs (8 tiles on 4, 16 on 8); every other combination runs the generic one.  A cap
that is not below the number of tiles leaves the launch to the one-tile kernel.
K = 512 and 1024 are below one weight ring (1 and 2 of its 4 slots in use), 4096 is two rings, 4096 + 8 has a ninth iteration that
only lane 0 is inside."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NOUTS = (16, 32, 48, 80, 112, 224)
KS = (512, 1024, 4096, 4096 + 8)
CAPS = (1, 2, 3, 4, 5, 8)
EPS = 1e-5


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _launch(W, x, g, nout, K, resident, skip=None, y16=None, y32=None):
    from usdm_amd import ops
    dev = W.device
    y16 = torch.full((nout,), -3.0, dtype=BF, device=dev) if y16 is None else y16
    y32 = torch.full((nout,), -3.0, device=dev) if y32 is None else y32
    ops.gemv(W, x, N=2 * nout, K=K, norm_w=g, eps=EPS, act=3, round_bf16=True, y16=y16, y32=y32, skip=skip, resident=resident)
    return y16, y32


def _random_case(nout, K, seed, dev):
    from usdm_amd.llm import _pack_gate_up
    gen = torch.Generator().manual_seed(seed)
    Wg, Wu = (torch.randn((nout, K), generator=gen) * K ** -0.5).to(BF), (torch.randn((nout, K), generator=gen) * K ** -0.5).to(BF)
    x = torch.randn(K, generator=gen).to(BF)
    g = 1.0 + 0.1 * torch.randn(K, generator=gen)
    return _pack_gate_up(Wg, Wu).to(dev), x.to(dev), g.to(dev)


def _integer_case(nout, K, seed, dev):
    """x = +-2 and eps = 1e-5 give bf16(x rstd) = +-1 (rstd is within 2^-11 of 1/2), so the normalised input is +-norm_w with norm_w
    in {1, 2}: integers.  W has entries in {-1, 0, 1}, about K / 16 of them random and the rest placed so that gate row o sums to
    32 or 64 and up row o to an integer u(o) in +-[1, 127] that depends on o: every partial sum is an integer below 2^24, exact in
    f32 in any order.  At g >= 32, 1 + exp(-g) = 1 in f32, so silu(g) = g and the output is g u(o) <= 64 x 127, exact in bf16.
    A row read from the wrong tile, a lost or repeated K iteration or a wrong norm weight changes the integer."""
    from usdm_amd.llm import _pack_gate_up
    gen = torch.Generator().manual_seed(seed)
    sgn = torch.randint(0, 2, (K,), generator=gen).double() * 2 - 1
    nw = torch.randint(1, 3, (K,), generator=gen).double()
    xp = sgn * nw                                               # the normalised input
    o = torch.arange(nout)
    tg = 32.0 * (1 + (o % 2)).double()
    tu = ((o * 37) % 127 + 1).double() * (1 - 2 * ((o // 2) % 2)).double()
    ones = (nw == 1).nonzero().flatten()

    def rows(target):
        W = (torch.rand((nout, K), generator=gen) < 1 / 16).double() * (torch.randint(0, 2, (nout, K), generator=gen).double() * 2 - 1)
        for r in range(nout):
            d = int(target[r] - W[r] @ xp)
            free = ones[W[r, ones] == 0]
            at = free[torch.randperm(free.numel(), generator=gen)[:abs(d)]]
            assert at.numel() == abs(d)
            W[r, at] = sgn[at] * (1 if d > 0 else -1)           # each adds +-1 to the row's sum
        assert torch.equal(W @ xp, target)
        return W.to(BF)

    Wp = _pack_gate_up(rows(tg), rows(tu))
    return Wp.to(dev), (2 * sgn).to(BF).to(dev), nw.float().to(dev), tg * tu


@pytest.mark.parametrize("K", KS)
def test_resident_equals_one_tile_form(dev, K):
    for i, nout in enumerate(NOUTS):
        W, x, g = _random_case(nout, K, 100 + i, dev)
        a16, a32 = _launch(W, x, g, nout, K, -1)
        assert a32.abs().max() > 0 and not (a32 == -3.0).any()
        for cap in CAPS:
            b16, b32 = _launch(W, x, g, nout, K, cap)
            assert torch.equal(_bits(b16), _bits(a16)) and torch.equal(_bits(b32), _bits(a32)), (nout, K, cap)


@pytest.mark.parametrize("K", KS)
def test_resident_exact_integers(dev, K):
    for i, nout in enumerate(NOUTS):
        W, x, g, ref = _integer_case(nout, K, 200 + i, dev)
        for res in (-1,) + CAPS:
            y16, y32 = _launch(W, x, g, nout, K, res)
            assert torch.equal(y32.cpu().double(), ref) and torch.equal(y16.cpu().double(), ref), (nout, K, res)


def test_resident_default_on_the_7b_shape(dev):
    """gate/up of the 7B, the launcher's own choice (resident on as many workgroups as the device holds) against one tile each"""
    nout, K = 14336, 4096
    gen = torch.Generator(device=dev).manual_seed(7)
    W = (torch.randn((2 * nout, K), generator=gen, device=dev) * K ** -0.5).to(BF)
    x = torch.randn(K, generator=gen, device=dev).to(BF)
    g = 1.0 + 0.1 * torch.randn(K, generator=gen, device=dev)
    a16, a32 = _launch(W, x, g, nout, K, -1)
    for res in (0, 512, 300):      # the default; the straight-line form whatever the device holds; an uneven split
        b16, b32 = _launch(W, x, g, nout, K, res)
        assert torch.equal(_bits(b16), _bits(a16)) and torch.equal(_bits(b32), _bits(a32)), res
    assert a32.abs().max() > 0


def test_resident_skip_word_writes_nothing(dev):
    skip = torch.ones(1, dtype=torch.int32, device=dev)
    for nout, K, cap in ((80, 1024, 2), (112, 4096, 4), (48, 4104, 1)):
        W, x, g = _random_case(nout, K, 300, dev)
        y16, y32 = _launch(W, x, g, nout, K, cap, skip=skip)
        assert (y16 == -3.0).all() and (y32 == -3.0).all()


def test_resident_replay_is_identical(dev):
    for nout, K, cap in ((80, 1024, 2), (112, 4096, 4), (224, 4096, 5), (48, 4104, 1)):
        W, x, g = _random_case(nout, K, 400, dev)
        y16, y32 = _launch(W, x, g, nout, K, cap)
        first = (y16.clone(), y32.clone())
        for _ in range(2):
            _launch(W, x, g, nout, K, cap, y16=y16, y32=y32)
            assert torch.equal(_bits(y16), _bits(first[0])) and torch.equal(_bits(y32), _bits(first[1]))


def test_generate_resident_on_and_off(dev, monkeypatch):
    """16 greedy tokens of the small random-init model (1024 gate/up outputs = 73 tiles and a ragged one, K = 512) with every
    gate/up launch in the one-tile form and resident on 20 workgroups (3 or 4 tiles each)"""
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                 num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
    sd = MO.random_state_dict(SMALL, seed=11)
    ids = torch.randint(0, SMALL["vocab_size"], (1, 23), generator=torch.Generator().manual_seed(3)).to(dev)
    out = {}
    for res in ("-1", "20"):
        monkeypatch.setenv("USDM_GEMV_RESIDENT", res)
        out[res] = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128).generate(input_ids=ids, max_new_tokens=16)
    assert out["-1"].shape[1] == 23 + 16 and torch.equal(out["-1"], out["20"])
