"""GPU: the MXFP4-weight matrix-core form (usdm_gemv_mxfp4_mfma, opt-in `mxfp4_matrix_cores=True`).  Every dequantized weight
W' = e2m1(code) * 2^s is a bf16 value and the kernel changes only the weight load and unpack, so it must equal the bf16 matrix-core
form (usdm_gemv_batch form 1 / 5) on W' BIT FOR BIT - kernel by kernel; independently of that kernel it must hold the exact integer
reference of tests/_gemv_reference.py; and the MXFP4 model with the flag must equal a bf16 model loaded from W' (lm_head: the fp8 W')
token for token in generate_batch, serving and speculative decoding."""
import ctypes as C

import pytest
import torch

from tests import _gemv_reference as R
from tests.test_fp8_gpu import SMALL
from tests.test_gemv_exact_gpu import Run, _run_all, run_case
from tests.test_mxfp4_gpu import _wprime

pytestmark = pytest.mark.gpu

NBS = (1, 5, 8, 13, 16)
SHAPES = [  # (name, N, K, mode, form, ks): the 7B decode projections, down_proj split and unsplit, then the generic forms
    ("qkv", 6144, 4096, "norm", 0, False), ("o", 4096, 4096, "res", 0, False), ("gu", 28672, 4096, "glu", 0, False),
    ("down_ks", 4096, 14336, "res", 0, True), ("down_f5", 4096, 14336, "res", 5, False),
    ("k512", 1003, 512, "norm", 0, False),          # 2 chunks per wave: the dword path, N % 16 != 0
    ("glu512", 96, 512, "glu", 0, False), ("glu1024", 96, 1024, "glu", 0, False),       # ... and one quad per wave
    ("k1024", 512, 1024, "res", 0, False), ("odd", 37, 1792, "res", 0, False),          # 7 chunks per wave
    ("stream6k", 200, 6144, "res", 5, False),       # streamed activations, 24 chunks per wave
    ("ks6k", 200, 6144, "res", 0, True)]            # a three-slice split


def _weights(N, K, seed, dev):
    """a [N][K] bf16 matrix whose block scales are spread over 2^-12 .. 2^12 from block to block (a scale taken from a neighbouring
    chunk of the quad, or a piece from a neighbouring lane, shows), two rows scaled by 40 and 1e-3; its Mxfp4Weight with both images"""
    from usdm_amd.quant import Mxfp4Weight
    g = torch.Generator(device=dev).manual_seed(seed)
    W = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
    W *= torch.exp2(torch.randint(-12, 13, (N, K // 32), device=dev, generator=g).float()).repeat_interleave(32, dim=1)
    W[3 % N] *= 40.0
    W[5 % N] *= 1e-3
    Wq = Mxfp4Weight.from_matrix(W.to(torch.bfloat16), matrix_cores=True)
    return Wq, Wq.dequantize()


@pytest.mark.parametrize("name,N,K,mode,form,use_ks", SHAPES)
def test_mxfp4_mfma_bit_identical_to_bf16_matrix_cores_on_dequantized_weights(dev, name, N, K, mode, form, use_ks):
    from usdm_amd import ops
    bf = torch.bfloat16
    seed = sum(map(ord, name))
    Wq, Wd = _weights(N, K, seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    X = torch.randn(16, K, device=dev, generator=g).to(bf)
    R_ = torch.randn(16, N, device=dev, generator=g).to(bf)
    nw = (1 + 0.1 * torch.randn(K, device=dev, generator=g)).float()
    nout = N // 2 if mode == "glu" else N
    kw = dict(norm_w=nw, eps=1e-5) if mode == "norm" else dict(act=3) if mode == "glu" else {}
    ks = ks2 = None
    if use_ks:
        ksf = ops.gemv_batch_ks_floats(N, K)
        assert ksf > 0
        ks = (torch.zeros(ksf, device=dev), torch.zeros(-(-N // 16), dtype=torch.int32, device=dev))
        ks2 = (torch.zeros(ksf, device=dev), torch.zeros(-(-N // 16), dtype=torch.int32, device=dev))

    def run(fn, W, nb, ksa, f):
        y = R_[:nb].clone() if mode == "res" else torch.zeros(nb, nout, dtype=bf, device=dev)
        fn(W, X, nb=nb, N=N, K=K, x_bs=K, y_bs=nout, res_bs=N, residual=y if mode == "res" else None, y16=y, form=f, ks=ksa, **kw)
        return y

    for nb in NBS:
        got = run(ops.gemv_mxfp4_mfma, Wq, nb, ks, form)
        ref = run(ops.gemv_batch, Wd, nb, ks2, 1 if form == 0 else form)
        assert torch.equal(got, ref), (name, nb, int((got != ref).sum()))
        if use_ks:
            assert int(ks[1].abs().sum()) == 0, "tile counters not back at zero"
    # float64 sanity bound on sequence 0 (the scales are applied the right way round), per output row.  The block scales differ by up
    # to 2^24 inside a row, so a row's sum is far smaller than its largest terms and a bound relative to max |y| (the FP8 test's, whose
    # scales are per row) does not hold for ANY kernel: one bf16 rounding of x' moves a term of 6e4 by 1e2.  The bound here is relative
    # to S = sum_k |W'| |x'| of the row.  x' carries two bf16 roundings (2 x 2^-9 of each term, fused RMSNorm only); the f32
    # accumulation at most K 2^-24 <= 2^-10 of S; the bf16 rounding of the sum 2^-9 |sum| <= 2^-9 S; the rounding after the residual
    # 2^-9 |y|.  Together below 2^-7 S (norm) / 2^-8 S (residual) + 2^-8 |y|.  A scale or a piece from the wrong place is an error
    # of the order of S itself.
    if mode in ("res", "norm"):
        x = X[0].double()
        if mode == "norm":
            x = x * torch.rsqrt(x.pow(2).mean() + 1e-5) * nw.double()
        y64 = Wd.double() @ x + (R_[0].double() if mode == "res" else 0)
        S = Wd.double().abs() @ x.abs()
        err = (got[0].double() - y64).abs()
        tol = (2.0 ** -7 if mode == "norm" else 2.0 ** -8) * S + 2.0 ** -8 * y64.abs() + 1e-3
        print(f"[mxfp4 mfma] {name}: worst error / bound {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), name


# ---- the exact integer reference (tests/_gemv_reference.py), independent of the bf16 kernel ----------------------------------------
GAP = 0xFF      # the fill of every gap: a scale byte 0xFF is the e8m0 NaN; a code byte 0xFF is two codes -6 under whatever scale follows


def _guarded_image(W):
    """The matrix-core image of W again, in buffers with a gap after every row (16 code bytes, 4 scale bytes) and one more row, all
    bytes 0xFF: a read past a row's K / 2 code bytes or K / 32 scale bytes, or past the last row, gives NaN or a wrong sum."""
    from usdm_amd.quant import Mxfp4Weight
    N, K = W.N, W.K
    cb = torch.full((N + 1, K // 2 + 16), GAP, dtype=torch.uint8, device=W.mq.device)
    sb = torch.full((N + 1, K // 32 + 4), GAP, dtype=torch.uint8, device=W.mq.device)
    cb[:N, :K // 2], sb[:N, :K // 32] = W.mq, W.ms
    return Mxfp4Weight(W.q, W.s, K, cb[:N, :K // 2], sb[:N, :K // 32])


class McRun(Run):
    """a matrix-core case of the reference with MXFP4 weights: the case is built as its FP8 twin (the reference has no MXFP4 cases on
    the matrix cores) and then given per-block weight exponents; launches go to usdm_gemv_mxfp4_mfma"""

    def __init__(self, c, dev):
        super().__init__(c, dev)
        self.W = _guarded_image(self.W.with_matrix_core_image())
        self.gaps = (self.W.mq.storage_offset(), self.W.ms.storage_offset())

    def launch(self, rbf, names, alt=False, inplace=False):
        from usdm_amd import ops
        c, dev = self.c, self.dev
        assert names == ["y16"]
        out = {"y16": (R.alt_sentinel if alt else R.sentinel)((self.sizes()["y16"],), R.BF, dev)}
        res = self.res
        if inplace:
            out["y16"].view(c.B + 1, c.y_bs)[:c.B, :c.nout] = self.d.rl.to(R.BF).to(dev)
            res = out["y16"]
        ops.gemv_mxfp4_mfma(self.W, self.x, N=c.N, K=c.K, norm_w=self.norm_w, eps=R.EPS, act=c.act, round_bf16=rbf, residual=res, y16=out["y16"],
                            nb=c.nb, x_bs=c.x_bs, y_bs=c.y_bs, res_bs=c.res_bs, ks=self.ks, form=c.form)
        torch.cuda.synchronize()
        if c.ks:
            part, cnt = self.ks[0].cpu(), self.ks[1].cpu()
            assert int(cnt[:self.nt16].abs().sum()) == 0, f"{c.name}: tile counters not back at zero"
            assert bool(R.is_sentinel(cnt[self.nt16:]).all()) and bool(R.is_sentinel(part[self.ksf:]).all()), f"{c.name}: written past the K-split scratch"
        return {"y16": out["y16"].cpu()}


def _mc_cases(cases):
    out = []
    for c in cases:
        if c.lm_head:
            continue
        c.fmt, c.name = "mxfp4", c.name.replace("fp8 ", "mxfp4 ")
        out.append(c)
    return out


def _run_mc(cases, dev, what):
    _run_all(_mc_cases(cases), dev, what, run=lambda c, dev: run_case(c, dev, McRun(c, dev)))


@pytest.mark.parametrize("nb", (5, 16))
def test_mxfp4_mfma_exact_ladder(dev, nb):
    """N = 37 over held and streamed activations, K = 4096 and 14336, the K split in 3, 7 and 8 slices (counters back at zero, the same
    bits on the same scratch); plain + residual, in place in the round_bf16 launch; sentinels around every output"""
    _run_mc(R.mfma_ladder_cases(nb, "fp8"), dev, "")


@pytest.mark.parametrize("nb", (5, 16))
def test_mxfp4_mfma_exact_tile_rows(dev, nb):
    """12-row tiles (N = 6144) and ragged 16-row tiles (N = 4085) on forms 0 and 5; N = 37 above runs 8-row tiles"""
    _run_mc(R.mfma_tile_cases(nb, "fp8"), dev, "")


@pytest.mark.parametrize("nb", (5, 16))
def test_mxfp4_mfma_exact_swiglu_and_norm(dev, nb):
    cases = R.mfma_swiglu_cases(nb, "fp8") + R.mfma_norm_cases(nb, "fp8")
    _run_mc([c for c in cases if c.kind != "probe"], dev, "SwiGLU error / bound")
    _run_mc([c for c in cases if c.kind == "probe"], dev, "share of the (1 + DELTA) reference")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_mxfp4_mfma_refusals(dev):
    from usdm_amd import ops
    from usdm_amd._lib import GemvMxfp4MfmaArgs, UsdmError, check, lib
    from usdm_amd.quant import Mxfp4Weight
    N, K = 256, 512
    Wq, Wd = _weights(N, K, 1, dev)
    x = torch.randn(17, K, device=dev).to(torch.bfloat16)
    y = torch.zeros(17, N, dtype=torch.bfloat16, device=dev)
    kw = dict(N=N, K=K, x_bs=K, y_bs=N, y16=y)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in (dict(nb=17), dict(nb=8, form=3), dict(nb=8, form=1), dict(nb=8, form=-1)):
        with pytest.raises(UsdmError):
            ops.gemv_mxfp4_mfma(Wq, x, **{**kw, **bad})
    with pytest.raises(UsdmError):        # K % 256
        Wk, _ = _weights(16, 384, 4, dev)
        ops.gemv_mxfp4_mfma(Wk, x, nb=8, N=16, K=384, x_bs=384, y_bs=16, y16=y)
    Wbig, _ = _weights(8, 8192, 2, dev)    # the fused RMSNorm with K > 4096
    xb = torch.randn(8, 8192, device=dev).to(torch.bfloat16)
    with pytest.raises(UsdmError):
        ops.gemv_mxfp4_mfma(Wbig, xb, nb=8, N=8, K=8192, x_bs=8192, y_bs=8, y16=y, norm_w=torch.ones(8192, device=dev))
    with pytest.raises(UsdmError):        # more than 64 tiles per workgroup: 256 x 64 x 16 rows + 1
        Wt, _ = _weights(256 * 64 * 16 + 16, 256, 3, dev)
        xs = torch.randn(8, 256, device=dev).to(torch.bfloat16)
        ops.gemv_mxfp4_mfma(Wt, xs, nb=8, N=Wt.N, K=256, x_bs=256, y_bs=Wt.N, y16=torch.zeros(8, Wt.N, dtype=torch.bfloat16, device=dev))
        del Wt

    def args(**fields):
        """the filled argument struct of a good call, then fields set directly (the checks run before anything is read)"""
        f = GemvMxfp4MfmaArgs()
        f.b = ops.gemv_batch(Wq, x, nb=8, only_args=True, **kw)
        f.codes, f.ldc, f.scales, f.lds = C.c_void_p(Wq.mq.data_ptr()), K // 2, C.c_void_p(Wq.ms.data_ptr()), K // 32
        for k, v in fields.items():
            setattr(f.b.g if hasattr(f.b.g, k) else f, k, v)
        return f

    check(lib.usdm_gemv_mxfp4_mfma(C.byref(args()), stream()), "the good call")
    dummy = C.c_void_p(y.data_ptr())
    # p2p / merged-attention input / hand-off / x_delta, the lm_head mode, misaligned pointers and strides, null pointers
    for bad in (dict(p2p=dummy), dict(p2p_mode=1), dict(mrg_po=dummy), dict(mrg_pm=dummy), dict(mrg_pl=dummy), dict(cmb_gran=dummy),
                dict(x_delta=dummy), dict(x_out=dummy), dict(part_val=dummy), dict(part_idx=dummy), dict(ban=dummy), dict(y32=dummy),
                dict(y16=C.c_void_p(0)), dict(codes=C.c_void_p(Wq.mq.data_ptr() + 4)), dict(scales=C.c_void_p(Wq.ms.data_ptr() + 2)),
                dict(x=C.c_void_p(x.data_ptr() + 8)), dict(ldc=K // 2 + 8), dict(ldc=K // 2 - 16), dict(lds=K // 32 + 2), dict(lds=K // 32 - 4),
                dict(codes=C.c_void_p(0)), dict(scales=C.c_void_p(0))):
        with pytest.raises(UsdmError):
            check(lib.usdm_gemv_mxfp4_mfma(C.byref(args(**bad)), stream()), str(bad))
    f = args()
    f.b.x_bs = K + 4                       # a stride of x that loses the 16-byte alignment
    with pytest.raises(UsdmError):
        check(lib.usdm_gemv_mxfp4_mfma(C.byref(f), stream()), "x_bs")
    for W in (Wd, Mxfp4Weight.from_matrix(Wd)):      # bf16 weights; an Mxfp4Weight without the matrix-core image
        with pytest.raises(TypeError):
            ops.gemv_mxfp4_mfma(W, x, nb=8, **kw)
    with pytest.raises(UsdmError):        # and the VALU entry point still stops at 4 sequences
        ops.gemv_batch(Wq, x, nb=8, **kw)
    torch.cuda.synchronize()


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _mc_pair(sd, cfg, dev, ctx_max=256):
    from usdm_amd.llm import USDMForCausalLM
    a = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, quantization="mxfp4", mxfp4_matrix_cores=True)
    b = USDMForCausalLM.from_state_dict(_wprime(sd), cfg, dev, ctx_max=ctx_max)
    return a, b


def test_mxfp4_matrix_cores_small_model(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=81)
    a, b = _mc_pair(sd, SMALL, dev)
    assert a.max_batch() == 16 and b.max_batch() == 16
    assert all(w[k].has_matrix_core_image for w in a.W["layers"] for k in ("qkv", "o", "gu", "down"))
    plain = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256, quantization="mxfp4")      # without the flag: as before
    assert plain.max_batch() == 4 and not any(w[k].has_matrix_core_image for w in plain.W["layers"] for k in ("qkv", "o", "gu", "down"))
    del plain
    g = torch.Generator().manual_seed(8)
    bad = [[i] for i in range(0, 300)]
    for n in (16, 11):
        prompts = [torch.randint(0, 1000, (1, int(L)), generator=g).to(dev) for L in torch.randint(10, 80, (n,), generator=g)]
        oa = a.generate_batch(prompts, 14, bad_words_ids=bad)
        ob = b.generate_batch(prompts, 14, bad_words_ids=bad)
        for i, (u, v) in enumerate(zip(oa, ob)):
            assert torch.equal(u, v), (n, i)
    assert 16 in a._batches and 11 in a._batches
    prompts = [torch.randint(0, 1000, (1, L), generator=g).to(dev) for L in (19, 33, 27)]
    for p, o in zip(prompts, a.generate_batch(prompts, 10)):     # a group of 3 keeps the VALU MXFP4 form: equal to generate()
        assert torch.equal(o, a.generate(input_ids=p, max_new_tokens=10))


def test_mxfp4_matrix_cores_full_width_two_layers(dev):
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=2)
    sd = MO.random_state_dict(cfg, seed=82)
    a, b = _mc_pair(sd, cfg, dev, ctx_max=1536)
    assert a.max_batch() == 16
    g = torch.Generator().manual_seed(10)
    prompts = [torch.randint(32002, cfg["vocab_size"], (int(L),), generator=g) for L in torch.randint(500, 621, (16,), generator=g)]
    bad = [[i] for i in range(32002)]                             # text -> unit: the lm_head skips the banned tiles
    new = 6
    oa = a.generate_batch([p[None].to(dev) for p in prompts], new, bad_words_ids=bad)
    ob = b.generate_batch([p[None].to(dev) for p in prompts], new, bad_words_ids=bad)
    for i, (u, v) in enumerate(zip(oa, ob)):
        assert torch.equal(u, v), i
    del b
    wp = _wprime(sd)
    for i in (0, 15):
        ref, ref_logits = MO.greedy_generate(wp, cfg, prompts[i], new, bad_words_ids=bad, return_logits=True)
        check_against_oracle(oa[i][0].tolist(), ref, ref_logits, prompts[i].numel())


def test_mxfp4_matrix_cores_serving(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=83)
    a, b = _mc_pair(sd, SMALL, dev)
    g = torch.Generator().manual_seed(11)
    ptoks = [torch.randint(0, 1000, (int(L),), generator=g).tolist() for L in torch.randint(8, 60, (22,), generator=g)]
    sps = []
    for i in range(22):
        if i % 3 == 1:
            sps.append(SamplingParams(max_tokens=6 + i % 9, temperature=0.9, top_k=40, top_p=0.9, seed=100 + i))
        else:
            sps.append(SamplingParams(max_tokens=5 + (i * 7) % 13, top_k=1))
    ea = LLM(model=a, quantization="mxfp4", mxfp4_matrix_cores=True, max_num_seqs=16)
    eb = LLM(model=b, max_num_seqs=16)
    ra = ea.generate(prompt_token_ids=ptoks, sampling_params=sps)
    rb = eb.generate(prompt_token_ids=ptoks, sampling_params=sps)
    assert ea.stats["max_active"] == 16 and eb.stats["max_active"] == 16
    for i in range(22):
        assert ra[i].outputs[0].token_ids == rb[i].outputs[0].token_ids, i
    with pytest.raises(ValueError):
        LLM(model=b, mxfp4_matrix_cores=True)
    with pytest.raises(ValueError):
        LLM(model=b, quantization=None, mxfp4_matrix_cores=True)


def test_mxfp4_matrix_cores_speculative(dev):
    """num_speculative_tokens = 7: a verify step of 8 rows, which the VALU form (max_batch() == 4) refuses"""
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(SMALL, seed=84)
    a, b = _mc_pair(sd, SMALL, dev)
    banned, new = 5, 40
    prompt = torch.randint(0, 1000, (1, 23), generator=torch.Generator().manual_seed(12)).to(dev)
    wrong = [banned] * (new + 8)                                   # a banned id: no pick can equal it

    def gen(m, script):
        out = m.generate(input_ids=prompt, max_new_tokens=new, bad_words_ids=[[banned]], num_speculative_tokens=7, _spec_script=script)
        return out[0, prompt.shape[1]:].tolist(), m.last_spec_stats

    ids_w, st_w = gen(a, wrong)
    ids_l, _ = gen(a, None)
    ref_w, _ = gen(b, wrong)
    ref_l, _ = gen(b, None)
    assert len(ids_w) == new and st_w["accepted"] == 0
    assert ids_w == ref_w and ids_l == ref_l
    assert ids_l == ids_w, "the ids depend on the drafts"
    own, st_o = gen(a, list(ids_w))                                # its own output as the script: every draft accepted
    assert own == ids_w and st_o["accepted"] > 0


def test_mxfp4_matrix_cores_needs_mxfp4(dev):
    from usdm_amd.llm import USDMForCausalLM
    for q in (None, "fp8"):
        with pytest.raises(ValueError):
            USDMForCausalLM(SMALL, dev, quantization=q, mxfp4_matrix_cores=True)
        with pytest.raises(ValueError):
            USDMForCausalLM.random_init(SMALL, dev, quantization=q, mxfp4_matrix_cores=True)
    with pytest.raises(ValueError):
        USDMForCausalLM(SMALL, dev, quantization="mxfp4", fp8_matrix_cores=True, mxfp4_matrix_cores=True)
