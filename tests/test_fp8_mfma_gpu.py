"""GPU: the FP8-weight matrix-core form (usdm_gemv_fp8_mfma, opt-in `fp8_matrix_cores=True`).  Every dequantized weight
W' = e4m3(q) * 2^e is a bf16 value and the kernel changes only the weight load and unpack, so it must equal the bf16 matrix-core form
(usdm_gemv_batch form 1 / 5) on W' BIT FOR BIT - kernel by kernel, and therefore the FP8 model with fp8_matrix_cores must equal a bf16
model loaded from W' token for token, in generate_batch and in serving."""
import ctypes as C

import pytest
import torch

from tests.test_fp8_gpu import SMALL, _wprime

pytestmark = pytest.mark.gpu

NBS = (1, 5, 8, 13, 16)
SHAPES = [  # (name, N, K, mode, form, ks): the 7B decode projections, down_proj split and unsplit, then the generic forms
    ("qkv", 6144, 4096, "norm", 0, False), ("o", 4096, 4096, "res", 0, False), ("gu", 28672, 4096, "glu", 0, False),
    ("lm_head", 42003, 4096, "head", 0, False), ("down_ks", 4096, 14336, "res", 0, True), ("down_f5", 4096, 14336, "res", 5, True),
    ("k512", 1003, 512, "norm", 0, False), ("glu512", 96, 512, "glu", 0, False), ("head512", 1003, 512, "head", 0, False),
    ("odd", 37, 1792, "res", 0, False), ("k1024", 512, 1024, "res", 0, False), ("stream6k", 200, 6144, "res", 5, False)]


def _weights(N, K, seed, dev):
    """a [N][K] bf16 matrix with row scales spread over 2^-12 .. 2^12 (very different row exponents), and its Fp8Weight"""
    from usdm_amd.quant import Fp8Weight
    g = torch.Generator(device=dev).manual_seed(seed)
    W = torch.randn(N, K, device=dev, generator=g) * K ** -0.5
    W *= torch.exp2(torch.randint(-12, 13, (N, 1), device=dev, generator=g).float())
    W[3 % N] *= 40.0
    W[5 % N] *= 1e-3
    Wq = Fp8Weight.from_matrix(W.to(torch.bfloat16))
    return Wq, Wq.dequantize()


@pytest.mark.parametrize("name,N,K,mode,form,use_ks", SHAPES)
def test_fp8_mfma_bit_identical_to_bf16_matrix_cores_on_dequantized_weights(dev, name, N, K, mode, form, use_ks):
    from usdm_amd import ops
    bf = torch.bfloat16
    seed = sum(map(ord, name))
    Wq, Wd = _weights(N, K, seed, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    X = torch.randn(16, K, device=dev, generator=g).to(bf)
    R = torch.randn(16, N, device=dev, generator=g).to(bf)
    nw = (1 + 0.1 * torch.randn(K, device=dev, generator=g)).float()
    nout = N // 2 if mode == "glu" else N
    kw = dict(norm_w=nw, eps=1e-5) if mode in ("norm", "head") else dict(act=3) if mode == "glu" else {}
    ban = None
    if mode == "head":
        ban = torch.zeros(N, dtype=torch.uint8, device=dev)
        ban[:min(N, 32002) // 4 * 3] = 1                         # text->unit: most text ids banned (whole tiles are skipped)
        ban[N - 7] = 1
    ks = ks2 = None
    if use_ks:
        ksf = ops.gemv_batch_ks_floats(N, K)
        assert ksf > 0
        ks = (torch.zeros(ksf, device=dev), torch.zeros(-(-N // 16), dtype=torch.int32, device=dev))
        ks2 = (torch.zeros(ksf, device=dev), torch.zeros(-(-N // 16), dtype=torch.int32, device=dev))
    nparts = 256

    def run(fn, W, nb, ksa, bf16_form):
        f = form if fn is ops.gemv_fp8_mfma else bf16_form
        if mode == "head":
            pv, pi = torch.zeros(nb, nparts, device=dev), torch.zeros(nb, nparts, dtype=torch.int32, device=dev)
            y32 = torch.zeros(nb, N, device=dev)
            fn(W, X, nb=nb, N=N, K=K, x_bs=K, y_bs=N, part_bs=nparts, ban=ban, part_val=pv, part_idx=pi, y32=y32, form=f, **kw)
            return pv, pi.view(torch.float32), y32
        y = R[:nb].clone() if mode == "res" else torch.zeros(nb, nout, dtype=bf, device=dev)
        fn(W, X, nb=nb, N=N, K=K, x_bs=K, y_bs=nout, res_bs=N, residual=y if mode == "res" else None, y16=y, form=f, ks=ksa, **kw)
        return (y,)

    for nb in NBS:
        got = run(ops.gemv_fp8_mfma, Wq, nb, ks, None)
        ref = run(ops.gemv_batch, Wd, nb, ks2, 1 if form == 0 else form)
        for u, v in zip(got, ref):
            assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                               v.view(torch.int32) if v.dtype == torch.float32 else v), (name, nb)
        if use_ks:
            assert int(ks[1].abs().sum()) == 0, "tile counters not back at zero"
    # float64 sanity bound on sequence 0 (the scale is applied the right way round)
    if mode in ("res", "norm"):
        x = X[0].double()
        if mode == "norm":
            x = x * torch.rsqrt(x.pow(2).mean() + 1e-5) * nw.double()
        y64 = Wd.double() @ x + (R[0].double() if mode == "res" else 0)
        y = got[0][0].double()
        assert (y - y64).abs().max() <= 2e-2 * y64.abs().max() + 1e-3, name


def test_fp8_mfma_refusals(dev):
    from usdm_amd import ops
    from usdm_amd._lib import GemvFp8Args, UsdmError, check, lib
    N, K = 256, 512
    Wq, _ = _weights(N, K, 1, dev)
    x = torch.randn(17, K, device=dev).to(torch.bfloat16)
    y = torch.zeros(17, N, dtype=torch.bfloat16, device=dev)
    kw = dict(N=N, K=K, x_bs=K, y_bs=N, y16=y)
    for bad in (dict(nb=17), dict(nb=8, form=3), dict(nb=8, form=1), dict(nb=8, form=-1)):
        with pytest.raises(UsdmError):
            ops.gemv_fp8_mfma(Wq, x, **{**kw, **bad})
    with pytest.raises(UsdmError):        # K % 256
        ops.gemv_fp8_mfma(Wq, x, nb=8, **{**kw, "K": 504, "x_bs": 504})
    Wbig, _ = _weights(8, 8192, 2, dev)    # the fused RMSNorm with K > 4096
    xb = torch.randn(8, 8192, device=dev).to(torch.bfloat16)
    with pytest.raises(UsdmError):
        ops.gemv_fp8_mfma(Wbig, xb, nb=8, N=8, K=8192, x_bs=8192, y_bs=8, y16=y, norm_w=torch.ones(8192, device=dev))
    with pytest.raises(UsdmError):        # more than 64 tiles per workgroup: 256 x 64 x 16 rows + 1
        Wt, _ = _weights(256 * 64 * 16 + 16, 256, 3, dev)
        xs = torch.randn(8, 256, device=dev).to(torch.bfloat16)
        ops.gemv_fp8_mfma(Wt, xs, nb=8, N=Wt.N, K=256, x_bs=256, y_bs=0, y32=torch.zeros(8, Wt.N, device=dev))
    # p2p / merged-attention input / hand-off / x_delta: set on the argument struct directly (the checks run before anything is read)
    dummy = C.c_void_p(y.data_ptr())
    for field in ("p2p", "mrg_po", "mrg_pm", "cmb_gran", "x_delta", "x_out"):
        b = ops.gemv_batch(Wq.q, x, nb=8, only_args=True, **kw)
        setattr(b.g, field, dummy)
        f = GemvFp8Args()
        f.b, f.row_exp = b, C.c_void_p(Wq.e.data_ptr())
        with pytest.raises(UsdmError):
            check(lib.usdm_gemv_fp8_mfma(C.byref(f), C.c_void_p(torch.cuda.current_stream().cuda_stream)), field)
    b = ops.gemv_batch(Wq.q, x, nb=8, only_args=True, **kw)
    b.g.p2p_mode = 1
    f = GemvFp8Args()
    f.b, f.row_exp = b, C.c_void_p(Wq.e.data_ptr())
    with pytest.raises(UsdmError):
        check(lib.usdm_gemv_fp8_mfma(C.byref(f), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "p2p_mode")
    with pytest.raises(TypeError):
        ops.gemv_fp8_mfma(Wq.dequantize(), x, nb=8, **kw)
    torch.cuda.synchronize()


def _mc_pair(sd, cfg, dev, ctx_max=256):
    from usdm_amd.llm import USDMForCausalLM
    a = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, quantization="fp8", fp8_matrix_cores=True)
    b = USDMForCausalLM.from_state_dict(_wprime(sd), cfg, dev, ctx_max=ctx_max)
    return a, b


def test_fp8_matrix_cores_small_model(dev):
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(SMALL, seed=71)
    a, b = _mc_pair(sd, SMALL, dev)
    assert a.max_batch() == 16 and b.max_batch() == 16
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
    for p, o in zip(prompts, a.generate_batch(prompts, 10)):     # a group of 3 keeps the VALU FP8 form: equal to generate()
        assert torch.equal(o, a.generate(input_ids=p, max_new_tokens=10))


def test_fp8_matrix_cores_full_width_two_layers(dev):
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=2)
    sd = MO.random_state_dict(cfg, seed=72)
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


def test_fp8_matrix_cores_serving(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=73)
    a, b = _mc_pair(sd, SMALL, dev)
    g = torch.Generator().manual_seed(11)
    ptoks = [torch.randint(0, 1000, (int(L),), generator=g).tolist() for L in torch.randint(8, 60, (22,), generator=g)]
    sps = []
    for i in range(22):
        if i % 3 == 1:
            sps.append(SamplingParams(max_tokens=6 + i % 9, temperature=0.9, top_k=40, top_p=0.9, seed=100 + i))
        else:
            sps.append(SamplingParams(max_tokens=5 + (i * 7) % 13, top_k=1))
    ea = LLM(model=a, quantization="fp8", max_num_seqs=16)
    eb = LLM(model=b, max_num_seqs=16)
    ra = ea.generate(prompt_token_ids=ptoks, sampling_params=sps)
    rb = eb.generate(prompt_token_ids=ptoks, sampling_params=sps)
    assert ea.stats["max_active"] == 16 and eb.stats["max_active"] == 16
    for i in range(22):
        assert ra[i].outputs[0].token_ids == rb[i].outputs[0].token_ids, i
    with pytest.raises(ValueError):
        LLM(model=b, fp8_matrix_cores=True)
    with pytest.raises(ValueError):
        LLM(model=b, quantization=None, fp8_matrix_cores=True)


def test_fp8_matrix_cores_needs_fp8(dev):
    from usdm_amd.llm import USDMForCausalLM
    with pytest.raises(ValueError):
        USDMForCausalLM(SMALL, dev, quantization=None, fp8_matrix_cores=True)
    with pytest.raises(ValueError):
        USDMForCausalLM.random_init(SMALL, dev, fp8_matrix_cores=True)
