"""GPU: weight-only MXFP4 (quantization="mxfp4", usdm_amd/quant.py).  Every dequantized weight W' = e2m1(code) * 2^s is a bf16
value, so the MXFP4 path must equal the bf16 path on W' BIT FOR BIT: usdm_dequant_mxfp4 against quant.dequantize_mxfp4 (starting
with the truth table of the hardware conversion, which pins nibble order and code values), usdm_gemv_mxfp4 against usdm_gemv /
usdm_gemv_batch, and the MXFP4 model (fp8 lm_head) against a bf16 model loaded from W'."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
bf = torch.bfloat16


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _wprime(sd):
    """the state dict with every layer matrix replaced by its dequantized MXFP4 form and the lm_head by its dequantized FP8 form
    (blocks run along K, so per matrix = per packed matrix)"""
    from usdm_amd.quant import dequantize_mxfp4, dequantize_rows, quantize_mxfp4, quantize_rows
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight":
            out[k] = dequantize_rows(*quantize_rows(v.to(bf)))
        elif any(p in k for p in PROJ):
            out[k] = dequantize_mxfp4(*quantize_mxfp4(v.to(bf)))
    return out


def _pair(sd, cfg, dev, ctx_max=256, **kw):
    from usdm_amd.llm import USDMForCausalLM
    a = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, quantization="mxfp4", **kw)
    b = USDMForCausalLM.from_state_dict(_wprime(sd), cfg, dev, ctx_max=ctx_max, **kw)
    a.keep_logits = b.keep_logits = True
    return a, b


def test_truth_table_of_the_hardware_conversion(dev):
    """all 256 byte values x scale bytes {2, 100, 127, 140, 252}: byte b holds element 2m (bits 3:0) and 2m+1 (bits 7:4)"""
    from usdm_amd import ops
    from usdm_amd.quant import E2M1_VALUES, Mxfp4Weight, dequantize_mxfp4
    scales = [2, 100, 127, 140, 252]
    K = 512                                        # 16 blocks of 32 elements = 16 bytes each: byte value 16 * block + j at byte j
    byts = torch.arange(256, dtype=torch.uint8).view(16, 16)
    codes = torch.stack((byts & 15, byts >> 4), dim=2).view(1, K).repeat(len(scales), 1)
    sc = torch.tensor(scales, dtype=torch.uint8)[:, None].repeat(1, K // 32)
    tab = torch.tensor(list(E2M1_VALUES) + [-x for x in E2M1_VALUES], dtype=torch.float64)
    want = (tab[codes.long()] * 2.0 ** (sc.double() - 127).repeat_interleave(32, dim=1)).to(bf)       # the host table, from the definition
    assert torch.equal(want, dequantize_mxfp4(codes, sc))
    W = Mxfp4Weight.from_codes(codes.to(dev), sc.to(dev))
    out = torch.full((len(scales), K), float("nan"), dtype=bf, device=dev)
    ops.dequant_mxfp4(W, out)
    torch.cuda.synchronize()
    got = out.cpu()
    # (negative-zero codes, which the quantizer never stores, compare as the bf16 bit patterns too: -0.0)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        [(int(i), int(j)) for i, j in (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8]]


def _hard_rows(W, K):
    """blocks of very different scales inside one row, a zero block, and a block at each clamp (in place; returns the K ranges whose
    x must be zero so that the products with the upper-clamp block stay finite)"""
    N = W.shape[0]
    r = 3 % N
    for b in range(K // 32):
        W[r, 32 * b:32 * b + 32] *= 2.0 ** ((b * 7) % 41 - 20)
    W[5 % N, 32:64] = 0.0                                          # a zero block
    W[5 % N, 64:96] *= 1e-3
    lo = torch.arange(32).float() % 8 * 2.0 ** -126                # lower clamp: amax = 7 * 2^-126 -> s = -125 after the clamp
    W[7 % N, 0:32] = lo * torch.tensor([1.0, -1.0]).repeat(16)
    W[7 % N, 96:128] = 0.0
    W[7 % N, 96] = 1.5 * 2.0 ** 127                                # upper end: s = 125
    W[7 % N, 97] = -2.0 ** 125
    return [(96, 128)]


SHAPES = [  # (name, N, K, mode): the 7B decode projections, then odd N and K tails
    ("qkv", 6144, 4096, "norm"), ("o", 4096, 4096, "res"), ("gu", 28672, 4096, "glu"), ("down", 4096, 14336, "res"),
    ("odd", 37, 1792, "res"), ("k512", 1003, 512, "norm"), ("glu512", 96, 512, "glu")]


@pytest.mark.parametrize("name,N,K,mode", SHAPES)
def test_gemv_mxfp4_bit_identical_to_bf16_on_dequantized_weights(dev, name, N, K, mode):
    from usdm_amd import ops
    from usdm_amd.quant import Mxfp4Weight
    seed = sum(map(ord, name))
    W = _r((N, K), seed, K ** -0.5)
    zero_x = _hard_rows(W, K)
    Wq = Mxfp4Weight.from_matrix(W.to(bf).to(dev))
    Wd = Wq.dequantize()
    assert torch.isfinite(Wd.float()).all() and float(Wd.float().abs().max()) >= 2.0 ** 127
    sb = Wq.unpack()[1]
    assert int(sb.min()) == 2 and int(sb.max()) == 252              # a block at each clamp
    nb_max = 4
    X = _r((nb_max, K), seed + 1)
    for k0, k1 in zero_x:
        X[:, k0:k1] = 0.0
    X = X.to(bf).to(dev)
    R = _r((nb_max, N), seed + 2).to(bf).to(dev)
    g = (1 + 0.1 * _r((K,), seed + 3)).float().to(dev)
    kw = {}
    nout = N // 2 if mode == "glu" else N
    if mode == "norm":
        kw = dict(norm_w=g, eps=1e-5)
    elif mode == "glu":
        kw = dict(act=3)

    def run1(Wt, b):
        y = torch.full((nout,), float("nan"), dtype=bf, device=dev)
        ops.gemv(Wt, X[b], N=N, K=K, residual=R[b] if mode == "res" else None, y16=y, **kw)
        return y

    ref = [run1(Wd, b) for b in range(nb_max)]
    for b in range(nb_max):
        got = run1(Wq, b)
        assert torch.isfinite(got.float()).all(), (name, b)
        assert torch.equal(got.view(torch.int16), ref[b].view(torch.int16)), (name, b, int((got != ref[b]).sum()))
    # the skip word: nothing is written
    y = torch.full((nout,), 7.0, dtype=bf, device=dev)
    ops.gemv(Wq, X[0], N=N, K=K, y16=y, skip=torch.ones(1, dtype=torch.int32, device=dev), **kw)
    assert (y == 7.0).all()
    # float64 bound: the scales are applied the right way round (both sides equally wrong cannot pass).  With d = W' x in float64 and
    # m = |W'| |x|: one bf16 rounding of d and one of d + r (2^-8 each, of |d| + |r|, doubled to 2^-7 for roundings that fall the
    # other way), the f32 accumulation (K * 2^-23 * m), and, with RMSNorm, one bf16 ulp on every element of x (2^-8 * m: the
    # kernel's f32 sum of squares runs in another order than this one)
    if mode in ("res", "norm"):
        xin = X[0].double()
        if mode == "norm":
            xn = (X[0].float() * torch.rsqrt(X[0].float().pow(2).mean() + 1e-5)).to(bf).float()
            xin = (xn * g).to(bf).double()
        d64 = Wd.double() @ xin
        m = Wd.double().abs() @ xin.abs()
        r64 = R[0].double() if mode == "res" else torch.zeros_like(d64)
        y64 = d64.to(bf).double() + r64 if mode == "res" else d64
        bound = 2.0 ** -7 * (d64.abs() + r64.abs()) + (K * 2.0 ** -23 + (2.0 ** -8 if mode == "norm" else 0.0)) * m + 1e-30
        for got in (ref[0], run1(Wq, 0)):
            err = (got.double() - y64).abs()
            assert (err <= bound).all(), (name, float((err / bound).max()))
    # nb = 2, 3, 4 (VALU batch kernel) equal nb = 1 per item
    for nb in (2, 3, 4):
        y = torch.full((nb, nout), float("nan"), dtype=bf, device=dev)
        ops.gemv_batch(Wq, X, nb=nb, N=N, K=K, x_bs=K, y_bs=nout, res_bs=N, residual=R if mode == "res" else None, y16=y, **kw)
        for b in range(nb):
            assert torch.equal(y[b].view(torch.int16), ref[b].view(torch.int16)), (name, nb, b)


def test_gemv_mxfp4_refuses_unsupported_forms(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError
    from usdm_amd.quant import Mxfp4Weight
    N, K = 256, 512
    Wq = Mxfp4Weight.from_matrix(_r((N, K), 1).to(bf).to(dev))
    x = _r((8, K), 2).to(bf).to(dev)
    y = torch.zeros(8, N, dtype=bf, device=dev)
    nparts = ops.gemv_nblocks(N)
    pv, pi, y32 = torch.zeros(nparts, device=dev), torch.zeros(nparts, dtype=torch.int32, device=dev), torch.zeros(N, device=dev)
    f3 = lambda n: torch.zeros(n, device=dev)
    with pytest.raises(UsdmError):
        ops.gemv_batch(Wq, x, nb=8, N=N, K=K, x_bs=K, y_bs=N, y16=y)        # matrix-core form (more than 4 sequences)
    with pytest.raises(UsdmError):
        ops.gemv_batch(Wq, x, nb=2, N=N, K=K, x_bs=K, y_bs=N, y16=y, form=1)
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], x_delta=torch.zeros(K, device=dev), x_out=x[1])
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, part_val=pv, part_idx=pi)             # lm_head mode
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], ban=torch.zeros(N, dtype=torch.uint8, device=dev))
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], y32=y32)
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], merge=(f3(4 * 8), f3(4 * 8), f3(4 * 8 * 128), 8))
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0][1:], N=N, K=K - 32, y16=y[0])                    # misaligned x
    with pytest.raises(ValueError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], only_args=True)             # no chained form
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,K", [(37, 1792), (6144, 4096), (28672, 4096), (4096, 14336), (5, 32)])
def test_dequant_kernel_equals_dequantize_mxfp4(dev, N, K):
    from usdm_amd import ops
    from usdm_amd.quant import Mxfp4Weight, dequantize_mxfp4, quantize_mxfp4
    W = _r((N, K), N + K, 0.02)
    W[0] *= 1e4
    W[1 % N, :32] = 0.0
    c, s = quantize_mxfp4(W.to(bf))
    Wq = Mxfp4Weight.from_codes(c.to(dev), s.to(dev))
    out = torch.full((N, K + 8), float("nan"), dtype=bf, device=dev)
    ops.dequant_mxfp4(Wq, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :K].cpu().view(torch.int16), dequantize_mxfp4(c, s).view(torch.int16))
    assert torch.equal(Wq.dequantize().cpu(), dequantize_mxfp4(c, s))
    assert torch.isnan(out[:, K:]).all()                      # nothing written past K


def _model_cases(a, b, V, dev, seed):
    """greedy + ban + EOS, sampled, and three rounds (exact prefix reuse with a bf16 cache): identical ids and last_logits"""
    g = torch.Generator().manual_seed(seed)
    bad = [[i] for i in range(0, V, 3)]
    p = torch.randint(0, V, (1, 41), generator=g).to(dev)
    ra = a.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad)
    rb = b.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad)
    assert torch.equal(ra, rb) and torch.equal(a.last_logits, b.last_logits)
    eos = int(ra[0, 41 + 4])                            # an id it emits: the device-side EOS must stop both at the same step
    ra = a.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad, eos_token_id=eos)
    rb = b.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad, eos_token_id=eos)
    assert torch.equal(ra, rb) and ra.shape[1] <= 41 + 5
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=1234, max_new_tokens=10)
    ra, rb = a.generate(input_ids=p, **kw), b.generate(input_ids=p, **kw)
    assert torch.equal(ra, rb) and torch.equal(a.last_logits, b.last_logits)
    for rnd, (new, extra) in enumerate([(9, 6), (7, 1), (8, 0)]):
        oa = a.generate(input_ids=p, max_new_tokens=new)
        ob = b.generate(input_ids=p, max_new_tokens=new)
        assert torch.equal(oa, ob) and torch.equal(a.last_logits, b.last_logits), rnd
        p = torch.cat([oa, torch.randint(0, V, (1, extra), generator=g).to(dev)], 1)
    if not a.kv8:
        assert any(k[1] > 0 for k in a._prefill_plans), "no partial prefill happened"
    prompts = [torch.randint(0, V, (1, L), generator=g).to(dev) for L in (23, 40, 17, 31, 28, 36)]
    for n in (3, 6):                                    # 6: groups of 4 + 2
        oa, ob = a.generate_batch(prompts[:n], 7), b.generate_batch(prompts[:n], 7, group=4)
        for x, y, q in zip(oa, ob, prompts):
            assert torch.equal(x, y)
            assert torch.equal(x, a.generate(input_ids=q, max_new_tokens=7))
    assert all(B <= 4 for B in a._batches)


@pytest.mark.parametrize("kv", [None, "fp8"])
def test_mxfp4_model_equals_bf16_model_on_dequantized_weights_small(dev, kv):
    from oracle import mistral_oracle as MO
    from usdm_amd.quant import Fp8Weight, Mxfp4Weight
    sd = MO.random_state_dict(SMALL, seed=71)
    a, b = _pair(sd, SMALL, dev, kv_cache_dtype=kv)
    L = a.W["layers"][0]
    assert all(isinstance(L[k], Mxfp4Weight) for k in ("qkv", "o", "gu", "down")) and isinstance(a.W["lm_head"], Fp8Weight)
    assert a.W["embed"].dtype == bf
    # 4.25 bits per weight in the layers (K = 512 / 1024 are padded to 2048 here), 8 + in the lm_head
    want = sum(l[k].nbytes for l in a.W["layers"] for k in ("qkv", "o", "gu", "down")) + a.W["lm_head"].nbytes
    assert a.weight_bytes_per_token() == want
    assert a.max_batch() == 4 and not a.cmb and not a.merge_in_oproj and a.chain == 0
    _model_cases(a, b, SMALL["vocab_size"], dev, 3)


@pytest.mark.parametrize("kv", [None, "fp8"])
def test_mxfp4_model_full_width_two_layers_exact_and_vs_oracle(dev, kv):
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=2)
    sd = MO.random_state_dict(cfg, seed=72)
    a, b = _pair(sd, cfg, dev, kv_cache_dtype=kv)
    lay = sum(l[k].numel() for l in b.W["layers"] for k in ("qkv", "o", "gu", "down"))
    assert a.weight_bytes_per_token() == lay * 17 // 32 + b.W["lm_head"].numel() + b.W["lm_head"].shape[0]   # 4.25 bits; fp8 head
    _model_cases(a, b, cfg["vocab_size"], dev, 4)
    del b
    if kv is None:
        # against the CPU oracle run on W' (near-tie rule), with the text->unit ban of the reference's TTS round
        ids = torch.randint(0, 32000, (37,), generator=torch.Generator().manual_seed(9))
        bad = [[i] for i in range(32002)]
        ref, ref_logits = MO.greedy_generate(_wprime(sd), cfg, ids, 8, bad_words_ids=bad, return_logits=True)
        out = a.generate(input_ids=ids[None].to(dev), max_new_tokens=8, bad_words_ids=bad)[0].tolist()
        check_against_oracle(out, ref, ref_logits, len(ids))


def test_mxfp4_constructors(dev):
    from usdm_amd import synth
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.quant import Fp8Weight, Mxfp4Weight
    m = USDMForCausalLM.random_init(SMALL, dev, seed=1, ctx_max=128, quantization="mxfp4")
    assert isinstance(m.W["layers"][1]["down"], Mxfp4Weight) and isinstance(m.W["lm_head"], Fp8Weight)
    out = m.generate(input_ids=torch.randint(0, 1000, (1, 9), generator=torch.Generator().manual_seed(1)).to(dev), max_new_tokens=4)
    assert out.shape == (1, 13)
    m2 = synth.make_llm(dev, cfg=SMALL, ctx_max=128, quantization="mxfp4")
    assert m2.quantization == "mxfp4" and isinstance(m2.W["layers"][0]["qkv"], Mxfp4Weight)


def test_mxfp4_serving(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=73)
    a, b = _pair(sd, SMALL, dev)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 1000, (1, L), generator=g).to(dev) for L in (23, 40, 17, 31, 28, 36)]
    eng = LLM(model=a, quantization="mxfp4", max_num_seqs=16)
    with pytest.raises(ValueError):
        LLM(model=a, quantization="fp8")                      # the model object was loaded with another format
    with pytest.raises(ValueError):
        LLM(model=b, quantization="mxfp4")
    sps = [SamplingParams(max_tokens=9, top_k=1), SamplingParams(max_tokens=11, temperature=1.2, top_p=0.9, top_k=50, seed=7),
           SamplingParams(max_tokens=6, top_k=1), SamplingParams(max_tokens=12, temperature=0.8, top_k=-1, seed=99),
           SamplingParams(max_tokens=8, top_k=1), SamplingParams(max_tokens=10, top_k=1)]
    ptoks = [p[0].tolist() for p in prompts]
    res = eng.generate(prompt_token_ids=ptoks, sampling_params=sps)
    assert eng.stats["max_active"] <= 4
    for i in range(len(ptoks)):
        alone = eng.generate(prompt_token_ids=[ptoks[i]], sampling_params=sps[i])[0].outputs[0].token_ids
        assert res[i].outputs[0].token_ids == alone, i


def test_cli_quantization_mxfp4_on_a_synthetic_model_cache_dir(dev, tmp_path):
    import os

    import numpy as np
    from scipy.io.wavfile import read, write

    import usdm_amd.inference as inf
    from tests.test_checkpoints_gpu import _write_decoders, _write_llm, _write_tokenizer, _write_w2v
    cache = str(tmp_path / "cache")
    os.makedirs(cache)
    _write_decoders(cache)
    _write_w2v(os.path.join(cache, "xlsr2_1b_v2"), n_layers=35)
    np.save(os.path.join(cache, "kmeans_10k.npy"), (torch.randn(10000, 256, generator=torch.Generator().manual_seed(6)) * 0.5).numpy())
    llm_dir = os.path.join(cache, "models--naver-ai--USDM-DailyTalk", "snapshots", "r0")
    _write_llm(llm_dir, seed=7, shard="30MB", rig_eos=True)
    _write_tokenizer(llm_dir)
    t = torch.arange(20000) / 16000.0
    wav = (0.2 * torch.sin(2 * torch.pi * 300 * t)).numpy().astype(np.float32)
    user, out = str(tmp_path / "user.wav"), str(tmp_path / "out.wav")
    write(user, 16000, wav)
    os.environ.pop("USDM_MODEL_CACHE_DIR", None)
    assert inf.main(["--input_path", user, "--model_cache_dir", cache, "--output_path", out, "--quantization", "mxfp4"]) == 0
    sr, data = read(out)
    assert sr == 22050 and data.dtype == np.float32 and data.size > 0 and np.isfinite(data).all()
