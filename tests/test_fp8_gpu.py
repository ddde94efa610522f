"""GPU: weight-only FP8 (quantization="fp8", usdm_amd/quant.py).  Because every dequantized weight W' = e4m3(q) * 2^e is a bf16
value, the FP8 path must equal the bf16 path on W' BIT FOR BIT: usdm_gemv_fp8 against usdm_gemv / usdm_gemv_batch, the dequant
kernel against quant.dequantize_rows, and the FP8 model against a bf16 model loaded from W'."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _wprime(sd):
    """the state dict with every streamed matrix replaced by its dequantized FP8 form W' (per matrix = per packed matrix)"""
    from usdm_amd.quant import dequantize_rows, quantize_rows
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight" or any(p in k for p in PROJ):
            out[k] = dequantize_rows(*quantize_rows(v.to(torch.bfloat16)))
    return out


def _pair(sd, cfg, dev, ctx_max=256):
    from usdm_amd.llm import USDMForCausalLM
    a = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, quantization="fp8")
    b = USDMForCausalLM.from_state_dict(_wprime(sd), cfg, dev, ctx_max=ctx_max)
    a.keep_logits = b.keep_logits = True
    return a, b


SHAPES = [  # (name, N, K, mode): the 7B decode projections, then odd N and K tails
    ("qkv", 6144, 4096, "norm"), ("o", 4096, 4096, "res"), ("gu", 28672, 4096, "glu"), ("down", 4096, 14336, "res"),
    ("lm_head", 42003, 4096, "head"), ("odd", 37, 1792, "res"), ("k512", 1003, 512, "norm"), ("glu512", 96, 512, "glu"),
    ("head512", 1003, 512, "head")]


@pytest.mark.parametrize("name,N,K,mode", SHAPES)
def test_gemv_fp8_bit_identical_to_bf16_on_dequantized_weights(dev, name, N, K, mode):
    from usdm_amd import ops
    from usdm_amd.quant import Fp8Weight
    bf = torch.bfloat16
    seed = sum(map(ord, name))
    W = _r((N, K), seed, K ** -0.5)
    W[3 % N] *= 40.0                                   # rows with different scales
    W[5 % N] *= 1e-3
    Wq = Fp8Weight.from_matrix(W.to(bf).to(dev))
    Wd = Wq.dequantize()
    nb_max = 4
    X = _r((nb_max, K), seed + 1).to(bf).to(dev)
    R = _r((nb_max, N), seed + 2).to(bf).to(dev)
    g = (1 + 0.1 * _r((K,), seed + 3)).float().to(dev)
    ban = None
    kw = {}
    nout = N // 2 if mode == "glu" else N
    if mode == "norm":
        kw = dict(norm_w=g, eps=1e-5)
    elif mode == "glu":
        kw = dict(act=3)
    if mode == "head":
        ban = torch.zeros(N, dtype=torch.uint8)
        ban[:min(N, 32002) // 4 * 3] = 1                # text->unit: most text ids banned (whole workgroups skip their rows)
        ban[N - 7] = 1
        ban = ban.to(dev)
    nparts = ops.gemv_nblocks(N)

    def run1(Wt, b):
        x = X[b]
        if mode == "head":
            pv, pi, y32 = (torch.zeros(nparts, device=dev), torch.zeros(nparts, dtype=torch.int32, device=dev),
                           torch.zeros(N, device=dev))
            ops.gemv(Wt, x, N=N, K=K, norm_w=g, eps=1e-5, ban=ban, part_val=pv, part_idx=pi, y32=y32)
            return pv, pi, y32
        y = torch.zeros(nout, dtype=bf, device=dev)
        ops.gemv(Wt, x, N=N, K=K, residual=R[b] if mode == "res" else None, y16=y, **kw)
        return (y,)

    ref = [run1(Wd, b) for b in range(nb_max)]
    for b in range(nb_max):
        got = run1(Wq, b)
        for u, v in zip(got, ref[b]):
            assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v), (name, b)
    # float64 sanity bound: the scale is applied the right way round
    if mode in ("res", "norm") or mode == "head":
        xin = X[0].double()
        if mode in ("norm", "head"):
            xin = (X[0].double() * torch.rsqrt(X[0].double().pow(2).mean() + 1e-5)) * g.double()
        y64 = Wd.double() @ xin + (R[0].double() if mode == "res" else 0)
        got = ref[0][0].double() if mode != "head" else ref[0][2].double()
        fin = torch.isfinite(got)
        assert (got[fin] - y64[fin]).abs().max() <= 2e-2 * y64[fin].abs().max() + 1e-3, name
    # nb = 2, 3, 4 (VALU batch kernel) equal nb = 1 per item
    for nb in (2, 3, 4):
        if mode == "head":
            pv, pi, y32 = (torch.zeros(nb, nparts, device=dev), torch.zeros(nb, nparts, dtype=torch.int32, device=dev),
                           torch.zeros(nb, N, device=dev))
            ops.gemv_batch(Wq, X, nb=nb, N=N, K=K, x_bs=K, y_bs=N, part_bs=nparts, norm_w=g, eps=1e-5, ban=ban, part_val=pv,
                           part_idx=pi, y32=y32)
            for b in range(nb):
                assert torch.equal(pv[b], ref[b][0]) and torch.equal(pi[b], ref[b][1]) and torch.equal(y32[b].view(torch.int32), ref[b][2].view(torch.int32))
        else:
            y = torch.zeros(nb, nout, dtype=bf, device=dev)
            ops.gemv_batch(Wq, X, nb=nb, N=N, K=K, x_bs=K, y_bs=nout, res_bs=N, residual=R if mode == "res" else None, y16=y, **kw)
            for b in range(nb):
                assert torch.equal(y[b], ref[b][0]), (name, nb, b)


def test_gemv_fp8_refuses_unsupported_forms(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError
    from usdm_amd.quant import Fp8Weight
    N, K = 256, 512
    Wq = Fp8Weight.from_matrix(_r((N, K), 1).to(torch.bfloat16).to(dev))
    x = _r((8, K), 2).to(torch.bfloat16).to(dev)
    y = torch.zeros(8, N, dtype=torch.bfloat16, device=dev)
    with pytest.raises(UsdmError):
        ops.gemv_batch(Wq, x, nb=8, N=N, K=K, x_bs=K, y_bs=N, y16=y)        # matrix-core form
    with pytest.raises(UsdmError):
        ops.gemv_batch(Wq, x, nb=2, N=N, K=K, x_bs=K, y_bs=N, y16=y, form=1)
    with pytest.raises(UsdmError):
        ops.gemv(Wq, x[0], N=N, K=K, y16=y[0], x_delta=torch.zeros(K, device=dev), x_out=x[1])


@pytest.mark.parametrize("N,K", [(28672, 4096), (4096, 14336), (37, 1792), (5, 8)])
def test_dequant_kernel_equals_dequantize_rows(dev, N, K):
    from usdm_amd import ops
    from usdm_amd.quant import Fp8Weight
    W = _r((N, K), N + K, 0.02)
    W[0] *= 1e4
    Wq = Fp8Weight.from_matrix(W.to(torch.bfloat16).to(dev))
    out = torch.full((N, K + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.dequant_fp8(Wq, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :K].view(torch.int16), Wq.dequantize().view(torch.int16))
    assert torch.isnan(out[:, K:]).all()                      # nothing written past K


def _model_cases(a, b, V, dev, seed):
    """greedy + ban + EOS, sampled, and three rounds of exact prefix reuse: identical ids and last_logits"""
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
    assert any(k[1] > 0 for k in a._prefill_plans), "no partial prefill happened"


def test_fp8_model_equals_bf16_model_on_dequantized_weights_small(dev):
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(SMALL, seed=61)
    a, b = _pair(sd, SMALL, dev)
    assert a.weight_bytes_per_token() <= 0.51 * b.weight_bytes_per_token()
    assert a.max_batch() == 4 and not a.cmb and a.chain == 0
    _model_cases(a, b, SMALL["vocab_size"], dev, 3)


def test_fp8_model_full_width_two_layers_exact_and_vs_oracle(dev):
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=2)
    sd = MO.random_state_dict(cfg, seed=62)
    a, b = _pair(sd, cfg, dev)
    assert a.weight_bytes_per_token() <= 0.51 * b.weight_bytes_per_token()
    _model_cases(a, b, cfg["vocab_size"], dev, 4)
    del b
    # against the CPU oracle run on W' (near-tie rule), with the text->unit ban of the reference's TTS round
    ids = torch.randint(0, 32000, (37,), generator=torch.Generator().manual_seed(9))
    bad = [[i] for i in range(32002)]
    ref, ref_logits = MO.greedy_generate(_wprime(sd), cfg, ids, 8, bad_words_ids=bad, return_logits=True)
    out = a.generate(input_ids=ids[None].to(dev), max_new_tokens=8, bad_words_ids=bad)[0].tolist()
    check_against_oracle(out, ref, ref_logits, len(ids))


def test_fp8_generate_batch_and_serving(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=63)
    a, _ = _pair(sd, SMALL, dev)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 1000, (1, L), generator=g).to(dev) for L in (23, 40, 17, 31, 28, 36)]
    outs = a.generate_batch(prompts, 10)                      # 6 prompts: groups of 4 + 2 on the VALU form
    assert 4 in a._batches and 2 in a._batches and all(B <= 4 for B in a._batches)
    for p, o in zip(prompts, outs):
        assert torch.equal(o, a.generate(input_ids=p, max_new_tokens=10))
    eng = LLM(model=a, quantization="fp8", max_num_seqs=16)
    with pytest.raises(ValueError):
        LLM(model=a, quantization="awq")
    sps = [SamplingParams(max_tokens=9, top_k=1), SamplingParams(max_tokens=11, temperature=1.2, top_p=0.9, top_k=50, seed=7),
           SamplingParams(max_tokens=6, top_k=1), SamplingParams(max_tokens=12, temperature=0.8, top_k=-1, seed=99),
           SamplingParams(max_tokens=8, top_k=1), SamplingParams(max_tokens=10, top_k=1)]
    ptoks = [p[0].tolist() for p in prompts]
    res = eng.generate(prompt_token_ids=ptoks, sampling_params=sps)
    assert eng.stats["max_active"] <= 4
    for i in range(len(ptoks)):
        alone = eng.generate(prompt_token_ids=[ptoks[i]], sampling_params=sps[i])[0].outputs[0].token_ids
        assert res[i].outputs[0].token_ids == alone, i


def test_cli_quantization_fp8_on_a_synthetic_model_cache_dir(dev, tmp_path):
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
    assert inf.main(["--input_path", user, "--model_cache_dir", cache, "--output_path", out, "--quantization", "fp8"]) == 0
    sr, data = read(out)
    assert sr == 22050 and data.dtype == np.float32 and data.size > 0 and np.isfinite(data).all()
