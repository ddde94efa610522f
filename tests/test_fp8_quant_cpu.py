"""CPU: the weight-only FP8 quantizer (usdm_amd/quant.py) - OCP e4m3fn bytes with one power-of-two scale per row - and the
checks of quantization="fp8" that run before anything touches the GPU."""
import pytest
import torch

from usdm_amd.quant import E4M3_MAX, EXP_MAX, EXP_MIN, Fp8Weight, dequantize_rows, quantize_rows


def _e4m3fn_table():
    """value of every e4m3fn byte from the OCP definition (bias 7, no infinities, S.1111.111 = NaN; fnuz would differ)."""
    vals = []
    for b in range(256):
        s, ex, m = b >> 7, (b >> 3) & 15, b & 7
        if ex == 15 and m == 7:
            vals.append(float("nan"))
            continue
        v = (m / 8.0) * 2.0 ** -6 if ex == 0 else (1 + m / 8.0) * 2.0 ** (ex - 7)
        vals.append(-v if s else v)
    return torch.tensor(vals, dtype=torch.float64)


def _rows():
    g = torch.Generator().manual_seed(3)
    rnd = torch.randn(24, 520, generator=g)
    # heavy-tailed rows (normal / uniform ratio), drawn from the test's own generator: the inputs are the same in every run
    heavy = torch.randn(24, 520, generator=g) / torch.rand(24, 520, generator=g).clamp_min(1e-3) * 0.02
    adv = torch.randn(8, 520, generator=g) * 0.01
    adv[0] = 0.0                                  # all-zero row
    adv[1, 17] = 1e4                              # one outlier
    adv[2] = 2.0 ** -9 * torch.randint(-7, 8, (520,), generator=g).float()   # every value an e4m3 subnormal at e = 0
    adv[2, 0] = 448.0                             # ... with the row maximum exactly 448
    adv[3, :] = 448.0
    adv[4] *= 1e-36                               # tiny row: clamped exponent
    adv[5, ::2] = -adv[5, ::2].abs() * 1e3
    adv[6] = torch.linspace(-3, 3, 520)
    adv[7, :] = 2.0 ** -130                       # (bf16 subnormal-range values)
    return torch.cat([rnd, heavy, adv]).to(torch.bfloat16)


def test_quantizer_invariants():
    w = _rows()
    q, e = quantize_rows(w)
    assert q.dtype == torch.uint8 and e.dtype == torch.int8 and q.shape == w.shape and e.shape == (w.shape[0],)
    tab = _e4m3fn_table()
    v = tab[q.long()]
    assert not torch.isnan(v).any()
    assert v.abs().max() <= E4M3_MAX
    # e minimal: max |w| / 2^e <= 448 < max |w| / 2^(e-1), unless clamped; all-zero row -> 0
    amax = w.double().abs().amax(1)
    ed = e.double()
    for r in range(w.shape[0]):
        if amax[r] == 0:
            assert e[r] == 0
            continue
        assert EXP_MIN <= e[r] <= EXP_MAX
        assert amax[r] / 2.0 ** ed[r] <= E4M3_MAX
        assert e[r] == EXP_MIN or amax[r] / 2.0 ** (ed[r] - 1) > E4M3_MAX, r
    assert e[24 + 24 + 1] == 5 and e[24 + 24 + 2] == 0 and e[24 + 24 + 3] == 0 and e[24 + 24 + 4] == EXP_MIN
    # every W' element is exactly a bf16 value, and dequantize_rows computes it
    wq = v * 2.0 ** ed[:, None]
    assert torch.equal(wq.to(torch.bfloat16).double(), wq)
    assert torch.equal(dequantize_rows(q, e).double(), wq)
    nz = wq != 0
    assert (wq[nz].abs() >= 2.0 ** -126).all()                  # nonzero W' values are normal bf16


def test_encoding_is_ocp_e4m3fn_with_round_to_nearest_even():
    w = _rows()
    q, e = quantize_rows(w)
    tab = _e4m3fn_table()
    # torch's float8_e4m3fn (the OCP encoding) reads every finite byte as the OCP table does
    fin = ~torch.isnan(tab)
    assert torch.equal(torch.arange(256, dtype=torch.uint8)[fin].view(torch.float8_e4m3fn).double(), tab[fin])
    # each byte is the nearest e4m3 value to w / 2^e, ties to the even code
    s = w.double() / 2.0 ** e.double()[:, None]
    cand = tab[fin][None, :]
    for r in range(0, w.shape[0], 7):
        d = (s[r][:, None] - cand).abs()
        best = d.min(1).values
        got = (tab[q[r].long()] - s[r]).abs()
        assert torch.equal(got, best), r
        tie = (d == best[:, None]).sum(1) > 1
        if tie.any():
            qt = q[r][tie].long()
            assert ((qt & 1) == 0).all() | (tab[qt] == 0).all()


def test_quantization_error_is_bounded():
    w = _rows()
    q, e = quantize_rows(w)
    wq = dequantize_rows(q, e).double()
    wd = w.double()
    s = wd.abs() / 2.0 ** e.double()[:, None]
    normal = s >= 2.0 ** -6                                       # values in e4m3's normal range
    assert ((wq - wd).abs()[normal] <= 2.0 ** -4 * wd.abs()[normal]).all()
    sub = ~normal
    assert ((wq - wd).abs()[sub] <= 2.0 ** -10 * 2.0 ** e.double()[:, None].expand_as(wd)[sub]).all()   # half an e4m3 subnormal step


def test_packed_then_quantized_equals_per_matrix():
    from usdm_amd.llm import _pack_gate_up, shard_weights
    g = torch.Generator().manual_seed(11)
    H, I = 64, 96
    gate, up = torch.randn(I, H, generator=g).to(torch.bfloat16), (torch.randn(I, H, generator=g) * 3).to(torch.bfloat16)
    dq = lambda t: dequantize_rows(*quantize_rows(t))
    assert torch.equal(dq(_pack_gate_up(gate, up)), _pack_gate_up(dq(gate), dq(up)))
    qm, km, vm = (torch.randn(n, H, generator=g).to(torch.bfloat16) * sc for n, sc in ((128, 1.0), (64, 0.01), (64, 50.0)))
    assert torch.equal(dq(torch.cat([qm, km, vm])), torch.cat([dq(qm), dq(km), dq(vm)]))
    # the loader (shard_weights) quantizes exactly those packed matrices
    cfg = dict(vocab_size=40, hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1,
               head_dim=64, rms_norm_eps=1e-5)
    sd = {"model.embed_tokens.weight": torch.randn(40, H, generator=g), "lm_head.weight": torch.randn(40, H, generator=g),
          "model.norm.weight": torch.ones(H)}
    p = "model.layers.0."
    sd.update({p + "self_attn.q_proj.weight": qm[:64], p + "self_attn.k_proj.weight": km, p + "self_attn.v_proj.weight": vm,
               p + "self_attn.o_proj.weight": torch.randn(H, 64, generator=g), p + "mlp.gate_proj.weight": gate,
               p + "mlp.up_proj.weight": up, p + "mlp.down_proj.weight": torch.randn(H, I, generator=g),
               p + "input_layernorm.weight": torch.ones(H), p + "post_attention_layernorm.weight": torch.ones(H)})
    W = shard_weights(lambda n: sd[n], cfg, 0, 1, "cpu", quantization="fp8")
    L = W["layers"][0]
    assert all(isinstance(L[k], Fp8Weight) for k in ("qkv", "o", "gu", "down")) and isinstance(W["lm_head"], Fp8Weight)
    assert W["embed"].dtype == torch.bfloat16 and L["ln1"].dtype == torch.float32
    assert torch.equal(L["gu"].dequantize(), _pack_gate_up(dq(gate), dq(up)))
    assert torch.equal(L["qkv"].dequantize(), torch.cat([dq(qm[:64]), dq(km), dq(vm)]))
    assert torch.equal(W["lm_head"].dequantize(), dq(sd["lm_head.weight"].to(torch.bfloat16)))


def test_fp8_rejections_before_any_gpu_work():
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.serving import LLM
    cfg = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
    with pytest.raises(ValueError):
        USDMForCausalLM(cfg, "cuda", quantization="int4")
    with pytest.raises(NotImplementedError):
        USDMForCausalLM(cfg, "cuda", quantization="fp8", tp_size=2, tp_rank=0)
    with pytest.raises(NotImplementedError):
        USDMForCausalLM(cfg, "cuda", quantization="fp8", tp_segments=True)
    with pytest.raises(ValueError):
        LLM(model="naver-ai/USDM-DailyTalk", quantization="awq")
    with pytest.raises(ValueError):
        quantize_rows(torch.tensor([[1.0, float("inf")] * 4]))
