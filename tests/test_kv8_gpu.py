"""GPU: the opt-in FP8 KV cache (kv_cache_dtype="fp8", usdm_amd/quant.py quantize_kv_rows).  Every dequantized cache row is a bf16
value, so the contracts are exact: usdm_attn_decode_fp8 on quantized caches equals usdm_attn_decode on the dequantized caches bit
for bit, the rows it appends are quantize_rows of the rows the bf16 kernel appends, and an fp8-KV model equals the bf16-KV model
whose cache rows are round-tripped before any later step reads them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)


def _rope_tables(ctx_max, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2).float() / 128))
    fr = torch.arange(ctx_max).float()[:, None] * inv[None, :]
    return fr.cos().to(torch.bfloat16).to(dev).contiguous(), fr.sin().to(torch.bfloat16).to(dev).contiguous()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _adversarial_rows():
    """[n, 128] bf16 rows that exercise the device-side quantizer's corners (the rows of tests/test_kv8_quant_cpu.py and more): an
    all-zero row, maxima exactly at / one bf16 ulp above / below 1.75 * 2^k (the exponent rule's mantissa test), a maximum that is
    a power of two, the EXP_MAX clamp with saturation at 448, the EXP_MIN clamp, bf16-subnormal rows, a lone outlier, -0.0."""
    g = torch.Generator().manual_seed(99)
    base = torch.randn(128, generator=g).clamp(-1.5, 1.5) * 0.4
    rows = [torch.zeros(128)]
    for k in (0, 8, -20, 60):
        for m in (1.75, 1.7578125, 1.7421875, 1.0, 1.9921875):     # bf16 values around the threshold
            r = base * 2.0 ** k
            r[(k + 7) % 128] = -m * 2.0 ** k
            rows.append(r)
    big = base * 2.0e38
    big[3], big[77] = 3.3e38, -3.0e38                               # above 448 * 2^119: saturates
    rows += [big, base * 1e-30, base * 1e-36, base * 1e-38, base * 3e-39, base * 1e-40]
    tiny = torch.zeros(128); tiny[5] = 9.2e-41                      # the smallest bf16 subnormal alone
    lone = torch.zeros(128); lone[100] = 449.0; lone[101] = 1e-3; lone[102] = -0.0
    rows += [tiny, lone]
    return torch.stack(rows).to(torch.bfloat16)


def _attn_case(dev, Hq, Hkv, ctx_max, NS, pos, batch=0, window=0, counters=False, skip=False, defer=False, seed=0, adversarial=False,
               cmb=False):
    """one launch of each kernel on the same arguments; returns nothing, asserts the contract.
    adversarial: the V rows the step appends (and the K rows of every sequence at pos 0, where RoPE is the identity) are the
    corner-case rows above, so kv8_row_exp / kv8_byte meet them on the device.  cmb: the o_proj hand-off granules are passed."""
    from usdm_amd import ops
    from usdm_amd.quant import dequantize_kv_rows, quantize_kv_rows
    B = max(1, batch)
    g = torch.Generator().manual_seed(seed)
    nq = (Hq + 2 * Hkv) * 128
    rows = lambda: (torch.randn(B, Hkv, ctx_max, 128, generator=g) * torch.exp(torch.randn(B, Hkv, ctx_max, 1, generator=g))).to(torch.bfloat16)
    k8, ke = quantize_kv_rows(rows().to(dev))
    v8, ve = quantize_kv_rows(rows().to(dev))
    kd, vd = dequantize_kv_rows(k8, ke), dequantize_kv_rows(v8, ve)
    qkv = torch.randn(B, nq, generator=g).to(torch.bfloat16)
    if adversarial:
        adv, n = _adversarial_rows(), 0
        for b in range(B):
            for h in range(Hkv):
                qkv[b, (Hq + Hkv + h) * 128:(Hq + Hkv + h + 1) * 128] = adv[n % len(adv)]
                if pos[b] == 0:
                    qkv[b, (Hq + h) * 128:(Hq + h + 1) * 128] = adv[(n + 11) % len(adv)]
                n += 1
        assert n >= len(adv), "not every adversarial row is used"
    qkv = qkv.to(dev)
    cos, sin = _rope_tables(ctx_max, dev)
    post = torch.tensor(pos, dtype=torch.int32, device=dev)
    assert post.numel() == B
    skp = torch.ones(1, dtype=torch.int32, device=dev) if skip else None
    res = []
    for fp8 in (False, True):
        kc, vc = (k8.clone(), v8.clone()) if fp8 else (kd.clone(), vd.clone())
        kx, vx = ke.clone(), ve.clone()
        pm, pl = torch.zeros(B * Hq * NS, device=dev), torch.zeros(B * Hq * NS, device=dev)
        po = torch.zeros(B * Hq * NS * 128, device=dev)
        out = torch.full((B, Hq * 128), 7.0, dtype=torch.bfloat16, device=dev)
        cnt = torch.zeros(B * Hkv, dtype=torch.int32, device=dev) if counters else None
        cbs = Hkv * ctx_max * 128
        gran = torch.full((Hq * 64,), (1 << 32) | 5, dtype=torch.int64, device=dev) if cmb else None      # tagged: the launch must clear them
        ops.attn_decode(qkv, post, cos, sin, kc[0], vc[0], pm, pl, po, out, Hq=Hq, Hkv=Hkv, ctx_max=ctx_max, NS=NS, scale=128 ** -0.5,
                        counters=cnt, batch=batch, qkv_bs=nq, out_bs=Hq * 128, cache_bs=cbs, skip=skp, defer_merge=defer, window=window,
                        cmb_gran=gran, kv8=(kx[0], vx[0]) if fp8 else None, exp_bs=cbs // 128)
        torch.cuda.synchronize()
        if gran is not None:
            assert not bool(gran.any()), "the hand-off granules' tags must be cleared by the attention launch"
        if cnt is not None:
            assert not bool(cnt.any()), "the merge counters must be left zero"
        res.append((kc, vc, kx, vx, pm, pl, po, out))
    (kb, vb, _, _, pmb, plb, pob, outb), (kf, vf, kef, vef, pmf, plf, pof, outf) = res
    live = [b for b in range(B) if pos[b] < ctx_max and not skip]
    if defer:
        assert torch.equal(_bits(outf), _bits(outb)) and bool((outf == 7.0).all()), "defer_merge must not write out"
    for b in live:
        assert torch.equal(_bits(outf[b]), _bits(outb[b])), f"sequence {b}: output bits differ"
        n = Hq * NS
        for x, y, w in ((pmf, pmb, 1), (plf, plb, 1), (pof, pob, 128)):
            assert torch.equal(_bits(x[b * n * w:(b + 1) * n * w]), _bits(y[b * n * w:(b + 1) * n * w])), f"sequence {b}: partials differ"
    if not live:
        assert torch.equal(_bits(outf), _bits(outb))
    # the caches: untouched except row pos of every live sequence, which is quantize_rows of the row the bf16 kernel appended
    ek8, eke, ev8, eve, ekd, evd = k8.clone(), ke.clone(), v8.clone(), ve.clone(), kd.clone(), vd.clone()
    for b in live:
        p = pos[b]
        assert not torch.equal(_bits(kb[b, :, p]), _bits(kd[b, :, p])), "the bf16 kernel appended nothing?"
        ekd[b, :, p], evd[b, :, p] = kb[b, :, p], vb[b, :, p]
        # (the reference quantizer runs on the CPU: its definition is exact arithmetic, and only there is torch.ldexp trusted to be)
        for c8, ce, row in ((ek8, eke, kb[b, :, p]), (ev8, eve, vb[b, :, p])):
            q_, e_ = quantize_kv_rows(row.cpu())
            c8[b, :, p], ce[b, :, p] = q_.to(dev), e_.to(dev)
    assert torch.equal(_bits(kb), _bits(ekd)) and torch.equal(_bits(vb), _bits(evd))
    assert torch.equal(kf, ek8) and torch.equal(kef, eke), "K rows / exponents"
    assert torch.equal(vf, ev8) and torch.equal(vef, eve), "V rows / exponents"


def test_attn_decode_fp8_equals_bf16_kernel_on_dequantized_caches(dev):
    # the 7B head counts (G = 4), batch 1 with 32 splits of ~20 keys; with the combine launch, the fused merge and deferred
    _attn_case(dev, 32, 8, 2048, 32, [613], seed=1)
    _attn_case(dev, 32, 8, 2048, 32, [640], counters=True, seed=2)
    _attn_case(dev, 32, 8, 2048, 32, [77], defer=True, seed=3)
    _attn_case(dev, 32, 8, 2048, 32, [77], defer=True, cmb=True, seed=12)           # as the 7B decode step launches it
    _attn_case(dev, 32, 8, 2048, 32, [0], cmb=True, seed=13)
    # 16 ragged sequences, 4 splits of up to 512 keys: the pipelined form with > 128 keys per split; pos 0, the last row, and a
    # position past the cache (refused by the kernel: nothing appended, nothing written)
    ragged = [0, 2047, 2048, 1999, 600, 613, 1, 31, 32, 33, 255, 256, 257, 1023, 1500, 5000]
    _attn_case(dev, 32, 8, 2048, 4, ragged, batch=16, seed=4)
    # the quantizer's corner cases as the rows the step appends (16 x 8 V rows, 8 K rows at pos 0)
    _attn_case(dev, 32, 8, 2048, 4, ragged, batch=16, adversarial=True, seed=14)
    _attn_case(dev, 32, 8, 2048, 4, ragged, batch=16, counters=True, seed=5)
    # G = 2, three sequences under a sliding window (pipelined: 150 keys per split); G = 1 single
    _attn_case(dev, 4, 2, 1024, 2, [1000, 299, 300], batch=3, window=300, seed=6)
    _attn_case(dev, 4, 2, 1024, 8, [10, 900, 301], batch=3, window=300, counters=True, seed=7)
    _attn_case(dev, 2, 2, 512, 8, [511], seed=8)
    _attn_case(dev, 2, 2, 512, 8, [0], counters=True, seed=9)
    _attn_case(dev, 2, 2, 512, 8, [512], seed=10)                       # pos >= ctx_max: both caches untouched
    _attn_case(dev, 32, 8, 2048, 32, [613], skip=True, seed=11)         # skip: nothing appended


def test_attn_decode_fp8_refusals(dev):
    from usdm_amd import _lib, ops
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    cos, sin = _rope_tables(256, dev)
    k8, ke = z(2, 256, 128, dt=torch.uint8), z(2, 256, dt=torch.int8)
    args = dict(Hq=4, Hkv=2, ctx_max=256, scale=0.1)
    call = lambda NS=8, kc=k8, kx=ke, **kw: ops.attn_decode(z(8 * 128), z(1, dt=torch.int32), cos, sin, kc, k8.clone(), z(64, dt=torch.float32),
                                                            z(64, dt=torch.float32), z(64 * 128, dt=torch.float32), z(512), NS=NS,
                                                            kv8=(kx, ke.clone()), **args, **kw)
    with pytest.raises(_lib.UsdmError, match="NS == 1"):
        call(NS=1)
    with pytest.raises(_lib.UsdmError, match="16-byte"):
        call(kc=z(2 * 256 * 128 + 16, dt=torch.uint8)[8:])
    with pytest.raises(_lib.UsdmError, match="4-byte"):
        call(kx=z(2 * 256 + 4, dt=torch.int8)[1:])
    with pytest.raises(TypeError):
        call(kc=z(2, 256, 128))
    call()                                                              # ... and the good call runs
    torch.cuda.synchronize()


@pytest.mark.parametrize("pos0", [0, 5])
def test_rope_cache_fp8_equals_quantized_bf16_rows(dev, pos0):
    from usdm_amd import ops
    from usdm_amd.quant import quantize_kv_rows
    Hq, Hkv, S, ctx = 4, 2, 37, 128
    nq, Spad = (Hq + 2 * Hkv) * 128, 64
    g = torch.Generator().manual_seed(3)
    qkv0 = (torch.randn(S, nq, generator=g) * torch.exp(torch.randn(S, 1, generator=g) * 2)).to(torch.bfloat16).to(dev)
    # the quantizer's corner cases: as V rows (stored as they are) and as the K rows of token 0 (with pos0 = 0 RoPE is the identity there)
    adv = _adversarial_rows().to(dev)
    for i in range(len(adv)):
        s_, h_ = (i // Hkv) % S, i % Hkv
        qkv0[s_, (Hq + Hkv + h_) * 128:(Hq + Hkv + h_ + 1) * 128] = adv[i]
    qkv0[0, Hq * 128:(Hq + 1) * 128], qkv0[0, (Hq + 1) * 128:(Hq + 2) * 128] = adv[1], adv[-1]
    cos, sin = _rope_tables(ctx, dev)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    qa, kc, vc, vta = qkv0.clone(), z(Hkv, ctx, 128), z(Hkv, ctx, 128), z(Hkv, 128, Spad)
    ops.rope_cache(qa, cos, sin, kc, vc, ld=nq, S=S, pos0=pos0, Hq=Hq, Hkv=Hkv, ctx_max=ctx, max_pos=ctx, vt=vta, vt_ld=Spad)
    qb, k8, v8, vtb, kscr = qkv0.clone(), z(Hkv, ctx, 128, dt=torch.uint8), z(Hkv, ctx, 128, dt=torch.uint8), z(Hkv, 128, Spad), z(Hkv, Spad, 128)
    ke, ve = z(Hkv, ctx, dt=torch.int8), z(Hkv, ctx, dt=torch.int8)
    ops.rope_cache(qb, cos, sin, k8, v8, ld=nq, S=S, pos0=pos0, Hq=Hq, Hkv=Hkv, ctx_max=ctx, max_pos=ctx, vt=vtb, vt_ld=Spad, kv8=(ke, ve),
                   kscr=kscr, kscr_ld=Spad)
    torch.cuda.synchronize()
    assert torch.equal(_bits(qa), _bits(qb)) and torch.equal(_bits(vta), _bits(vtb))
    assert torch.equal(_bits(kscr[:, :S]), _bits(kc[:, pos0:pos0 + S])) and not bool(kscr[:, S:].any())
    for c8, ce, cb in ((k8, ke, kc), (v8, ve, vc)):      # whole caches: rows outside pos0 .. pos0+S-1 are zero rows on both sides
        q, e = quantize_kv_rows(cb.cpu())                # (on the CPU, as above)
        bad = (c8.cpu() != q).nonzero()
        assert torch.equal(ce.cpu(), e), (ce.cpu() != e).nonzero()[:4]
        assert not len(bad), [(i.tolist(), float(cb.cpu()[tuple(i)]), int(c8.cpu()[tuple(i)]), int(q[tuple(i)])) for i in bad[:4]]
        assert bool(cb[:, pos0:pos0 + S].any())


# ------------------------------------------------------------------------------------------------------------------ model
def _rt_hook(b):
    """_logits_hook of a bf16-cache model: round-trip every cache row written so far (rows 0 .. pos; the hook runs after the step's
    attention launches appended row pos and before the pick advances pos, and after the prefill) - before any later step reads them"""
    from usdm_amd.quant import roundtrip_kv_rows

    def hook():
        n = min(int(b.st_pos.item()) + 1, b.ctx_max)
        b.kcache[:, :, :n] = roundtrip_kv_rows(b.kcache[:, :, :n])
        b.vcache[:, :, :n] = roundtrip_kv_rows(b.vcache[:, :, :n])
    return hook


def _pair(sd, cfg, dev, ctx_max=256, **kw):
    from usdm_amd.llm import USDMForCausalLM
    a = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, kv_cache_dtype="fp8", **kw)
    b = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=ctx_max, **kw)
    b.reuse_prefix = False                           # (USDM_PREFIX_REUSE=0: a reused prefix would have been round-tripped)
    a.keep_logits = b.keep_logits = True
    assert a.reuse_prefix is False and a.vtc is None and a.kcache.dtype == torch.uint8
    return a, b


def _model_cases(a, b, V, dev, seed):
    """Greedy with a ban mask, with a device-side EOS, and sampled with a fixed seed: identical ids and last_logits.
    Greedy runs go through the hook path on BOTH sides (a no-op hook on the fp8 side): the hook path picks with usdm_sample_final
    (top_k = 1, a seeded draw among EXACT ties of the bf16-valued logits), the graph path with usdm_argmax_final (lowest id), so
    hook against graph could differ at an exact tie with identical logits.  Sampled runs compare the fp8 model's graph path."""
    g = torch.Generator().manual_seed(seed)
    bad = [[i] for i in range(0, V, 3)]
    p = torch.randint(0, V, (1, 41), generator=g).to(dev)
    noop, hook = (lambda: None), _rt_hook(b)
    kw = dict(input_ids=p, max_new_tokens=12, bad_words_ids=bad, seed=5)
    ra, la = a.generate(_logits_hook=noop, **kw), a.last_logits.clone()
    rb = b.generate(_logits_hook=hook, **kw)
    assert torch.equal(ra, rb) and torch.equal(la, b.last_logits)
    plain = b.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad)
    print("tokens that differ from the bf16-cache model:", int((plain != ra).sum()), "of 12")
    eos = int(ra[0, 41 + 4])                            # an id it emits: the device-side EOS must stop both at the same step
    ra = a.generate(_logits_hook=noop, eos_token_id=eos, **kw)
    rb = b.generate(_logits_hook=hook, eos_token_id=eos, **kw)
    assert torch.equal(ra, rb) and ra.shape[1] <= 41 + 5
    # the fp8 model's captured-graph greedy path against its own hook path: equal unless a step had an exact tie at the top
    rg = a.generate(input_ids=p, max_new_tokens=12, bad_words_ids=bad)
    rh = a.generate(_logits_hook=noop, **kw)
    if not torch.equal(rg, rh):
        i = int((rg != rh).nonzero()[0, 1])
        a.generate(_logits_hook=noop, **dict(kw, max_new_tokens=i - 41 + 1))
        top = torch.topk(a.last_logits, 2).values
        assert float(top[0]) == float(top[1]), "graph and hook pick differ without an exact tie"
    skw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, seed=1234, max_new_tokens=10)
    ra, la = a.generate(input_ids=p, **skw), a.last_logits.clone()
    rb = b.generate(input_ids=p, _logits_hook=hook, **skw)
    assert torch.equal(ra, rb) and torch.equal(la, b.last_logits)


def test_fp8_kv_model_equals_bf16_model_on_round_tripped_rows_small(dev):
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(SMALL, seed=81)
    a, b = _pair(sd, SMALL, dev)
    _model_cases(a, b, SMALL["vocab_size"], dev, 3)
    del a, b
    a, b = _pair(sd, SMALL, dev, quantization="fp8")       # fp8 weights on both sides
    _model_cases(a, b, SMALL["vocab_size"], dev, 4)


def test_fp8_kv_model_full_width_two_layers(dev):
    from oracle import mistral_oracle as MO
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=2)
    sd = MO.random_state_dict(cfg, seed=82)
    a, b = _pair(sd, cfg, dev)
    assert a.cmb and b.cmb, "the o_proj hand-off combine reads partials, not caches: kept with an fp8 cache"
    _model_cases(a, b, cfg["vocab_size"], dev, 5)
    del a, b
    a, b = _pair(sd, cfg, dev, quantization="fp8")        # fp8 weights on both sides: the 4096-wide fp8 GEMVs with the fp8 cache
    assert not a.cmb and not b.cmb
    _model_cases(a, b, cfg["vocab_size"], dev, 6)


def test_fp8_kv_generate_and_batch16_vs_kv_quantized_oracle(dev):
    """generate() and a 16-sequence generate_batch (matrix-core form) against the KV-quantized CPU reference, near-tie rule and caps
    of tests/_greedy_compare.py unchanged; once more with fp8 weights on the matrix cores (the reference then on W')."""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from tests._kv8_reference import ORACLE_SMALL, kv8_greedy_generate, small_oracle_prompts, wprime
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=ORACLE_SMALL["sd_seed"])
    prompts, new, bad = small_oracle_prompts(), ORACLE_SMALL["new"], ORACLE_SMALL["bad"]
    for kw, w in ((dict(), sd), (dict(quantization="fp8", fp8_matrix_cores=True), wprime(sd))):
        refs = [kv8_greedy_generate(w, SMALL, p, new, bad_words_ids=bad, return_logits=True) for p in prompts]
        m = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256, kv_cache_dtype="fp8", **kw)
        assert m.max_batch() == 16
        batch = m.generate_batch([p[None].to(dev) for p in prompts], max_new_tokens=new, bad_words_ids=bad)
        assert list(m._batches) == [16]
        firsts = [check_against_oracle(o[0].tolist(), ref, lg, p.numel()) for p, (ref, lg), o in zip(prompts, refs, batch)]
        print("batch of 16 vs the KV-quantized reference, first differences (None = identical):", firsts)
        singles = []
        for p, (ref, lg) in list(zip(prompts, refs))[:4]:
            out = m.generate(input_ids=p[None].to(dev), max_new_tokens=new, bad_words_ids=bad)[0].tolist()
            singles.append(check_against_oracle(out, ref, lg, p.numel()))
        print("generate() vs the KV-quantized reference:", singles)
        del m


def test_fp8_kv_generate_batch_and_serving(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=83)
    a, b = _pair(sd, SMALL, dev)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 1000, (1, L), generator=g).to(dev) for L in (23, 40, 17, 31, 28, 36)]
    outs = a.generate_batch(prompts, 10, group=4)             # 6 prompts: groups of 4 + 2 on the VALU form
    assert 4 in a._batches and 2 in a._batches and all(B <= 4 for B in a._batches)
    for p, o in zip(prompts, outs):
        assert torch.equal(o, a.generate(input_ids=p, max_new_tokens=10))
    eng = LLM(model=a, kv_cache_dtype="fp8", max_num_seqs=4)
    with pytest.raises(ValueError):
        LLM(model=b, kv_cache_dtype="fp8")
    with pytest.raises(ValueError):
        LLM(model=a, kv_cache_dtype="int8")
    with pytest.raises(ValueError):
        USDMForCausalLM.from_state_dict(sd, SMALL, dev, kv_cache_dtype="int8")
    with pytest.raises(NotImplementedError):
        USDMForCausalLM.from_state_dict(sd, SMALL, dev, kv_cache_dtype="fp8", tp_segments=True)
    sps = [SamplingParams(max_tokens=9, top_k=1), SamplingParams(max_tokens=11, temperature=1.2, top_p=0.9, top_k=50, seed=7),
           SamplingParams(max_tokens=6, top_k=1), SamplingParams(max_tokens=12, temperature=0.8, top_k=-1, seed=99),
           SamplingParams(max_tokens=8, top_k=1), SamplingParams(max_tokens=10, top_k=1)]
    ptoks = [p[0].tolist() for p in prompts]
    res = eng.generate(prompt_token_ids=ptoks, sampling_params=sps)
    assert eng.stats["max_active"] <= 4
    for i in range(len(ptoks)):
        alone = eng.generate(prompt_token_ids=[ptoks[i]], sampling_params=sps[i])[0].outputs[0].token_ids
        assert res[i].outputs[0].token_ids == alone, i


def test_fp8_kv_batched_request_running_into_the_context_limit(dev):
    """the fp8 twin of tests/test_serving_gpu.py::test_batched_request_running_into_the_context_limit"""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from tests._kv8_reference import kv8_greedy_generate
    from usdm_amd.llm import USDMForCausalLM, step_kind
    from usdm_amd.serving import LLM, SamplingParams
    sd = MO.random_state_dict(SMALL, seed=47)
    m = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128, kv_cache_dtype="fp8")
    eng = LLM(model=m, max_num_seqs=4)
    g = torch.Generator().manual_seed(5)
    lens = (101, 20, 99, 33, 25)
    want = (100000, 70, 100000, 60, 50)
    prompts = [torch.randint(0, 1000, (L,), generator=g) for L in lens]
    sps = [SamplingParams(max_tokens=w, top_k=1) for w in want]
    outs = eng.generate(prompt_token_ids=[p.tolist() for p in prompts], sampling_params=sps)
    for p, w, o in zip(prompts, want, outs):
        n = min(w, 128 - p.numel())
        ref, ref_logits = kv8_greedy_generate(sd, SMALL, p, n, return_logits=True)
        toks = o.outputs[0].token_ids
        check_against_oracle(p.tolist() + toks, ref, ref_logits, p.numel())
        assert len(toks) == n and o.outputs[0].finish_reason == "length"
    assert eng.stats["batched_requests"] == 5 and eng.stats["max_active"] == 4
    ds = m.decode_slots(4)
    before = [getattr(ds, k).clone() for k in ("kc", "vc", "ke", "ve")]
    ds.pos.fill_(128); ds.step.zero_()
    ds.steps[step_kind()].run()
    torch.cuda.synchronize()
    for k, t in zip(("kc", "vc", "ke", "ve"), before):
        assert torch.equal(t, getattr(ds, k)), k


def test_fp8_kv_cache_footprint(dev):
    from usdm_amd.llm import USDMForCausalLM

    def cache_bytes(m, B):
        ds = m.decode_slots(B)
        ts = [m.kcache, m.vcache, getattr(m, "vtc", None), getattr(m, "kexp", None), getattr(m, "vexp", None)]
        ts += [getattr(ds, k) for k in ("kc", "vc", "ke", "ve")]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)
    a = USDMForCausalLM.random_init(SMALL, dev, seed=1, ctx_max=512, kv_cache_dtype="fp8")
    b = USDMForCausalLM.random_init(SMALL, dev, seed=1, ctx_max=512)
    assert a.vtc is None and b.vtc is not None
    assert cache_bytes(a, 16) <= 0.51 * cache_bytes(b, 16)
    assert a.kv_bytes_per_token_row() == 2 * 2 * 2 * 129 and b.kv_bytes_per_token_row() == 2 * 2 * 2 * 256
