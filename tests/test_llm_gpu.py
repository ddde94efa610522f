"""GPU parity of the Mistral decode/prefill path (HIP) against the CPU oracle (HF-equivalent bf16 math).
ids must match exactly while the oracle's top-2 logit gap exceeds bf16 noise; logits within bf16 tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)


@pytest.mark.parametrize("N,K", [(64, 512), (100, 4096), (37, 1792), (512, 14336)])
def test_gemv_plain_residual_norm(dev, N, K):
    from usdm_amd import ops
    bf = torch.bfloat16
    W, x, r = _r((N, K), 1, K ** -0.5).to(bf), _r((K,), 2).to(bf), _r((N,), 3).to(bf)
    g = (1 + 0.1 * _r((K,), 4)).to(bf)
    y = torch.zeros(N, dtype=bf, device=dev)
    ops.gemv(W.to(dev), x.to(dev), N=N, K=K, residual=r.to(dev), y16=y)
    ref = (W.float() @ x.float()).to(bf) + r
    assert (y.cpu().float() - ref.float()).abs().max() <= 2e-2 * ref.float().abs().max()
    # fused RMSNorm
    ops.gemv(W.to(dev), x.to(dev), N=N, K=K, norm_w=g.float().to(dev), eps=1e-5, y16=y)
    xf = x.float()
    xn = g * (xf * torch.rsqrt(xf.pow(2).mean() + 1e-5)).to(bf)
    ref = (W.float() @ xn.float()).to(bf)
    assert (y.cpu().float() - ref.float()).abs().max() <= 2e-2 * ref.float().abs().max()


def test_gemv_swiglu_and_argmax(dev):
    from usdm_amd import ops
    from usdm_amd.llm import _pack_gate_up
    bf = torch.bfloat16
    I, K = 96, 512
    Wg, Wu, x = _r((I, K), 1, K ** -0.5).to(bf), _r((I, K), 2, K ** -0.5).to(bf), _r((K,), 3).to(bf)
    y = torch.zeros(I, dtype=bf, device=dev)
    ops.gemv(_pack_gate_up(Wg, Wu).to(dev), x.to(dev), N=2 * I, K=K, act=3, y16=y)
    ref = torch.nn.functional.silu((Wg.float() @ x.float()).to(bf)) * (Wu.float() @ x.float()).to(bf)
    assert (y.cpu().float() - ref.float()).abs().max() <= 3e-2 * ref.float().abs().max()
    # lm_head mode with a ban mask
    V = 1003
    W = _r((V, K), 5, K ** -0.5).to(bf)
    ban = torch.zeros(V, dtype=torch.uint8)
    logits = (W.float() @ x.float()).to(bf).float()
    ban[logits.argmax()] = 1  # ban the winner: the runner-up must be returned
    nb = ops.gemv_nblocks(V)
    pv, pi = torch.zeros(nb, device=dev), torch.zeros(nb, dtype=torch.int32, device=dev)
    lg = torch.zeros(V, device=dev)
    ops.gemv(W.to(dev), x.to(dev), N=V, K=K, ban=ban.to(dev), part_val=pv, part_idx=pi, y32=lg, idx_offset=0)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    nxt, out, step, pos = i32(1), i32(8), i32(1), i32(1)
    E = _r((V, 64), 9).to(bf).to(dev)
    hrow = torch.zeros(64, dtype=bf, device=dev)
    ops.argmax_final(pv, pi, nb, ops.decode_state(nxt, out, step, pos), embed=E, h_out=hrow, Hd=64)
    masked = logits.clone()
    masked[ban.bool()] = -float("inf")
    got = int(nxt.item())
    assert masked[got] >= masked.max() - 1e-6 and ban[got] == 0
    assert int(step.item()) == 1 and int(pos.item()) == 1 and int(out[0].item()) == got
    assert torch.equal(hrow, E[got])
    fin = torch.isfinite(masked)
    assert (lg.cpu()[fin] - masked[fin]).abs().max() <= 2e-2 * masked[fin].abs().max()


@pytest.mark.parametrize("ctx", [1, 5, 130, 700])
def test_attn_decode(dev, ctx):
    """One decode step of GQA attention vs fp64 math (rope in bf16 as HF)."""
    from oracle import mistral_oracle as MO
    from usdm_amd import ops
    bf = torch.bfloat16
    Hq, Hkv, d, ctx_max, NS = 8, 2, 128, 1024, 8
    pos = ctx - 1
    cfg = dict(head_dim=d, rope_theta=10000.0)
    qkv = _r(((Hq + 2 * Hkv) * d,), 1).to(bf)
    kc = _r((Hkv, ctx_max, d), 2).to(bf)   # already-roped cached keys
    vc = _r((Hkv, ctx_max, d), 3).to(bf)
    cosf, sinf = MO.rope_tables(cfg, torch.arange(ctx_max), bf)
    cos, sin = cosf[:, :64].contiguous(), sinf[:, :64].contiguous()
    q = qkv[:Hq * d].view(Hq, d)
    k = qkv[Hq * d:(Hq + Hkv) * d].view(Hkv, d)
    v = qkv[(Hq + Hkv) * d:].view(Hkv, d)
    qr = (q * cosf[pos]) + (MO.rotate_half(q) * sinf[pos])
    kr = (k * cosf[pos]) + (MO.rotate_half(k) * sinf[pos])
    K = torch.cat([kc[:, :pos], kr[:, None]], 1).double().repeat_interleave(Hq // Hkv, 0)
    V = torch.cat([vc[:, :pos], v[:, None]], 1).double().repeat_interleave(Hq // Hkv, 0)
    w = torch.softmax((qr.double()[:, None] @ K.transpose(1, 2)) * d ** -0.5, -1)
    ref = (w @ V).reshape(Hq * d)
    kcd, vcd = kc.to(dev), vc.to(dev)
    out = torch.zeros(Hq * d, dtype=bf, device=dev)
    pm, pl = torch.zeros(Hq * NS, device=dev), torch.zeros(Hq * NS, device=dev)
    po = torch.zeros(Hq * NS * d, device=dev)
    ops.attn_decode(qkv.to(dev), torch.tensor([pos], dtype=torch.int32, device=dev), cos.to(dev), sin.to(dev), kcd, vcd,
                    pm, pl, po, out, Hq=Hq, Hkv=Hkv, ctx_max=ctx_max, NS=NS, scale=d ** -0.5)
    assert (out.cpu().double() - ref).abs().max() <= 2e-2 * ref.abs().max()
    # single-workgroup-per-kv-head form (NS = 1)
    out1 = torch.zeros_like(out)
    ops.attn_decode(qkv.to(dev), torch.tensor([pos], dtype=torch.int32, device=dev), cos.to(dev), sin.to(dev), kc.to(dev), vc.to(dev),
                    pm, pl, po, out1, Hq=Hq, Hkv=Hkv, ctx_max=ctx_max, NS=1, scale=d ** -0.5)
    assert (out1.cpu().double() - ref).abs().max() <= 2e-2 * ref.abs().max()
    # the new K/V row was appended
    assert torch.equal(kcd[:, pos].cpu(), kr) and torch.equal(vcd[:, pos].cpu(), v)
    # partials left for the consumer (defer_merge) and merged inside a GEMV's x-staging prologue (the o_proj of the decode
    # step): with W = identity the GEMV returns exactly the merged, bf16-rounded attention output
    for ns in (8, 3):
        pm2, pl2, po2 = torch.zeros(Hq * ns, device=dev), torch.zeros(Hq * ns, device=dev), torch.zeros(Hq * ns * d, device=dev)
        ops.attn_decode(qkv.to(dev), torch.tensor([pos], dtype=torch.int32, device=dev), cos.to(dev), sin.to(dev), kc.to(dev), vc.to(dev),
                        pm2, pl2, po2, None, Hq=Hq, Hkv=Hkv, ctx_max=ctx_max, NS=ns, scale=d ** -0.5, defer_merge=True)
        eye = torch.eye(Hq * d, dtype=bf, device=dev)
        y = torch.zeros(Hq * d, dtype=bf, device=dev)
        ops.gemv(eye, y, N=Hq * d, K=Hq * d, y16=y.clone(), merge=(pm2, pl2, po2, ns))        # x pointer is ignored in merge mode
        y2 = torch.zeros(Hq * d, dtype=bf, device=dev)
        ops.gemv(eye, y, N=Hq * d, K=Hq * d, y16=y2, merge=(pm2, pl2, po2, ns))
        assert (y2.cpu().double() - ref).abs().max() <= 2e-2 * ref.abs().max()
        if ns == NS:   # same partials as the combine kernel saw: equal up to the last bf16 bit (different summation order)
            assert (y2.float() - out.float()).abs().max() <= 2 ** -7 * out.float().abs().max()


def test_split_merges_agree_bit_for_bit(dev):
    """The three merges of the context-split partials share csrc/attn_merge.h and must give the same bf16 bits on the same inputs:
    (a) the combine launch, (b) the last-arriving workgroup of the attention launch (counters), (c) the first workgroups of the
    o_proj launch (defer_merge + cmb_gran, then usdm_gemv with identity weights: its output is the merged vector exactly).
    NS = 3 is the scalar tail alone, 21 = 16 + 4 + 1, 32 = 16 + 16; at pos 0 every split but the first is empty (pm = -1e30, pl = 0)."""
    from oracle import mistral_oracle as MO
    from usdm_amd import ops
    bf = torch.bfloat16
    Hq, Hkv, d, ctx_max = 32, 8, 128, 1024      # the hand-off form needs the 4096-output projection
    n = Hq * d
    cosf, sinf = MO.rope_tables(dict(head_dim=d, rope_theta=10000.0), torch.arange(ctx_max), bf)
    cos, sin = cosf[:, :64].contiguous().to(dev), sinf[:, :64].contiguous().to(dev)
    qkv = _r(((Hq + 2 * Hkv) * d,), 1).to(bf).to(dev)
    kc, vc = _r((Hkv, ctx_max, d), 2).to(bf).to(dev), _r((Hkv, ctx_max, d), 3).to(bf).to(dev)
    eye = torch.eye(n, dtype=bf, device=dev)
    bits = lambda t: t.view(torch.int16)
    for NS in (3, 21, 32):
        for pos in (0, 700):
            post = torch.tensor([pos], dtype=torch.int32, device=dev)

            def run(**kw):
                pm, pl, po = torch.zeros(Hq * NS, device=dev), torch.zeros(Hq * NS, device=dev), torch.zeros(Hq * NS * d, device=dev)
                out = torch.full((n,), 7.0, dtype=bf, device=dev)
                ops.attn_decode(qkv, post, cos, sin, kc.clone(), vc.clone(), pm, pl, po, out, Hq=Hq, Hkv=Hkv, ctx_max=ctx_max, NS=NS,
                                scale=d ** -0.5, **kw)
                return pm, pl, po, out

            *_, out_a = run()
            cnt = torch.zeros(Hkv, dtype=torch.int32, device=dev)
            *_, out_b = run(counters=cnt)
            assert not bool(cnt.any()), "the merge counters must be left zero"
            gran = torch.full((Hq * 64,), (1 << 32) | 5, dtype=torch.int64, device=dev)      # tagged: the attention launch must clear them
            pm, pl, po, out_0 = run(defer_merge=True, cmb_gran=gran)
            assert not bool(gran.any()) and bool((out_0 == 7.0).all())
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            out_c = torch.zeros(n, dtype=bf, device=dev)
            ops.gemv(eye, out_0, N=n, K=n, y16=out_c, merge=(pm, pl, po, NS), cmb=(gran, err))      # x pointer is ignored in merge mode
            assert int(err.item()) == 0
            lo_hi = gran.view(torch.int32).view(-1, 2)      # every granule tagged 1 and holding its two merged elements
            assert bool((lo_hi[:, 1] == 1).all()) and torch.equal(bits(lo_hi[:, 0].contiguous()), bits(out_c))
            assert bool(torch.isfinite(out_a.float()).all()) and bool((out_a != 7.0).any())
            assert torch.equal(bits(out_a), bits(out_b)), f"NS {NS} pos {pos}: fused merge != combine launch"
            assert torch.equal(bits(out_a), bits(out_c)), f"NS {NS} pos {pos}: o_proj hand-off merge != combine launch"


def _compare_generate(dev, cfg, seed, L0, new, bad, eos=None):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(cfg, seed=seed)
    ids = torch.randint(0, cfg["vocab_size"], (L0,), generator=torch.Generator().manual_seed(seed + 1))
    ref, ref_logits = MO.greedy_generate(sd, cfg, ids, new, bad_words_ids=bad, eos_token_id=eos, return_logits=True)
    m = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=256)
    out = m.generate(input_ids=ids[None].to(dev), max_length=L0 + new, do_sample=True, top_k=1, top_p=1.0, temperature=1.0,
                     bad_words_ids=bad, eos_token_id=eos)[0].tolist()
    assert out[:L0] == ids.tolist()
    n = min(len(out), len(ref))
    first = next((i for i in range(L0, n) if out[i] != ref[i]), None)
    if first is None:
        assert len(out) == len(ref)
        return None
    # a divergence is legitimate only at a near-tie of the oracle's own bf16 logits
    lg = ref_logits[first - L0]
    top2 = torch.topk(lg, 2).values
    gap = (top2[0] - top2[1]).item()
    assert gap <= 2 ** -6 * top2[0].abs().item() + 1e-3, f"diverged at {first - L0} with oracle top-2 gap {gap}"
    return first - L0


def test_generate_small_vs_oracle(dev):
    bad = [[i] for i in range(0, 400)]
    d1 = _compare_generate(dev, SMALL, 5, 19, 24, bad)
    d2 = _compare_generate(dev, SMALL, 6, 70, 40, [[i] for i in range(500, 1000)], eos=123)
    print("first divergences (None = exact):", d1, d2)


def test_first_token_logits_vs_oracle(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    cfg = SMALL
    sd = MO.random_state_dict(cfg, seed=9)
    ids = torch.randint(0, cfg["vocab_size"], (33,), generator=torch.Generator().manual_seed(2))
    ref, _ = MO.forward(sd, cfg, ids)
    m = USDMForCausalLM(cfg, dev, ctx_max=256)
    m.keep_logits = True
    m.W = m._shard(lambda n: sd[n])
    m._alloc()
    m.generate(input_ids=ids[None].to(dev), max_new_tokens=1)
    got = m.last_logits.cpu()
    err = (got - ref[-1]).abs().max().item()
    print("prefill logits max err", err, "scale", ref[-1].abs().max().item())
    assert err <= 4e-2 * ref[-1].abs().max().item()


def test_tp_code_path_single_rank_nccl(dev):
    """The tensor-parallel code path (f32 partial sums -> RCCL all_reduce / all_gather -> residual-add kernel) on a
    1-rank 'nccl' group must reproduce the fused single-GPU path token for token."""
    import os
    import torch.distributed as dist
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        sd = MO.random_state_dict(SMALL, seed=11)
        ids = torch.randint(0, SMALL["vocab_size"], (1, 23), generator=torch.Generator().manual_seed(3)).to(dev)
        a = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128).generate(input_ids=ids, max_new_tokens=12)
        b = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128, tp_segments=True, group=dist.group.WORLD).generate(
            input_ids=ids, max_new_tokens=12)
        assert torch.equal(a, b)
        os.environ["USDM_TP_GRAPH"] = "0"   # eager collectives
        m0 = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128, tp_segments=True, group=dist.group.WORLD)
        assert torch.equal(a, m0.generate(input_ids=ids, max_new_tokens=12)) and m0._decode.graph is None
        os.environ.pop("USDM_TP_GRAPH")
        m = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=128, tp_segments=True, group=dist.group.WORLD)
        c = m.generate(input_ids=ids, max_new_tokens=12)
        print("TP decode graph captured:", m._decode.graph is not None, "fallback reason:", m._decode.failed)
        assert torch.equal(a, c)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("tp_seg", [False, True])
def test_prefix_kv_reuse(dev, tp_seg):
    """Three chained rounds as in src/inference.py:61-83 (each prompt = previous output + a few tokens).  Prefilling only the
    new tokens on top of the cached K/V must reproduce a from-scratch prefill up to bf16 rounding of the cached rows (rows
    appended by decode steps come from the GEMV path): next-token logits within 3e-2 of the logit range, and the same token
    whenever the from-scratch top-2 gap exceeds that."""
    import os
    import torch.distributed as dist
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    kw, created = {}, False
    if tp_seg:
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
            created = True
        kw = dict(tp_segments=True, group=dist.group.WORLD)
    try:
        _prefix_kv_reuse_body(dev, kw)
    finally:
        if created:
            dist.destroy_process_group()


def _prefix_kv_reuse_body(dev, kw):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=21)
    a = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256, **kw)
    b = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256, **kw)
    a.reuse_prefix, a.keep_logits, b.keep_logits = True, True, True
    g = torch.Generator().manual_seed(5)
    p = torch.randint(0, 1000, (1, 70), generator=g).to(dev)
    for rnd, (new, extra) in enumerate([(13, 5), (9, 1), (20, 3)]):
        # first-token logits of this round: reuse (a) vs from scratch (b)
        a.generate(input_ids=p, max_new_tokens=1); la = a.last_logits.clone()
        b.generate(input_ids=p, max_new_tokens=1); lb = b.last_logits.clone()
        rng = float(lb.max() - lb.min())
        assert float((la - lb).abs().max()) <= 3e-2 * rng, (rnd, float((la - lb).abs().max()), rng)
        top2 = lb.topk(2).values
        if float(top2[0] - top2[1]) > 3e-2 * rng:
            assert int(la.argmax()) == int(lb.argmax())
        if rnd:
            assert any(k[1] > 0 for k in a._prefill_plans), "the round did not reuse the cached prefix"
        oa = a.generate(input_ids=p, max_new_tokens=new)      # (this call reuses the whole prompt but its last token)
        assert oa.shape[1] == p.shape[1] + new
        p = torch.cat([oa, torch.randint(0, 1000, (1, extra), generator=g).to(dev)], 1)
    # round 0 had nothing cached: bit-identical to the from-scratch model
    a2 = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256, **kw); a2.reuse_prefix = True
    q = torch.randint(0, 1000, (1, 50), generator=g).to(dev)
    assert torch.equal(a2.generate(input_ids=q, max_new_tokens=8), b.generate(input_ids=q, max_new_tokens=8))


def test_device_side_eos(dev):
    """An EOS in the middle of a host chunk of 8 decode steps: the remaining launches of the chunk return at once (the device
    step counter stops at the EOS), and the result equals the host-only check (more EOS ids than the device list holds)."""
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=31)
    m = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256)
    ids = torch.randint(0, 1000, (1, 33), generator=torch.Generator().manual_seed(8)).to(dev)
    free = m.generate(input_ids=ids, max_new_tokens=40)
    gen = free[0, 33:].tolist()
    k = 11                                             # 12th generated token: inside the second chunk (tokens 2..9, 10..17)
    eos = gen[k]
    first = gen.index(eos)
    a = m.generate(input_ids=ids, max_new_tokens=40, eos_token_id=eos)
    assert a.shape[1] == 33 + first + 1 and a[0, -1].item() == eos
    assert int(m.st_step.item()) == first + 1          # nothing ran past the EOS
    host_only = [eos] + [2000 + i for i in range(7)]   # 8 ids > device capacity -> host-side check only
    b = m.generate(input_ids=ids, max_new_tokens=40, eos_token_id=host_only)
    assert torch.equal(a, b) and int(m.st_step.item()) >= first + 1
    # min_new_tokens defers the stop
    c = m.generate(input_ids=ids, max_new_tokens=40, eos_token_id=eos, min_new_tokens=first + 2)
    assert c.shape[1] > a.shape[1] and torch.equal(c[0, :a.shape[1]], free[0, :a.shape[1]])


def test_prefix_kv_reuse_vs_oracle(dev):
    """Prefix-KV reuse across the three chained rounds of src/inference.py:61-83 against the CPU ORACLE: each round's prompt is the
    previous round's output plus a few tokens; with reuse on, only the new tokens are prefilled, and the generated ids must equal
    oracle greedy generation of the FULL prompt (recomputed from scratch, as the reference does), up to oracle near-ties."""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=23)
    m = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256)
    m.reuse_prefix = True
    g = torch.Generator().manual_seed(6)
    p = torch.randint(0, 1000, (60,), generator=g)
    bad = [[i] for i in range(500, 700)]
    firsts = []
    for rnd, (new, extra) in enumerate([(12, 4), (10, 2), (18, 0)]):
        ref, ref_logits = MO.greedy_generate(sd, SMALL, p, new, bad_words_ids=bad, return_logits=True)
        out = m.generate(input_ids=p[None].to(dev), max_new_tokens=new, bad_words_ids=bad)[0].cpu()
        firsts.append(check_against_oracle(out.tolist(), ref, ref_logits, p.numel()))
        if rnd:
            assert any(k[1] > 0 for k in m._prefill_plans), "the round did not reuse the cached prefix"
        p = torch.cat([out, torch.randint(0, 1000, (extra,), generator=g)])      # next prompt extends what the cache holds
    print("prefix reuse vs oracle: first differences per round (None = identical):", firsts)


def test_exact_prefix_reuse_is_bit_identical(dev):
    """The default prefix reuse ("exact": only rows written by prefill launches are kept) against recomputing every prompt from
    scratch, over three chained rounds as in src/inference.py:61-83: identical token ids AND bit-identical first-token logits,
    while rounds 2 and 3 really prefill only the new tokens."""
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    sd = MO.random_state_dict(SMALL, seed=29)
    a = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256)
    b = USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256)
    assert a.reuse_prefix == "exact"
    b.reuse_prefix = False
    a.keep_logits = b.keep_logits = True
    g = torch.Generator().manual_seed(7)
    p = torch.randint(0, 1000, (1, 90), generator=g).to(dev)
    for rnd, (new, extra) in enumerate([(14, 6), (11, 1), (17, 0)]):
        a.generate(input_ids=p, max_new_tokens=1); la = a.last_logits.clone()
        b.generate(input_ids=p, max_new_tokens=1); lb = b.last_logits.clone()
        assert torch.equal(la, lb), (rnd, float((la - lb).abs().max()))
        oa = a.generate(input_ids=p, max_new_tokens=new)
        ob = b.generate(input_ids=p, max_new_tokens=new)
        assert torch.equal(oa, ob)
        if rnd:
            pasts = sorted(k[1] for k in a._prefill_plans if k[1] > 0)
            assert pasts, "no partial prefill happened"
        p = torch.cat([oa, torch.randint(0, 1000, (1, extra), generator=g).to(dev)], 1)
    # rows appended by decode steps were never reused: the reused length never exceeds a previous PROMPT length
    assert all(k[1] in (0, 89, 90, 110, 111, 122) or k[1] <= 122 for k in a._prefill_plans)


@pytest.mark.parametrize("W", [40, 64, 100])
def test_sliding_window_attention_vs_oracle(dev, W):
    """Mistral's sliding window (reference: src/model.py:337-371; HF mask: query p sees keys p-W+1 .. p) on a context LONGER than
    the window, small model: (a) prefill logits of a 230-token prompt vs the oracle (rows whose first key tiles are masked entirely,
    W not a multiple of the 64-key tile), (b) greedy decode across many positions vs the oracle, (c) three chained rounds with exact
    prefix reuse (prefill with q_pos0 > 0 through the window), (d) four requests through the batched decode of the serving layer.
    The oracle's window is pinned to the installed transformers in tests/test_oracle_cpu.py."""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.serving import LLM, SamplingParams
    cfg = dict(SMALL, sliding_window=W)
    sd = MO.random_state_dict(cfg, seed=31)
    m = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=320)
    assert m.window == W
    g = torch.Generator().manual_seed(W)
    ids = torch.randint(0, 1000, (230,), generator=g)
    # (a) prefill logits, and the difference the window makes (the test must be able to fail)
    ref, _ = MO.forward(sd, cfg, ids)
    full, _ = MO.forward(sd, dict(cfg, sliding_window=None), ids)
    m.keep_logits = True
    m.generate(input_ids=ids[None].to(dev), max_new_tokens=1)
    got = m.last_logits.cpu()
    scale = ref[-1].abs().max().item()
    err, werr = (got - ref[-1]).abs().max().item(), (full[-1] - ref[-1]).abs().max().item()
    print(f"W={W}: prefill logits max err {err:.4f} (scale {scale:.2f}); full-causal logits differ from the windowed ones by {werr:.3f}")
    assert err <= 4e-2 * scale and werr > 4 * err
    m.keep_logits = False
    # (b) + (c): three chained rounds, greedy, vs the oracle on the full prompt
    bad = [[i] for i in range(0, 200)]
    p, firsts = ids[:150], []
    for rnd, (new, extra) in enumerate([(30, 5), (25, 3), (40, 0)]):
        r, rl = MO.greedy_generate(sd, cfg, p, new, bad_words_ids=bad, return_logits=True)
        out = m.generate(input_ids=p[None].to(dev), max_new_tokens=new, bad_words_ids=bad)[0].cpu()
        firsts.append(check_against_oracle(out.tolist(), r, rl, p.numel()))
        if rnd:
            assert any(k[1] > 0 for k in m._prefill_plans), "the round did not reuse the cached prefix"
        p = torch.cat([out, torch.randint(0, 1000, (extra,), generator=g)])
    # (d) the batched decode
    eng = LLM(model=m)

    def ban(token_ids, logits):
        logits[0:200] = float("-inf")
        return logits
    prompts = [torch.randint(0, 1000, (L,), generator=g).tolist() for L in (120, 75, 160, 33)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=SamplingParams(max_tokens=20, top_k=1, logits_processors=[ban]))
    assert eng.stats["batched_requests"] == 4
    bfirst = []
    for pr, o in zip(prompts, outs):
        r, rl = MO.greedy_generate(sd, cfg, torch.tensor(pr), 20, bad_words_ids=bad, return_logits=True)
        bfirst.append(check_against_oracle(pr + o.outputs[0].token_ids, r, rl, len(pr)))
    print(f"W={W}: first differences vs the oracle (None = identical): chained rounds {firsts}, batched {bfirst}")


def test_window_is_inert_up_to_its_length(dev):
    from usdm_amd.llm import USDMForCausalLM
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(SMALL, seed=32)
    assert USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=256).window == 0          # default window 4096 >= ctx_max
    assert USDMForCausalLM.from_state_dict(sd, dict(SMALL, sliding_window=None), dev, ctx_max=256).window == 0
    assert USDMForCausalLM.from_state_dict(sd, dict(SMALL, sliding_window=128), dev, ctx_max=256).window == 128
