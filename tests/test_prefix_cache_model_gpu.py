"""GPU: prefix caching (enable_prefix_caching) through the model and the serving layer, SMALL model, ctx_max = 256.
bf16 cache: a row of the prefill path does not depend on its company and the decode steps are deterministic, so every result with
the option on equals the option-off result exactly (==).  FP8 cache: the extended 8d contract - the model equals the bf16-cache
model whose rows are round-tripped before a later step or a later call reads them - checked bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
CTX = 256


@pytest.fixture(scope="module")
def sd():
    from oracle import mistral_oracle as MO
    return MO.random_state_dict(SMALL, seed=29)


def _model(sd, dev, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.from_state_dict(sd, SMALL, dev, ctx_max=CTX, **kw)


def _rand(g, n):
    return torch.randint(0, 1000, (n,), generator=g).tolist()


def _same_logprobs(x, y):
    return (torch.equal(x.token_logprobs, y.token_logprobs) and torch.equal(x.ranks, y.ranks) and torch.equal(x.top_ids, y.top_ids)
            and torch.equal(x.top_logprobs, y.top_logprobs))


# ------------------------------------------------------------------------------------------------------------------ generate_batch
@pytest.mark.parametrize("B", [3, 5])      # the VALU step and the matrix-core step
def test_three_chained_rounds_through_generate_batch(dev, sd, B):
    """the rounds of tests/test_llm_gpu.py::test_exact_prefix_reuse_is_bit_identical, B sequences at once"""
    on, off = _model(sd, dev, enable_prefix_caching=True), _model(sd, dev)
    g = torch.Generator().manual_seed(7 + B)
    prompts = [torch.tensor([_rand(g, 90)], device=dev) for _ in range(B)]
    earlier = set()
    for rnd, (new, extra) in enumerate([(14, 6), (11, 1), (17, 0)]):
        oa = on.generate_batch(prompts, new, logprobs=20)
        la = on.last_logprobs
        ob = off.generate_batch(prompts, new, logprobs=20)
        for b in range(B):
            assert oa[b].tolist() == ob[b].tolist(), (rnd, b)
            assert _same_logprobs(la[b], off.last_logprobs[b]), (rnd, b)
        pasts = [k[1] for k in on._batches[B].prefill]
        if rnd == 0:
            assert not any(pasts) and on.stats["prefix_hits"] == 0 and on.stats["prefill_rows"] == B * 90
        else:
            assert on.stats["prefix_hits"] == rnd * B, "a round did not reuse its cached prefix"
        # rows appended by decode steps are never reused: a past is an earlier PROMPT's length
        assert all(p == 0 or p in earlier for p in pasts), (pasts, earlier)
        earlier |= {int(p.shape[1]) for p in prompts}
        prompts = [torch.cat([o, torch.tensor([_rand(g, extra)], dtype=torch.long, device=dev)], 1) for o in oa]
    assert sorted({k[1] for k in on._batches[B].prefill}) == [0, 90, 110]
    assert on.stats["prefix_rows_reused"] == B * (90 + 110) and on.stats["prefix_copies"] == 0      # every sequence found its rows in its own slot
    assert all(k[1] == 0 for k in off._batches[B].prefill) and off._batches[B].prefix is None and not off.stats


# ------------------------------------------------------------------------------------------------------------------ serving
def _replay(log, nslots):
    """what the CPU index predicts for an admission order: [(source, past)]"""
    from usdm_amd.prefix import PrefixIndex
    px, out = PrefixIndex(nslots, CTX), []
    for slot, ids in log:
        out.append(px.match(list(ids), slot))
        px.admit(slot, ids)
    return out


def _tokens(outs):
    return [[(c.token_ids, c.finish_reason) for c in o.outputs] for o in outs]


def test_serving_reuses_prefixes_across_slots_and_calls(dev, sd):
    from usdm_amd.serving import LLM, SamplingParams
    on = LLM(model=_model(sd, dev, enable_prefix_caching=True), max_num_seqs=4, enable_prefix_caching=True)
    off = LLM(model=_model(sd, dev), max_num_seqs=4)
    g = torch.Generator().manual_seed(3)
    f40, f64, f100 = _rand(g, 40), _rand(g, 64), _rand(g, 100)
    # ten requests on four slots: three families sharing 40-, 64- and 100-token prefixes and two unrelated prompts; the first four are
    # admitted at once, so 1 finds its prefix in slot 0 and 3 in slot 2 while those still decode
    prompts = [f40 + _rand(g, 9), f40 + _rand(g, 21), f64 + _rand(g, 5), f64 + _rand(g, 30), _rand(g, 57), f100 + _rand(g, 3),
               f40 + _rand(g, 2), _rand(g, 33), f100 + _rand(g, 17), f64 + _rand(g, 1)]
    greedy = lambda n: SamplingParams(max_tokens=n, top_k=1)
    sampled = lambda n, s: SamplingParams(max_tokens=n, temperature=0.8, top_k=50, top_p=0.9, seed=s)
    sps = [greedy(20), sampled(9, 11), greedy(12), sampled(25, 12), greedy(7), sampled(18, 13), greedy(10), sampled(14, 14), greedy(22), sampled(6, 15)]
    ra, rb = on.generate(prompt_token_ids=prompts, sampling_params=sps), off.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert _tokens(ra) == _tokens(rb)
    st = on.stats
    assert st["batched_requests"] == 10 and st["admissions"] == 10 and off.stats["admissions"] == 10
    # (requests 1, 3, 6, 8 and 9 find their family's prefix as long as no admission in between replaced the slot's entry: the replay
    # below says exactly which did)
    assert st["prefix_hits"] >= 3 and st["prefix_copies"] > 0 and st["prefix_hits_live"] > 0
    # a second call whose prompts extend the first call's prompts: those the four slots hold now, in slot order (the first four
    # admissions go to slots 0 .. 3) - as prompt + what was generated + new tokens, or prompt + new tokens - and a fifth of slot 0's family
    px = on.llm._batches[4].prefix
    held = [list(e) for e in px.entries]
    assert all(h in prompts for h in held)
    more = [h + ra[prompts.index(h)].outputs[0].token_ids + _rand(g, 4) for h in held[:2]] + [held[2] + _rand(g, 6), held[3] + _rand(g, 11)]
    more.append(held[0] + _rand(g, 9))
    sps2 = [greedy(8), sampled(8, 21), greedy(5), sampled(12, 22), greedy(9)]
    assert _tokens(on.generate(prompt_token_ids=more, sampling_params=sps2)) == _tokens(off.generate(prompt_token_ids=more, sampling_params=sps2))
    pred = _replay(on.admission_log, 4)
    assert len(pred) == 15
    assert st["prefix_rows_reused"] == sum(p for _, p in pred) and st["prefix_hits"] == sum(p > 0 for _, p in pred)
    assert st["prefix_copies"] == sum(s is not None and s != slot for (s, _), (slot, _) in zip(pred, on.admission_log))
    assert st["prefill_rows"] == sum(len(i) for _, i in on.admission_log) - st["prefix_rows_reused"]
    assert sum(p > 0 for _, p in pred[10:]) == 5, "an extending prompt of the second call found nothing"
    # idle slots: two requests on the four slots, unrelated to everything cached - slots 2 and 3 idle through the whole call, parked
    # behind their recorded rows ...
    px = on.llm._batches[4].prefix
    kept = [list(px.entries[2]), list(px.entries[3])]
    assert all(len(k) >= 16 for k in kept)
    two = [_rand(g, 45), _rand(g, 38)]
    sp = [greedy(20), sampled(20, 31)]
    assert _tokens(on.generate(prompt_token_ids=two, sampling_params=sp)) == _tokens(off.generate(prompt_token_ids=two, sampling_params=sp))
    assert [list(px.entries[2]), list(px.entries[3])] == kept and [px.park(2), px.park(3)] == [len(kept[0]), len(kept[1])]
    # ... so a call that extends THEIR prompts still reuses their rows (parked at 0 they would have decoded garbage into rows 0 .. 7)
    before = dict(st)
    ext = [kept[0] + _rand(g, 5), kept[1] + _rand(g, 8)]
    sp = [sampled(10, 41), greedy(10)]
    assert _tokens(on.generate(prompt_token_ids=ext, sampling_params=sp)) == _tokens(off.generate(prompt_token_ids=ext, sampling_params=sp))
    assert st["prefix_hits"] == before["prefix_hits"] + 2 and st["prefix_copies"] == before["prefix_copies"] + 2
    assert st["prefix_rows_reused"] == before["prefix_rows_reused"] + len(kept[0]) + len(kept[1])
    # reset_prefix_cache: nothing is reused afterwards
    assert on.reset_prefix_cache() and px.entries == [None] * 4
    before = dict(st)
    assert _tokens(on.generate(prompt_token_ids=ext, sampling_params=sp)) == _tokens(off.generate(prompt_token_ids=ext, sampling_params=sp))
    assert st["prefix_hits"] == before["prefix_hits"] and st["prefill_rows"] == before["prefill_rows"] + len(ext[0]) + len(ext[1])
    assert "prefix_hits" not in off.stats and not hasattr(off, "admission_log")


def test_n_copies_prefill_one_row_each(dev, sd):
    from usdm_amd.serving import LLM, SamplingParams
    on = LLM(model=_model(sd, dev, enable_prefix_caching=True), max_num_seqs=4, enable_prefix_caching=True)
    off = LLM(model=_model(sd, dev), max_num_seqs=4)
    prompt = _rand(torch.Generator().manual_seed(9), 50)
    sp = SamplingParams(n=3, max_tokens=10, temperature=0.9, top_k=40, seed=5)
    ra, rb = on.generate(prompt_token_ids=[prompt], sampling_params=sp), off.generate(prompt_token_ids=[prompt], sampling_params=sp)
    assert len(ra[0].outputs) == 3 and _tokens(ra) == _tokens(rb)
    assert len({tuple(c.token_ids) for c in ra[0].outputs}) > 1, "the copies did not draw from their own streams"
    st = on.stats
    assert st["prefill_rows"] == 50 + 1 + 1 and st["prefix_rows_reused"] == 2 * 49 and st["prefix_copies"] == 2 and st["prefix_hits_live"] == 2
    assert sorted(k[:2] for k in on.llm._batches[4].prefill) == [(1, 49), (1, 49), (50, 0)]


def test_model_object_without_the_flag_is_refused_by_the_engine(dev, sd):
    from usdm_amd.serving import LLM
    with pytest.raises(ValueError, match="enable_prefix_caching"):
        LLM(model=_model(sd, dev), enable_prefix_caching=True)


# ------------------------------------------------------------------------------------------------------------------ fp8 cache
def _roundtrip_rows(t, lo, hi):
    """rows [lo, hi) of a bf16 cache [..., ctx, 128] round-tripped in place (on the CPU: quant.py's exact definition)"""
    from usdm_amd.quant import roundtrip_kv_rows
    t[..., lo:hi, :] = roundtrip_kv_rows(t[..., lo:hi, :].cpu()).to(t.device)


def _admit(m, bb_b, b, ids, kind):
    ds = m.decode_slots(bb_b)
    ds.require(kind)
    return ds.admit(b, torch.tensor(ids, dtype=torch.long), kind), ds      # (sampling=None: greedy on the sampling step)


def test_fp8_cache_contract_on_the_batch_slots(dev, sd):
    from usdm_amd.llm import read_logprobs, step_kind
    from usdm_amd.quant import dequantize_kv_rows, quantize_kv_rows, roundtrip_kv_rows
    A = _model(sd, dev, kv_cache_dtype="fp8", enable_prefix_caching=True)
    Bm = _model(sd, dev, enable_prefix_caching=True)
    kind = step_kind(logprobs=20)
    g = torch.Generator().manual_seed(13)
    p1 = _rand(g, 90)
    (_, pa), ba = _admit(A, 2, 0, p1, kind)
    (_, pb), bb = _admit(Bm, 2, 0, p1, kind)
    torch.cuda.synchronize()
    assert pa == pb == 0
    # 2. the rows A holds are the round-tripped rows of B
    for c8, ce, cb in (("kc", "ke", "kc"), ("vc", "ve", "vc")):
        got = dequantize_kv_rows(getattr(ba, c8)[0, :, :, :90].cpu(), getattr(ba, ce)[0, :, :, :90].cpu())
        want = roundtrip_kv_rows(getattr(bb, cb)[0, :, :, :90].cpu())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool(want.any())
    # 3. B reads its rows as an fp8 cache would return them
    for name in ("kc", "vc"):
        _roundtrip_rows(getattr(bb, name)[0], 0, 90)
    # 4. / 5. the prompt + 12 tokens: both reuse the 90 rows of their own slot; first token, its log-probability and the top 20 are equal
    p2 = p1 + _rand(g, 12)
    (sa, pa), _ = _admit(A, 2, 0, p2, kind)
    (sb, pb), _ = _admit(Bm, 2, 0, p2, kind)
    torch.cuda.synchronize()
    assert (sa, pa) == (sb, pb) == (0, 90)
    assert any(k[:2] == (12, 90) for k in ba.prefill) and any(k[:2] == (12, 90) for k in bb.prefill)
    assert int(ba.out[0, 0]) == int(bb.out[0, 0])
    la, lb = read_logprobs(ba.lp, 1, 20, 0), read_logprobs(bb.lp, 1, 20, 0)
    assert torch.equal(la.token_logprobs, lb.token_logprobs) and torch.equal(la.top_ids, lb.top_ids) and torch.equal(la.top_logprobs, lb.top_logprobs)
    # 6. the rows A appended are the quantized rows B appended; the reused rows are untouched
    for c8, ce, cb in (("kc", "ke", "kc"), ("vc", "ve", "vc")):
        q, e = quantize_kv_rows(getattr(bb, cb)[0, :, :, 90:102].cpu())
        assert torch.equal(getattr(ba, c8)[0, :, :, 90:102].cpu(), q) and torch.equal(getattr(ba, ce)[0, :, :, 90:102].cpu(), e)
    # ... and once more through the other slot: rows, bytes and exponents copied from slot 0 (usdm_kv_reorder), three rows prefilled
    for name in ("kc", "vc"):
        _roundtrip_rows(getattr(bb, name)[0], 90, 102)
    p3 = p2 + _rand(g, 3)
    (sa, pa), _ = _admit(A, 2, 1, p3, kind)
    (sb, pb), _ = _admit(Bm, 2, 1, p3, kind)
    torch.cuda.synchronize()
    assert (sa, pa) == (sb, pb) == (0, 102)
    assert torch.equal(ba.kc[1, :, :, :102], ba.kc[0, :, :, :102]) and torch.equal(ba.ve[1, :, :, :102], ba.ve[0, :, :, :102])
    assert int(ba.out[1, 0]) == int(bb.out[1, 0])
    la, lb = read_logprobs(ba.lp, 1, 20, 1), read_logprobs(bb.lp, 1, 20, 1)
    assert torch.equal(la.token_logprobs, lb.token_logprobs) and torch.equal(la.top_ids, lb.top_ids) and torch.equal(la.top_logprobs, lb.top_logprobs)


def _rt_hook(b):
    """_logits_hook of the bf16-cache model: every cache row written so far, and its image in the persistent V^T, round-tripped before
    a later step - or, with prefix reuse, a later call - reads it"""
    from usdm_amd.quant import roundtrip_kv_rows

    def hook():
        n = min(int(b.st_pos.item()) + 1, b.ctx_max)
        b.kcache[:, :, :n] = roundtrip_kv_rows(b.kcache[:, :, :n])
        b.vcache[:, :, :n] = roundtrip_kv_rows(b.vcache[:, :, :n])
        b.vtc[:, :, :, :n] = b.vcache[:, :, :n].transpose(2, 3)
    return hook


def test_fp8_cache_contract_on_the_single_sequence(dev, sd):
    A = _model(sd, dev, kv_cache_dtype="fp8", enable_prefix_caching=True)
    Bm = _model(sd, dev)
    assert A.reuse_prefix == "exact" and A.vtc is None and Bm.reuse_prefix == "exact"
    A.keep_logits = Bm.keep_logits = True
    g = torch.Generator().manual_seed(17)
    noop, hook = (lambda: None), _rt_hook(Bm)
    p = torch.tensor([_rand(g, 80)], device=dev)
    kw = dict(max_new_tokens=6, seed=5)
    ra, rb = A.generate(input_ids=p, _logits_hook=noop, **kw), Bm.generate(input_ids=p, _logits_hook=hook, **kw)
    assert torch.equal(ra, rb)
    # generate() round 2: the 80 prompt rows are reused (exact rule: not the 5 rows the decode steps appended), as the cache holds them
    p2 = torch.cat([ra, torch.tensor([_rand(g, 3)], device=dev)], 1)
    ra, la = A.generate(input_ids=p2, _logits_hook=noop, **kw), A.last_logits.clone()
    rb = Bm.generate(input_ids=p2, _logits_hook=hook, **kw)
    assert torch.equal(ra, rb) and torch.equal(la, Bm.last_logits)
    assert [k[:2] for k in A._prefill_plans if k[1]] == [(9, 80)] and [k[:2] for k in Bm._prefill_plans if k[1]] == [(9, 80)]
    # score(): three candidates behind one 80-token context; the first call prefills everything, the others their own rows only
    ctx = _rand(g, 80)
    cands = [_rand(g, 6), _rand(g, 4), _rand(g, 9)]
    for i, c in enumerate(cands):
        ids = torch.tensor([ctx + c], device=dev)
        sa = A.score(ids, top_logprobs=5, start=81)
        sb = Bm.score(ids, top_logprobs=5, start=81)
        assert torch.equal(sa.token_logprobs, sb.token_logprobs) and torch.equal(sa.ranks, sb.ranks), i
        assert torch.equal(sa.top_ids, sb.top_ids) and torch.equal(sa.top_logprobs, sb.top_logprobs), i
        n = 80 + len(c)      # B's rows of this call, as the fp8 cache returns them to the next one
        _roundtrip_rows(Bm.kcache, 0, n)
        _roundtrip_rows(Bm.vcache, 0, n)
        Bm.vtc[:, :, :, :n] = Bm.vcache[:, :, :n].transpose(2, 3)
    assert sorted(k[:3] for k in A._score_plans) == [(4, 80, 0), (9, 80, 0), (86, 0, 80)]


def test_fp8_cache_without_the_flag_reuses_nothing(dev, sd):
    m = _model(sd, dev, kv_cache_dtype="fp8")
    assert m.reuse_prefix is False and not m.prefix_caching
    g = torch.Generator().manual_seed(19)
    p = torch.tensor([_rand(g, 60)], device=dev)
    out = m.generate(input_ids=p, max_new_tokens=5)
    m.generate(input_ids=torch.cat([out, torch.tensor([_rand(g, 3)], device=dev)], 1), max_new_tokens=5)
    ids = torch.tensor([_rand(g, 40)], device=dev)
    m.score(ids, start=30)
    m.score(torch.cat([ids, ids[:, :4]], 1), start=41)
    two = [p, torch.tensor([_rand(g, 50)], device=dev)]
    outs = m.generate_batch(two, 4)
    m.generate_batch([torch.cat([o, o[:, :2]], 1) for o in outs], 4)
    assert all(k[1] == 0 for k in m._prefill_plans) and all(k[1] == 0 for k in m._score_plans)
    assert all(k[1] == 0 for k in m._batches[2].prefill) and m._batches[2].prefix is None


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, sd, monkeypatch):
    from usdm_amd.llm import USDMForCausalLM
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        USDMForCausalLM(SMALL, dev, ctx_max=CTX, tp_segments=True, enable_prefix_caching=True)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        USDMForCausalLM(SMALL, dev, ctx_max=CTX, tp_size=2, tp_rank=0, enable_prefix_caching=True)
    monkeypatch.setenv("USDM_PREFIX_REUSE", "0")
    with pytest.raises(ValueError, match="USDM_PREFIX_REUSE"):
        _model(sd, dev, enable_prefix_caching=True)
    _model(sd, dev)      # without the flag the variable keeps its meaning
