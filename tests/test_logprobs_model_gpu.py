"""Per-token log-probabilities through the model (USDMForCausalLM.generate(logprobs=K)) and the serving surface
(SamplingParams(logprobs=K)) on small synthetic models.  Ground truth without a new oracle: the eager hook path exposes the logits
row of every step (the prefill's included); every reported row must equal the float64 reference on it (tests/_logprob_reference:
ids and ranks exactly, values within the kernel tolerance derived there), and the captured-graph path must equal the hook path
bit for bit."""
import numpy as np
import pytest
import torch

from tests import _logprob_reference as R

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
BAD = [[i] for i in range(250)]


def _model(dev, seed=5, cfg=SMALL, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.random_init(cfg, dev, seed=seed, ctx_max=256, **kw)


def _prompt(dev, n=40, seed=1):
    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _same(a, b):
    return all(torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32))
               for f in ("token_logprobs", "ranks", "top_ids", "top_logprobs")) and a.cumulative == b.cumulative


def _check_rows(lp, toks, rows, K, tol):
    assert lp.token_logprobs.shape == (len(toks),) and lp.top_ids.shape == (len(toks), K) and len(rows) >= len(toks)
    for t, tok in enumerate(toks):
        R.check_row(rows[t], tok, lp.token_logprobs[t], lp.ranks[t], lp.top_ids[t], lp.top_logprobs[t], K, tol)
    assert lp.cumulative == float(lp.token_logprobs.double().sum())


@pytest.mark.parametrize("sampled", [False, True])
def test_generate_rows_match_the_hooked_logits_and_the_graph_path(dev, sampled):
    m, ids, K, tol = _model(dev), _prompt(dev), 5, R.kernel_tolerance()
    kw = dict(input_ids=ids, max_new_tokens=12, bad_words_ids=BAD)
    if sampled:
        kw.update(do_sample=True, temperature=1.3, top_k=50, top_p=0.9, seed=11)
    rows = []
    out_h = m.generate(_logits_hook=lambda: rows.append(m.last_logits.cpu().numpy().copy()), logprobs=K, **kw)
    toks, lp_h = out_h[0, 40:].tolist(), m.last_logprobs
    assert len(toks) == 12 and len(rows) == 12
    _check_rows(lp_h, toks, rows, K, tol)                      # the first token (picked by the prefill) included
    out_g = m.generate(logprobs=K, **kw)                       # captured graph: same ids, the same bits
    assert torch.equal(out_g, out_h) and _same(m.last_logprobs, lp_h)
    if not sampled:
        assert (lp_h.ranks == 1).all()
        plain = m.generate(**kw)                               # the arg-max path: ids unchanged by logprobs=, nothing reported
        assert torch.equal(plain, out_g) and m.last_logprobs is None
        m.generate(logprobs=0, **kw)
        assert m.last_logprobs.top_ids.shape == (12, 0) and torch.equal(m.last_logprobs.token_logprobs, lp_h.token_logprobs)
    with pytest.raises(ValueError, match="logprobs"):
        m.generate(logprobs=21, **kw)


def test_device_side_eos_keeps_the_stop_tokens_row(dev):
    m, ids, K = _model(dev), _prompt(dev), 3
    kw = dict(input_ids=ids, bad_words_ids=BAD, logprobs=K)
    full = m.generate(max_new_tokens=14, **kw)[0, 40:].tolist()
    lp_full = m.last_logprobs
    eos = full[4]
    j = full.index(eos)
    cut = m.generate(max_new_tokens=14, eos_token_id=eos, **kw)[0, 40:].tolist()
    lp = m.last_logprobs
    assert cut == full[:j + 1] and int(m.st_done.item()) == 1
    assert lp.token_logprobs.shape[0] == j + 1 and _same(lp, lp_full.trimmed(j + 1, K))          # the last row is the stop token's
    assert int(lp.top_ids[j, 0]) == eos and int(lp.ranks[j]) == 1
    one = m.generate(max_new_tokens=1, **kw)[0, 40:].tolist()                                      # a single token: exactly one row
    assert one == full[:1] and _same(m.last_logprobs, lp_full.trimmed(1, K))


def test_generate_batch_equals_generate_per_sequence(dev):
    """generate_batch(logprobs=K) in the <= 4-slot form: every sequence's ids and log-probabilities are generate(logprobs=K)'s bit
    for bit, the ids are the plain greedy batch's, and the list keeps the prompts' order across groups (3 prompts in groups of 2,
    one of them ending early at a stop id)."""
    m, K = _model(dev), 4
    prompts = [_prompt(dev, n, seed) for n, seed in ((40, 1), (23, 2), (31, 3))]
    kw = dict(max_new_tokens=11, bad_words_ids=BAD)
    eos = m.generate(input_ids=prompts[0], **kw)[0, 40:].tolist()[3]
    kw["eos_token_id"] = eos
    plain = m.generate_batch(prompts, **kw)
    assert m.last_logprobs is None
    for group in (None, 2):
        outs = m.generate_batch(prompts, logprobs=K, group=group, **kw)
        lps = m.last_logprobs
        assert isinstance(lps, list) and len(lps) == len(outs) == 3
        for p, o, o_plain, lp in zip(prompts, outs, plain, lps):
            assert torch.equal(o, o_plain)                         # greedy ids unchanged by logprobs=
            alone = m.generate(input_ids=p, logprobs=K, **kw)
            n = o.shape[1] - p.shape[1]
            assert torch.equal(o, alone) and lp.token_logprobs.shape == (n,) and lp.top_ids.shape == (n, K)
            assert _same(lp, m.last_logprobs) and (lp.ranks == 1).all()
        assert outs[0].shape[1] - 40 <= 4 and int(outs[0][0, -1]) == eos and int(lps[0].top_ids[-1, 0]) == eos
    outs = m.generate_batch(prompts, logprobs=K, **dict(kw, max_new_tokens=0))      # nothing generated: no record per sequence
    assert m.last_logprobs == [None] * 3 and all(torch.equal(o, p) for o, p in zip(outs, prompts))
    with pytest.raises(ValueError, match="logprobs"):
        m.generate_batch(prompts, logprobs=-1, **kw)


def _requests(n, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [17 + (11 * i) % 40 for i in range(n)]
    return [torch.randint(0, 1000, (L,), generator=g).tolist() for L in lens]


def _params(i, stop=None):
    from usdm_amd.serving import SamplingParams
    ks = (5, None, 0, 20, 1, None, 5)
    max_tokens = (14, 9, 1, 21, 12, 6, 17)[i % 7]
    kw = dict(max_tokens=max_tokens, logprobs=ks[i % 7], ignore_eos=True, stop_token_ids=[stop] if stop is not None else None)
    if i % 2:
        return SamplingParams(temperature=0.7 + 0.1 * i, top_k=40 + i, top_p=0.95, seed=100 + i, **kw)
    return SamplingParams(top_k=1, **kw)


def test_serving_four_slots_equal_the_requests_served_alone(dev):
    from usdm_amd.serving import LLM
    eng = LLM(model=_model(dev, seed=7), max_num_seqs=4)
    prompts = _requests(7, 3)
    probe = eng.generate(prompt_token_ids=[prompts[4]], sampling_params=_params(4))[0].outputs[0].token_ids
    sps = [_params(i, stop=probe[3] if i == 4 else None) for i in range(7)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 7 and eng.stats["admissions"] == 7 and eng.stats["max_active"] == 4
    for i, (p, sp, o) in enumerate(zip(prompts, sps, outs)):
        got = o.outputs[0]
        alone = eng.generate(prompt_token_ids=[p], sampling_params=sp)[0].outputs[0]
        assert got.token_ids == alone.token_ids and got.finish_reason == alone.finish_reason, i
        if sp.logprobs is None:
            assert got.logprobs is None and got.cumulative_logprob is None
            continue
        assert got.logprobs == alone.logprobs and got.cumulative_logprob == alone.cumulative_logprob, i      # bit for bit
        assert len(got.logprobs) == len(got.token_ids) and all(len(d) in (sp.logprobs, sp.logprobs + 1) for d in got.logprobs)
    assert outs[4].outputs[0].finish_reason == "stop" and len(outs[4].outputs[0].token_ids) <= 4
    assert len(outs[2].outputs[0].token_ids) == 1 and len(outs[2].outputs[0].logprobs) == 1


def _consistent(o, sp):
    K, toks = sp.logprobs, o.token_ids
    assert len(o.logprobs) == len(toks)
    total = 0.0
    for tok, d in zip(toks, o.logprobs):
        pick = d[tok]
        total += pick.logprob
        assert np.isfinite(pick.logprob) and pick.rank >= 1 and all(e.logprob <= 0 for e in d.values())
        rest = [(i, e) for i, e in d.items() if i != tok]
        ranks = [e.rank for _, e in rest]
        gap = sorted(set(range(1, K + 1)) - set(ranks))            # the position the picked token takes in the top list, if any
        assert ranks == sorted(ranks) and len(gap) == (1 if len(d) == K else 0) and len(d) in (K, K + 1)
        full = sorted(rest + ([(tok, type(pick)(pick.logprob, gap[0]))] if gap else []), key=lambda ie: ie[1].rank)
        assert [e.rank for _, e in full] == list(range(1, K + 1))
        for (i0, e0), (i1, e1) in zip(full, full[1:]):
            assert e0.logprob > e1.logprob or (e0.logprob == e1.logprob and i0 < i1)      # descending, exact ties lowest id first
        if pick.rank <= K:      # it sits at its rank, or later among entries that tie with it exactly
            pos = gap[0] if gap else K + 1
            assert pos >= pick.rank and all(e.logprob == pick.logprob for _, e in full[pick.rank - 1:pos - 1])
        else:
            assert not gap
        if sp.greedy:
            assert pick.rank == 1
    assert o.cumulative_logprob == total


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_serving_sixteen_slots_outputs_are_consistent(dev, quant):
    from usdm_amd.serving import LLM
    kw = dict(quantization="fp8", fp8_matrix_cores=True, kv_cache_dtype="fp8") if quant else {}
    eng = LLM(model=_model(dev, seed=9, **kw), max_num_seqs=16)
    prompts = _requests(18, 5)
    sps = [_params(i) for i in range(18)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 18 and eng.stats["max_active"] == 16
    for sp, o in zip(sps, outs):
        got = o.outputs[0]
        assert 1 <= len(got.token_ids) <= sp.max_tokens
        if sp.logprobs is None:
            assert got.logprobs is None and got.cumulative_logprob is None
        else:
            _consistent(got, sp)


def test_n_completions_carry_their_own_logprobs(dev):
    from usdm_amd.serving import LLM, SamplingParams
    eng = LLM(model=_model(dev, seed=7), max_num_seqs=4)
    p = _requests(1, 8)[0]
    kw = dict(temperature=1.1, top_k=60, top_p=0.9, max_tokens=10, logprobs=4, ignore_eos=True)
    outs = eng.generate(prompt_token_ids=[p], sampling_params=SamplingParams(n=3, seed=50, **kw))[0].outputs
    assert len(outs) == 3
    for j, got in enumerate(outs):
        alone = eng.generate(prompt_token_ids=[p], sampling_params=SamplingParams(seed=50 + j, **kw))[0].outputs[0]
        assert got.token_ids == alone.token_ids and got.logprobs == alone.logprobs and got.cumulative_logprob == alone.cumulative_logprob
    assert outs[0].token_ids != outs[1].token_ids


def test_tensor_parallel_ranks_agree_and_match_the_gathered_row(dev):
    from tests._tp_lockstep import _run_lockstep
    from usdm_amd import ops
    from usdm_amd.llm import USDMForCausalLM, read_logprobs
    from usdm_amd.p2p import InProcessGroup
    cfg = dict(SMALL, vocab_size=1003, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=4)
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(cfg, seed=13)      # (one state dict: both ranks shard the same model)
    grp = InProcessGroup(2)
    ranks = [USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=128, tp_rank=r, tp_size=2, group=grp) for r in range(2)]
    ids, K, new, V, tol = _prompt(dev, 21, 4), 5, 8, 1003, R.kernel_tolerance()
    for m in ranks:
        ops.set_sample_params(m.sample_params, 0.9, 50, 0.95, 21)
    _run_lockstep([m._setup_call(ids, 0, True, BAD, None, 0, logprobs=K)[0] for m in ranks])
    torch.cuda.synchronize()
    rows = [ranks[0].last_logits[:V].cpu().numpy().copy()]      # keep_logits of a sampled tensor-parallel call: the gathered row
    decode = [m._build_decode(True, logprobs=K) for m in ranks]
    for _ in range(1, new):
        _run_lockstep(decode)
        torch.cuda.synchronize()
        rows.append(ranks[0].last_logits[:V].cpu().numpy().copy())
    lps = [read_logprobs(m._lp, new, K) for m in ranks]
    toks = [m.st_out[:new].tolist() for m in ranks]
    assert toks[0] == toks[1] and _same(lps[0], lps[1])
    _check_rows(lps[0], toks[0], rows, K, tol)
