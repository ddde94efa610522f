"""Repetition / frequency / presence penalties through the model (USDMForCausalLM.generate / generate_batch) and the serving surface
(SamplingParams) on small synthetic models.  Ground truth without a new oracle: the eager hook path exposes the logits row of every
step (the prefill's included); a hook that applies tests/_penalty_reference.penalize_row to it, with the prompt and the tokens
generated so far, must give the same ids and bit-identical log-probabilities as the on-device penalties, captured graph included."""
import numpy as np
import pytest
import torch

from tests import _penalty_reference as P

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
BAD = [[i] for i in range(250)]
KNOBS = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=-0.5)
LOOP = dict(frequency_penalty=-2.0)       # rewards every repeat by 2 per occurrence: locks a random-init model into a loop


def _model(dev, seed=5, cfg=SMALL, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.random_init(cfg, dev, seed=seed, ctx_max=256, **kw)


def _prompt(dev, n=40, seed=1):
    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _same(a, b):
    return all(torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32))
               for f in ("token_logprobs", "ranks", "top_ids", "top_logprobs")) and a.cumulative == b.cumulative


def _rfp(knobs):
    return knobs.get("repetition_penalty", 1.0), knobs.get("frequency_penalty", 0.0), knobs.get("presence_penalty", 0.0)


def _hook(m, ids, knobs, rows=None):
    """The penalties as a Python logits hook: the reference on the host, with the prompt and st_out[:step]"""
    prompt = ids[0].tolist()

    def h():
        step = int(m.st_step.item())
        row = m.last_logits.cpu().numpy()
        m.last_logits.copy_(torch.from_numpy(P.penalize_row(row, prompt, m.st_out[:step].tolist(), *_rfp(knobs))))
        if rows is not None:
            rows.append(m.last_logits.cpu().numpy().copy())
    return h


def _table(m):
    return m._pen["table"].cpu().numpy()


@pytest.mark.parametrize("knobs", [KNOBS, LOOP], ids=["all_three", "loop"])
@pytest.mark.parametrize("sampled", [False, True])
def test_device_penalties_equal_the_hooked_reference(dev, sampled, knobs):
    m, ids, K = _model(dev), _prompt(dev), 5
    kw = dict(input_ids=ids, max_new_tokens=12, bad_words_ids=BAD)
    if sampled:
        kw.update(do_sample=True, temperature=1.3, top_k=50, top_p=0.9, seed=11)
    plain = m.generate(**kw)
    out_h = m.generate(_logits_hook=_hook(m, ids, knobs), logprobs=K, **kw)
    lp_h = m.last_logprobs
    if knobs is LOOP and not sampled:
        # the precondition that keeps this test from passing vacuously: the penalised ids are NOT the plain ones
        assert not torch.equal(out_h, plain), "the penalties do not change this model's greedy ids: choose another seed / knobs"
    n_dec = len(m._decodes)
    for _ in range(2):      # the captured graph, twice: same ids, the same bits, run to run
        out_g = m.generate(logprobs=K, **kw, **knobs)
        assert torch.equal(out_g, out_h), (out_g[0, 40:].tolist(), out_h[0, 40:].tolist())
        assert _same(m.last_logprobs, lp_h)
    assert len(m._decodes) == n_dec + 1
    # the invariant: the table is the histogram of every token that was fed back, plus the prompt flags
    toks = out_g[0, 40:].tolist()
    assert np.array_equal(_table(m), P.table(1000, ids[0].tolist(), toks[:-1]))
    # without log-probabilities: the same ids (a plan of its own)
    assert torch.equal(m.generate(**kw, **knobs), out_h) and m.last_logprobs is None
    # both: the hook sees the PENALISED row (penalty launch first, then the hook)
    rows = []
    seen = lambda: rows.append(m.last_logits.cpu().numpy().copy())
    out_b = m.generate(_logits_hook=seen, **kw, **knobs)
    rows_h = []
    m.generate(_logits_hook=_hook(m, ids, knobs, rows_h), **kw)
    assert torch.equal(out_b, out_h) and len(rows) == len(rows_h) == 12
    assert all(np.array_equal(P.bits(a), P.bits(b)) for a, b in zip(rows, rows_h))


def test_neutral_knobs_are_the_plain_call_and_build_nothing(dev):
    from usdm_amd.llm import step_kind
    m, ids = _model(dev), _prompt(dev)
    kw = dict(input_ids=ids, max_new_tokens=12, bad_words_ids=BAD)
    plain = m.generate(**kw)
    keys = set(m._decodes)
    out = m.generate(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, **kw)
    assert torch.equal(out, plain) and set(m._decodes) == keys == {step_kind()} and m._pen is None
    assert not any(k[4] for k in m._prefill_plans)
    outs = m.generate_batch([ids, _prompt(dev, 23, 2)], 6, bad_words_ids=BAD, repetition_penalty=[1.0, 1.0], frequency_penalty=0.0)
    assert m._batches[2].pen is None and torch.equal(outs[0][0, :46], plain[0, :46])
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=2.5), dict(presence_penalty=3.0), dict(frequency_penalty=float("nan"))):
        with pytest.raises(ValueError, match="penalty"):
            m.generate(**kw, **bad)
    with pytest.raises(ValueError, match="one value per sequence"):
        m.generate_batch([ids, ids], 4, repetition_penalty=[1.2])


def test_device_side_eos_with_penalties_and_logprobs(dev):
    m, ids, K = _model(dev), _prompt(dev), 3
    kw = dict(input_ids=ids, bad_words_ids=BAD, logprobs=K, max_new_tokens=14)
    full = m.generate(**kw, **KNOBS)[0, 40:].tolist()
    eos = full[4]
    j = full.index(eos)
    cut_h = m.generate(_logits_hook=_hook(m, ids, KNOBS), eos_token_id=eos, **kw)[0, 40:].tolist()
    lp_h = m.last_logprobs
    cut = m.generate(eos_token_id=eos, **kw, **KNOBS)[0, 40:].tolist()
    assert cut == cut_h == full[:j + 1] and j + 1 < 14 and int(m.st_done.item()) == 1 and _same(m.last_logprobs, lp_h)
    # the steps replayed inside the host's chunk after `done` counted nothing: the table holds every token that was fed back (all the
    # returned ones but the final one, which no pick ever followed), each once
    assert np.array_equal(_table(m), P.table(1000, ids[0].tolist(), cut[:-1])) and int(m._pen["count"].item()) == j


@pytest.mark.parametrize("r", [1.5, 0.5])
def test_prefix_reuse_still_flags_the_whole_prompt(dev, r):
    """(r = 0.5 doubles the positive logits of the prompt's ids: the picks then come from the prompt, so ids of the reused part that
    were not flagged would show)"""
    a, b = _model(dev), _model(dev)
    first, knobs = _prompt(dev, 40, 1), dict(repetition_penalty=r)
    second = torch.cat([first, _prompt(dev, 20, 9)], dim=1)          # extends the first prompt by 20 ids
    kw = dict(max_new_tokens=10, bad_words_ids=BAD)
    a.generate(input_ids=first, **kw, **knobs)
    out = a.generate(input_ids=second, **kw, **knobs)
    assert any(k[1] == 40 for k in a._prefill_plans), list(a._prefill_plans)      # the first 40 ids' K/V were reused
    fresh = b.generate(input_ids=second, **kw, **knobs)
    assert torch.equal(out, fresh)
    assert np.array_equal(_table(a), P.table(1000, second[0].tolist(), out[0, 60:-1].tolist()))
    if r == 0.5:
        assert not torch.equal(fresh, b.generate(input_ids=second, **kw))       # (the penalty matters on this prompt)
        assert set(fresh[0, 60:].tolist()) & set(first[0].tolist())             # ... through ids of the reused part


def test_generate_batch_equals_generate_per_sequence(dev):
    """4 sequences with per-sequence knobs, one of them neutral, on the 4-slot VALU form: each equals generate() on its own."""
    m, K = _model(dev), 4
    prompts = [_prompt(dev, n, seed) for n, seed in ((40, 1), (23, 2), (31, 3), (36, 4))]
    r, f, p = [1.3, 1.0, 0.8, 1.0], [0.7, 0.0, -2.0, 0.0], [-0.5, 0.0, -1.0, 1.5]      # ([2] rewards repeats: its ids must change)
    kw = dict(max_new_tokens=11, bad_words_ids=BAD)
    outs = m.generate_batch(prompts, logprobs=K, repetition_penalty=r, frequency_penalty=f, presence_penalty=p, **kw)
    lps = m.last_logprobs
    differ = 0
    for b, (q, o, lp) in enumerate(zip(prompts, outs, lps)):
        alone = m.generate(input_ids=q, logprobs=K, repetition_penalty=r[b], frequency_penalty=f[b], presence_penalty=p[b], **kw)
        assert torch.equal(o, alone) and _same(lp, m.last_logprobs), b
        toks = o[0, q.shape[1]:].tolist()
        assert np.array_equal(m._batches[4].pen["table"][b].cpu().numpy(), P.table(1000, q[0].tolist(), toks[:-1])), b
        differ += not torch.equal(o, m.generate(input_ids=q, **kw))
    assert torch.equal(outs[1], m.generate(input_ids=prompts[1], **kw))      # the neutral one is the plain one
    assert differ >= 1 and not torch.equal(outs[2], m.generate(input_ids=prompts[2], **kw))
    one = m.generate_batch(prompts[:2], frequency_penalty=-2.0, **kw)                          # one value for all
    assert all(torch.equal(o, m.generate(input_ids=q, frequency_penalty=-2.0, **kw)) for o, q in zip(one, prompts))


def _requests(n, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [17 + (11 * i) % 40 for i in range(n)]
    return [torch.randint(0, 1000, (L,), generator=g).tolist() for L in lens]


def test_serving_four_slots_equal_the_requests_served_alone(dev):
    """6 ragged requests over 4 slots: two penalised (one sampled with a seed), four plain.  Request 4 is penalised and is admitted
    into a slot that a plain request held before: the slot's table is reset and reseeded."""
    from usdm_amd.serving import LLM, SamplingParams
    eng = LLM(model=_model(dev, seed=7), max_num_seqs=4)
    prompts = _requests(6, 3)
    mk = lambda mt, **kw: SamplingParams(max_tokens=mt, ignore_eos=True, **kw)
    sps = [mk(6, top_k=1), mk(15, temperature=1.2, top_k=40, top_p=0.95, seed=77, repetition_penalty=1.4, presence_penalty=1.0, logprobs=3),
           mk(9, top_k=1), mk(14, top_k=1), mk(16, top_k=1, frequency_penalty=-2.0), mk(12, top_k=1)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 6 and eng.stats["admissions"] == 6 and eng.stats["max_active"] == 4
    assert eng.stats["hook_requests"] == 0
    plain_idx = [0, 2, 3, 5]
    all_plain = eng.generate(prompt_token_ids=[prompts[i] for i in plain_idx], sampling_params=[sps[i] for i in plain_idx])
    for i, (q, sp, o) in enumerate(zip(prompts, sps, outs)):
        got = o.outputs[0]
        alone = eng.generate(prompt_token_ids=[q], sampling_params=sp)[0].outputs[0]
        assert got.token_ids == alone.token_ids and got.finish_reason == alone.finish_reason, i
        assert got.logprobs == alone.logprobs and got.cumulative_logprob == alone.cumulative_logprob, i
        if i in plain_idx:
            assert got.token_ids == all_plain[plain_idx.index(i)].outputs[0].token_ids, i
    assert eng.stats["hook_requests"] == 0                   # a penalised request alone: the single-sequence graph, not the hook path
    unpen = eng.generate(prompt_token_ids=[prompts[4]], sampling_params=mk(16, top_k=1))[0].outputs[0].token_ids
    assert unpen != outs[4].outputs[0].token_ids             # the second occupant's penalty was in force
    # a hook request with penalties gets both: a history-dependent processor that bans the previous token, on the penalised row
    def no_repeat(hist, logits):
        logits[hist[-1]] = float("-inf")
        return logits
    sp_h = mk(8, top_k=1, frequency_penalty=-2.0, logits_processors=[no_repeat], static_logits_mask=False)
    toks = eng.generate(prompt_token_ids=[prompts[4]], sampling_params=sp_h)[0].outputs[0].token_ids
    assert eng.stats["hook_requests"] == 1 and all(a != b for a, b in zip(toks, toks[1:])) and toks[0] != prompts[4][-1]


def _consistent(o, sp):
    """The reported picked token's rank / log-probability against its own top-K list (nothing recomputed on the host)"""
    K = sp.logprobs
    assert len(o.logprobs) == len(o.token_ids)
    total = 0.0
    for tok, d in zip(o.token_ids, o.logprobs):
        pick = d[tok]
        total += pick.logprob
        assert np.isfinite(pick.logprob) and pick.rank >= 1 and all(e.logprob <= 0 for e in d.values()) and len(d) in (K, K + 1)
        rest = sorted((e.rank, e.logprob, i) for i, e in d.items() if i != tok)
        assert all(a[1] > b[1] or (a[1] == b[1] and a[2] < b[2]) for a, b in zip(rest, rest[1:]))      # descending, ties lowest id first
        if len(d) == K + 1:
            assert pick.rank > K or pick.logprob == rest[-1][1]      # outside the list (or tied with its last entry)
            assert pick.logprob <= rest[-1][1]
        else:
            assert pick.rank <= K
        if sp.greedy:
            assert pick.rank == 1 and all(pick.logprob >= e[1] for e in rest)
    assert o.cumulative_logprob == total


def test_serving_sixteen_slots_outputs_are_consistent(dev):
    """18 requests through 16 slots; all share one static mask that leaves ALLOWED ids, so that a greedy request with more tokens than
    that repeats an id when unpenalised (pigeonhole) - the case presence_penalty = 2.0 must change."""
    from usdm_amd.serving import LLM, SamplingParams
    eng = LLM(model=_model(dev, seed=9), max_num_seqs=16)
    prompts = _requests(18, 5)
    ALLOWED = 12

    def only(token_ids, logits):
        logits[:250] = float("-inf")
        logits[250 + ALLOWED:] = float("-inf")
        return logits

    def params(i, pen=True):
        kw = dict(max_tokens=(14, 9, 5, 21, 12, 6, 17)[i % 7], ignore_eos=True, logits_processors=[only])
        if pen and i % 3 == 0:
            kw.update(presence_penalty=2.0, logprobs=5 if i % 2 == 0 else None)
        elif pen and i % 3 == 1:
            kw.update(repetition_penalty=1.2, frequency_penalty=0.5, logprobs=2)
        if i % 4 == 3:
            return SamplingParams(temperature=0.8 + 0.05 * i, top_k=40 + i, top_p=0.95, seed=100 + i, **kw)
        return SamplingParams(top_k=1, **kw)
    sps = [params(i) for i in range(18)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 18 and eng.stats["max_active"] == 16
    plain = eng.generate(prompt_token_ids=prompts, sampling_params=[params(i, pen=False) for i in range(18)])
    differ = []
    for i, (sp, o, o_plain) in enumerate(zip(sps, outs, plain)):
        got = o.outputs[0]
        assert 1 <= len(got.token_ids) <= sp.max_tokens
        if sp.logprobs is None:
            assert got.logprobs is None and got.cumulative_logprob is None
        else:
            _consistent(got, sp)
        assert all(250 <= t < 250 + ALLOWED for t in got.token_ids)
        if sp.presence_penalty == 2.0 and sp.greedy and sp.max_tokens > ALLOWED:
            assert len(set(o_plain.outputs[0].token_ids)) < sp.max_tokens       # unpenalised: an id repeats
            differ.append(got.token_ids != o_plain.outputs[0].token_ids)
    print("presence_penalty = 2.0, greedy: ids differ from the unpenalised request:", differ)
    assert len(differ) == 2 and any(differ), differ      # presence_penalty = 2 changes a greedy request's ids


def test_tensor_parallel_ranks_agree_and_match_the_single_gpu_model(dev):
    """Two logical ranks in lockstep on the penalised sampling step (greedy: top_k = 1): the ranks agree, and the ids are the
    single-GPU model's with the same knobs - equal, or first differing at a near-tie of the single-GPU model's own penalised row
    (tests/_greedy_compare.check_against_oracle, the rule the tensor-parallel tests compare with their oracle by)."""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from tests._tp_lockstep import _run_lockstep
    from usdm_amd import ops
    from usdm_amd.llm import USDMForCausalLM, check_penalties
    from usdm_amd.p2p import InProcessGroup
    cfg = dict(SMALL, vocab_size=1003, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=4)
    sd = MO.random_state_dict(cfg, seed=13)      # (one state dict: both ranks shard the same model)
    grp = InProcessGroup(2)
    ranks = [USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=128, tp_rank=r, tp_size=2, group=grp) for r in range(2)]
    ids, new, V = _prompt(dev, 21, 4), 10, 1003
    knobs = dict(repetition_penalty=0.8, frequency_penalty=-2.0, presence_penalty=0.5)      # rewards repeats: the ids must change
    pen = check_penalties(**knobs)
    for m in ranks:
        ops.set_sample_params(m.sample_params, 1.0, 1, 1.0, 0)
    _run_lockstep([m._setup_call(ids, 0, True, BAD, None, 0, penalties=pen)[0] for m in ranks])
    decode = [m._build_decode(True, penalties=True) for m in ranks]
    for _ in range(1, new):
        _run_lockstep(decode)
    torch.cuda.synchronize()
    toks = [m.st_out[:new].tolist() for m in ranks]
    assert toks[0] == toks[1]
    want_tbl = P.table(V, ids[0].tolist(), toks[0][:-1])
    assert all(np.array_equal(m._pen["table"].cpu().numpy(), want_tbl) for m in ranks)
    # the last step's gathered row on both ranks: penalised alike
    assert np.array_equal(P.bits(ranks[0].last_logits[:V].cpu().numpy()), P.bits(ranks[1].last_logits[:V].cpu().numpy()))
    one = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=128)
    rows = []
    ref = one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD,
                       _logits_hook=lambda: rows.append(one.last_logits.cpu().clone()), **knobs)[0].tolist()
    assert torch.equal(one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD, **knobs)[0], torch.tensor(ref, device=dev))
    check_against_oracle(ids[0].tolist() + toks[0], ref, torch.stack(rows), 21)
    assert ref[21:] != one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD)[0, 21:].tolist()
