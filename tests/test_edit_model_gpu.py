"""min_p, logit_bias and no_repeat_ngram_size through the model (USDMForCausalLM.generate / generate_batch) and the serving surface
(SamplingParams) on small synthetic models.  Ground truth without a new oracle: the eager hook path exposes the logits row of every
step (the prefill's included); a hook that applies tests/_edit_reference.edit_row to it, with the prompt and the tokens generated so
far, must give the same ids and bit-identical log-probabilities as the on-device edits, captured graph included."""
import numpy as np
import pytest
import torch

from tests import _edit_reference as E
from tests import _penalty_reference as P

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
BAD = [[i] for i in range(250)]
LOOP = dict(frequency_penalty=-2.0)       # rewards every repeat by 2 per occurrence: locks a random-init model into a loop
KNOBS = dict(repetition_penalty=1.3, frequency_penalty=0.7, presence_penalty=-0.5)
UP, DOWN = 777, 555                        # the ids biased by +100 / -100 (allowed by BAD; the prompts below do not hold them)


def _model(dev, seed=5, cfg=SMALL, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.random_init(cfg, dev, seed=seed, ctx_max=256, **kw)


def _prompt(dev, n=40, seed=1):
    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


def _same(a, b):
    return all(torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32))
               for f in ("token_logprobs", "ranks", "top_ids", "top_logprobs")) and a.cumulative == b.cumulative


def _hook(m, ids, bias, n, pen=None, rows=None):
    """The edits (and then, pen = (r, f, p), the penalties) as a Python logits hook: the references on the host, with the prompt and
    st_out[:step]; rows collects the rows as the hook leaves them"""
    prompt = ids[0].tolist()

    def h():
        out = m.st_out[:int(m.st_step.item())].tolist()
        row = E.edit_row(m.last_logits.cpu().numpy(), bias, n, prompt, out)
        if pen is not None:
            row = P.penalize_row(row, prompt, out, *pen)
        m.last_logits.copy_(torch.from_numpy(row))
        if rows is not None:
            rows.append(row.copy())
    return h


def _bigrams_twice(seq):
    pairs = list(zip(seq, seq[1:]))
    return len(pairs) - len(set(pairs))


def _check_up_down(prompt, toks, n, banned=range(250)):
    """DOWN (-100) never appears; UP (+100) is picked at every step at which neither the ban mask nor the n-gram rule bans it"""
    assert DOWN not in toks
    picked = 0
    for s, t in enumerate(toks):
        if UP in banned or UP in E.banned_ngram_ids(list(prompt) + toks[:s], n):
            assert t != UP, s
        else:
            assert t == UP, (s, t)
            picked += 1
    return picked


@pytest.mark.parametrize("sampled", [False, True])
def test_device_edits_equal_the_hooked_reference(dev, sampled):
    m, ids, K, new = _model(dev), _prompt(dev), 5, 14
    assert UP not in ids[0].tolist() and DOWN not in ids[0].tolist()
    kw = dict(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD)
    if sampled:
        kw.update(do_sample=True, temperature=1.3, top_k=50, top_p=0.9, seed=11)
    plain = m.generate(**kw)[0, 40:].tolist()
    bias = {plain[0]: -100.0, plain[1]: -7.5, 300: 2.25, 0: 50.0, 999: -0.5}       # (id 0 is banned by BAD: stays -inf)
    edits = dict(logit_bias=bias, no_repeat_ngram_size=2)
    out_h = m.generate(_logits_hook=_hook(m, ids, bias, 2), logprobs=K, **kw)
    lp_h = m.last_logprobs
    assert out_h[0, 40:].tolist() != plain and plain[0] not in out_h[0, 40:].tolist()      # the edits matter on this model
    n_dec = len(m._decodes)
    for _ in range(2):      # the captured graph, twice: same ids, the same bits, run to run
        out_g = m.generate(logprobs=K, **kw, **edits)
        assert torch.equal(out_g, out_h), (out_g[0, 40:].tolist(), out_h[0, 40:].tolist())
        assert _same(m.last_logprobs, lp_h)
    assert len(m._decodes) == n_dec + 1      # exactly one new decode plan
    assert torch.equal(m.generate(**kw, **edits), out_h) and m.last_logprobs is None      # without log-probabilities: a plan of its own
    # the hook, log-probabilities and last_logits see the EDITED row (edit launch first, then the hook)
    rows, rows_h = [], []
    out_b = m.generate(_logits_hook=lambda: rows.append(m.last_logits.cpu().numpy().copy()), **kw, **edits)
    m.generate(_logits_hook=_hook(m, ids, bias, 2, rows=rows_h), **kw)
    assert torch.equal(out_b, out_h) and len(rows) == len(rows_h) == new
    assert all(np.array_equal(E.bits(a), E.bits(b)) for a, b in zip(rows, rows_h))


def test_ngram_ban_breaks_the_loop_and_the_big_biases_rule(dev):
    m, ids, new = _model(dev), _prompt(dev), 24
    prompt = ids[0].tolist()
    kw = dict(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD)
    assert _bigrams_twice(prompt) == 0
    looped = m.generate(**kw, **LOOP)[0].tolist()
    # the precondition that keeps this test from passing vacuously: the plain greedy output under LOOP repeats a bigram
    assert _bigrams_twice(looped) > 0, "frequency_penalty = -2 does not lock this model into a loop: choose another seed"
    out = m.generate(**kw, **LOOP, no_repeat_ngram_size=2)[0].tolist()
    assert _bigrams_twice(out) == 0 and len(out) == 40 + new
    # ... and equals the hook that bans on top of the device's penalties (-inf commutes with them)
    assert m.generate(_logits_hook=_hook(m, ids, {}, 2), **kw, **LOOP)[0].tolist() == out
    for n in (1, 3):
        toks = m.generate(**kw, **LOOP, no_repeat_ngram_size=n)[0].tolist()
        if n == 1:
            assert len(set(toks[40:])) == new and not set(toks[40:]) & set(prompt)
        else:
            tri = list(zip(toks, toks[1:], toks[2:]))
            assert len(tri) == len(set(tri))
    # +100 / -100 (greedy): with n = 2 the biased id is picked whenever the bigram rule allows it
    big = {UP: 100.0, DOWN: -100.0}
    for n in (0, 2, 1):
        toks = m.generate(**kw, logit_bias=big, no_repeat_ngram_size=n)[0, 40:].tolist()
        picked = _check_up_down(prompt, toks, n)
        assert (picked == new) if n == 0 else (picked == 1) if n == 1 else (2 <= picked < new)
    assert DOWN not in m.generate(**kw, logit_bias={m.generate(**kw)[0, 40].item(): -100.0, DOWN: -100.0})[0, 40:].tolist()
    # values beyond vLLM's range are clamped to it: the same call
    assert torch.equal(m.generate(**kw, logit_bias={UP: 1e6, DOWN: -1e6}, no_repeat_ngram_size=2),
                       m.generate(**kw, logit_bias=big, no_repeat_ngram_size=2))


def test_bias_then_penalties_is_the_order(dev):
    """HF's and vLLM's order: bias, n-gram ban, then the penalties - against a hook that does all of it on the plain row"""
    from usdm_amd.llm import check_penalties
    m, ids, K = _model(dev), _prompt(dev), 4
    kw = dict(input_ids=ids, max_new_tokens=12, bad_words_ids=BAD, logprobs=K)
    plain = m.generate(**kw)[0, 40:].tolist()
    bias = {plain[1]: 3.5, plain[2]: 3.5, plain[5]: -2.0, plain[0]: -100.0}
    out_h = m.generate(_logits_hook=_hook(m, ids, bias, 3, pen=check_penalties(**KNOBS)), **kw)
    lp_h = m.last_logprobs
    out = m.generate(logit_bias=bias, no_repeat_ngram_size=3, **kw, **KNOBS)
    assert torch.equal(out, out_h) and _same(m.last_logprobs, lp_h)
    assert plain[0] not in out[0, 40:].tolist()      # (the edits matter next to the penalties)


def test_neutral_knobs_are_the_plain_call_and_build_nothing(dev):
    from usdm_amd.llm import step_kind
    m, ids = _model(dev), _prompt(dev)
    kw = dict(input_ids=ids, max_new_tokens=12, bad_words_ids=BAD)
    plain = m.generate(**kw)
    keys = set(m._decodes)
    for neutral in (dict(min_p=0.0, logit_bias=None, no_repeat_ngram_size=0), dict(logit_bias={}, no_repeat_ngram_size=None), dict(min_p=0.5)):
        out = m.generate(**kw, **neutral)      # (min_p on a greedy call: the maximum always survives)
        assert torch.equal(out, plain) and set(m._decodes) == keys == {step_kind()} and m._edt is None
    assert all(len(k) == 6 and not k[4] and not k[5] for k in m._prefill_plans)
    outs = m.generate_batch([ids, _prompt(dev, 23, 2)], 6, bad_words_ids=BAD, logit_bias=[None, {}], no_repeat_ngram_size=0, min_p=0.0)
    assert m._batches[2].edt is None and torch.equal(outs[0][0, :46], plain[0, :46])
    for bad, word in ((dict(min_p=1.5), "min_p"), (dict(min_p=float("nan")), "min_p"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                      (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"), (dict(logit_bias={1000: 1.0}), "logit_bias"),
                      (dict(logit_bias={-1: 1.0}), "logit_bias"), (dict(logit_bias={5: float("inf")}), "logit_bias"),
                      (dict(logit_bias={i: 0.5 for i in range(1025)}), "logit_bias"), (dict(logit_bias=[1, 2]), "logit_bias")):
        with pytest.raises(ValueError, match=word):
            m.generate(**kw, **bad)
    with pytest.raises(ValueError, match="one value per sequence"):
        m.generate_batch([ids, ids], 4, no_repeat_ngram_size=[2])
    with pytest.raises(ValueError, match="one value per sequence"):
        m.generate_batch([ids, ids], 4, logit_bias=[{5: 1.0}, None, None])
    assert torch.equal(m.generate(**kw), plain) and set(m._decodes) == keys


def test_min_p_through_generate(dev):
    m, ids, new = _model(dev), _prompt(dev), 16
    kw = dict(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD, do_sample=True, seed=21, logprobs=3)
    plain = m.generate(temperature=1.5, **kw)
    lp = m.last_logprobs
    keys = set(m._decodes)
    assert torch.equal(m.generate(temperature=1.5, min_p=0.0, **kw), plain) and _same(m.last_logprobs, lp)      # bit for bit
    for T, min_p in ((1.5, 1.0), (1.5, 0.2), (0.8, 0.2)):
        rows = []
        out_h = m.generate(temperature=T, min_p=min_p, _logits_hook=lambda: rows.append(m.last_logits.cpu().numpy().astype(np.float64)), **kw)
        toks = out_h[0, 40:].tolist()
        assert len(rows) == len(toks) == new
        for x, t in zip(rows, toks):
            ratio = np.exp((x[t] - x.max()) / T)
            print(f"T={T} min_p={min_p}: token {t}, p / p_max = {ratio:.6f}")
            assert ratio >= min_p * (1 - 1e-4)
            assert min_p < 1.0 or x[t] == x.max()
        out_g = m.generate(temperature=T, min_p=min_p, **kw)      # the captured path equals the hook path
        assert torch.equal(out_g, out_h)
    assert set(m._decodes) - keys == {("hook", 3, False, False)}      # min_p itself changes no plan and no step kind
    assert not torch.equal(m.generate(temperature=1.5, min_p=0.2, **kw), plain)


def test_prefix_reuse_keeps_the_whole_prompt_as_history(dev):
    """n = 1 bans every id of the history: ids of the part of the prompt whose K/V were reused would show if they were missing"""
    a, b = _model(dev), _model(dev)
    first = _prompt(dev, 40, 1)
    second = torch.cat([first, _prompt(dev, 20, 9)], dim=1)          # extends the first prompt by 20 ids
    kw = dict(max_new_tokens=10, bad_words_ids=BAD, no_repeat_ngram_size=1, frequency_penalty=-2.0)
    a.generate(input_ids=first, **kw)
    out = a.generate(input_ids=second, **kw)
    assert any(k[1] == 40 for k in a._prefill_plans), list(a._prefill_plans)      # the first 40 ids' K/V were reused
    assert torch.equal(out, b.generate(input_ids=second, **kw))
    toks = out[0, 60:].tolist()
    assert len(set(toks)) == 10 and not set(toks) & set(second[0].tolist())


def test_generate_batch_equals_generate_per_sequence(dev):
    """4 sequences with per-sequence knobs, one of them neutral, on the 4-slot VALU form: each equals generate() on its own."""
    m, K = _model(dev), 4
    prompts = [_prompt(dev, n, seed) for n, seed in ((40, 1), (23, 2), (31, 5), (36, 4))]
    kw = dict(max_new_tokens=11, bad_words_ids=BAD)
    first = [m.generate(input_ids=q, **kw)[0, q.shape[1]].item() for q in prompts]
    bias = [{first[0]: -100.0, UP: 4.0}, None, {UP: 100.0}, {}]
    ng = [2, 0, 1, 3]
    f = [-2.0, 0.0, 0.0, -2.0]
    outs = m.generate_batch(prompts, logprobs=K, logit_bias=bias, no_repeat_ngram_size=ng, frequency_penalty=f, **kw)
    lps = m.last_logprobs
    for b, (q, o, lp) in enumerate(zip(prompts, outs, lps)):
        alone = m.generate(input_ids=q, logprobs=K, logit_bias=bias[b], no_repeat_ngram_size=ng[b], frequency_penalty=f[b], **kw)
        assert torch.equal(o, alone) and _same(lp, m.last_logprobs), b
    assert torch.equal(outs[1], m.generate(input_ids=prompts[1], **kw))      # the neutral one is the plain one
    assert first[0] not in outs[0][0, 40:].tolist() and _bigrams_twice(outs[0][0].tolist()) == 0
    t2 = outs[2][0, 31:].tolist()
    assert t2[0] == UP and UP not in t2[1:] and len(set(t2)) == 11
    one = m.generate_batch(prompts[:2], logit_bias={UP: 100.0}, no_repeat_ngram_size=2, **kw)                          # one value for all
    assert all(torch.equal(o, m.generate(input_ids=q, logit_bias={UP: 100.0}, no_repeat_ngram_size=2, **kw)) for o, q in zip(one, prompts))


def _requests(n, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [17 + (11 * i) % 40 for i in range(n)]
    reqs = [torch.randint(0, 1000, (L,), generator=g).tolist() for L in lens]
    return [[t if t not in (UP, DOWN) else 600 for t in r] for r in reqs]


def test_serving_four_slots_equal_the_requests_served_alone(dev):
    """6 ragged requests over 4 slots: three with edits / min_p (one sampled with a seed), three plain.  Request 4 has edits and is
    admitted into a slot that a plain request held before: the slot's edit state is rewritten."""
    from usdm_amd.serving import LLM, SamplingParams
    eng = LLM(model=_model(dev, seed=7), max_num_seqs=4)
    prompts = _requests(6, 3)
    mk = lambda mt, **kw: SamplingParams(max_tokens=mt, ignore_eos=True, **kw)
    sps = [mk(6, top_k=1), mk(15, temperature=1.2, top_k=40, top_p=0.95, seed=77, min_p=0.1, no_repeat_ngram_size=2, logit_bias={DOWN: -100.0, UP: 1.5},
                              presence_penalty=1.0, logprobs=3),
           mk(9, top_k=1), mk(14, top_k=1, temperature=1.0, min_p=0.3), mk(16, top_k=1, logit_bias={UP: 100.0, DOWN: -100.0}, no_repeat_ngram_size=2),
           mk(12, temperature=1.4, seed=5, min_p=0.25)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 6 and eng.stats["admissions"] == 6 and eng.stats["max_active"] == 4
    assert eng.stats["hook_requests"] == 0
    for i, (q, sp, o) in enumerate(zip(prompts, sps, outs)):
        got = o.outputs[0]
        alone = eng.generate(prompt_token_ids=[q], sampling_params=sp)[0].outputs[0]
        assert got.token_ids == alone.token_ids and got.finish_reason == alone.finish_reason, i
        assert got.logprobs == alone.logprobs and got.cumulative_logprob == alone.cumulative_logprob, i
    assert eng.stats["hook_requests"] == 0                   # a request with edits alone: the single-sequence graph, not the hook path
    assert _check_up_down(prompts[4], outs[4].outputs[0].token_ids, 2, banned=()) >= 2
    assert _bigrams_twice(prompts[1] + outs[1].outputs[0].token_ids) <= _bigrams_twice(prompts[1]) and DOWN not in outs[1].outputs[0].token_ids
    no_min_p = eng.generate(prompt_token_ids=[prompts[5]], sampling_params=mk(12, temperature=1.4, seed=5))[0].outputs[0].token_ids
    assert no_min_p != outs[5].outputs[0].token_ids          # min_p was in force inside the batch
    with pytest.raises(ValueError, match="logit_bias"):      # ids are checked against the model's vocabulary when the request is served
        eng.generate(prompt_token_ids=[prompts[0]], sampling_params=mk(4, logit_bias={1000: 1.0}))
    # a hook request with edits gets both: a history-dependent processor next to the device's n-gram ban and bias
    def never_up_twice(hist, logits):
        if UP in hist[len(prompts[4]):]:
            logits[UP] = float("-inf")
        return logits
    sp_h = mk(8, top_k=1, logit_bias={UP: 100.0}, no_repeat_ngram_size=2, logits_processors=[never_up_twice], static_logits_mask=False)
    toks = eng.generate(prompt_token_ids=[prompts[4]], sampling_params=sp_h)[0].outputs[0].token_ids
    assert eng.stats["hook_requests"] == 1 and toks[0] == UP and UP not in toks[1:] and _bigrams_twice(prompts[4] + toks) <= _bigrams_twice(prompts[4])


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_serving_sixteen_slots_properties_hold_per_request(dev, quant):
    """18 requests through 16 slots (the matrix-core step; fp8: usdm_gemv_fp8_mfma): per request, the -100 id never appears, the +100 id
    is picked whenever the n-gram rule allows it, and no n-gram of the request's size occurs twice beyond the prompt's own"""
    from usdm_amd.serving import LLM, SamplingParams
    kw = dict(quantization="fp8", fp8_matrix_cores=True) if quant else {}
    eng = LLM(model=_model(dev, seed=9, **kw), max_num_seqs=16)
    prompts = _requests(18, 5)

    def params(i):
        kw = dict(max_tokens=(14, 9, 5, 21, 12, 6, 17)[i % 7], ignore_eos=True, logits_processors=[lambda ids, lg: _mask(lg)])
        if i % 3 == 0:
            kw.update(logit_bias={UP: 100.0, DOWN: -100.0}, no_repeat_ngram_size=2)
        elif i % 3 == 1:
            kw.update(no_repeat_ngram_size=1, frequency_penalty=-2.0, logprobs=2)
        if i % 4 == 3:
            return SamplingParams(temperature=0.8 + 0.05 * i, top_k=40 + i, top_p=0.95, seed=100 + i, min_p=0.05, **kw)
        return SamplingParams(top_k=1, **kw)

    def _mask(lg):
        lg[:250] = float("-inf")
        return lg
    sps = [params(i) for i in range(18)]
    outs = eng.generate(prompt_token_ids=prompts, sampling_params=sps)
    assert eng.stats["batched_requests"] == 18 and eng.stats["max_active"] == 16 and eng.stats["hook_requests"] == 0
    for i, (q, sp, o) in enumerate(zip(prompts, sps, outs)):
        toks = o.outputs[0].token_ids
        assert 1 <= len(toks) <= sp.max_tokens and all(t >= 250 for t in toks)
        if i % 3 == 0:
            assert DOWN not in toks, i
            if sp.greedy:
                assert _check_up_down(q, toks, 2, banned=()) >= 1, i
            assert _bigrams_twice(q + toks) <= _bigrams_twice(q), i
        elif i % 3 == 1:
            assert len(set(toks)) == len(toks) and not set(toks) & set(q), i      # n = 1: no id of the history again


def test_device_side_eos_with_edits_penalties_and_logprobs(dev):
    from usdm_amd.llm import check_penalties
    m, ids, K = _model(dev), _prompt(dev), 3
    kw = dict(input_ids=ids, bad_words_ids=BAD, logprobs=K, max_new_tokens=14)
    first = m.generate(**kw)[0, 40].item()
    edits = dict(logit_bias={first: -100.0, UP: 1.0}, no_repeat_ngram_size=2)
    full = m.generate(**kw, **edits, **KNOBS)[0, 40:].tolist()
    eos = full[4]
    j = full.index(eos)
    cut_h = m.generate(_logits_hook=_hook(m, ids, edits["logit_bias"], 2, pen=check_penalties(**KNOBS)), eos_token_id=eos, **kw)[0, 40:].tolist()
    lp_h = m.last_logprobs
    cut = m.generate(eos_token_id=eos, **kw, **edits, **KNOBS)[0, 40:].tolist()
    # the stop token's row is kept: the launches replayed inside the host's chunk after `done` touched nothing
    assert cut == cut_h == full[:j + 1] and j + 1 < 14 and int(m.st_done.item()) == 1 and _same(m.last_logprobs, lp_h)
    assert m.last_logprobs.token_logprobs.numel() == j + 1 and first not in cut


def test_tensor_parallel_ranks_agree_and_match_the_hooked_reference(dev):
    """Two logical ranks in lockstep on the edited sampling step (greedy: top_k = 1), the launch on the gathered row on every rank:
    the ranks agree, every token is the arg-max of the gathered row as the launch left it, that row carries the reference's bans,
    and the ids are the single-GPU model's hooked reference's (equal, or first differing at a near-tie of its own row)."""
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from tests._tp_lockstep import _run_lockstep
    from usdm_amd import ops
    from usdm_amd.llm import USDMForCausalLM, check_edits
    from usdm_amd.p2p import InProcessGroup
    cfg = dict(SMALL, vocab_size=1003, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=4)
    sd = MO.random_state_dict(cfg, seed=13)      # (one state dict: both ranks shard the same model)
    grp = InProcessGroup(2)
    ranks = [USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=128, tp_rank=r, tp_size=2, group=grp) for r in range(2)]
    ids, new, V = _prompt(dev, 21, 4), 12, 1003
    prompt = ids[0].tolist()
    bias = {UP: 100.0, DOWN: -100.0, 1002: 3.0, 501: -1.0, 502: 1.0}      # (ids of both ranks' shards, the last id of the vocabulary)
    edt = check_edits(bias, 2, V)
    for m in ranks:
        ops.set_sample_params(m.sample_params, 1.0, 1, 1.0, 0)
    _run_lockstep([m._setup_call(ids, 0, True, BAD, None, 0, edits=edt)[0] for m in ranks])
    torch.cuda.synchronize()
    rows = [[m.last_logits[:V].cpu().numpy().copy() for m in ranks]]
    decode = [m._build_decode(True, edits=True) for m in ranks]
    for _ in range(1, new):
        _run_lockstep(decode)
        torch.cuda.synchronize()
        rows.append([m.last_logits[:V].cpu().numpy().copy() for m in ranks])
    toks = [m.st_out[:new].tolist() for m in ranks]
    assert toks[0] == toks[1]
    for s, (r0, r1) in enumerate(rows):
        assert np.array_equal(E.bits(r0), E.bits(r1))                          # edited alike on both ranks
        ban = E.banned_ngram_ids(prompt + toks[0][:s], 2)
        assert all(np.isneginf(r0[i]) for i in ban) and np.isneginf(r0[:250]).all()
        assert int(np.isneginf(r0).sum()) == 250 + len([i for i in ban if i >= 250])
        assert toks[0][s] == int(np.argmax(r0))
    assert _check_up_down(prompt, toks[0], 2) >= 2
    one = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=128)
    ref_rows = []
    ref = one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD, _logits_hook=_hook(one, ids, dict(edt[0]), 2, rows=ref_rows))[0].tolist()
    assert torch.equal(one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD, logit_bias=bias, no_repeat_ngram_size=2)[0],
                       torch.tensor(ref, device=dev))
    check_against_oracle(prompt + toks[0], ref, torch.from_numpy(np.stack(ref_rows)), 21)
    assert ref[21:] != one.generate(input_ids=ids, max_new_tokens=new, bad_words_ids=BAD)[0, 21:].tolist()
