"""Speculative greedy decoding through generate() and serving.LLM on the small model of tests/test_batch_gpu.py (ctx_max 256, bf16,
one GPU).  A call generates 49 tokens: the prefill's pick, which is no speculative step, and 48 tokens from speculative steps - the
48 the step counts below are about (last_spec_stats counts the steps on the device).
Scripts: `script[j]` is the draft for output j.  The all-wrong script holds a BANNED id, which no pick can equal."""
import pytest
import torch

from tests import _spec_reference as R
from tests._greedy_compare import NEAR_TIE_ABS, NEAR_TIE_REL, check_against_oracle, compare_greedy

pytestmark = pytest.mark.gpu
NEW, L0, V = R.NEW, R.PROMPT_LEN, R.SMALL_CFG["vocab_size"]
BANNED = 5
BAD = [[BANNED]]
_SD = {}


def _sd():
    from oracle import mistral_oracle as MO
    if "sd" not in _SD:
        _SD["sd"] = MO.random_state_dict(R.SMALL_CFG, R.MODEL_SEED)
    return _SD["sd"]


def _model(dev, cfg=None, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.from_state_dict(_sd(), cfg or R.SMALL_CFG, dev, ctx_max=256, **kw)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def prompt(dev):
    return R.small_prompt()[None].to(dev)


def _gen(m, prompt, k, script=None, bad=BAD, new=NEW, **kw):
    out = m.generate(input_ids=prompt, max_new_tokens=new, bad_words_ids=bad, num_speculative_tokens=k, _spec_script=script, **kw)
    return out[0, prompt.shape[1]:].tolist(), m.last_spec_stats


def _scripts(gen):
    wrong = [BANNED] * (NEW + 8)
    third = [BANNED if j % 3 == 0 else t for j, t in enumerate(gen)]
    return wrong, list(gen), third


@pytest.fixture(scope="module")
def wrong_run(model, prompt):
    """the all-wrong run at k = 3, computed once: the ids every other run of the bf16 model with <= 4 rows is compared with"""
    return _gen(model, prompt, 3, [BANNED] * (NEW + 8))


@pytest.mark.parametrize("k", [1, 3, 7])
def test_ids_do_not_depend_on_the_drafts(model, prompt, k):
    wrong, st_w = _gen(model, prompt, k, [BANNED] * (NEW + 8))
    assert len(wrong) == NEW and st_w == dict(steps=NEW - 1, drafted=k * (NEW - 1), accepted=0)
    _, own_s, third_s = _scripts(wrong)
    own, st_o = _gen(model, prompt, k, own_s)
    third, st_t = _gen(model, prompt, k, third_s)
    look, st_l = _gen(model, prompt, k)
    assert own == wrong and third == wrong and look == wrong
    full, rest = divmod(NEW - 1, k + 1)
    assert st_o["steps"] == -(-(NEW - 1) // (k + 1)) and st_o["accepted"] == full * k + max(0, rest - 1)
    assert 0 < st_t["accepted"] < st_o["accepted"]
    for st in (st_w, st_o, st_t, st_l):
        assert st["accepted"] + st["steps"] == NEW - 1 and st["accepted"] <= st["drafted"] <= k * st["steps"]


def _near_tie(sd, prefix, a, b):
    """both ids inside the oracle's near-tie band of the token after `prefix` (the rule of tests/_greedy_compare.py)"""
    from oracle import mistral_oracle as MO
    _, lg = MO.greedy_generate(sd, R.SMALL_CFG, torch.tensor(prefix), 1, bad_words_ids=BAD, return_logits=True)
    top = lg[0].max().item()
    tol = NEAR_TIE_REL * abs(top) + NEAR_TIE_ABS
    return top - lg[0][a].item() <= tol and top - lg[0][b].item() <= tol


@pytest.mark.parametrize("k", [3, 7])
def test_against_the_plain_path_and_the_oracle(dev, model, prompt, k):
    from oracle import mistral_oracle as MO
    ids = prompt[0].cpu()
    plain = model.generate(input_ids=prompt, max_new_tokens=NEW, bad_words_ids=BAD)[0].tolist()
    spec = prompt[0].tolist() + _gen(model, prompt, k)[0]
    first = next((i for i in range(len(plain)) if plain[i] != spec[i]), None)
    if first is not None:      # the verify attention and (k = 7) the matrix-core projections sum in another order than the plain step
        assert _near_tie(_sd(), plain[:first], plain[first], spec[first]), f"token {first - L0}: speculative and plain ids differ away from a near-tie"
    ref, ref_logits = MO.greedy_generate(_sd(), R.SMALL_CFG, ids, NEW, bad_words_ids=BAD, return_logits=True)
    check_against_oracle(spec, ref, ref_logits, L0)
    div, n = compare_greedy(model, dev, ids, ref, ref_logits, NEW, bad_words_ids=BAD, num_speculative_tokens=k)
    print(f"[spec] k={k}: first difference from the plain path {None if first is None else first - L0}, near-tie divergences from the oracle {div} of {n}")


def test_lookup_with_a_ban_mask(model, prompt):
    """the seed and mask that tests/test_spec_cpu.py checks on the oracle: the output cycles, the lookup's drafts are accepted"""
    bad = R.lookup_bad_words()
    wrong, st_w = _gen(model, prompt, R.LOOKUP_K, [0] * (NEW + 8), bad=bad)
    look, st = _gen(model, prompt, R.LOOKUP_K, bad=bad)
    assert look == wrong and set(look) <= set(R.LOOKUP_KEEP) and st_w["accepted"] == 0
    assert st["accepted"] > 0 and st["accepted"] + st["steps"] == NEW - 1
    print(f"[spec] lookup: {st}")


def test_stop_id_inside_an_accepted_run(model, prompt, wrong_run):
    gen = wrong_run[0]
    # own-output script at k = 3: steps emit outputs 1-4, 5-8, ...; outputs 6, 7, 10, 11 .. sit inside a run
    j = next(j for j in (6, 7, 10, 11, 14, 15, 18, 19) if gen[j] not in gen[:j])
    eos = gen[j]
    model.st_out.fill_(-1)
    got, st = _gen(model, prompt, 3, list(gen), eos_token_id=eos)
    assert got == gen[:j + 1] and int(model.st_step.item()) == j + 1 and int(model.st_done.item()) == 1
    assert bool((model.st_out[j + 1:] == -1).all()), "a token was emitted after the stop id"
    assert st["steps"] + st["accepted"] == j
    cut, _ = _gen(model, prompt, 3, [BANNED] * (NEW + 8), eos_token_id=eos)
    assert cut == got
    # min_new_tokens beyond it: the id is passed
    later, _ = _gen(model, prompt, 3, list(gen), eos_token_id=eos, min_new_tokens=j + 2)
    assert later[:j + 2] == gen[:j + 2] and len(later) > j + 1


def test_prefix_reuse_after_a_speculative_call(dev, model, prompt, wrong_run):
    gen = wrong_run[0]
    _gen(model, prompt, 3, list(gen))
    assert model._kv_ids == prompt[0].tolist() + gen[:NEW - 1] and model._vt_upto == L0      # committed rows only
    tail = torch.randint(0, V, (9,), generator=torch.Generator().manual_seed(3))
    p2 = torch.cat([prompt[0].cpu(), torch.tensor(gen[:20]), tail])[None].to(dev)
    a = model.generate(input_ids=p2, max_new_tokens=12, bad_words_ids=BAD)
    b = _model(dev).generate(input_ids=p2, max_new_tokens=12, bad_words_ids=BAD)
    assert torch.equal(a, b)


@pytest.mark.parametrize("what", ["window", "fp8", "mxfp4"])
def test_window_and_quantized_weights(dev, prompt, what):
    """window 40 (every generated position is past it), fp8 and mxfp4 weights: the ids do not depend on the script at k = 3"""
    m = _model(dev, cfg=dict(R.SMALL_CFG, sliding_window=40)) if what == "window" else _model(dev, quantization=what)
    assert m.window == (40 if what == "window" else 0) and m.max_batch() >= 4
    wrong, st_w = _gen(m, prompt, 3, [BANNED] * (NEW + 8))
    own, st_o = _gen(m, prompt, 3, list(wrong))
    look, _ = _gen(m, prompt, 3)
    assert own == wrong and look == wrong
    assert st_w == dict(steps=NEW - 1, drafted=3 * (NEW - 1), accepted=0) and st_o["steps"] == 12 and st_o["accepted"] == 36
    plain = m.generate(input_ids=prompt, max_new_tokens=NEW, bad_words_ids=BAD)[0, L0:].tolist()
    print(f"[spec] {what}: first difference from the plain path {next((i for i in range(NEW) if plain[i] != wrong[i]), None)}")


def test_off_by_default(dev, prompt):
    m = _model(dev)
    a = m.generate(input_ids=prompt, max_new_tokens=20, bad_words_ids=BAD)
    steps = dict(m._decodes)
    for k in (None, 0):
        b = m.generate(input_ids=prompt, max_new_tokens=20, bad_words_ids=BAD, num_speculative_tokens=k)
        assert torch.equal(a, b) and m._spec is None and m.last_spec_stats is None
        assert dict(m._decodes) == steps and all(m._decodes[x] is steps[x] for x in steps)


def test_refusals(dev, model, prompt):
    kw = dict(input_ids=prompt, max_new_tokens=8, num_speculative_tokens=3)
    for extra, word in ((dict(do_sample=True, top_k=5), "sampling"), (dict(logprobs=1), "logprobs"), (dict(repetition_penalty=1.2), "penalties"),
                        (dict(logit_bias={3: 1.0}), "logit_bias"), (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
                        (dict(do_sample=True, top_k=1, min_p=0.1), "min_p"), (dict(_logits_hook=lambda: None), "_logits_hook"),
                        (dict(num_beams=2), "num_beams")):
        with pytest.raises(NotImplementedError, match=word):
            model.generate(**kw, **extra)
    with pytest.raises(NotImplementedError, match="unquantized"):
        _model(dev, kv_cache_dtype="fp8").generate(**kw)
    for bad in (8, -1, 2.5):
        with pytest.raises(ValueError):
            model.generate(**dict(kw, num_speculative_tokens=bad))
    with pytest.raises(ValueError, match="at most 4"):      # the mxfp4 step takes 4 rows
        _model(dev, quantization="mxfp4").generate(**dict(kw, num_speculative_tokens=4))
    # greedy spelled the reference's way is no refusal
    assert model.generate(do_sample=True, top_k=1, **kw).shape[1] == L0 + 8


def test_serving(dev, model, prompt):
    from usdm_amd.serving import LLM, SamplingParams
    gen, _ = _gen(model, prompt, 3, bad=None)      # the model-level ids (no processors: the static mask bans nothing)
    ids = prompt[0].tolist()
    sp = SamplingParams(temperature=0.0, max_tokens=NEW)
    with pytest.raises(NotImplementedError, match="eagle"):
        LLM(model=model, speculative_config={"method": "eagle", "num_speculative_tokens": 3})
    srv = LLM(model=model, speculative_config={"method": "ngram", "num_speculative_tokens": 3, "prompt_lookup_max": 3, "prompt_lookup_min": 1})
    out = srv.generate(prompt_token_ids=[ids], sampling_params=sp)
    assert list(out[0].outputs[0].token_ids) == gen
    st = srv.stats
    assert st["spec_requests"] == 1 and st["spec_steps"] + st["spec_accepted"] == NEW - 1 and st["spec_drafted"] >= st["spec_accepted"]
    # two concurrent requests run exactly as without the option
    ids2 = ids[:-3]
    plain = LLM(model=model)
    want = plain.generate(prompt_token_ids=[ids, ids2], sampling_params=sp)
    got = srv.generate(prompt_token_ids=[ids, ids2], sampling_params=sp)
    for a, b in zip(want, got):
        assert list(a.outputs[0].token_ids) == list(b.outputs[0].token_ids)
    assert srv.stats["spec_requests"] == 1 and srv.stats["batched_requests"] == 2
    # a request with log-probabilities is served alone but not speculatively
    srv.generate(prompt_token_ids=[ids], sampling_params=SamplingParams(temperature=0.0, max_tokens=8, logprobs=0))
    assert srv.stats["spec_requests"] == 1
