"""Batched speculative greedy decoding through generate_batch() and serving.LLM on the small model of tests/test_spec_model_gpu.py
(ctx_max 256, bf16, one GPU), ragged prompts.  A sequence generates 49 tokens: the prefill's pick, which is no speculative step, and 48
from speculative steps of B slots x (k + 1) rows.  Scripts: `script[j]` is the draft for output j; the all-wrong script holds a BANNED
id, which no pick can equal."""
import pytest
import torch

from tests import _spec_reference as R
from tests._greedy_compare import NEAR_TIE_ABS, NEAR_TIE_REL, check_against_oracle

pytestmark = pytest.mark.gpu
NEW, V = R.NEW, R.SMALL_CFG["vocab_size"]
BANNED = 5
BAD = [[BANNED]]
LENS = (24, 17, 21, 9, 13, 19, 11, 15)      # ragged
_MEMO = {}


def _sd():
    from oracle import mistral_oracle as MO
    if "sd" not in _MEMO:
        _MEMO["sd"] = MO.random_state_dict(R.SMALL_CFG, R.MODEL_SEED)
    return _MEMO["sd"]


def _model(dev, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.from_state_dict(_sd(), R.SMALL_CFG, dev, ctx_max=256, **kw)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


@pytest.fixture(scope="module")
def prompts(dev):
    """eight prompts of different lengths; the first is the prompt of tests/test_spec_model_gpu.py"""
    g = torch.Generator().manual_seed(R.PROMPT_SEED + 1)
    ps = [R.small_prompt()] + [torch.randint(0, V, (n,), generator=g) for n in LENS[1:]]
    return [p[None].to(dev) for p in ps]


def _oracle(p, bad=BAD):
    """the oracle's ids and masked logits for one prompt (computed once per prompt and mask)"""
    from oracle import mistral_oracle as MO
    key = (tuple(p[0].tolist()), bad is None)
    if key not in _MEMO:
        _MEMO[key] = MO.greedy_generate(_sd(), R.SMALL_CFG, p[0].cpu(), NEW, bad_words_ids=bad, return_logits=True)
    return _MEMO[key]


def _gen(m, ps, k, scripts=None, bad=BAD, new=NEW, **kw):
    outs = m.generate_batch(ps, new, bad_words_ids=bad, num_speculative_tokens=k, _spec_script=scripts, **kw)
    return [o[0, p.shape[1]:].tolist() for o, p in zip(outs, ps)], m.last_spec_stats


WRONG = [BANNED] * (NEW + 8)


@pytest.mark.parametrize("B,k", [(2, 1), (2, 3), (4, 3), (2, 7), (8, 1)])
def test_ids_do_not_depend_on_the_drafts(model, prompts, B, k):
    ps = prompts[:B]
    wrong, st_w = _gen(model, ps, k, [WRONG] * B)
    assert all(len(w) == NEW for w in wrong) and st_w == [dict(steps=NEW - 1, drafted=k * (NEW - 1), accepted=0)] * B
    own, st_o = _gen(model, ps, k, [list(w) for w in wrong])
    third, st_t = _gen(model, ps, k, [[BANNED if j % 3 == 0 else t for j, t in enumerate(w)] for w in wrong])
    look, st_l = _gen(model, ps, k)
    assert own == wrong and third == wrong and look == wrong
    for b in range(B):
        assert st_o[b]["steps"] == -(-(NEW - 1) // (k + 1))
        assert 0 < st_t[b]["accepted"] < st_o[b]["accepted"]
        for st in (st_w[b], st_o[b], st_t[b], st_l[b]):
            assert st["accepted"] + st["steps"] == NEW - 1 and st["accepted"] <= st["drafted"] <= k * st["steps"]
    assert k + 1 in model.spec_slots(B).spec_steps      # the slots' step of B x (k + 1) rows ran


def test_four_rows_equal_the_single_sequence_call(model, prompts):
    """(2, 1): four rows on the VALU form - every sequence's ids == generate(num_speculative_tokens=1) on that prompt alone"""
    ps = prompts[:2]
    got, _ = _gen(model, ps, 1)
    for p, g in zip(ps, got):
        alone = model.generate(input_ids=p, max_new_tokens=NEW, bad_words_ids=BAD, num_speculative_tokens=1)[0, p.shape[1]:].tolist()
        assert g == alone


@pytest.mark.parametrize("B,k", [(2, 3), (4, 3)])
def test_more_than_four_rows_against_the_oracle(model, prompts, B, k):
    """the matrix-core projections sum K in another order: equal to the oracle up to its near-ties (tests/_greedy_compare.py)"""
    ps = prompts[:B]
    got, _ = _gen(model, ps, k)
    for p, g in zip(ps, got):
        ref, ref_logits = _oracle(p)
        first = check_against_oracle(p[0].tolist() + g, ref, ref_logits, p.shape[1])
        print(f"[spec-batch] ({B}, {k}) prompt of {p.shape[1]}: first near-tie difference from the oracle {first}")


def test_co_tenants(model, prompts):
    """(2, 3): a sequence's ids are the same in slot 0 and slot 1, and next to two different neighbours"""
    a, x, y = prompts[0], prompts[1], prompts[2]
    base = _gen(model, [a, x], 3)[0]
    swapped = _gen(model, [x, a], 3)[0]
    other = _gen(model, [a, y], 3)[0]
    assert swapped[1] == base[0] and swapped[0] == base[1] and other[0] == base[0]
    wrong = _gen(model, [y, a], 3, [WRONG, WRONG])[0]
    assert wrong[1] == base[0] and wrong[0] == other[1]


def _plain(model, ps, max_new, **kw):
    outs = model.generate_batch(ps, max(max_new), bad_words_ids=BAD, **kw)
    return [o[0, p.shape[1]:p.shape[1] + n].tolist() for o, p, n in zip(outs, ps, max_new)]


def _alone(model, p, k, new, **kw):
    return model.generate(input_ids=p, max_new_tokens=new, bad_words_ids=BAD, num_speculative_tokens=k, **kw)[0, p.shape[1]:].tolist()


@pytest.mark.parametrize("case", ["max_new", "stop"])
def test_ends(model, prompts, case):
    """(2, 1): different max_new_tokens per sequence / a stop id that one sequence hits early.  The lengths equal the plain path's and
    the ids those of generate(num_speculative_tokens=1) on each prompt alone (==: four rows on the VALU form); the finished slot's out
    row and its cache rows behind the last rows its own steps wrote still hold the sentinels they held before the call, although the
    other slot ran on."""
    ps, T = prompts[:2], 2
    if case == "max_new":
        max_new, kw = [NEW, 20], {}
    else:      # an id that sequence 1 emits for the first time at j and that sequence 0 never emits, on either path
        full, spec0 = _plain(model, ps, [NEW, NEW]), _alone(model, ps[0], 1, NEW)
        j = next(j for j in range(4, 16) if full[1][j] not in full[1][:j] and full[1][j] not in full[0] + spec0)
        max_new, kw = [NEW, 30], dict(eos_token_id=full[1][j])
    plain = _plain(model, ps, max_new, **kw)
    want = [_alone(model, p, 1, n, **kw) for p, n in zip(ps, max_new)]
    assert [len(w) for w in plain] == ([NEW, 20] if case == "max_new" else [NEW, j + 1])
    ss = model.spec_slots(2)
    ss.out.fill_(-1)
    ss.kc.fill_(777.0)
    ss.vc.fill_(777.0)
    got, st = _gen(model, ps, 1, new=max_new, **kw)
    assert got == want and [len(g) for g in got] == [len(w) for w in plain]
    n1, L1 = len(got[1]), ps[1].shape[1]
    assert int(ss.step[1]) == n1 and int(ss.done[1]) == 1 and int(ss.pos[1]) == L1 + n1 - 1
    assert bool((ss.out[1, n1:] == -1).all()), "the finished slot emitted a token after its end"
    dead = L1 + n1 - 1 + T - 1      # first row no step of slot 1 can have written
    assert bool((ss.kc[1, :, :, dead:] == 777.0).all()) and bool((ss.vc[1, :, :, dead:] == 777.0).all()), "the finished slot's cache was written after its end"
    assert not bool((ss.kc[1, :, :, :L1 + n1 - 1] == 777.0).any())
    assert int(ss.step[0]) == NEW and st[1]["steps"] + st[1]["accepted"] == n1 - 1 and st[0]["steps"] + st[0]["accepted"] == NEW - 1


def _near_tie(prefix, a, b, bad, sd=None):
    """both ids inside the oracle's near-tie band of the token after `prefix` (the rule of tests/_greedy_compare.py)"""
    from oracle import mistral_oracle as MO
    _, lg = MO.greedy_generate(sd or _sd(), R.SMALL_CFG, torch.tensor(prefix), 1, bad_words_ids=bad, return_logits=True)
    top = lg[0].max().item()
    tol = NEAR_TIE_REL * abs(top) + NEAR_TIE_ABS
    return top - lg[0][a].item() <= tol and top - lg[0][b].item() <= tol


def test_serving(model, prompts):
    from usdm_amd.serving import LLM, SamplingParams
    ids = [p[0].tolist() for p in prompts[:6]]
    alone_probe = LLM(model=model).generate(prompt_token_ids=[ids[2]], sampling_params=SamplingParams(temperature=0.0, max_tokens=12))
    stop = alone_probe[0].outputs[0].token_ids[7]
    lims = [NEW, 20, 33, 12, 40, 25]
    sps = [SamplingParams(temperature=0.0, max_tokens=n, stop_token_ids=[stop] if i == 2 else None) for i, n in enumerate(lims)]
    srv = LLM(model=model, speculative_config={"method": "ngram", "num_speculative_tokens": 3}, max_num_seqs=4)
    sampled = SamplingParams(temperature=0.8, top_k=20, seed=1, max_tokens=10)
    outs = srv.generate(prompt_token_ids=ids + [ids[0]], sampling_params=sps + [sampled])
    st = dict(srv.stats)
    assert st["spec_max_active"] >= 2 and st["spec_batched_requests"] == 6 and st["spec_max_active"] <= 4
    assert st["sampled_in_batch"] == 1 and st["spec_requests"] == 0      # the sampled request: down the batched path, as without the option
    assert len(outs[6].outputs[0].token_ids) == 10
    assert st["spec_steps"] + st["spec_accepted"] == sum(len(o.outputs[0].token_ids) - 1 for o in outs[:6])
    for i in range(6):      # the same requests one at a time on the same engine: the single-sequence speculative path
        one = srv.generate(prompt_token_ids=[ids[i]], sampling_params=sps[i])[0].outputs[0]
        got = outs[i].outputs[0]
        a, b = list(one.token_ids), list(got.token_ids)
        first = next((t for t in range(min(len(a), len(b))) if a[t] != b[t]), None)
        if first is None:
            assert len(a) == len(b) and one.finish_reason == got.finish_reason, (i, len(a), len(b))
        else:       # 16 rows run the matrix-core projections, 4 rows the VALU form
            assert _near_tie(ids[i] + a[:first], a[first], b[first], None), f"request {i}, token {first}: batched and single ids differ away from a near-tie"
        assert len(b) <= lims[i] and (got.finish_reason == "stop") == (bool(b) and b[-1] == stop and i == 2)
    assert srv.stats["spec_requests"] == 6 and srv.stats["spec_batched_requests"] == 6


def test_refusals_and_fallbacks(dev, model, prompts):
    ps = prompts[:2]
    kw = dict(max_new_tokens=8, num_speculative_tokens=3)
    for extra, word in ((dict(logprobs=1), "logprobs"), (dict(repetition_penalty=1.2), "penalties"), (dict(logit_bias={3: 1.0}), "logit_bias"),
                        (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(min_p=0.1), "min_p")):
        with pytest.raises(NotImplementedError, match=word):
            model.generate_batch(ps, **kw, **extra)
    with pytest.raises(NotImplementedError, match="unquantized"):
        _model(dev, kv_cache_dtype="fp8").generate_batch(ps, **kw)
    pc = _model(dev, enable_prefix_caching=True)
    with pytest.raises(NotImplementedError, match="enable_prefix_caching"):
        pc.generate_batch(ps, **kw)
    one = pc.generate_batch(ps[:1], **kw)      # a group of one: the single-sequence path keeps working there
    assert torch.equal(one[0], model.generate(input_ids=ps[0], **kw))
    for bad in (8, -1, 2.5):
        with pytest.raises(ValueError):
            model.generate_batch(ps, 8, num_speculative_tokens=bad)
    with pytest.raises(ValueError):
        model.generate_batch(ps, 8, num_speculative_tokens=3, _spec_script=[WRONG])      # one script per sequence
    mx = _model(dev, quantization="mxfp4")
    with pytest.raises(ValueError, match="at most 4"):      # the mxfp4 step takes 4 rows
        mx.generate_batch(ps, 8, num_speculative_tokens=4)
    # mxfp4 with k = 3: no room for two sequences in a step of 4 rows - single-sequence groups, the same ids as the plain path
    assert mx.spec_group(3) == 1 and mx.spec_group(1) == 2
    got = mx.generate_batch(ps, NEW, bad_words_ids=BAD, num_speculative_tokens=3)
    assert not mx._spec_batches and len(mx.last_spec_stats) == 2
    plain = mx.generate_batch(ps, NEW, bad_words_ids=BAD)
    wprime = _mxfp4_wprime(_sd())
    for g, w, p in zip(got, plain, ps):
        assert torch.equal(g, mx.generate(input_ids=p, max_new_tokens=NEW, bad_words_ids=BAD, num_speculative_tokens=3))
        g, w = g[0].tolist(), w[0].tolist()
        diff = next((i for i in range(len(g)) if g[i] != w[i]), None)
        print(f"[spec-batch] mxfp4 k=3 fallback: first difference from the plain path {None if diff is None else diff - p.shape[1]}")
        # the verify attention sums in another order than the plain step's: equal, or apart at a near-tie of the oracle on the
        # dequantized weights (what test_spec_model_gpu.py::test_against_the_plain_path_and_the_oracle asks of the bf16 model)
        assert len(g) == len(w) and (diff is None or _near_tie(w[:diff], w[diff], g[diff], BAD, wprime))


def _mxfp4_wprime(sd):
    """the state dict whose layer matrices are the dequantized MXFP4 forms and whose lm_head is the dequantized FP8 form: the bf16
    model the mxfp4 model equals bit for bit (tests/test_mxfp4_gpu.py)"""
    from usdm_amd.quant import dequantize_mxfp4, dequantize_rows, quantize_mxfp4, quantize_rows
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight":
            out[k] = dequantize_rows(*quantize_rows(v.to(torch.bfloat16)))
        elif any(n in k for n in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")):
            out[k] = dequantize_mxfp4(*quantize_mxfp4(v.to(torch.bfloat16)))
    return out


def test_off_by_default(dev, prompts):
    m = _model(dev)
    a = m.generate_batch(prompts[:2], 12, bad_words_ids=BAD)
    for k in (None, 0):
        b = m.generate_batch(prompts[:2], 12, bad_words_ids=BAD, num_speculative_tokens=k)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and not m._spec_batches and m._spec is None


@pytest.mark.parametrize("what,B,k", [("fp8_mfma", 2, 7), ("mxfp4", 2, 1)])
def test_quantized_weights(dev, prompts, what, B, k):
    """fp8 weights on the matrix cores at (2, 7) and mxfp4 at (2, 1): the ids do not depend on the drafts"""
    m = _model(dev, quantization="fp8", fp8_matrix_cores=True) if what == "fp8_mfma" else _model(dev, quantization="mxfp4")
    assert m.spec_group(k) >= B
    ps = prompts[:B]
    wrong, st_w = _gen(m, ps, k, [WRONG] * B)
    own, st_o = _gen(m, ps, k, [list(w) for w in wrong])
    look, _ = _gen(m, ps, k)
    assert own == wrong and look == wrong and B in m._spec_batches
    assert st_w == [dict(steps=NEW - 1, drafted=k * (NEW - 1), accepted=0)] * B
    assert all(s["steps"] == -(-(NEW - 1) // (k + 1)) for s in st_o)
