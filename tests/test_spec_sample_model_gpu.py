"""Sampled speculation through generate(), generate_batch() and serving.LLM on the small model of
tests/_spec_reference.py (ctx_max 256, one GPU).  A call generates NEW = 49 tokens: the prefill's pick, drawn by usdm_sample_final at
counter 0, and 48 from speculative steps, whose rows usdm_spec_sample draws at the counters of their positions.
Scripts: `script[j]` is the draft for output j.  The all-wrong script holds a BANNED id, which no draw can equal.

The replay test compares every emitted token with tests/_sample_reference.py's sampler on the row the step itself materialised.  The
kernel's fast exp and numpy's differ by a few ulp, which can move a draw whose target lies within SLACK = 1e-4 of a neighbouring id's
interval: such draws are excluded, and at most 2 of the 48 may be (a condition, set before any run; the seed was chosen on the CPU
from the oracle's trajectory, tests/test_spec_sample_cpu.py)."""
import numpy as np
import pytest
import torch

from tests import _sample_reference as SR
from tests import _spec_reference as R
from tests import _spec_sample_reference as S

pytestmark = pytest.mark.gpu
NEW, L0 = R.NEW, R.PROMPT_LEN
BANNED, BAD = S.BANNED, [[S.BANNED]]
SEED = 1234


@pytest.fixture(scope="module")
def sd():
    from oracle import mistral_oracle as MO
    return MO.random_state_dict(R.SMALL_CFG, R.MODEL_SEED)


def _model(dev, sd, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.from_state_dict(sd, R.SMALL_CFG, dev, ctx_max=256, **kw)


@pytest.fixture(scope="module")
def model(dev, sd):
    return _model(dev, sd)


@pytest.fixture(scope="module")
def prompt(dev):
    return R.small_prompt()[None].to(dev)


def _gen(m, prompt, k, script=None, seed=SEED, knobs=S.KNOBS_TK, new=NEW, **kw):
    out = m.generate(input_ids=prompt, max_new_tokens=new, bad_words_ids=BAD, do_sample=True, seed=seed, num_speculative_tokens=k,
                     speculative_sampling=True, _spec_script=script, **knobs, **kw)
    return out[0, prompt.shape[1]:].tolist(), m.last_spec_stats


def _four_scripts(m, prompt, k, **kw):
    """the all-wrong, own-output, every-third-corrupted and lookup runs -> their (ids, stats)"""
    wrong = _gen(m, prompt, k, [BANNED] * (NEW + 8), **kw)
    own = _gen(m, prompt, k, list(wrong[0]), **kw)
    third = _gen(m, prompt, k, [BANNED if j % 3 == 0 else t for j, t in enumerate(wrong[0])], **kw)
    look = _gen(m, prompt, k, **kw)
    return wrong, own, third, look


def _check_four(runs, k):
    (wrong, st_w), (own, st_o), (third, st_t), (look, st_l) = runs
    assert len(wrong) == NEW and BANNED not in wrong and len(set(wrong)) > 10           # it samples
    assert own == wrong and third == wrong and look == wrong
    assert st_w == dict(steps=NEW - 1, drafted=k * (NEW - 1), accepted=0)
    full, rest = divmod(NEW - 1, k + 1)
    assert st_o["steps"] == -(-(NEW - 1) // (k + 1)) and st_o["accepted"] == full * k + max(0, rest - 1)      # own output: everything accepted
    assert 0 < st_t["accepted"] < st_o["accepted"]
    for st in (st_w, st_o, st_t, st_l):
        assert st["accepted"] + st["steps"] == NEW - 1 and st["accepted"] <= st["drafted"] <= k * st["steps"]


@pytest.mark.parametrize("knobs", [S.KNOBS_TK, S.KNOBS_ALL], ids=["top_k", "top_k+top_p+min_p"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_ids_do_not_depend_on_the_drafts(model, prompt, k, knobs):
    _check_four(_four_scripts(model, prompt, k, knobs=knobs), k)


def test_ids_do_not_depend_on_the_drafts_fp8(dev, sd, prompt):
    _check_four(_four_scripts(_model(dev, sd, quantization="fp8"), prompt, 3), 3)


def test_seeds_and_the_plain_call(model, prompt):
    """another seed gives other ids; the first token is the plain sampled call's: the prefill's draw at counter 0 (behind it the verify
    attention sums in another order than the decode attention, so the logits agree up to rounding and a draw may move)"""
    a, _ = _gen(model, prompt, 3, seed=SEED)
    b, _ = _gen(model, prompt, 3, seed=SEED + 1)
    assert a != b
    plain = model.generate(input_ids=prompt, max_new_tokens=NEW, bad_words_ids=BAD, do_sample=True, seed=SEED, **S.KNOBS_TK)[0, L0:].tolist()
    assert plain[0] == a[0] and len(plain) == NEW


def test_replay_over_its_own_rows(model, prompt):
    k, T, rec = 3, 4, []
    toks, st = _gen(model, prompt, k, seed=S.REPLAY_SEED, _spec_on_step=rec.append)
    assert len(toks) == NEW and len(rec) == st["steps"] and st["accepted"] + st["steps"] == NEW - 1
    checked, excluded = 0, 0
    for r in rec:
        s0, drafts, rows = r["step"], r["drafts"], r["rows"].numpy()
        assert rows.shape == (T, R.SMALL_CFG["vocab_size"]) and np.isneginf(rows[:, BANNED]).all()
        n = 0                                                  # the accepted run, from the emitted tokens themselves
        while n < T - 1 and s0 + n < NEW and drafts[n + 1] == toks[s0 + n]:
            n += 1
        for i in range(n + 1):
            if s0 + i >= NEW:
                break
            _, _, want, slack = SR.sample_ref(rows[i], s0 + i, seed=S.REPLAY_SEED, **S.KNOBS_TK)
            checked += 1
            if slack < SR.SLACK:
                excluded += 1
                continue
            assert toks[s0 + i] == want == r["picks"][i], (s0, i, slack)
    print(f"replay: {checked} tokens checked, {excluded} excluded for slack < {SR.SLACK}")
    assert checked == NEW - 1 and excluded <= 2


def test_greedy_inside_the_sampled_step(model, prompt):
    for k in (1, 3):
        want = model.generate(input_ids=prompt, max_new_tokens=NEW, bad_words_ids=BAD, num_speculative_tokens=k)[0, L0:].tolist()
        st_w = model.last_spec_stats
        got = model.generate(input_ids=prompt, max_new_tokens=NEW, bad_words_ids=BAD, do_sample=True, top_k=1, num_speculative_tokens=k,
                             speculative_sampling=True)[0, L0:].tolist()
        assert got == want and model.last_spec_stats == st_w
        assert (k + 1, "sampled") in model._spec.spec_steps


# ------------------------------------------------------------------------------------------------ slots
def _prompts(dev, n):
    g = torch.Generator().manual_seed(R.PROMPT_SEED + 1)
    return [torch.randint(0, R.SMALL_CFG["vocab_size"], (L,), generator=g)[None].to(dev) for L in (24, 17, 31, 20)[:n]]


SLOT_KNOBS = dict(do_sample=[True, True, False, True], temperature=[0.8, 1.2, 1.0, 0.7], top_k=[20, 0, None, 50], top_p=[1.0, 0.9, 1.0, 0.95],
                  min_p=[0.0, 0.05, 0.0, 0.0], seed=[11, 2 ** 40 + 7, 0, 13])


def _slot_kw(n, idx=None):
    return {k: (v[:n] if idx is None else v[idx]) for k, v in SLOT_KNOBS.items()}


def test_slots_equal_the_single_sequence_call(dev, model):
    """(B, k) = (2, 1): 4 rows, the VALU projections - every sequence equals its own sampled speculative call bit for bit"""
    ps = _prompts(dev, 2)
    outs = model.generate_batch(ps, NEW, bad_words_ids=BAD, num_speculative_tokens=1, speculative_sampling=True, **_slot_kw(2))
    stats = model.last_spec_stats
    assert (2, "sampled") in model.spec_slots(2).spec_steps and outs[0][0, ps[0].shape[1]:].tolist() != outs[1][0, ps[1].shape[1]:].tolist()
    for b, (p, o) in enumerate(zip(ps, outs)):
        kw = _slot_kw(2, b)
        one = model.generate(input_ids=p, max_new_tokens=NEW, bad_words_ids=BAD, num_speculative_tokens=1, speculative_sampling=True,
                             **dict(kw, top_k=kw["top_k"] or None))
        assert torch.equal(o, one), b
        assert model.last_spec_stats == stats[b] and stats[b]["steps"] + stats[b]["accepted"] == NEW - 1


def test_slots_ids_depend_on_neither_scripts_nor_neighbours(dev, model):
    """(B, k) = (4, 3): 16 rows on the matrix cores; slot 2 is greedy inside the sampled step"""
    ps, B, k = _prompts(dev, 4), 4, 3
    run = lambda prompts, scripts, **kw: [o[0, p.shape[1]:].tolist() for p, o in zip(prompts, model.generate_batch(
        prompts, NEW, bad_words_ids=BAD, num_speculative_tokens=k, speculative_sampling=True, _spec_script=scripts, **kw))]
    wrong = run(ps, [[BANNED] * (NEW + 8)] * B, **_slot_kw(B))
    st_w = model.last_spec_stats
    assert all(len(t) == NEW for t in wrong) and all(s == dict(steps=NEW - 1, drafted=k * (NEW - 1), accepted=0) for s in st_w)
    own = run(ps, [list(t) for t in wrong], **_slot_kw(B))
    st_o = model.last_spec_stats
    look = run(ps, None, **_slot_kw(B))
    assert own == wrong and look == wrong
    assert all(s["steps"] == -(-(NEW - 1) // (k + 1)) and s["steps"] + s["accepted"] == NEW - 1 for s in st_o)
    # other neighbours: the slots in another order, each with its own knobs
    perm = [2, 0, 3, 1]
    kw = {name: [v[i] for i in perm] for name, v in SLOT_KNOBS.items()}
    moved = run([ps[i] for i in perm], [[BANNED] * (NEW + 8)] * B, **kw)
    assert [moved[perm.index(i)] for i in range(B)] == wrong


# ------------------------------------------------------------------------------------------------ serving
def test_serving(dev, model, prompt):
    from usdm_amd.serving import LLM, SamplingParams
    ids, ids2 = prompt[0].tolist(), prompt[0].tolist()[:-3]
    cfg = {"method": "ngram", "num_speculative_tokens": 3, "speculative_sampling": True}
    sps = [SamplingParams(temperature=0.8, top_k=20, seed=11, max_tokens=NEW), SamplingParams(temperature=1.2, top_p=0.9, min_p=0.05, seed=12, max_tokens=NEW)]
    srv = LLM(model=model, speculative_config=cfg, max_num_seqs=2)      # two speculative slots: the slots generate_batch runs two prompts on
    assert srv.stats["spec_sampled_requests"] == 0
    outs = srv.generate(prompt_token_ids=[ids, ids2], sampling_params=sps)
    st = srv.stats
    assert st["spec_batched_requests"] == 2 and st["spec_sampled_requests"] == 2 and st["spec_requests"] == 0
    t = lambda x: torch.tensor([x], dtype=torch.long, device=dev)
    want = model.generate_batch([t(ids), t(ids2)], NEW, num_speculative_tokens=3, speculative_sampling=True, do_sample=True,
                                temperature=[0.8, 1.2], top_k=[20, 0], top_p=[1.0, 0.9], min_p=[0.0, 0.05], seed=[11, 12])
    for o, w, p in zip(outs, want, (ids, ids2)):
        assert list(o.outputs[0].token_ids) == w[0, len(p):].tolist()
    # a lone sampled request: the single-sequence sampled speculative step
    one = srv.generate(prompt_token_ids=[ids], sampling_params=sps[0])
    assert srv.stats["spec_requests"] == 1 and srv.stats["spec_sampled_requests"] == 3 and srv.stats["spec_batched_requests"] == 2
    alone = model.generate(input_ids=prompt, max_new_tokens=NEW, do_sample=True, temperature=0.8, top_k=20, seed=11, num_speculative_tokens=3,
                           speculative_sampling=True)
    assert list(one[0].outputs[0].token_ids) == alone[0, L0:].tolist()
