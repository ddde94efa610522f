"""Sampled speculation without a GPU: the opt-in flag's argument checks, what stays refused, serving's eligibility
with and without the flag, the struct sizes against the library, the equivalence of "draw with the position's own uniform, accept
the draft iff it equals the draw" with textbook rejection sampling against a one-hot proposal in exact rational arithmetic, and the
choice of the replay test's seed."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import _sample_reference as SR
from tests import _spec_sample_reference as S


def test_flag_argument_checks():
    from usdm_amd.spec import check_spec_args, check_speculative_config, check_speculative_sampling, config_speculative_sampling
    assert check_speculative_sampling(False) is False and check_speculative_sampling(True) is True
    assert check_speculative_sampling(False, spec=False) is False
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="speculative_sampling"):
            check_speculative_sampling(bad)
    with pytest.raises(ValueError, match="num_speculative_tokens"):
        check_speculative_sampling(True, spec=False)
    # the 3-tuples stay what they are; the flag travels beside them
    assert check_spec_args(3) == (3, 3, 1)
    cfg = {"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_max": 5, "speculative_sampling": True}
    assert check_speculative_config(cfg) == (4, 5, 1) and config_speculative_sampling(cfg) is True
    assert config_speculative_sampling({"num_speculative_tokens": 2}) is False and config_speculative_sampling(None) is False
    with pytest.raises(ValueError):
        config_speculative_sampling({"num_speculative_tokens": 2, "speculative_sampling": 1})
    with pytest.raises(ValueError):
        config_speculative_sampling({"num_speculative_tokens": 0, "speculative_sampling": True})
    with pytest.raises(ValueError):
        check_speculative_config({"num_speculative_tokens": 2, "speculative_sampling": True, "model": "x"})


def test_what_the_flag_lifts_and_what_stays_refused():
    from usdm_amd.spec import check_spec_call
    check_spec_call(sampled=True, speculative_sampling=True)
    check_spec_call(sampled=True, min_p=0.1, speculative_sampling=True)
    check_spec_call(min_p=0.1, speculative_sampling=True)
    for kw, word in ((dict(logprobs=0), "logprobs"), (dict(penalties=(1.1, 0.0, 0.0)), "penalties"), (dict(edits=((), 2)), "no_repeat_ngram_size"),
                     (dict(logits_hook=lambda: None), "_logits_hook"), (dict(num_beams=2), "num_beams"), (dict(tensor_parallel=True), "tensor parallelism"),
                     (dict(kv_cache_fp8=True), "unquantized")):
        with pytest.raises(NotImplementedError, match=word):
            check_spec_call(sampled=True, speculative_sampling=True, **kw)
    with pytest.raises(NotImplementedError, match="sampling"):      # without the flag: today's refusal
        check_spec_call(sampled=True, speculative_sampling=False)
    with pytest.raises(NotImplementedError, match="min_p"):
        check_spec_call(min_p=0.1)


def test_generate_refuses_the_flag_without_speculation():
    """generate() / generate_batch() check the flag before they touch the device"""
    from usdm_amd.llm import USDMForCausalLM
    m = object.__new__(USDMForCausalLM)
    with pytest.raises(ValueError, match="num_speculative_tokens"):
        m.generate(input_ids=None, max_new_tokens=4, speculative_sampling=True)
    with pytest.raises(ValueError, match="speculative_sampling"):
        m.generate(input_ids=None, max_new_tokens=4, num_speculative_tokens=2, speculative_sampling="yes")
    with pytest.raises(ValueError, match="num_speculative_tokens"):
        m.generate_batch([], 4, speculative_sampling=True)
    # generate_batch's sampling arguments exist for the flag only: every one is refused without it, none silently ignored
    m.cfg = dict(vocab_size=10)
    for kw in (dict(do_sample=True), dict(temperature=0.8), dict(top_k=20), dict(top_p=0.9), dict(seed=1), dict(top_k=[None, 5]),
               dict(seed=3, num_speculative_tokens=2)):
        with pytest.raises(ValueError, match="generate_batch picks greedily"):
            m.generate_batch([None, None], 4, **kw)
    for bad in (-1, 2.5, True):      # with the flag a slot's top_k is checked on the host, as generate()'s is used
        with pytest.raises(ValueError, match="top_k"):
            m._slot_sampling(True, 1.0, bad, 1.0, 1, 0.0)
    assert m._slot_sampling(True, 0.8, 20, 0.9, 7, 0.05) == (0.8, 20, 0.9, 7, 0.05) and m._slot_sampling(True, 1.0, 1, 1.0, 7, 0.0) is None
    assert m._slot_sampling(False, 1.0, None, 1.0, None, 0.0) is None and m._slot_sampling(True, 1.0, None, 1.0, 7, 0.0) == (1.0, 0, 1.0, 7, 0.0)


def test_eligibility_with_and_without_the_flag():
    from usdm_amd.serving import LLM, SamplingParams
    srv = object.__new__(LLM)
    srv.spec = (3, 3, 1)
    assert srv.spec_sampling is False                                          # the class default: off where __init__ never ran
    req = lambda **kw: dict(sp=SamplingParams(max_tokens=8, **kw), mask=object())
    greedy, sampled = req(temperature=0.0), req(temperature=0.8, top_k=20, seed=1)
    minp, lp = req(temperature=0.8, min_p=0.1, seed=1), req(temperature=0.8, logprobs=0, seed=1)
    pen, hook = req(temperature=0.8, repetition_penalty=1.2, seed=1), dict(sp=SamplingParams(temperature=0.8, max_tokens=8), mask=None)
    assert [srv._spec_eligible(r) for r in (greedy, sampled, minp, lp, pen, hook)] == [True, False, False, False, False, False]
    srv.spec_sampling = True
    assert [srv._spec_eligible(r) for r in (greedy, sampled, minp, lp, pen, hook)] == [True, True, True, False, False, False]
    srv.spec = None
    assert not srv._spec_eligible(sampled)


CLI_BASE = ["--input_path", "x", "--model_cache_dir", "y", "--output_path", "z"]


def test_cli_flag_refusals(capsys):
    """The error itself - the last line of stderr, behind argparse's usage, which names every option whatever went wrong."""
    from usdm_amd import inference
    spec = ["--num_speculative_tokens", "3", "--speculative_sampling"]
    for extra, message in ((["--speculative_sampling"], "speculative_sampling=True needs num_speculative_tokens >= 1"),      # asks for nothing
                           (spec + ["--logprobs", "0"], "num_speculative_tokens > 0 with logprobs:"),                        # stays refused
                           (spec + ["--repetition_penalty", "1.2"], "num_speculative_tokens > 0 with repetition / presence / frequency penalties:"),
                           (spec + ["--no_repeat_ngram_size", "2"], "num_speculative_tokens > 0 with logit_bias / no_repeat_ngram_size:"),
                           (spec + ["--num_beams", "2"], "num_speculative_tokens > 0 with num_beams > 1:"),
                           (spec + ["--kv_cache_dtype", "fp8"], 'num_speculative_tokens > 0 with kv_cache_dtype="fp8":')):
        with pytest.raises(SystemExit) as e:
            inference.main(CLI_BASE + extra)
        last = capsys.readouterr().err.strip().splitlines()[-1]
        assert e.value.code == 2 and "error: " + message in last, (extra, last)


def test_cli_flag_reaches_the_rounds(monkeypatch, capsys):
    """--num_speculative_tokens 3 --speculative_sampling --min_p 0.1 passes the argument checks (without the flag min_p is their
    refusal) and sample() gets the flag, with the loaders and sample() replaced by recorders"""
    from usdm_amd import inference
    seen = []
    monkeypatch.setattr(inference, "load_models", lambda *a, **kw: (None,) * 5)
    monkeypatch.setattr(inference, "sample", lambda *a, **kw: seen.append(kw))
    argv = CLI_BASE + ["--num_speculative_tokens", "3", "--min_p", "0.1"]
    with pytest.raises(SystemExit) as e:
        inference.main(argv)
    assert e.value.code == 2 and "error: num_speculative_tokens > 0 with min_p:" in capsys.readouterr().err.strip().splitlines()[-1] and not seen
    assert inference.main(argv + ["--speculative_sampling"]) == 0
    assert len(seen) == 1 and seen[0]["speculative_sampling"] is True and seen[0]["min_p"] == 0.1 and seen[0]["num_speculative_tokens"] == 3
    assert inference.main(CLI_BASE + ["--num_speculative_tokens", "3"]) == 0 and seen[1]["speculative_sampling"] is False      # default: off


def test_struct_sizes_match_the_library():
    from usdm_amd import _lib
    assert _lib.lib.usdm_sizeof_spec_sample_args() == ctypes.sizeof(_lib.SpecSampleArgs) == 72
    assert _lib.SpecSampleArgs.V.offset == 16 and _lib.SpecSampleArgs.dev_params.offset == 32 and _lib.SpecSampleArgs.picks.offset == 64
    # the picks forms take the arg-max forms' structs, which have not moved
    assert _lib.lib.usdm_sizeof_spec_args() == ctypes.sizeof(_lib.SpecArgs) and _lib.SpecArgs.drafts.offset == 24
    assert _lib.lib.usdm_sizeof_spec_batch_args() == ctypes.sizeof(_lib.SpecBatchArgs) and _lib.SpecBatchArgs.s.offset == 0
    assert _lib.lib.usdm_sizeof_sample_args() == ctypes.sizeof(_lib.SampleArgs)
    for name in ("usdm_spec_sample", "usdm_spec_commit_picks", "usdm_spec_commit_batch_picks"):
        assert getattr(_lib.lib, name).restype is ctypes.c_int


# ------------------------------------------------------------------------------------------------ the equivalence, in rationals
def _masses(seed, V=12, **knobs):
    """filter_ref's integer masses of a small seeded row -> the exact rational token law p"""
    g = np.random.default_rng(seed)
    row = (g.standard_normal(V) * 2).astype(np.float32)
    row[g.random(V) < 0.25] = -np.inf
    row[int(g.integers(V))] = 1.0                                              # at least one finite logit
    F = SR.filter_ref(row, **knobs)
    assert F.Zk > 0
    return [Fraction(int(m), F.Zk) for m in F.mass]


@pytest.mark.parametrize("knobs", [dict(), dict(temperature=0.8, top_k=5), dict(temperature=1.3, top_p=0.7), dict(top_k=4, top_p=0.9, min_p=0.2),
                                   dict(top_k=1)])
def test_accept_if_equal_is_rejection_sampling_against_a_one_hot_proposal(knobs):
    for seed in range(20):
        p = _masses(seed, **knobs)
        assert sum(p) == 1
        for d in list(range(len(p))) + [-1]:                                   # every draft, with and without mass, and "no draft"
            law_a, acc_a = S.law_accept_if_equal(p, d)
            law_r, acc_r = S.law_rejection_sampling(p, d)
            assert law_a == law_r and acc_a == acc_r == (p[d] if d >= 0 else 0), (seed, d)
            assert sum(law_a.values()) == 1 and law_a == {x: px for x, px in enumerate(p) if px}      # the plain sampled call's law


def test_the_replay_seed_has_slack_on_the_oracle_trajectory():
    """tests/test_spec_sample_model_gpu.py replays the sampled speculative call over its own logits rows with REPLAY_SEED.  On the
    oracle's teacher-forced rows of that trajectory every draw is at least 10 * SLACK away from a neighbouring id's interval, so the
    few ulp between the kernel's fast exp and numpy's, and the bf16 grain between the model and the oracle, leave room; and no smaller
    seed has that property (the seed is the first, not a favourable pick among many)."""
    toks, slacks = S.oracle_trajectory(S.REPLAY_SEED, **S.KNOBS_TK)
    assert len(toks) == 49 and min(slacks) >= S.REPLAY_SLACK, min(slacks)
    assert len(set(toks)) > 10 and S.BANNED not in toks                        # it does sample
    for seed in range(S.REPLAY_SEED):
        assert min(S.oracle_trajectory(seed, **S.KNOBS_TK)[1]) < S.REPLAY_SLACK, seed
