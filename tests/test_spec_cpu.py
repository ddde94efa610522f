"""Speculative decoding without a GPU: the numpy restatement of usdm_spec_commit (tests/_spec_reference.py) on hand-built cases, the
proposer's cases, the seed and ban mask of the GPU lookup test checked on the CPU oracle, argument validation and refusals, and the
ctypes structs against the library's usdm_sizeof_* functions."""
import ctypes

import pytest
import torch

from tests import _spec_reference as R


def test_hand_cases_give_the_expected_words():
    """accept counts, a stop id inside an accepted run, min_new, limit / max_out cuts, ties, and every proposer case"""
    names = set()
    for name, s, exp in R.hand_cases():
        a = R.spec_commit_ref(s)
        got = dict(emitted=R.emitted(s, a), done=a["done"], drafts=a["drafts"][1:s["T"]].tolist(),
                   steps=int(a["counters"][0] - s["counters"][0]), drafted=int(a["counters"][1] - s["counters"][1]),
                   accepted=int(a["counters"][2] - s["counters"][2]))
        for k, v in exp.items():
            assert got[k] == v, (name, k, got[k], v)
        m = len(got["emitted"])
        assert a["step"] == s["step"] + m and a["pos"] == s["pos"] + m and got["accepted"] == max(0, m - 1) * got["steps"]
        if m:
            assert a["next_token"] == got["emitted"][-1]
        assert name not in names
        names.add(name)
    for need in ("no match", "two matches, the most recent wins", "longest n first", "continuation runs off the end", "history shorter than n",
                 "stop id inside the accepted run", "stop id under min_new is passed", "limit cuts the run", "max_out cuts the run",
                 "ties go to the lowest id, NaN never wins"):
        assert need in names


def test_done_launch_changes_nothing():
    s = R.from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], done=1, counters=(4, 5, 6))
    a = R.spec_commit_ref(s)
    assert a["rows"] is None and a["step"] == 1 and (a["drafts"] == s["drafts"]).all() and (a["counters"] == s["counters"]).all()


def test_proposer_properties_on_random_histories():
    """the draft is always the continuation of an EARLIER occurrence of the tail, the most recent one of the longest n that matches"""
    import numpy as np
    g = np.random.default_rng(0)
    for _ in range(300):
        hist = g.integers(0, 4, int(g.integers(1, 40))).tolist()
        lmax, lmin, k = int(g.integers(1, 5)), 1, int(g.integers(1, 8))
        d = R.propose(hist, k, lmax, lmin)
        Lh = len(hist)
        found = None
        for n in range(lmax, lmin - 1, -1):
            js = [j for j in range(Lh - n) if hist[j:j + n] == hist[Lh - n:]]
            if Lh >= n + 1 and js:
                found = (n, max(js))
                break
        if found is None:
            assert d == [-1] * k
        else:
            n, j = found
            assert d == [(hist[j + n + i] if j + n + i < Lh else -1) for i in range(k)] and d[0] >= 0


def test_simulated_run_over_a_periodic_output():
    out = [1, 2, 3] * 16
    steps, drafted, accepted = R.simulate_lookup([9, 9], out, 3)
    assert steps + accepted == len(out) - 1 and accepted >= 30
    steps, drafted, accepted = R.simulate_lookup([9, 9], list(range(100, 148)), 3)
    assert (steps, drafted, accepted) == (47, 0, 0)


def test_lookup_seed_accepts_on_the_cpu_oracle():
    """The seed and the 3-id ban mask of tests/test_spec_model_gpu.py::test_lookup_with_a_ban_mask: over the oracle's greedy output
    the restated proposer accepts at least 8 drafts in 48 tokens, so the GPU test's `accepted > 0` neither passes nor fails by luck."""
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(R.SMALL_CFG, R.MODEL_SEED)
    ids = R.small_prompt()
    out = MO.greedy_generate(sd, R.SMALL_CFG, ids, R.NEW, bad_words_ids=R.lookup_bad_words())
    gen = out[len(ids):]
    assert len(gen) == R.NEW and set(gen) <= set(R.LOOKUP_KEEP)
    steps, drafted, accepted = R.simulate_lookup(ids.tolist(), gen, R.LOOKUP_K)
    print(f"[spec] lookup seed: {steps} steps, {drafted} drafted, {accepted} accepted over {R.NEW - 1} tokens")
    assert accepted >= 8 and steps + accepted == R.NEW - 1


def test_attention_reference_agrees_with_itself_across_bases():
    """the float64 reference: the token at position p gets the same output whichever row of a step it is"""
    Hq, Hkv, cm = 4, 2, 64
    g = torch.Generator().manual_seed(1)
    qa = torch.randn(cm, (Hq + 2 * Hkv) * 128, generator=g).to(torch.bfloat16)
    tab = R.rope_tables(cm)
    rows = qa.view(cm, Hq + 2 * Hkv, 128)
    K = torch.stack([R.rope_rows(rows[p, Hq:Hq + Hkv], p, tab) for p in range(cm)], 1)
    V = rows[:, Hq + Hkv:].transpose(0, 1).contiguous()
    p = 20
    outs = []
    for T, i in ((1, 0), (4, 3), (8, 5)):
        o, w, kr, vr = R.attn_verify_ref(qa[p - i:p - i + T], K, V, p - i, Hq=Hq, Hkv=Hkv, window=7, scale=128 ** -0.5, tables=tab)
        outs.append(o[i])
        assert bool((w[i, :, :p - 6] == 0).all()) and bool((w[i, :, p + 1:] == 0).all()) and torch.equal(kr[i], K[:, p])
    assert torch.allclose(outs[0], outs[1], rtol=0, atol=1e-12) and torch.allclose(outs[0], outs[2], rtol=0, atol=1e-12)
    o, _, kr, _ = R.attn_verify_ref(qa[:4], K, V, cm - 2, Hq=Hq, Hkv=Hkv, window=0, scale=1.0, tables=tab)
    assert o.shape[0] == 2 and kr.shape[0] == 2      # rows past the cache are dropped


def test_argument_validation():
    from usdm_amd.spec import check_spec_args, check_speculative_config
    assert check_spec_args(None) is None and check_spec_args(0) is None
    assert check_spec_args(3) == (3, 3, 1) and check_spec_args(7, 5, 2) == (7, 5, 2)
    for bad in (dict(num_speculative_tokens=8), dict(num_speculative_tokens=-1), dict(num_speculative_tokens=True),
                dict(num_speculative_tokens=2.0), dict(num_speculative_tokens=2, prompt_lookup_max=0),
                dict(num_speculative_tokens=2, prompt_lookup_max=17), dict(num_speculative_tokens=2, prompt_lookup_min=0),
                dict(num_speculative_tokens=2, prompt_lookup_max=2, prompt_lookup_min=3)):
        with pytest.raises(ValueError):
            check_spec_args(**bad)
    assert check_speculative_config(None) is None
    assert check_speculative_config({"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_max": 5}) == (4, 5, 1)
    assert check_speculative_config({"num_speculative_tokens": 2}) == (2, 3, 1)
    for method in ("eagle", "medusa", "draft_model", "mlp_speculator"):
        with pytest.raises(NotImplementedError, match=method):
            check_speculative_config({"method": method, "num_speculative_tokens": 2})
    for bad in ({"method": "ngram"}, {"num_speculative_tokens": 2, "model": "x"}, "ngram"):
        with pytest.raises(ValueError):
            check_speculative_config(bad)


def test_refusals_name_their_reason():
    from usdm_amd.spec import check_spec_call
    check_spec_call()
    check_spec_call(num_beams=1)
    for kw, word in ((dict(sampled=True), "sampling"), (dict(logprobs=0), "logprobs"), (dict(penalties=(1.1, 0.0, 0.0)), "penalties"),
                     (dict(edits=((), 2)), "no_repeat_ngram_size"), (dict(min_p=0.1), "min_p"), (dict(logits_hook=lambda: None), "_logits_hook"),
                     (dict(num_beams=2), "num_beams"), (dict(tensor_parallel=True), "tensor parallelism"), (dict(kv_cache_fp8=True), "unquantized")):
        with pytest.raises(NotImplementedError, match=word):
            check_spec_call(**kw)


def test_struct_sizes_match_the_library():
    from usdm_amd import _lib
    assert _lib.lib.usdm_sizeof_attn_verify_args() == ctypes.sizeof(_lib.AttnVerifyArgs)
    assert _lib.lib.usdm_sizeof_spec_args() == ctypes.sizeof(_lib.SpecArgs)
    # the fields a C caller fills sit where the header puts them
    assert _lib.AttnVerifyArgs.pos.offset == 16 and _lib.AttnVerifyArgs.C.offset == 40 and _lib.SpecArgs.drafts.offset == 24


def test_cli_refuses_bad_combinations():
    from usdm_amd import inference
    base = ["--input_path", "x", "--model_cache_dir", "y", "--output_path", "z", "--num_speculative_tokens"]
    for extra in (["9"], ["3", "--logprobs", "2"], ["3", "--num_beams", "2"], ["3", "--kv_cache_dtype", "fp8"], ["3", "--prompt_lookup_min", "4"]):
        with pytest.raises(SystemExit) as e:
            inference.main(base + extra)
        assert e.value.code == 2
