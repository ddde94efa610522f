"""CPU: the host side of batched speculative decoding - the group sizing max_batch() // (k + 1), generate_batch's
argument checks (on a model object without weights: every check fires before the first launch), the eligibility split of a mixed
serving group, the numpy restatement of the batched commit, and the sizes of the two new ctypes structs."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import _spec_batch_reference as RB
from tests import _spec_reference as R


def _bare_model(max_batch=16, **kw):
    """a USDMForCausalLM without weights or buffers: what generate_batch's checks read"""
    from usdm_amd.llm import USDMForCausalLM
    m = object.__new__(USDMForCausalLM)
    m.cfg = dict(R.SMALL_CFG)
    m.tp_path, m.kv8, m.prefix_caching, m.ctx_max, m.spec_split, m.max_out = False, False, False, 256, 128, 128
    m.max_batch = lambda: max_batch
    m.__dict__.update(kw)
    return m


def test_group_sizing():
    for mb, k, want in ((16, 1, 8), (16, 3, 4), (16, 7, 2), (16, 2, 5), (16, 6, 2), (4, 1, 2), (4, 3, 1), (4, 2, 1)):
        assert _bare_model(mb).spec_group(k) == want == mb // (k + 1)
    from usdm_amd.serving import LLM
    srv = object.__new__(LLM)
    srv.spec, srv.prefix_caching, srv.max_slots, srv.llm = (3, 3, 1), False, 16, _bare_model(16)
    assert srv._spec_slot_count() == 4
    srv.max_slots = 3
    assert srv._spec_slot_count() == 3
    srv.max_slots, srv.llm = 16, _bare_model(4)
    assert srv._spec_slot_count() == 1                      # no room for two: everybody keeps the single path
    srv.llm, srv.prefix_caching = _bare_model(16), True
    assert srv._spec_slot_count() == 0                      # the prefix index and the speculative slots do not mix
    srv.spec, srv.prefix_caching = None, False
    assert srv._spec_slot_count() == 0


def test_generate_batch_argument_checks():
    m = _bare_model()
    ps = [torch.zeros(1, 5, dtype=torch.long), torch.zeros(1, 7, dtype=torch.long)]
    for bad in (8, -1, 2.5, True):
        with pytest.raises(ValueError):
            m.generate_batch(ps, 8, num_speculative_tokens=bad)
    for kw in (dict(prompt_lookup_max=0), dict(prompt_lookup_max=17), dict(prompt_lookup_max=2, prompt_lookup_min=3)):
        with pytest.raises(ValueError):
            m.generate_batch(ps, 8, num_speculative_tokens=2, **kw)
    for extra, word in ((dict(logprobs=1), "logprobs"), (dict(repetition_penalty=1.2), "penalties"), (dict(presence_penalty=[0.0, 0.5]), "penalties"),
                        (dict(logit_bias={3: 1.0}), "logit_bias"), (dict(no_repeat_ngram_size=[0, 2]), "no_repeat_ngram_size"),
                        (dict(min_p=0.1), "min_p")):
        with pytest.raises(NotImplementedError, match=word):
            m.generate_batch(ps, 8, num_speculative_tokens=3, **extra)
    with pytest.raises(NotImplementedError, match="unquantized"):
        _bare_model(kv8=True).generate_batch(ps, 8, num_speculative_tokens=3)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        _bare_model(tp_path=True).generate_batch(ps, 8, num_speculative_tokens=3)
    with pytest.raises(ValueError, match="at most 4"):
        _bare_model(4).generate_batch(ps, 8, num_speculative_tokens=4)
    with pytest.raises(ValueError, match="one script per sequence"):
        m.generate_batch(ps, 8, num_speculative_tokens=3, _spec_script=[[1, 2]])
    with pytest.raises(ValueError, match=r"\[1, L\]"):
        m.generate_batch([torch.zeros(5, dtype=torch.long)] * 2, 8, num_speculative_tokens=3)
    with pytest.raises(ValueError):      # one max_new_tokens per sequence, or one for all
        m.generate_batch(ps, [8, 8, 8], num_speculative_tokens=3)
    with pytest.raises(ValueError, match="keys per split"):
        _bare_model(ctx_max=128 * 65).generate_batch(ps, 8, num_speculative_tokens=3)
    # the slots refuse a model with the prefix index, by name, before anything is allocated
    from usdm_amd.slots import SpecSlots
    with pytest.raises(NotImplementedError, match="enable_prefix_caching"):
        SpecSlots(_bare_model(prefix_caching=True), 2, None)
    # no room for a single token: the prompts come back, with empty statistics
    full = [torch.zeros(1, 256, dtype=torch.long), torch.zeros(1, 9, dtype=torch.long)]
    out = m.generate_batch(full, 8, num_speculative_tokens=3)
    assert all(torch.equal(a, b) for a, b in zip(out, full)) and m.last_spec_stats == [dict(steps=0, drafted=0, accepted=0)] * 2


def test_stop_block():
    """slots.stop_block: {n, min_new, ids...} in 8 int32 words - the ids sorted and zero-padded; more than 6 ids: n = 0, no ids, and
    nothing for the device to check (the host checks every id anyway)"""
    from usdm_amd.slots import stop_block
    for stops, min_new, words, dev in ((set(), 0, [0, 0, 0, 0, 0, 0, 0, 0], []),
                                       ({9}, 3, [1, 3, 9, 0, 0, 0, 0, 0], [9]),
                                       ({40, 7, 300, 2, 11, 5}, 2, [6, 2, 2, 5, 7, 11, 40, 300], [2, 5, 7, 11, 40, 300]),
                                       ({40, 7, 300, 2, 11, 5, 1}, 4, [0, 4, 0, 0, 0, 0, 0, 0], []),
                                       ([8, 3], 1, [2, 1, 3, 8, 0, 0, 0, 0], [3, 8])):
        block, ids = stop_block(stops, min_new)
        assert block.dtype == torch.int32 and block.tolist() == words and ids == dev


def _req(i, **kw):
    from usdm_amd.serving import SamplingParams
    mask = kw.pop("mask", torch.zeros(8, dtype=torch.uint8))
    return dict(i=(i, 0), sp=SamplingParams(**dict(dict(temperature=0.0, max_tokens=8), **kw)), mask=mask)


def test_eligibility_split_of_a_mixed_group():
    from usdm_amd.serving import LLM
    srv = object.__new__(LLM)
    srv.spec, srv.prefix_caching, srv.max_slots, srv.llm = (3, 3, 1), False, 4, _bare_model(16)
    greedy = [_req(0), _req(1, top_k=1, temperature=1.0), _req(2, stop_token_ids=[3], min_tokens=2)]
    others = [_req(3, temperature=0.8, top_k=20), _req(4, logprobs=2), _req(5, repetition_penalty=1.3), _req(6, logit_bias={1: 2.0}),
              _req(7, no_repeat_ngram_size=2), _req(8, temperature=0.8, min_p=0.1), _req(9, mask=None)]
    assert all(srv._spec_eligible(r) for r in greedy) and not any(srv._spec_eligible(r) for r in others)
    fast, rest = srv._spec_split(greedy + others)
    assert [r["i"][0] for r in fast] == [0, 1, 2] and [r["i"][0] for r in rest] == [3, 4, 5, 6, 7, 8, 9]
    fast, rest = srv._spec_split([others[0], greedy[0], others[1]])      # a lone eligible request: nobody moves
    assert fast == [] and [r["i"][0] for r in rest] == [3, 0, 4]
    srv.llm = _bare_model(4)                                             # k = 3 on a step of 4 rows: one slot
    assert srv._spec_split(greedy + others)[0] == []
    srv.llm, srv.prefix_caching = _bare_model(16), True
    assert srv._spec_split(greedy + others)[0] == []
    srv.prefix_caching, srv.spec = False, None
    assert srv._spec_split(greedy)[0] == [] and not srv._spec_eligible(greedy[0])


def test_batch_reference_is_the_single_reference_slot_by_slot():
    for seed in range(50):
        states = RB.random_batch(seed)
        RB.check_batch(states)
        after = RB.spec_commit_batch_ref(states)
        for s, a in zip(states, after):
            one = R.spec_commit_ref(s)
            assert all(np.array_equal(a[k], one[k]) for k in ("drafts", "out_tokens", "counters"))
            assert all(a[k] == one[k] for k in ("step", "pos", "next_token", "done", "rows"))
        lo = seed % len(states)
        part = RB.spec_commit_batch_ref(states, lo, 1)
        for b, (s, a) in enumerate(zip(states, part)):
            if b != lo:
                assert a["rows"] is None and a["step"] == s["step"] and np.array_equal(a["out_tokens"], s["out_tokens"])


def test_struct_sizes_match_the_library():
    from usdm_amd import _lib
    assert _lib.lib.usdm_sizeof_attn_verify_batch_args() == C.sizeof(_lib.AttnVerifyBatchArgs)
    assert _lib.lib.usdm_sizeof_spec_batch_args() == C.sizeof(_lib.SpecBatchArgs)
    # the single-sequence structs are embedded unchanged at offset 0
    assert _lib.AttnVerifyBatchArgs.v.offset == 0 and _lib.AttnVerifyBatchArgs.v.size == _lib.lib.usdm_sizeof_attn_verify_args()
    assert _lib.SpecBatchArgs.s.offset == 0 and _lib.SpecBatchArgs.s.size == _lib.lib.usdm_sizeof_spec_args()
