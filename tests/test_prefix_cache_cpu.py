"""CPU: the prefix index of the batch slots (usdm_amd/prefix.py, enable_prefix_caching): which rows of which slot a new prompt may
reuse.  Host bookkeeping only - the module must not need torch."""
import subprocess
import sys

import pytest

from usdm_amd.prefix import MIN_MATCH, PrefixIndex, common_prefix, reusable_past


def _ids(n, base=0):
    return [base + i for i in range(n)]


def test_module_imports_without_torch():
    code = "import sys; import usdm_amd.prefix; assert 'torch' not in sys.modules, 'usdm_amd.prefix pulled torch in'"
    assert subprocess.run([sys.executable, "-c", code], cwd=__file__.rsplit("/tests/", 1)[0]).returncode == 0


def test_common_prefix():
    assert common_prefix([1, 2, 3], [1, 2, 4], 10) == 2
    assert common_prefix([1, 2, 3], [1, 2, 3, 4], 10) == 3
    assert common_prefix([1, 2, 3], [1, 2, 3], 2) == 2
    assert common_prefix([], [1], 5) == 0


def test_reusable_past_floor_of_16_tokens():
    assert reusable_past(_ids(40), _ids(15) + [777] * 30, 39, 45, True) == 0      # 15 common tokens: none
    assert reusable_past(_ids(40), _ids(16) + [777] * 30, 39, 46, True) == 16     # 16: a match
    assert reusable_past(_ids(40), _ids(40), 15, 40, False) == 0                  # a cap below the floor: none either


def test_reusable_past_caps():
    L, cached = 50, _ids(80)
    assert reusable_past(_ids(L), cached, L - 1, 80, True) == 49       # generate(): the last token is always prefilled
    assert reusable_past(_ids(L), _ids(30), L - 1, 30, True) == 30     # a shorter cached sequence: all of it
    start = 41                                                        # score(): rows start - 1 .. L - 2 are scored, so at most start - 1 are skipped
    assert reusable_past(_ids(L), cached, start - 1, 80, True) == 40
    assert reusable_past(_ids(L), _ids(20) + [999] * 60, start - 1, 80, True) == 20      # the common prefix ends below the cap


def test_reusable_past_exact_clamps_to_the_prefill_written_rows():
    cached = _ids(60)      # 40 rows written by a prefill, 20 appended by decode steps
    assert reusable_past(_ids(70), cached, 69, 40, True) == 40
    assert reusable_past(_ids(70), cached, 69, 40, False) == 60
    assert reusable_past(_ids(70), cached, 69, 10, True) == 0          # the clamp comes before the floor: 10 written rows are none
    assert reusable_past(_ids(70), cached, 69, 10, False) == 60


@pytest.mark.parametrize("cached", [None, [], ()])
def test_reusable_past_without_a_cache(cached):
    assert reusable_past(_ids(50), cached, 49, 0, True) == 0
    assert reusable_past(_ids(50), cached, 49, 50, False) == 0


def test_empty_index_matches_nothing():
    px = PrefixIndex(4, 256)
    assert px.match(_ids(50), 0) == (None, 0)
    assert [px.length(s) for s in range(4)] == [0, 0, 0, 0]


def test_longest_match_over_slots_including_an_active_one():
    px = PrefixIndex(4, 256)
    px.admit(1, _ids(40))                     # slot 1: still decoding as far as the scheduler knows - the index does not care
    px.admit(3, _ids(64) + [999] * 10)
    px.admit(2, _ids(30, base=5000))
    prompt = _ids(100)
    assert px.match(prompt, 0) == (3, 64)     # the longest one, not the first one
    assert px.match(prompt, 1) == (3, 64)     # ... even when the target holds a shorter match itself
    assert px.match(_ids(100, base=5000), 0) == (2, 30)


def test_cap_at_len_minus_one():
    px = PrefixIndex(2, 256)
    px.admit(0, _ids(50))
    assert px.match(_ids(50), 1) == (0, 49)   # the same prompt again (n > 1): everything but the last token
    assert px.match(_ids(50), 0) == (0, 49)
    assert px.match(_ids(30), 1) == (0, 29)   # a prompt that is a prefix of the entry
    assert px.match(_ids(51), 1) == (0, 50)   # one token more than the entry: the whole entry


def test_floor_of_16_tokens():
    assert MIN_MATCH == 16
    px = PrefixIndex(2, 256)
    px.admit(0, _ids(15) + [777] * 30)
    assert px.match(_ids(40), 1) == (None, 0)                # 15 common tokens: none
    px.admit(0, _ids(16) + [777] * 30)
    assert px.match(_ids(40), 1) == (0, 16)                  # 16: a match
    px.admit(0, _ids(17))
    assert px.match(_ids(17), 1) == (0, 16)                  # capped to 16 by len - 1: still a match
    assert px.match(_ids(16), 1) == (None, 0)                # capped to 15: none


def test_ties_go_to_the_target_then_to_the_lowest_slot():
    px = PrefixIndex(4, 256)
    for s in (1, 2, 3):
        px.admit(s, _ids(40) + [s] * 5)
    prompt = _ids(40) + [9] * 5
    assert px.match(prompt, 2) == (2, 40)     # the target itself: no copy needed
    assert px.match(prompt, 0) == (1, 40)     # else the lowest slot
    assert px.match(prompt, 3) == (3, 40)
    px.admit(2, _ids(41) + [2] * 5)           # a strictly longer match elsewhere beats the target's own
    assert px.match(_ids(60), 3) == (2, 41)


def test_entry_after_admission_is_the_prompt_and_decoded_ids_are_never_recorded():
    px = PrefixIndex(2, 256)
    prompt = _ids(40)
    px.admit(0, prompt)
    assert px.entries[0] == tuple(prompt) and px.length(0) == 40
    # the slot then generated 12 tokens; a prompt that extends prompt + generated reuses the PROMPT's rows only (the rows behind
    # them were appended by decode steps: there is no call that could record them)
    generated = [7000 + i for i in range(12)]
    assert px.match(prompt + generated + [1, 2, 3], 1) == (0, 40)
    assert px.match(prompt + generated + [1, 2, 3], 0) == (0, 40)
    assert not hasattr(px, "append") and not hasattr(px, "extend")
    px.admit(0, _ids(20, base=300))           # a new admission replaces the entry
    assert px.entries[0] == tuple(_ids(20, base=300))
    assert px.match(prompt + [5], 1) == (None, 0)
    prompt.append(1)                          # the entry is a copy, not the caller's list
    assert px.length(0) == 20


def test_parking_position_and_drop_near_ctx_max():
    px = PrefixIndex(3, 256, chunk=8)
    assert px.park(0) == 0                    # nothing recorded: row 0, as without the option
    px.admit(0, _ids(100))
    assert px.park(0) == 100 and px.length(0) == 100          # behind the recorded rows, which stay
    px.admit(1, _ids(247))                    # 9 rows left: chunk + 1, still room for a chunk of garbage rows 247 .. 254
    assert px.park(1) == 247 and px.length(1) == 247
    px.admit(2, _ids(248))                    # 8 rows left: fewer than chunk + 1 -> dropped, parked at 0
    assert px.park(2) == 0 and px.length(2) == 0 and px.entries[2] is None
    assert px.match(_ids(250), 0) == (1, 247)


def test_reset_prefix_cache_clears_all_entries():
    px = PrefixIndex(3, 256)
    for s in range(3):
        px.admit(s, _ids(30 + s))
    px.reset()
    assert px.entries == [None] * 3 and px.match(_ids(40), 0) == (None, 0)
    px.drop(1)                                # dropping an empty entry is harmless
    px.admit(1, _ids(20))
    px.drop(1)
    assert px.length(1) == 0


def test_replay_of_an_admission_order():
    """what the serving test replays: rows reused over a sequence of (slot, prompt) admissions"""
    px, reused = PrefixIndex(2, 256), []
    fam = _ids(40)
    for slot, prompt in ((0, fam + [1] * 10), (1, fam + [2] * 10), (0, _ids(30, base=900)), (1, fam + [2] * 10 + [3] * 4), (0, fam + [1] * 10)):
        reused.append(px.match(prompt, slot))
        px.admit(slot, prompt)
    assert reused == [(None, 0), (0, 40), (None, 0), (1, 50), (1, 40)]


@pytest.mark.parametrize("flag_env", ["0", "off"])
def test_flag_with_reuse_switched_off_is_a_value_error_before_anything_else(monkeypatch, flag_env):
    from usdm_amd.llm import USDMForCausalLM
    monkeypatch.setenv("USDM_PREFIX_REUSE", flag_env)
    with pytest.raises(ValueError, match="USDM_PREFIX_REUSE"):
        USDMForCausalLM(dict(head_dim=128), "cpu", enable_prefix_caching=True)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        USDMForCausalLM(dict(head_dim=128), "cpu", enable_prefix_caching=True, tp_size=2)
