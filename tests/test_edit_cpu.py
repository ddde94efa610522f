"""CPU: the semantics of logit_bias, no_repeat_ngram_size and min_p (tests/_edit_reference.py, the numpy restatement the GPU tests
compare usdm_logit_edit and usdm_sample_final with) against the installed transformers, the range checks of the public surface, the
step key, and the library's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _edit_reference as E

NAN, INF = float("nan"), float("inf")


def _row(V, seed, ninf=True):
    x = E.bf16_row(V, seed)
    if ninf:
        x[np.random.default_rng(seed + 1).integers(0, V, V // 8)] = -np.inf
    return x


def _histories(V, n, seed):
    """Histories of length n - 1, n, n + 1, longer ones over a small alphabet (so n-grams do repeat), and an all-equal one"""
    g = np.random.default_rng(seed)
    small = lambda L: g.integers(0, 2, L).tolist()
    return [small(L) for L in (n - 1, n, n + 1, 40, 97)] + [[V - 1] * (n + 5)]


@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_ngram_ban_equals_transformers(n):
    tr = pytest.importorskip("transformers")
    proc = tr.NoRepeatNGramLogitsProcessor(n)
    hits = 0
    for V, seed in ((7, 1), (1000, 2)):
        x = _row(V, seed)
        for hist in _histories(V, n, seed + n):
            want = proc(torch.tensor([hist], dtype=torch.long), torch.from_numpy(x.copy())[None])[0].numpy()
            got = E.edit_row(x, None, n, hist[:len(hist) // 2], hist[len(hist) // 2:])      # (the split point does not matter)
            assert np.array_equal(E.bits(got), E.bits(want)), (V, n, hist)
            hits += int(not np.array_equal(E.bits(got), E.bits(x)))
            if len(hist) < n:
                assert np.array_equal(E.bits(got), E.bits(x))
    assert hits >= 2      # the cases do ban something (at least once per vocabulary size)
    # by hand: after ... 5 6 | 5 the bigram rule bans 6; the trigram rule needs "6 5" to have occurred
    assert E.banned_ngram_ids([5, 6, 5], 2) == {6} and E.banned_ngram_ids([5, 6, 5], 3) == set()
    assert E.banned_ngram_ids([1, 2, 3, 1, 2], 3) == {3} and E.banned_ngram_ids([4, 4, 4, 4], 3) == {4}
    assert E.banned_ngram_ids([9, 8, 9], 1) == {8, 9} and E.banned_ngram_ids([], 1) == set() and E.banned_ngram_ids([1, 2], 0) == set()
    assert E.edit_row(np.zeros(4, np.float32), None, 1, [1], [12], id_offset=10).tolist() == [0.0, -INF, -INF, 0.0]


def test_bias_equals_transformers_sequence_bias():
    tr = pytest.importorskip("transformers")
    for V, seed in ((7, 3), (1000, 4)):
        x = _row(V, seed)
        x[1] = -np.inf
        g = np.random.default_rng(seed)
        ids = sorted({0, 1, V - 1} | set(g.integers(0, V, 5).tolist()))
        bias = {i: float(np.float32(g.uniform(-100, 100))) for i in ids}
        proc = tr.SequenceBiasLogitsProcessor(sequence_bias={(i,): v for i, v in bias.items()})
        want = proc(torch.zeros(1, 3, dtype=torch.long), torch.from_numpy(x.copy())[None])[0].numpy()
        got = E.bias_row(x, bias)
        assert np.array_equal(E.bits(got), E.bits(want)) and np.isneginf(got[1]) and not np.array_equal(E.bits(got), E.bits(x))
    y = E.bias_row(np.array([NAN, -INF, 1.0], dtype=np.float32), {0: 5.0, 1: 100.0, 2: -0.5, 7: 1.0})
    assert np.isnan(y[0]) and np.isneginf(y[1]) and y[2] == 0.5
    # bias, then ban: a biased id that is also banned ends at -inf
    assert np.isneginf(E.edit_row(np.zeros(3, np.float32), {2: 100.0}, 1, [2], [])[2])


@pytest.mark.parametrize("T", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("min_p", [0.05, 0.3, 1.0])
def test_min_p_kept_set_equals_transformers(T, min_p):
    tr = pytest.importorskip("transformers")
    for V, seed in ((1000, 5), (42003, 6)):
        x = _row(V, seed)
        assert E.min_p_band_empty(x, T, min_p)
        scores = torch.from_numpy(x)[None] / T
        want = tr.MinPLogitsWarper(min_p=min_p)(None, scores.clone())[0].numpy()
        keep = E.min_p_keep(x, T, min_p)
        assert np.array_equal(keep, ~np.isneginf(want)) and keep.any() and (min_p < 1.0 or np.array_equal(keep, x == x.max()))
        assert keep.sum() < (~np.isneginf(x)).sum()
    assert E.min_p_keep(x, T, 0.0).sum() == (~np.isneginf(x)).sum()


def test_struct_sizes_match_the_library():
    from usdm_amd import _lib, ops
    lib = _lib.lib
    assert lib.usdm_sizeof_logit_edit_args() == ctypes.sizeof(_lib.LogitEditArgs)
    assert lib.usdm_sizeof_logit_edit_params() == ctypes.sizeof(_lib.LogitEditParams) == 16
    assert lib.usdm_sizeof_sample_args() == ctypes.sizeof(_lib.SampleArgs) and ctypes.sizeof(_lib.SampleParams) == 24
    assert _lib.SampleParams.min_p.offset == 12 and _lib.SampleParams.seed.offset == 16 and ops.LOGIT_BIAS_MAX == 1024
    t = torch.zeros(24, dtype=torch.uint8)
    ops.set_sample_params(t, 0.5, 7, 0.25, 9)                     # positional, as before: min_p stays zero bits
    assert t[12:16].tolist() == [0, 0, 0, 0]
    ops.set_sample_params(t, 0.5, 7, 0.25, 9, min_p=0.125)
    assert np.frombuffer(t.numpy().tobytes(), dtype=np.float32)[3] == 0.125
    blk = torch.zeros(16, dtype=torch.uint8)
    ops.set_edit_params(blk, 3, 40, 2)
    assert np.frombuffer(blk.numpy().tobytes(), dtype=np.int32).tolist() == [3, 40, 2, 0]
    with pytest.raises(ValueError, match="n_bias"):
        ops.set_edit_params(blk, 0, 0, 1025)


BAD = [dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=NAN), dict(min_p="x"), dict(min_p=None),
       dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.5), dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size="3"),
       dict(logit_bias=[(1, 2.0)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={"7": 1.0}),
       dict(logit_bias={3: NAN}), dict(logit_bias={3: INF}), dict(logit_bias={3: None}), dict(logit_bias={3: "a"}),
       dict(logit_bias={i: 1.0 for i in range(1025)})]


@pytest.mark.parametrize("kw", BAD, ids=[f"{next(iter(k))}-{i}" for i, k in enumerate(BAD)])
def test_public_surface_rejects_out_of_range_knobs(kw):
    from usdm_amd.llm import check_edits, check_min_p
    from usdm_amd.serving import SamplingParams
    knob = next(iter(kw))
    with pytest.raises(ValueError, match=knob):
        SamplingParams(**kw)
    with pytest.raises(ValueError, match=knob):
        check_min_p(kw["min_p"]) if knob == "min_p" else check_edits(kw.get("logit_bias"), kw.get("no_repeat_ngram_size", 0))


def test_known_good_knobs_are_stored_and_clamped():
    from usdm_amd.inference import parse_logit_bias
    from usdm_amd.llm import check_edits, check_min_p
    from usdm_amd.serving import SamplingParams
    assert check_edits(None, 0) is None and check_edits({}, None) is None and check_edits() is None
    assert check_edits({9: 250, 3: -1e9, 4: 0.5}, 0) == (((3, -100.0), (4, 0.5), (9, 100.0)), 0)      # vLLM's / OpenAI's range
    assert check_edits(None, 3) == ((), 3) and check_edits({0: 1}, 2, vocab=1) == (((0, 1.0),), 2)
    with pytest.raises(ValueError, match="logit_bias"):
        check_edits({1000: 1.0}, 0, vocab=1000)
    assert check_edits({i: 1.0 for i in range(1024)}, 0)[0][-1] == (1023, 1.0)
    assert check_min_p(0) == 0.0 and check_min_p(1) == 1.0 and check_min_p(0.05) == 0.05
    sp = SamplingParams(min_p=0.1, logit_bias={5: -200.0}, no_repeat_ngram_size=4)
    assert sp.min_p == 0.1 and sp.edits == (((5, -100.0),), 4) and sp.logit_bias == {5: -200.0} and sp.no_repeat_ngram_size == 4
    assert SamplingParams().edits is None and SamplingParams().min_p == 0.0 and SamplingParams(no_repeat_ngram_size=None).edits is None
    with pytest.raises(NotImplementedError):
        SamplingParams(prompt_logprobs=1, min_p=0.1)
    assert parse_logit_bias(None) is None and parse_logit_bias('{"17": -100, "3": 2.5}') == {17: -100, 3: 2.5}
    for bad in ("[1, 2]", "{", '{"a": 1}'):
        with pytest.raises(ValueError, match="logit_bias"):
            parse_logit_bias(bad)


def test_step_kind_with_edits_is_a_key_of_its_own():
    from usdm_amd.llm import StepKind, step_kind
    assert step_kind() == StepKind(False, None, False) == (False, None, False, False)
    assert step_kind(edits=True) == StepKind(True, None, False, True) and step_kind(edits=True).sampling is True
    assert step_kind(True, 5, True) == (True, 5, True, False) and step_kind("hook", edits=1) == ("hook", None, False, True)
    assert len({step_kind(), step_kind(True), step_kind(edits=True), step_kind(penalties=True), step_kind(penalties=True, edits=True)}) == 5
    assert StepKind._fields == ("sampling", "logprobs", "penalties", "edits")


def test_library_refuses_bad_arguments_without_a_launch():
    """The bad-argument style of tests/test_abi_cpu.py: an error code and a message naming the entry point, nothing launched."""
    from usdm_amd import _lib
    lib, ok = _lib.lib, 0x1000                                   # `ok`: an aligned non-null address that is never dereferenced

    def args(**kw):
        a = _lib.LogitEditArgs(logits=ok, V=1000, logits_bs=1000, dev_params=ok, bias_id=ok, bias_val=ok, bias_max=1024, bias_bs=1024,
                               prompt=ok, prompt_max=256, prompt_bs=256)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def state(**kw):
        st = _lib.DecodeState(next_token=ok, out_tokens=ok, step=ok, pos=ok, max_out=8, batch=0)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def refused(a, st, word, seg=None):
        if seg is None:
            rc = lib.usdm_logit_edit(ctypes.byref(a), ctypes.byref(st), ctypes.c_void_p(0))
        else:
            rc = lib.usdm_logit_edit_seg(ctypes.byref(a), ctypes.c_int32(seg[0]), ctypes.c_int64(seg[1]), ctypes.c_int32(seg[2]),
                                         ctypes.byref(st), ctypes.c_void_p(0))
        msg = lib.usdm_last_error()
        name = b"usdm_logit_edit_seg:" if seg is not None else b"usdm_logit_edit:"
        assert rc == 2 and name in msg and word in msg, (rc, msg)

    for V in (0, -1, (1 << 20) + 1):
        refused(args(V=V), state(), b"V")
    refused(args(logits=None), state(), b"logits")
    refused(args(dev_params=None), state(), b"dev_params")
    refused(args(bias_id=None), state(), b"bias_id")
    refused(args(bias_val=None), state(), b"bias_val")
    refused(args(bias_max=1025), state(), b"bias_max")
    refused(args(bias_max=-1), state(), b"bias_max")
    refused(args(prompt=None), state(), b"prompt")
    refused(args(prompt_max=-1), state(), b"prompt_max")
    refused(args(logits=ok + 2), state(), b"aligned")
    refused(args(bias_id=ok + 1), state(), b"aligned")
    refused(args(bias_val=ok + 2), state(), b"aligned")
    refused(args(prompt=ok + 3), state(), b"aligned")
    refused(args(dev_params=ok + 8), state(), b"aligned")
    refused(args(), state(out_tokens=None), b"decode state")
    refused(args(), state(max_out=0), b"decode state")
    refused(args(logits_bs=0), state(batch=4), b"batched")       # the batched form without strides
    refused(args(bias_bs=1023), state(batch=4), b"batched")
    refused(args(prompt_bs=0), state(batch=4), b"batched")
    # the segmented entry point: its own name in every message
    refused(args(V=0), state(), b"V", seg=(2, 512, 512))
    refused(args(), state(), b"cover", seg=(2, 400, 400))        # 2 x 400 ids do not cover V = 1000
    refused(args(), state(), b"cover", seg=(0, 512, 512))
    refused(args(logits_bs=512), state(batch=4), b"overlap", seg=(2, 1024, 512))
    refused(args(logits_bs=511), state(batch=4), b"batched", seg=(2, 4096, 512))
    refused(args(prompt_bs=255, logits_bs=512), state(batch=4), b"batched", seg=(2, 4096, 512))
    # min_p of the non-dev_params form of the sampler
    sa = _lib.SampleArgs(logits=ok, V=1000, temperature=1.0, top_k=0, top_p=1.0, min_p=1.5)
    assert lib.usdm_sample_final(ctypes.byref(sa), ctypes.byref(state()), None, 0, None, ctypes.c_void_p(0)) == 2
    assert b"usdm_sample_final: min_p" in lib.usdm_last_error()
    sa.min_p = NAN
    assert lib.usdm_sample_final_seg(ctypes.byref(sa), 2, ctypes.c_int64(512), 512, ctypes.byref(state()), None, 0, None, ctypes.c_void_p(0)) == 2
    assert b"usdm_sample_final_seg: min_p" in lib.usdm_last_error()
    with pytest.raises(_lib.UsdmError):                          # and no CPU fallback
        from usdm_amd import ops
        ops.logit_edit(torch.zeros(8), state(), dev_params=torch.zeros(16, dtype=torch.uint8))


def test_wrapper_checks_its_tensors(monkeypatch):
    from usdm_amd import _lib, ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)      # reach the shape checks on the CPU
    st = _lib.DecodeState(next_token=0x1000, out_tokens=0x1000, step=0x1000, pos=0x1000, max_out=8, batch=0)
    row, blk = torch.zeros(8), torch.zeros(16, dtype=torch.uint8)
    i32, f32 = torch.zeros(4, dtype=torch.int32), torch.zeros(4)
    with pytest.raises(ValueError, match="float32"):
        ops.logit_edit(row.double(), st, dev_params=blk)
    with pytest.raises(ValueError, match="dev_params"):
        ops.logit_edit(row, st, dev_params=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="go together"):
        ops.logit_edit(row, st, dev_params=blk, bias_id=i32)
    with pytest.raises(ValueError, match="bias_id"):
        ops.logit_edit(row, st, dev_params=blk, bias_id=f32, bias_val=f32)
    with pytest.raises(ValueError, match="same shape"):
        ops.logit_edit(row, st, dev_params=blk, bias_id=i32, bias_val=torch.zeros(5))
    with pytest.raises(ValueError, match="at most 1024"):
        ops.logit_edit(row, st, dev_params=blk, bias_id=torch.zeros(1025, dtype=torch.int32), bias_val=torch.zeros(1025))
    with pytest.raises(ValueError, match="prompt"):
        ops.logit_edit(row, st, dev_params=blk, prompt=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="logit_edit") as e:      # the row checks the pick wrappers share
        ops.logit_edit(torch.zeros(1, 2, 8), st, dev_params=blk)
    assert "seg_len" in str(e.value)
