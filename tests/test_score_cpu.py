"""Host side of scoring given tokens (USDMForCausalLM.score / serving.LLM.score): the ctypes struct of usdm_prompt_logprobs, the
argument checks that need no device, the pure assembly of a ScoreOutput, and the refusal SamplingParams(prompt_logprobs=) keeps
(no GPU)."""
import ctypes as C
import math

import pytest
import torch

OK = 0x1000      # an aligned non-null address that is never dereferenced


def test_prompt_logprob_args_struct_size():
    from usdm_amd import _lib
    assert C.sizeof(_lib.PromptLogprobArgs) == _lib.lib.usdm_sizeof_prompt_logprob_args()
    names = [f[0] for f in _lib.PromptLogprobArgs._fields_]
    assert names == ["logits", "V", "K", "logits_bs", "ids", "n_ids", "row0", "rows", "tok_lp", "tok_rank", "top_id", "top_lp"]


def _args(**kw):
    from usdm_amd import _lib
    base = dict(logits=OK, V=100, K=5, logits_bs=100, ids=OK, n_ids=9, row0=2, rows=5, tok_lp=OK, tok_rank=OK, top_id=OK, top_lp=OK)
    return _lib.PromptLogprobArgs(**dict(base, **kw))


@pytest.mark.parametrize("kw,msg", [(dict(K=21), b"K must be 0 .. 20"), (dict(K=-1), b"K must be 0 .. 20"), (dict(V=0), b"logits / V"),
                                    (dict(V=(1 << 20) + 1), b"logits / V"), (dict(logits=None), b"logits / V"), (dict(ids=None), b"ids"),
                                    (dict(tok_lp=None), b"tok_lp"), (dict(top_lp=None), b"top_id / top_lp"), (dict(rows=0), b"rows"),
                                    (dict(row0=-1), b"row0"), (dict(row0=4), b"n_ids"), (dict(rows=7), b"n_ids")])
def test_entry_points_refuse_bad_arguments_without_a_launch(kw, msg):
    """(no device here: a call that got as far as a launch would fail with another error than rc = 2)"""
    from usdm_amd import _lib
    a = _args(**kw)
    rc = _lib.lib.usdm_prompt_logprobs(C.byref(a), None)
    assert rc == 2 and b"usdm_prompt_logprobs" in _lib.lib.usdm_last_error() and msg in _lib.lib.usdm_last_error(), _lib.lib.usdm_last_error()
    rc = _lib.lib.usdm_prompt_logprobs_seg(C.byref(a), C.c_int32(2), C.c_int64(1000), C.c_int32(50), None)
    assert rc == 2 and b"usdm_prompt_logprobs_seg" in _lib.lib.usdm_last_error() and msg in _lib.lib.usdm_last_error()


def test_row_stride_and_segments_are_checked():
    from usdm_amd import _lib
    lib = _lib.lib
    assert lib.usdm_prompt_logprobs(C.byref(_args(logits_bs=99)), None) == 2 and b"logits_bs" in lib.usdm_last_error()
    seg = lambda a, nseg, stride, slen: lib.usdm_prompt_logprobs_seg(C.byref(a), C.c_int32(nseg), C.c_int64(stride), C.c_int32(slen), None)
    assert seg(_args(logits_bs=50), 2, 1000, 40) == 2 and b"cover V" in lib.usdm_last_error()            # 2 x 40 ids < V
    assert seg(_args(logits_bs=50), 2, 249, 50) == 2 and b"overlap" in lib.usdm_last_error()              # 5 rows of a segment need 250
    assert seg(_args(logits_bs=40), 2, 1000, 50) == 2 and b"logits_bs" in lib.usdm_last_error()           # rows of a segment overlap


def test_ops_wrapper_checks_shapes(monkeypatch):
    from usdm_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)      # reach the shape checks on the CPU
    ids = torch.zeros(9, dtype=torch.int64)
    out = dict(tok_lp=torch.zeros(9), tok_rank=torch.zeros(9, dtype=torch.int32), top_id=torch.zeros(45, dtype=torch.int32), top_lp=torch.zeros(45))
    with pytest.raises(ValueError, match="float32"):
        ops.prompt_logprobs(torch.zeros(5, 100, dtype=torch.bfloat16), ids, row0=2, K=5, **out)
    with pytest.raises(ValueError, match="int64"):
        ops.prompt_logprobs(torch.zeros(5, 100), ids.int(), row0=2, K=5, **out)
    with pytest.raises(ValueError, match="more rows"):
        ops.prompt_logprobs(torch.zeros(5, 100), ids, row0=2, rows=6, K=5, **out)
    with pytest.raises(ValueError, match="top_id"):       # [n_ids][K] does not fit
        ops.prompt_logprobs(torch.zeros(5, 100), ids, row0=2, K=6, **out)
    with pytest.raises(ValueError, match="seg_len"):
        ops.prompt_logprobs(torch.zeros(2, 5, 100), ids, row0=2, K=5, **out)
    with pytest.raises(ValueError, match="segmented"):
        ops.prompt_logprobs(torch.zeros(2, 5, 50), ids, row0=2, K=5, nseg=2, seg_stride=100, seg_len=50, **out)      # seg_stride is 250


def _bare_model(ctx_max=64):
    """score() validates before it touches the device: an object without weights or buffers is enough to see that"""
    from usdm_amd.llm import USDMForCausalLM
    m = USDMForCausalLM.__new__(USDMForCausalLM)
    m.ctx_max = ctx_max
    return m


def test_score_validates_its_arguments_before_touching_the_device():
    m = _bare_model()
    ids = torch.arange(10)[None]
    for bad in (ids[0], torch.arange(20).view(2, 10), None):
        with pytest.raises(ValueError, match=r"\[1, L\]"):
            m.score(bad)
    with pytest.raises(ValueError, match="ctx_max"):
        m.score(ids[:, :1])
    with pytest.raises(ValueError, match="ctx_max"):
        m.score(torch.zeros(1, 65, dtype=torch.long))
    for bad in (0, 10, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="start"):
            m.score(ids, start=bad)
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError, match="logprobs"):
            m.score(ids, top_logprobs=bad)


def test_score_rows_must_be_a_positive_multiple_of_16():
    from usdm_amd.llm import USDMForCausalLM
    for bad in (0, 8, 24, -16, 16.0, True):
        with pytest.raises(ValueError, match="score_rows"):
            USDMForCausalLM(dict(head_dim=128), "cpu", score_rows=bad)
    with pytest.raises(RuntimeError, match="MI355X"):      # a good value gets as far as the device check
        USDMForCausalLM(dict(head_dim=128), "cpu", score_rows=32)


class _Tok:
    def decode(self, ids):
        return "".join(f"<{i}>" for i in ids)


class _Rows:
    def __init__(self, token_logprobs, ranks, top_ids, top_logprobs):
        self.token_logprobs, self.ranks, self.top_ids, self.top_logprobs = token_logprobs, ranks, top_ids, top_logprobs


def test_score_output_assembly():
    from usdm_amd.serving import Logprob, ScoreOutput, assemble_score
    ids, start = [11, 12, 7, 3, 9], 2                       # tokens 7, 3, 9 are scored
    rows = _Rows([-0.5, -2.0, -4.0], [1, 2, 4], [[7, 2, 5], [8, 3, 1], [4, 5, 6]], [[-0.5, -1.5, -2.5], [-1.0, -2.0, -3.0], [-1.0, -1.5, -2.0]])
    o = assemble_score(ids, start, rows, 3, _Tok(), prompt="p")
    assert isinstance(o, ScoreOutput) and o.prompt == "p" and o.prompt_token_ids == ids
    assert len(o.prompt_logprobs) == len(ids) and o.prompt_logprobs[:2] == [None, None]
    assert [len(d) for d in o.prompt_logprobs[2:]] == [3, 3, 4]          # the token inside the top K: K entries; outside: K + 1
    assert o.prompt_logprobs[2][7] == Logprob(-0.5, 1, "<7>") and o.prompt_logprobs[3][3] == Logprob(-2.0, 2, "<3>")
    assert o.prompt_logprobs[4][9] == Logprob(-4.0, 4, "<9>") and [o.prompt_logprobs[4][i].rank for i in (4, 5, 6)] == [1, 2, 3]
    assert o.cumulative_logprob == -6.5
    o0 = assemble_score(ids, start, rows, 0)                 # K = 0: the given token only
    assert [list(d) for d in o0.prompt_logprobs[2:]] == [[7], [3], [9]] and o0.prompt_logprobs[2][7].decoded_token is None
    # the cumulative value is a float64 sum of the f32 values; tensors are taken as well as lists
    vals = [-(2.0 ** -20) * (i + 1) for i in range(50)]
    t = _Rows(torch.tensor(vals), torch.ones(50, dtype=torch.int32), torch.zeros(50, 0, dtype=torch.int32), torch.zeros(50, 0))
    o = assemble_score(list(range(51)), 1, t, 0)
    assert o.cumulative_logprob == sum(vals) and o.prompt_logprobs[0] is None and len(o.prompt_logprobs) == 51
    assert math.isfinite(o.cumulative_logprob)


def test_llm_score_checks_its_list_arguments():
    from usdm_amd.serving import LLM
    eng = LLM.__new__(LLM)
    eng.tokenizer = None
    with pytest.raises(ValueError, match="required"):
        eng.score()
    with pytest.raises(ValueError, match="start"):
        eng.score(prompt_token_ids=[[1, 2, 3], [4, 5, 6]], start=[1])
    with pytest.raises(ValueError, match="logprobs"):
        eng.score(prompt_token_ids=[[1, 2, 3]], top_logprobs=21)
    with pytest.raises(ValueError, match="tokenizer"):
        eng.score(prompts=["hello"])


def test_sampling_params_prompt_logprobs_still_refused_and_points_to_score():
    from usdm_amd.serving import SamplingParams
    with pytest.raises(NotImplementedError, match="prompt_logprobs") as e:
        SamplingParams(prompt_logprobs=1)
    assert "LLM.score()" in str(e.value) and "USDMForCausalLM.score()" in str(e.value)
    assert SamplingParams(prompt_logprobs=None).logprobs is None
