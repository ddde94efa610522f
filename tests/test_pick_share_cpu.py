"""CPU: what the three pick kernels (usdm_sample_final, usdm_logprobs, usdm_penalize) share on the host.
  * the segment checks of csrc/logits_row.h behind all three *_seg entry points: refused with the entry point's own name, no launch;
  * the row-shape checks of ops._logits_row behind ops.sample_final / ops.logprobs / ops.penalize;
  * llm.step_kind, the key of every cache of built plans."""
import ctypes

import pytest
import torch

OK = 0x1000      # an aligned non-null address that is never dereferenced


def _seg_call(name, V, nseg, seg_stride, seg_len):
    from usdm_amd import _lib
    lib = _lib.lib
    st = _lib.DecodeState(next_token=OK, out_tokens=OK, step=OK, pos=OK, max_out=4, batch=0)
    seg = (ctypes.c_int32(nseg), ctypes.c_int64(seg_stride), ctypes.c_int32(seg_len), ctypes.byref(st))
    if name == "usdm_sample_final_seg":
        a = _lib.SampleArgs(logits=OK, V=V, temperature=1.0, top_k=0, top_p=1.0)
        rc = lib.usdm_sample_final_seg(ctypes.byref(a), *seg, None, ctypes.c_int32(0), None, None)
    elif name == "usdm_logprobs_seg":
        a = _lib.LogprobArgs(logits=OK, V=V, K=0, tok_lp=OK, tok_rank=OK)
        rc = lib.usdm_logprobs_seg(ctypes.byref(a), *seg, None)
    else:
        a = _lib.PenaltyArgs(logits=OK, V=V, table=OK, dev_params=OK)
        rc = lib.usdm_penalize_seg(ctypes.byref(a), *seg, None)
    return rc, lib.usdm_last_error()


@pytest.mark.parametrize("name", ["usdm_sample_final_seg", "usdm_logprobs_seg", "usdm_penalize_seg"])
def test_seg_entry_points_refuse_bad_segments(name):
    rc, msg = _seg_call(name, 1000, 2, 600, 400)          # 2 x 400 ids
    assert rc == 2 and name.encode() in msg and b"cover V" in msg, (rc, msg)
    rc, msg = _seg_call(name, 1000, 2, 100, 500)          # the second segment begins inside the first
    assert rc == 2 and name.encode() in msg and b"overlap" in msg, (rc, msg)
    rc, msg = _seg_call(name, 4, 4, 1, 1)                 # seg_len 1 is outside the kernels' index arithmetic
    assert rc == 2 and name.encode() in msg, (rc, msg)


def _wrapper_call(name, logits, st, **seg):
    from usdm_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    if name == "sample_final":
        return ops.sample_final(logits, st, **seg)
    if name == "logprobs":
        return ops.logprobs(logits, st, K=0, tok_lp=torch.zeros(2, 4), tok_rank=i32(8).view(2, 4), **seg)
    return ops.penalize(logits, st, table=i32(16).view(2, 8), dev_params=torch.zeros(2, 16, dtype=torch.uint8), **seg)


@pytest.mark.parametrize("name", ["sample_final", "logprobs", "penalize"])
def test_wrappers_refuse_rows_the_kernels_would_misread(monkeypatch, name):
    from usdm_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)      # reach the shape checks on the CPU
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    st = ops.decode_state(i32(2), i32(2, 4), i32(2), i32(2), batch=2)
    with pytest.raises(ValueError, match="seg_len") as e:          # [nseg][B][seg_len] on the contiguous form: a wrong row stride
        _wrapper_call(name, torch.zeros(1, 2, 8), st)
    assert name in str(e.value)
    for bad in (torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float32") as e:
            _wrapper_call(name, bad, st)
        assert name in str(e.value)
    with pytest.raises(ValueError, match="float32") as e:          # ... with unit inner stride
        _wrapper_call(name, torch.zeros(2, 16)[:, ::2], st)
    with pytest.raises(ValueError, match=name):                    # the last dimension of a segmented tensor is seg_len
        _wrapper_call(name, torch.zeros(2, 2, 8), st, nseg=2, seg_stride=16, seg_len=4)
    with pytest.raises(ValueError, match=name):                    # ... and nseg segments of B rows fit into it
        _wrapper_call(name, torch.zeros(2, 2, 8), st, nseg=3, seg_stride=16, seg_len=8)


def test_step_kind():
    from usdm_amd.llm import StepKind, step_kind
    assert step_kind() == step_kind(None) == step_kind(False) == StepKind(False, None, False)
    assert step_kind(True) == StepKind(True, None, False) and step_kind(1).sampling is True
    assert step_kind(False, logprobs=0).sampling is True and step_kind(None, penalties=True).sampling is True
    assert step_kind(False, logprobs=0) == step_kind(True, logprobs=0)
    assert step_kind("hook", logprobs=3).sampling == "hook" and step_kind("hook", penalties=True) == StepKind("hook", None, True)
    assert step_kind(True, None, 1).penalties is True
    # greedy, sampled, hooked, with K = 0 / 5 / 20 rows, penalised with K = None / 0 / 5: each is a key of its own (a plan of its own)
    old = [(False,), (True,), ("hook",)] + [(True, K) for K in (0, 5, 20)] + [(True, K, "penalties") for K in (None, 0, 5)]
    kinds = [step_kind(k[0], k[1] if len(k) > 1 else None, len(k) > 2) for k in old]
    assert len(set(kinds)) == len(old) == 9
    assert len({k: None for k in kinds}) == 9 and all(k[0] == o[0] for k, o in zip(kinds, old))      # sampling keeps its position
