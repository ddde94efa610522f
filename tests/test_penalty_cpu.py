"""CPU: the semantics of the repetition / frequency / presence penalties (tests/_penalty_reference.py, the numpy float32 restatement
the GPU tests compare usdm_penalize with bit for bit), the range checks of the public surface, and the library's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _penalty_reference as P

NAN = float("nan")


@pytest.mark.parametrize("r", [1.3, 0.7, 2.0])
def test_repetition_only_equals_transformers_bit_for_bit(r):
    tr = pytest.importorskip("transformers")
    if not hasattr(tr, "RepetitionPenaltyLogitsProcessor"):
        pytest.skip("transformers has no RepetitionPenaltyLogitsProcessor")
    proc = tr.RepetitionPenaltyLogitsProcessor(penalty=r)
    for V, seed in ((1000, 1), (32003, 2)):
        x = P.bf16_row(V, seed)
        prompt, out = P.history(V, seed + 10)
        hist = torch.from_numpy(np.concatenate([prompt, out]))[None]
        want = proc(hist, torch.from_numpy(x.copy())[None])[0].numpy()
        got = P.penalize_row(x, prompt, out, r, 0.0, 0.0)
        assert np.isneginf(x).sum() > V // 8 and np.array_equal(P.bits(got), P.bits(want))
        assert not np.array_equal(P.bits(got), P.bits(x))


def test_frequency_and_presence_on_hand_made_cases():
    f32 = np.float32
    #            0: prompt only  1: generated 3x  2: x = 0, generated 1x  3: -inf, generated 2x  4: unseen  5: prompt + generated, x < 0
    x = np.array([2.0, 4.0, 0.0, -np.inf, -1.5, -3.0], dtype=f32)
    prompt, out = [0, 5], [1, 1, 1, 2, 3, 3, 5]
    r, f, p = 1.5, 0.25, -0.5
    y = P.penalize_row(x, prompt, out, r, f, p)
    rr, ff, pp = f32(r), f32(f), f32(p)
    want = np.array([
        f32(2.0) / rr,                                          # repetition yes, frequency / presence no
        (f32(4.0) / rr - ff * f32(3)) - pp * f32(1),            # the two subtractions, in that order
        (f32(0.0) / rr - ff * f32(1)) - pp * f32(1),            # 0 is not < 0: divided, stays 0
        -np.inf,                                                 # banned stays banned
        -1.5,                                                    # never seen: untouched
        (f32(-3.0) * rr - ff * f32(1)) - pp * f32(1),           # negative: multiplied
    ], dtype=f32)
    assert np.array_equal(P.bits(y), P.bits(want))
    assert y[0] == f32(2.0) / rr and y[2] == f32(0.25) and y[4] == x[4]
    # frequency alone counts occurrences, presence alone counts ids; neither looks at the prompt
    yf = P.penalize_row(x, prompt, out, 1.0, 1.0, 0.0)
    assert yf.tolist()[:3] == [2.0, 1.0, -1.0] and yf[5] == -4.0
    yp = P.penalize_row(x, prompt, out, 1.0, 0.0, 2.0)
    assert yp.tolist()[:3] == [2.0, 2.0, -2.0] and yp[5] == -5.0 and np.isneginf(yp[3])
    # NaN stays NaN
    assert np.isnan(P.penalize_row(np.array([NAN, 1.0], dtype=f32), [0], [0], 1.2, 0.1, 0.1)[0])


def test_neutral_knobs_return_the_input_bits():
    x = P.bf16_row(1000, 3)
    x[7] = -0.0
    prompt, out = P.history(1000, 4)
    assert np.array_equal(P.bits(P.penalize_row(x, prompt, out, 1.0, 0.0, 0.0)), P.bits(x))
    t = P.table(1000, prompt, out)
    assert int((t & (P.PROMPT_BIT - 1)).sum()) == len(out) and int((t >= P.PROMPT_BIT).sum()) == len(set(prompt.tolist()))


BAD_KNOBS = [dict(repetition_penalty=0), dict(repetition_penalty=2.5), dict(presence_penalty=3), dict(repetition_penalty=NAN),
             dict(presence_penalty=NAN), dict(frequency_penalty=NAN), dict(frequency_penalty=-2.5), dict(repetition_penalty=-1)]


@pytest.mark.parametrize("kw", BAD_KNOBS)
def test_public_surface_rejects_out_of_range_knobs(kw):
    from usdm_amd.llm import check_penalties          # generate()'s and generate_batch()'s argument check
    from usdm_amd.serving import SamplingParams
    with pytest.raises(ValueError, match="penalty"):
        check_penalties(**kw)
    with pytest.raises(ValueError, match="penalty"):
        SamplingParams(**kw)


def test_known_good_knobs_are_stored():
    from usdm_amd import ops
    from usdm_amd.llm import check_penalties
    from usdm_amd.serving import SamplingParams
    sp = SamplingParams(repetition_penalty=1.25, presence_penalty=-2.0, frequency_penalty=2.0)
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty) == (1.25, -2.0, 2.0)
    assert sp.penalties == (1.25, 2.0, -2.0)                      # usdm_penalty_params' order: repetition, frequency, presence
    assert SamplingParams().penalties is None and check_penalties() is None and check_penalties(1.0, 0.0, 0.0) is None
    assert check_penalties(2.0, 0.0, 0.0) == (2.0, 0.0, 0.0)      # the ends of the ranges are inside
    blk = ops.penalty_params(1.25, 2.0, -2.0)
    assert np.frombuffer(bytes(blk), dtype=np.float32)[:3].tolist() == [1.25, 2.0, -2.0] and len(bytes(blk)) == 16


def test_library_refuses_bad_arguments_without_a_launch():
    """The bad-argument style of tests/test_abi_cpu.py: an error code and a message, nothing launched (no GPU here)."""
    from usdm_amd import _lib
    lib, ok = _lib.lib, 0x1000                                   # `ok`: an aligned non-null address that is never dereferenced
    assert lib.usdm_sizeof_penalty_args() == ctypes.sizeof(_lib.PenaltyArgs) and lib.usdm_sizeof_penalty_params() == 16

    def args(**kw):
        a = _lib.PenaltyArgs(logits=ok, V=1000, logits_bs=1000, table=ok, table_bs=1000, dev_params=ok, count=ok)
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
            rc = lib.usdm_penalize(ctypes.byref(a), ctypes.byref(st), ctypes.c_void_p(0))
        else:
            rc = lib.usdm_penalize_seg(ctypes.byref(a), ctypes.c_int32(seg[0]), ctypes.c_int64(seg[1]), ctypes.c_int32(seg[2]),
                                       ctypes.byref(st), ctypes.c_void_p(0))
        msg = lib.usdm_last_error()
        assert rc == 2 and b"usdm_penalize" in msg and word in msg, (rc, msg)

    for V in (0, -1, (1 << 20) + 1):
        refused(args(V=V), state(), b"V")
    refused(args(logits=None), state(), b"logits")
    refused(args(table=None), state(), b"table")
    refused(args(dev_params=None), state(), b"dev_params")
    refused(args(logits=ok + 2), state(), b"aligned")
    refused(args(table=ok + 1), state(), b"aligned")
    refused(args(dev_params=ok + 8), state(), b"aligned")
    refused(args(count=ok + 2), state(), b"aligned")
    refused(args(count=None), state(done=ok), b"done")           # a device-side `done` word without the tokens-counted word
    refused(args(), state(out_tokens=None), b"decode state")
    refused(args(logits_bs=0), state(batch=4), b"batched")       # the batched form without strides
    refused(args(table_bs=0), state(batch=4), b"batched")
    refused(args(table_bs=999), state(batch=4), b"batched")
    refused(args(), state(), b"cover", seg=(2, 400, 400))        # 2 x 400 ids do not cover V = 1000
    refused(args(logits_bs=512), state(batch=4), b"overlap", seg=(2, 1024, 512))
    p = _lib.PenaltyParams()
    for r, f, q in ((0.0, 0.0, 0.0), (2.5, 0.0, 0.0), (1.0, 0.0, 3.0), (NAN, 0.0, 0.0), (1.0, NAN, 0.0), (1.0, 0.0, NAN)):
        rc = lib.usdm_penalty_params_init(ctypes.byref(p), ctypes.c_float(r), ctypes.c_float(f), ctypes.c_float(q))
        assert rc == 2 and b"penalty" in lib.usdm_last_error()
    assert lib.usdm_penalty_params_init(ctypes.byref(p), ctypes.c_float(2.0), ctypes.c_float(-2.0), ctypes.c_float(2.0)) == 0
    with pytest.raises(_lib.UsdmError):                          # and no CPU fallback
        from usdm_amd import ops
        ops.penalize(torch.zeros(8), state(), table=torch.zeros(8, dtype=torch.int32), dev_params=torch.zeros(16, dtype=torch.uint8))
