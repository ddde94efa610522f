"""Host side of the per-token log-probabilities: SamplingParams validation, the pure assembly of vLLM's CompletionOutput.logprobs from
the device's rows, and the ctypes struct of usdm_logprobs (no GPU)."""
import ctypes as C
import math

import pytest


def test_sampling_params_validate_logprobs():
    from usdm_amd.serving import SamplingParams
    assert SamplingParams().logprobs is None
    for k in (0, 1, 20):
        assert SamplingParams(logprobs=k).logprobs == k
    for bad in (-1, 21, 1.5, "3", True):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad)
    with pytest.raises(NotImplementedError, match="prompt_logprobs"):
        SamplingParams(prompt_logprobs=1)


class _Tok:
    def decode(self, ids):
        return "".join(f"<{i}>" for i in ids)


def test_assemble_logprobs():
    from usdm_amd.serving import Logprob, assemble_logprobs
    toks = [7, 3, 9]
    tok_lp, tok_rank = [-0.5, -2.0, -4.0], [1, 2, 4]
    top_id = [[7, 2, 5], [8, 3, 1], [4, 5, 6]]
    top_lp = [[-0.5, -1.5, -2.5], [-1.0, -2.0, -3.0], [-1.0, -1.5, -2.0]]
    lps, total = assemble_logprobs(toks, tok_lp, tok_rank, top_id, top_lp, 3, _Tok())
    assert [len(d) for d in lps] == [3, 3, 4]                     # the pick inside the top K: K entries; outside: K + 1
    assert list(lps[0]) == [7, 2, 5] and lps[0][7] == Logprob(-0.5, 1, "<7>") and lps[0][5] == Logprob(-2.5, 3, "<5>")
    assert lps[1][3] == Logprob(-2.0, 2, "<3>") and lps[1][8].rank == 1 and lps[1][1].rank == 3
    assert lps[2][9] == Logprob(-4.0, 4, "<9>") and [lps[2][i].rank for i in (4, 5, 6)] == [1, 2, 3]
    assert total == -6.5
    # a request's own K below the width of the rows: only its first K columns count; K = 0: the picked token only
    lps2, _ = assemble_logprobs(toks, tok_lp, tok_rank, top_id, top_lp, 1)
    assert [sorted(d) for d in lps2] == [[7], [3, 8], [4, 9]] and lps2[0][7].decoded_token is None
    lps0, total0 = assemble_logprobs(toks, tok_lp, tok_rank, top_id, top_lp, 0)
    assert [list(d) for d in lps0] == [[7], [3], [9]] and total0 == -6.5
    # padding ids of -1 (fewer ids than K) are dropped
    lpsp, _ = assemble_logprobs([1], [-0.25], [1], [[1, 0, -1, -1]], [[-0.25, -1.5, -math.inf, -math.inf]], 4)
    assert sorted(lpsp[0]) == [0, 1]
    # the cumulative sum is a float64 sum of the f32 values
    vals = [-(2.0 ** -20) * (i + 1) for i in range(50)]
    _, tot = assemble_logprobs(list(range(50)), vals, [1] * 50, [[]] * 50, [[]] * 50, 0)
    assert tot == sum(vals)
    # tensors are taken as well as lists
    import torch
    lpt, tt = assemble_logprobs(toks, torch.tensor(tok_lp), torch.tensor(tok_rank, dtype=torch.int32), torch.tensor(top_id, dtype=torch.int32),
                                torch.tensor(top_lp), 3, _Tok())
    assert lpt == lps and tt == total


def test_completion_output_defaults_stay_none():
    from usdm_amd.serving import CompletionOutput
    o = CompletionOutput(0, "", [1, 2], "length")
    assert o.logprobs is None and o.cumulative_logprob is None


def test_generate_refuses_bad_logprobs_values():
    from usdm_amd.llm import check_logprobs
    assert check_logprobs(None) is None and check_logprobs(0) == 0 and check_logprobs(20) == 20
    for bad in (-1, 21, 2.0, False):
        with pytest.raises(ValueError):
            check_logprobs(bad)


def test_logprob_args_struct_size():
    from usdm_amd import _lib
    assert C.sizeof(_lib.LogprobArgs) == _lib.lib.usdm_sizeof_logprob_args()
    names = [f[0] for f in _lib.LogprobArgs._fields_]
    assert names == ["logits", "V", "K", "logits_bs", "tok_lp", "tok_rank", "top_id", "top_lp", "tok_bs", "top_bs", "count"]
