"""CPU: beam search as the project defines it (tests/_beam_reference.py) equals the installed transformers' generate(num_beams=B,
do_sample=False[, bad_words_ids, renormalize_logits=True]) on a tiny float32 MistralForCausalLM; the product's host replay
(usdm_amd.beam.BeamReplay), fed the step logs of the reference's beam_step on the same rows, returns the same sequences and scores;
and the argument checks of the public surface.

The model, the prompt and the EOS ids were picked on the CPU so that the sweep cannot pass vacuously (asserted in
test_preconditions_of_the_sweep): beams change parents, hypotheses finish before max_length, and an EOS shows up among the first B
candidates.  B = 1: transformers runs greedy search there, which is the reference's one-beam search that stops at its first finished
hypothesis (early_stopping=True); only the ids are compared, greedy search reports no sequences_scores and takes no
length_penalty / early_stopping to sweep."""
import functools

import numpy as np
import pytest
import torch

from tests import _beam_reference as R

V, PROMPT, MAX_NEW = 100, [3, 17, 42, 8, 23], 12
EOS_SETS = ([66], [66, 60])
BAD = [5, 6, 7, 17]          # 17: the most frequent token of the unconstrained search, so that the ban changes it
SWEEP = [(B, lp, es, n, len(EOS_SETS[e]), bad) for B in (1, 2, 4) for lp in (0.6, 1.0, 2.0) for es in (False, True, "never")
         for n in sorted({1, B}) for e in (0, 1) for bad in (False, True) if B > 1 or (lp == 1.0 and es is False)]


@functools.lru_cache(maxsize=None)
def model():
    tr = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tr.MistralConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=16, max_position_embeddings=128, initializer_range=0.2, pad_token_id=None,
                           bos_token_id=None, eos_token_id=None)
    return tr.MistralForCausalLM(cfg).eval().float()


def row_fn(bad):
    """The logits rows of the running beams, from a full forward pass over prompt + beam (no cache); banned ids -inf"""
    m = model()

    def rows(running):
        with torch.no_grad():
            lg = m(torch.tensor([PROMPT + r for r in running])).logits[:, -1].float().numpy().copy()
        if bad:
            lg[:, BAD] = -np.inf
        return lg
    return rows


@functools.lru_cache(maxsize=None)
def hf(B, lp, es, n, n_eos, bad):
    eos = EOS_SETS[n_eos - 1]
    kw = dict(num_beams=B, do_sample=False, max_new_tokens=MAX_NEW, eos_token_id=eos, pad_token_id=eos[0], num_return_sequences=n,
              return_dict_in_generate=True, output_scores=True)
    if B > 1:
        kw.update(length_penalty=lp, early_stopping=es)
    if bad:
        kw.update(bad_words_ids=[[b] for b in BAD], renormalize_logits=True)
    with torch.no_grad():
        out = model().generate(torch.tensor([PROMPT]), **kw)
    return out.sequences[:, len(PROMPT):].tolist(), (out.sequences_scores.numpy() if B > 1 else None)


@functools.lru_cache(maxsize=None)
def ref(B, lp, es, n, n_eos, bad):
    eos = EOS_SETS[n_eos - 1]
    return R.beam_search(row_fn(bad), B, MAX_NEW, eos, lp, True if B == 1 else es, n, pad=eos[0])


def same_sequences(a, b, pad):
    w = max(len(a[0]), len(b[0]))
    return [s + [pad] * (w - len(s)) for s in a] == [s + [pad] * (w - len(s)) for s in b]


@pytest.mark.parametrize("B,lp,es,n,n_eos,bad", SWEEP)
def test_reference_equals_transformers(B, lp, es, n, n_eos, bad):
    want, want_scores = hf(B, lp, es, n, n_eos, bad)
    got, got_scores, _ = ref(B, lp, es, n, n_eos, bad)
    assert same_sequences(got, want, EOS_SETS[n_eos - 1][0]), (got, want)
    if B > 1:
        assert np.abs(got_scores - want_scores).max() <= 1e-5, (got_scores, want_scores)


def test_preconditions_of_the_sweep():
    moved = early = eos_first = banned_differs = 0
    for B, lp, es, n, n_eos, bad in SWEEP:
        if B == 1:
            continue
        eos = EOS_SETS[n_eos - 1]
        seqs, _, trace = ref(B, lp, es, n, n_eos, bad)
        moved += any((st["parent"] != np.arange(B)).any() for st in trace[1:])
        early += any(0 < len([t for t in s if t not in eos]) < MAX_NEW - 1 and s[-1] in eos for s in seqs) and len(trace) <= MAX_NEW
        eos_first += any(any(int(t) in eos for t in st["cand_token"][:B]) for st in trace)
        if bad:
            banned_differs += ref(B, lp, es, n, n_eos, False)[0] != seqs
            assert not any(t in BAD for s in seqs for t in s)
    assert moved and early and eos_first and banned_differs, (moved, early, eos_first, banned_differs)


@pytest.mark.parametrize("B,lp,es,n,n_eos,bad", [c for c in SWEEP if c[0] > 1])
def test_host_replay_equals_reference(B, lp, es, n, n_eos, bad):
    """usdm_amd.beam.BeamReplay sees only what the device logs (scores, tokens, parents per step) and must stop where HF stops"""
    from usdm_amd.beam import BeamReplay
    eos = EOS_SETS[n_eos - 1]
    want, want_scores, trace = ref(B, lp, es, n, n_eos, bad)
    rp = BeamReplay(B, eos, MAX_NEW, lp, es)
    over = [rp.feed(st["cand_score"], st["cand_token"], st["cand_parent"]) for st in trace]
    assert over == [False] * (len(trace) - 1) + [True]
    for t, st in enumerate(trace[:-1]):
        assert rp.running_parents(t) == st["parent"].tolist()
    got, got_scores = rp.results(n)
    assert got == want and np.array_equal(got_scores, want_scores)
    hf_seqs, hf_scores = hf(B, lp, es, n, n_eos, bad)
    assert same_sequences(got, hf_seqs, eos[0]) and np.abs(got_scores - hf_scores).max() <= 1e-5
    with pytest.raises(RuntimeError):
        rp.feed(trace[-1]["cand_score"], trace[-1]["cand_token"], trace[-1]["cand_parent"])


def test_beam_step_total_order_on_exact_ties():
    """equal values are listed by flat index; -0.0 ties with +0.0; banned ids come last, in flat-index order"""
    rows = np.full((2, 8), -np.inf)
    rows[0, [1, 6]] = 0.0
    rows[1, [1, 6]] = 0.0
    st = R.beam_step(rows, np.array([0.0, -0.0]), 2, [6], 2)
    assert st["cand_parent"].tolist() == [0, 0, 1, 1] and st["cand_token"].tolist() == [1, 6, 1, 6]
    assert np.allclose(st["cand_score"], np.log(0.5)) and st["next_token"].tolist() == [1, 1] and st["parent"].tolist() == [0, 1]
    rows[:, 6] = -np.inf
    st = R.beam_step(rows, np.array([0.0, 0.0]), 2, [], 2)
    assert st["cand_token"].tolist() == [1, 1, 0, 2] and st["cand_parent"].tolist() == [0, 1, 0, 0]
    assert st["cand_score"][:2].tolist() == [0.0, 0.0] and np.isneginf(st["cand_score"][2:]).all()


def test_argument_checks():
    from usdm_amd import beam, ops
    assert ops.beam_candidates(16, 1) == 32 and ops.beam_candidates(4, 3) == 16 and ops.beam_candidates(2, 0) == 4
    for B, n_eos in ((16, 2), (11, 3), (17, 0), (0, 0), (4, 4), (True, 0)):      # KC > 32, or outside the kernel's ranges
        with pytest.raises(ValueError):
            ops.beam_candidates(B, n_eos)
    with pytest.raises(ValueError, match="vocabulary"):
        beam.check_beam_args(4, 1, n_eos=1, vocab=7)                              # V < KC
    for bad_n in (5, 0, -1, True, 1.0):
        with pytest.raises(ValueError, match="num_return_sequences"):
            beam.check_beam_args(4, bad_n)                                        # n > B and its kin
    for es in ("always", None, 1):
        with pytest.raises(ValueError, match="early_stopping"):
            beam.check_beam_args(4, 1, early_stopping=es)
    for lp in (float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match="length_penalty"):
            beam.check_beam_args(4, 1, length_penalty=lp)
    assert beam.check_beam_args(4, None, 2, "never", 1, 100) == (4, 1, 2.0, "never", 8)
    beam.check_beam_call()
    for kw in (dict(do_sample=True), dict(logprobs=0), dict(penalties=(1.2, 0.0, 0.0)), dict(edits=(((3, 1.0),), 0)), dict(min_p=0.1),
               dict(logits_hook=lambda: None), dict(min_new_tokens=2), dict(tensor_parallel=True)):
        with pytest.raises(NotImplementedError, match="num_beams > 1 with"):
            beam.check_beam_call(**kw)


def test_cli_num_beams_flag():
    """--num_beams: off by default, 2 .. 16 alone, an error next to any non-default generation flag (before the models load)"""
    import argparse
    from usdm_amd.inference import check_num_beams
    base = dict(num_beams=None, logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0,
                no_repeat_ngram_size=0, logit_bias=None)
    ns = lambda **kw: argparse.Namespace(**{**base, **kw})
    for n in (None, 1, 2, 16):
        check_num_beams(ns(num_beams=n))
    check_num_beams(ns(num_beams=1, min_p=0.1))      # (one beam is the plain call: its flags are its own business)
    for n in (0, 17, -2):
        with pytest.raises(ValueError):
            check_num_beams(ns(num_beams=n))
    for kw in (dict(logprobs=0), dict(repetition_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5), dict(min_p=0.05),
               dict(no_repeat_ngram_size=3), dict(logit_bias='{"5": 1}')):
        with pytest.raises(ValueError, match="--num_beams cannot be combined with --" + next(iter(kw))):
            check_num_beams(ns(num_beams=4, **kw))
