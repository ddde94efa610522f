"""Beam search through the model (USDMForCausalLM.generate(num_beams=)) and the serving surface (LLM.beam_search) on the small
synthetic model of tests/test_penalty_model_gpu.py, ctx_max = 256.

Ground truth without a new oracle: an eager run records the [B][V] logits rows of every step (generate(_beam_keep_rows=True)); the
numpy search of tests/_beam_reference.py, replayed over those rows, must take the same decisions step by step and end with the same
hypotheses.  That the rows really belong to the hypotheses (the KV rows followed their beams) is checked twice: bit for bit on the
caches after every step, and independently by rescoring every returned sequence with score().

test_scores_are_those_of_score: the tolerance is measured, not assumed - four times the largest difference between
generate(logprobs=0).cumulative and the sum of score()'s token log-probabilities on greedy continuations of the same lengths, both
existing paths on this model (decode GEMVs against prefill GEMMs, bf16).  Measured on an MI355X: largest difference 1.596e-02, so
the tolerance is 6.385e-02; the four hypotheses were off by 0.8e-03 .. 1.6e-02."""
import numpy as np
import pytest
import torch

from tests import _beam_reference as R
from tests import _logprob_reference as LR
from tests.test_penalty_model_gpu import BAD, SMALL

pytestmark = pytest.mark.gpu

L0, MAX_NEW = 40, 12


def _model(dev, seed=5, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.random_init(SMALL, dev, seed=seed, ctx_max=256, **kw)


def _prompt(dev, n=L0, seed=1):
    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.fixture(scope="module")
def model(dev):
    return _model(dev)


def _eos_that_finishes_early(m, ids, B, **kw):
    """the best candidate of step 3 of the search without an EOS: as an EOS id it ends a hypothesis there at the latest"""
    m.generate(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=B, **kw)
    return m.last_beam_replay.tokens[3][0]


def _replay_recorded_rows(m, ids, B, **kw):
    eos = [_eos_that_finishes_early(m, ids, B, **kw)]
    call = dict(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=B, num_return_sequences=B, eos_token_id=eos, **kw)
    out_e = m.generate(_beam_keep_rows=True, **call)
    rows, rp, sc_e = m.last_beam_rows, m.last_beam_replay, m.last_beam_scores.clone()
    assert len(rows) == rp.steps
    it = iter(rows)
    seqs, scores, trace = R.beam_search(lambda running: next(it), B, MAX_NEW, eos, 1.0, False, B, pad=eos[0])
    assert len(trace) == rp.steps
    tol = LR.kernel_tolerance() + 0.5 * float(np.spacing(np.float32(64.0)))      # one step: the lp and the f32 sum (|s| < 128)
    for t, st in enumerate(trace):
        assert rp.tokens[t] == st["cand_token"].tolist() and rp.parents[t] == st["cand_parent"].tolist(), t
    log = m._beams[(B, 1)].log_score[:rp.steps].cpu().numpy().astype(np.float64)
    for t, st in enumerate(trace):
        fin = np.isfinite(st["cand_score"])
        assert np.abs(log[t][fin] - st["cand_score"][fin]).max() <= tol * (t + 1), (t, np.abs(log[t][fin] - st["cand_score"][fin]).max())
    assert any(rp.running_parents(t) != list(range(B)) for t in range(1, rp.steps - 1)), "no beam ever changed its parent: choose another seed"
    assert any(eos[0] in s and s.index(eos[0]) + 1 < MAX_NEW for s in seqs), "no hypothesis finished before max_length"
    assert out_e[:, L0:].tolist() == seqs and torch.equal(out_e[:, :L0], ids.expand(B, -1))
    assert np.abs(sc_e.numpy() - scores).max() <= tol * rp.steps
    for _ in range(2):      # the captured graph, twice: the same ids, the same bits
        out_g = m.generate(**call)
        assert torch.equal(out_g, out_e) and torch.equal(m.last_beam_scores.view(torch.int32), sc_e.view(torch.int32))
    assert m._beams[(B, 1)].beam_graph.graph is not None
    return out_e, sc_e


def test_num_beams_1_is_the_plain_call(dev, model):
    ids = _prompt(dev)
    plain = model.generate(input_ids=ids, max_new_tokens=MAX_NEW, bad_words_ids=BAD)
    assert torch.equal(model.generate(input_ids=ids, max_new_tokens=MAX_NEW, bad_words_ids=BAD, num_beams=1), plain)
    assert torch.equal(model.generate(input_ids=ids, max_new_tokens=MAX_NEW, bad_words_ids=BAD, num_beams=None, length_penalty=2.0), plain)
    assert model._beams == {} and model.last_beam_scores is None
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, max_new_tokens=4, num_return_sequences=2)


@pytest.mark.parametrize("B", [2, 4, 5])      # 2, 4: the VALU form of the batched step; 5: the matrix cores
def test_search_equals_the_reference_on_its_recorded_rows(dev, B):
    m = _model(dev)
    n_batches = len(m._batches)
    _replay_recorded_rows(m, _prompt(dev), B, bad_words_ids=BAD)
    assert len(m._batches) == n_batches and list(m._beams) == [(B, 0), (B, 1)]      # a cache of its own


@pytest.mark.parametrize("kw", [dict(kv_cache_dtype="fp8"), dict(quantization="fp8")], ids=["kv_fp8", "w_fp8"])
def test_search_with_fp8_cache_and_fp8_weights(dev, kw):
    _replay_recorded_rows(_model(dev, **kw), _prompt(dev), 4, bad_words_ids=BAD)


@pytest.mark.parametrize("kw", [{}, dict(kv_cache_dtype="fp8")], ids=["bf16", "kv_fp8"])
def test_cache_rows_follow_their_beams(dev, kw):
    """eager stepping: after every step slot b's rows [0, pos) are, bit for bit, the rows slot parent[b] held before the reorder"""
    m, ids, B = _model(dev, **kw), _prompt(dev), 4
    names = ["kc", "vc"] + (["ke", "ve"] if m.kv8 else [])
    snap, seen = {}, []

    def on_step(phase, bm):
        if phase == "pick":
            snap.update({k: getattr(bm, k).clone() for k in names})
            return
        pos, parent = int(bm.pos[0].item()), bm.parent.tolist()
        for k in names:
            for b in range(B):
                assert torch.equal(getattr(bm, k)[b][:, :, :pos], snap[k][parent[b]][:, :, :pos]), (k, b, pos)
            assert torch.equal(getattr(bm, k)[:, :, :, pos:], snap[k][:, :, :, pos:])      # rows past pos are not touched
        seen.append(parent)

    m.generate(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=B, bad_words_ids=BAD, _beam_on_step=on_step)
    assert seen[0] == [0] * B and len(seen) == m.last_beam_replay.steps
    assert any(p != list(range(B)) and len(set(p)) < B for p in seen[1:]), "no step with a parent map that is not a permutation"


def test_scores_are_those_of_score(dev, model):
    """every returned hypothesis, rescored by score() (a prefill over prompt + hypothesis, the raw model: no ban mask here): the sum
    of its tokens' log-probabilities is sequences_score x length ** length_penalty, within four times the largest difference between
    generate(logprobs=0).cumulative and score() on greedy continuations of the same lengths (a stale KV row would be off by nats)."""
    ids, B, lp_exp = _prompt(dev), 4, 0.6
    eos = [_eos_that_finishes_early(model, ids, B)]
    out = model.generate(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=B, num_return_sequences=B, eos_token_id=eos, length_penalty=lp_exp, pad_token_id=-1)
    scores = model.last_beam_scores.double().tolist()
    hyps = [[t for t in row if t != -1] for row in out[:, L0:].tolist()]
    assert len(set(map(tuple, hyps))) == B
    base = 0.0
    for n in sorted(set(map(len, hyps))):
        g = model.generate(input_ids=ids, max_new_tokens=n, logprobs=0)
        base = max(base, abs(model.last_logprobs.cumulative - float(model.score(g, start=L0).token_logprobs.double().sum())))
    tol = 4 * base
    print(f"generate(logprobs=0).cumulative vs score(): largest difference {base:.3e} -> tolerance {tol:.3e}")
    assert tol < 0.5
    for h, s in zip(hyps, scores):
        full = torch.cat([ids[0], torch.tensor(h, device=dev)])[None]
        rescored = float(model.score(full, start=L0).token_logprobs.double().sum())
        print(f"  length {len(h)}: beam {s * len(h) ** lp_exp:.6f}  score() {rescored:.6f}")
        assert abs(rescored - s * len(h) ** lp_exp) <= tol, (h, rescored, s * len(h) ** lp_exp, tol)


def test_length_and_stopping(dev, model):
    ids, B = _prompt(dev), 4
    eos = [_eos_that_finishes_early(model, ids, B, bad_words_ids=BAD)]
    kw = dict(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=B, num_return_sequences=B, eos_token_id=eos, bad_words_ids=BAD)
    out = model.generate(**kw)
    sc, steps_false = model.last_beam_scores, model.last_beam_replay.steps
    assert out.shape[0] == B and len(set(map(tuple, out.tolist()))) == B
    assert all(sc[i] >= sc[i + 1] for i in range(B - 1))
    assert (out[:, L0:] == eos[0]).any() and not any(t in range(250) for t in out[:, L0:].flatten().tolist())
    best = model.generate(**{**kw, "num_return_sequences": 1})
    assert torch.equal(best[0], out[0][:best.shape[1]]) and (out[0][best.shape[1]:] == eos[0]).all()
    model.generate(**kw, early_stopping=True)
    assert model.last_beam_replay.steps <= steps_false
    model.generate(**kw, early_stopping="never")
    assert model.last_beam_replay.steps >= steps_false
    with pytest.raises(NotImplementedError):
        model.generate(**kw, do_sample=True)
    with pytest.raises(NotImplementedError):
        model.generate(**kw, repetition_penalty=1.2)
    with pytest.raises(ValueError):
        model.generate(**{**kw, "num_return_sequences": 5})
    with pytest.raises(ValueError):
        model.generate(**{**kw, "eos_token_id": [1, 2, 3, 4]})


def test_serving_beam_search_equals_generate(dev, model):
    from usdm_amd.serving import LLM, BeamSearchParams
    ids, W = _prompt(dev), 4
    mask = torch.zeros(1000, dtype=torch.uint8, device=dev)
    mask[:250] = 1
    eos = _eos_that_finishes_early(model, ids, W, ban_mask=mask)
    want = model.generate(input_ids=ids, max_new_tokens=MAX_NEW, num_beams=W, num_return_sequences=W, eos_token_id=[eos], ban_mask=mask, pad_token_id=-1)
    want_scores = model.last_beam_scores.double().tolist()
    llm = LLM(model=model, tokenizer=None)
    outs = llm.beam_search([ids[0].tolist(), {"prompt_token_ids": ids[0].tolist()}],
                           BeamSearchParams(beam_width=W, max_tokens=MAX_NEW, stop_token_ids=[eos], static_logits_mask=mask))
    assert len(outs) == 2
    for o in outs:
        assert [s.tokens for s in o.sequences] == [[t for t in row if t != -1] for row in want.tolist()]
        for s, sc in zip(o.sequences, want_scores):
            assert s.cum_logprob == sc * (len(s.tokens) - L0) and s.text is None      # length_penalty 1.0
