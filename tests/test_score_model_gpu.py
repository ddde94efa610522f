"""Scoring given tokens through the model (USDMForCausalLM.score) and the serving surface (LLM.score) on small synthetic models,
score_rows = 16 so that short prompts cross chunk boundaries.

Two yardsticks.  EXACT: keep_score_logits exposes the logits rows the device scored; every reported row must equal the float64
reference on its row (tests/_logprob_reference: ids and ranks exactly, values within the kernel tolerance derived there).
ORACLE: log_softmax of oracle.mistral_oracle.forward's logits at the given ids.  Tolerance per row 2 x 4e-2 x max|ref logits of the
row|: tests/test_llm_gpu.py::test_first_token_logits_vs_oracle bounds the prefill's logits error by 4e-2 x scale, and a log-probability
moves by at most the error in x_tok plus the error in the logsumexp (which is at most the largest logit error).  Only token
log-probabilities are compared with the oracle; ids and ranks are judged by the exact check, so near-ties between two GEMM orders need
no exception list.  The tests print the largest error they see; on an MI355X: 1.61e-02 at a tolerance of 3.20e-01 (40-token prompt),
1.60e-02 at 2.83e-01 (fp8 weights), 3.10e-02 at 2.69e-01 (two tensor-parallel ranks), 1.59e-02 at 2.31e-01 (against generate's rows)."""
import os
import threading

import numpy as np
import pytest
import torch

from tests import _logprob_reference as R

pytestmark = pytest.mark.gpu

SMALL = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
TP_CFG = dict(SMALL, vocab_size=1003, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=4)
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
FIELDS = ("token_logprobs", "ranks", "top_ids", "top_logprobs")


@pytest.fixture(scope="module")
def sd():
    from oracle import mistral_oracle as MO
    return MO.random_state_dict(SMALL, seed=5)


def _model(dev, sd, cfg=SMALL, score_rows=16, **kw):
    from usdm_amd.llm import USDMForCausalLM
    return USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=256, score_rows=score_rows, **kw)


def _ids(n, seed=1, vocab=1000):
    return torch.randint(0, vocab, (1, n), generator=torch.Generator().manual_seed(seed))


def _same(a, b):
    return all(torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32)) for f in FIELDS) and a.cumulative == b.cumulative


def _check_exact(lp, ids, start, rows, K):
    """every scored row against the float64 reference on the logits row the device scored"""
    toks, tol = ids[0, start:].tolist(), R.kernel_tolerance()
    assert lp.token_logprobs.shape == (len(toks),) and lp.top_ids.shape == (len(toks), K) and tuple(rows.shape)[0] == len(toks)
    for i, tok in enumerate(toks):
        R.check_row(rows[i], tok, lp.token_logprobs[i], lp.ranks[i], lp.top_ids[i], lp.top_logprobs[i], K, tol)
    assert lp.cumulative == float(lp.token_logprobs.double().sum())


def _oracle(sd, cfg, ids):
    """(float64 log-probability of ids[t] given ids[< t] for t = 1 .. L-1, the tolerance of each) from the CPU oracle"""
    from oracle import mistral_oracle as MO
    ref, _ = MO.forward(sd, cfg, ids[0])
    lp = torch.log_softmax(ref[:-1].double(), -1).gather(1, ids[0, 1:, None])[:, 0]
    return lp, 2 * 4e-2 * ref[:-1].abs().max(-1).values.double()


def _check_oracle(lp, want, tol, what):
    err = (lp.token_logprobs.double() - want).abs()
    print(f"{what}: largest |lp - oracle| {err.max().item():.3e} at a tolerance of {tol[err.argmax()].item():.3e}")
    assert (err <= tol).all(), (err.max().item(), tol.min().item())


@pytest.fixture(scope="module")
def base(dev, sd):
    """the 40-token prompt scored once with K = 5 (chunks of 16 / 16 / 7 rows), and the logits rows the device scored"""
    m = _model(dev, sd)
    m.keep_score_logits = True
    ids = _ids(40)
    lp = m.score(ids.to(dev), top_logprobs=5)
    return dict(m=m, ids=ids, lp=lp, rows=m.last_score_logits.cpu().numpy().copy())


def test_exact_against_the_devices_own_logits(base):
    rows = base["rows"]
    assert rows.shape == (39, 1000)
    assert np.array_equal(rows, torch.from_numpy(rows).to(torch.bfloat16).float().numpy())      # bf16-valued, as the lm_head GEMV writes
    _check_exact(base["lp"], base["ids"], 1, rows, 5)
    assert (40, 0, 0, 5) in base["m"]._score_plans


def test_against_the_cpu_oracle(base, sd):
    want, tol = _oracle(sd, SMALL, base["ids"])
    _check_oracle(base["lp"], want, tol, "40-token prompt")


def test_chunking_does_not_matter(dev, sd, base):
    for rows in (32, 256):
        assert _same(_model(dev, sd, score_rows=rows).score(base["ids"].to(dev), top_logprobs=5), base["lp"]), rows
    again = base["m"].score(base["ids"].to(dev), top_logprobs=5)       # (and the cached plan replays to the same bits)
    assert _same(again, base["lp"])
    k0 = base["m"].score(base["ids"].to(dev))                          # K = 0 / None: the given tokens only
    assert k0.top_ids.shape == (39, 0) and torch.equal(k0.token_logprobs, base["lp"].token_logprobs) and torch.equal(k0.ranks, base["lp"].ranks)
    part = base["m"].score(base["ids"].to(dev), top_logprobs=5, start=30)
    assert all(torch.equal(getattr(part, f), getattr(base["lp"], f)[29:]) for f in FIELDS)


def test_relation_to_generation(dev, sd):
    """prompt + 6 generated tokens, scored: the rows of the generated tokens came from decode GEMVs (the first from the prefill's last
    row) when they were generated and come from the GEMM here; both are within the oracle tolerance of each other"""
    m = _model(dev, sd)
    prompt = _ids(23, seed=3).to(dev)
    out = m.generate(input_ids=prompt, max_new_tokens=6, logprobs=0, bad_words_ids=None)
    gen = m.last_logprobs
    assert out.shape[1] == 29 and gen.token_logprobs.shape == (6,)
    lp = _model(dev, sd).score(out, start=23)
    _, tol = _oracle(sd, SMALL, out.cpu())
    err = (lp.token_logprobs.double() - gen.token_logprobs.double()).abs()
    print(f"score vs generate(logprobs=0): largest difference {err.max().item():.3e} (first token {err[0].item():.3e}), tolerance {tol[22:].min().item():.3e}")
    assert (err <= tol[22:]).all()


def test_prefix_reuse(dev, sd):
    m = _model(dev, sd)
    assert m.reuse_prefix
    A, B1, B2 = _ids(32, seed=11), _ids(8, seed=12), _ids(11, seed=13)
    c1, c2 = torch.cat([A, B1], 1).to(dev), torch.cat([A, B2], 1).to(dev)
    got1 = m.score(c1, top_logprobs=3, start=32)
    got2 = m.score(c2, top_logprobs=3, start=32)
    keys = list(m._score_plans.keys())
    assert keys[0] == (40, 0, 31, 3) and keys[1][1] >= 16 and keys[1] == (43 - keys[1][1], keys[1][1], 31 - keys[1][1], 3), keys
    for c, got in ((c1, got1), (c2, got2)):
        fresh = _model(dev, sd)
        fresh.reuse_prefix = False
        assert _same(fresh.score(c, top_logprobs=3, start=32), got)
        assert list(fresh._score_plans.keys())[0][1] == 0
    # a generate() after a score(): exactly what a fresh model returns
    kw = dict(max_new_tokens=7, bad_words_ids=[[i] for i in range(250)])
    assert torch.equal(m.generate(input_ids=c2, **kw), _model(dev, sd).generate(input_ids=c2, **kw))
    assert any(k[1] > 0 for k in m._prefill_plans), "the generate() after the score() did not reuse the scored rows"


def test_score_leaves_the_generation_state_alone(dev, sd):
    m = _model(dev, sd)
    m.keep_logits = True
    ids = _ids(40).to(dev)
    kw = dict(input_ids=ids, max_new_tokens=9, do_sample=True, temperature=1.1, top_k=50, top_p=0.9, seed=17, logprobs=3, repetition_penalty=1.2,
              bad_words_ids=[[i] for i in range(250)])
    out1, lp1 = m.generate(**kw), m.last_logprobs
    logits1 = m.last_logits.clone()
    m.score(_ids(37, seed=9).to(dev), top_logprobs=2)
    assert m.last_logprobs is lp1 and torch.equal(m.last_logits.view(torch.int32), logits1.view(torch.int32))
    out2 = m.generate(**kw)
    assert torch.equal(out1, out2) and _same(m.last_logprobs, lp1)


def _wprime(sd):
    """the state dict with every streamed matrix replaced by its dequantized FP8 form W' (row scales: per matrix = per packed matrix)"""
    from usdm_amd.quant import dequantize_rows, quantize_rows
    return {k: dequantize_rows(*quantize_rows(v.to(torch.bfloat16))) if (k == "lm_head.weight" or any(p in k for p in PROJ)) else v
            for k, v in sd.items()}


@pytest.mark.parametrize("quant", ["fp8", "mxfp4"])
def test_quantized_weights(dev, sd, quant):
    m = _model(dev, sd, quantization=quant)
    m.keep_score_logits = True
    ids = _ids(40)
    lp = m.score(ids.to(dev), top_logprobs=5)
    _check_exact(lp, ids, 1, m.last_score_logits.cpu().numpy(), 5)
    assert m._head_bf16 is not None and m._head_bf16.shape == (1000, 512) and m.dq_scratch.numel() == 2 * 1024 * 512      # (not grown)
    head = m._head_bf16
    assert _same(m.score(ids.to(dev), top_logprobs=5), lp) and m._head_bf16 is head                    # dequantized once
    if quant == "fp8":      # exactly the bf16 model with the dequantized weights W': the oracle on W'
        want, tol = _oracle(_wprime(sd), SMALL, ids)
        _check_oracle(lp, want, tol, "fp8 weights, oracle on the dequantized state dict")


def test_fp8_kv_cache_scores_like_the_bf16_cache(dev, sd, base):
    """the prompt's own attention reads its unquantized K / V, so nothing changes; and nothing is reused"""
    m = _model(dev, sd, kv_cache_dtype="fp8")
    assert _same(m.score(base["ids"].to(dev), top_logprobs=5), base["lp"])
    assert _same(m.score(base["ids"].to(dev), top_logprobs=5, start=30), base["lp"].__class__(*(getattr(base["lp"], f)[29:] for f in FIELDS)))
    assert all(k[1] == 0 for k in m._score_plans.keys())


def test_tensor_parallel_two_logical_ranks(dev):
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.p2p import InProcessGroup
    tp, K = 2, 5
    sd = MO.random_state_dict(TP_CFG, seed=13)
    ids = _ids(40, seed=4, vocab=1003)
    grp = InProcessGroup(tp, threaded=True)
    os.environ["USDM_NO_GRAPH"] = "1"          # as tests/test_tp_batch_gpu.py runs its two threads
    try:
        ranks = [USDMForCausalLM.from_state_dict(sd, TP_CFG, dev, ctx_max=128, tp_rank=r, tp_size=tp, group=grp, score_rows=16) for r in range(tp)]
        torch.cuda.synchronize()
        outs, rows, errs = [None] * tp, [None] * tp, [None] * tp

        def work(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    ranks[r].keep_score_logits = True
                    outs[r] = ranks[r].score(ids.to(dev), top_logprobs=K)
                    rows[r] = ranks[r].last_score_logits.cpu().numpy().copy()
                    torch.cuda.current_stream().synchronize()
            except Exception as e:  # noqa: BLE001 - reported below
                errs[r] = e
                try:
                    grp._bar.abort()
                except Exception:  # noqa: BLE001
                    pass
        th = [threading.Thread(target=work, args=(r,)) for r in range(tp)]
        for t in th:
            t.start()
        for t in th:
            t.join(180)
        assert not any(t.is_alive() for t in th), "a rank is stuck"
        assert errs == [None] * tp, errs
    finally:
        os.environ.pop("USDM_NO_GRAPH", None)
    assert _same(outs[0], outs[1]), "logical ranks disagree"
    for r in range(tp):
        assert rows[r].shape == (39, 1003)
        _check_exact(outs[r], ids, 1, rows[r], K)
        want, tol = _oracle(sd, TP_CFG, ids)
        _check_oracle(outs[r], want, tol, f"tensor parallel, rank {r}")


def test_serving_score(dev, sd):
    from usdm_amd.serving import LLM, SamplingParams, ScoreOutput, assemble_logprobs
    m = _model(dev, sd)
    eng = LLM(model=m, max_num_seqs=4)
    prompts = [_ids(n, seed=20 + n)[0].tolist() for n in (19, 40, 27)]
    starts, K = [1, 5, 12], 4
    sp = SamplingParams(top_k=1, max_tokens=6, logprobs=2, ignore_eos=True)
    # (one prompt: the single-sequence path, whose cache score() writes; two: the batch slots)
    run = lambda: [(o.outputs[0].token_ids, o.outputs[0].logprobs) for n in (1, 2) for o in eng.generate(prompt_token_ids=prompts[:n], sampling_params=sp)]
    before = run()
    outs = eng.score(prompt_token_ids=prompts, top_logprobs=K, start=starts)
    assert len(outs) == 3 and all(isinstance(o, ScoreOutput) for o in outs)
    for p, s, o in zip(prompts, starts, outs):
        lp = _model(dev, sd).score(torch.tensor([p], device=dev), top_logprobs=K, start=s)
        want, total = assemble_logprobs(p[s:], lp.token_logprobs, lp.ranks, lp.top_ids, lp.top_logprobs, K)
        assert o.prompt_token_ids == p and len(o.prompt_logprobs) == len(p)
        assert o.prompt_logprobs[:s] == [None] * s and o.prompt_logprobs[s:] == want
        assert o.cumulative_logprob == total and abs(total - lp.cumulative) <= 1e-9
        assert all(len(d) in (K, K + 1) and p[s + i] in d for i, d in enumerate(o.prompt_logprobs[s:]))
    one = eng.score(prompt_token_ids=prompts[0])                   # a single prompt, start = None = 1, K = 0
    assert len(one) == 1 and one[0].prompt_logprobs[0] is None and all(list(d) == [t] for d, t in zip(one[0].prompt_logprobs[1:], prompts[0][1:]))
    assert run() == before
