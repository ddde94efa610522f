"""Batched decode on the tensor-parallel path (SURVEY.md 8e x 8f-2; VERDICT r03 next 8: code + one-GPU validation, no timing):
row-parallel projections leave f32 partials [B][H] -> ONE all-reduce per projection for the whole batch -> usdm_residual_add;
vocab-parallel pick over the ranks' gathered partials (usdm_argmax_final_seg).  Validated the two ways a one-GPU box allows:
  1. the code path on a 1-rank RCCL group (real collectives, captured or eager) must equal the single-GPU batched step bit for bit;
  2. two LOGICAL ranks (real shards of every weight) in two threads with in-process collectives: both ranks produce the same tokens,
     and every sequence equals oracle greedy generation under the near-tie rule."""
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(vocab_size=1003, hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8,
           num_key_value_heads=4, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
BAD = [[i] for i in range(100, 400)]


def _prompts(dev, B, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 1000, (1, 19 + 5 * b), generator=g).to(dev) for b in range(B)]


@pytest.mark.parametrize("B", [3, 6])
def test_tp_batched_code_path_single_rank_rccl(dev, B):
    """B = 3: VALU batch kernel; B = 6: matrix-core form.  tp_segments=True runs the tensor-parallel plan (partials, collectives,
    residual-add kernel, gathered pick) on a 1-rank group: the same arithmetic as the fused epilogues -> identical tokens."""
    import torch.distributed as dist
    from oracle import mistral_oracle as MO
    from usdm_amd.llm import USDMForCausalLM, step_kind
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        sd = MO.random_state_dict(CFG, seed=13)
        ps = _prompts(dev, B)
        a = USDMForCausalLM.from_state_dict(sd, CFG, dev, ctx_max=128).generate_batch(ps, max_new_tokens=14, bad_words_ids=BAD)
        m = USDMForCausalLM.from_state_dict(sd, CFG, dev, ctx_max=128, tp_segments=True, group=dist.group.WORLD)
        b = m.generate_batch(ps, max_new_tokens=14, bad_words_ids=BAD)
        dec = m._batches[B].steps[step_kind()]
        print(f"B={B}: TP batched step graph captured: {dec.graph is not None} (fallback reason: {dec.failed})")
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("B", [3, 6])
def test_tp_batched_two_logical_ranks_vs_oracle(dev, B):
    from oracle import mistral_oracle as MO
    from tests._greedy_compare import check_against_oracle
    from usdm_amd.llm import USDMForCausalLM
    from usdm_amd.p2p import InProcessGroup
    tp, new = 2, 12
    sd = MO.random_state_dict(CFG, seed=13)
    ps = _prompts(dev, B)
    grp = InProcessGroup(tp, threaded=True)
    os.environ["USDM_NO_GRAPH"] = "1"          # two threads capturing at once would trip over each other; launches stay eager
    try:
        ranks = [USDMForCausalLM.from_state_dict(sd, CFG, dev, ctx_max=128, tp_rank=r, tp_size=tp, group=grp) for r in range(tp)]
        torch.cuda.synchronize()
        outs, errs = [None] * tp, [None] * tp

        def work(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    outs[r] = [o[0].tolist() for o in ranks[r].generate_batch(ps, max_new_tokens=new, bad_words_ids=BAD)]
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
        assert outs[0] == outs[1], "logical ranks disagree on the generated tokens"
    finally:
        os.environ.pop("USDM_NO_GRAPH", None)
    firsts = []
    for p, seq in zip(ps, outs[0]):
        ref, ref_logits = MO.greedy_generate(sd, CFG, p[0].cpu(), new, bad_words_ids=BAD, return_logits=True)
        firsts.append(check_against_oracle(seq, ref, ref_logits, p.shape[1]))
    print(f"B={B}, 2 logical ranks: first differences vs the oracle (near-ties only): {firsts}")
