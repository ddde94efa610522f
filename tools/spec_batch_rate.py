"""Cost of a batched speculative step (generate_batch(num_speculative_tokens=k)) on the random-init 7B, bf16, ONE process, 600-token
prompts, every case alternated with the others, short-minus-long differencing, best of --repeats (as tools/spec_rate.py).  Acceptance
with real weights cannot be measured here (there are none): the tool measures the two ends and the cost per step.
For (B, k) in (2, 7), (4, 3), (8, 1) - 16 rows per step each:
  plain_B      generate_batch's plain step for the B sequences                                    (the parent's code path)
  single_k     generate(num_speculative_tokens=k) for ONE sequence, all-wrong script              (the parent's code path)
  floor        the B sequences on the speculative slots, all-wrong scripts: every step emits 1 token per sequence
  ceiling      their own outputs as scripts: every step emits k + 1 tokens per sequence
  ms per step, tokens/s of the group; break-even = the mean tokens per step PER SEQUENCE at which the batched speculative call matches
  the plain batch = ms per batched speculative step / ms per plain step of B.
Then the two kernels alone, hip-event time per launch of 200 back-to-back launches:
  usdm_attn_verify_batch  on the 7B's head shape (Hq 32, Hkv 8, bf16, C = the model's split), every slot at 600 cached rows, against
                          its byte count 2 (K, V) x B x Hkv x rows x 256 B
  usdm_spec_commit_batch  on [B * T][nparts] partials of a 42 003-id vocabulary, every slot with a 600 + 100 token history (the state
                          is reset by replayed copies; those launches are timed alone and subtracted)
Prints one JSON line.
    python tools/spec_batch_rate.py [--new 128] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.spec_rate import V, _timed  # noqa: E402
from usdm_amd import ops, synth  # noqa: E402

SHAPES = ((2, 7), (4, 3), (8, 1))


def attn_verify_batch_us(dev, B, T, rows, C, Hq=32, Hkv=8, ctx=2048, d=128):
    bf = torch.bfloat16
    kc, vc = (torch.randn(B, Hkv, ctx, d, device=dev).to(bf) for _ in range(2))
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * d, device=dev).to(bf)
    n = B * T * Hq * ops.attn_verify_splits(ctx, C)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    ang = torch.arange(ctx, device=dev).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, d, 2, device=dev).float() / d)))[None]
    plan = ops.Plan()
    ops.attn_verify_batch(qkv, torch.full((B,), rows, dtype=torch.int32, device=dev), ang.cos().to(bf).contiguous(), ang.sin().to(bf).contiguous(),
                          kc, vc, f32(n), f32(n), f32(n * d), torch.zeros(B * T, Hq * d, dtype=bf, device=dev), B=B, T=T, Hq=Hq, Hkv=Hkv,
                          ctx_max=ctx, C=C, scale=d ** -0.5, cache_bs=Hkv * ctx * d, plan=plan)
    us = _timed(plan)
    nbytes = 2 * B * Hkv * rows * d * 2
    return dict(us=round(us, 2), bytes=nbytes, gb_s=round(nbytes / us / 1e3, 1))


def spec_commit_batch_us(dev, B, T, Hd=4096, P=600, nout=100, max_out=2048):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(1)
    nparts = ops.gemv_nblocks(V)
    pv = torch.randn(B * T, nparts, generator=g).to(dev)
    pi = torch.randint(0, V, (B * T, nparts), generator=g, dtype=torch.int32).to(dev)
    out = torch.zeros(B, max_out, dtype=torch.int32, device=dev)
    out[:, :nout] = torch.randint(32002, 42002, (B, nout), generator=g, dtype=torch.int32).to(dev)
    nxt, stp, pos, stp0, pos0 = i32([0] * B), i32([nout] * B), i32([P + nout] * B), i32([nout] * B), i32([P + nout] * B)
    st = ops.decode_state(nxt, out, stp, pos, batch=B, done=i32([0] * B), eos=i32([[0] * 8] * B))
    st.max_out = max_out
    E = torch.zeros(V, Hd, dtype=torch.bfloat16, device=dev)
    bufs = dict(drafts=i32([[-1] * 8] * B), limit=i32([max_out] * B), prompt=torch.randint(32002, 42002, (B, P), generator=g, dtype=torch.int32).to(dev),
                prompt_len=i32([P] * B), params=i32([3, 1, 0, 0]), counters=i32([[0, 0, 0]] * B))
    reset, both = ops.Plan(), ops.Plan()
    for p in (reset, both):      # (steps and positions back to their start, so that every launch does the same work)
        ops.copy_bytes(stp, stp0, 4 * B, plan=p)
        ops.copy_bytes(pos, pos0, 4 * B, plan=p)
    ops.spec_commit_batch(pv, pi, nparts, st, T=T, V=V, embed=E, h_out=torch.zeros(B * T, Hd, dtype=torch.bfloat16, device=dev), Hd=Hd, plan=both, **bufs)
    return round(_timed(both) - _timed(reset), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600), generator=g).to(dev) for _ in range(8)]
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    short, long_ = 8, 8 + a.new
    wrong = [0] * (long_ + 8)      # id 0 is banned: no pick equals it
    cases = {}
    for B, k in SHAPES:
        ps = prompts[:B]
        cases[f"plain_B{B}"] = (B, lambda n, ps=ps: (m.generate_batch(ps, n, bad_words_ids=ban), None)[1])

        def single(n, k=k):
            m.generate(input_ids=prompts[0], max_new_tokens=n, bad_words_ids=ban, num_speculative_tokens=k, _spec_script=wrong)
            return m.last_spec_stats["steps"]

        def batch(n, scripts, ps=ps, k=k):
            m.generate_batch(ps, n, bad_words_ids=ban, num_speculative_tokens=k, _spec_script=scripts)
            return max(s["steps"] for s in m.last_spec_stats)
        outs = m.generate_batch(ps, long_, bad_words_ids=ban, num_speculative_tokens=k, _spec_script=[wrong] * B)
        own = [o[0, 600:].tolist() for o in outs]
        cases[f"single_k{k}"] = (1, single)
        cases[f"B{B}_k{k}_floor"] = (B, lambda n, batch=batch, B=B: batch(n, [wrong] * B))
        cases[f"B{B}_k{k}_ceiling"] = (B, lambda n, batch=batch, own=own: batch(n, own))
    for _, run in cases.values():      # plans + graphs
        run(24)
    torch.cuda.synchronize()
    rows = {c: [] for c in cases}
    for _ in range(a.repeats):
        for c, (nseq, run) in cases.items():
            t = time.perf_counter(); s1 = run(short); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); s2 = run(long_); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            steps = a.new if s1 is None else s2 - s1
            rows[c].append((1e3 * (t2 - t1) / steps, nseq * a.new / (t2 - t1), steps))
    res = dict(new=a.new, repeats=a.repeats, spec_split=m.spec_split, prompt_len=600)
    for c, vs in rows.items():
        res[c] = dict(ms_per_step=[round(v[0], 3) for v in vs], best_ms_per_step=round(min(v[0] for v in vs), 3),
                      tokens_per_s=round(max(v[1] for v in vs), 1), steps=vs[0][2])
    for B, k in SHAPES:
        plain, single = res[f"plain_B{B}"]["best_ms_per_step"], res[f"single_k{k}"]["best_ms_per_step"]
        for end in ("floor", "ceiling"):
            r = res[f"B{B}_k{k}_{end}"]
            r["break_even_tokens_per_step_per_sequence"] = round(r["best_ms_per_step"] / plain, 3)
            r["step_vs_single_sequence_step"] = round(r["best_ms_per_step"] / single, 3)
    res["usdm_attn_verify_batch"] = {f"B{B}_T{k + 1}_rows600": attn_verify_batch_us(dev, B, k + 1, 600, m.spec_split) for B, k in SHAPES}
    res["usdm_spec_commit_batch_us_per_launch"] = {f"B{B}_T{k + 1}": spec_commit_batch_us(dev, B, k + 1) for B, k in SHAPES}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
