"""Cost of a speculative step (generate(num_speculative_tokens=k)) on the random-init 7B, bf16, ONE process, alternated with the plain
step, short-minus-long differencing (as tools/beam_rate.py).  Acceptance with real weights cannot be measured here (there are none):
the tool measures the two ends and the cost per step.
  floor    an all-wrong script (a banned id as every draft): every step emits 1 token
  ceiling  the run's own output as script: every step emits k + 1 tokens
  ms per step and tokens/s at both ends for k in {1, 3, 7}, next to the plain step's; break-even = the mean tokens per step at which
  the speculative call matches the plain one = ms per speculative step / ms per plain step.
Then the two kernels alone, hip-event time per launch of 200 back-to-back launches:
  usdm_attn_verify  on the 7B's head shape (Hq 32, Hkv 8, bf16, C = the model's split) at 600 and 3 500 cached rows, T in {2, 4, 8},
                    against its byte count 2 (K, V) x Hkv x rows x 256 B
  usdm_spec_commit  on [T][nparts] partials of a 42 003-id vocabulary with a 600 + 100 token history (the state is reset by a replayed
                    copy; that launch is timed alone and subtracted)
Prints one JSON line.
    python tools/spec_rate.py [--new 128] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402

V = 42003


def _timed(plan, n=200):
    for _ in range(10):
        plan.run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        plan.run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def attn_verify_us(dev, T, rows, C, Hq=32, Hkv=8, ctx=4096, d=128):
    bf = torch.bfloat16
    kc, vc = (torch.randn(Hkv, ctx, d, device=dev).to(bf) for _ in range(2))
    qkv = torch.randn(T, (Hq + 2 * Hkv) * d, device=dev).to(bf)
    ns = ops.attn_verify_splits(ctx, C)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    ang = torch.arange(ctx, device=dev).float()[:, None] * (1.0 / (10000.0 ** (torch.arange(0, d, 2, device=dev).float() / d)))[None]
    plan = ops.Plan()
    ops.attn_verify(qkv, torch.tensor([rows], dtype=torch.int32, device=dev), ang.cos().to(bf).contiguous(), ang.sin().to(bf).contiguous(), kc, vc,
                    f32(T * Hq * ns), f32(T * Hq * ns), f32(T * Hq * ns * d), torch.zeros(T, Hq * d, dtype=bf, device=dev), T=T, Hq=Hq,
                    Hkv=Hkv, ctx_max=ctx, C=C, scale=d ** -0.5, plan=plan)
    us = _timed(plan)
    nbytes = 2 * Hkv * rows * d * 2
    return dict(us=round(us, 2), bytes=nbytes, gb_s=round(nbytes / us / 1e3, 1))


def spec_commit_us(dev, T, Hd=4096, P=600, nout=100, max_out=2048):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(1)
    nparts = ops.gemv_nblocks(V)
    pv = torch.randn(T, nparts, generator=g).to(dev)
    pi = torch.randint(0, V, (T, nparts), generator=g, dtype=torch.int32).to(dev)
    out = torch.zeros(max_out, dtype=torch.int32, device=dev)
    out[:nout] = torch.randint(32002, 42002, (nout,), generator=g, dtype=torch.int32).to(dev)
    nxt, stp, pos, stp0, pos0 = i32([0]), i32([nout]), i32([P + nout]), i32([nout]), i32([P + nout])
    st = ops.decode_state(nxt, out, stp, pos, done=i32([0]), eos=i32([0] * 8))
    E = torch.zeros(V, Hd, dtype=torch.bfloat16, device=dev)
    bufs = dict(drafts=i32([-1] * 8), limit=i32([max_out]), prompt=torch.randint(32002, 42002, (P,), generator=g, dtype=torch.int32).to(dev),
                prompt_len=i32([P]), params=i32([3, 1, 0, 0]), counters=i32([0, 0, 0]))
    reset, both = ops.Plan(), ops.Plan()
    for p in (reset, both):      # (step and position back to their start, so that every launch does the same work)
        ops.copy_bytes(stp, stp0, 4, plan=p)
        ops.copy_bytes(pos, pos0, 4, plan=p)
    ops.spec_commit(pv, pi, nparts, st, T=T, V=V, embed=E, h_out=torch.zeros(T, Hd, dtype=torch.bfloat16, device=dev), Hd=Hd, plan=both, **bufs)
    return round(_timed(both) - _timed(reset), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ks", default="1,3,7")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    prompt = torch.randint(32002, 42002, (1, 600), generator=torch.Generator().manual_seed(3)).to(dev)
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    short, long_ = 8, 8 + a.new
    wrong = [0] * (long_ + 8)      # id 0 is banned: no pick equals it
    cases = {"plain": lambda n: (m.generate(input_ids=prompt, max_new_tokens=n, bad_words_ids=ban), None)[1]}
    for k in (int(x) for x in a.ks.split(",")):
        own = m.generate(input_ids=prompt, max_new_tokens=long_, bad_words_ids=ban, num_speculative_tokens=k, _spec_script=wrong)[0, 600:].tolist()

        def run(n, k=k, script=None):
            m.generate(input_ids=prompt, max_new_tokens=n, bad_words_ids=ban, num_speculative_tokens=k, _spec_script=script)
            return m.last_spec_stats["steps"]
        cases[f"k{k}_floor"] = lambda n, run=run: run(n, script=wrong)
        cases[f"k{k}_ceiling"] = lambda n, run=run, own=own: run(n, script=own)
    for run in cases.values():      # plans + graphs
        run(24)
    torch.cuda.synchronize()
    rows = {c: [] for c in cases}
    for _ in range(a.repeats):
        for c, run in cases.items():
            t = time.perf_counter(); s1 = run(short); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); s2 = run(long_); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            steps = a.new if s1 is None else s2 - s1
            rows[c].append((1e3 * (t2 - t1) / steps, a.new / (t2 - t1), steps))
    res = dict(new=a.new, repeats=a.repeats, spec_split=m.spec_split)
    for c, vs in rows.items():
        res[c] = dict(ms_per_step=[round(v[0], 3) for v in vs], best_ms_per_step=round(min(v[0] for v in vs), 3),
                      tokens_per_s=round(max(v[1] for v in vs), 1), steps=vs[0][2])
    plain = res["plain"]["best_ms_per_step"]
    for c in rows:
        if c != "plain":
            res[c]["break_even_tokens_per_step"] = round(res[c]["best_ms_per_step"] / plain, 3)
    res["usdm_attn_verify"] = {f"T{T}_rows{r}": attn_verify_us(dev, T, r, m.spec_split) for T in (2, 4, 8) for r in (600, 3500)}
    res["usdm_spec_commit_us_per_launch"] = {f"T{T}": spec_commit_us(dev, T) for T in (2, 4, 8)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
