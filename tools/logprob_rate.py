"""Cost of per-token log-probabilities (generate(logprobs=K) / generate_batch(logprobs=K)) on the random-init 7B, bf16, ONE process,
cases alternated per repeat, short-minus-long differencing (as tools/kv8_batch_rate.py).

Cases at batch 1 (generate) and at 16 sequences (generate_batch):
  off      greedy on the arg-max path (the default step: must equal the parent commit within the spread this tool reports)
  sampled  batch 1 only: the sampling step (top_k = 50) without log-probabilities - the step a log-probability request runs on
  k0 / k20 log-probabilities of the picked token only / with the 20 most likely ids.  A greedy request with log-probabilities runs on
           the sampling step with top_k = 1, so against "off" these carry usdm_sample_final as well; against "sampled" only usdm_logprobs
Then usdm_logprobs alone: hip-event time per launch of 200 back-to-back launches on [1][42003] and [16][42003] rows, K = 0 and 20.
Prints one JSON line.  --cases off,sampled runs on a tree without the feature too (the parent commit's "off" to compare with).
    python tools/logprob_rate.py [--new 128] [--repeats 3] [--cases off,sampled,k0,k20]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402


def kernel_us(dev, B, K, n=200):
    V, max_out = 42003, 64
    x = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16).float()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    nxt, stp, pos, out = i32(B) + 17, i32(B) + 1, i32(B), i32(B, max_out)
    st = ops.decode_state(nxt, out if B > 1 else out[0], stp, pos, batch=B if B > 1 else 0)
    f = (lambda t: t) if B > 1 else (lambda t: t[0])
    bufs = dict(tok_lp=f(torch.zeros(B, max_out, device=dev)), tok_rank=f(i32(B, max_out)), top_id=f(i32(B, max_out * 20)),
                top_lp=f(torch.zeros(B, max_out * 20, device=dev)))
    plan = ops.Plan()
    ops.logprobs(f(x), st, K=K, plan=plan, **bufs)
    for _ in range(10):
        plan.run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        plan.run()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / n, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="off,sampled,k0,k20")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 16
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600 - 7 * b), generator=gen).to(dev) for b in range(B)]
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    one = {"off": dict(), "sampled": dict(do_sample=True, top_k=50, seed=1), "k0": dict(logprobs=0), "k20": dict(logprobs=20)}
    many = {"off": dict(), "k0": dict(logprobs=0), "k20": dict(logprobs=20)}
    want = a.cases.split(",")
    one, many = ({c: kw for c, kw in d.items() if c in want} for d in (one, many))
    run1 = lambda kw, n: m.generate(input_ids=prompts[0], max_new_tokens=n, bad_words_ids=ban, **kw)
    runB = lambda kw, n: m.generate_batch(prompts, max_new_tokens=n, bad_words_ids=ban, **kw)
    res = dict(new=a.new, repeats=a.repeats)
    for name, cases, run, nb in (("batch1", one, run1, 1), ("batch16", many, runB, B)):
        for kw in cases.values():      # plans + decode graphs
            run(kw, 24)
        torch.cuda.synchronize()
        rates = {c: [] for c in cases}
        for _ in range(a.repeats):
            for c, kw in cases.items():
                t = time.perf_counter(); run(kw, 8); torch.cuda.synchronize()
                t1 = time.perf_counter() - t
                t = time.perf_counter(); run(kw, 8 + a.new); torch.cuda.synchronize()
                t2 = time.perf_counter() - t
                rates[c].append(nb * a.new / (t2 - t1))
        res[name] = {c: dict(tok_s=[round(r, 1) for r in rs], best=round(max(rs), 1), spread_pct=round(100 * (max(rs) - min(rs)) / max(rs), 2),
                             us_per_step=round(1e6 * nb / max(rs), 1)) for c, rs in rates.items()}
    if "k0" in want or "k20" in want:
        res["usdm_logprobs_us_per_launch"] = {f"B{b}_K{k}": kernel_us(dev, b, k) for b in (1, 16) for k in (0, 20)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
