"""Cost of scoring given tokens (USDMForCausalLM.score) on the random-init 7B, bf16, ONE process, cases alternated per repeat.

For a prompt of L ~ 600 and L ~ 3500 unit ids:
  gen1       generate(max_new_tokens=1) of the same prompt on the same tree: the prefill + ONE lm_head row + the arg-max pick, the
             floor that score() cannot go below (it runs the same prefill)
  k0 / k20   score() of every token but the first, the given token only / with the 20 most likely ids per position
each for score_rows = 128 / 256 / 512 (rows per lm_head GEMM + usdm_prompt_logprobs launch; a model attribute, the plans are rebuilt).
Prefix reuse is off, so every call prefills the whole prompt.  Times are wall-clock per call after a warm-up call that builds the plan
(best and spread over --repeats).  Then usdm_prompt_logprobs alone: hip-event time per launch over [rows][42003] chunks.
Prints one JSON line and writes the same text to --out (default profiles/score_rate.txt).
    python tools/score_rate.py [--repeats 3] [--lengths 600,3500] [--rows 128,256,512]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usdm_amd import ops, synth  # noqa: E402


def kernel_us(dev, rows, K, n=50):
    V = 42003
    ld = (V + 3) // 4 * 4
    x = (torch.randn(rows, ld, device=dev) * 3).to(torch.bfloat16).float()
    ids = torch.randint(0, V, (rows + 1,), device=dev)
    bufs = dict(tok_lp=torch.zeros(rows + 1, device=dev), tok_rank=torch.zeros(rows + 1, dtype=torch.int32, device=dev),
                top_id=torch.zeros((rows + 1) * 20, dtype=torch.int32, device=dev), top_lp=torch.zeros((rows + 1) * 20, device=dev))
    plan = ops.Plan()
    ops.prompt_logprobs(x[:, :V], ids, row0=0, K=K, plan=plan, **bufs)
    for _ in range(5):
        plan.run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        plan.run()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / n, 1)


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lengths", default="600,3500")
    ap.add_argument("--rows", default="128,256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_rate.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lengths, rows = [int(x) for x in a.lengths.split(",")], [int(x) for x in a.rows.split(",")]
    m = synth.make_llm(dev, ctx_max=max(lengths) + 64)
    m.reuse_prefix = False
    gen = torch.Generator().manual_seed(3)
    res = dict(repeats=a.repeats, ms_per_call={})
    for L in lengths:
        ids = torch.randint(32002, 42002, (1, L), generator=gen).to(dev)
        cases = {"gen1": lambda: m.generate(input_ids=ids, max_new_tokens=1)}
        for R in rows:
            for K in (0, 20):
                def run(R=R, K=K):
                    if m.score_rows != R:      # (the plans bake the chunking in)
                        m.score_rows = R
                        m._score_plans.clear()
                    m.score(ids, top_logprobs=K)
                cases[f"rows{R}_k{K}"] = run
        times = {c: [] for c in cases}
        for rep in range(a.repeats + 1):
            for c, f in cases.items():
                if c != "gen1":
                    f()                # builds the plan of this (score_rows, K) again: the timed call below replays it
                t = timed(f)
                if rep:                # (the first round warms caches and allocations)
                    times[c].append(t)
        res["ms_per_call"][f"L{L}"] = {c: dict(ms=[round(t, 2) for t in ts], best=round(min(ts), 2),
                                                spread_pct=round(100 * (max(ts) - min(ts)) / min(ts), 1)) for c, ts in times.items()}
    res["usdm_prompt_logprobs_us_per_launch"] = {f"rows{R}_K{K}": kernel_us(dev, R, K) for R in rows for K in (0, 20)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
