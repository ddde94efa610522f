"""Cost of the on-device repetition / frequency / presence penalties (generate(repetition_penalty=...) / generate_batch(...)) on the
random-init 7B, bf16, ONE process, cases alternated per repeat, short-minus-long differencing (as tools/logprob_rate.py).

Cases at batch 1 (generate) and at 16 sequences (generate_batch):
  off      greedy on the arg-max path (the default step: must equal the parent commit within the spread this tool reports)
  sampled  batch 1 only: the sampling step (top_k = 50) without penalties - separates the sampler's cost from the penalty kernel's
  on       greedy + penalties (r = 1.2, f = 0.3, p = 0.3): the sampling step with top_k = 1 plus the usdm_penalize launch.  Against "off"
           this carries usdm_sample_final as well; against "sampled" only usdm_penalize
Then usdm_penalize alone: hip-event time per launch of 200 back-to-back launches on [1][42003] and [16][42003] rows, penalised and
neutral knobs.  Prints one JSON line.  --cases off,sampled runs on a tree without the feature too (the parent commit's "off").
    python tools/penalty_rate.py [--new 128] [--repeats 3] [--cases off,sampled,on]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402


def kernel_us(dev, B, knobs, n=200):
    V, max_out = 42003, 64
    x = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16).float()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    nxt, stp, pos, out = i32(B) + 17, i32(B) + 1, i32(B), i32(B, max_out) + 17
    st = ops.decode_state(nxt, out if B > 1 else out[0], stp, pos, batch=B if B > 1 else 0)
    f = (lambda t: t) if B > 1 else (lambda t: t[0])
    table = torch.randint(0, 3, (B, V), dtype=torch.int32, device=dev)      # about two thirds of the ids seen: every branch runs
    params = ops.penalty_params_tensor(dev, B).view(B, -1)
    for b in range(B):
        ops.set_penalty_params(params[b], *knobs)
    count = i32(B)      # count < step at the first launch only: the later ones are replays and count nothing (the table cannot overflow)
    plan = ops.Plan()
    ops.penalize(f(x), st, table=f(table), dev_params=f(params), count=count, plan=plan)
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
    ap.add_argument("--cases", default="off,sampled,on")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 16
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600 - 7 * b), generator=gen).to(dev) for b in range(B)]
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    pen = dict(repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.3)
    one = {"off": dict(), "sampled": dict(do_sample=True, top_k=50, seed=1), "on": pen}
    many = {"off": dict(), "on": pen}
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
    if "on" in want:
        res["usdm_penalize_us_per_launch"] = {f"B{b}_{k}": kernel_us(dev, b, kn) for b in (1, 16)
                                              for k, kn in (("penalised", (1.2, 0.3, 0.3)), ("neutral", ops.PENALTY_NEUTRAL))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
