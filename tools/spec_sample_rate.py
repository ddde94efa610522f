"""Cost of the SAMPLED speculative step (generate(num_speculative_tokens=k, speculative_sampling=True)) on the
random-init 7B, bf16, ONE process, alternated with the greedy speculative step at the same k and the plain sampled step,
short-minus-long differencing (as tools/spec_rate.py).  Acceptance on real text cannot be measured here (there are no real weights):
the tool measures the two ends and the cost per step.
  floor    an all-wrong script (a banned id as every draft): every step emits 1 token
  ceiling  the run's own output as script: every step emits k + 1 tokens (for a fixed seed the ids do not depend on the drafts)
  ms per step and tokens/s at both ends for k in {1, 3, 7}; break-even = the mean tokens per step at which the sampled speculative call
  matches the plain sampled one = ms per sampled speculative step / ms per plain sampled step.
Then usdm_spec_sample alone, hip-event time per launch of 200 back-to-back launches, on T in {2, 4, 8} rows of a 42 003-id vocabulary
(every row reachable; temperature 0.8, top_k 20, top_p 0.9).
Prints one JSON line.
    python tools/spec_sample_rate.py [--new 128] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402

V = 42003
KNOBS = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=17)


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


def spec_sample_us(dev, T):
    g = torch.Generator().manual_seed(T)
    rows = (torch.randn(T, V, generator=g) * 3).to(dev)
    block = ops.sample_params_tensor(dev, 2)[:1]
    ops.set_sample_params(block[0], 0.8, 20, 0.9, 17)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    plan = ops.Plan()
    ops.spec_sample(rows, torch.zeros(T, dtype=torch.int32, device=dev), T=T, n=1, dev_params=block, step=i32([100]), done=i32([0]),
                    drafts=i32([[0] * 8]), plan=plan)
    return round(_timed(plan), 2)


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
    gen = lambda n, **kw: m.generate(input_ids=prompt, max_new_tokens=n, bad_words_ids=ban, **kw)
    cases = {"plain_sampled": lambda n: (gen(n, **KNOBS), None)[1]}
    for k in (int(x) for x in a.ks.split(",")):
        own_s = gen(long_, num_speculative_tokens=k, speculative_sampling=True, _spec_script=wrong, **KNOBS)[0, 600:].tolist()
        own_g = gen(long_, num_speculative_tokens=k, _spec_script=wrong)[0, 600:].tolist()

        def run(n, k=k, script=None, sampled=True):
            gen(n, num_speculative_tokens=k, _spec_script=script, **(dict(KNOBS, speculative_sampling=True) if sampled else {}))
            return m.last_spec_stats["steps"]
        cases[f"sampled_k{k}_floor"] = lambda n, run=run: run(n, script=wrong)
        cases[f"sampled_k{k}_ceiling"] = lambda n, run=run, own=own_s: run(n, script=own)
        cases[f"greedy_k{k}_floor"] = lambda n, run=run: run(n, script=wrong, sampled=False)
        cases[f"greedy_k{k}_ceiling"] = lambda n, run=run, own=own_g: run(n, script=own, sampled=False)
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
    res = dict(new=a.new, repeats=a.repeats, spec_split=m.spec_split, knobs={k: v for k, v in KNOBS.items() if k != "do_sample"})
    for c, vs in rows.items():
        res[c] = dict(ms_per_step=[round(v[0], 3) for v in vs], best_ms_per_step=round(min(v[0] for v in vs), 3),
                      tokens_per_s=round(max(v[1] for v in vs), 1), steps=vs[0][2])
    plain = res["plain_sampled"]["best_ms_per_step"]
    for c in rows:
        if c.startswith("sampled_"):
            res[c]["break_even_tokens_per_step"] = round(res[c]["best_ms_per_step"] / plain, 3)
    res["usdm_spec_sample_us_per_launch"] = {f"T{T}": spec_sample_us(dev, T) for T in (2, 4, 8)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
