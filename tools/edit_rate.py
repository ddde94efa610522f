"""Cost of the on-device logit bias / n-gram ban (generate(logit_bias=, no_repeat_ngram_size=)) and of min_p on the random-init 7B,
bf16, ONE process, cases alternated per repeat, short-minus-long differencing (as tools/penalty_rate.py).

Cases at batch 1 (generate) and at 16 sequences (generate_batch, which has no sampled form: off and edits only):
  off      greedy on the arg-max path (the default step: must equal the parent commit within the spread this tool reports)
  sampled  batch 1 only: the sampling step (top_k = 50) - the baseline of the next two
  min_p    batch 1 only: the same call with min_p = 0.05 (inside usdm_sample_final: no launch of its own)
  edits    greedy + no_repeat_ngram_size = 3 + 16 bias entries: the sampling step with top_k = 1 plus the usdm_logit_edit launch.  Against
           "off" this carries usdm_sample_final as well; against "sampled" only usdm_logit_edit
Then the kernels alone: hip-event time per launch of 200 back-to-back launches of usdm_logit_edit on [1][42003] and [16][42003] rows
(n = 3 over a history of 600 + 64 ids plus 16 bias entries; neutral), and of usdm_sample_final (top_k = 50) with min_p = 0 / 0.05.
Prints one JSON line.  --cases off,sampled runs on a tree without the feature too (the parent commit's).
    python tools/edit_rate.py [--new 128] [--repeats 3] [--cases off,sampled,min_p,edits]"""
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
    return round(1e3 * e0.elapsed_time(e1) / n, 2)


def _state(dev, B, max_out, step):
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    nxt, stp, pos = i32(B), i32(B) + step, i32(B)
    out = torch.randint(32002, 42002, (B, max_out), dtype=torch.int32, device=dev)
    return ops.decode_state(nxt, out if B > 1 else out[0], stp, pos, batch=B if B > 1 else 0), (nxt, stp, pos, out)


def edit_us(dev, B, on):
    x = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16).float()
    st, keep = _state(dev, B, 64, 64)
    f = (lambda t: t) if B > 1 else (lambda t: t[0])
    params = ops.edit_params_tensor(dev, B).view(B, -1)
    bias_id = torch.arange(40000, 40000 + ops.LOGIT_BIAS_MAX, dtype=torch.int32, device=dev).repeat(B, 1)
    bias_val = torch.zeros(B, ops.LOGIT_BIAS_MAX, device=dev)      # (adds 0: the row does not drift over the replays)
    prompt = torch.randint(32002, 42002, (B, 2048), dtype=torch.int32, device=dev)
    for b in range(B):
        ops.set_edit_params(params[b], *((3, 600, 16) if on else (0, 0, 0)))
    plan = ops.Plan()
    ops.logit_edit(f(x), st, dev_params=f(params), bias_id=f(bias_id), bias_val=f(bias_val), prompt=f(prompt), plan=plan)
    return _timed(plan)


def sample_us(dev, B, min_p):
    x = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16).float()
    st, keep = _state(dev, B, 4096, 0)
    sp = ops.sample_params_tensor(dev, B).view(B, -1)
    for b in range(B):
        ops.set_sample_params(sp[b], 1.0, 50, 1.0, b, **(dict(min_p=min_p) if min_p else {}))
    plan = ops.Plan()
    ops.sample_final(x if B > 1 else x[0], st, dev_params=sp if B > 1 else sp[0], plan=plan)
    return _timed(plan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="off,sampled,min_p,edits")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 16
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600 - 7 * b), generator=gen).to(dev) for b in range(B)]
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    edits = dict(no_repeat_ngram_size=3, logit_bias={32010 + 7 * i: (-1.0) ** i * (0.5 + i) for i in range(16)})
    sampled = dict(do_sample=True, top_k=50, seed=1)
    one = {"off": dict(), "sampled": sampled, "min_p": dict(sampled, min_p=0.05), "edits": edits}
    many = {"off": dict(), "edits": edits}
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
    if "edits" in want:
        res["usdm_logit_edit_us_per_launch"] = {f"B{b}_{k}": edit_us(dev, b, on) for b in (1, 16) for k, on in (("edits", True), ("neutral", False))}
    if "min_p" in want:
        res["usdm_sample_final_us_per_launch"] = {f"B{b}_min_p_{p}": sample_us(dev, b, p) for b in (1, 16) for p in (0.0, 0.05)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
