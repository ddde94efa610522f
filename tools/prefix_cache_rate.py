"""What enable_prefix_caching buys and costs on the random-init 7B, ONE process, option on and off alternated:
  batch    16 sequences through three chained generate_batch rounds with bench.py's pipeline_throughput lengths (560-token prompts
           + 32 text tokens, + 6 template tokens + 32 text tokens, + 1 token + `--units` unit tokens), bf16 cache: per round the
           admission (prefill) time of the 16 prompts - every DecodeSlots.admit call between two device synchronisations - the rows prefilled and
           the usdm_kv_reorder copies (each sequence finds its prefix in its own slot: none are expected)
  single   one fp8-cache sequence through generate()'s three rounds of the same lengths, and score() of 8 candidates of 20 tokens
           behind one 500-token context: the prefill time (the plan's launches between two synchronisations) and the rows prefilled,
           with reuse_prefix "exact" (what the flag switches on) against False (an fp8 model without the flag)
  kernels  usdm_kv_expand per launch (hip events over 200 back-to-back launches) on one layer of the 7B's cache (Hkv = 8, ctx 2048) at
           n = 592 and 630 rows, bf16 and fp8, against its byte count (read: Hkv x n x 256 B, fp8 2 x Hkv x n x 129 B; written: Hkv x n x
           256 B, fp8 twice that); and one usdm_kv_reorder copy of 592 rows of all layers between two of 16 slots
Prints one JSON line.
    python tools/prefix_cache_rate.py [--repeats 3] [--units 500] [--parts batch,single,kernels]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402

ROUNDS = ((32, 6), (32, 1))      # (new tokens, template tokens in front of the next round) of rounds 1 and 2; round 3 generates --units


class Stopwatch:
    """wraps a bound method: every call runs between two device synchronisations and adds its wall time to .ms"""

    def __init__(self, fn):
        self.fn, self.ms = fn, 0.0

    def __call__(self, *a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = self.fn(*a, **kw)
        torch.cuda.synchronize()
        self.ms += 1e3 * (time.perf_counter() - t)
        return out

    def take(self):
        ms, self.ms = self.ms, 0.0
        return round(ms, 2)


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


def batch_rounds(m, prompts, units, g, on):
    """the three rounds once -> per round dict(admit_ms, rows_prefilled, copies)"""
    m.prefix_caching = on
    m.reset_prefix_cache()
    m.stats.clear()
    watch, out = m.decode_slots(len(prompts)).admit, []
    for new, glue in ROUNDS + ((units, 0),):
        copies0 = m.stats.get("prefix_copies", 0)
        rows0 = m.stats.get("prefill_rows", 0)
        outs = m.generate_batch(prompts, max_new_tokens=new)
        rows = (m.stats.get("prefill_rows", 0) - rows0) if on else sum(int(p.shape[1]) for p in prompts)
        out.append(dict(admit_ms=watch.take(), rows_prefilled=rows, kv_reorder_copies=m.stats.get("prefix_copies", 0) - copies0))
        prompts = [torch.cat([o, torch.randint(0, 32000, (1, glue), generator=g).to(o.device)], 1) for o in outs]
    return out


def single_rounds(m, prompt, units, g, mode, ctx_ids, cands):
    m.reuse_prefix = mode
    m.reset_prefix_cache()
    watch, out = m._run_segs, dict(rounds=[], score=[])
    p = prompt
    for new, glue in ROUNDS + ((units, 0),):
        o = m.generate(input_ids=p, max_new_tokens=new)
        # (the plan this call ran is keyed (rows, past): with reuse on, the one with the largest past among those of this length)
        rows = int(p.shape[1]) - (max((k[1] for k in m._prefill_plans if k[0] + k[1] == p.shape[1]), default=0) if mode else 0)
        out["rounds"].append(dict(prefill_ms=watch.take(), rows_prefilled=rows))
        p = torch.cat([o, torch.randint(0, 32000, (1, glue), generator=g).to(o.device)], 1)
    for c in cands:
        ids = torch.cat([ctx_ids, c], 1)
        m.score(ids, start=int(ctx_ids.shape[1]) + 1)
        out["score"].append(watch.take())
    return out


def expand_us(dev, n, fp8, Hkv=8, ctx=2048):
    dt = torch.uint8 if fp8 else torch.bfloat16
    kc, vc = torch.zeros(Hkv, ctx, 128, dtype=dt, device=dev), torch.zeros(Hkv, ctx, 128, dtype=dt, device=dev)
    Spad = (n + 38 + 63) // 64 * 64
    vt = torch.zeros(Hkv, 128, Spad, dtype=torch.bfloat16, device=dev)
    kw = {}
    if fp8:
        kw = dict(kv8=(torch.zeros(Hkv, ctx, dtype=torch.int8, device=dev), torch.zeros(Hkv, ctx, dtype=torch.int8, device=dev)),
                  kscr=torch.zeros(Hkv, Spad, 128, dtype=torch.bfloat16, device=dev), kscr_ld=Spad)
    plan = ops.Plan()
    ops.kv_expand(kc, vc, vt, n=n, Hkv=Hkv, ctx_max=ctx, vt_ld=Spad, plan=plan, **kw)
    us = _timed(plan)
    nbytes = Hkv * n * (2 * 129 + 2 * 256 if fp8 else 256 + 256)
    return dict(us=round(us, 2), bytes=nbytes, gb_s=round(nbytes / us / 1e3, 1))


def reorder_us(dev, rows, B=16, L=32, Hkv=8, ctx=2048):
    kc = torch.zeros(B, L * Hkv, ctx, 128, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    plan = ops.Plan()
    ops.kv_reorder([kc, vc], i32([0, 0] + list(range(2, B))), i32([0]), i32([rows]), B=B, nblk=L * Hkv, ctx_max=ctx, plan=plan)
    us = _timed(plan, 50)
    nbytes = 2 * L * Hkv * rows * 256 * 2      # K and V, read + write
    return dict(us=round(us, 2), bytes=nbytes, gb_s=round(nbytes / us / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--units", type=int, default=500)
    ap.add_argument("--parts", default="batch,single,kernels")
    a = ap.parse_args()
    dev, parts = torch.device("cuda:0"), a.parts.split(",")
    g = torch.Generator().manual_seed(3)
    res = dict(repeats=a.repeats, units=a.units)
    if "batch" in parts:
        m = synth.make_llm(dev, ctx_max=2048, enable_prefix_caching=True)
        prompts = [torch.randint(0, 32000, (1, 560), generator=g).to(dev) for _ in range(16)]
        ds = m.decode_slots(len(prompts))      # the 16 slots generate_batch runs these prompts on
        ds.admit = Stopwatch(ds.admit)
        for on in (False, True):      # plans, graphs
            batch_rounds(m, prompts, a.units, torch.Generator().manual_seed(4), on)
        runs = {"off": [], "on": []}
        for _ in range(a.repeats):
            for name, on in (("off", False), ("on", True)):
                runs[name].append(batch_rounds(m, prompts, a.units, torch.Generator().manual_seed(4), on))
        res["batch16"] = {name: [dict(rows_prefilled=r[0][i]["rows_prefilled"], kv_reorder_copies=r[0][i]["kv_reorder_copies"],
                                      admit_ms=[x[i]["admit_ms"] for x in r], best=min(x[i]["admit_ms"] for x in r)) for i in range(3)]
                          for name, r in runs.items()}
        del m
        torch.cuda.empty_cache()
    if "single" in parts:
        m = synth.make_llm(dev, ctx_max=2048, kv_cache_dtype="fp8", enable_prefix_caching=True)
        m._run_segs = Stopwatch(m._run_segs)
        prompt = torch.randint(0, 32000, (1, 560), generator=g).to(dev)
        ctx_ids = torch.randint(0, 32000, (1, 500), generator=g).to(dev)
        cands = [torch.randint(0, 32000, (1, 20), generator=g).to(dev) for _ in range(8)]
        modes = (("off", False), ("on", "exact"))
        for _, mode in modes:
            single_rounds(m, prompt, a.units, torch.Generator().manual_seed(5), mode, ctx_ids, cands)
        runs = {"off": [], "on": []}
        for _ in range(a.repeats):
            for name, mode in modes:
                runs[name].append(single_rounds(m, prompt, a.units, torch.Generator().manual_seed(5), mode, ctx_ids, cands))
        res["fp8_single"] = {name: dict(rounds=[dict(rows_prefilled=r[0]["rounds"][i]["rows_prefilled"],
                                                     prefill_ms=[x["rounds"][i]["prefill_ms"] for x in r],
                                                     best=min(x["rounds"][i]["prefill_ms"] for x in r)) for i in range(3)],
                                        score8_ms=[round(sum(x["score"]), 2) for x in r], score_first_ms=min(x["score"][0] for x in r),
                                        score_later_ms=min(min(x["score"][1:]) for x in r)) for name, r in runs.items()}
        del m
        torch.cuda.empty_cache()
    if "kernels" in parts:
        res["usdm_kv_expand"] = {f"{'fp8' if f else 'bf16'}_n{n}": expand_us(dev, n, f) for f in (False, True) for n in (592, 630)}
        res["usdm_kv_reorder_592_rows"] = reorder_us(dev, 592)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
