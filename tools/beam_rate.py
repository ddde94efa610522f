"""Cost of a beam-search step (generate(num_beams=B)) on the random-init 7B, bf16, ONE process, short-minus-long differencing (as
tools/edit_rate.py): ms per step at B = 4 and 16, next to generate_batch's greedy step of the same B sequences (the step the beam
step extends by usdm_beam_step + usdm_kv_reorder; --cases greedy runs on a tree without the feature too, which is how the parent
commit's figure is taken).  Then the two kernels alone, hip-event time per launch of 200 back-to-back launches:
  usdm_beam_step   on [B][42003] rows, one EOS id (the state is reset by a replayed copy; that launch is timed alone and subtracted)
  usdm_kv_reorder  of the 7B's caches (L = 32, Hkv = 8, d = 128, bf16), rows [600, 600 + gen) by a 3-cycle + duplicates map, against
                   its byte count 2 (K, V) x moved slots x L x Hkv x (pos - lo) x 256 B, read + write
Prints one JSON line.
    python tools/beam_rate.py [--new 64] [--repeats 3] [--cases greedy,beam] [--gen 64]"""
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


def beam_step_us(dev, B):
    KC = ops.beam_candidates(B, 1)
    x = (torch.randn(B, V, device=dev) * 3).to(torch.bfloat16).float()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    nxt, stp, pos, out = i32(B), i32(B), i32(B), i32(B, 64)
    st = ops.decode_state(nxt, out, stp, pos, batch=B)
    score, zero = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    stp0 = i32(B)
    bufs = dict(score=score, parent=i32(B), eos=i32(3) + 32002, log_score=torch.zeros(64, KC, device=dev), log_token=i32(64, KC),
                log_parent=i32(64, KC), cand_score=torch.zeros(B, KC, device=dev), cand_index=i32(B, KC))
    reset, both = ops.Plan(), ops.Plan()
    for p in (reset, both):      # (scores and the step counter back to their start, so that every launch does the same work)
        ops.copy_bytes(score, zero, 4 * B, plan=p)
        ops.copy_bytes(stp, stp0, 4 * B, plan=p)
    ops.beam_step(x, st, nlive=B, n_eos=1, plan=both, **bufs)
    return round(_timed(both) - _timed(reset), 2)


def reorder_us(dev, B, gen, lo=600, L=32, Hkv=8, ctx=2048, d=128):
    kc = torch.zeros(B, L * Hkv, ctx, d, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    par = [1, 2, 0, 0] + list(range(4, B)) if B == 4 else [1, 2, 0, 0, 4, 4, 7, 6] + list(range(8, B))
    moved = sum(p != b for b, p in enumerate(par))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    plan = ops.Plan()
    ops.kv_reorder([kc, vc], i32(par), i32([lo]), i32([lo + gen] * B), B=B, nblk=L * Hkv, ctx_max=ctx, plan=plan)
    us = _timed(plan)
    nbytes = 2 * moved * L * Hkv * gen * 2 * d * 2      # K and V, read + write
    return dict(us=round(us, 2), moved_slots=moved, bytes=nbytes, gb_s=round(nbytes / us / 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="greedy,beam")
    ap.add_argument("--gen", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    want = a.cases.split(",")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompt = torch.randint(32002, 42002, (1, 600), generator=gen).to(dev)
    m = synth.make_llm(dev, ctx_max=2048)
    m.reuse_prefix = False
    res = dict(new=a.new, repeats=a.repeats)
    for B in (4, 16):
        cases = {}
        if "greedy" in want:
            cases["greedy"] = lambda n, B=B: m.generate_batch([prompt] * B, max_new_tokens=n, bad_words_ids=ban)
        if "beam" in want:      # no EOS id and early_stopping="never": the search runs all n steps
            cases["beam"] = lambda n, B=B: m.generate(input_ids=prompt, max_new_tokens=n, bad_words_ids=ban, num_beams=B, early_stopping="never")
        for run in cases.values():      # plans + graphs
            run(24)
        torch.cuda.synchronize()
        ms = {c: [] for c in cases}
        for _ in range(a.repeats):
            for c, run in cases.items():
                t = time.perf_counter(); run(8); torch.cuda.synchronize()
                t1 = time.perf_counter() - t
                t = time.perf_counter(); run(8 + a.new); torch.cuda.synchronize()
                t2 = time.perf_counter() - t
                ms[c].append(1e3 * (t2 - t1) / a.new)
        res[f"B{B}"] = {c: dict(ms_per_step=[round(v, 3) for v in vs], best=round(min(vs), 3)) for c, vs in ms.items()}
    if "beam" in want:
        res["usdm_beam_step_us_per_launch"] = {f"B{B}": beam_step_us(dev, B) for B in (4, 16)}
        res["usdm_kv_reorder"] = {f"B{B}": reorder_us(dev, B, a.gen) for B in (4, 16)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
