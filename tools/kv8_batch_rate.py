"""bf16 vs fp8 KV cache (kv_cache_dtype="fp8") at 16 sequences per decode step, random-init 7B (32 layers), fp8 weights on the matrix
cores, ONE process, cases alternated per repeat, short-minus-long generate_batch differencing, the text->unit ban mask.

Two context regimes: "600" = ragged ~600-row unit prompts at ctx_max 2048 (the setting of tools/fp8_batch_rate.py), "3500" = ragged
~3 500-row prompts at ctx_max 4096.  Prints one JSON line: tok/s per repeat, best / spread, ms per step and the bytes a step streams
(weight_bytes_per_token() + the sum over the sequences of kv_bytes_per_token_row() x mean context during the timed steps).
    python tools/kv8_batch_rate.py [--new 128] [--repeats 3] [--regime 600|3500] [--only bf16|fp8]
(--only: one cache type, e.g. under rocprofv3 --kernel-trace --stats; condense with tools/prof_summary.py.)
Two 7B models with 16-slot caches of 4096 rows are ~2 x (7.2 + 8.6 / 4.3) GB: one regime per process keeps that bounded."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import synth  # noqa: E402

REGIMES = {"600": (2048, 600), "3500": (4096, 3500)}      # ctx_max, longest prompt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--regime", choices=sorted(REGIMES), default="600")
    ap.add_argument("--only", choices=["bf16", "fp8"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 16
    ctx_max, L0 = REGIMES[a.regime]
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, L0 - 7 * b), generator=gen).to(dev) for b in range(B)]
    cases = [a.only] if a.only else ["bf16", "fp8"]
    models = {}
    for c in cases:       # same seed: the same weights, only the cache type differs
        models[c] = synth.make_llm(dev, ctx_max=ctx_max, quantization="fp8", fp8_matrix_cores=True, kv_cache_dtype=c)
        models[c].generate_batch(prompts, max_new_tokens=24, bad_words_ids=ban)      # plans + decode graph
        torch.cuda.synchronize()
    rates = {c: [] for c in cases}
    for _ in range(a.repeats):
        for c in cases:
            m = models[c]
            t = time.perf_counter(); m.generate_batch(prompts, max_new_tokens=8, bad_words_ids=ban); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); m.generate_batch(prompts, max_new_tokens=8 + a.new, bad_words_ids=ban); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            rates[c].append(B * a.new / (t2 - t1))
    rows = sum(p.shape[1] + 8 + a.new / 2 for p in prompts)      # cached rows read per timed step, summed over the sequences (mean)
    res = dict(regime=a.regime, ctx_max=ctx_max, B=B, new=a.new)
    for c in cases:
        best, m = max(rates[c]), models[c]
        wb, kvb = m.weight_bytes_per_token(), m.kv_bytes_per_token_row() * rows
        res[c] = dict(tok_s=[round(r, 1) for r in rates[c]], best=round(best, 1), spread_pct=round(100 * (best - min(rates[c])) / best, 2),
                      ms_per_step=round(1e3 * B / best, 4), weight_GB_per_step=round(wb / 1e9, 3), kv_GB_per_step=round(kvb / 1e9, 3))
    if len(cases) == 2:
        res["fp8_over_bf16"] = round(res["fp8"]["best"] / res["bf16"]["best"], 3)
        res["bytes_fp8_over_bf16"] = round((res["fp8"]["weight_GB_per_step"] + res["fp8"]["kv_GB_per_step"]) /
                                           (res["bf16"]["weight_GB_per_step"] + res["bf16"]["kv_GB_per_step"]), 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
