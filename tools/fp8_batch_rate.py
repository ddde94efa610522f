"""Aggregate batched-decode tokens/s of the random-init 7B (32 layers) in ONE process, alternated: bf16 at B = 16 (matrix cores),
quantization="fp8" with fp8_matrix_cores at B = 16 (usdm_gemv_fp8_mfma), and FP8 at B = 4 (the VALU FP8 form; the same FP8 model,
whose groups of <= 4 keep that form).

ctx_max 2048, ragged unit-id prompts of 600 - 7 b tokens, the text->unit ban mask of the reference's TTS round (as tools/batch_rate.py).
Each repeat times a short and a long generate_batch of each case (the difference is pure decode steps) and alternates the cases, so
all see the same clocks.  Prints one JSON line: tok/s per repeat, best / spread, ms per step, and the ratios.
    python tools/fp8_batch_rate.py [--new 128] [--repeats 3] [--only bf16_b16|fp8mc_b16|fp8_b4]
(--only: one case, e.g. under rocprofv3 --kernel-trace --stats.)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import synth  # noqa: E402

CASES = {"bf16_b16": ("bf16", 16), "fp8mc_b16": ("fp8", 16), "fp8_b4": ("fp8", 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600 - 7 * b), generator=gen).to(dev) for b in range(16)]
    cases = [a.only] if a.only else list(CASES)
    models = {}
    for c in cases:       # same seed: the FP8 model is the quantized bf16 model
        kind, B = CASES[c]
        if kind not in models:
            models[kind] = synth.make_llm(dev, ctx_max=2048, **({} if kind == "bf16" else dict(quantization="fp8", fp8_matrix_cores=True)))
        models[kind].generate_batch(prompts[:B], max_new_tokens=24, bad_words_ids=ban)      # plans + decode graph
        torch.cuda.synchronize()
    rates = {c: [] for c in cases}
    for _ in range(a.repeats):
        for c in cases:
            kind, B = CASES[c]
            m = models[kind]
            t = time.perf_counter(); m.generate_batch(prompts[:B], max_new_tokens=8, bad_words_ids=ban); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); m.generate_batch(prompts[:B], max_new_tokens=8 + a.new, bad_words_ids=ban); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            rates[c].append(B * a.new / (t2 - t1))
    res = {}
    for c in cases:
        best = max(rates[c])
        res[c] = dict(tok_s=[round(r, 1) for r in rates[c]], best=round(best, 1), spread_pct=round(100 * (best - min(rates[c])) / best, 2),
                      ms_per_step=round(1e3 * CASES[c][1] / best, 4))
    if len(cases) == 3:
        res["fp8mc_b16_over_bf16_b16"] = round(res["fp8mc_b16"]["best"] / res["bf16_b16"]["best"], 3)
        res["fp8mc_b16_over_fp8_b4"] = round(res["fp8mc_b16"]["best"] / res["fp8_b4"]["best"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
