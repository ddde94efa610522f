"""Batch-1 decode tokens/s of the random-init 7B (32 layers): bf16, quantization="fp8" and quantization="mxfp4" in ONE process,
alternated.

600-token prompt of unit ids, the text->unit ban mask of the reference's TTS round.  Each repeat times a short and a long
generate() of each model (the difference is pure decode steps) and alternates the models, so all see the same clocks.
Prints one JSON line: tok/s per repeat, best / spread, ms per token, weight bytes per token and the implied TB/s.
    python tools/mxfp4_decode_rate.py [--new 256] [--prompt 600] [--repeats 3] [--only bf16|fp8|mxfp4]
(--only: one model, e.g. under rocprofv3 --kernel-trace --stats.)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import synth  # noqa: E402

KINDS = ["bf16", "fp8", "mxfp4"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=KINDS, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    ids = torch.randint(32002, 42002, (1, a.prompt), generator=torch.Generator().manual_seed(3)).to(dev)
    kinds = [a.only] if a.only else KINDS
    models = {}
    for k in kinds:       # same seed: the quantized models are the quantized bf16 model
        models[k] = synth.make_llm(dev, ctx_max=2048, quantization=None if k == "bf16" else k)
        models[k].generate(input_ids=ids, max_new_tokens=24, bad_words_ids=ban)      # plans + decode graph
        torch.cuda.synchronize()
    rates = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for k in kinds:
            m = models[k]
            t = time.perf_counter(); m.generate(input_ids=ids, max_new_tokens=8, bad_words_ids=ban); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); m.generate(input_ids=ids, max_new_tokens=8 + a.new, bad_words_ids=ban); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            rates[k].append(a.new / (t2 - t1))
    res = {}
    for k in kinds:
        best = max(rates[k])
        wb = models[k].weight_bytes_per_token()
        res[k] = dict(tok_s=[round(r, 1) for r in rates[k]], best=round(best, 1), spread_pct=round(100 * (best - min(rates[k])) / best, 2),
                      ms_per_token=round(1e3 / best, 4), weight_bytes_per_token=wb, weight_tb_s=round(wb * best / 1e12, 3))
    if not a.only:
        res["mxfp4_over_bf16"] = round(res["mxfp4"]["best"] / res["bf16"]["best"], 3)
        res["mxfp4_over_fp8"] = round(res["mxfp4"]["best"] / res["fp8"]["best"], 3)
        res["fp8_over_bf16"] = round(res["fp8"]["best"] / res["bf16"]["best"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
