"""Aggregate batched-decode tokens/s of the random-init 7B (32 layers) at 8 and 16 sequences in ONE process, alternated:
  mxfp4mc  quantization="mxfp4" with mxfp4_matrix_cores (usdm_gemv_mxfp4_mfma, one step per token for the whole group);
  mxfp4    quantization="mxfp4" without the flag: what an mxfp4 user had before (max_batch() == 4: generate_batch runs groups of 4);
  fp8mc    quantization="fp8" with fp8_matrix_cores (usdm_gemv_fp8_mfma);
  bf16     the default (usdm_gemv_batch on the matrix cores).
Then the four projection launches of a layer alone (qkv with the fused RMSNorm, o with the residual, gate/up with SwiGLU, down with
the K split) at 8 and 16 sequences for mxfp4mc, fp8mc and bf16, against the bytes one pass over the matrix streams.

ctx_max 2048, ragged unit-id prompts of 600 - 7 b tokens, the text->unit ban mask of the reference's TTS round (as
tools/fp8_batch_rate.py).  Each repeat times a short and a long generate_batch of each case (the difference is pure decode steps)
and alternates the cases, so all see the same clocks; best of --repeats.  The projection launches run over the 32 layers' own
matrices in turn (7B: 0.8 - 7.5 GB per pass, no matrix is still cached when its turn comes again) between two device events.
Prints one JSON line.
    python tools/mxfp4_batch_rate.py [--new 128] [--repeats 3] [--only mxfp4mc|mxfp4|fp8mc|bf16] [--no-projections]
(--only: one case, e.g. under rocprofv3 --kernel-trace --stats.)"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from usdm_amd import ops, synth  # noqa: E402

KINDS = {"mxfp4mc": dict(quantization="mxfp4", mxfp4_matrix_cores=True), "mxfp4": dict(quantization="mxfp4"),
         "fp8mc": dict(quantization="fp8", fp8_matrix_cores=True), "bf16": {}}
BATCHES = (8, 16)


def projections(m, kind, nb, passes):
    """{projection: (us per launch, bytes per launch)} of model m's layer matrices at nb sequences"""
    dev, bf = m.device, torch.bfloat16
    c = m.cfg
    H, I, nq = c["hidden_size"], m.I, m.W["layers"][0]["qkv"].shape[0]
    fn = {"mxfp4mc": ops.gemv_mxfp4_mfma, "fp8mc": ops.gemv_fp8_mfma, "bf16": ops.gemv_batch}[kind]
    form = 1 if kind == "bf16" else 0
    g = torch.Generator(device=dev).manual_seed(5)
    xh, xa, xi = (torch.randn(16, k, device=dev, generator=g).to(bf) for k in (H, m.Hq * c["head_dim"], I))
    yq, yh, yi = (torch.zeros(16, n, dtype=bf, device=dev) for n in (nq, H, I))
    ksf = ops.gemv_batch_ks_floats(H, I)
    ks = (torch.zeros(ksf, device=dev), torch.zeros(-(-H // 16), dtype=torch.int32, device=dev)) if ksf else None
    calls = {
        "qkv": lambda L: fn(L["qkv"], xh, nb=nb, N=nq, K=H, x_bs=H, y_bs=nq, norm_w=L["ln1"], eps=c["rms_norm_eps"], y16=yq, form=form),
        "o": lambda L: fn(L["o"], xa, nb=nb, N=H, K=xa.shape[1], x_bs=xa.shape[1], y_bs=H, res_bs=H, residual=yh, y16=yh, form=form),
        "gate_up": lambda L: fn(L["gu"], xh, nb=nb, N=2 * I, K=H, x_bs=H, y_bs=I, norm_w=L["ln2"], eps=c["rms_norm_eps"], act=3, y16=yi, form=form),
        "down": lambda L: fn(L["down"], xi, nb=nb, N=H, K=I, x_bs=I, y_bs=H, res_bs=H, residual=yh, y16=yh, form=form, ks=ks)}
    key = {"qkv": "qkv", "o": "o", "gate_up": "gu", "down": "down"}
    out = {}
    for name, call in calls.items():
        for L in m.W["layers"]:      # warm-up: code objects, every matrix touched once
            call(L)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(passes):
            for L in m.W["layers"]:
                call(L)
        e1.record()
        torch.cuda.synchronize()
        W = m.W["layers"][0][key[name]]
        nbytes = W.nbytes_matrix_cores if kind == "mxfp4mc" else W.nbytes if kind == "fp8mc" else W.numel() * 2
        us = 1e3 * e0.elapsed_time(e1) / (passes * len(m.W["layers"]))
        out[name] = dict(us=round(us, 2), mb=round(nbytes / 1e6, 2), tb_s=round(nbytes / us / 1e6, 3))
    out["sum_us"] = round(sum(v["us"] for v in out.values()), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=sorted(KINDS), default=None)
    ap.add_argument("--no-projections", action="store_true")
    ap.add_argument("--passes", type=int, default=8, help="passes over the 32 layers per projection timing")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ban = [[i] for i in range(32002) if i != 28705]      # text -> unit: only unit ids and the EOS
    gen = torch.Generator().manual_seed(3)
    prompts = [torch.randint(32002, 42002, (1, 600 - 7 * b), generator=gen).to(dev) for b in range(16)]
    kinds = [a.only] if a.only else list(KINDS)
    models = {}
    for k in kinds:       # same seed: every quantized model is the quantized bf16 model
        models[k] = synth.make_llm(dev, ctx_max=2048, **KINDS[k])
        for B in BATCHES:
            models[k].generate_batch(prompts[:B], max_new_tokens=24, bad_words_ids=ban)      # plans + decode graphs
        torch.cuda.synchronize()
    cases = [(k, B) for B in BATCHES for k in kinds]
    rates = {c: [] for c in cases}
    for _ in range(a.repeats):
        for k, B in cases:
            m = models[k]
            t = time.perf_counter(); m.generate_batch(prompts[:B], max_new_tokens=8, bad_words_ids=ban); torch.cuda.synchronize()
            t1 = time.perf_counter() - t
            t = time.perf_counter(); m.generate_batch(prompts[:B], max_new_tokens=8 + a.new, bad_words_ids=ban); torch.cuda.synchronize()
            t2 = time.perf_counter() - t
            rates[(k, B)].append(B * a.new / (t2 - t1))
    res = dict(max_batch={k: models[k].max_batch() for k in kinds})
    for k, B in cases:
        r = rates[(k, B)]
        best = max(r)
        # ms per token of the whole group: one step on the matrix cores, ceil(B / 4) steps of four without them
        res[f"{k}_b{B}"] = dict(tok_s=[round(x, 1) for x in r], best=round(best, 1), spread_pct=round(100 * (best - min(r)) / best, 2),
                               ms_per_token_of_the_group=round(1e3 * B / best, 4))
    if not a.only:
        for B in BATCHES:
            for other in ("mxfp4", "fp8mc", "bf16"):
                res[f"mxfp4mc_over_{other}_b{B}"] = round(res[f"mxfp4mc_b{B}"]["best"] / res[f"{other}_b{B}"]["best"], 3)
    if not a.no_projections:
        for k in kinds:
            if k != "mxfp4":
                for B in BATCHES:
                    res[f"projections_{k}_b{B}"] = projections(models[k], k, B, a.passes)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
