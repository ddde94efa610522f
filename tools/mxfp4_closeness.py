"""How close are the quantized LLMs (quantization="fp8", quantization="mxfp4") to the bf16 model?  Not a pass / fail number: a
measurement, and on random-init weights, whose logits are nearly flat: it says little about a trained checkpoint.

Teacher-forced along the bf16 model's own greedy continuation of a random prompt.  Per step the relative L2 of the logits
(quantized vs bf16) and whether the arg-max agrees; printed per format: the mean and the maximum relative L2 over the steps and the
share of agreeing arg-maxes.
    python tools/mxfp4_closeness.py --side cpu|gpu [--layers 2] [--steps 32] [--prompt 32]
cpu: oracle.mistral_oracle.forward on the dequantized weights W' against the plain oracle;
gpu: the quantized models against the bf16 model, forced through generate(_logits_hook=...).
Full-width Mistral-7B shapes with --layers layers (32 = the random-init 7B), oracle-style random weights (seed 0)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mistral_oracle as MO  # noqa: E402
from usdm_amd.quant import dequantize_mxfp4, dequantize_rows, quantize_mxfp4, quantize_rows  # noqa: E402

PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
bf = torch.bfloat16


def wprime(sd, kind):
    """the state dict the quantized model computes with: W' of every streamed matrix (mxfp4: the lm_head is fp8)"""
    f8 = lambda t: dequantize_rows(*quantize_rows(t.to(bf)))
    f4 = lambda t: dequantize_mxfp4(*quantize_mxfp4(t.to(bf)))
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight":
            out[k] = f8(v)
        elif any(p in k for p in PROJ):
            out[k] = f8(v) if kind == "fp8" else f4(v)
    return out


def summarize(side, kind, la, lb, extra):
    rel = (lb - la).double().norm(dim=1) / la.double().norm(dim=1)
    agree = la.argmax(1) == lb.argmax(1)
    print(json.dumps(dict(side=side, quantization=kind, steps=int(rel.numel()), rel_l2_mean=round(float(rel.mean()), 5),
                          rel_l2_max=round(float(rel.max()), 5), argmax_agree=int(agree.sum()),
                          argmax_agree_share=round(float(agree.float().mean()), 4), **extra)), flush=True)


def cpu_side(cfg, ids, steps):
    sd = MO.random_state_dict(cfg, seed=0)

    def run(w, forced):
        logits, cache = MO.forward(w, cfg, ids)
        rows, toks = [logits[-1].clone()], []
        for i in range(steps):
            tok = forced[i] if forced is not None else int(torch.argmax(rows[-1]))
            toks.append(tok)
            logits, cache = MO.forward(w, cfg, torch.tensor([tok]), cache)
            rows.append(logits[-1].clone())
        return torch.stack(rows).float(), toks
    la, toks = run(sd, None)
    return la, {k: run(wprime(sd, k), toks)[0] for k in ("fp8", "mxfp4")}


def gpu_side(cfg, ids, steps):
    from usdm_amd.llm import USDMForCausalLM
    dev = torch.device("cuda:0")
    sd = MO.random_state_dict(cfg, seed=0)
    out = {}
    forced = None
    for kind in ("bf16", "fp8", "mxfp4"):
        m = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=256, quantization=None if kind == "bf16" else kind)
        m.keep_logits = True
        rows = []

        def hook():
            rows.append(m.last_logits.clone())
            if forced is not None and len(rows) <= len(forced):      # force the pick: every other id to -inf
                m.last_logits.fill_(float("-inf"))
                m.last_logits[forced[len(rows) - 1]] = 0.0
        o = m.generate(input_ids=ids[None].to(dev), max_new_tokens=steps + 1, _logits_hook=hook, seed=1)
        out[kind] = torch.stack(rows).cpu()
        if forced is None:
            forced = o[0, ids.numel():].tolist()
        del m
        torch.cuda.empty_cache()
    return out["bf16"], {k: out[k] for k in ("fp8", "mxfp4")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=32)
    a = ap.parse_args()
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=a.layers)
    ids = torch.randint(0, cfg["vocab_size"], (a.prompt,), generator=torch.Generator().manual_seed(7))
    la, q = (cpu_side if a.side == "cpu" else gpu_side)(cfg, ids, a.steps)
    for kind, lb in q.items():
        summarize(a.side, kind, la, lb, dict(layers=a.layers, prompt=a.prompt))


if __name__ == "__main__":
    main()
