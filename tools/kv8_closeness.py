"""How close is the fp8 KV cache (kv_cache_dtype="fp8") to the bf16 cache?  Not a pass / fail number: a measurement.

Teacher-forced along the bf16-cache model's own greedy continuation of a random prompt: step 0 comes from the prefill (identical by
construction: the prompt attends to its unquantized K / V), steps 1 .. N are decode steps that read the cached rows.  Per step the
relative L2 of the logits (fp8 cache vs bf16 cache) and whether the arg-max agrees; printed: the last step's relative L2, the mean and
the maximum over the decode steps, and the share of agreeing arg-maxes.
    python tools/kv8_closeness.py --side cpu|gpu [--layers 2] [--steps 64] [--prompt 32]
cpu: the KV-quantized reference (oracle.mistral_oracle.forward + quant.roundtrip_kv_rows) against the plain oracle;
gpu: the fp8-KV model against the bf16-KV model (same weights), forced through generate(_logits_hook=...).
Full-width Mistral-7B shapes with --layers layers (32 = the random-init 7B), oracle-style random weights (seed 0)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mistral_oracle as MO  # noqa: E402
from usdm_amd.quant import roundtrip_kv_rows  # noqa: E402


def summarize(name, la, lb, extra):
    """la / lb: [N + 1, V] logits of the bf16-cache and the fp8-cache side (row 0 = the prefill's)."""
    rel = ((lb - la).double().norm(dim=1) / la.double().norm(dim=1))[1:]
    agree = (la.argmax(1) == lb.argmax(1))[1:]
    res = dict(side=name, steps=int(rel.numel()), prefill_logits_identical=bool(torch.equal(la[0], lb[0])),
               rel_l2_last=round(float(rel[-1]), 5), rel_l2_mean=round(float(rel.mean()), 5), rel_l2_max=round(float(rel.max()), 5),
               argmax_agree=int(agree.sum()), argmax_agree_share=round(float(agree.float().mean()), 4), **extra)
    print(json.dumps(res), flush=True)


def cpu_side(cfg, ids, steps):
    sd = MO.random_state_dict(cfg, seed=0)
    ident = lambda t: t

    def run(rt, forced):
        logits, cache = MO.forward(sd, cfg, ids)
        cache = [(rt(k), rt(v)) for k, v in cache]
        rows, toks = [logits[-1].clone()], []
        for i in range(steps):
            tok = forced[i] if forced is not None else int(torch.argmax(rows[-1]))
            toks.append(tok)
            logits, cache = MO.forward(sd, cfg, torch.tensor([tok]), cache)
            cache = [(torch.cat([k[:, :-1], rt(k[:, -1:])], 1), torch.cat([v[:, :-1], rt(v[:, -1:])], 1)) for k, v in cache]
            rows.append(logits[-1].clone())
        return torch.stack(rows), toks
    la, toks = run(ident, None)
    lb, _ = run(roundtrip_kv_rows, toks)
    return la, lb


def gpu_side(cfg, ids, steps):
    from usdm_amd.llm import USDMForCausalLM
    dev = torch.device("cuda:0")
    sd = MO.random_state_dict(cfg, seed=0)
    out = {}
    forced = None
    for kind in ("bf16", "fp8"):
        m = USDMForCausalLM.from_state_dict(sd, cfg, dev, ctx_max=256, kv_cache_dtype=kind)
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
    return out["bf16"], out["fp8"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=32)
    a = ap.parse_args()
    cfg = dict(MO.MISTRAL_7B_USDM, num_hidden_layers=a.layers)
    ids = torch.randint(0, cfg["vocab_size"], (a.prompt,), generator=torch.Generator().manual_seed(7))
    la, lb = (cpu_side if a.side == "cpu" else gpu_side)(cfg, ids, a.steps)
    summarize(a.side, la, lb, dict(layers=a.layers, prompt=a.prompt))


if __name__ == "__main__":
    main()
