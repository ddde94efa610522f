"""The KV-quantized CPU reference of kv_cache_dtype="fp8": the plain oracle (oracle.mistral_oracle.forward, which hands its cache
to the caller) reading round-tripped cache rows.  Prefill runs on the plain oracle (the prompt attends to its unquantized K / V);
then every cached row is round-tripped through the fp8 format, and after each decode step the row that step appended (the step
itself saw its own K / V unquantized, as the kernels take them from LDS)."""
import torch

from oracle import mistral_oracle as MO
from usdm_amd.quant import roundtrip_kv_rows


def kv8_greedy_generate(sd, cfg, ids, max_new_tokens, bad_words_ids=None, eos_token_id=None, return_logits=False, roundtrip=roundtrip_kv_rows):
    """MO.greedy_generate with an fp8 KV cache.  roundtrip: [Hkv, T, d] -> [Hkv, T, d]; the identity gives the plain oracle."""
    ban = MO.ban_mask(cfg["vocab_size"], bad_words_ids)
    out = list(ids.tolist())
    logits, cache = MO.forward(sd, cfg, ids)
    cache = [(roundtrip(k), roundtrip(v)) for k, v in cache]
    all_logits = []
    for _ in range(max_new_tokens):
        last = logits[-1].clone()
        last[ban] = -float("inf")
        all_logits.append(last)
        tok = int(torch.argmax(last))
        out.append(tok)
        if eos_token_id is not None and tok == eos_token_id:
            break
        logits, cache = MO.forward(sd, cfg, torch.tensor([tok]), cache)
        cache = [(torch.cat([k[:, :-1], roundtrip(k[:, -1:])], 1), torch.cat([v[:, :-1], roundtrip(v[:, -1:])], 1)) for k, v in cache]
    return (out, torch.stack(all_logits)) if return_logits else out


def near_ties(ref_logits):
    """indices of the steps whose top-2 gap lies inside tests/_greedy_compare's near-tie band"""
    from tests._greedy_compare import NEAR_TIE_ABS, NEAR_TIE_REL
    bad = []
    for j, lg in enumerate(ref_logits):
        t = torch.topk(lg, 2).values
        if (t[0] - t[1]).item() <= NEAR_TIE_REL * t[0].abs().item() + NEAR_TIE_ABS:
            bad.append(j)
    return bad


# the prompts / seeds of the oracle comparison in tests/test_kv8_gpu.py (checked for near-ties on the CPU in test_kv8_quant_cpu.py)
ORACLE_SMALL = dict(sd_seed=77, prompt_seed=6, n=16, new=20, bad=[[i] for i in range(0, 300)])


def small_oracle_prompts():
    gen = torch.Generator().manual_seed(ORACLE_SMALL["prompt_seed"])
    return [torch.randint(0, 1000, (int(L),), generator=gen) for L in torch.randint(12, 60, (ORACLE_SMALL["n"],), generator=gen)]


def wprime(sd):
    """the state dict with every streamed matrix replaced by its dequantized FP8 form W' (quantization="fp8" is exactly that model)"""
    from usdm_amd.quant import dequantize_rows, quantize_rows
    proj = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight" or any(p in k for p in proj):
            out[k] = dequantize_rows(*quantize_rows(v.to(torch.bfloat16)))
    return out
