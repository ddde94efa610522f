"""Mistral-7B speech-text LLM on MI355X: drop-in for the object the reference obtains from
`AutoModelForCausalLM.from_pretrained('naver-ai/USDM-DailyTalk', torch_dtype=bf16)` (src/inference.py:116-124)
as far as the hot path uses it: `.generate(input_ids=[1,L], max_length, do_sample, bad_words_ids, top_p, top_k,
temperature, eos_token_id) -> LongTensor[1,L']` (src/inference.py:63-83).

Host side: Python plans of C-ABI launches (libusdm_hip.so).
  prefill : usdm_embed_rows, usdm_norm(rms), usdm_gemm (MFMA bf16; SwiGLU / residual epilogues), usdm_rope_cache,
            usdm_attention(mode 1, causal GQA)                                   — one eager plan per prompt length
  decode  : usdm_gemv x4 per layer (RMSNorm, residual add, SwiGLU fused), usdm_attn_decode, lm_head GEMV with
            ban-mask + arg-max, all state on the device -> ONE hipGraph replayed per token
  TP > 1  : Megatron-style shards (q/k/v heads, MLP columns, vocab rows).  Decode: the all-reduce of the o_proj/down_proj
            partial sums is fused into those GEMVs' epilogues as a one-shot peer-to-peer exchange over xGMI
            (usdm_amd.p2p.P2PComm; the decode step stays ONE hipGraph with no collective launch), the vocab-parallel token
            pick likewise (usdm_argmax_p2p).  Prefill (4 MB messages) and the validation path use RCCL through
            torch.distributed ('nccl'): f32 partial sums all-reduced, arg-max partials all-gathered.  Sampling gathers the
            full logits row on every rank (usdm_logits_p2p in the P2P step) and draws from it with rank 0's seed.
Weights: HF state-dict key names (model.layers.N.self_attn.q_proj.weight, ...), bf16.  quantization="fp8" (opt-in): the streamed
matrices (qkv, o, gate/up, down, lm_head) are held as e4m3 with a power-of-two scale per row (usdm_amd/quant.py), which makes the
model exactly the bf16 model with the dequantized weights W'; decode streams half the bytes (usdm_gemv_fp8), prefill dequantizes
each matrix into one bf16 scratch right before its usdm_gemm.  Single GPU only.  quantization="mxfp4" (opt-in): the layers' matrices
as OCP MXFP4 (e2m1, one power-of-two scale per 32 elements; 4.25 bits per weight, about 11.5 % relative weight error), the lm_head
fp8; the same contract and the same structure (usdm_gemv_mxfp4, usdm_dequant_mxfp4), at most 4 sequences per decode step
unless mxfp4_matrix_cores=True (opt-in): a second image of the layers' codes, and steps of 5..16 sequences on usdm_gemv_mxfp4_mfma.
KV cache: bf16 rows.  kv_cache_dtype="fp8" (opt-in, independent of `quantization`): every cached row (one token, one kv head) is
held as e4m3 bytes + one power-of-two exponent (quant.quantize_kv_rows), written by usdm_rope_cache_fp8 / usdm_attn_decode_fp8.
The model is then exactly the bf16-cache model whose decode steps read the round-tripped rows K', V'; a prompt's own prefill
attention reads its unquantized K / V from per-plan scratch.  Half the cache bytes per step and per slot; no prefix reuse unless
enable_prefix_caching asks for it; single GPU.
Prefix caching: enable_prefix_caching=True (opt-in; vLLM's keyword): a prompt admitted into a batch slot (generate_batch, serving.LLM,
n > 1) reuses the prefill-written rows of the longest prefix any slot holds (usdm_amd/prefix.py; usdm_kv_reorder copies them between
slots, usdm_kv_expand puts them into the prefill plan's scratch), bit-identical with the option off on a bf16 cache; an fp8-cache model
then reuses its prefix on the single sequence too, reading the reused rows as the cache holds them.
"""
import math
import os
import time
from collections import namedtuple

import torch

from . import ops
from ._lib import ACT_SWIGLU, UsdmError
from .graph import GraphedPlan, GraphedSegments
from .plancache import LRU
from .prefix import reusable_past
from .quant import Fp8Weight, Mxfp4Weight, check_kv_cache_dtype
from .wpack import PackedWeight
from .slots import (CHUNK, NO_CANDIDATE_IDX, BeamSlots, DecodeSlots, SpecSequence, SpecSlots, TokenLogprobs, edit_buffers, logprob_buffers,
                    penalty_buffers, read_logprobs, seed_edits, seed_penalties, stop_block, stop_index)

MISTRAL_7B_USDM = dict(vocab_size=42003, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
                       num_attention_heads=32, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5,
                       rope_theta=10000.0, max_position_embeddings=32768)


def _pack_gate_up(gate, up):
    """[I,K] gate and up -> [2I,K] in blocks of 32 rows = 16 gate + 16 up (SwiGLU epilogue layout)."""
    I, K = gate.shape
    return torch.stack([gate.reshape(I // 16, 16, K), up.reshape(I // 16, 16, K)], 1).reshape(2 * I, K).contiguous()


def vocab_shard(V, rank, tp):
    """Vocab-parallel lm_head layout: (Vloc, v0, v1, nparts).  Every rank owns Vloc = ceil(V/tp) row SLOTS (the last rank
    fewer real rows: 42 003 / 8 -> 7 x 5251 + 5246) and nparts = usdm_gemv_nblocks(Vloc) arg-max partial slots, so the
    partial buffers that are exchanged have the SAME size on every rank (a collective with per-rank counts that differ is
    undefined behaviour in RCCL); unused slots keep their (-inf, 0x7fffffff) fill and can never win."""
    Vloc = (V + tp - 1) // tp
    v0 = min(V, rank * Vloc)
    v1 = min(V, v0 + Vloc)
    return Vloc, v0, v1, ops.gemv_nblocks(Vloc)


def agree_seed(seed, group, rank, device=None):
    """Rank 0's value of `seed`, on every rank of a tensor-parallel group: one 8-byte all-gather that every rank must reach.
    Ranks draw a seed from their own torch generator when the caller gives none; sampled tokens, and with them the device-side
    EOS and the number of steps (hence the collectives), only agree across ranks if the Philox streams do.  Transport as the
    model's other gathers: InProcessGroup (threaded: a lockstep group completes a gather only at its last rank), host-staged
    on gloo, RCCL otherwise."""
    import torch.distributed as dist
    if hasattr(group, "usdm_all_gather"):
        src = torch.tensor([int(seed)], dtype=torch.int64, device=device)
        dst = torch.zeros(group.world, dtype=torch.int64, device=device)
        group.usdm_all_gather(rank, [dst], [src])
    elif dist.get_backend(group) == "gloo":
        dst = torch.zeros(dist.get_world_size(group), dtype=torch.int64)
        dist.all_gather_into_tensor(dst, torch.tensor([int(seed)], dtype=torch.int64), group=group)
    else:
        dst = torch.zeros(dist.get_world_size(group), dtype=torch.int64, device=device)
        dist.all_gather_into_tensor(dst, torch.tensor([int(seed)], dtype=torch.int64, device=device), group=group)
    return int(dst[0].item())


QUANT_KEYS = ("qkv", "o", "gu", "down")    # the streamed matrices of a layer (quantization="fp8"; with the lm_head shard)


QUANTIZATIONS = (None, "fp8", "mxfp4")


def check_quantization(quantization, fp8_matrix_cores, mxfp4_matrix_cores=False):
    """The values of the weight-format arguments (USDMForCausalLM and serving.LLM take them)."""
    if quantization not in QUANTIZATIONS:
        raise ValueError(f"quantization={quantization!r}: supported are None (bf16), 'fp8' (e4m3 weights, power-of-two row scales) "
                         "and 'mxfp4' (e2m1 weights, one power-of-two scale per 32 elements; the lm_head stays fp8)")
    if fp8_matrix_cores and quantization != "fp8":
        raise ValueError("fp8_matrix_cores=True needs quantization='fp8'")
    if mxfp4_matrix_cores and quantization != "mxfp4":
        raise ValueError("mxfp4_matrix_cores=True needs quantization='mxfp4'")


def stop_ids(eos_token_id):
    """generate()'s eos_token_id (None, an id or a list of ids) as a set."""
    if eos_token_id is None:
        return set()
    return set(eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])


def check_logprobs(logprobs):
    """generate()'s / SamplingParams' logprobs: None (off) or the number K of most likely ids reported per token, 0 .. 20 (vLLM's
    cap; 0 = the picked token only)."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or not isinstance(logprobs, int) or not 0 <= logprobs <= ops.LOGPROBS_MAX_K:
        raise ValueError(f"logprobs must be None or an integer 0 .. {ops.LOGPROBS_MAX_K}, got {logprobs!r}")
    return logprobs


def check_penalties(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """generate()'s / SamplingParams' penalty knobs -> None when all are neutral (no penalty plan is built), else the tuple
    (repetition, frequency, presence) in usdm_penalty_params' order.  Ranges as vLLM's: repetition in (0, 2], the other two in
    [-2, 2]; anything else, NaN included, is a ValueError (the library's own check: usdm_penalty_params_init)."""
    p = ops.penalty_params(repetition_penalty, frequency_penalty, presence_penalty)
    knobs = (p.repetition, p.frequency, p.presence)
    return None if knobs == ops.PENALTY_NEUTRAL else knobs


def check_min_p(min_p):
    """generate()'s / SamplingParams' min_p (HF MinPLogitsWarper, vLLM): a number in [0, 1], 0 = off."""
    try:
        v = float(min_p)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(min_p, bool) or not 0.0 <= v <= 1.0:
        raise ValueError(f"min_p must be a number in [0, 1] (0 = off), got {min_p!r}")
    return v


LOGIT_BIAS_CLAMP = 100.0      # vLLM's and OpenAI's range of a logit_bias value


def check_edits(logit_bias=None, no_repeat_ngram_size=0, vocab=None):
    """generate()'s / SamplingParams' logit_bias and no_repeat_ngram_size -> None when both are neutral (no edit plan is built), else
    (bias, n): bias a tuple of (id, value) pairs in ascending id order, the values clamped to [-100, 100] (vLLM's and OpenAI's
    range), n the n-gram size (0 = off).  logit_bias: None or a dict of at most 1024 integer ids in [0, vocab) (vocab=None: the
    caller does not know it yet, >= 0) to finite numbers; no_repeat_ngram_size: None or an integer >= 0.  Anything else is a
    ValueError."""
    n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"no_repeat_ngram_size must be None or an integer >= 0, got {no_repeat_ngram_size!r}")
    if logit_bias is None:
        logit_bias = {}
    if not isinstance(logit_bias, dict):
        raise ValueError(f"logit_bias must be None or a dict {{token id: bias}}, got {type(logit_bias).__name__}")
    if len(logit_bias) > ops.LOGIT_BIAS_MAX:
        raise ValueError(f"logit_bias holds {len(logit_bias)} entries, at most {ops.LOGIT_BIAS_MAX} are supported")
    bias = []
    for i, v in logit_bias.items():
        if isinstance(i, bool) or not isinstance(i, int) or i < 0 or (vocab is not None and i >= vocab):
            raise ValueError(f"logit_bias: token id {i!r} is not an integer in [0, {'vocab' if vocab is None else vocab})")
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if isinstance(v, bool) or not math.isfinite(f):
            raise ValueError(f"logit_bias: the bias of token {i} must be a finite number, got {v!r}")
        bias.append((i, max(-LOGIT_BIAS_CLAMP, min(LOGIT_BIAS_CLAMP, f))))
    return (tuple(sorted(bias)), n) if (bias or n) else None


def _per_sequence(value, n):
    """A generate_batch knob: one value (a number, a dict, None) for all n sequences, or a list with one per sequence."""
    per = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(per) != n:
        raise ValueError("a sampling knob is one value for all sequences or a list with one value per sequence")
    return per


StepKind = namedtuple("StepKind", "sampling logprobs penalties edits", defaults=(False,))


def step_kind(sampling=None, logprobs=None, penalties=False, edits=False):
    """Which variant of a step (the prefill's pick, the decode step) runs: the key of every cache of built plans, in the builders'
    argument order.  sampling: False = the ban-masked arg-max, True = usdm_sample_final, "hook" = Python logits processors in front
    of it; logprobs: None or K; penalties: whether usdm_penalize runs; edits: whether usdm_logit_edit (logit bias, n-gram ban) runs.
    Log-probabilities, penalties and edits work on the logits row, which only the sampling step materialises, so each turns a greedy
    step into the sampling step (run with top_k = 1: the same ids)."""
    sampling = "hook" if sampling == "hook" else bool(sampling)
    return StepKind(sampling or logprobs is not None or bool(penalties) or bool(edits), logprobs, bool(penalties), bool(edits))


class _Segments:
    """A plan under construction as the list of its segments: launches are added to .plan; cut() ends that plan, with a host call
    to run after it (a collective, the logits hook) or without (the boundary between a peer-to-peer put and its get), and starts
    the next one."""

    def __init__(self):
        self.segs, self.plan = [], ops.Plan()

    def cut(self, host_call=None):
        self.segs.append(self.plan)
        if host_call is not None:
            self.segs.append(host_call)
        self.plan = ops.Plan()

    def finish(self):
        """The segments; the first one holds every tensor any of them keeps."""
        self.segs.append(self.plan)
        self.segs[0].hold(*[t for s in self.segs if isinstance(s, ops.Plan) for t in s.keep])
        return self.segs


def shard_weights(sd_get, cfg, rank, tp, device, dtype=torch.bfloat16, quantization=None, mxfp4_matrix_cores=False):
    """This rank's packed weights for tensor parallelism of degree `tp` (Megatron-style): q/k/v heads and MLP
    columns split by rank, o_proj/down_proj split along K (their outputs are partial sums), vocab rows split.
    quantization="fp8": every streamed matrix becomes a quant.Fp8Weight as soon as its layer is packed (rows quantized after the
    qkv concatenation and the gate/up packing; per-row scales do not depend on the row order), so at most one layer is ever held
    in bf16 next to the FP8 copy.  The embedding stays bf16, the norms f32.
    quantization="mxfp4": likewise with quant.Mxfp4Weight for qkv, o, gate/up and down (blocks of 32 run along K, so the row packing
    only permutes rows of blocks); the lm_head shard is an Fp8Weight.  mxfp4_matrix_cores: every Mxfp4Weight also holds its
    matrix-core image (usdm_gemv_mxfp4_mfma), packed from the same codes."""
    qz = {"fp8": Fp8Weight.from_matrix, "mxfp4": lambda t: Mxfp4Weight.from_matrix(t, matrix_cores=mxfp4_matrix_cores)}.get(quantization, lambda t: t)
    qz_head = Fp8Weight.from_matrix if quantization in ("fp8", "mxfp4") else (lambda t: t)
    d = cfg["head_dim"]
    Hq, Hkv, I = cfg["num_attention_heads"] // tp, cfg["num_key_value_heads"] // tp, cfg["intermediate_size"] // tp
    V = cfg["vocab_size"]
    _, v0, v1, _ = vocab_shard(V, rank, tp)
    g = lambda n: sd_get(n).to(device, dtype)
    f = lambda n: sd_get(n).to(device, torch.float32).contiguous()
    W = {"embed": g("model.embed_tokens.weight").contiguous(), "norm": f("model.norm.weight"),
         "lm_head": qz_head(g("lm_head.weight")[v0:v1].contiguous()), "layers": [], "v0": v0, "v1": v1}
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{l}."
        q = g(p + "self_attn.q_proj.weight")[rank * Hq * d:(rank + 1) * Hq * d]
        k = g(p + "self_attn.k_proj.weight")[rank * Hkv * d:(rank + 1) * Hkv * d]
        v = g(p + "self_attn.v_proj.weight")[rank * Hkv * d:(rank + 1) * Hkv * d]
        o = g(p + "self_attn.o_proj.weight")[:, rank * Hq * d:(rank + 1) * Hq * d]
        ga = g(p + "mlp.gate_proj.weight")[rank * I:(rank + 1) * I]
        up = g(p + "mlp.up_proj.weight")[rank * I:(rank + 1) * I]
        dn = g(p + "mlp.down_proj.weight")[:, rank * I:(rank + 1) * I]
        W["layers"].append(dict(qkv=qz(torch.cat([q, k, v], 0).contiguous()), o=qz(o.contiguous()), gu=qz(_pack_gate_up(ga, up)),
                                down=qz(dn.contiguous()), ln1=f(p + "input_layernorm.weight"),
                                ln2=f(p + "post_attention_layernorm.weight")))
        del q, k, v, o, ga, up, dn
    return W


class USDMForCausalLM:
    def __init__(self, cfg, device, ctx_max=2048, tp_rank=0, tp_size=1, group=None, decode_splits=None, tp_segments=None, p2p=None,
                 p2p_fused=None, quantization=None, fp8_matrix_cores=False, kv_cache_dtype=None, score_rows=256,
                 enable_prefix_caching=False, weight_packing=None, mxfp4_matrix_cores=False):
        check_quantization(quantization, fp8_matrix_cores, mxfp4_matrix_cores)
        # weight_packing (default on; USDM_WPACK=0 or False turns it off for A/B runs): the single-sequence decode step streams
        # down_proj and gate/up from lossless 13-bit images of their bf16 weights (usdm_amd/wpack.py; identical bits, 13/16 of the
        # bytes).  One GPU, plain bf16 weights and the 7B's MLP shapes only; the images are built at load, beside the bf16 matrices.
        # USDM_WPACK_GU=0: down_proj only (A/B runs of the gate/up image).
        self.weight_packing = (os.environ.get("USDM_WPACK", "1") != "0") if weight_packing is None else bool(weight_packing)
        self.weight_packing_gu = self.weight_packing and os.environ.get("USDM_WPACK_GU", "1") != "0"
        self.wpack_report = None
        # enable_prefix_caching (vLLM's name; opt-in): batch slots reuse cached prompt rows (usdm_amd/prefix.py), and an
        # fp8-cache model reuses its prefix on the single sequence too.  Off: no index, no buffer and no plan of it is built.
        self.prefix_caching = bool(enable_prefix_caching)
        if self.prefix_caching:
            if tp_size > 1 or tp_segments or p2p is not None:
                raise NotImplementedError("enable_prefix_caching runs on one GPU: tensor parallelism (tp_size > 1, tp_segments, p2p) is not supported")
            if os.environ.get("USDM_PREFIX_REUSE", "exact") in ("0", "off"):
                raise ValueError("enable_prefix_caching=True contradicts USDM_PREFIX_REUSE=0 (prefix reuse switched off)")
        # score(): prompt rows per lm_head GEMM + usdm_prompt_logprobs launch.  256 is reasoned, not measured: one 1024-thread workgroup per
        # row is about one round of the 256 CUs, and a 256 x 42003 x 4 B = 43 MB chunk should stay cache-resident between the GEMM's write
        # and the kernel's 2 - 9 read passes (tools/score_rate.py sweeps it)
        if isinstance(score_rows, bool) or not isinstance(score_rows, int) or score_rows < 16 or score_rows % 16:
            raise ValueError(f"score_rows must be a positive multiple of 16, got {score_rows!r}")
        self.score_rows = score_rows
        if quantization is not None and (tp_size > 1 or tp_segments or p2p is not None):
            raise NotImplementedError(f"quantization={quantization!r} runs on one GPU: tensor parallelism (tp_size > 1, tp_segments, p2p) takes bf16 weights")
        self.kv_cache_dtype = check_kv_cache_dtype(kv_cache_dtype)
        self.kv8 = self.kv_cache_dtype == "fp8"
        if self.kv8 and (tp_size > 1 or tp_segments or p2p is not None):
            raise NotImplementedError("kv_cache_dtype='fp8' runs on one GPU: tensor parallelism (tp_size > 1, tp_segments, p2p) takes a bf16 cache")
        if self.kv8 and os.environ.get("USDM_GEMV_CHAIN", "0") not in ("", "0"):
            raise NotImplementedError("kv_cache_dtype='fp8': the chained decode GEMVs (USDM_GEMV_CHAIN) take a bf16 cache")
        self.quantization = quantization
        # fp8_matrix_cores (opt-in): decode steps of 5..16 sequences on the matrix cores (usdm_gemv_fp8_mfma) instead of groups of 4;
        # like bf16's matrix-core form they equal the oracle up to near-ties, not generate() bit for bit
        self.fp8_matrix_cores = bool(fp8_matrix_cores)
        # mxfp4_matrix_cores (opt-in): likewise for mxfp4 (usdm_gemv_mxfp4_mfma); the layers' matrices then hold a second, matrix-core
        # image of their codes (about as many bytes again)
        self.mxfp4_matrix_cores = bool(mxfp4_matrix_cores)
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("USDMForCausalLM (usdm_amd) runs on the MI355X only; there is no CPU fallback")
        c = self.cfg
        if c["head_dim"] != 128:
            raise NotImplementedError("decode/prefill attention kernels are built for head_dim 128 (Mistral-7B)")
        self.tp_rank, self.tp_size, self.group = tp_rank, tp_size, group
        # tp_segments: run the tensor-parallel code path (f32 partial sums + all-reduce + residual-add kernels) even at
        # tp_size 1 — used to exercise that path on a single GPU
        self.tp_path = (tp_size > 1) if tp_segments is None else bool(tp_segments)
        # p2p: a committed usdm_amd.p2p.P2PComm -> the decode step exchanges its partial sums peer to peer inside the GEMV
        # epilogues (p2p_fused, default) or through put + usdm_allreduce_p2p_reduce launches (split form, USDM_P2P_FUSED=0)
        self.p2p = p2p
        self.p2p_fused = (os.environ.get("USDM_P2P_FUSED", "1") == "1") if p2p_fused is None else bool(p2p_fused)
        if p2p is not None:
            if not self.tp_path:
                raise ValueError("p2p needs the tensor-parallel path (tp_size > 1 or tp_segments=True)")
            if (p2p.rank, p2p.world) != (tp_rank, tp_size) and os.environ.get("USDM_P2P_PROXY") != "1":   # (tools/tp8_proxy.py)
                raise ValueError(f"P2PComm is rank {p2p.rank}/{p2p.world}, the model shard is rank {tp_rank}/{tp_size}")
            if p2p.n_sites < 2 * c["num_hidden_layers"] + 1 or p2p.max_elems < c["hidden_size"]:
                raise ValueError("P2PComm too small: needs 2*layers+1 sites of hidden_size elements")
        self.Hq, self.Hkv = c["num_attention_heads"] // tp_size, c["num_key_value_heads"] // tp_size
        if self.Hq * tp_size != c["num_attention_heads"] or self.Hkv * tp_size != c["num_key_value_heads"] or self.Hkv < 1:
            raise ValueError("tp_size must divide both head counts")
        self.I = c["intermediate_size"] // tp_size
        if self.I * tp_size != c["intermediate_size"] or self.I % 16:
            raise ValueError("intermediate_size / tp_size must be a multiple of 16")
        V = c["vocab_size"]
        self.Vloc, self.v0, self.v1, self.nparts = vocab_shard(V, tp_rank, tp_size)
        self.ctx_max = (ctx_max + 63) // 64 * 64
        # Mistral-7B-v0.1 attends to the last `sliding_window` (4096) positions only (reference: src/model.py:337-371 keeps
        # W - 1 past keys + the new one; HF sliding-window mask: query p sees keys p-W+1 .. p).  The caches here keep every row up
        # to ctx_max and the attention kernels take the window as a key-range bound, so nothing changes while ctx_max <= W.
        W = c.get("sliding_window", 4096)
        self.window = int(W) if (W and self.ctx_max > int(W)) else 0
        # Decode attention is split over the context (NS workgroups per kv head).  The NS partials per head are merged in the
        # o_proj GEMV's x-staging prologue (usdm_gemv mrg_*; no combine launch) -> few, fat splits: every o_proj workgroup reads
        # all of them (NS x 16 KB from L2).  USDM_ATTN_MERGE_IN_OPROJ=0 restores the separate combine kernel (NS = 32).
        # Measured (profiles/r02_decode_ablation.txt) and OFF by default: on the single-GPU 7B shapes the merge costs the o_proj
        # launch more than the combine launch it removes (2.97 -> 3.10 ms/token at NS = 8: 128 KB of partials per workgroup and
        # two dependent L2 round trips no longer hide under the weight ring; NS = 32: 3.28), and the fewer, fatter splits it
        # wants make the latency-bound split kernel slower (rank-0-of-8 proxy: 1.10 -> 1.23 ms/token).  USDM_ATTN_MERGE_IN_OPROJ=1
        # enables it.
        self.merge_in_oproj = os.environ.get("USDM_ATTN_MERGE_IN_OPROJ", "0") == "1"
        # Hand-off form (round 3, usdm_gemv cmb_gran; the DEFAULT since round 4): no combine launch either, but the merge is done ONCE
        # per head by the o_proj launch's first 32 workgroups and handed to the others as granules, under the launch's first weight
        # ring.  Single-GPU 7B shape only (4096 outputs = one 16-wave workgroup per CU).  -0.8 % per token, token- and logit-identical
        # (profiles/r03_decode_ablation.txt 5, tests/test_fullsize_gpu.py).  The o_proj launch then carries the merge (7.7 -> 9.3 us);
        # bench.py's roofline object reports that launch both ways.  USDM_ATTN_CMB=0 restores the separate combine kernel.
        self.cmb = (os.environ.get("USDM_ATTN_CMB", "1") == "1" and tp_size == 1 and not self.tp_path and not self.merge_in_oproj
                    and c["hidden_size"] == 4096 and self.Hq * c["head_dim"] == 4096)
        dflt = max(8, -(-self.ctx_max // 512)) if self.merge_in_oproj else 32
        self.NS = int(os.environ.get("USDM_DECODE_SPLITS", str(dflt))) if decode_splits is None else decode_splits
        if self.kv8 and self.NS == 1:
            # usdm_attn_decode_fp8 has the split form only: the fewest splits the 512-keys-per-split bound allows
            self.NS = max(2, -(-(self.window or self.ctx_max) // 512))
        if self.NS == 1:
            self.merge_in_oproj = False          # one workgroup per kv head: nothing to merge
        # Chained decode GEMVs (usdm_gemv_chain): consecutive projections of a layer in ONE persistent launch whose weight stream
        # runs across the phase boundaries.  0 = off (one launch per projection; the DEFAULT: measured slower, see below),
        # 3 = o_proj -> gate/up -> down_proj, 4 = ... -> the next layer's qkv as well.  Single-GPU path only (the kernel needs the
        # whole GPU resident).  Measured (profiles/r02_decode_ablation.txt section 3): 85 vs 69 us per layer for 3 phases - a flat
        # counter grid barrier at 2 workgroups per CU costs ~13 us, more than the launch boundary + ramp it replaces, and one
        # workgroup shape for every phase streams 10-25 % slower than the per-shape tuned kernels.
        # "e3" / "e4": the same chains on the loader / consumer engine (usdm_gemv_engine: LDS-DMA weight ring, granule hand-offs).
        mode = os.environ.get("USDM_GEMV_CHAIN", "0")
        self.chain_engine = mode.startswith("e")
        self.chain = int(mode.lstrip("e") or 0)
        if self.tp_path or c["hidden_size"] != 4096:
            self.chain = 0
        if quantization is not None:
            # the FP8 / MXFP4 GEMVs have the plain forms only (usdm_gemv_fp8, usdm_gemv_mxfp4): the attention partials are combined by their own launch
            # (bit-identical with the hand-off form) and every projection is its own launch
            self.cmb = self.merge_in_oproj = False
            self.chain = 0
        self.chain_sync = None
        # decode attention of a step of more than 4 sequences (tools/batch_rate.py A/B): workgroup target of the context split, and
        # the merge by the last-arriving workgroup of a kv head instead of the combine launch
        self.batch_attn_wgs, self.batch_fused_merge = 512, False
        self.W = None
        # bounded caches (plancache.LRU): prefill plans are keyed by exact prompt length (a plan is argument structs + ~60 KB of
        # workspace per token; no hipGraph), decode plans / graphs by {greedy, sampling} only
        self._prefill_plans = LRU(24)
        self._decode = None
        self._decodes = {}
        self._batches = {}
        self._beams = {}          # beam search: the slots.BeamSlots (buffers, prefill plans, step) of (num_beams, n_eos), built at first use
        self.last_beam_scores = None   # generate(num_beams > 1): HF's sequences_scores of the returned sequences (float32 tensor [n])
        self.last_beam_rows, self.last_beam_replay = None, None   # ... its recorded logits rows (tests: _beam_keep_rows) and its beam.BeamReplay
        self._ban_cache = LRU(8)
        self.stats = {}
        self.logits_hook = None   # generate(_logits_hook=f): f() runs between the lm_head launch and the sampling pick of every step
        self.keep_logits = False  # debug/tests: keep the fp32 (bf16-valued) logits of the last step
        self.last_logits = None
        self._lp = None           # log-probability rows of the single sequence (logprob_buffers; allocated at first use)
        self.last_logprobs = None  # generate(logprobs=K): TokenLogprobs of the last call (generate_batch: a list); None when not asked
        self._pen = None          # penalty state of the single sequence (penalty_buffers; allocated at first use)
        self._edt = None          # logit-edit state of the single sequence (edit_buffers; allocated at first use)
        # speculative greedy decoding: the single sequence's slots.SpecSequence - the device words of usdm_spec_commit,
        # the rows, plan and graph per T - built at first use; generate(num_speculative_tokens=None / 0) touches none of it
        self._spec = None
        self._spec_batches = {}        # B -> slots.SpecSlots: generate_batch(num_speculative_tokens=k), serving
        self.last_spec_stats = None    # generate(num_speculative_tokens=k): dict(steps=, drafted=, accepted=) of the last call
        # usdm_attn_verify's keys per split: a plan constant (fixed absolute key ranges).  Reasoned, not measured: 128 keys x 2 x 256 B
        # = 64 KB per workgroup, 5 .. 28 splits x 8 kv heads over the 600 .. 3 500 rows of an utterance, at most one per CU; 256 where
        # ctx_max / 128 would exceed the 64 splits the merge takes
        self.spec_split = int(os.environ.get("USDM_SPEC_SPLIT", 128 if self.ctx_max <= 64 * 128 else 256))
        # score(): plans keyed (S, past, j0, K) in a cache of their own (scoring never evicts generate()'s prefill plans), the output
        # rows [ctx_max] / [ctx_max][20] and the bf16 copy of a quantized lm_head, all allocated at first use
        self._score_plans = LRU(8)
        self._score_out = None
        self._head_bf16 = None
        self.keep_score_logits = False   # debug/tests: keep the fp32 (bf16-valued) logits of every scored row
        self.last_score_logits = None    # ... of the last score() call: [rows scored][V] (tensor parallel: the gathered logical rows)

    # ------------------------------------------------------------------ weights
    def _shard(self, sd_get):
        """Build this rank's packed weights from a getter name -> tensor (any device)."""
        W = shard_weights(sd_get, self.cfg, self.tp_rank, self.tp_size, self.device, quantization=self.quantization,
                          mxfp4_matrix_cores=self.mxfp4_matrix_cores)
        assert (W["v0"], W["v1"]) == (self.v0, self.v1)
        return W

    @classmethod
    def from_state_dict(cls, sd, cfg, device, **kw):
        m = cls(cfg, device, **kw)
        m.W = m._shard(lambda n: sd[n])
        m._alloc()
        return m

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, device="cuda", cache_dir=None, torch_dtype=torch.bfloat16, **kw):
        """Load an HF-format Mistral checkpoint directory (config.json + [sharded] safetensors or .bin), as the reference does
        with AutoModelForCausalLM.from_pretrained('naver-ai/USDM-DailyTalk', cache_dir=..., torch_dtype=bf16)
        (src/inference.py:116-123).  Hub names resolve inside cache_dir (no network).  Tensors stream from the memory-mapped
        shards to the GPU one at a time; a tensor-parallel rank slices its shard on the way (tp_rank / tp_size in **kw)."""
        from .checkpoints import TensorSource, read_mistral_config, resolve_local
        if torch_dtype != torch.bfloat16:
            raise NotImplementedError("the decode kernels stream bf16 weights (the reference loads torch_dtype=torch.bfloat16)")
        path = pretrained_model_name_or_path
        if not os.path.isdir(path):
            if cache_dir is None:
                raise FileNotFoundError(f"{path}: not a directory, and no cache_dir to resolve the hub name in (no network)")
            path = resolve_local(cache_dir, path, must_contain=("config.json",))
        for drop in ("attn_implementation", "device_map", "low_cpu_mem_usage"):     # the reference's HF-only knobs
            kw.pop(drop, None)
        cfg = read_mistral_config(path)
        m = cls(cfg, device, **kw)
        src = TensorSource(path)
        m.W = m._shard(src)
        m._alloc()
        m.name_or_path = path
        return m

    def to(self, device):
        """The reference calls .to(device) on the loaded model (inference.py:123); weights already live on the GPU."""
        if torch.device(device).type != "cuda":
            raise RuntimeError("USDMForCausalLM (usdm_amd) runs on the MI355X only; there is no CPU fallback")
        return self

    def eval(self):
        return self

    @classmethod
    def random_init(cls, cfg, device, seed=0, **kw):
        """Random weights generated shard-by-shard ON the device (synthetic benchmark weights;
        values differ from oracle.mistral_oracle.random_state_dict, which is CPU-generated)."""
        m = cls(cfg, device, **kw)
        c, d = m.cfg, m.cfg["head_dim"]
        H, I, V = c["hidden_size"], c["intermediate_size"], c["vocab_size"]
        gen = torch.Generator(device=m.device).manual_seed(seed)
        shapes = {"model.embed_tokens.weight": ((V, H), 1.0), "lm_head.weight": ((V, H), H ** -0.5)}
        for l in range(c["num_hidden_layers"]):
            p = f"model.layers.{l}."
            shapes.update({p + "self_attn.q_proj.weight": ((c["num_attention_heads"] * d, H), H ** -0.5),
                           p + "self_attn.k_proj.weight": ((c["num_key_value_heads"] * d, H), H ** -0.5),
                           p + "self_attn.v_proj.weight": ((c["num_key_value_heads"] * d, H), H ** -0.5),
                           p + "self_attn.o_proj.weight": ((H, c["num_attention_heads"] * d), H ** -0.5),
                           p + "mlp.gate_proj.weight": ((I, H), H ** -0.5), p + "mlp.up_proj.weight": ((I, H), H ** -0.5),
                           p + "mlp.down_proj.weight": ((H, I), I ** -0.5)})

        def get(n):
            if n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                return torch.ones(H, device=m.device)
            shape, sc = shapes[n]
            return (torch.randn(shape, device=m.device, dtype=torch.float32, generator=gen) * sc).to(torch.bfloat16)
        m.W = m._shard(get)
        m._alloc()
        return m

    def weight_bytes_per_token(self):
        """weight bytes a decode step must stream on this rank (layers + lm_head shard): bf16, e4m3 + row exponents with fp8, or packed e2m1
        codes + block scale bytes (and the fp8 lm_head) with mxfp4."""
        if self.quantization is not None:
            return sum(l[k].nbytes for l in self.W["layers"] for k in QUANT_KEYS) + self.W["lm_head"].nbytes
        n = sum(l[k].numel() for l in self.W["layers"] for k in ("qkv", "o", "gu", "down")) + self.W["lm_head"].numel()
        return 2 * n

    def kv_bytes_per_token_row(self):
        """K + V bytes a decode step reads per cached token of ONE sequence on this rank (all layers): bf16 rows, or e4m3 rows +
        one exponent byte each with kv_cache_dtype="fp8".  A step of B sequences streams the sum over them of this x context."""
        d = self.cfg["head_dim"]
        return 2 * self.cfg["num_hidden_layers"] * self.Hkv * ((d + 1) if self.kv8 else 2 * d)

    def _pack_weights(self):
        """The 13-bit images of the layers' down_proj matrices (weight_packing; the conditions: one GPU, plain bf16 weights, the
        7B's shape N 4096 / K 14336 - where usdm_gemv has the straight-line form) and, under the same conditions and unless
        USDM_WPACK_GU=0, of their interleaved gate/up matrices (N 28672 / K 4096).  Each image verifies its own round trip
        (wpack.PackedWeight.from_matrix raises otherwise).  wpack_report: per down_proj matrix the share of marked rows, the extra
        device memory and the time the packing took; the gu_* keys say the same of the gate/up images (marked OUTPUTS: a gate or an
        up row marked), the other keys keep their down_proj-only meaning."""
        self.wpack_down = self.wpack_gu = None
        if not (self.weight_packing and self.tp_size == 1 and not self.tp_path and self.p2p is None and self.quantization is None
                and self.cfg["hidden_size"] == 4096 and self.I == 14336):
            return
        t0 = time.perf_counter()
        self.wpack_down = [PackedWeight.from_matrix(w["down"]) for w in self.W["layers"]]
        torch.cuda.synchronize(self.device)
        self.wpack_report = {"down_marked_share": [p.marked_share for p in self.wpack_down],
                             "down_marked_rows": sum(len(p.marked_rows) for p in self.wpack_down),
                             "extra_bytes": sum(p.nbytes for p in self.wpack_down), "seconds": time.perf_counter() - t0}
        if self.weight_packing_gu:
            t0 = time.perf_counter()
            self.wpack_gu = [PackedWeight.from_matrix(w["gu"], glu=True) for w in self.W["layers"]]
            torch.cuda.synchronize(self.device)
            self.wpack_report.update({"gu_marked_outputs": [len(p.marked_outputs) for p in self.wpack_gu],
                                      "gu_extra_bytes": sum(p.nbytes for p in self.wpack_gu), "gu_seconds": time.perf_counter() - t0})

    # ------------------------------------------------------------------ buffers
    def _alloc(self):
        self._pack_weights()
        c, dev = self.cfg, self.device
        L, d = c["num_hidden_layers"], c["head_dim"]
        bf = torch.bfloat16
        if self.kv8:   # e4m3 rows + one exponent per (token, kv head); all-zero = rows of 0.0 (pad keys stay finite)
            self.kcache = torch.zeros(L, self.Hkv, self.ctx_max, d, dtype=torch.uint8, device=dev)
            self.vcache = torch.zeros(L, self.Hkv, self.ctx_max, d, dtype=torch.uint8, device=dev)
            self.kexp = torch.zeros(L, self.Hkv, self.ctx_max, dtype=torch.int8, device=dev)
            self.vexp = torch.zeros(L, self.Hkv, self.ctx_max, dtype=torch.int8, device=dev)
        else:
            self.kcache = torch.zeros(L, self.Hkv, self.ctx_max, d, dtype=bf, device=dev)
            self.vcache = torch.zeros(L, self.Hkv, self.ctx_max, d, dtype=bf, device=dev)
        # V^T of the prompt tokens (what the prefill attention consumes), kept across generate() calls so that a prompt which
        # extends the cached sequence only prefills its new tokens (the reference's three rounds: src/inference.py:61-83)
        # reuse_prefix = "exact" (default; USDM_PREFIX_REUSE=exact): only cache rows that a PREFILL launch wrote are reused.  A row of
        # the prefill path does not depend on how many tokens were prefilled with it (per-row GEMM and flash-attention arithmetic is
        # independent of the tile a row sits in), so the result is bit-identical with recomputing the whole prompt as the reference
        # does - checked on logits in tests/test_llm_gpu.py::test_exact_prefix_reuse_is_bit_identical.
        # reuse_prefix = True (USDM_PREFIX_REUSE=1): rows appended by decode steps are reused too; they come from the GEMV path and can
        # differ from a from-scratch prefill by a bf16 ulp (close to, not identical with, the reference).  False / 0: off.
        mode = os.environ.get("USDM_PREFIX_REUSE", "exact")
        self.reuse_prefix = {"0": False, "off": False, "1": True, "all": True}.get(mode, "exact")
        if self.kv8:
            # fp8 cache: no persistent V^T, and no reuse unless enable_prefix_caching asks for it.  A reused prefix is dequantized for the
            # prefill attention (usdm_kv_expand into the plan's scratch) and no longer equals a recomputed prompt, which attends to its
            # unquantized K / V: without the flag every call prefills its whole prompt.
            self.vtc = None
            if not self.prefix_caching:
                self.reuse_prefix = False
        else:
            self.vtc = torch.zeros(L, self.Hkv, d, self.ctx_max, dtype=bf, device=dev)
        self._kv_ids, self._vt_upto = None, 0
        # rope tables exactly as HF MistralRotaryEmbedding computes them (fp32 on the host, cast to bf16)
        inv_freq = 1.0 / (c["rope_theta"] ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
        fr = torch.arange(self.ctx_max).float()[:, None] * inv_freq[None, :]
        self.cos = fr.cos().to(bf).to(dev).contiguous()
        self.sin = fr.sin().to(bf).to(dev).contiguous()
        i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
        self.max_out = self.ctx_max
        self.st_next, self.st_step, self.st_pos = i32(1), i32(1), i32(1)
        self.st_out = i32(self.max_out)
        # device-side end of sequence: st_eos = {count, min_new, ids...}; st_done is set by the token-picking kernel and read by
        # every decode kernel as its skip word, so steps launched past an EOS inside a host chunk return immediately
        self.st_done, self.st_eos = i32(1), i32(8)
        self.sample_params = ops.sample_params_tensor(dev)   # usdm_sample_params of the current request
        self.ban_all_off = torch.zeros(self.v1 - self.v0, dtype=torch.uint8, device=dev)
        self.ban = torch.zeros(self.v1 - self.v0, dtype=torch.uint8, device=dev)  # live mask read by the graphs
        self.h_dec = torch.zeros(c["hidden_size"], dtype=bf, device=dev)  # residual stream of the decode step
        # usdm_gemv_chain sync blocks (generation, error, arrival counters): ONE PER CHAIN PATTERN - the counters of a block are
        # monotonic in lockstep with its generation, so launches with different phase counts must not share a block
        self.chain_sync = torch.zeros(2, 8, dtype=torch.int32, device=dev)
        self.chain_gran = torch.zeros(3 * 8192, dtype=torch.int64, device=dev)     # usdm_gemv_engine hand-off granules
        self.cmb_err = torch.zeros(1, dtype=torch.int32, device=dev) if self.cmb else None      # error word of the o_proj hand-off (usdm_gemv cmb_gran)
        # arg-max partials: nparts slots per rank, the same on every rank (vocab_shard); slots the lm_head launch does not
        # write (last rank's shorter shard) stay "no candidate"
        nv = lambda n: torch.full((n,), float("-inf"), dtype=torch.float32, device=dev)
        ni = lambda n: torch.full((n,), NO_CANDIDATE_IDX, dtype=torch.int32, device=dev)
        self.part_val, self.part_idx = nv(self.nparts * self.tp_size), ni(self.nparts * self.tp_size)
        self.part_val_loc = nv(self.nparts) if self.tp_path else self.part_val
        self.part_idx_loc = ni(self.nparts) if self.tp_path else self.part_idx
        # sampling under tensor parallelism: this rank's Vloc logits (the last rank's padding slots are never read) and the
        # gathered [tp * Vloc] row in global-id order (v0 = rank * Vloc) that every rank samples with the same seed and step
        if self.tp_path:
            self.logits_loc = torch.zeros(self.Vloc, dtype=torch.float32, device=dev)
            self.logits_row = torch.zeros(self.tp_size * self.Vloc, dtype=torch.float32, device=dev)
            self._shard_logits = None
        # fp8 / mxfp4: ONE bf16 scratch for the prefill GEMM operand, sized for the largest streamed matrix (7B: gate/up, 235 MB); each
        # matrix is dequantized into it right before its usdm_gemm (plans run their launches in order on one stream)
        self.dq_scratch = None
        if self.quantization is not None:
            mats = [l[k] for l in self.W["layers"] for k in QUANT_KEYS]
            self.dq_scratch = torch.empty(max(m.numel() for m in mats), dtype=bf, device=dev)

    def _gemm_w(self, W, plan):
        """The bf16 operand of a prefill usdm_gemm: the weight itself, or (fp8 / mxfp4) its dequantization into the shared scratch."""
        if not isinstance(W, (Fp8Weight, Mxfp4Weight)):
            return W
        out = self.dq_scratch[:W.N * W.K].view(W.N, W.K)
        (ops.dequant_mxfp4 if isinstance(W, Mxfp4Weight) else ops.dequant_fp8)(W, out, plan=plan)
        return out

    # ------------------------------------------------------------------ collectives (TP only)
    def _host_staged(self):
        """A gloo group (validation runs with several ranks on ONE GPU, where RCCL refuses to form a group): collectives are
        staged through host memory.  Never the production transport."""
        import torch.distributed as dist
        return dist.get_backend(self.group) == "gloo"

    def _all_reduce(self, t):
        import torch.distributed as dist
        if hasattr(self.group, "usdm_all_reduce"):      # in-process logical ranks (usdm_amd.p2p.InProcessGroup)
            return self.group.usdm_all_reduce(self.tp_rank, t)
        if self._host_staged():
            c = t.cpu()
            dist.all_reduce(c, group=self.group)
            t.copy_(c)
            return
        dist.all_reduce(t, group=self.group)

    def _gather_partials(self, dsts=None, srcs=None):
        """all-gather of the ranks' arg-max partials (rank-major: dst = concatenation of the ranks' src along dim 0).  Default: the
        single sequence's buffers; a batch slot / the batched step pass their own."""
        import torch.distributed as dist
        dsts = [self.part_val, self.part_idx] if dsts is None else dsts
        srcs = [self.part_val_loc, self.part_idx_loc] if srcs is None else srcs
        if hasattr(self.group, "usdm_all_gather"):
            return self.group.usdm_all_gather(self.tp_rank, dsts, srcs)
        if self._host_staged():
            for dst, src in zip(dsts, srcs):
                c = torch.empty(dst.shape, dtype=dst.dtype)
                dist.all_gather_into_tensor(c, src.cpu(), group=self.group)
                dst.copy_(c)
            return
        for dst, src in zip(dsts, srcs):
            dist.all_gather_into_tensor(dst, src, group=self.group)

    def _agree_seed(self, seed):
        """A seed drawn on this rank -> rank 0's (tensor-parallel path); unchanged on one GPU."""
        return agree_seed(seed, self.group, self.tp_rank, self.device) if self.tp_path else seed

    def _check_p2p_sampling(self):
        from .p2p import P2PComm
        need = P2PComm.sites_needed(self.cfg, self.tp_size, True, max_elems=self.p2p.max_elems)
        if self.p2p.n_sites < need:
            raise ValueError(f"sampling on a peer-to-peer model needs a P2PComm of {need} sites (2 * layers + 1 + ceil(Vloc / "
                             f"max_elems) for the logits exchange); this one has {self.p2p.n_sites}")

    def _p2p_exchange(self, rec, st, launch):
        """A peer-to-peer exchange launch: put + get in ONE launch (phase 0, p2p_fused), or the split form: put | get as two
        launches with a segment boundary between them."""
        if self.p2p_fused:
            return launch(0)
        launch(1)
        rec.plan.hold(st)
        rec.cut()
        launch(2)

    def _pick_state(self, kind):
        """What a step of this kind needs beyond the sampler's state, for the single sequence (allocated at first use)."""
        if kind.logprobs is not None and self._lp is None:
            self._lp = logprob_buffers(self.device, self.max_out)
        if kind.penalties and self._pen is None:
            self._pen = penalty_buffers(self.device, self.cfg["vocab_size"])
        if kind.edits and self._edt is None:
            self._edt = edit_buffers(self.device, self.ctx_max)

    def _lm_head_and_pick(self, rec, x, advance_pos, sampling=None, x_delta=None, slot=None, skip=None, batch_gemv=None, logprobs=None,
                          penalties=False, edits=False, beam=None):
        """lm_head GEMV + token choice, for the single sequence (slot=None), a batch slot's prefill, and the batched step
        (slot = the slots' "all" view, batch_gemv = its projection launcher).  sampling=None: ban-masked arg-max (the reference's
        top_k=1 path); sampling=True: usdm_sample_final over the ban-masked logits, knobs read from the device block sample_params
        (written per request by generate(): plans and graphs do not depend on temperature / top-k / top-p / seed).
        Under tensor parallelism the ranks' arg-max partials, or (sampled) their Vloc ban-masked logits, are gathered first - in the
        kernels on a peer-to-peer model, else through the group; the sampler then runs unchanged over the full row on every rank with
        the same seed and step: every rank draws the same token.
        logprobs=K (sampled picks only): usdm_logprobs right after the pick, on the row it drew from (after the hook: as the hook left
        it; tensor parallel: the gathered row, on every rank), into the sequence's / the slots' log-probability buffers.
        penalties (sampled picks only): usdm_penalize on the row the sampler will read, BEFORE the hook and the pick - it counts the
        previous step's token into the sequence's / the slots' table and applies the knobs of their device block (tensor parallel: on
        the gathered row, on every rank; the table holds global ids and is the same on all ranks, so every rank still draws the
        same token).  The hook, the log-probabilities and last_logits see the penalised row.
        edits (sampled picks only): usdm_logit_edit directly in front of usdm_penalize (HF's and vLLM's order: bias, then penalties) -
        the logit bias and the n-gram ban of the sequence's / the slots' edit state (tensor parallel: on the gathered row, on every
        rank, with global ids).  Everything after it sees the edited row.
        beam (a slots.BeamSlots; one GPU, no hook, no penalties, no edits, no log-probabilities): the pick is the beam
        search's (_beam_pick) over ALL rows of those slots - from the batched step (slot = their "all" view) with every row live,
        from the prompt's prefill into slot 0 (slot = that slot) with row 0 live."""
        c, H = self.cfg, self.cfg["hidden_size"]
        for what, asked in (("log-probabilities", logprobs is not None), ("penalties", penalties), ("logit edits", edits)):
            if asked and not sampling:
                raise ValueError(f"{what} need the sampling step (the arg-max path has no logits row); greedy runs it with top_k = 1")
        sl = slot or self   # where the picked token, the decode state and the next input row live (self = the single sequence)
        single = sl is self
        B = 0 if single else sl.batch
        tp_sampled = bool(sampling) and self.tp_path
        p2p = self.p2p if single else None      # a batch exchanges through the group, on a peer-to-peer model too
        if tp_sampled:
            if sampling == "hook":
                raise NotImplementedError("logits processors under tensor parallelism are not supported")
            if p2p is not None:
                self._check_p2p_sampling()
            logits = self.logits_loc if single else sl.logits
        else:
            want_logits = bool(sampling) or (self.keep_logits and not B)
            if want_logits and not B and self.last_logits is None:
                self.last_logits = torch.zeros(self.v1 - self.v0, dtype=torch.float32, device=self.device)
            # a batch slot samples from ITS logits row with ITS knobs (per-slot sampling inside a continuous batch)
            logits = (self.last_logits if single else sl.logits) if want_logits else None
        head = dict(N=self.v1 - self.v0, K=H, norm_w=self.W["norm"], eps=c["rms_norm_eps"], y32=logits, ban=self.ban,
                    part_val=sl.part_val_loc, part_idx=sl.part_idx_loc, idx_offset=self.v0)
        if B:
            batch_gemv(self.W["lm_head"], x, part_bs=self.nparts, y_bs=self.Vloc if sampling else 0, **head)
        else:
            ops.gemv(self.W["lm_head"], x, x_delta=x_delta, skip=skip, plan=rec.plan, **head)
        st = ops.decode_state(sl.st_next, sl.st_out, sl.st_step, sl.st_pos, advance_pos=advance_pos, batch=B, done=sl.st_done, eos=sl.st_eos)
        # the picked token's embedding row is written straight into the decode step's input vector
        out = dict(embed=self.W["embed"], h_out=sl.h_dec, Hd=H)
        if single:
            self._pick_state(step_kind(sampling, logprobs, penalties, edits))
        lp = None if logprobs is None else dict(self._lp if single else sl.lp, K=logprobs)      # (the plan is named at the launch: rec.cut() below starts a new one)
        pen = (self._pen if single else sl.pen) if penalties else None
        edt = (self._edt if single else sl.edt) if edits else None
        if tp_sampled:
            row = sl.logits_row     # a batch: [rank][sequence][Vloc] gathered, one draw per sequence over its nseg = tp segments
            if p2p is not None:
                site0 = 2 * c["num_hidden_layers"] + 1
                self._p2p_exchange(rec, st, lambda ph: ops.logits_p2p(logits, self.Vloc, st, p2p, site0, row, phase=ph, plan=rec.plan))
            else:
                rec.cut(lambda: self._gather_partials([row], [logits]))
            seg = dict(nseg=self.tp_size, seg_stride=B * self.Vloc, seg_len=self.Vloc) if B else {}
            if edt:
                ops.logit_edit(row, st, V=c["vocab_size"], plan=rec.plan, **seg, **edt)
            if pen:
                ops.penalize(row, st, V=c["vocab_size"], plan=rec.plan, **seg, **pen)
            ops.sample_final(row, st, V=c["vocab_size"], dev_params=sl.sample_params, plan=rec.plan, **seg, **out)
            if lp:
                ops.logprobs(row, st, V=c["vocab_size"], plan=rec.plan, **seg, **lp)
        elif beam is not None:
            self._beam_pick(rec, beam, nlive=B or 1, advance_pos=advance_pos)
        elif sampling:
            if edt:
                ops.logit_edit(logits, st, V=self.v1 - self.v0, plan=rec.plan, **edt)
            if pen:
                ops.penalize(logits, st, V=self.v1 - self.v0, plan=rec.plan, **pen)
            if sampling == "hook":      # Python logits processors (usdm_amd.serving): a host call between the two kernels
                rec.cut(lambda: self.logits_hook())
            ops.sample_final(logits, st, dev_params=sl.sample_params, plan=rec.plan, **out)
            if lp:
                ops.logprobs(logits, st, V=self.v1 - self.v0, plan=rec.plan, **lp)
        elif p2p is not None:
            # vocab-parallel pick across ranks in ONE launch (pairs exchanged peer to peer; advances the exchange epoch)
            site = 2 * c["num_hidden_layers"]
            self._p2p_exchange(rec, st, lambda ph: ops.argmax_p2p(sl.part_val_loc, sl.part_idx_loc, self.nparts, st, p2p, site, phase=ph,
                                                                  plan=rec.plan, **out))
        else:
            if self.tp_path:      # (the single sequence: the bound method itself, which tools/tp8_proxy.py replaces)
                rec.cut(self._gather_partials if single else
                        (lambda: self._gather_partials([sl.part_val, sl.part_idx], [sl.part_val_loc, sl.part_idx_loc])))
            # a batch's gathered partials are [rank][sequence][nparts], one pick per sequence over the nseg = tp segments; a single
            # sequence's are one row of tp * nparts
            seg = dict(nseg=self.tp_size, seg_stride=B * self.nparts) if (B and self.tp_path) else {}
            ops.argmax_final(sl.part_val, sl.part_idx, self.nparts * (1 if B else self.tp_size), st, plan=rec.plan, **seg, **out)
        rec.plan.hold(st)

    # ------------------------------------------------------------------ plans
    def _dims(self):
        c = self.cfg
        H, d = c["hidden_size"], c["head_dim"]
        return H, d, c["num_hidden_layers"], self.Hq, self.Hkv, self.I, (self.Hq + 2 * self.Hkv) * d

    def _layers(self, rec, gemv, attn, h, qkv, ao, act, way, n=0, parts=None, h_alt=None, down_kw={}, down_wp=None, gu_wp=None):
        """The Mistral layers of every plan: this loop is the one statement of a layer's launch order.
        gemv(W, x, N=, K=, ...): the plan's projection launcher, in usdm_gemv's keywords (norm_w / eps: RMSNorm of x fused in front).
        attn(l): rope, cache and attention of layer l from qkv into ao; returns the keywords its hand-off adds to the o_proj launch.
        way: how a row-parallel projection (o_proj, down_proj; partial sums under tensor parallelism) lands in the residual stream h:
          "fused"    one GPU: residual add in the launch's epilogue;
          "reduce"   f32 partial sums (parts[0] o_proj, parts[1] down_proj) + all-reduce through the group + usdm_residual_add over n
                     values; the plan is cut at the collective;
          "deferred" the same, but the add is folded into the NEXT GEMV's prologue (usdm_gemv x_delta / x_out) instead of a
                     usdm_residual_add launch; the residual stream ping-pongs between h and h_alt because workgroup 0 publishes the
                     updated stream while the others still read the old one;
          "p2p"      the exchange in the launch's epilogue (p2p_fused) or put there and followed by usdm_allreduce_p2p_reduce
                     (split); cut at every exchange so that a single-process harness can interleave logical ranks.
        Returns (h, pend): the residual stream after the last layer and the all-reduced sum not yet added to it (or None)."""
        H, d, _, Hq, Hkv, I, nq = self._dims()
        eps, h0, pend = self.cfg["rms_norm_eps"], h, None

        def proj(W, ln, N, out, a=0, **kw):
            nonlocal h, pend
            if pend is None:
                return gemv(W, h, N=N, K=H, norm_w=ln, eps=eps, act=a, y16=out, **kw)
            nxt = h_alt if h is h0 else h0
            gemv(W, h, N=N, K=H, norm_w=ln, eps=eps, act=a, y16=out, x_delta=pend, x_out=nxt, **kw)
            h, pend = nxt, None

        def land(W, x, K, site, **kw):
            nonlocal pend
            if way == "fused":
                return gemv(W, x, N=H, K=K, residual=h, y16=h, **kw)
            if way == "p2p":
                mode = 1 if self.p2p_fused else 2
                gemv(W, x, N=H, K=K, residual=h, y16=h, p2p=self.p2p, p2p_site=site, p2p_mode=mode, **kw)
                rec.cut()
                if mode == 2:
                    ops.p2p_reduce(self.p2p, site, H, h, skip=self.st_done, plan=rec.plan)
                return
            part = parts[site & 1]
            gemv(W, x, N=H, K=K, round_bf16=False, y32=part, **kw)
            rec.cut(lambda: self._all_reduce(part))
            if way == "deferred":
                pend = part
            else:
                ops.residual_add(h, part, n, plan=rec.plan)

        for l, w in enumerate(self.W["layers"]):
            proj(w["qkv"], w["ln1"], nq, qkv)
            o_kw = attn(l) or {}
            land(w["o"], ao, Hq * d, 2 * l, **o_kw)
            proj(w["gu"], w["ln2"], 2 * I, act, ACT_SWIGLU, **({"wpack": gu_wp[l]} if gu_wp else {}))
            land(w["down"], act, I, 2 * l + 1, **down_kw, **({"wpack": down_wp[l]} if down_wp else {}))
        return h, pend

    def _prefill_rows(self, S, slot=None, past=0):
        """The launches every plan over a prompt's rows begins with: embedding, the layers, K/V rows into the cache (of the slot, or of
        the single sequence), for S new tokens at positions past .. past+S-1 (past > 0: the KV cache already holds the first `past`
        tokens of the same sequence: the single bf16 sequence keeps their V^T, a slot or an fp8 cache gets them from usdm_kv_expand).  Returns (rec, io, h, xn):
        the open plan, its input ids, the final hidden state of every row [S][H] and the [S][H] scratch of the normalised rows."""
        dev, bf = self.device, torch.bfloat16
        H, d, L, Hq, Hkv, I, nq = self._dims()
        scratch = slot is not None or self.kv8      # batch slots / fp8 cache: V^T (fp8: and the bf16 K rows) are scratch of this plan
        # ... which then covers the cached rows in front of the new ones as well: every layer's usdm_kv_expand writes them (past > 0)
        Spad = ((past if scratch else 0) + S + 63) // 64 * 64
        rec = _Segments()
        Z = lambda *s, dt=bf: rec.plan.hold(torch.zeros(*s, device=dev, dtype=dt))
        io = dict(ids=Z(S, dt=torch.int64))
        h, xn, qkv, ao, act = Z(S, H), Z(S, H), Z(S, nq), Z(S, Hq * d), Z(S, I)
        vt = Z(Hkv, d, Spad) if scratch else None
        kscr = Z(Hkv, Spad, d) if self.kv8 else None           # fp8 cache: the bf16 K rows (one scratch, reused by every layer)
        part = Z(S, H, dt=torch.float32) if self.tp_path else None
        ops.embed_rows(self.W["embed"], h, Hd=H, ids=io["ids"], n=S, plan=rec.plan)

        def gemm(W, x, *, N, K, norm_w=None, eps=None, act=0, residual=None, y16=None, y32=None, round_bf16=True):
            """usdm_gemv's keywords on the prefill launches: usdm_norm (when asked for) + usdm_gemm (fp8: the matrix dequantized
            first), which rounds to bf16 only in front of an epilogue"""
            if norm_w is not None:
                ops.norm(x, norm_w, None, rows=S, C=H, eps=eps, rms=True, round_bf16=True, out16=xn, plan=rec.plan)
                x = xn
            ops.gemm(x, self._gemm_w(W, rec.plan), M=S, N=N, Kc=K, act=act, round_bf16=round_bf16 and (bool(act) or residual is not None),
                     residual=residual, ldr=H if residual is not None else 0, out32=y32, out16=y16, ldc=N // 2 if act else N, plan=rec.plan)

        # Rows go to the cache of the slot or of the single sequence (fp8 cache: quantized).  The prompt's own attention reads K from
        # that cache, or (fp8 cache) the unquantized K rows from scratch, and V^T from this plan's scratch or the persistent V^T of the
        # single bf16 sequence
        cs = slot if slot is not None else self
        k_ld = Spad if self.kv8 else self.ctx_max
        vt_ld = Spad if vt is not None else self.ctx_max

        def attn(l):
            vtl = vt if vt is not None else self.vtc[l]
            kv8 = (cs.kexp[l], cs.vexp[l]) if self.kv8 else None
            if past and scratch:      # the cached rows: V^T columns / K rows [0, past); beyond past + S the scratch stays zero
                ops.kv_expand(cs.kcache[l], cs.vcache[l], vt, n=past, Hkv=Hkv, ctx_max=self.ctx_max, vt_ld=Spad, kv8=kv8, kscr=kscr,
                              kscr_ld=Spad if self.kv8 else 0, plan=rec.plan)
            ops.rope_cache(qkv, self.cos, self.sin, cs.kcache[l], cs.vcache[l], ld=nq, S=S, pos0=past, Hq=Hq, Hkv=Hkv, ctx_max=self.ctx_max,
                           max_pos=self.ctx_max, vt=vtl[:, :, past:], vt_ld=vt_ld, kv8=kv8,
                           kscr=kscr[:, past:] if self.kv8 else None, kscr_ld=Spad if self.kv8 else 0, plan=rec.plan)
            ops.attention(qkv, kscr if self.kv8 else cs.kcache[l], vtl, ao, mode=1, dh=d, B=1, Hq=Hq, Hkv=Hkv, Sq=S, Skv=past + S,
                          Skv_alloc=vt_ld, q_pos0=past, q_strides=(0, d, nq), k_strides=(0, k_ld * d, d), v_strides=(0, d * vt_ld, vt_ld),
                          o_strides=(0, Hq * d), scale=d ** -0.5, window=self.window, plan=rec.plan)

        self._layers(rec, gemm, attn, h, qkv, ao, act, "reduce" if self.tp_path else "fused", n=S * H, parts=(part, part))
        return rec, io, h, xn

    def _build_prefill(self, S, sampling=None, slot=None, past=0, logprobs=None, penalties=False, edits=False, beam=None):
        """Prefill of S new tokens at positions past .. past+S-1 (_prefill_rows), then the lm_head over the LAST row and the pick of the
        first generated token (beam: the prompt into slot 0 of those beam slots, logits row 0, the search's first pick)."""
        rec, io, h, _ = self._prefill_rows(S, slot=slot, past=past)
        self._lm_head_and_pick(rec, h[S - 1], False, sampling, slot=slot, logprobs=logprobs, penalties=penalties, edits=edits, beam=beam)
        return rec.finish(), io

    def _score_head(self):
        """The bf16 [v1 - v0][H] operand of score()'s lm_head GEMMs: the weight itself, or (fp8 / mxfp4 models, whose lm_head is fp8) its
        dequantization, done ONCE at first use into a tensor of its own that the model keeps (344 MB on the 7B): dq_scratch is sized
        for the largest layer matrix, which is smaller than the lm_head, and is rewritten by every layer of every prefill."""
        W = self.W["lm_head"]
        if not isinstance(W, Fp8Weight):
            return W
        if self._head_bf16 is None:
            self._head_bf16 = torch.empty(W.N, W.K, dtype=torch.bfloat16, device=self.device)
            ops.dequant_fp8(W, self._head_bf16)
        return self._head_bf16

    def _build_score(self, S, past, j0, K):
        """The plan of score(): _prefill_rows over S new tokens at positions past .. past+S-1, one usdm_norm (the final RMSNorm) over
        all S rows, then per chunk of score_rows rows over the new-token rows j0 .. S-2 one lm_head usdm_gemm into an f32 chunk
        [score_rows][Vloc, padded to 4] (round_bf16: the bf16-valued logits the lm_head GEMV writes and HF's bf16 head produces) and one
        usdm_prompt_logprobs against io["ids"] (local row j's target is ids[j + 1]; outputs at the target's local row).  No ban mask,
        no penalties, no edits, no pick, no decode-state write, no host sync.  Tensor parallel: every rank's chunk is gathered rank-major
        into [tp][score_rows][Vloc] (the plan is cut at the collective) and every rank runs usdm_prompt_logprobs_seg on it with the
        global ids.  keep_score_logits: every chunk is also copied into io["logits"] [S - 1 - j0][V]."""
        dev, c, H, V = self.device, self.cfg, self.cfg["hidden_size"], self.cfg["vocab_size"]
        rec, io, h, xn = self._prefill_rows(S, past=past)
        R, Vn, tp = self.score_rows, self.v1 - self.v0, self.tp_size if self.tp_path else 1
        ldl = (self.Vloc + 3) // 4 * 4      # row stride of the chunk: 16-byte rows, so that the GEMM's epilogue stores float4s
        Zf = lambda *s: rec.plan.hold(torch.zeros(*s, device=dev, dtype=torch.float32))
        chunk = Zf(R, ldl)
        gathered = Zf(tp, R, ldl) if self.tp_path else None
        head = self._score_head()
        if self._score_out is None:
            n, kk = self.ctx_max, self.ctx_max * ops.LOGPROBS_MAX_K
            self._score_out = dict(tok_lp=torch.zeros(n, dtype=torch.float32, device=dev), tok_rank=torch.zeros(n, dtype=torch.int32, device=dev),
                                   top_id=torch.zeros(kk, dtype=torch.int32, device=dev), top_lp=torch.zeros(kk, dtype=torch.float32, device=dev))
        keep = Zf(S - 1 - j0, ldl if not self.tp_path else tp * self.Vloc) if self.keep_score_logits else None
        io.update(logits=None if keep is None else keep[:, :V], keep=self.keep_score_logits)
        ops.norm(h, self.W["norm"], None, rows=S, C=H, eps=c["rms_norm_eps"], rms=True, round_bf16=True, out16=xn, plan=rec.plan)
        for j in range(j0, S - 1, R):
            rows = min(R, S - 1 - j)
            ops.gemm(xn[j:], head, M=rows, N=Vn, Kc=H, round_bf16=True, out32=chunk, ldc=ldl, plan=rec.plan)
            if self.tp_path:
                def gather(j=j, rows=rows):
                    self._gather_partials([gathered], [chunk])
                    if keep is not None:      # the logical rows: the ranks' Vloc slots side by side (the last rank's padding is past V)
                        keep[j - j0:j - j0 + rows] = gathered[:, :rows, :self.Vloc].transpose(0, 1).reshape(rows, tp * self.Vloc)
                rec.cut(gather)
                ops.prompt_logprobs(gathered[:, :, :self.Vloc], io["ids"], row0=j, rows=rows, K=K, V=V, nseg=tp, seg_stride=R * ldl, seg_len=self.Vloc,
                                    plan=rec.plan, **self._score_out)
            else:
                if keep is not None:
                    ops.copy_bytes(keep[j - j0], chunk, rows * ldl * 4, plan=rec.plan)
                ops.prompt_logprobs(chunk, io["ids"], row0=j, rows=rows, K=K, V=V, plan=rec.plan, **self._score_out)
        return rec.finish(), io

    def _build_decode(self, sampling=None, logprobs=None, penalties=False, edits=False):
        """One decode step of the single sequence.  Tensor parallel with a P2PComm: the launch sequence of the single-GPU step over
        this rank's shards, o_proj / down_proj carry the exchange (_layers, way "p2p"); returned as segments cut at every exchange,
        which a real rank runs back to back inside one hipGraph."""
        dev, bf = self.device, torch.bfloat16
        H, d, L, Hq, Hkv, I, nq = self._dims()
        if self.p2p is not None:
            way = "p2p"
        elif not self.tp_path:
            way = "fused"
        else:
            way = "deferred" if os.environ.get("USDM_TP_FUSED_RESIDUAL", "1") == "1" else "reduce"
        collective = way in ("deferred", "reduce")
        rec = _Segments()
        Z = lambda *s, dt=bf: rec.plan.hold(torch.zeros(*s, device=dev, dtype=dt))
        h, qkv, ao, act = self.h_dec, Z(nq), Z(Hq * d), Z(I)
        pm, pl, po = Z(Hq * self.NS, dt=torch.float32), Z(Hq * self.NS, dt=torch.float32), Z(Hq * self.NS * d, dt=torch.float32)
        parts = (Z(H, dt=torch.float32), Z(H, dt=torch.float32)) if collective else None
        h_alt = Z(H) if collective else None
        # last-arriver counters of the fused partial merge (self-resetting).  Off by default: measured 11.3-11.6 us per layer
        # against 5.9 + 4.6 us for the split kernel + merge kernel (profiles/r01_decode_ablation.txt)
        cnt = Z(Hkv, dt=torch.int32) if (os.environ.get("USDM_ATTN_FUSED_MERGE", "0") == "1" and way != "p2p") else None
        skp = self.st_done   # decode kernels return at once after a device-side EOS (see _alloc)
        cmb_gran = Z(L, Hq * 64, dt=torch.int64) if self.cmb else None      # one granule block per layer (tags cleared by the layer's attention launch)
        # the chained forms (USDM_GEMV_CHAIN): o_proj -> gate/up -> down_proj [-> the next layer's qkv] become the phases of ONE
        # launch; `chain` holds the phases of the open chain (None: every projection is its own launch)
        chained = way == "fused" and self.chain in (3, 4) and cnt is None and not self.merge_in_oproj
        use_cmb = self.cmb and way == "fused" and not chained and cnt is None and self.NS > 1
        mrg = (pm, pl, po, self.NS) if ((self.merge_in_oproj or use_cmb) and cnt is None) else None
        chain = None

        def flush():
            nonlocal chain
            sync = self.chain_sync[0 if len(chain) == self.chain else 1]
            if self.chain_engine:
                ops.gemv_engine(chain, sync, self.chain_gran, plan=rec.plan)
            else:
                ops.gemv_chain(chain, sync, plan=rec.plan)
            chain = None

        def gemv(W, x, **kw):
            if chain is None:
                return ops.gemv(W, x, skip=skp, plan=rec.plan, **kw)
            chain.append(ops.gemv(W, x, skip=skp, only_args=True, **kw))
            if len(chain) == self.chain:
                flush()

        def attn(l):   # h already holds the embedding of the current token (written by usdm_argmax_final)
            nonlocal chain
            gran = cmb_gran[l] if use_cmb else None
            ops.attn_decode(qkv, self.st_pos, self.cos, self.sin, self.kcache[l], self.vcache[l], pm, pl, po, ao, Hq=Hq, Hkv=Hkv,
                            ctx_max=self.ctx_max, NS=self.NS, scale=d ** -0.5, counters=cnt, skip=skp, defer_merge=mrg is not None, window=self.window,
                            cmb_gran=gran, kv8=(self.kexp[l], self.vexp[l]) if self.kv8 else None, plan=rec.plan)
            if chained:
                chain = []
                return None
            return dict(merge=mrg, cmb=(gran, self.cmb_err) if use_cmb else None)

        # (down_wp, gu_wp: the 13-bit images of the down_proj and gate/up matrices - this step only; a chained step keeps its bf16
        # phases)
        h, pend = self._layers(rec, gemv, attn, h, qkv, ao, act, way, n=H, parts=parts, h_alt=h_alt,
                               down_wp=self.wpack_down if way == "fused" else None, gu_wp=self.wpack_gu if way == "fused" else None)
        if chain:     # the last layer's chain has no next qkv to wait for
            flush()
        # (pend: the last down-projection's sum goes into the final norm + lm_head)
        self._lm_head_and_pick(rec, h, True, sampling, x_delta=pend, skip=skp, logprobs=logprobs, penalties=penalties, edits=edits)
        return rec.finish()

    @staticmethod
    def _run_segs(segs):
        for s in segs:
            if isinstance(s, ops.Plan):
                s.run()
            else:
                s()

    def _graphed(self, built, enabled=None):
        """What a builder returned -> the step that replays it: a GraphedPlan when no host call sits between the launches (segments
        that were cut for the lockstep harness only, the peer-to-peer step, are joined: kernels only, one plan, one hipGraph), else
        GraphedSegments."""
        segs = built if isinstance(built, list) else [built]
        if any(not isinstance(s, ops.Plan) for s in segs):
            return GraphedSegments(segs, self._run_segs, enabled=enabled)
        plan = segs[0]
        if len(segs) > 1:
            plan = ops.Plan()
            for s in segs:
                plan.calls += s.calls
                plan.hold(*s.keep)
        return GraphedPlan(plan)

    def _reused_past(self, input_ids, cap):
        """Prefix reuse of the single sequence: (the prompt's ids as a list, or None with reuse off; past = how many of them, at most
        cap, are not prefilled again because their K/V are already cached - the same ids at the same positions, prefix.reusable_past)."""
        if not self.reuse_prefix:
            return None, 0
        ids_host = input_ids[0].tolist()
        past = reusable_past(ids_host, self._kv_ids, cap, self._vt_upto, self.reuse_prefix == "exact")
        if past > self._vt_upto and self.vtc is not None:   # K/V appended by decode steps have no V^T yet: one transposed copy over all layers (fp8 cache: the plan's usdm_kv_expand covers them)
            a0 = self._vt_upto
            self.vtc[:, :, :, a0:past] = self.vcache[:, :, a0:past, :].transpose(2, 3)
        return ids_host, past

    @torch.no_grad()
    def score(self, input_ids, top_logprobs=0, start=1):
        """Log-probabilities of tokens that were GIVEN: TokenLogprobs whose row i describes token start + i of input_ids [1, L] given
        the tokens in front of it, for start <= start + i < L (log p(token_t | tokens_<t), its rank, and the top_logprobs most likely ids
        of that position, 0 .. 20; None = 0), with .cumulative as generate(logprobs=) reports it.  Nothing is generated: one prefill over
        the rows, the lm_head as GEMMs over chunks of score_rows rows and usdm_prompt_logprobs per chunk, all on the device.
        The distribution is the RAW model's over all vocab_size ids - no ban mask, no penalties, no bias, no temperature: vLLM's
        definition of prompt log-probabilities (generate(logprobs=) reports the ban-masked row it picked from instead).
        With reuse_prefix on, cached rows of a common prefix are reused up to start - 1 tokens under generate()'s rule ("exact": rows a
        prefill wrote), and the call leaves the prompt's ids behind as cached prefill-written rows: N candidates behind one prefix
        prefill and score their own rows only.  With the fp8 KV cache nothing is reused unless the model was built with
        enable_prefix_caching=True; the reused rows are then read as the cache holds them, quantized.
        last_logits, last_logprobs, the sampler's, the penalties' and the edits' state are not touched.
        keep_score_logits = True (debug / tests): last_score_logits is then the [L - start][vocab_size] f32 logits rows scored."""
        K = check_logprobs(top_logprobs) or 0
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("input_ids must be a LongTensor of shape [1, L] (batch 1)")
        L = int(input_ids.shape[1])
        if L < 2 or L > self.ctx_max:
            raise ValueError(f"score() needs 2 <= L <= ctx_max = {self.ctx_max} tokens, got {L}")
        if isinstance(start, bool) or not isinstance(start, int) or not 1 <= start <= L - 1:
            raise ValueError(f"start must be an integer 1 .. L - 1 = {L - 1}, got {start!r}")
        ids_host, past = self._reused_past(input_ids, start - 1)
        S, j0 = L - past, start - 1 - past
        key = (S, past, j0, K)
        hit = self._score_plans.get(key)
        if hit is None or hit[1]["keep"] != self.keep_score_logits:
            hit = self._score_plans.put(key, self._build_score(*key))
        segs, io = hit
        io["ids"].copy_(input_ids[0, past:])
        self._kv_ids, self._vt_upto = None, L
        self._run_segs(segs)
        if self.reuse_prefix:      # every row of the prompt now sits in the cache, written by prefill launches
            self._kv_ids = ids_host
        self.last_score_logits = io["logits"]
        o = self._score_out
        top = lambda t: t[:S * K].view(S, K)[j0 + 1:].cpu()
        return TokenLogprobs(o["tok_lp"][j0 + 1:S].cpu(), o["tok_rank"][j0 + 1:S].cpu(), top(o["top_id"]), top(o["top_lp"]))

    # ------------------------------------------------------------------ batched decode (the slots: usdm_amd/slots.py)
    def decode_slots(self, B):
        """The B slots that decode in lockstep (slots.DecodeSlots), built at first use and kept."""
        if B not in self._batches:
            self._batches[B] = DecodeSlots(self, B)
        return self._batches[B]

    def _batch_gemv(self, n, rec):
        """(gemv, ks) of a step over n rows (B sequences; the T rows of a speculative step) into the open plan rec.  gemv: the projection
        launcher, usdm_gemv's keywords over the n rows: x [n][K], outputs [n][N] (SwiGLU: half of that), residual [n][N].  ks: down_proj
        on the matrix cores (K = 14336, n > 4): K split over workgroups, each holding its activation slice (usdm_gemv_batch ks_*); one
        scratch for all layers - the launches of a step are serial and each leaves the counters zero.  fp8_matrix_cores: the FP8
        projections of 5..16 rows on the matrix cores (usdm_gemv_fp8_mfma: the bf16 form's tiles, K split and epilogues, so the same ks
        scratch); <= 4 keep the VALU FP8 form of gemv_batch.  mxfp4_matrix_cores: likewise, per weight (the lm_head of an mxfp4 model is fp8)."""
        H, Z = self.cfg["hidden_size"], lambda n, dt: rec.plan.hold(torch.zeros(n, device=self.device, dtype=dt))
        ksf = ops.gemv_batch_ks_floats(H, self.I) if n > 4 else 0
        ks = (Z(ksf, torch.float32), Z(-(-H // 16), torch.int32)) if ksf else None
        gemv_b = ops.gemv_fp8_mfma if (self.fp8_matrix_cores and n > 4) else ops.gemv_batch
        if self.mxfp4_matrix_cores and n > 4:      # per weight: the layers' Mxfp4Weight on usdm_gemv_mxfp4_mfma, the fp8 lm_head on usdm_gemv_fp8_mfma
            gemv_b = lambda W, x, **kw: (ops.gemv_mxfp4_mfma if isinstance(W, Mxfp4Weight) else ops.gemv_fp8_mfma)(W, x, **kw)

        def gemv(W, x, *, N, K, act=0, residual=None, y_bs=None, **kw):
            gemv_b(W, x, nb=n, N=N, K=K, x_bs=K, y_bs=(N // 2 if act else N) if y_bs is None else y_bs, res_bs=N if residual is not None else 0,
                   act=act, residual=residual, plan=rec.plan, **kw)
        return gemv, ks

    def _build_decode_batch(self, B, sampling=False, logprobs=None, penalties=False, edits=False, beam=None):
        """One decode step of the B decode slots: weights streamed once (usdm_gemv_batch), attention / token pick batched over items.
        sampling: the pick is usdm_sample_final's batched form - every slot draws with its OWN knobs (row b of the slots' sp:
        temperature, top-k, top-p, seed) and its own Philox counter; a greedy slot carries top_k = 1.
        beam (a slots.BeamSlots): the step of a beam search over those slots instead - the pick is usdm_beam_step over
        the B rows, followed by usdm_kv_reorder; returned as its two segments (the pick's end is where an eager run can look)."""
        dev, bf = self.device, torch.bfloat16
        H, d, L, Hq, Hkv, I, nq = self._dims()
        ds = self.decode_slots(B) if beam is None else beam
        rec = _Segments()
        Z = lambda *s, dt=bf: rec.plan.hold(torch.zeros(*s, device=dev, dtype=dt))
        h, qkv, ao, act = ds.h, Z(B, nq), Z(B, Hq * d), Z(B, I)
        NS = max(2, self.NS)
        if B > 4:
            # many sequences: B x Hkv x NS workgroups of ctx / NS keys each.  The batch-1 choice (32 splits of ~20 keys: latency-bound,
            # one per CU) would be 4096 tiny workgroups at B = 16 (measured 35.6 us per layer); ~512 workgroups with up to 512 keys
            # (the split kernel's LDS bound) keep the KV stream at full width.  (B <= 4 keeps the batch-1 splits: bit-identical.)
            NS = max(-(-self.ctx_max // 512), min(self.NS, max(2, self.batch_attn_wgs // (B * Hkv))))
        pm, pl, po = Z(B * Hq * NS, dt=torch.float32), Z(B * Hq * NS, dt=torch.float32), Z(B * Hq * NS * d, dt=torch.float32)
        cnt = Z(B * Hkv, dt=torch.int32) if B > 4 and self.batch_fused_merge else None
        cache_bs = L * Hkv * self.ctx_max * d
        gemv, ks = self._batch_gemv(B, rec)
        # Tensor parallel (SURVEY.md 8e x 8f-2; round 4, the collective form): the row-parallel projections leave f32 partial sums
        # [B][H], all-reduced through the job's process group (RCCL: one collective of B x 16 KB per projection instead of B of them),
        # then usdm_residual_add applies HF's rounding points; the plan is cut into segments at the collectives, as the
        # single-sequence RCCL path is (_layers, way "reduce").  Sampled: the slots' logits rows are gathered and drawn from on every
        # rank (usdm_sample_final_seg).
        tp = self.tp_path
        parts = (Z(B, H, dt=torch.float32), Z(B, H, dt=torch.float32)) if tp else None

        def attn(l):
            ops.attn_decode(qkv, ds.pos, self.cos, self.sin, ds.kc[0, l], ds.vc[0, l], pm, pl, po, ao, Hq=Hq, Hkv=Hkv,
                            ctx_max=self.ctx_max, NS=NS, scale=d ** -0.5, batch=B, qkv_bs=nq, out_bs=Hq * d, cache_bs=cache_bs, window=self.window,
                            counters=cnt, kv8=(ds.ke[0, l], ds.ve[0, l]) if self.kv8 else None, exp_bs=cache_bs // d, plan=rec.plan)

        self._layers(rec, gemv, attn, h, qkv, ao, act, "reduce" if tp else "fused", n=B * H, parts=parts, down_kw={} if tp else dict(ks=ks))
        self._lm_head_and_pick(rec, h, True, sampling, slot=ds.all, batch_gemv=gemv, logprobs=logprobs, penalties=penalties, edits=edits,
                               beam=beam)
        segs = rec.finish()
        return segs if (tp or beam is not None) else segs[0]

    # ------------------------------------------------------------------ speculative greedy decoding (the states: usdm_amd/slots.py)
    def _build_spec_step(self, state, T, sampled=False):
        """One speculative step of a slots.SpecState: its n sequences x T rows each (row b * T + i: sequence b's token at position
        pos[b] + i - the token to continue from and T - 1 drafts) through _layers with the batched projections of _build_decode_batch
        over n * T rows (weights streamed once; <= 4 rows on the VALU form, bit-identical per row with the single step, 5 .. 16 on the
        matrix cores), the state's verify attention on its caches (SpecSequence: usdm_attn_verify, every cached row read once for all
        rows; SpecSlots: usdm_attn_verify_batch), the lm_head in batched arg-max mode, the state's commit (usdm_spec_commit /
        usdm_spec_commit_batch).  Sequences with done != 0 are skipped by the attention and the commit.  One plan, one graph per
        state, T and sampled.
        sampled: the lm_head also materialises the rows' f32 logits (y32, as the sampled batched step and beam search
        do), usdm_spec_sample draws row i of sequence b with b's knobs at the counter step[b] + i - the token the plain sampled call
        draws at that position from that row - and the commit takes those picks in place of the arg-max."""
        dev, bf = self.device, torch.bfloat16
        H, d, L, Hq, Hkv, I, nq = self._dims()
        n = state.n * T
        if n > self.max_batch():
            raise ValueError(f"{state.n} slots of {T} rows: a decode step of this model takes at most {self.max_batch()} rows")
        r = state.spec_rows(T)
        rec = _Segments()
        Z = lambda *s, dt=bf: rec.plan.hold(torch.zeros(*s, device=dev, dtype=dt))
        h, qkv, ao, act = r["h"], Z(n, nq), Z(n, Hq * d), Z(n, I)
        nsp = ops.attn_verify_splits(self.ctx_max, self.spec_split)
        pm, pl, po = Z(n * Hq * nsp, dt=torch.float32), Z(n * Hq * nsp, dt=torch.float32), Z(n * Hq * nsp * d, dt=torch.float32)
        gemv, ks = self._batch_gemv(n, rec)

        def attn(l):
            state.attn(l, qkv, pm, pl, po, ao, T=T, Hq=Hq, Hkv=Hkv, ctx_max=self.ctx_max, C=self.spec_split, scale=d ** -0.5,
                       window=self.window, plan=rec.plan)

        self._layers(rec, gemv, attn, h, qkv, ao, act, "fused", n=n * H, down_kw=dict(ks=ks))
        if sampled:
            gemv(self.W["lm_head"], h, N=self.v1 - self.v0, K=H, norm_w=self.W["norm"], eps=self.cfg["rms_norm_eps"], ban=self.ban,
                 y32=state.sample_rows(T)["logits"], part_val=r["pv"], part_idx=r["pi"], idx_offset=self.v0, part_bs=self.nparts, y_bs=self.Vloc)
            state.sample(T, rec.plan)
            state.commit(T, rec.plan, sampled=True)
            return rec.finish()[0]
        gemv(self.W["lm_head"], h, N=self.v1 - self.v0, K=H, norm_w=self.W["norm"], eps=self.cfg["rms_norm_eps"], ban=self.ban,
             part_val=r["pv"], part_idx=r["pi"], idx_offset=self.v0, part_bs=self.nparts, y_bs=0)
        state.commit(T, rec.plan)
        return rec.finish()[0]

    def spec_slots(self, B):
        """The B slots of batched speculative decoding (slots.SpecSlots), built at first use and kept."""
        if B not in self._spec_batches:
            self._spec_batches[B] = SpecSlots(self, B, step_kind())
        return self._spec_batches[B]

    def _check_spec_shape(self, k):
        """ValueError where this model's step or context cannot take k drafts"""
        if k + 1 > self.max_batch():
            raise ValueError(f"num_speculative_tokens={k}: a decode step of this model takes at most {self.max_batch()} rows")
        if -(-self.ctx_max // self.spec_split) > 64 or self.spec_split % ops.ATTN_VERIFY_TILE or not 0 < self.spec_split <= ops.ATTN_VERIFY_CMAX:
            raise ValueError(f"speculative decoding: ctx_max = {self.ctx_max} with {self.spec_split} keys per split (a multiple of "
                             f"{ops.ATTN_VERIFY_TILE} up to {ops.ATTN_VERIFY_CMAX}, at most 64 splits) is not supported")

    def spec_group(self, k):
        """Sequences per speculative step with k drafts each: the rows of a step shared out in slots of k + 1"""
        return self.max_batch() // (k + 1)

    def _generate_spec_group(self, ids_list, limits, spec, scripts, bad_words_ids, eos_token_id, min_new_tokens, samplings=None):
        """A group of 2 .. max_batch() // (k + 1) sequences on the speculative slots: per-slot prefill, then the step of B x (k + 1)
        rows replayed in chunks (SpecSlots.serve).  samplings (a list: per sequence the slot's knobs or None = greedy): the sampled
        step.  -> (the sequences, their dict(steps=, drafted=, accepted=))"""
        k, lookup_max, lookup_min = spec
        ss = self.spec_slots(len(ids_list))
        self.load_ban(bad_words_ids)
        ss.set_lookup(lookup_max, lookup_min, scripts is not None)
        stops = stop_ids(eos_token_id)
        reqs = [dict(ids=ids[0], limit=lim, stops=stops, min_new=min_new_tokens, script=None if scripts is None else scripts[b],
                     sampling=None if samplings is None else samplings[b])
                for b, (ids, lim) in enumerate(zip(ids_list, limits))]
        res, _ = ss.serve(reqs, k + 1, sampled=samplings is not None)
        outs = [torch.cat([ids[0], torch.tensor(toks, dtype=torch.long, device=ids.device)]).unsqueeze(0) for ids, (toks, _) in zip(ids_list, res)]
        return outs, [st for _, st in res]

    MAX_BATCH = 16      # sequences per decode step (usdm_gemv_batch: VALU form up to 4, matrix-core form up to 16)

    def max_batch(self):
        """Sequences one decode step can take with THIS model's (per-rank) shapes: 16 where the matrix-core launcher takes every
        projection and the lm_head shard (its own answer: ops.gemv_mfma_select), else the 4 of the VALU form."""
        H, d, _, Hq, _, I, nq = self._dims()
        fmt = "bf16"
        if self.quantization in ("fp8", "mxfp4"):
            if not (self.fp8_matrix_cores if self.quantization == "fp8" else self.mxfp4_matrix_cores):
                return 4                        # usdm_gemv_fp8 / usdm_gemv_mxfp4: the VALU form only
            fmt = self.quantization
        # (N, K, mode, format) of qkv, o_proj, gate/up, down_proj and the lm_head shard (fp8 in an mxfp4 model) as _layers launches them
        shapes = ((nq, H, dict(norm=True), fmt), (H, Hq * d, {}, fmt), (2 * I, H, dict(norm=True, glu=True), fmt), (H, I, dict(ks=True), fmt),
                  (self.v1 - self.v0, H, dict(norm=True, lm_head=True), "fp8" if fmt == "mxfp4" else fmt))
        try:
            for N, K, mode, f in shapes:
                ops.gemv_mfma_select(N, K, form=1 if f == "bf16" else 0, fmt=f, **mode)
        except UsdmError:
            return 4
        return self.MAX_BATCH

    @torch.no_grad()
    def generate_batch(self, input_ids_list, max_new_tokens, bad_words_ids=None, eos_token_id=None, min_new_tokens=0, group=None,
                       logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None,
                       no_repeat_ngram_size=0, num_speculative_tokens=None, prompt_lookup_max=3, prompt_lookup_min=1, _spec_script=None,
                       speculative_sampling=False, do_sample=False, temperature=1.0, top_k=None, top_p=1.0, seed=None):
        """Greedy generation of several utterances in lockstep (the serving-side batching of inference_vllm.py:109-125): up to
        `group` (default 16) sequences per step, longer lists run in groups.  Each prompt is prefilled on its own; every decode
        step then streams the weights once for the whole group.  Groups of <= 4 run on the VALU kernel and equal generate() per
        sequence bit for bit; larger groups run on the matrix cores (usdm_gemv_batch form 1): the same rounding points, K summed
        in another order - equal to the oracle up to its near-ties, not bit-identical with generate().
        logprobs=K (0 .. 20): self.last_logprobs is then the list of the sequences' TokenLogprobs (see generate()).
        repetition_penalty / presence_penalty / frequency_penalty: one value for all sequences or a list with one per sequence (see
        generate()); a group with a non-neutral knob runs on the penalised sampling step, its other sequences with neutral knobs.
        logit_bias / no_repeat_ngram_size: one dict / integer for all sequences or a list with one per sequence, likewise (the step
        with usdm_logit_edit).  min_p is accepted and range-checked for symmetry with generate(): these picks are greedy (top_k = 1),
        where it changes nothing.
        On a model built with enable_prefix_caching=True every prompt reuses the rows of the longest prefix (>= 16 tokens) that a slot
        of the group's buffers holds from an earlier prefill, and prefills the rest (DecodeSlots.admit; self.stats counts prefix_hits,
        prefix_rows_reused, prefix_copies, prefill_rows); bf16 cache: the same ids and log-probabilities, bit for bit.
        num_speculative_tokens=k in 1 .. 7 (None / 0: this call is what it is without the argument, nothing is built): batched
        speculative greedy decoding (see generate()).  The list runs in groups of max_batch() // (k + 1) sequences
        (`group`, if given, caps that too); every step verifies k drafts of EVERY sequence of the group in one pass over the weights:
        B x (k + 1) rows.  A group of one - a list of one, the last of an odd list, a model whose step has no room for two (mxfp4 / VALU
        fp8 weights with k > 1) - runs generate()'s single-sequence path.  The ids do not depend on the drafts; at B * (k + 1) <= 4 rows
        they equal generate(num_speculative_tokens=k) bit for bit, above they are equal up to near-ties (the matrix cores).
        max_new_tokens may then be a list with one value per sequence.  self.last_spec_stats = [dict(steps=, drafted=, accepted=)] per
        sequence.  _spec_script (tests, tools/spec_batch_rate.py): one script per sequence.  Refused as in generate()
        (spec.check_spec_call), and (NotImplementedError) groups of two or more on a model built with enable_prefix_caching=True.
        speculative_sampling=True (with num_speculative_tokens=k; DESIGN.md 8k-3, see generate()): the groups run the SAMPLED
        speculative step, every slot with its own knobs and seed - do_sample, temperature, top_k, top_p, seed and min_p are then one
        value for all sequences or a list with one per sequence (seed None: drawn as generate() draws it).  A sequence with do_sample
        False or top_k == 1 is greedy inside the step (top_k = 1).  For a fixed seed a sequence's ids depend neither on the drafts nor
        on its neighbours; at B * (k + 1) <= 4 rows they equal generate(..., speculative_sampling=True) of that sequence bit for bit.
        Without the flag the sampling arguments are refused (ValueError): these picks are greedy."""
        from .spec import check_spec_args, check_spec_call, check_speculative_sampling
        spec = check_spec_args(num_speculative_tokens, prompt_lookup_max, prompt_lookup_min)
        spec_sampled = check_speculative_sampling(speculative_sampling, spec is not None)
        lpk = check_logprobs(logprobs)
        n = len(input_ids_list)
        pens = [check_penalties(*k) for k in zip(*(_per_sequence(k, n) for k in (repetition_penalty, presence_penalty, frequency_penalty)))]
        for v in _per_sequence(min_p, n):
            check_min_p(v)
        V = self.cfg["vocab_size"]
        edits = [check_edits(lb, ng, V) for lb, ng in zip(_per_sequence(logit_bias, n), _per_sequence(no_repeat_ngram_size, n))]
        knobs = [_per_sequence(v, n) for v in (do_sample, temperature, top_k, top_p, seed)]
        if not spec_sampled and (any(knobs[0]) or any(t != 1.0 for t in knobs[1]) or any(k is not None for k in knobs[2])
                                 or any(p != 1.0 for p in knobs[3]) or any(s is not None for s in knobs[4])):
            raise ValueError("generate_batch picks greedily: do_sample / temperature / top_k / top_p / seed need num_speculative_tokens "
                             "with speculative_sampling=True")
        if spec is not None:
            check_spec_call(False, lpk, next((p for p in pens if p is not None), None), next((e for e in edits if e is not None), None),
                            any(_per_sequence(min_p, n)), tensor_parallel=self.tp_path, kv_cache_fp8=self.kv8, speculative_sampling=spec_sampled)
            samplings = [self._slot_sampling(*k) for k in zip(*knobs, _per_sequence(min_p, n))] if spec_sampled else None
            return self._generate_batch_spec(input_ids_list, max_new_tokens, spec, _spec_script, bad_words_ids, eos_token_id, min_new_tokens, group,
                                             samplings)
        group = self.max_batch() if group is None else max(1, min(int(group), self.max_batch()))
        outs, self.last_logprobs = [], (None if lpk is None else [])
        for g0 in range(0, n, group):
            outs += self._generate_group(input_ids_list[g0:g0 + group], max_new_tokens, bad_words_ids, eos_token_id, min_new_tokens, lpk,
                                         pens[g0:g0 + group], edits[g0:g0 + group])
        return outs

    def _slot_sampling(self, do_sample, temperature, top_k, top_p, seed, min_p):
        """One sequence's knobs of a sampled speculative group -> (temperature, top_k, top_p, seed, min_p) for its slot's sampler
        block, or None where it is greedy (do_sample False or top_k == 1), checked and seeded as generate() does it"""
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0):
            raise ValueError(f"top_k must be None or an integer >= 0 (0 = off), got {top_k!r}")
        if not do_sample:
            if temperature != 1.0 or top_p != 1.0:
                raise ValueError("temperature / top_p only apply with do_sample=True")
            return None
        if top_k == 1:
            return None
        if not (temperature > 0) or not (0 < top_p <= 1):
            raise ValueError("temperature must be > 0 and top_p in (0, 1]")
        if seed is None:
            seed = self._agree_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))
        return (temperature, int(top_k or 0), top_p, seed, min_p)

    def _generate_batch_spec(self, ids_list, max_new_tokens, spec, scripts, bad_words_ids, eos_token_id, min_new_tokens, group=None,
                             samplings=None):
        """generate_batch(num_speculative_tokens=k): the groups of spec_group(k) sequences; a group of one is generate()'s call.
        samplings (speculative_sampling=True): per sequence _slot_sampling's value; the groups then run the sampled step."""
        k, lookup_max, lookup_min = spec
        n = len(ids_list)
        self._check_spec_shape(k)
        if scripts is not None and len(scripts) != n:
            raise ValueError("_spec_script: one script per sequence")
        for ids in ids_list:
            if ids.dim() != 2 or ids.shape[0] != 1:
                raise ValueError("every prompt must be a LongTensor of shape [1, L]")
        per = _per_sequence(max_new_tokens, n)
        size = max(1, self.spec_group(k) if group is None else min(int(group), self.spec_group(k)))
        outs, stats = [], []
        for g0 in range(0, n, size):
            grp = ids_list[g0:g0 + size]
            room = self.ctx_max - max(int(ids.shape[1]) for ids in grp)      # (the group's common bound, as _generate_group's)
            limits = [min(mx, room, self.max_out) for mx in per[g0:g0 + size]]
            sc = None if scripts is None else scripts[g0:g0 + size]
            if max(limits) <= 0:
                outs += [ids.clone() for ids in grp]
                stats += [dict(steps=0, drafted=0, accepted=0) for _ in grp]
            elif len(grp) == 1:
                one = {} if samplings is None else dict(speculative_sampling=True)
                if samplings is not None and samplings[g0] is not None:
                    t, tk, tp_, sd, mp = samplings[g0]
                    one.update(do_sample=True, temperature=t, top_k=tk or None, top_p=tp_, seed=sd, min_p=mp)
                outs.append(self.generate(grp[0], max_new_tokens=limits[0], bad_words_ids=bad_words_ids, eos_token_id=eos_token_id,
                                          min_new_tokens=min_new_tokens, num_speculative_tokens=k, prompt_lookup_max=lookup_max,
                                          prompt_lookup_min=lookup_min, _spec_script=None if sc is None else sc[0], **one))
                stats.append(self.last_spec_stats)
            else:
                res, st = self._generate_spec_group(grp, limits, spec, sc, bad_words_ids, eos_token_id, min_new_tokens,
                                                    None if samplings is None else samplings[g0:g0 + size])
                outs, stats = outs + res, stats + st
        self.last_spec_stats = stats
        return outs

    def reset_prefix_cache(self):
        """vLLM's name: forget every reusable row, of the batch slots and of the single sequence (nothing on the device changes)."""
        for ds in self._batches.values():
            ds.reset_prefix()
        self._kv_ids, self._vt_upto = None, 0

    def _generate_group(self, ids_list, max_new_tokens, bad_words_ids, eos_token_id, min_new_tokens, logprobs=None, pens=None, edits=None):
        B = len(ids_list)
        # one penalised / edited sequence: the group runs on the penalised / edited step
        kind = step_kind(logprobs=logprobs, penalties=pens is not None and any(k is not None for k in pens),
                         edits=edits is not None and any(k is not None for k in edits))
        for ids in ids_list:
            if ids.dim() != 2 or ids.shape[0] != 1:
                raise ValueError("every prompt must be a LongTensor of shape [1, L]")
        ds = self.decode_slots(B)
        self.load_ban(bad_words_ids)
        L0 = [int(ids.shape[1]) for ids in ids_list]
        max_new = min(max_new_tokens, self.ctx_max - max(L0), self.max_out)
        if max_new <= 0:
            if logprobs is not None:
                self.last_logprobs += [None] * B
            return [ids.clone() for ids in ids_list]
        for b, ids in enumerate(ids_list):      # (greedy knobs: on the sampling step these picks run with top_k = 1)
            ds.admit(b, ids[0], kind, knobs=pens[b] if kind.penalties else None, edits=edits[b] if kind.edits else None)
        decode = ds.step_plan(kind)
        eos = stop_ids(eos_token_id)
        produced, ends = 1, [None] * B
        while True:
            toks = ds.tokens(produced)     # host sync point (EOS check)
            for b in range(B):
                if ends[b] is None:
                    ends[b] = stop_index(toks[b], eos, min_new_tokens)
            if all(e is not None for e in ends) or produced >= max_new:
                break
            n = min(CHUNK, max_new - produced)
            for _ in range(n):
                decode.run()
            produced += n
        res = []
        for b, ids in enumerate(ids_list):
            n = ends[b] if ends[b] is not None else min(produced, max_new)
            res.append(torch.cat([ids[0], torch.tensor(toks[b][:n], dtype=torch.long, device=ids.device)]).unsqueeze(0))
            if logprobs is not None:
                self.last_logprobs.append(ds.logprobs(b, n, logprobs))
        return res

    # ------------------------------------------------------------------ beam search
    def _beam_pick(self, rec, bm, nlive, advance_pos):
        """usdm_beam_step over the rows of the beam slots bm (slots.BeamSlots), a segment boundary, usdm_kv_reorder of every cache array by the parents
        the pick just wrote.  (The boundary costs nothing: a captured step joins its segments into one hipGraph.)"""
        H, d, L, Hq, Hkv, I, nq = self._dims()
        al = bm.all
        st = ops.decode_state(al.st_next, al.st_out, al.st_step, al.st_pos, advance_pos=advance_pos, batch=al.batch)
        ops.beam_step(bm.logits, st, V=self.v1 - self.v0, score=bm.score, parent=bm.parent, nlive=nlive, eos=bm.eos,
                      n_eos=bm.n_eos, log_score=bm.log_score, log_token=bm.log_token, log_parent=bm.log_parent,
                      cand_score=bm.cand_score, cand_index=bm.cand_index, embed=self.W["embed"], h_out=bm.h, Hd=H, plan=rec.plan)
        rec.plan.hold(st)
        rec.cut()
        ops.kv_reorder(bm.cache_arrays(), bm.parent, bm.lo, bm.pos, B=al.batch, nblk=L * Hkv, ctx_max=self.ctx_max, plan=rec.plan)

    def _generate_beam(self, input_ids, max_new_tokens, B, n, length_penalty, early_stopping, eos_list, pad_token_id, bad_words_ids,
                       ban_mask, keep_rows=False, on_step=None):
        """generate(num_beams=B): one prefill of the prompt into slot 0, whose pick is usdm_beam_step with row 0 live and whose
        usdm_kv_reorder (lo = 0, every parent 0) hands the prompt's rows to all slots; then per token ONE captured graph: the batched
        decode step of the B slots, usdm_beam_step, usdm_kv_reorder of the rows behind the prompt (lo = prompt length).  Every 8
        steps the host reads the new rows of the step log and replays HF's finished-beam bookkeeping on them (beam.BeamReplay);
        steps the device ran past HF's stopping point are not fed.
        keep_rows / on_step (tests; either one runs the step's two segments as plain launches instead of the graph): copy every step's
        [B][V] logits rows to self.last_beam_rows; call on_step(phase, bm) with phase "pick" between the pick and the reorder and "step"
        after it.  self.last_beam_replay keeps the BeamReplay (the step log's tokens and parents as the host saw them)."""
        from .beam import BeamReplay
        key = (B, len(eos_list))
        if key not in self._beams:
            self._beams[key] = BeamSlots(self, *key)
        bm = self._beams[key]
        L0, V = int(input_ids.shape[1]), self.v1 - self.v0
        self.load_ban(bad_words_ids, ban_mask)
        bm.eos.copy_(torch.tensor((eos_list + [0] * ops.BEAM_MAX_EOS)[:ops.BEAM_MAX_EOS], dtype=torch.int32))
        bm.pos.fill_(L0)
        bm.step.zero_()
        bm.score.zero_()
        bm.lo.zero_()
        segs, io = bm.prefill.get_or_build(L0, lambda: self._build_prefill(L0, True, slot=bm.slots[0], beam=bm))
        io["ids"].copy_(input_ids[0])
        rows = [] if keep_rows else None
        hooked = keep_rows or on_step is not None

        def run(step_segs):      # a list of segments (the prefill; the eager step) or the captured step
            if not hooked:
                return self._run_segs(step_segs) if isinstance(step_segs, list) else step_segs.run()
            *head, last = step_segs
            self._run_segs(head)
            if rows is not None:
                rows.append(bm.logits[:, :V].cpu().numpy().copy())
            if on_step is not None:
                on_step("pick", bm)
            last.run()
            if on_step is not None:
                on_step("step", bm)

        run(segs)      # prefill + first pick + the prompt's rows to every slot
        bm.lo.fill_(L0)
        if hooked and bm.beam_eager is None:
            bm.beam_eager = self._build_decode_batch(B, True, beam=bm)
        if not hooked and bm.beam_graph is None:
            bm.beam_graph = self._graphed(self._build_decode_batch(B, True, beam=bm))
        step = bm.beam_eager if hooked else bm.beam_graph
        rp = BeamReplay(B, eos_list, max_new_tokens, length_penalty, early_stopping)
        produced, fed = 1, 0
        while True:
            log = [t[fed:produced].cpu().numpy() for t in (bm.log_score, bm.log_token, bm.log_parent)]      # host sync point
            over = False
            for r in range(produced - fed):
                over = rp.feed(log[0][r], log[1][r], log[2][r])
                if over:
                    break
            fed = produced
            if over or produced >= max_new_tokens:
                break
            for _ in range(min(CHUNK, max_new_tokens - produced)):
                run(step)
                produced += 1
        seqs, scores = rp.results(n, pad_token_id)
        self.last_beam_scores = torch.from_numpy(scores)
        self.last_beam_rows = None if rows is None else rows[:rp.steps]
        self.last_beam_replay = rp
        gen = torch.tensor(seqs, dtype=torch.long, device=input_ids.device).view(n, -1)
        return torch.cat([input_ids[0].expand(n, -1), gen], 1)

    def _generate_spec(self, input_ids, ids_host, max_new, spec, script, dev_eos, eos, min_new, sampled=False, on_step=None):
        """The decode loop of generate(num_speculative_tokens=k) behind the prefill: the captured step is replayed in chunks and the
        host reads step / done after each, since a replay emits 1 .. k + 1 tokens.  A chunk never holds more replays than the
        remaining tokens could need at k + 1 per step, so no replay runs past the limit by the host's doing; replays past a
        device-side stop change nothing.  sampled: the step whose picks are drawn.  on_step (tests; sampled only):
        every chunk is ONE replay and on_step(dict(step=, drafts=, rows=, picks=)) gets host copies of the step word and the drafts
        the replay started from and of the T logits rows and picks it left."""
        k, lookup_max, lookup_min = spec
        T = k + 1
        if self._spec is None:
            self._spec = SpecSequence(self)
        sp = self._spec      # behind the prefill, whose pick is committed (step = 1): the call's words, then the first drafts and input rows
        sp.seed(0, input_ids[0], max_new, script)
        sp.set_lookup(lookup_max, lookup_min, script is not None)
        sp.propose(T, 0)
        step = sp.spec_step(T, sampled)
        if on_step is not None and not sampled:
            raise ValueError("_spec_on_step records logits rows, which only the sampled speculative step materialises")

        def recorded():      # one replay, its inputs and rows copied out
            rows = sp.sample_rows(T)
            before = dict(step=int(self.st_step.item()), drafts=sp.drafts[0, :T].tolist())
            step.run()
            on_step(dict(before, rows=rows["logits"].cpu().clone(), picks=rows["picks"].tolist()))
        while True:
            produced = min(int(self.st_step.item()), max_new)      # host sync point
            toks = self.st_out[:produced].tolist()
            end = stop_index(toks, eos, min_new)
            if end is not None:
                toks = toks[:end]
                break
            if produced >= max_new or int(self.st_done.item()):
                break
            if on_step is not None:
                recorded()
                continue
            for _ in range(max(1, min(CHUNK, -(-(max_new - produced) // T)))):
                step.run()
        if self.reuse_prefix:   # committed rows only: the prompt and every emitted token that was fed back and accepted
            self._kv_ids = ids_host + (self.st_out[:produced - 1].tolist() if produced > 1 else [])
        self.last_spec_stats = sp.stats(0)
        out = torch.cat([input_ids[0], torch.tensor(toks, dtype=torch.long, device=input_ids.device)])
        return out.unsqueeze(0)

    # ------------------------------------------------------------------ generate
    def _ban_mask(self, bad_words_ids):
        if not bad_words_ids:
            return self.ban_all_off
        key = id(bad_words_ids)
        hit = self._ban_cache.get(key)
        if hit is not None and hit[0] is bad_words_ids:
            return hit[1]
        m = torch.zeros(self.cfg["vocab_size"], dtype=torch.uint8)
        for w in bad_words_ids:
            if len(w) != 1:
                raise NotImplementedError("multi-token bad words are not used by the reference path (inference.py:41-45)")
            m[w[0]] = 1
        t = m[self.v0:self.v1].to(self.device).contiguous()
        self._ban_cache.put(key, (bad_words_ids, t))
        return t

    def load_ban(self, bad_words_ids=None, ban_mask=None):
        """The live ban mask, read by every plan and graph: ban_mask (a ready-made [vocab] 0/1 mask: serving's static processors) or else bad_words_ids."""
        self.ban.copy_(self._ban_mask(bad_words_ids) if ban_mask is None else ban_mask.to(torch.uint8)[self.v0:self.v1])

    def _max_new(self, L0, max_new_tokens, max_length):
        """generate()'s token budget: max_new_tokens, or else max_length - L0; at most what the context and the output row hold."""
        if max_new_tokens is None:
            if max_length is None:
                raise ValueError("max_length or max_new_tokens is required")
            max_new_tokens = max_length - L0
        return min(max_new_tokens, self.ctx_max - L0, self.max_out)

    def _setup_call(self, input_ids, past, sampling, bad_words_ids, eos_token_id, min_new_tokens, ban_mask=None, logprobs=None,
                    penalties=None, edits=None):
        """Per-call device state of generate(): prompt ids into the (cached) prefill plan, ban mask, position / step counters,
        device-side EOS list; penalties = the knobs (repetition, frequency, presence) of a penalised call, edits = check_edits()'s
        (bias, n) of a call with a logit bias or an n-gram ban.  Returns (prefill
        segments, the EOS ids the device checks).  (The call shape is the lockstep harnesses' too, which step several logical
        ranks through it: it takes the three values, not the kind.)"""
        kind = step_kind(sampling, logprobs, penalties is not None, edits is not None)
        L0, sampling = input_ids.shape[1], kind.sampling
        if self.tp_path:      # keep_logits: a sampled call exposes the gathered row, a greedy one this rank's shard
            if sampling and self.last_logits is not self.logits_row:
                self._shard_logits, self.last_logits = self.last_logits, self.logits_row
            elif not sampling and self.last_logits is self.logits_row:
                self.last_logits = self._shard_logits
        self._pick_state(kind)
        if kind.penalties:
            # the whole prompt is flagged, the ids whose K/V are reused from the cache included; zeroed together with st_step below
            seed_penalties(self._pen, input_ids[0], penalties)
        if kind.edits:
            seed_edits(self._edt, input_ids[0], edits)      # (the whole prompt, likewise)
        segs, io = self._prefill_plans.get_or_build((L0 - past, past, *kind), lambda: self._build_prefill(L0 - past, sampling, past=past,
                                                                                                          logprobs=kind.logprobs, penalties=kind.penalties,
                                                                                                          edits=kind.edits))
        if kind.logprobs is not None:
            self._lp["count"].zero_()      # rows written so far (usdm_logprobs keys its write on it: the device-side EOS)
        io["ids"].copy_(input_ids[0, past:])
        self._kv_ids, self._vt_upto = None, L0      # (set again once this call's decode steps are known)
        self.load_ban(bad_words_ids, ban_mask)
        self.st_pos.fill_(L0)
        self.st_step.zero_()
        block, dev_eos = stop_block(stop_ids(eos_token_id), min_new_tokens)      # more ids than the block holds: host-side check only
        self.st_eos.copy_(block)
        self.st_done.zero_()
        return segs, dev_eos

    @torch.no_grad()
    def generate(self, input_ids=None, max_length=None, do_sample=False, bad_words_ids=None, top_p=1.0, top_k=None,
                 temperature=1.0, eos_token_id=None, max_new_tokens=None, min_new_tokens=0, seed=None, ban_mask=None,
                 _logits_hook=None, logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0,
                 logit_bias=None, no_repeat_ngram_size=0, num_beams=None, num_return_sequences=None, length_penalty=1.0,
                 early_stopping=False, pad_token_id=None, _beam_keep_rows=False, _beam_on_step=None, num_speculative_tokens=None,
                 prompt_lookup_max=3, prompt_lookup_min=1, _spec_script=None, speculative_sampling=False, _spec_on_step=None, **unused):
        """Generation with the call shape of src/inference.py:63-83.  Greedy when do_sample is False or top_k == 1 (what the
        reference passes: arg-max of the ban-masked logits).  Otherwise temperature / top-k / top-p sampling on the device
        (usdm_sample_final).  `seed` keys its Philox stream; seed=None draws a fresh one from torch's global CPU generator,
        so calls differ from each other as HF sampling does and are reproducible under torch.manual_seed.
        logprobs=K (0 .. 20; None = off): self.last_logprobs is then the TokenLogprobs of the returned tokens, the first one (picked by
        the prefill) included - computed on the device inside the step (usdm_logprobs), before temperature / top-k / top-p.  A greedy
        call then runs on the sampling step with top_k = 1 (the arg-max path never materialises a logits row); its ids are the same.
        repetition_penalty r in (0, 2] (HF / vLLM: ids of the prompt and of the output so far), frequency_penalty and presence_penalty
        in [-2, 2] (vLLM: ids of the output so far): applied on the device to the ban-masked row of every step before the hook and
        the pick (usdm_penalize), so log-probabilities and last_logits are those of the penalised row.  With a
        non-neutral knob a greedy call runs on the sampling step with top_k = 1 too, and its ids may differ from the plain call's:
        that is the point.  All neutral (the default): no penalty plan is built, every launch is what it is without the arguments.
        min_p in [0, 1] (HF MinPLogitsWarper / vLLM; sampled calls): after temperature, top-k and top-p, ids with p < min_p * p_max
        are dropped (inside usdm_sample_final: no other plan; a greedy pick keeps the maximum anyway).
        logit_bias {id: bias} (at most 1024 ids, values clamped to [-100, 100]) and no_repeat_ngram_size n (HF
        NoRepeatNGramLogitsProcessor over prompt + output) run on the device in front of the penalties (usdm_logit_edit);
        a greedy call then runs on the sampling step with top_k = 1.  Both neutral (None / 0): no edit plan, no buffers.
        num_beams=B in 2 .. 16 (B <= max_batch(); None / 1: this call is what it is without the argument, no beam buffers and no
        beam plans are built): beam search on the device (usdm_beam_step, usdm_kv_reorder) with the semantics of the
        installed transformers' generate(num_beams=B, do_sample=False, renormalize_logits=True): num_return_sequences=n <= B (default
        1), length_penalty (default 1.0), early_stopping False / True / "never", at most 3 eos ids with max(2, 1 + n_eos) * B <= 32.
        The log-probabilities are normalised over the ALLOWED ids (banned lm_head rows are never streamed), which is HF's
        renormalize_logits=True; without bad_words_ids / ban_mask it is plain HF.  Returns [n][Lmax]: the prompt and each hypothesis,
        padded with pad_token_id (default: the first eos id); self.last_beam_scores holds HF's sequences_scores (float32 [n]).
        Not combined with (NotImplementedError): do_sample, logprobs, the penalties, logit_bias / no_repeat_ngram_size, min_p,
        _logits_hook, min_new_tokens > 0, tensor parallelism.  The single sequence's KV cache and its prefix reuse are not touched.
        num_speculative_tokens=k in 1 .. 7 (k + 1 <= max_batch(); None / 0: this call is what it is without the argument, no buffers
        and no plan are built): speculative greedy decoding with n-gram drafts (vLLM's speculative_config method
        "ngram").  Every step verifies k drafts of the sequence's own continuation in ONE pass over the weights and emits 1 .. k + 1
        tokens; the drafts follow the most recent earlier occurrence of the last prompt_lookup_max .. prompt_lookup_min tokens of
        prompt + output, found on the device.  The ids do not depend on the drafts (usdm_attn_verify is position-invariant by
        construction); against the plain call they are equal up to near-ties of the logits, as generate_batch's are (k + 1 <= 4 rows
        run the VALU projections, bit-identical per row with the single step; more rows the matrix cores).  self.last_spec_stats =
        dict(steps=, drafted=, accepted=) counts the speculative steps, the drafts fed (ids, not the -1 of "no draft") and the drafts
        accepted: tokens emitted by the steps = steps + accepted (the prefill's pick is the call's first token and no step).
        _spec_script (tests, tools/spec_rate.py): an int sequence / tensor whose entry j replaces the lookup as the draft for output j.
        Not combined with (NotImplementedError): sampling with top_k != 1, logprobs, the penalties, logit_bias / no_repeat_ngram_size,
        min_p, _logits_hook, num_beams > 1, tensor parallelism, kv_cache_dtype="fp8".  Cache rows behind the committed position are
        dead; prefix reuse after the call counts committed rows only.
        speculative_sampling=True (with num_speculative_tokens=k; default False: everything above holds as it stands): speculation for
        SAMPLED calls.  The step materialises its k + 1 logits rows, usdm_spec_sample draws row i with the call's
        knobs and seed at the Philox counter of ITS position - the token the plain sampled call draws there - and a draft is accepted
        iff it equals that draw.  The output distribution is the plain sampled call's, and for a fixed seed the ids do not depend on
        the drafts.  do_sample with top_k != 1 and min_p are then allowed; a greedy call runs on the same step with top_k = 1 (the ids
        of the greedy speculative call).  Still refused: logprobs, the penalties, logit_bias / no_repeat_ngram_size, _logits_hook,
        num_beams > 1, tensor parallelism, kv_cache_dtype="fp8".  _spec_on_step (tests): see _generate_spec."""
        from .spec import check_spec_args, check_spec_call, check_speculative_sampling
        spec = check_spec_args(num_speculative_tokens, prompt_lookup_max, prompt_lookup_min)
        spec_sampled = check_speculative_sampling(speculative_sampling, spec is not None)
        lpk = check_logprobs(logprobs)
        pen = check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        min_p = check_min_p(min_p)
        edt = check_edits(logit_bias, no_repeat_ngram_size, self.cfg["vocab_size"])
        self.last_logprobs = self.last_beam_scores = self.last_spec_stats = None
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("input_ids must be a LongTensor of shape [1, L] (batch 1, as the reference calls it)")
        if spec is not None:
            check_spec_call(bool(do_sample) and top_k != 1, lpk, pen, edt, min_p, _logits_hook, num_beams, self.tp_path, self.kv8,
                            speculative_sampling=spec_sampled)
            self._check_spec_shape(spec[0])
        if num_beams is not None and num_beams != 1:
            from .beam import check_beam_args, check_beam_call
            eos_list = list(dict.fromkeys(int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else
                                                          ([] if eos_token_id is None else [eos_token_id]))))
            B, n, length_penalty, early_stopping, _ = check_beam_args(num_beams, num_return_sequences, length_penalty, early_stopping,
                                                                      len(eos_list), self.v1 - self.v0)
            check_beam_call(do_sample, lpk, pen, edt, min_p, _logits_hook, min_new_tokens, self.tp_path)
            if temperature != 1.0 or top_p != 1.0:
                raise ValueError("temperature / top_p only apply with do_sample=True")
            if B > self.max_batch():
                raise ValueError(f"num_beams={B}: a decode step of this model takes at most {self.max_batch()} sequences")
            max_new_tokens = self._max_new(input_ids.shape[1], max_new_tokens, max_length)
            if max_new_tokens <= 0:
                return input_ids.expand(n, -1).clone()
            return self._generate_beam(input_ids, max_new_tokens, B, n, length_penalty, early_stopping, eos_list, pad_token_id,
                                       bad_words_ids, ban_mask, keep_rows=_beam_keep_rows, on_step=_beam_on_step)
        if num_return_sequences not in (None, 1):
            raise ValueError("num_return_sequences > 1 needs num_beams > 1")
        sampling = False
        if _logits_hook is not None:      # arbitrary Python logits processors: eager steps, knobs still on the device
            if seed is None:
                seed = self._agree_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))
            sampling, self.logits_hook = "hook", _logits_hook
            ops.set_sample_params(self.sample_params, temperature if do_sample else 1.0, int(top_k or 0) if do_sample else 1,
                                  top_p if do_sample else 1.0, seed, min_p=min_p if do_sample else 0.0)
        elif do_sample and top_k != 1:
            if not (temperature > 0) or not (0 < top_p <= 1):
                raise ValueError("temperature must be > 0 and top_p in (0, 1]")
            if seed is None:
                seed = self._agree_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))
            sampling = True
            ops.set_sample_params(self.sample_params, temperature, int(top_k or 0), top_p, seed, min_p=min_p)
        else:
            if (temperature != 1.0 or top_p != 1.0) and not do_sample:
                raise ValueError("temperature / top_p only apply with do_sample=True")
        kind = step_kind(sampling or spec_sampled, lpk, pen is not None, edt is not None)      # (sampled speculation: the prefill's pick is the sampler's)
        if kind.sampling and not sampling:      # greedy on the sampling step: top_k = 1
            ops.set_sample_params(self.sample_params, 1.0, 1, 1.0, 0)
        max_new_tokens = self._max_new(input_ids.shape[1], max_new_tokens, max_length)
        if max_new_tokens <= 0:
            return input_ids.clone()
        ids_host, past = self._reused_past(input_ids, input_ids.shape[1] - 1)      # (the last token is always prefilled: its row yields the first pick)
        segs, dev_eos = self._setup_call(input_ids, past, kind.sampling, bad_words_ids, eos_token_id, min_new_tokens, ban_mask=ban_mask,
                                          logprobs=lpk, penalties=pen, edits=edt)
        self._run_segs(segs)  # prefill + first token
        if spec is not None:
            return self._generate_spec(input_ids, ids_host, max_new_tokens, spec, _spec_script, dev_eos, stop_ids(eos_token_id), min_new_tokens,
                                       sampled=spec_sampled, on_step=_spec_on_step)
        if kind not in self._decodes:      # a plan / graph of its own per kind (the hooked step has host code inside: never captured)
            self._decodes[kind] = self._graphed(self._build_decode(*kind), enabled=False if kind.sampling == "hook" else None)
        self._decode = self._decodes[kind]
        eos = stop_ids(eos_token_id)
        produced = 1
        toks = []
        while True:
            n_dev = int(self.st_step.item()) if dev_eos else produced   # steps past a device-side EOS did not run
            produced = min(produced, n_dev)
            toks = self.st_out[:produced].tolist()  # host sync point (EOS check)
            if self.p2p is not None:
                self.p2p.raise_if_failed()          # a peer that never delivered surfaces here, not as a hang
            if self.chain and int(self.chain_sync[:, 1].sum().item()):
                raise RuntimeError("usdm_gemv_chain: a grid barrier timed out (the persistent decode kernel was not fully resident); "
                                   "results are invalid - rerun with USDM_GEMV_CHAIN=0")
            if self.cmb_err is not None and int(self.cmb_err.item()):
                raise RuntimeError("usdm_gemv (cmb_gran): the in-launch attention hand-off timed out (the o_proj launch was not fully "
                                   "resident); results are invalid - rerun with USDM_ATTN_CMB=0")
            end = stop_index(toks, eos, min_new_tokens)
            if end is not None:
                toks = toks[:end]
                break
            if produced >= max_new_tokens:
                toks = toks[:max_new_tokens]
                break
            n = min(CHUNK, max_new_tokens - produced)
            for _ in range(n):
                self._decode.run()
            produced += n
        if self.reuse_prefix:   # ids whose K/V now sit in the cache: the prompt and every generated token that was fed back
            fed = self.st_out[:produced - 1].tolist() if produced > 1 else []
            self._kv_ids = ids_host + fed
        if lpk is not None:
            self.last_logprobs = read_logprobs(self._lp, len(toks), lpk)
        out = torch.cat([input_ids[0], torch.tensor(toks, dtype=torch.long, device=input_ids.device)])
        return out.unsqueeze(0)
