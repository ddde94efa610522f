"""vLLM-style serving surface of the speech-text LLM (reference: src/inference_vllm.py:42-66,70-83,109-125 and the demo's
knobs, src/streamlit_demo.py:201-211,258-287): `LLM(model=..., download_dir=...)`, `SamplingParams(max_tokens, top_p, top_k,
temperature, stop_token_ids, logits_processors)`, `llm.generate(prompts, sampling_params) -> [RequestOutput]` with
`.outputs[0].text / .token_ids`, on top of usdm_amd.llm.USDMForCausalLM.

How requests are executed
  * logits processors that are STATIC masks (the reference's three `bad_word_processor_*` only write -inf into fixed id ranges)
    are recognised by probing and turned into the device-side ban mask: banned lm_head rows are not even streamed, and the
    decode step stays one hipGraph;
  * several requests that share a mask - greedy (top_k = 1 / temperature = 0, what the reference passes) AND sampled - are served by
    CONTINUOUS BATCHING over the 16 sequence slots of the batched decode (usdm_gemv_batch: the weights are streamed once per step
    for all slots; 4 slots for groups of <= 4 requests): a finished sequence's slot is refilled from the queue at the next scheduling point (every 8 steps) while
    the other slots keep decoding.  Sampling state is PER SLOT (usdm_sample_final's batched form: every slot has its own
    temperature / top-k / top-p / seed block on the device and its own Philox counter), so a request sampled inside a batch
    returns exactly the tokens it returns alone; a greedy request in a sampled batch carries top_k = 1;
  * a single request uses the single-sequence graph (usdm_sample_final: temperature / top-k / top-p on the device, `seed` per
    request);
  * under tensor parallelism both forms sample as well: every rank gathers the full ban-masked logits row (the ranks' lm_head
    shards) and draws from it with the same seed and step, so every rank picks the same token; a seed left to the server is
    rank 0's draw on every rank.  Processors that depend on the history are not supported there (they would see one shard);
  * SamplingParams(repetition_penalty=, presence_penalty=, frequency_penalty=) - the history-dependent processors every HF / vLLM
    user reaches for - run on the device inside the step (usdm_penalize, in front of the pick): graph-captured,
    continuously batched and tensor parallel like any other request.  One penalised request puts its whole group on the penalised
    step, which is also the sampling step; the other slots carry neutral knobs, which leave every bit of their rows alone;
  * SamplingParams(min_p=, logit_bias=, no_repeat_ngram_size=) run on the device too: min_p inside the sampler, per slot, next to
    top-k and top-p; the logit bias and HF's n-gram ban in usdm_logit_edit, in front of the penalties.  One request
    with a bias or an n-gram size puts its group on the step with that launch; the other slots' neutral blocks leave their rows alone;
  * other processors that really depend on the token history run as Python between the lm_head launch and the pick of every step
    (eager launches: correct, not fast); with penalties they get both, the processors seeing the penalised row;
  * LLM.score(prompt_token_ids, top_logprobs=K, start=...) scores tokens that were GIVEN (vLLM's prompt_logprobs, as an entry point of
    its own: nothing is generated): one prefill, the lm_head over every scored row, usdm_prompt_logprobs on the device;
  * SamplingParams(logprobs=K), K = 0 .. 20: per-token log-probabilities computed on the device inside the step (usdm_logprobs, right
    after the pick, on the row it drew from): lp(i) = x_i - logsumexp(x) over the ban-masked logits, i.e. the model's distribution
    over the allowed ids BEFORE temperature / top-k / top-p.  One asking request puts its whole group on the log-probability step
    (K = the group's maximum, trimmed per request on the host); a greedy request then runs on the sampling step with top_k = 1;
  * LLM(enable_prefix_caching=True) (vLLM's keyword; opt-in): a request admitted into a slot reuses the prefill-written
    rows of the longest prefix (>= 16 tokens) that any slot holds - a slot still decoding included - and prefills the rest; rows of
    another slot are copied on the device (usdm_kv_reorder), idle slots are parked behind their cached rows.  bf16 cache: every
    request returns exactly what it returns with the option off.  stats: prefix_hits, prefix_rows_reused, prefill_rows.
"""
import os
from collections import deque

import torch

from .llm import USDMForCausalLM, check_edits, check_logprobs, check_min_p, check_penalties, check_quantization, step_kind, stop_index
from .quant import check_kv_cache_dtype
from .slots import CHUNK

MAX_SLOTS = 16      # usdm_gemv_batch streams the weights once per step for up to 16 sequences (matrix-core form above 4)
SMALL_SLOTS = 4     # groups of <= 4 requests use the 4-slot plan (VALU form: per slot bit-identical with the single-request path)


class SamplingParams:
    """The subset of vllm.SamplingParams the reference and its demo use (inference_vllm.py:109-123)."""

    def __init__(self, n=1, temperature=1.0, top_p=1.0, top_k=-1, max_tokens=16, min_tokens=0, stop_token_ids=None,
                 logits_processors=None, seed=None, skip_special_tokens=True, ignore_eos=False, static_logits_mask=None, logprobs=None,
                 prompt_logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, logit_bias=None,
                 no_repeat_ngram_size=0, **unused):
        if not isinstance(n, int) or n < 1:
            raise ValueError("n must be a positive integer")
        if temperature < 0 or not (0 < top_p <= 1) or (top_k < -1 or top_k == 0):
            raise ValueError("temperature >= 0, 0 < top_p <= 1, top_k = -1 (off) or >= 1")
        self.n, self.temperature, self.top_p, self.top_k = n, float(temperature), float(top_p), int(top_k)
        self.max_tokens, self.min_tokens = int(max_tokens), int(min_tokens)
        self.stop_token_ids = list(stop_token_ids or [])
        self.logits_processors = list(logits_processors or [])
        self.seed, self.skip_special_tokens, self.ignore_eos = seed, skip_special_tokens, ignore_eos
        self.static_logits_mask = static_logits_mask      # None: probe the processors; True / False: caller's word
        # logprobs (vllm's name): None, or the number of most likely ids reported per generated token next to the picked one, 0 .. 20
        self.logprobs = check_logprobs(logprobs)
        # vllm's penalties: repetition in (0, 2] over prompt + output ids, presence / frequency in [-2, 2] over output ids (usdm_penalize)
        self.penalties = check_penalties(repetition_penalty, presence_penalty, frequency_penalty)      # None: all neutral
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = (
            float(repetition_penalty), float(presence_penalty), float(frequency_penalty))
        # min_p in [0, 1] (inside usdm_sample_final); logit_bias {id: bias in [-100, 100] after clamping} and HF's no_repeat_ngram_size
        # (usdm_logit_edit).  The ids' upper bound is the model's vocabulary: checked when the request is served
        self.min_p = check_min_p(min_p)
        self.edits = check_edits(logit_bias, no_repeat_ngram_size)      # None: both neutral
        self.logit_bias, self.no_repeat_ngram_size = (dict(logit_bias) if logit_bias else None), int(no_repeat_ngram_size or 0)
        if prompt_logprobs is not None:
            raise NotImplementedError("prompt_logprobs is not supported as a SamplingParams field (it needs the lm_head over every prompt row, "
                                      "which a generating request does not run); logprobs= covers the generated tokens - to score given "
                                      "tokens use LLM.score() / USDMForCausalLM.score()")
        if self.n > 1 and self.greedy:
            raise ValueError("n must be 1 when using greedy sampling (the n completions would be identical)")   # as vllm

    @property
    def greedy(self):
        return self.temperature == 0.0 or self.top_k == 1


class Logprob:
    """vllm.sequence.Logprob: log-probability, rank (1 = most likely) and text of one candidate token."""
    __slots__ = ("logprob", "rank", "decoded_token")

    def __init__(self, logprob, rank=None, decoded_token=None):
        self.logprob, self.rank, self.decoded_token = logprob, rank, decoded_token

    def __eq__(self, other):
        return isinstance(other, Logprob) and (self.logprob, self.rank, self.decoded_token) == (other.logprob, other.rank, other.decoded_token)

    def __repr__(self):
        return f"Logprob(logprob={self.logprob}, rank={self.rank}, decoded_token={self.decoded_token!r})"


def assemble_logprobs(token_ids, tok_lp, tok_rank, top_id, top_lp, k, tokenizer=None):
    """vLLM's CompletionOutput.logprobs / .cumulative_logprob from the device's rows (sequences or tensors; top_id / top_lp are [n][>= k]
    in descending log-probability, id -1 = padding): per generated token a dict {token_id: Logprob} holding the picked token and the k
    most likely ones - k entries when the pick is among them, else k + 1 - and the float64 sum of the picked tokens' log-probabilities.
    Entry j of the top list has rank j + 1 (its position; among exactly tied logits that is the lowest-id-first order, while the
    picked token carries vLLM's rank: 1 + the number of strictly greater logits)."""
    lst = lambda t: t.tolist() if hasattr(t, "tolist") else list(t)
    tok_lp, tok_rank, top_id, top_lp = lst(tok_lp), lst(tok_rank), lst(top_id), lst(top_lp)
    text = (lambda i: tokenizer.decode([i])) if tokenizer is not None else (lambda i: None)
    out, total = [], 0.0
    for t, tok in enumerate(token_ids):
        d = {int(tok): Logprob(float(tok_lp[t]), int(tok_rank[t]), text(int(tok)))}
        for j in range(k):
            i = int(top_id[t][j])
            if i >= 0 and i != tok:
                d[i] = Logprob(float(top_lp[t][j]), j + 1, text(i))
        out.append(d)
        total += float(tok_lp[t])
    return out, total


class CompletionOutput:
    def __init__(self, index, text, token_ids, finish_reason, stop_reason=None, cumulative_logprob=None, logprobs=None):
        self.index, self.text, self.token_ids, self.finish_reason, self.stop_reason = index, text, token_ids, finish_reason, stop_reason
        self.cumulative_logprob, self.logprobs = cumulative_logprob, logprobs

    def __repr__(self):
        return f"CompletionOutput(index={self.index}, text={self.text!r}, token_ids={self.token_ids}, finish_reason={self.finish_reason})"


class ScoreOutput:
    """One scored prompt (LLM.score): prompt_token_ids, prompt_logprobs in vLLM's shape - None for the `start` leading tokens that were
    not scored, then per token the dict {token_id: Logprob} of assemble_logprobs - and cumulative_logprob, the float64 sum over the
    scored tokens."""

    def __init__(self, prompt, prompt_token_ids, prompt_logprobs, cumulative_logprob):
        self.prompt, self.prompt_token_ids, self.prompt_logprobs, self.cumulative_logprob = prompt, prompt_token_ids, prompt_logprobs, cumulative_logprob

    def __repr__(self):
        return f"ScoreOutput(tokens={len(self.prompt_token_ids)}, cumulative_logprob={self.cumulative_logprob})"


def assemble_score(prompt_token_ids, start, lp, k, tokenizer=None, prompt=None):
    """ScoreOutput of a prompt whose tokens start .. L-1 were scored into the TokenLogprobs (or any object with its four row fields) lp."""
    ids = list(prompt_token_ids)
    rows, total = assemble_logprobs(ids[start:], lp.token_logprobs, lp.ranks, lp.top_ids, lp.top_logprobs, k, tokenizer)
    return ScoreOutput(prompt, ids, [None] * start + rows, total)


class BeamSearchParams:
    """vllm.sampling_params.BeamSearchParams(beam_width, max_tokens, ignore_eos=False, length_penalty=1.0), plus what a request of this
    package carries next to it: stop_token_ids (at most 3 stop ids in all, the tokenizer's EOS included unless ignore_eos) and the
    static -inf mask, as logits_processors that are one (static_mask_of) or a ready-made static_logits_mask [vocab] of 0 / 1."""

    def __init__(self, beam_width, max_tokens, ignore_eos=False, temperature=0.0, length_penalty=1.0, stop_token_ids=None,
                 logits_processors=None, static_logits_mask=None):
        if temperature not in (0, 0.0):
            raise NotImplementedError("beam search with a temperature is not supported (the search ranks exact log-probabilities)")
        self.beam_width, self.max_tokens, self.ignore_eos, self.temperature = beam_width, int(max_tokens), bool(ignore_eos), 0.0
        self.length_penalty = length_penalty
        self.stop_token_ids, self.logits_processors, self.static_logits_mask = list(stop_token_ids or []), logits_processors, static_logits_mask


class BeamSearchSequence:
    """One hypothesis: tokens = prompt + generated ids (its stop id included), cum_logprob = the sum of its tokens' log-probabilities
    (HF's sequences_scores x length ** length_penalty), text = the decoded generated ids (None without a tokenizer)"""

    def __init__(self, tokens, cum_logprob, text=None):
        self.tokens, self.cum_logprob, self.text = tokens, cum_logprob, text

    def __repr__(self):
        return f"BeamSearchSequence(tokens={self.tokens!r}, cum_logprob={self.cum_logprob!r}, text={self.text!r})"


class BeamSearchOutput:
    def __init__(self, sequences):
        self.sequences = sequences

    def __repr__(self):
        return f"BeamSearchOutput(sequences={self.sequences!r})"


class RequestOutput:
    def __init__(self, request_id, prompt, prompt_token_ids, outputs):
        self.request_id, self.prompt, self.prompt_token_ids, self.outputs, self.finished = request_id, prompt, prompt_token_ids, outputs, True

    def __repr__(self):
        return f"RequestOutput(request_id={self.request_id}, outputs={self.outputs})"


def static_mask_of(processors, vocab, device):
    """If the processors only ever write -inf into a FIXED set of ids (and leave every other logit alone), return that set as a
    0/1 uint8 mask [vocab]; else None.  Decided by probing with several histories / logit vectors (a heuristic: a processor that
    reacts only to some particular history can pass; SamplingParams(static_logits_mask=False) forces the general path)."""
    if not processors:
        return torch.zeros(vocab, dtype=torch.uint8, device=device)
    g = torch.Generator().manual_seed(0)
    hists = [[], [vocab - 1], [5, vocab // 2, 3, vocab // 2], [vocab // 3] * 9 + [vocab - 2], list(range(7, min(vocab, 39)))]
    probes = [(h, torch.zeros(vocab) if i == 0 else torch.randn(vocab, generator=g)) for i, h in enumerate(hists)]
    masks = []
    for hist, lg in probes:
        out = lg.clone().to(device)
        for p in processors:
            out = p(list(hist), out)
        if not torch.is_tensor(out) or out.shape != (vocab,):
            return None
        out = out.float().cpu()
        m = torch.isneginf(out)
        if not torch.equal(out[~m], lg[~m]):
            return None
        masks.append(m)
    if any(not torch.equal(masks[0], m) for m in masks[1:]):
        return None
    return masks[0].to(torch.uint8).to(device)


class LLM:
    """`LLM(model='naver-ai/USDM-DailyTalk', download_dir=cache)` as in inference_vllm.py:105 (hub names resolve inside
    download_dir), or `LLM(model=<USDMForCausalLM>, tokenizer=<tokenizer>)` around objects that are already loaded."""

    spec_sampling = False      # speculative_config's "speculative_sampling" (DESIGN.md 8k-3); off unless __init__ reads it from the config

    def __init__(self, model, tokenizer=None, download_dir=None, gpu_memory_utilization=0.9, max_model_len=None, device="cuda",
                 dtype="bfloat16", max_num_seqs=MAX_SLOTS, quantization=None, fp8_matrix_cores=False, kv_cache_dtype=None,
                 enable_prefix_caching=False, speculative_config=None, mxfp4_matrix_cores=False, **unused):
        # max_num_seqs (vllm's name): sequences decoded per step, 1..16.  <= 4: the VALU batch kernel (per slot bit-identical with the
        # single-request path); above: the matrix-core form (usdm_gemv_batch form 1)
        self.max_slots = max(1, min(int(max_num_seqs), MAX_SLOTS))
        # quantization (vllm's name): None = bf16, "fp8" = e4m3 weights with power-of-two row scales (usdm_amd/quant.py); the
        # FP8 model decodes at most 4 sequences per step (its max_batch()) unless fp8_matrix_cores (opt-in) runs steps of 5..16
        # sequences on the matrix cores (usdm_gemv_fp8_mfma)
        # "mxfp4" = e2m1 weights with one power-of-two scale per 32 elements (fp8 lm_head): at most 4 sequences per step unless
        # mxfp4_matrix_cores (opt-in) runs steps of 5..16 sequences on the matrix cores (usdm_gemv_mxfp4_mfma, a second image of the codes)
        check_quantization(quantization, fp8_matrix_cores, mxfp4_matrix_cores)
        # kv_cache_dtype (vllm's name): None / "bf16", or "fp8" = e4m3 cache rows with one power-of-two scale per (token, kv head)
        kvd = check_kv_cache_dtype(kv_cache_dtype)
        if isinstance(model, USDMForCausalLM):
            if kv_cache_dtype is not None and model.kv_cache_dtype != kvd:
                raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}, but the model object was loaded with "
                                 f"kv_cache_dtype={model.kv_cache_dtype!r}")
            if quantization is not None and model.quantization != quantization:
                raise ValueError(f"quantization={quantization!r}, but the model object was loaded with "
                                 f"quantization={model.quantization!r}")
            if fp8_matrix_cores and not model.fp8_matrix_cores:
                raise ValueError("fp8_matrix_cores=True, but the model object was loaded with fp8_matrix_cores=False")
            if mxfp4_matrix_cores and not model.mxfp4_matrix_cores:
                raise ValueError("mxfp4_matrix_cores=True, but the model object was loaded with mxfp4_matrix_cores=False")
            if enable_prefix_caching and not model.prefix_caching:
                raise ValueError("enable_prefix_caching=True, but the model object was loaded with enable_prefix_caching=False")
            self.llm = model
        else:
            from .checkpoints import resolve_local
            path = model if os.path.isdir(str(model)) else resolve_local(download_dir or ".", model, must_contain=("config.json",))
            if tokenizer is None:
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(path, local_files_only=True)
            ctx = min(int(max_model_len or getattr(tokenizer, "model_max_length", 4096) or 4096), 8192)
            self.llm = USDMForCausalLM.from_pretrained(path, device=device, ctx_max=ctx, quantization=quantization,
                                                       fp8_matrix_cores=fp8_matrix_cores, mxfp4_matrix_cores=mxfp4_matrix_cores,
                                                       kv_cache_dtype=kv_cache_dtype,
                                                       enable_prefix_caching=enable_prefix_caching)
        if isinstance(tokenizer, str):
            from transformers import AutoTokenizer
            tokenizer = AutoTokenizer.from_pretrained(tokenizer, local_files_only=True)
        self.tokenizer = tokenizer
        self.stats = dict(requests=0, batched_requests=0, admissions=0, max_active=0, batched_steps=0, hook_requests=0)
        # enable_prefix_caching (vLLM's name): an admitted prompt reuses the rows of the longest prefix that any slot
        # holds.  prefix_hits = admissions that reused rows, prefix_rows_reused / prefill_rows = rows reused / prefilled, prefix_copies =
        # hits served from another slot (usdm_kv_reorder), prefix_hits_live = hits whose source slot was still decoding;
        # admission_log = the last (slot, prompt ids) admissions in order (what a PrefixIndex replays)
        self.prefix_caching = self.llm.prefix_caching
        if self.prefix_caching:
            self.stats.update(prefix_hits=0, prefix_rows_reused=0, prefill_rows=0, prefix_copies=0, prefix_hits_live=0)
            self.admission_log = deque(maxlen=256)
        # speculative_config (vLLM's name and shape): {"method": "ngram", "num_speculative_tokens": k, "prompt_lookup_max": ..,
        # "prompt_lookup_min": ..} - greedy requests with a static mask run on the speculative step: two or more of a group share the
        # speculative slots (slots.SpecSlots), one that is alone runs generate(num_speculative_tokens=k);
        # everything else runs as without the option.  "speculative_sampling": True makes sampled requests, min_p
        # included, eligible too: a group with one of them runs the sampled speculative step (its greedy members with top_k = 1)
        from .spec import check_spec_call, check_speculative_config, config_speculative_sampling
        self.spec = check_speculative_config(speculative_config)
        self.spec_sampling = config_speculative_sampling(speculative_config)
        if self.spec is not None:
            check_spec_call(tensor_parallel=self.llm.tp_path, kv_cache_fp8=self.llm.kv8)
            if self.spec[0] + 1 > self.llm.max_batch():
                raise ValueError(f"num_speculative_tokens={self.spec[0]}: a decode step of this model takes at most {self.llm.max_batch()} rows")
            # spec_requests: served alone on the single-sequence speculative step; spec_batched_requests: served through the speculative
            # slots (counted in batched_requests too), spec_max_active: the most of them decoding in one step;
            # spec_steps / spec_drafted / spec_accepted: per-sequence steps, drafts fed and drafts accepted of both
            self.stats.update(spec_requests=0, spec_steps=0, spec_drafted=0, spec_accepted=0, spec_batched_requests=0, spec_max_active=0)
            if self.spec_sampling:      # sampled requests served on a speculative step, alone or through the slots
                self.stats.update(spec_sampled_requests=0)
        self._next_id = 0

    def get_tokenizer(self):
        return self.tokenizer

    def reset_prefix_cache(self):
        """vLLM's name: forget every cached prefix (enable_prefix_caching); later prompts prefill all their rows again."""
        self.llm.reset_prefix_cache()
        return True

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def generate(self, prompts=None, sampling_params=None, prompt_token_ids=None, use_tqdm=False):
        if prompts is None and prompt_token_ids is None:
            raise ValueError("prompts or prompt_token_ids is required")
        if isinstance(prompts, str):
            prompts = [prompts]
        if prompt_token_ids is not None and prompt_token_ids and isinstance(prompt_token_ids[0], int):
            prompt_token_ids = [prompt_token_ids]
        n = len(prompts) if prompts is not None else len(prompt_token_ids)
        sps = sampling_params if isinstance(sampling_params, (list, tuple)) else [sampling_params or SamplingParams()] * n
        if len(sps) != n:
            raise ValueError("one SamplingParams per prompt (or a single one for all)")
        dev, V = self.llm.device, self.llm.cfg["vocab_size"]
        reqs = []
        for i in range(n):
            if prompt_token_ids is not None:
                ids = list(prompt_token_ids[i])
                text = prompts[i] if prompts is not None else None
            else:
                if self.tokenizer is None:
                    raise ValueError("text prompts need a tokenizer")
                text = prompts[i]
                ids = list(self.tokenizer(text).input_ids)
            sp = sps[i]
            check_edits(sp.logit_bias, sp.no_repeat_ngram_size, V)      # (ids against this model's vocabulary)
            mask = sp.static_logits_mask
            if mask is None or mask is True:
                m = static_mask_of(sp.logits_processors, V, dev)
                if m is None and mask is True:
                    raise ValueError("static_logits_mask=True but the processors are not a fixed -inf mask")
                mask = m
            else:
                mask = None if sp.logits_processors else torch.zeros(V, dtype=torch.uint8, device=dev)
            stops = set(sp.stop_token_ids)
            eos = getattr(self.tokenizer, "eos_token_id", None)
            if eos is not None and not sp.ignore_eos:
                stops.add(int(eos))
            room = self.llm.ctx_max - len(ids)
            seed = sp.seed
            if not sp.greedy and seed is None:      # as generate(): a fresh stream per call, reproducible under torch.manual_seed
                # (tensor parallel: rank 0's draw on every rank, so that all ranks sample the same tokens)
                seed = self.llm._agree_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))
            # n > 1 (vllm.SamplingParams.n): the request fans out into n sequences that share prompt, knobs and mask and draw from
            # the Philox streams seed, seed + 1, ...: completion j is exactly what a single request with seed + j returns, and the
            # copies ride the continuous batch like any other requests (the prompt is prefilled once per copy; with
            # enable_prefix_caching copies 2 .. n find it in copy 1's slot and prefill one row)
            for j in range(sp.n):
                reqs.append(dict(i=(i, j), rid=str(self._next_id + i), text=text, ids=ids, sp=sp, mask=mask, stops=stops,
                                 seed=(seed + j) if seed is not None else None,
                                 max_new=max(0, min(sp.max_tokens, room, self.llm.max_out))))
        self._next_id += n
        self.stats["requests"] += n
        done = {}
        # continuous batching: requests with the same static mask (greedy and sampled alike), at least two of them
        groups = {}
        for r in reqs:
            # (tensor parallel: every rank serves the same request list with the same seeds and sees the same tokens, so all ranks
            # take the same scheduling decisions)
            if r["mask"] is not None and r["max_new"] > 0:
                groups.setdefault(bytes(r["mask"].cpu().numpy().tobytes()), []).append(r)
        for grp in groups.values():
            if len(grp) >= 2:
                fast, grp = self._spec_split(grp)
                for r, toks, why, lp in (self._run_spec_batched(fast) if fast else []) + (self._run_batched(grp) if grp else []):
                    done[r["i"]] = (toks, why, lp)
        for r in reqs:
            if r["i"] not in done:
                done[r["i"]] = self._run_single(r)
        outs = []
        for r in reqs:
            if r["i"][1] == 0:
                outs.append(RequestOutput(r["rid"], r["text"], r["ids"], []))
            outs[-1].outputs.append(self._finish(r, *done[r["i"]]))
        return outs

    @torch.no_grad()
    def beam_search(self, prompts, params):
        """vLLM's LLM.beam_search(prompts, BeamSearchParams): one BeamSearchOutput per prompt with its beam_width best hypotheses, best
        first.  prompts: a text, a list of token ids, {"prompt": text} / {"prompt_token_ids": ids}, or a list of those.  One request
        at a time, each one USDMForCausalLM.generate(num_beams=beam_width, num_return_sequences=beam_width, length_penalty=...,
        early_stopping=False) over the request's static mask and stop ids; the hypotheses are ordered by HF's
        length-normalised score, cum_logprob is the unnormalised sum."""
        llm = self.llm
        if isinstance(prompts, (str, dict)) or (isinstance(prompts, (list, tuple)) and prompts and isinstance(prompts[0], int)):
            prompts = [prompts]
        V, outs = llm.cfg["vocab_size"], []
        mask = params.static_logits_mask
        if mask is None or mask is True:
            mask = static_mask_of(params.logits_processors, V, llm.device)
            if mask is None and params.logits_processors:
                raise NotImplementedError("beam search takes a static -inf mask only: these logits processors are not one")
        stops = list(dict.fromkeys(int(t) for t in params.stop_token_ids))
        eos = getattr(self.tokenizer, "eos_token_id", None)
        if eos is not None and not params.ignore_eos and int(eos) not in stops:
            stops.insert(0, int(eos))
        for p in prompts:
            if isinstance(p, dict):
                p = p["prompt_token_ids"] if p.get("prompt_token_ids") is not None else p["prompt"]
            if isinstance(p, str):
                if self.tokenizer is None:
                    raise ValueError("text prompts need a tokenizer")
                p = self.tokenizer(p).input_ids
            ids = [int(t) for t in p]
            W = params.beam_width
            out = llm.generate(input_ids=torch.tensor([ids], dtype=torch.long, device=llm.device), max_new_tokens=params.max_tokens,
                               num_beams=W, num_return_sequences=W, length_penalty=params.length_penalty, eos_token_id=stops or None,
                               ban_mask=mask, pad_token_id=-1)
            self.stats["requests"] += 1
            seqs = []
            for row, sc in zip(out[:, len(ids):].tolist(), llm.last_beam_scores.tolist()):
                toks = [t for t in row if t != -1]
                text = self.tokenizer.decode(toks) if self.tokenizer is not None and hasattr(self.tokenizer, "decode") else None
                seqs.append(BeamSearchSequence(ids + toks, float(sc) * max(1, len(toks)) ** float(params.length_penalty), text))
            outs.append(BeamSearchOutput(seqs))
        return outs

    @torch.no_grad()
    def score(self, prompts=None, prompt_token_ids=None, top_logprobs=0, start=None):
        """Log-probabilities of GIVEN tokens (what vLLM reports as prompt_logprobs): one ScoreOutput per prompt, whose tokens
        start .. L-1 are scored given the tokens in front of them over the raw model's distribution (USDMForCausalLM.score), with the
        top_logprobs (0 .. 20) most likely ids of every scored position.  start: None = 1 (everything but the first token), an integer for
        all prompts or a list with one per prompt - the length of a shared context when candidates behind it are compared.  Nothing is
        generated and no SamplingParams apply.  The prompts run one after another on the single-sequence path (prefill is compute-bound;
        with prefix reuse on, prompts that share a prefix of >= 16 tokens up to start - 1 prefill their own rows only)."""
        if prompts is None and prompt_token_ids is None:
            raise ValueError("prompts or prompt_token_ids is required")
        if isinstance(prompts, str):
            prompts = [prompts]
        if prompt_token_ids is not None and prompt_token_ids and isinstance(prompt_token_ids[0], int):
            prompt_token_ids = [prompt_token_ids]
        n = len(prompts) if prompt_token_ids is None else len(prompt_token_ids)
        k = check_logprobs(top_logprobs) or 0
        starts = list(start) if isinstance(start, (list, tuple)) else [1 if start is None else start] * n
        if len(starts) != n:
            raise ValueError("start is one value for all prompts or a list with one value per prompt")
        outs = []
        for i in range(n):
            text = prompts[i] if prompts is not None else None
            if prompt_token_ids is not None:
                ids = list(prompt_token_ids[i])
            else:
                if self.tokenizer is None:
                    raise ValueError("text prompts need a tokenizer")
                ids = list(self.tokenizer(text).input_ids)
            lp = self.llm.score(torch.tensor([ids], dtype=torch.long, device=self.llm.device), top_logprobs=k, start=starts[i])
            outs.append(assemble_score(ids, starts[i], lp, k, self.tokenizer, text))
        return outs

    # ------------------------------------------------------------------ one request on the single-sequence graph
    def _run_single(self, r):
        sp, llm = r["sp"], self.llm
        if r["max_new"] <= 0:
            return [], "length", None
        ids = torch.tensor([r["ids"]], dtype=torch.long, device=llm.device)
        kw = dict(input_ids=ids, max_new_tokens=r["max_new"], eos_token_id=sorted(r["stops"]) or None, min_new_tokens=sp.min_tokens,
                  logprobs=sp.logprobs, repetition_penalty=sp.repetition_penalty, presence_penalty=sp.presence_penalty,
                  frequency_penalty=sp.frequency_penalty, min_p=sp.min_p, logit_bias=sp.logit_bias, no_repeat_ngram_size=sp.no_repeat_ngram_size)
        sampled = not sp.greedy
        if sampled:
            kw.update(do_sample=True, temperature=sp.temperature, top_p=sp.top_p, top_k=(sp.top_k if sp.top_k > 0 else None), seed=r["seed"])
        if self._spec_eligible(r):        # a plain greedy request served alone: the speculative step (sampled, with the flag: its sampled variant)
            k, lmax, lmin = self.spec
            if sampled or (self.spec_sampling and sp.min_p):      # (a greedy request with min_p: eligible with the flag only, top_k = 1)
                kw.update(speculative_sampling=True)
                self.stats["spec_sampled_requests"] += int(sampled)
            out = llm.generate(ban_mask=r["mask"], num_speculative_tokens=k, prompt_lookup_max=lmax, prompt_lookup_min=lmin, **kw)
            st = llm.last_spec_stats
            self.stats["spec_requests"] += 1
            for name in ("steps", "drafted", "accepted"):
                self.stats["spec_" + name] += st[name]
        elif r["mask"] is not None:
            out = llm.generate(ban_mask=r["mask"], **kw)
        else:       # history-dependent processors: Python between the lm_head launch and the pick of every step
            self.stats["hook_requests"] += 1
            prompt = list(r["ids"])

            def hook():
                step = int(llm.st_step.item())
                hist = prompt + llm.st_out[:step].tolist()
                lg = llm.last_logits
                for p in sp.logits_processors:
                    lg = p(hist, lg)
                if lg is not llm.last_logits:
                    llm.last_logits.copy_(lg)
            if not sampled:
                kw.update(do_sample=False)
            out = llm.generate(_logits_hook=hook, **kw)
        toks = out[0, len(r["ids"]):].tolist()
        why = "stop" if (toks and toks[-1] in r["stops"] and len(toks) >= sp.min_tokens) else "length"
        return toks, why, llm.last_logprobs

    # ------------------------------------------------------------------ speculative decoding: who, and the slots
    def _spec_eligible(self, r):
        """speculative_config is on and the request is plain greedy with a static mask: no logprobs, min_p, penalties or edits.  With
        speculative_sampling in the config a sampled request, with or without min_p, is eligible too."""
        sp = r["sp"]
        return (self.spec is not None and r["mask"] is not None and ((sp.greedy and not sp.min_p) or self.spec_sampling)
                and sp.logprobs is None and sp.penalties is None and sp.edits is None)

    def _spec_slot_count(self):
        """Slots of the batched speculative step: the rows of a step shared out in slots of k + 1, at most max_num_seqs; 0 = off (no
        speculative_config, or a model with enable_prefix_caching, whose index the speculative slots do not keep)"""
        if self.spec is None or self.prefix_caching:
            return 0
        return min(self.max_slots, self.llm.spec_group(self.spec[0]))

    def _spec_split(self, grp):
        """A group of requests with one mask -> (those served through the speculative slots, the rest).  Fewer than two eligible
        requests or fewer than two slots: nobody - a lone eligible request keeps the single path, the others go where they went."""
        fast = [r for r in grp if self._spec_eligible(r)]
        if len(fast) < 2 or self._spec_slot_count() < 2:
            return [], grp
        return fast, [r for r in grp if not self._spec_eligible(r)]

    def _run_spec_batched(self, grp):
        """Eligible requests of one mask through the speculative slots, with turnover as in _run_batched (SpecSlots.serve); per-request
        stop ids and max_tokens go into the slot's stop block and limit."""
        llm, (k, lmax, lmin) = self.llm, self.spec
        ss = llm.spec_slots(self._spec_slot_count())
        llm.load_ban(ban_mask=grp[0]["mask"])
        ss.set_lookup(lmax, lmin, False)
        knobs = lambda r: None if r["sp"].greedy else (r["sp"].temperature, max(r["sp"].top_k, 0), r["sp"].top_p, r["seed"], r["sp"].min_p)
        reqs = [dict(ids=torch.tensor(r["ids"], dtype=torch.long), limit=r["max_new"], stops=r["stops"], min_new=r["sp"].min_tokens,
                     sampling=knobs(r)) for r in grp]
        n_sampled = sum(q["sampling"] is not None for q in reqs)      # one sampled request -> the whole group runs the sampled step
        res, max_active = ss.serve(reqs, k + 1, sampled=n_sampled > 0)
        st = self.stats
        if n_sampled:
            st["spec_sampled_requests"] += n_sampled
        st["batched_requests"] += len(grp)
        st["spec_batched_requests"] += len(grp)
        st["spec_max_active"] = max(st["spec_max_active"], max_active)
        out = []
        for r, (toks, c) in zip(grp, res):
            for name in ("steps", "drafted", "accepted"):
                st["spec_" + name] += c[name]
            why = "stop" if (toks and toks[-1] in r["stops"] and len(toks) >= r["sp"].min_tokens) else "length"
            out.append((r, toks, why, None))
        return out

    # ------------------------------------------------------------------ continuous batching over the decode slots
    def _run_batched(self, grp):
        llm = self.llm
        nslots = min(self.max_slots, llm.max_batch(), SMALL_SLOTS if len(grp) <= SMALL_SLOTS else MAX_SLOTS)
        ds = llm.decode_slots(nslots)
        # one request with log-probabilities -> the whole group runs on the log-probability step (the sampling step + usdm_logprobs),
        # with the group's largest K; every request's rows are trimmed to its own K on the host
        ks = [r["sp"].logprobs for r in grp if r["sp"].logprobs is not None]
        lpk = max(ks) if ks else None
        # one penalised request -> the whole group runs on the penalised step (usdm_penalize + the sampling step); the other
        # requests and the idle slots carry neutral knobs
        pen = any(r["sp"].penalties is not None for r in grp)
        edt = any(r["sp"].edits is not None for r in grp)      # likewise: the step with usdm_logit_edit
        kind = step_kind(any(not r["sp"].greedy for r in grp), lpk, pen, edt)       # one sampled request -> the whole group runs on the sampling graph
        decode = ds.step_plan(kind)
        self.stats["sampled_in_batch"] = self.stats.get("sampled_in_batch", 0) + sum(not r["sp"].greedy for r in grp)
        for b in range(nslots):                               # idle slots: harmless greedy knobs, neutral penalties and edits
            ds.reset_knobs(b)
        llm.load_ban(ban_mask=grp[0]["mask"])
        queue, slots, results = deque(grp), [None] * nslots, []
        self.stats["batched_requests"] += len(grp)
        while queue or any(s is not None for s in slots):
            for b in range(nslots):                               # admit: prefill the prompt into the free slot's cache
                if slots[b] is None and queue:
                    r = queue.popleft()
                    sp = r["sp"]
                    knobs = None if sp.greedy else (sp.temperature, max(sp.top_k, 0), sp.top_p, r["seed"], sp.min_p)
                    src, past = ds.admit(b, torch.tensor(r["ids"], dtype=torch.long), kind, knobs=sp.penalties, edits=sp.edits, sampling=knobs)      # (+ first token)
                    if self.prefix_caching:
                        st = self.stats
                        st["prefix_hits"] += past > 0
                        st["prefix_rows_reused"] += past
                        st["prefill_rows"] += len(r["ids"]) - past
                        st["prefix_copies"] += src is not None and src != b
                        st["prefix_hits_live"] += src is not None and src != b and slots[src] is not None
                        self.admission_log.append((b, tuple(r["ids"])))
                    slots[b] = dict(r=r, produced=1)
                    self.stats["admissions"] += 1
            active = [b for b in range(nslots) if slots[b] is not None]
            self.stats["max_active"] = max(self.stats["max_active"], len(active))
            for b in range(nslots):                               # idle slots decode garbage where it destroys nothing (DecodeSlots.park)
                if slots[b] is None:
                    ds.park(b)
            # tokens already known (the prefill's first token) are checked before any further step is spent
            toks = ds.tokens()                                       # host sync = scheduling point
            need, freed = 0, False
            for b in active:
                s, r = slots[b], slots[b]["r"]
                seq = toks[b][:s["produced"]]
                end = stop_index(seq, r["stops"], r["sp"].min_tokens)
                if end is not None or s["produced"] >= r["max_new"]:
                    n = end if end is not None else r["max_new"]
                    # the slot's rows are read HERE, before a refill restarts its step at 0 and overwrites them; rows decoded past
                    # the stop, up to the end of the chunk, are dropped with their tokens
                    k = r["sp"].logprobs
                    lp = ds.logprobs(b, len(seq[:n]), lpk).trimmed(len(seq[:n]), k) if k is not None else None
                    results.append((r, seq[:n], "stop" if end is not None and end <= n else "length", lp))
                    slots[b] = None
                    ds.reset_knobs(b)      # the idle slot keeps decoding garbage: with neutral knobs
                    freed = True
                else:
                    need = max(need, 1)
            if not need or (freed and queue):
                continue                                             # refill the freed slot(s) before spending more steps
            live = [b for b in range(nslots) if slots[b] is not None]
            # never more steps than the slot with the FEWEST tokens left: batch slots have no device-side `done` word, so a
            # slot would otherwise keep decoding to the end of the chunk - past its max_new, and for a request that runs to the
            # context limit (the reference passes max_tokens = model_max_length) past ctx_max, i.e. into the next head's / the
            # next slot's cache rows.  usdm_attn_decode additionally refuses positions >= ctx_max.
            n = min(CHUNK, min(slots[b]["r"]["max_new"] - slots[b]["produced"] for b in live))
            for _ in range(n):
                decode.run()
            self.stats["batched_steps"] += n
            for b in live:
                slots[b]["produced"] = min(slots[b]["produced"] + n, slots[b]["r"]["max_new"])
        return results

    # ------------------------------------------------------------------ detokenise
    def _finish(self, r, toks, why, lp=None):
        text = ""
        if self.tokenizer is not None:
            text = self.tokenizer.decode(toks, skip_special_tokens=r["sp"].skip_special_tokens)
        stop_reason = toks[-1] if (why == "stop" and toks) else None
        k = r["sp"].logprobs
        if k is None:
            return CompletionOutput(r["i"][1], text, toks, why, stop_reason)
        if lp is None:      # (no room for a single token)
            return CompletionOutput(r["i"][1], text, toks, why, stop_reason, 0.0, [])
        lps, total = assemble_logprobs(toks, lp.token_logprobs, lp.ranks, lp.top_ids, lp.top_logprobs, k, self.tokenizer)
        return CompletionOutput(r["i"][1], text, toks, why, stop_reason, total, lps)
