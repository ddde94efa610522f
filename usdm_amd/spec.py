"""Speculative greedy decoding with n-gram (prompt-lookup) drafts: argument checks shared by generate(), usdm_amd.serving and the CLI
(DESIGN.md 8k).  The kernels are usdm_attn_verify and usdm_spec_commit; the host state is slots.SpecState (the single sequence:
slots.SpecSequence), the step USDMForCausalLM._build_spec_step.  Batches: usdm_attn_verify_batch and
usdm_spec_commit_batch, slots.SpecSlots, the same state and step.  Sampled requests (opt-in, speculative_sampling):
usdm_spec_sample draws the rows' picks and usdm_spec_commit_picks / usdm_spec_commit_batch_picks commit from them."""
from . import ops

MAX_SPECULATIVE_TOKENS = ops.SPEC_MAX_T - 1      # k drafts + the token to continue from = T <= 8 rows
MAX_LOOKUP = 16                                  # usdm_spec_commit compares at most 16 tokens per candidate


def check_spec_args(num_speculative_tokens, prompt_lookup_max=3, prompt_lookup_min=1):
    """-> None (off: None or 0) or (k, lookup_max, lookup_min)"""
    k = num_speculative_tokens
    if k is None or (isinstance(k, int) and not isinstance(k, bool) and k == 0):
        return None
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_SPECULATIVE_TOKENS:
        raise ValueError(f"num_speculative_tokens must be None / 0 or an integer 1 .. {MAX_SPECULATIVE_TOKENS}, got {k!r}")
    for name, v in (("prompt_lookup_max", prompt_lookup_max), ("prompt_lookup_min", prompt_lookup_min)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_LOOKUP:
            raise ValueError(f"{name} must be an integer 1 .. {MAX_LOOKUP}, got {v!r}")
    if prompt_lookup_min > prompt_lookup_max:
        raise ValueError(f"prompt_lookup_min = {prompt_lookup_min} exceeds prompt_lookup_max = {prompt_lookup_max}")
    return k, prompt_lookup_max, prompt_lookup_min


def check_speculative_sampling(speculative_sampling, spec=True):
    """The opt-in flag of sampled speculation -> bool.  A bool only; spec: whether the call speculates at all
    (check_spec_args' value is not None) - the flag without num_speculative_tokens asks for nothing and is refused."""
    if not isinstance(speculative_sampling, bool):
        raise ValueError(f"speculative_sampling must be True or False, got {speculative_sampling!r}")
    if speculative_sampling and not spec:
        raise ValueError("speculative_sampling=True needs num_speculative_tokens >= 1")
    return speculative_sampling


def check_spec_call(sampled=False, logprobs=None, penalties=None, edits=None, min_p=0.0, logits_hook=None, num_beams=None,
                    tensor_parallel=False, kv_cache_fp8=False, speculative_sampling=False):
    """What generate(num_speculative_tokens > 0) cannot be combined with: NotImplementedError, each with its reason.  penalties / edits
    are llm.check_penalties' / llm.check_edits' values (None = neutral); sampled: do_sample with top_k != 1.  speculative_sampling
    (DESIGN.md 8k-3): the rows' picks are drawn by usdm_spec_sample, so `sampled` and `min_p` are no reasons; the others stay."""
    if speculative_sampling:
        sampled, min_p = False, 0.0
    reasons = (
        (sampled, "sampling (do_sample with top_k != 1): only greedy verification is exact by construction; sampled speculation needs "
                  "rejection sampling, which is not built"),
        (logprobs is not None, "logprobs: the speculative step picks from arg-max partials and never materialises a logits row"),
        (penalties is not None, "repetition / presence / frequency penalties: a row's penalty table would depend on drafts not yet accepted"),
        (edits is not None, "logit_bias / no_repeat_ngram_size: they run on the logits row of the sampling step, which the speculative step does not have"),
        (bool(min_p), "min_p: a sampling filter; the speculative step is greedy"),
        (logits_hook is not None, "_logits_hook: Python logits processors cannot run inside the captured speculative step"),
        (num_beams not in (None, 1), "num_beams > 1: the beams already fill the rows of the batched step"),
        (tensor_parallel, "tensor parallelism: usdm_attn_verify and usdm_spec_commit run on one GPU"),
        (kv_cache_fp8, 'kv_cache_dtype="fp8": a plain step reads the rows of earlier steps quantized, a verify step would read its own earlier '
                       "rows unquantized, so the two models differ and the result would depend on the drafts"),
    )
    for hit, why in reasons:
        if hit:
            raise NotImplementedError("num_speculative_tokens > 0 with " + why)


def config_speculative_sampling(cfg):
    """speculative_config's "speculative_sampling" (default False; a bool) - carried beside check_speculative_config's tuple"""
    if not isinstance(cfg, dict):
        return False
    return check_speculative_sampling(cfg.get("speculative_sampling", False), cfg.get("num_speculative_tokens") not in (None, 0))


def check_speculative_config(cfg):
    """serving.LLM(speculative_config=...) in vLLM's shape -> None or check_spec_args' tuple; other methods are refused by name.
    ("speculative_sampling" is read by config_speculative_sampling.)"""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("speculative_config must be a dict such as {'method': 'ngram', 'num_speculative_tokens': 3}")
    method = cfg.get("method", "ngram")
    if method != "ngram":
        raise NotImplementedError(f"speculative_config method {method!r}: only 'ngram' (prompt lookup) is built; there is no draft model")
    unknown = set(cfg) - {"method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min", "speculative_sampling"}
    if unknown:
        raise ValueError(f"speculative_config: unknown keys {sorted(unknown)}")
    if "num_speculative_tokens" not in cfg:
        raise ValueError("speculative_config needs num_speculative_tokens")
    return check_spec_args(cfg["num_speculative_tokens"], cfg.get("prompt_lookup_max", 3), cfg.get("prompt_lookup_min", 1))
