"""Drop-in for the reference CLI module src/inference.py: same helper names, same `sample(...)`
signature and control flow (ASR round -> text round -> unit round -> reconstruct_speech -> wav).

Differences forced by the environment: models are passed in / loaded from local paths (no hub), and
librosa is absent, so audio loading uses scipy (polyphase resampling to 16 kHz; host I/O outside the hot path).
"""
import argparse
import re
import sys

import numpy as np
import torch
from scipy.io.wavfile import read as wav_read
from scipy.io.wavfile import write
from scipy.signal import resample_poly

from .voicebox.util.model_util import initialize_decoder, reconstruct_speech  # noqa: F401

device = torch.device("cuda")


def default_template(user_unit, user_text=None, agent_text=None):
    """Unified template for the ASR, T2T and TTS stages (src/inference.py:16-27)."""
    template = (
        "Below is a conversation between the user and the agent. Each turn includes the user's speech and its corresponding transcript, "
        "along with the agent's response text and the corresponding speech.\n"
        "\n### User\n"
        f"{user_unit}<|correspond|>"
    )
    if user_text:
        template += f"{user_text}\n### Agent\n"
    if agent_text:
        template += f"{agent_text}<|correspond|>"
    return template


def strip_exact_multiple(text, patterns):
    """src/inference.py:31-37."""
    for pattern in patterns:
        if text.startswith(pattern):
            text = text[len(pattern):]
        if text.endswith(pattern):
            text = text[:-len(pattern)]
    return text


def generate_bad_words_ids(start, end, exclude=[]):
    """src/inference.py:41-45 (note: `pop` removes by INDEX; correct only because start == 0 whenever exclude is used)."""
    bad_words_ids = [[token_id] for token_id in range(start, end)]
    for e in exclude:
        bad_words_ids.pop(e)
    return bad_words_ids


def load_audio_16k(path):
    sr, data = wav_read(path)
    x = data.astype(np.float32)
    if data.dtype == np.int16:
        x /= 32768.0
    elif data.dtype == np.int32:
        x /= 2147483648.0
    if x.ndim == 2:
        x = x.mean(axis=1)
    if sr != 16000:
        g = np.gcd(16000, sr)
        x = resample_poly(x, 16000 // g, sr // g).astype(np.float32)
    return x


_BAD = {}


def _bad(name, *a, **k):
    if name not in _BAD:
        _BAD[name] = generate_bad_words_ids(*a, **k)
    return _BAD[name]


@torch.inference_mode()
def sample(user_path, reference_path, model, unit_extractor, voicebox, vocoder, tokenizer, output_path,
           reference_mel=None, n_timesteps=50, logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
           min_p=0.0, logit_bias=None, no_repeat_ngram_size=0, num_beams=None, num_speculative_tokens=None, prompt_lookup_max=3,
           prompt_lookup_min=1, speculative_sampling=False):
    """src/inference.py:48-89.  logprobs=K (0 .. 20): the LLM also computes per-token log-probabilities (USDMForCausalLM.generate) and the
    cumulative log-probability of each of the three rounds goes to stderr; nothing else changes.
    repetition_penalty / presence_penalty / frequency_penalty: passed to all three rounds (USDMForCausalLM.generate; on the device).
    min_p / logit_bias / no_repeat_ngram_size: likewise (the rounds pick with top_k = 1, where min_p changes nothing).
    num_beams=N > 1: the three rounds run beam search on the device instead (USDMForCausalLM.generate(num_beams=N): the best
    hypothesis, HF's defaults length_penalty = 1 and early_stopping = False); its score goes to stderr.  Not with the knobs above.
    num_speculative_tokens=k (1 .. 7): the three rounds run speculative greedy decoding with n-gram drafts
    (USDMForCausalLM.generate(num_speculative_tokens=k, prompt_lookup_max, prompt_lookup_min)); steps, drafts and accepted drafts of
    each round go to stderr.  Not with the knobs above or num_beams.
    speculative_sampling=True (with num_speculative_tokens): the rounds run the SAMPLED speculative step
    (USDMForCausalLM.generate(speculative_sampling=True)), on which their top_k = 1 picks give the same ids and min_p is allowed."""
    bad_words_ids_unit2text = _bad("u2t", 32000, 42003)
    bad_words_ids_text2text = _bad("t2t", 32002, 42003)
    bad_words_ids_text2unit = _bad("t2u", 0, 32002, exclude=[28705])
    pattern = re.compile(r"<\|unit(\d+)\|>")

    user_wav = load_audio_16k(user_path) if isinstance(user_path, str) else user_path
    user_unit = ''.join([f'<|unit{i}|>' for i in unit_extractor.predict(torch.as_tensor(user_wav, dtype=torch.float32).to(device), 35 - 1).cpu().tolist()])

    def run(model_input, bad, eos, name):
        ids = torch.LongTensor(tokenizer(model_input).input_ids).to(device).unsqueeze(0)
        if num_beams is not None and num_beams > 1:
            out = model.generate(input_ids=ids, max_length=tokenizer.model_max_length, bad_words_ids=bad, eos_token_id=eos, num_beams=num_beams)
            print(f"{name}: beam search over {num_beams} beams, score {float(model.last_beam_scores[0]):.4f}", file=sys.stderr)
            return out
        out = model.generate(input_ids=ids, max_length=tokenizer.model_max_length, do_sample=True, bad_words_ids=bad,
                             top_p=1.0, top_k=1, temperature=1.0, eos_token_id=eos, logprobs=logprobs,
                             repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                             min_p=min_p, logit_bias=logit_bias, no_repeat_ngram_size=no_repeat_ngram_size,
                             num_speculative_tokens=num_speculative_tokens, prompt_lookup_max=prompt_lookup_max,
                             prompt_lookup_min=prompt_lookup_min, **(dict(speculative_sampling=True) if speculative_sampling else {}))
        if model.last_spec_stats is not None:
            st = model.last_spec_stats
            print(f"{name}: {st['steps']} speculative steps, {st['drafted']} drafts, {st['accepted']} accepted", file=sys.stderr)
        lp = model.last_logprobs
        if lp is not None:
            print(f"{name}: {lp.token_logprobs.numel()} tokens, cumulative log-probability {lp.cumulative:.4f}", file=sys.stderr)
        return out

    outputs = run(default_template(user_unit=user_unit), bad_words_ids_unit2text, tokenizer("\n").input_ids[-1], "unit-to-text")
    user_text = strip_exact_multiple(tokenizer.decode(outputs[0]).split("<|correspond|>")[-1], ["\n", " "])
    outputs = run(default_template(user_unit=user_unit, user_text=user_text), bad_words_ids_text2text,
                  tokenizer("<|correspond|>").input_ids[-1], "text-to-text")
    agent_text = strip_exact_multiple(tokenizer.decode(outputs[0]).split("\n")[-1], ["\n", " ", "<|correspond|>"])
    outputs = run(default_template(user_unit=user_unit, user_text=user_text, agent_text=agent_text), bad_words_ids_text2unit, 28705, "text-to-unit")
    agent_unit = tokenizer.decode(outputs[0]).split("<|correspond|>")[-1]

    matches = [int(x) for x in pattern.findall(agent_unit)]
    agent_unit = torch.LongTensor(matches).to(device)
    reference_unit = None
    if reference_mel is not None:
        if reference_path is None:
            raise ValueError("reference_mel needs reference_path too (the prompt's unit ids are extracted from that audio)")
        ref_wav = load_audio_16k(reference_path)
        reference_unit = unit_extractor.predict(torch.as_tensor(ref_wav, dtype=torch.float32).to(device), 35 - 1)
        reference_path = None
    audio = reconstruct_speech(agent_unit, device, reference_path, unit_extractor, voicebox, vocoder, n_timesteps=n_timesteps,
                               reference_mel=reference_mel, reference_unit=reference_unit)
    write(output_path, vocoder.h.sampling_rate, audio)
    return audio


def parse_logit_bias(text):
    """--logit_bias: a JSON object {"token id": bias} -> {int id: bias} (None: no bias); anything else is a ValueError."""
    if text is None:
        return None
    import json
    try:
        obj = json.loads(text)
    except ValueError as e:
        raise ValueError(f"logit_bias is not JSON: {e}") from None
    if not isinstance(obj, dict):
        raise ValueError("logit_bias must be a JSON object {\"token id\": bias}")
    try:
        return {int(k): v for k, v in obj.items()}
    except ValueError:
        raise ValueError("logit_bias: every key must be an integer token id") from None


def check_num_beams(args):
    """--num_beams: None or 1 (off), or 2 .. 16 with every other generation flag at its default.  ValueError otherwise."""
    n = args.num_beams
    if n is None or n == 1:
        return
    from .ops import beam_candidates
    beam_candidates(n, 1)      # (every round has one EOS id)
    flags = dict(logprobs=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, no_repeat_ngram_size=0,
                 logit_bias=None)
    used = [f"--{k}" for k, v in flags.items() if getattr(args, k) != v]
    if used:
        raise ValueError(f"--num_beams cannot be combined with {', '.join(used)}: beam search ranks the model's own log-probabilities")


def load_models(model_cache_dir, dev=None, ctx_max=None, quantization=None, kv_cache_dtype=None, enable_prefix_caching=False):
    """What the reference's __main__ does between argument parsing and sample() (src/inference.py:105-129), from LOCAL copies:
    hub names resolve inside model_cache_dir (huggingface_hub cache layout or plain <name>/ directories, checkpoints.py)."""
    import os
    from .checkpoints import resolve_local
    from .llm import USDMForCausalLM
    from .unit_extractor import UnitExtractor
    dev = torch.device(dev or device)
    # Load voicebox, vocoder configuration and checkpoint
    voicebox, vocoder = initialize_decoder(model_cache_dir, dev)
    # Load unit extractor (speech tokenizer): the reference's own call, resolved inside the cache directory
    os.environ.setdefault("USDM_MODEL_CACHE_DIR", model_cache_dir)
    unit_extractor = UnitExtractor("xlsr2_1b_v2", "https://dl.fbaipublicfiles.com/seamlessM4T/models/unit_extraction/kmeans_10k.npy",
                                   device=dev, cache_dir=model_cache_dir)
    # Load USDM model and tokenizer
    llm_dir = resolve_local(model_cache_dir, "naver-ai/USDM-DailyTalk", must_contain=("config.json",))
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(llm_dir, local_files_only=True)
    # the reference generates up to tokenizer.model_max_length (inference.py:64); beyond the 4096-token sliding window the attention
    # kernels bound their key range (llm.py), so the cache may be longer than the window.  8192 = the USDM tokenizer's limit.
    want = ctx_max or min(int(getattr(tokenizer, "model_max_length", 4096) or 4096), 8192)
    model = USDMForCausalLM.from_pretrained(llm_dir, device=dev, torch_dtype=torch.bfloat16, ctx_max=want,
                                            quantization=quantization, kv_cache_dtype=kv_cache_dtype,
                                            enable_prefix_caching=enable_prefix_caching).to(dev).eval()
    return model, unit_extractor, voicebox, vocoder, tokenizer


def main(argv=None):
    global device
    parser = argparse.ArgumentParser()
    parser.add_argument('--input_path', type=str, required=True,
                        help="Path to the input file containing the speech data to process.")
    parser.add_argument('--reference_path', type=str, default=None,
                        help="Path to the reference audio file for speaker adaptation (optional). If not provided, the model will perform speaker unconditional generation.")
    parser.add_argument('--model_cache_dir', type=str, required=True,
                        help="Directory holding the model checkpoints (the reference's download cache, or local <name>/ directories).")
    parser.add_argument('--output_path', type=str, required=True,
                        help="Path to save the spoken response.")
    parser.add_argument('--quantization', type=str, default=None, choices=["fp8", "mxfp4"],
                        help="Weight-only quantization of the LLM (opt-in, default bf16): fp8 (e4m3, power-of-two row scales) or mxfp4 "
                             "(e2m1 with a power-of-two scale per 32 elements, fp8 lm_head; about 11.5 %% weight error).")
    parser.add_argument('--kv_cache_dtype', type=str, default=None, choices=["bf16", "fp8"],
                        help="KV cache of the LLM: bf16 (default) or fp8 (e4m3 rows, one power-of-two scale per token and kv head; opt-in, "
                             "switches prefix reuse between the three rounds off unless --enable_prefix_caching is given).")
    parser.add_argument('--enable_prefix_caching', action='store_true',
                        help="Prefix caching (vLLM's name; opt-in): batch slots reuse cached prompt rows, and with --kv_cache_dtype fp8 the three "
                             "rounds reuse their prefix again (its rows are then read as the cache holds them: quantized).")
    parser.add_argument('--logprobs', type=int, default=None, choices=range(21), metavar="K",
                        help="Also compute per-token log-probabilities on the device (K = 0 .. 20 most likely ids per token) and print the "
                             "cumulative log-probability of each of the three LLM rounds to stderr.")
    parser.add_argument('--repetition_penalty', type=float, default=1.0,
                        help="Repetition penalty of the three LLM rounds, in (0, 2]; 1 = off (HF generate / vLLM: ids of the prompt and the output).")
    parser.add_argument('--presence_penalty', type=float, default=0.0,
                        help="Presence penalty of the three LLM rounds, in [-2, 2]; 0 = off (vLLM: ids generated so far).")
    parser.add_argument('--frequency_penalty', type=float, default=0.0,
                        help="Frequency penalty of the three LLM rounds, in [-2, 2]; 0 = off (vLLM: per occurrence among the ids generated so far).")
    parser.add_argument('--min_p', type=float, default=0.0,
                        help="min-p of the three LLM rounds, in [0, 1]; 0 = off (HF / vLLM: drops ids with p < min_p * p_max; the rounds "
                             "pick with top_k = 1, where it changes nothing).")
    parser.add_argument('--no_repeat_ngram_size', type=int, default=0,
                        help="HF no_repeat_ngram_size of the three LLM rounds: no n-gram of this size occurs twice in prompt + output; 0 = off.")
    parser.add_argument('--logit_bias', type=str, default=None, metavar="JSON",
                        help='Additive logit bias of the three LLM rounds as a JSON object {"token id": bias}, at most 1024 entries, '
                             'values clamped to [-100, 100] (OpenAI / vLLM).')
    parser.add_argument('--num_beams', type=int, default=None, metavar="N",
                        help="Beam search over N beams (2 .. 16) in the three LLM rounds instead of the greedy pick, on the device (HF "
                             "generate(num_beams=N): length_penalty 1, early_stopping False, the best hypothesis).  An error together with "
                             "--logprobs, the penalties, --min_p, --no_repeat_ngram_size or --logit_bias.")
    parser.add_argument('--num_speculative_tokens', type=int, default=None, metavar="K",
                        help="Speculative greedy decoding in the three LLM rounds: every step verifies K (1 .. 7) n-gram drafts taken from "
                             "the round's own prompt and output (vLLM speculative_config method 'ngram').  The ids do not depend on the drafts.  "
                             "An error together with --logprobs, the penalties, --min_p, --no_repeat_ngram_size, --logit_bias, --num_beams "
                             "or --kv_cache_dtype fp8.")
    parser.add_argument('--prompt_lookup_max', type=int, default=3, help="Longest n-gram the draft lookup matches (1 .. 16).")
    parser.add_argument('--prompt_lookup_min', type=int, default=1, help="Shortest n-gram the draft lookup matches.")
    parser.add_argument('--speculative_sampling', action='store_true',
                        help="With --num_speculative_tokens: verify the drafts on the sampled speculative step, whose picks are drawn with "
                             "each position's own Philox counter (the ids of a fixed seed do not depend on the drafts).  Lifts the error "
                             "with --min_p; the others stay.")
    args = parser.parse_args(argv)
    from .llm import check_edits, check_min_p, check_penalties
    from .spec import check_spec_args, check_spec_call, check_speculative_sampling
    try:
        spec = check_spec_args(args.num_speculative_tokens, args.prompt_lookup_max, args.prompt_lookup_min)
        check_speculative_sampling(args.speculative_sampling, spec is not None)
        if spec is not None:
            try:
                check_spec_call(False, args.logprobs, check_penalties(args.repetition_penalty, args.presence_penalty, args.frequency_penalty),
                                check_edits(parse_logit_bias(args.logit_bias), args.no_repeat_ngram_size), args.min_p, None, args.num_beams,
                                False, args.kv_cache_dtype == "fp8", speculative_sampling=args.speculative_sampling)
            except NotImplementedError as e:
                raise ValueError(str(e)) from None
        check_num_beams(args)
        check_penalties(args.repetition_penalty, args.presence_penalty, args.frequency_penalty)
        check_min_p(args.min_p)
        logit_bias = parse_logit_bias(args.logit_bias)
        check_edits(logit_bias, args.no_repeat_ngram_size)
    except ValueError as e:
        parser.error(str(e))

    device = torch.device("cuda")
    model, unit_extractor, voicebox, vocoder, tokenizer = load_models(args.model_cache_dir, device, quantization=args.quantization,
                                                                         kv_cache_dtype=args.kv_cache_dtype,
                                                                         enable_prefix_caching=args.enable_prefix_caching)
    try:
        sample(args.input_path, args.reference_path, model, unit_extractor, voicebox, vocoder, tokenizer, args.output_path, logprobs=args.logprobs,
               repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty, frequency_penalty=args.frequency_penalty,
               min_p=args.min_p, logit_bias=logit_bias, no_repeat_ngram_size=args.no_repeat_ngram_size, num_beams=args.num_beams,
               num_speculative_tokens=args.num_speculative_tokens, prompt_lookup_max=args.prompt_lookup_max,
               prompt_lookup_min=args.prompt_lookup_min, speculative_sampling=args.speculative_sampling)
    except Exception as e:       # the reference swallows sampling errors the same way (src/inference.py:131-134)
        print(f"Error while sampling: {e}")
        return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
