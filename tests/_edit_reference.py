"""numpy restatement of usdm_logit_edit (logit bias, then HF's n-gram ban) and of min_p's kept set, for the kernel and model tests.
The bias is one float32 add per entry, the ban a direct port of the rule in include/usdm_hip.h, so the edited row is compared with
the kernel's bit for bit; the min_p kept set is computed in float64."""
import numpy as np

from tests._logprob_reference import bf16_row      # noqa: F401  (the rows the tests run on)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def bias_row(x, bias):
    """x[id] = x[id] + value, one float32 add per (distinct) id; ids outside [0, V) are ignored"""
    y = np.array(x, dtype=np.float32, copy=True)
    for i, v in (bias.items() if isinstance(bias, dict) else bias):
        if 0 <= i < y.shape[0]:
            with np.errstate(invalid="ignore"):
                y[i] = np.float32(y[i]) + np.float32(v)
    return y


def banned_ngram_ids(hist, n):
    """The ids HF's no_repeat_ngram_size = n bans after the history `hist`: for every j in 0 .. Lh - n whose hist[j .. j+n-2] equals
    the last n - 1 tokens, hist[j+n-1] (n = 1: the tail is empty, every id of the history)."""
    hist = [int(t) for t in hist]
    Lh = len(hist)
    if n < 1 or Lh < n:
        return set()
    tail = hist[Lh - (n - 1):] if n > 1 else []
    return {hist[j + n - 1] for j in range(Lh - n + 1) if hist[j:j + n - 1] == tail}


def edit_row(x, bias, n, prompt, out, id_offset=0):
    """The row usdm_logit_edit leaves: bias first, then -inf over the banned ids; out holds the ids as out_tokens does (+ id_offset)"""
    y = bias_row(x, bias or {})
    hist = [int(t) for t in prompt] + [int(t) - id_offset for t in out]
    for i in banned_ngram_ids(hist, n):
        if 0 <= i < y.shape[0]:
            y[i] = -np.inf
    return y


def min_p_ratio(x, T):
    """p_i / p_max = exp((x_i - max) / T) in float64 (0 for -inf)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(x), 0.0, np.exp((x - x.max()) / float(T)))


def min_p_keep(x, T, min_p):
    """HF MinPLogitsWarper's / vLLM's kept set: p_i >= min_p * p_max, among the ids that are not banned"""
    return (min_p_ratio(x, T) >= float(min_p)) & ~np.isneginf(np.asarray(x))


def min_p_band_empty(x, T, min_p, rel=1e-4):
    """The condition the exact comparison rests on: no id's p_i / p_max within relative `rel` of min_p (the maximum and its exact
    ties, ratio exactly 1, are not near anything: they are kept for every min_p <= 1)"""
    r = min_p_ratio(x, T)
    r = r[r < 1.0]
    return not bool((np.abs(r - min_p) <= rel * min_p).any())
