"""Numpy float32 restatement of usdm_penalize, the rows and tables its tests run on.

Every operation is one IEEE float32 operation on float32 operands, in the kernel's order, so the result is compared bit for bit:
    seen = in_prompt(i) or c(i) > 0
    x = seen ? (x < 0 ? x * r : x / r) : x
    x = x - (f * float(c(i)))
    x = x - (p * (c(i) > 0 ? 1 : 0))
c(i) = occurrences of id i among the generated ids, in_prompt(i) = id i occurs in the prompt.  The knobs are rounded to float32
first, as the device block holds them."""
import numpy as np

PROMPT_BIT = 1 << 30


def table(V, prompt_ids, out_ids):
    """usdm_penalize's table of one sequence: c(i) in the low bits, in_prompt(i) in bit 30 (int32 [V])"""
    t = np.bincount(np.asarray(out_ids, dtype=np.int64), minlength=V).astype(np.int32)
    t[np.unique(np.asarray(prompt_ids, dtype=np.int64))] |= PROMPT_BIT
    return t


def penalize_table(x, tbl, r, f, p):
    """The penalised copy of the f32 row x under the table tbl"""
    x = np.asarray(x, dtype=np.float32)
    r, f, p = np.float32(r), np.float32(f), np.float32(p)
    if r == 1 and f == 0 and p == 0:
        return x.copy()
    c = (tbl & (PROMPT_BIT - 1)).astype(np.int32)
    seen = tbl != 0
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(seen, np.where(x < 0, x * r, x / r), x).astype(np.float32)
        y = (y - (f * c.astype(np.float32))).astype(np.float32)
        y = (y - (p * (c > 0).astype(np.float32))).astype(np.float32)
    return y


def penalize_row(x, prompt_ids, out_ids, r, f, p):
    return penalize_table(x, table(np.asarray(x).shape[0], prompt_ids, out_ids), r, f, p)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def bf16_row(V, seed, banned=0.25):
    """f32 logits holding bf16-valued numbers (what the lm_head writes), about `banned` of them -inf, a few exact zeros"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(V) * 3).astype(np.float32)
    x = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).copy()
    x[g.random(V) < banned] = -np.inf
    x[g.integers(0, V, 3)] = 0.0
    return x


def history(V, seed, n_prompt=40, n_out=30):
    """A random prompt and a random output history with repeats (ids drawn from a small pool, the first pool id 5 times at least)"""
    g = np.random.default_rng(seed)
    prompt = g.integers(0, V, n_prompt)
    pool = np.concatenate([g.integers(0, V, 8), prompt[:3]])
    out = np.concatenate([g.choice(pool, n_out), np.repeat(pool[0], 5)])
    return prompt, out
