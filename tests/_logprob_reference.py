"""Float64 reference of usdm_logprobs, the rows its tests run on, and the tolerance those tests use.

Tolerance.  The kernel computes lp(i) = f32( f64(x_i - max) - log Z ), Z = sum_i floor(exp_f32(x_i - max) * 2^40) / 2^40 with the
logarithm in f64: its only error sources are the f32 exponential (about 1 ulp per term, averaging out in Z), the truncation to 2^-40
(at most V * 2^-40 < 4e-8 relative) and the final rounding to f32 (half an ulp of the result: 9.5e-7 for 16 <= |lp| < 32, 1.9e-6
up to 64).  emulate_f32() below is that arithmetic in numpy; kernel_tolerance() runs it against float64 on exactly the rows of the
kernel test (every vocabulary size x ban pattern, every finite id) and returns FOUR TIMES the largest error seen.  Measured on the
CPU: largest error 8.50e-07 (the final rounding of an lp of -18.08 in the V = 42003 row with the banned range; ulp / 2 there is
9.5e-07), so the tolerance is 3.40e-06; the tests assert that it stays <= 1e-4 (a wrong logsumexp is off by far more)."""
import functools

import numpy as np
import torch

CASES = [(42003, (0, 1, 5, 20)), (1000, (1, 5, 20)), (20, (5, 20)), (7, (20,))]     # V, the K values used with it
BANS = ("none", "range", "all_but_one")


def bf16_row(V, seed):
    """f32 logits holding bf16-valued numbers (what the lm_head writes: exact ties are common)."""
    x = (np.random.default_rng(seed).standard_normal(V) * 3).astype(np.float32)
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def banned(x, pattern):
    """none / about 30 % as one contiguous id range (as the reference's masks are) / every id but one"""
    x, V = x.copy(), x.shape[0]
    if pattern == "range":
        x[V // 5:V // 5 + max(1, (3 * V) // 10)] = -np.inf
    elif pattern == "all_but_one":
        keep = (2 * V) // 3
        v = x[keep]
        x[:] = -np.inf
        x[keep] = v
    return x


def case_row(V, pattern):
    return banned(bf16_row(V, 7 * V + 1), pattern)


def reference(x):
    """(lp float64 [V], ids in descending log-probability with exact ties by lowest id, rank of every id as vLLM counts it).
    A row without a finite logit is -inf everywhere (log_softmax itself would give NaN)."""
    x = np.asarray(x, dtype=np.float32)
    if np.isneginf(x).all():
        lp = np.full(x.shape, -np.inf)
    else:
        lp = torch.log_softmax(torch.from_numpy(x).double(), 0).numpy()
    order = np.lexsort((np.arange(x.shape[0]), -x.astype(np.float64)))       # stable: by -value, then id
    srt = np.sort(x)
    rank = 1 + (x.shape[0] - np.searchsorted(srt, x, side="right"))          # 1 + number of strictly greater logits
    return lp, order, rank


def emulate_f32(x):
    """The kernel's own arithmetic (see the module docstring) in numpy."""
    x = np.asarray(x, dtype=np.float32)
    m = x.max()
    with np.errstate(invalid="ignore"):
        d = np.where(x == m, np.float32(0), x - m).astype(np.float32)
        e = np.where(np.isneginf(x), np.float32(0), np.exp(d, dtype=np.float32))
    z = int(np.floor(e.astype(np.float64) * 2.0 ** 40).astype(np.int64).sum())
    if z == 0:
        return np.full(x.shape, -np.inf, dtype=np.float32)
    log_z = np.log(float(z)) - 40.0 * np.log(2.0)
    return np.where(np.isneginf(x), -np.inf, d.astype(np.float64) - log_z).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kernel_error():
    worst = 0.0
    for V, _ in CASES:
        for pattern in BANS:
            x = case_row(V, pattern)
            ref, emu = reference(x)[0], emulate_f32(x).astype(np.float64)
            fin = np.isfinite(ref)
            assert (np.isneginf(emu) == ~fin).all()
            worst = max(worst, float(np.abs(emu[fin] - ref[fin]).max()))
    return worst


def kernel_tolerance():
    tol = 4.0 * kernel_error()
    assert 0 < tol <= 1e-4, tol
    return tol


def check_row(x, tok, got_lp, got_rank, got_ids, got_lps, K, tol):
    """One written row against the float64 reference on logits row x: ids and rank exactly, values within tol."""
    lp, order, rank = reference(x)
    V = x.shape[0]
    assert int(got_rank) == int(rank[tok]), (int(got_rank), int(rank[tok]))
    if np.isfinite(lp[tok]):
        assert abs(float(got_lp) - lp[tok]) <= tol, (float(got_lp), lp[tok])
    else:
        assert float(got_lp) == lp[tok]
    n = min(K, V)
    assert list(map(int, got_ids[:n])) == order[:n].tolist()
    assert all(int(i) == -1 for i in got_ids[n:K]) and all(np.isneginf(float(v)) for v in got_lps[n:K])
    want = lp[order[:n]]
    got = np.asarray([float(v) for v in got_lps[:n]])
    fin = np.isfinite(want)
    assert (got[~fin] == want[~fin]).all()
    assert (np.abs(got[fin] - want[fin]) <= tol).all(), float(np.abs(got[fin] - want[fin]).max())
