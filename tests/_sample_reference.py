"""The sampling head (usdm_sample_final / usdm_sample_final_seg, csrc/sample_k.hip) in numpy and Python integers (TEST INFRASTRUCTURE
ONLY), written from the kernel's contract: temperature -> top-k -> softmax numerators in f32 -> 2^32 fixed-point masses -> top-p
by whole tie blocks -> min-p -> one Philox draw located by an integer walk in index order.  Plus the hand-built rows that
tests/test_sample_reference_cpu.py proves on the CPU and tests/test_sample_exact_gpu.py runs through the kernel.

Every sum is a sum of integers below 2^53 (V <= 2^20 masses of at most 2^32), held in uint64 arrays or Python ints: no tolerance
anywhere in this file.  The only float arithmetic is what the kernel does in the same IEEE operations: the f32 scaling and
subtraction, the f32 exp (numpy's; the kernel's fast exp differs by a few ulp, which is why the GPU rows are built from ties and
margins), and the two double products (1 - top_p) * Ztot and u * Zk."""
import functools
import math

import numpy as np

from oracle.sampling_oracle import philox_uniform

NT = 1024                      # threads of the kernel's one workgroup: thread t owns ids [t * per, (t + 1) * per), per = ceil(V / NT)
NINF = float("-inf")
Q1 = 1 << 32                   # the fixed-point mass of e = 1
MARGIN = 1e-3                  # relative mass margin of every threshold decision of a level row that is not a tie
SLACK = 1e-4                   # least slack of a (seed, step) pair used on a level row
F32_ONE_BELOW = float(np.nextafter(np.float32(1), np.float32(0)))


def sanitize(temperature, top_k, top_p, min_p=0.0):
    """what the kernel makes of a device parameter block: temperature <= 0 or NaN -> 1, top_p <= 0, > 1 or NaN -> 1, top_k < 0 -> 0,
    min_p outside [0, 1] or NaN -> 0"""
    t, p, m = float(np.float32(temperature)), float(np.float32(top_p)), float(np.float32(min_p))
    return (t if t > 0 else 1.0, max(int(top_k), 0), p if 0 < p <= 1 else 1.0, m if 0 <= m <= 1 else 0.0)


class Filtered:
    """one row after the filters: x (scaled logits), e (f32 numerators), q (uint64 masses of ALL top-k survivors), kept (bool: what the
    kernel keeps; an id with e > 0 but q = 0 is kept and has probability 0), mass (q where kept, else 0), Ztot, R, Zk, cum (inclusive
    cumulative kept mass in index order), kth (value of the k-th largest scaled logit, None with top-k off), blocks (ascending
    [(e, block mass, cumulative mass up to and with the block)] of the top-p stage), top_k"""


def filter_ref(row, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    row = np.asarray(row, np.float32)
    V, F = row.shape[0], Filtered()
    F.V, F.row, F.top_k = V, row, int(top_k)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (row * (np.float32(1.0) / np.float32(temperature))).astype(np.float32)
        keep_k, F.kth = np.ones(V, bool), None
        if 0 < top_k < V:
            F.kth = np.partition(x, V - top_k)[V - top_k]
            keep_k = ~(x < F.kth)                               # HF: `scores < kth` is removed; values compare, so -0.0 == +0.0
        live = keep_k & np.isfinite(x)
        m = x[live].max() if live.any() else np.float32(NINF)
        e = np.where(live, np.exp((x - m).astype(np.float32)), np.float32(0)).astype(np.float32)
    q = (e.astype(np.float64) * 4294967296.0).astype(np.uint64)   # floor(e * 2^32), exact: e has 24 bits
    F.x, F.e, F.q = x, e, q
    F.Ztot = int(q.sum(dtype=np.uint64))
    kept = e > 0
    F.R, F.blocks = None, []
    if np.float32(top_p) < 1:
        F.R = int((1.0 - float(np.float32(top_p))) * float(F.Ztot))
        order = np.argsort(e, kind="stable")
        order = order[e[order] > 0]
        if order.size:
            es = e[order]
            first = np.flatnonzero(np.r_[True, es[1:] != es[:-1]])
            bm = np.add.reduceat(q[order], first)
            cum, thr = 0, None
            for v, b in zip(es[first].tolist(), bm.tolist()):
                cum += int(b)
                F.blocks.append((v, int(b), cum))
                if thr is None and cum > F.R:                   # the first block that does not fit under R is kept whole, with all above
                    thr = v
            kept &= e >= np.float32(thr if thr is not None else np.inf)
    if min_p > 0:
        kept &= e >= np.float32(min_p)
    F.kept, F.mass = kept, np.where(kept, q, np.uint64(0)).astype(np.uint64)
    F.cum = np.cumsum(F.mass, dtype=np.uint64)
    F.Zk = int(F.cum[-1])
    return F


def probs(F):
    """float64 probabilities (mass / Zk; all zero when nothing has mass)"""
    return F.mass.astype(np.float64) / float(F.Zk) if F.Zk else np.zeros(F.V)


def fallback(row):
    """the token when no id has mass: the lowest-index arg-max of the finite logits (+inf counts, NaN and -inf do not), else 0"""
    row = np.asarray(row, np.float32)
    ok = ~np.isnan(row) & (row > NINF)
    return int(np.flatnonzero(ok & (row == row[ok].max()))[0]) if ok.any() else 0


def _locate(F, t):
    """t = u * Zk as the double product -> (id, slack).  Slack: the distance of t from the nearest end of the drawn id's interval
    that another kept id shares, over Zk; 0 and Zk are no such ends (u * Zk never leaves [0, Zk) whatever the masses are)."""
    target = min(int(t), F.Zk - 1)
    i = int(np.searchsorted(F.cum, np.uint64(target), side="right"))
    hi, lo = int(F.cum[i]), int(F.cum[i]) - int(F.mass[i])
    d = min(t - lo if lo > 0 else math.inf, hi - t if hi < F.Zk else math.inf)
    return i, d / F.Zk


def draw_ref(F, seed, step):
    """-> (token, slack) of the draw at Philox (seed, counter = step); top_k == 1 takes u = 0 (the lowest id among exact ties)"""
    if F.Zk == 0:
        return fallback(F.row), math.inf
    u = 0.0 if F.top_k == 1 else philox_uniform(seed, step & 0xFFFFFFFF)
    return _locate(F, u * float(F.Zk))


def sample_ref(row, step, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=0):
    """-> (kept mask, integer masses, token, slack)"""
    F = filter_ref(row, temperature, top_k, top_p, min_p)
    tok, slack = draw_ref(F, seed, step)
    return F.kept, F.mass, tok, slack


def margin(F, min_p=0.0):
    """the least relative distance of a threshold from a decision it did not take: |cumulative block mass - R| / Ztot over the top-p
    blocks, |e - min_p| / min_p over the values of e"""
    out = math.inf
    if F.R is not None and F.Ztot:
        out = min([out] + [abs(c - F.R) / F.Ztot for _, _, c in F.blocks[:-1]])      # (the maximum's block stays whatever R is)
    if min_p > 0:
        out = min([out] + [abs(v - min_p) / min_p for v in np.unique(F.e[F.e > 0]).tolist()])
    return out


# ----------------------------------------------------------------------------------------------- choosing (seed, step) pairs on the CPU
M32 = np.uint64(0xFFFFFFFF)
POOL_SEEDS = (2 ** 40 + 7, 12345, 2 ** 33 + 1, 99, 2 ** 63 + 5, 7, 2 ** 32 + 3, 31337)
POOL_STEPS = 1 << 21
FIXED_PAIRS = tuple((s, t) for t in (0, 2 ** 31 - 1) for s in (0, 2 ** 32 + 3, 2 ** 40 + 7, 12345))


def philox_uniform_np(seed, ctrs):
    """oracle.sampling_oracle.philox_uniform for an array of counters (only used to SEARCH for pairs; every pair found is then
    drawn with the oracle's function)"""
    c0, c1, c2, c3 = np.asarray(ctrs, np.uint64) & M32, np.uint64(0), np.uint64(0), np.uint64(0)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (((c0 >> np.uint64(5)) << np.uint64(26)) | (c1 >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


@functools.lru_cache(maxsize=None)
def _pool(j):
    """candidate pool j: (seed, uniforms of steps 0 .. POOL_STEPS - 1)"""
    return POOL_SEEDS[j], philox_uniform_np(POOL_SEEDS[j], np.arange(POOL_STEPS, dtype=np.uint64))


def pairs_for(F, want_ids, n_min=0, slack=0.0):
    """(seed, step) pairs whose draws cover every id of want_ids, every pair with slack >= `slack`; FIXED_PAIRS (step 0, step 2^31 - 1,
    seeds above 2^32) come first where they qualify, and arbitrary further pairs fill up to n_min.  -> [(seed, step, id)]"""
    out, want = [], set(int(i) for i in want_ids)
    for s, t in FIXED_PAIRS:
        i, sl = draw_ref(F, s, t)
        if sl >= slack:
            out.append((s, t, i))
            want.discard(i)
    seen = {(s, t) for s, t, _ in out}

    def add(s, t, i):
        if (s, t) not in seen:
            seen.add((s, t))
            out.append((s, t, i))
            want.discard(i)
    if F.top_k == 1:                     # u = 0 whatever the pair: every pair draws the same id
        assert not want
        return out + [(s, 1 + j, out[0][2]) for j, s in enumerate(POOL_SEEDS[:max(0, n_min - len(out))])]
    cum = F.cum.astype(np.float64)       # (exact: every partial sum is below 2^53)
    has = np.flatnonzero(F.mass)
    flat = F.Zk == has.size * Q1         # an exact row: the n-th id with mass is drawn where floor(u * n_kept) == n
    for j in range(len(POOL_SEEDS)):
        if not want and len(out) >= n_min:
            break
        seed, u = _pool(j)
        t = u * float(F.Zk)
        if flat:
            ids = has[(t * (1.0 / Q1)).astype(np.int64)]
        else:
            ids = np.searchsorted(F.cum, np.minimum(t, float(F.Zk - 1)).astype(np.uint64), side="right")
        hi = cum[ids]
        lo = hi - F.mass[ids].astype(np.float64)
        sl = np.minimum(np.where(lo > 0, t - lo, np.inf), np.where(hi < F.Zk, hi - t, np.inf)) / F.Zk
        ok = sl >= slack
        hit = np.flatnonzero(ok & np.isin(ids, np.fromiter(want, np.int64, len(want)))) if want else np.zeros(0, np.int64)
        _, first = np.unique(ids[hit], return_index=True)
        for st in hit[first].tolist():
            add(seed, st, int(ids[st]))
        for st in np.flatnonzero(ok)[:max(0, n_min - len(out)) + 4].tolist():
            if len(out) < n_min:
                add(seed, st, int(ids[st]))
    assert not want, f"no pair found for ids {sorted(want)[:8]} ..."
    return out


# ----------------------------------------------------------------------------------------------------------------------- exact rows
EXACT_V = (1, 2, 63, 64, 1023, 1024, 1025, 2047, 2049, 42003)
BIG_V = 1 << 20
EXACT_C = np.float32(-2.5)


def thread_range(V, t):
    per = -(-V // NT)
    return min(V, t * per), min(V, (t + 1) * per)


def exact_patterns(V):
    """-> [(name, kept ids)]: every logit is EXACT_C on the kept ids and -inf elsewhere"""
    per, out = -(-V // NT), [("none banned", np.arange(V))]
    if V == BIG_V:
        return out + [("every second id banned", np.arange(1, V, 2))]
    if V > 1:
        out += [("only id 0", np.array([0])), ("only id V - 1", np.array([V - 1]))]
        last = (V - 1) // per                                   # the last thread that owns an id
        out.append(("only the last thread's range", np.arange(*thread_range(V, last))))
        # kept ranges whose neighbouring threads own nothing kept: threads 1, 5 and last - 2 where V has them
        ts = sorted({t for t in (1, 5, last - 2) if 0 < t < last})
        if ts:
            out.append(("only ranges between empty neighbours", np.concatenate([np.arange(*thread_range(V, t)) for t in ts])))
        if V >= 63:
            out.append(("every third id", np.arange(V % 3, V, 3)))
    return out


def exact_row(V, kept):
    row = np.full(V, NINF, np.float32)
    row[kept] = EXACT_C
    return row


def edge_ids(V, kept):
    """the first and the last kept id, and the kept ids on both sides of every thread-range boundary that has kept ids next to it"""
    per = -(-V // NT)
    kept = np.asarray(kept)
    t = kept // per
    edge = np.r_[True, t[1:] != t[:-1]] | np.r_[t[1:] != t[:-1], True]     # first or last kept id of its thread
    return sorted(set(kept[edge].tolist()))


def exact_pairs(V, kept):
    """>= 64 pairs for the row: the n-th kept id is drawn where floor(u * n_kept) == n"""
    F = filter_ref(exact_row(V, kept))
    return F, pairs_for(F, edge_ids(V, kept), n_min=64)


# ----------------------------------------------------------------------------------------------------------------------- level rows
LV = 3001                      # per = 3; no multiple of 64, of the thread count or of a segment length used below
PZ, NZ = np.float32(0.0), np.float32(-0.0)


def f32_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def level_row(levels, seed, V=LV):
    """levels: [(f32 value, count)]; the rest of the V ids is -inf.  Scattered over the index range by a seeded permutation."""
    vals = np.concatenate([np.full(n, v, np.float32) for v, n in levels])
    assert vals.size <= V
    row = np.full(V, NINF, np.float32)
    row[:vals.size] = vals
    return row[np.random.default_rng(seed).permutation(V)]


def fkey(x):
    """the kernel's order-preserving key of an f32"""
    u = int(np.array([x], np.float32).view(np.uint32)[0])
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


BASE = [(3.0, 4), (2.0, 10), (1.0, 30), (0.0, 100), (-2.0, 2757)]                    # + 100 banned: the top-p rows
TOPK = [(4.0, 3), (3.0, 5), (2.5, 40), (1.0, 200), (NZ, 7), (PZ, 6), (-1.0, 500), (-2.0, 2140)]     # + 100 banned: 2901 finite
NEG = [(-1.0, 3), (-1.5, 5), (-3.0, 40), (-6.0, 2900)]
ZERO = [(2.0, 2), (PZ, 3), (NZ, 4), (-1.0, 2900)]
ULP = [(f32_bits(0x3FC00005), 2), (f32_bits(0x3FC00002), 3), (f32_bits(0x3FC00001), 4), (f32_bits(0x3FC00000), 5), (0.5, 2900)]
HUGE = [(f32_bits(0x7F000000), 3), (f32_bits(0x7EFF0000), 4), (1.0, 2800)]            # 2^127: key 0xFF000000
D16 = [(2.0, 2), (f32_bits(0x3FFF0000), 3), (f32_bits(0x3FFE0000), 4), (1.0, 2900)]  # 1.9921875: key 0xBFFF0000
TINY = [(3.0, 4), (2.0, 10), (-21.0, 2900)]                                            # e(-24) < 2^-32: q = 0 although e > 0
EQR = [(22.0, 1), (3.0, 10), (2.0, 20), (0.0, 96)]      # masses 2^32, 24, 8 and 1: small integers that no few-ulp error of exp moves
TEMP = [(2.0, 3), (1.875, 5), (1.75, 40), (1.625, 200), (0.5, 2600), (NZ, 20), (-0.5, 33)]


def _c(name, levels, keep, T=1.0, k=0, p=1.0, min_p=0.0, **kw):
    return dict(name=name, levels=levels, keep=keep, T=T, k=k, p=p, min_p=min_p, **kw)


# keep: the level VALUES whose ids have positive probability (0.0 stands for both zeros).  digits: {shift: digit of the k-th key}.
# straddle: the value of the tie block that R falls into (kept whole); fits: the value of the last block that fits under R (dropped).
# equal_R: the one row whose decision is an equality instead of a margin.  With top_p = 1 - 2^-24 and one id at the maximum R is
# floor(2^-24 * Ztot) = 256 whatever the small masses are, and the two lowest blocks weigh 96 * 1 + 20 * 8 = 256: a block whose
# cumulative mass EQUALS R still fits under it.
LEVEL_CASES = [
    _c("k=1, three-way tie at the maximum", TOPK, [4.0], k=1, lowest=True),
    _c("k = the top block", TOPK, [4.0], k=3),
    _c("k = the top block - 1", TOPK, [4.0], k=2),
    _c("k ends inside the second block", TOPK, [4.0, 3.0], k=7),
    _c("k = finite logits", TOPK, [4.0, 3.0, 2.5, 1.0, 0.0, -1.0, -2.0], k=2901),
    _c("k = finite logits + 1", TOPK, [4.0, 3.0, 2.5, 1.0, 0.0, -1.0, -2.0], k=2902, digits={24: 0x00, 16: 0x7F, 8: 0xFF, 0: 0xFF}),
    _c("k = V - 1", TOPK, [4.0, 3.0, 2.5, 1.0, 0.0, -1.0, -2.0], k=LV - 1),
    _c("k = V", TOPK, [4.0, 3.0, 2.5, 1.0, 0.0, -1.0, -2.0], k=LV),
    _c("k > V", TOPK, [4.0, 3.0, 2.5, 1.0, 0.0, -1.0, -2.0], k=LV + 7),
    _c("keys differ in the last byte only", ULP, [ULP[0][0], ULP[1][0]], k=4, digits={24: 0xBF, 16: 0xC0, 8: 0x00, 0: 0x02}),
    _c("k-th key 0xFF000000", HUGE, [HUGE[0][0]], k=2, digits={24: 0xFF, 16: 0x00, 8: 0x00, 0: 0x00}),
    _c("k-th key 0xBFFF0000", D16, [2.0, D16[1][0]], k=4, digits={24: 0xBF, 16: 0xFF, 8: 0x00, 0: 0x00}),
    _c("all negative", NEG, [-1.0, -1.5], k=5),
    _c("all negative, T=0.7", NEG, [-1.0, -1.5, -3.0], k=9, T=0.7),
    _c("signed zeros at the k-th rank, T=1", ZERO, [2.0, 0.0], k=4, signed_zero=True),
    _c("signed zeros at the k-th rank, T=0.7", ZERO, [2.0, 0.0], k=4, T=0.7, signed_zero=True),
    _c("top-p: tie block straddles R", BASE, [3.0, 2.0, 1.0, 0.0], p=0.4, straddle=0.0, fits=-2.0),
    _c("top-p: the block fits under R", BASE, [3.0, 2.0, 1.0], p=0.32, straddle=1.0, fits=0.0),
    _c("top-p = 1e-6", BASE, [3.0], p=1e-6, straddle=3.0, fits=2.0),
    _c("top-p = nextafter(1, 0)", BASE, [3.0, 2.0, 1.0, 0.0, -2.0], p=F32_ONE_BELOW, straddle=-2.0),
    _c("top-k leaves a tie block, top-p drops it", BASE, [3.0], k=6, p=0.5, straddle=3.0, fits=2.0),
    _c("top-k leaves a tie block, top-p keeps it", BASE, [3.0, 2.0], k=6, p=0.6, straddle=2.0),
    _c("e > 0 with q = 0", TINY, [3.0, 2.0], zero_mass=-21.0),
    _c("e > 0 with q = 0 under top-p", TINY, [3.0, 2.0], p=0.9, zero_mass=-21.0, straddle=2.0),
    _c("min-p", BASE, [3.0, 2.0, 1.0], min_p=0.1),
    _c("T=0.05", TEMP, [2.0, 1.875, 1.75, 1.625], T=0.05, p=0.99, straddle=1.625, zero_mass=0.5),
    _c("T=1", TEMP, [2.0, 1.875, 1.75, 1.625, 0.5], T=1.0, p=0.95, straddle=0.5, fits=0.0),
    _c("top-p: cumulative mass equal to R", EQR, [22.0, 3.0], p=F32_ONE_BELOW, straddle=3.0, fits=2.0, equal_R=True),
    _c("T=8", TEMP, [2.0, 1.875, 1.75, 1.625, 0.5, 0.0], T=8.0, p=0.987, straddle=0.0, fits=-0.5),
]
LEVEL_PAIRS = 8


@functools.lru_cache(maxsize=None)
def level_case(i):
    """-> (case, row, Filtered, [(seed, step, token)]): LEVEL_PAIRS pairs or more, every one with slack >= SLACK, covering the first
    and the last id with mass where its interval is wide enough for that slack (4 * SLACK of the kept mass)"""
    c = LEVEL_CASES[i]
    row = level_row(c["levels"], 1000 + i)
    row.setflags(write=False)
    F = filter_ref(row, c["T"], c["k"], c["p"], c["min_p"])
    has = np.flatnonzero(F.mass)
    ends = [i for i in (has[0], has[-1])[:1 if c["k"] == 1 else 2] if int(F.mass[i]) >= 4 * SLACK * F.Zk]
    return c, row, F, pairs_for(F, ends, n_min=LEVEL_PAIRS, slack=SLACK)


def keep_mask(c, row):
    """the case's STATED expectation: ids whose level value is in c['keep']"""
    return np.isin(row, np.array(c["keep"], np.float32))
