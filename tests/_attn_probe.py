"""Shared helper of tests/test_attn_exact_gpu.py and tests/test_attn_probe_cpu.py: read the visibility matrix and the softmax weights
themselves out of an attention kernel and compare them, element by element, with an fp64 reference.

Probe method: V is one-hot.  Per launch dh probe keys j_0 .. j_{dh-1} get V[j_c, c] = 1 (everything else 0), so column c of the
output row of query i IS the softmax weight p(i, j_c), rounded to bf16; ceil(Skv / dh) launches recover the whole weight matrix.
All inputs are exactly representable in bf16, so the fp64 reference sees the kernel's inputs.

The checker (check_weights) takes "a function that returns the weight matrix": on the GPU that is the probe launches, on the CPU
(test_attn_probe_cpu.py) an fp64 attention with the two bf16 roundings of a flash-attention kernel (emulate_weights), which is also
where deliberately wrong masks are built to show the checker rejects them.

  assertion 1 (exact):     a weight whose key is invisible in the reference is == 0.0
  assertion 2 (relative):  a visible weight with p_ref >= floor satisfies |p - p_ref| <= TOL * p_ref; below the floor (allowed only
                           where tail_ok: the bidirectional kernels drop key tiles 40 binades under the running maximum by design)
                           only 0 <= p <= (1 + TOL) * p_ref (+ one bf16 subnormal step, 2^-133, where p_ref itself is under the
                           smallest normal bf16 and no bf16 output can be relatively accurate).
TOL = 2^-6: P is rounded to bf16 before P.V and the output is rounded to bf16, each up to 2^-8 relative; a factor 2 is left for the
exp2 approximation and the f32 accumulation (test_attn_probe_cpu.py prints what the two roundings alone need: < 2^-7).
"""
import math

import torch

TOL = 2.0 ** -6
FLOOR_BIDIR = 2.0 ** -24     # mode 0: two-sided bound down to here, one-sided below (far-tile skipping)
FLOOR_EXACT = 2.0 ** -100    # causal / decode kernels skip fully masked tiles only: two-sided for every visible weight of the tests
BF = torch.bfloat16
# Under the smallest normal bf16 the format's rounding error is absolute, not 2^-8 relative: the two roundings TOL is derived from
# (P, output) are each up to half a subnormal step there.  Only the one-sided far-tail bound of mode 0 can meet such weights.
BF16_MIN_NORMAL = 2.0 ** -126
BF16_SUBNORMAL_STEP = 2.0 ** -133
PAD_BIG = 1.0e3              # value of the padding keys [Skv, Skv_alloc): finite, as the header promises, and loud if it leaks


# ------------------------------------------------------------------------------------------------------------------ checker
class Stats:
    """what one or more check_weights calls looked at (printed per kernel path by the GPU tests)"""

    def __init__(self):
        self.pairs = self.zeros = self.tail = 0
        self.worst = 0.0

    def add(self, o):
        self.pairs += o.pairs; self.zeros += o.zeros; self.tail += o.tail
        self.worst = max(self.worst, o.worst)
        return self

    def line(self, what):
        share = self.tail / max(1, self.pairs)
        return (f"[attn-probe] {what}: {self.pairs} (query, key) pairs, {self.zeros} exact-zero checks, worst |p - p_ref| / (tol * p_ref) = "
                f"{self.worst:.3f}, one-sided (p_ref < floor) share {share:.2e}")


def check_weights(weights_fn, ref, vis, *, tol=TOL, floor=FLOOR_EXACT, tail_ok=False, what=""):
    """weights_fn() -> [..., Sq, Skv] weights (any float dtype); ref fp64 and vis bool of the same shape.  Raises AssertionError
    naming the first offending (index, got, ref); returns Stats."""
    got = weights_fn().double().cpu()
    assert got.shape == ref.shape == vis.shape, (got.shape, ref.shape, vis.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite weight at {_first(~torch.isfinite(got), got, ref)}"
    st = Stats()
    st.pairs = got.numel()
    hidden = ~vis
    st.zeros = int(hidden.sum())
    bad = hidden & (got != 0)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} invisible keys carry weight, first (index, got, ref) {_first(bad, got, ref)}"
    two = vis & (ref >= floor)
    tail = vis & ~two
    st.tail = int(tail.sum())
    assert tail_ok or st.tail == 0, f"{what}: {st.tail} visible reference weights under the two-sided floor {floor:g}: {_first(tail, got, ref)}"
    err = (got - ref).abs()
    bad = two & (err > tol * ref)
    ratio = torch.where(two, err / (tol * ref.clamp_min(1e-300)), torch.zeros_like(err))
    st.worst = float(ratio.max()) if ratio.numel() else 0.0
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} visible weights off by more than {tol:g} relative (worst ratio {st.worst:.3g}), "
                                 f"first (index, got, ref) {_first(bad, got, ref)}")
    bad = tail & ((got < 0) | (got > (1 + tol) * ref + torch.where(ref < BF16_MIN_NORMAL, BF16_SUBNORMAL_STEP, 0.0)))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} far-tail weights above (1 + tol) * p_ref, first {_first(bad, got, ref)}"
    return st


def _first(mask, got, ref):
    i = tuple(int(x) for x in mask.nonzero()[0])
    return i, float(got[i]), float(ref[i])


# ------------------------------------------------------------------------------------------------------------------ references
def alibi_slopes(H):
    return torch.tensor([2.0 ** (-(h + 1) / 2) for h in range(H)])


def visibility(mode, B, Sq, Skv, q_pos0=0, window=0, kv_len=None):
    """bool [B, 1, Sq, Skv]: mode 0 keys < kv_len[b]; mode 1 keys q_pos0 + i - window < j <= q_pos0 + i (window 0 = no far edge)"""
    j = torch.arange(Skv).view(1, 1, 1, Skv)
    qp = (torch.arange(Sq) + q_pos0).view(1, 1, Sq, 1)
    vis = torch.ones(B, 1, Sq, Skv, dtype=torch.bool)
    if kv_len is not None:
        vis = vis & (j < torch.as_tensor(kv_len).view(B, 1, 1, 1))
    if mode == 1:
        vis = vis & (j <= qp)
        if window > 0:
            vis = vis & (j > qp - window)
    return vis


def scores_fp64(q, k, scale, slopes=None, q_pos0=0, col0_zero=True, dist_off=0):
    """fp64 scores [B, Hq, Sq, Skv] of bf16 q [B, Hq, Sq, dh], k [B, Hkv, Skv, dh]; slopes: the bidirectional ALiBi bias
    -slope * |i - j| (key 0 unbiased when col0_zero).  dist_off: the CPU test's "distance off by one" mutation."""
    Hq, Hkv = q.shape[1], k.shape[1]
    s = (q.double() @ k.double().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scale
    if slopes is not None:
        Sq, Skv = q.shape[2], k.shape[2]
        d = (torch.arange(Sq).view(-1, 1) + q_pos0 - torch.arange(Skv).view(1, -1) + dist_off).abs().double()
        bias = -slopes.double().view(1, Hq, 1, 1) * d
        if col0_zero:
            bias[..., 0] = 0
        s = s + bias
    return s


def softmax_ref(scores, vis):
    """fp64 softmax over the visible keys; invisible -> exactly 0"""
    s = scores.masked_fill(~vis, -float("inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    return p / p.sum(-1, keepdim=True)


def emulate_weights(scores, vis, mult=None):
    """What a correct flash-attention kernel returns through the probes, on the CPU: fp64 everywhere except the two roundings such a
    kernel has - exp(s - m) rounded to bf16 before P.V (the denominator sums the unrounded values) and the output rounded to bf16.
    mult [.., Skv] (CPU test only): how many times a key is counted (a key in two splits: 2, a dropped key: 0)."""
    vis = vis.expand_as(scores)
    s = scores.masked_fill(~vis, -float("inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    if mult is not None:
        p = p * mult
    l = p.sum(-1, keepdim=True)
    return (p.to(BF).double() / l).to(BF).double()


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gauss(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _ramp_into(K, d_hi, d_lo, sign):
    """K[..., j, d_lo] = j % 32, K[..., j, d_hi] = j // 32 (both exact in bf16 and in e4m3 up to 16): with q = a * (32 e_hi + e_lo) the
    score is a * j"""
    j = torch.arange(K.shape[-2])
    K[..., d_lo] = sign * (j % 32).float()
    K[..., d_hi] = sign * (j // 32).float()


PREFILL_FAMILIES_BIDIR = ("uniform", "alibi", "alibi_nocol0", "ramp_up", "ramp_down", "spike_first", "spike_last")
PREFILL_FAMILIES_CAUSAL = ("uniform", "ramp_up", "ramp_down", "spike_first", "spike_last")
SPIKE = 28.0        # nats = 40.4 log2 units


def prefill_case(mode, family, *, dh, B, Hq, Hkv, Sq, Skv, q_pos0=0, seed=0):
    """-> dict(q [B,Hq,Sq,dh] bf16, k [B,Hkv,Skv,dh] bf16, scale, slopes f32 [Hq] or None, col0_zero).  Score families:
    uniform: q = 0, K Gaussian (must not matter), no slopes -> p = 1 / n_visible
    alibi / alibi_nocol0 (mode 0): q = 0, slopes 2^-(h+1)/2, key-0 exception on / off
    ramp_up / ramp_down: score = +-slope * j (0.125 per key in mode 0; 1/16 in mode 1 so that no visible weight of <= 1500 keys falls
                   under 2^-100): the running maximum moves in every tile / sits in the first tile
    spike_first / spike_last: one key 28 nats (40.4 binades) above the rest, at the first (64) / last (127) key of tile 1, moved into
                   the visible range for short rows"""
    q = torch.zeros(B, Hq, Sq, dh)
    k = _gauss((B, Hkv, Skv, dh), 100 + seed)
    slopes, col0, scale = None, True, (1.0 if mode == 0 else 0.5)
    if family in ("alibi", "alibi_nocol0"):
        assert mode == 0
        slopes, col0 = alibi_slopes(Hq), family == "alibi"
    elif family in ("ramp_up", "ramp_down"):
        a = 0.125 / scale if mode == 0 else 0.0625 / scale
        k[..., 0:2] = 0
        _ramp_into(k, 1, 0, 1.0 if family == "ramp_up" else -1.0)
        q[..., 0], q[..., 1] = a, 32 * a
    elif family in ("spike_first", "spike_last"):
        k[..., 0] = 0
        for hk in range(Hkv):       # kv heads carry the spike on different keys: 64 / 127, then shifted by one tile
            j = (64 if family == "spike_first" else 127) + 64 * (hk % 2)
            k[:, hk, min(j, Skv - 1), 0] = SPIKE
        q[..., 0] = 1.0 / scale
    elif family != "uniform":
        raise ValueError(family)
    if mode == 0 and slopes is None:
        slopes = torch.zeros(Hq)
    return dict(q=q.to(BF), k=k.to(BF), scale=scale, slopes=slopes, col0_zero=col0, q_pos0=q_pos0)


def prefill_reference(mode, c, *, window=0, kv_len=None):
    """(ref fp64 [B,Hq,Sq,Skv], vis bool the same shape, scores fp64) of a prefill_case"""
    q, k = c["q"], c["k"]
    sc = scores_fp64(q, k, c["scale"], c["slopes"] if mode == 0 else None, c["q_pos0"], c["col0_zero"])
    vis = visibility(mode, q.shape[0], q.shape[2], k.shape[2], c["q_pos0"], window, kv_len).expand_as(sc)
    return softmax_ref(sc, vis), vis, sc


# ---- decode: one new token at position pos, cached keys 0 .. pos-1 + its own row
def decode_splits(pos, NS, window):
    """the key ranges [k0, k1) of the NS splits as the header defines them: keys lo .. pos with lo = max(0, pos + 1 - window), divided
    into NS chunks of ceil(n / NS)"""
    ctx = pos + 1
    lo = ctx - window if (window > 0 and ctx > window) else 0
    chunk = -(-(ctx - lo) // NS)
    return lo, [(min(ctx, lo + s * chunk), min(ctx, lo + (s + 1) * chunk)) for s in range(NS)]


DECODE_FAMILIES = ("uniform", "ramp_up", "ramp_down", "spike_split_first", "spike_split_last")


def decode_case(family, *, Hq, Hkv, ctx_max, pos, NS, window, seed=0):
    """-> dict(qkv bf16 [(Hq+2Hkv)*128] with v = 0 (the probe goes there), kc bf16 [Hkv, ctx_max, 128] "already roped" cached keys,
    scale).  The ramp lives on dims 62 / 63 (rotation angle <= 0.14 rad up to position 1023, so the roped q keeps the ramp's sign and
    size; the reference ropes q and the new k exactly as the kernel does, in bf16).  spike_split_*: the spike sits on the first key of
    split 1 / the last key of split 0 (for NS = 1: of the second / first 32-key sweep)."""
    d = 128
    qkv = torch.zeros(Hq + 2 * Hkv, d)
    kc = _gauss((Hkv, ctx_max, d), 200 + seed)
    scale = 0.5
    if family in ("ramp_up", "ramp_down"):
        kc[..., 62:64] = 0; kc[..., 126:128] = 0
        _ramp_into(kc, 62, 63, 1.0 if family == "ramp_up" else -1.0)
        qkv[:Hq, 63], qkv[:Hq, 62] = 0.0625 / scale, 32 * 0.0625 / scale
    elif family in ("spike_split_first", "spike_split_last"):
        kc[..., 63] = 0; kc[..., 127] = 0
        lo, sp = decode_splits(pos, max(NS, 1), window)
        edge = sp[0][1] if NS > 1 else lo + 32
        j = min(pos, edge if family == "spike_split_first" else max(lo, edge - 1))
        kc[:, j, 63] = SPIKE
        qkv[:Hq, 63] = 1.0 / scale
    elif family != "uniform":
        raise ValueError(family)
    kc = kc.to(BF)
    qkv[Hq:Hq + Hkv] = kc[:, pos].float()          # the new token's own (un-roped) k: the row the ramp / spike puts at key pos
    return dict(qkv=qkv.to(BF).reshape(-1), kc=kc, scale=scale, Hq=Hq, Hkv=Hkv, pos=pos, ctx_max=ctx_max)


def rope_rows(x, pos, ctx_max):
    """HF apply_rotary_pos_emb in bf16 on rows x [n, 128] at position pos (what the decode kernels do to q and the new k)"""
    from oracle import mistral_oracle as MO
    cosf, sinf = MO.rope_tables(dict(head_dim=128, rope_theta=10000.0), torch.arange(ctx_max), BF)
    return (x * cosf[pos]) + (MO.rotate_half(x) * sinf[pos])


def rope_tables64(ctx_max):
    from oracle import mistral_oracle as MO
    cosf, sinf = MO.rope_tables(dict(head_dim=128, rope_theta=10000.0), torch.arange(ctx_max), BF)
    return cosf[:, :64].contiguous(), sinf[:, :64].contiguous()


def decode_reference(c, *, window=0, k_cached=None):
    """(ref fp64 [Hq, ctx_max], vis bool [Hq, ctx_max], scores, roped new k bf16 [Hkv, 128]) of a decode_case.  k_cached: the values
    the kernel reads from the cache (the dequantized rows of an FP8 cache); the new token's own k enters unquantized."""
    Hq, Hkv, pos, ctx_max = c["Hq"], c["Hkv"], c["pos"], c["ctx_max"]
    rows = c["qkv"].view(Hq + 2 * Hkv, 128)
    qr = rope_rows(rows[:Hq], pos, ctx_max)
    kr = rope_rows(rows[Hq:Hq + Hkv], pos, ctx_max)
    K = (c["kc"] if k_cached is None else k_cached).clone()
    K[:, pos] = kr
    sc = scores_fp64(qr[None, :, None], K[None], c["scale"])[0, :, 0]          # [Hq, ctx_max]
    j = torch.arange(ctx_max)
    vis = (j <= pos) & ((j > pos - window) if window > 0 else torch.ones_like(j, dtype=torch.bool))
    vis = vis.view(1, -1).expand_as(sc)
    return softmax_ref(sc, vis), vis, sc, kr


def min_visible(ref, vis):
    return float(ref[vis].min()) if bool(vis.any()) else math.inf


# ------------------------------------------------------------------------------------------------------------------ case lists
# (shared by the GPU test, which launches them, and the CPU test, which shows that a correct kernel's two bf16 roundings pass them)
BIDIR_SQ = (17, 64, 65, 129, 300, 1118)          # ends inside a 16- / 32-query wave, at / one past a 64-key tile, past a 128-query block
CAUSAL_SHAPES = ((0, 200), (377, 200), (63, 1), (64, 65), (130, 577))      # (q_pos0, Sq), Skv = q_pos0 + Sq
CAUSAL_WINDOWS = (0, 1, 40, 64, 100, 128)
CAUSAL_CONFIGS = ((128, 1, 4, 1), (128, 1, 2, 2), (64, 2, 2, 2))           # (dh, B, Hq, Hkv)
DECODE_CTX_MAX = 1024
DECODE_POS = (0, 1, 31, 32, 63, 64, 255, 256, 699, DECODE_CTX_MAX - 1)
DECODE_NS = (2, 3, 8)
DECODE_WINDOW_POS = ((1, 0), (1, 5), (100, 31), (100, 99), (100, 100), (100, 255), (100, 699), (300, 1), (300, 299), (300, 300),
                     (300, 699), (300, DECODE_CTX_MAX - 1))                # (window, pos): pos below, at and above the window


def bidir_kv_len(Sq):
    return [Sq, max(1, Sq - 37), 1]


def causal_cases(cfg_index):
    """(q_pos0, Sq, window, families) for one head configuration: every shape x every window with the uniform family and one of the
    others in turn (every family meets every shape and every window over the list)"""
    n = cfg_index
    for q_pos0, Sq in CAUSAL_SHAPES:
        for window in CAUSAL_WINDOWS:
            n += 1
            yield q_pos0, Sq, window, ("uniform", PREFILL_FAMILIES_CAUSAL[1 + n % 4])


def decode_cases(ns_list, offset=0):
    """(pos, NS, window, G, families) of the single-sequence decode tests: every pos x NS without a window and every (window, pos) x
    NS with one (ns_list == (1,): no window, the one-workgroup form refuses it); G and the non-uniform family are dealt in turn."""
    n = offset
    both = [(0, p) for p in DECODE_POS] + (list(DECODE_WINDOW_POS) if tuple(ns_list) != (1,) else [])
    for window, pos in both:
        for NS in ns_list:
            n += 1
            yield pos, NS, window, (1, 2, 4)[n % 3], ("uniform", DECODE_FAMILIES[1 + (n // 3) % 4])
