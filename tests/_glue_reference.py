"""Plain CPU references and input builders of tests/test_glue_gpu.py (the small kernels between the GEMMs and the attention:
usdm_norm's untested paths, w2v_k.hip, vb_k.hip, bigvgan_k.hip and three entry points of llm_k.hip / llm_attn_k.hip), checked themselves by
tests/test_glue_cpu.py against the project's oracles and torch ops.

Conventions
  * a pure move, or a fixed sequence of individually rounded f32 / bf16 operations, has a reference in the SAME arithmetic (torch
    float32 / bfloat16 on the CPU): the GPU test compares bits;
  * a few f32 operations: the reference is fp64 and the bound k * 2^-23 * (sum of |terms|), k = roundings on the element's path
    (few_ops_bound);
  * reductions and transcendentals: the reference is fp64; the bound is 4 x what torch's own float32 evaluation of the same
    operation loses against fp64 on the same inputs (the *_TORCH_FP32_ERR constants below, each recomputed by test_glue_cpu.py
    with the *_torch_err function next to it).  The factor 4 is the one tests/test_attn_exact_gpu.py::test_softmax_alibi_weights
    uses: a 64-lane tree sum and the device's expf / erff / sinf differ from torch's order and polynomials by a few ulp.
Each constant is the measured figure (in its comment) rounded up by at most a tenth: torch's vectorised float32 kernels differ a
little between CPUs, and the CPU test also refuses a constant more than a quarter above what it measures.
Every error of the third kind is measured as max |got - ref| / max |ref| (tests/test_kernels_gpu.py::_close), except the softmax
weights (relative per weight, tests/_attn_probe.check_weights) and the time token (absolute: sines and cosines).
"""
import math

import torch
import torch.nn.functional as Fn

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
ULP32 = 2.0 ** -23
SENT32 = 7.0            # sentinel of every f32 / integer output buffer
SENT16_BITS = 0x7f7f    # ... and of every bf16 one (a finite bf16, 3.39e38)


# ------------------------------------------------------------------------------------------------------------------ helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def bits(t):
    """the bit pattern of a float tensor as integers (so that torch.equal tells -0.0 from 0.0 and compares NaN-free sentinels)"""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def sentinel(shape, dtype, device=None):
    """a buffer pre-filled with the sentinel of its dtype"""
    if dtype == BF:
        return torch.full(shape, SENT16_BITS, dtype=torch.int16, device=device).view(BF)
    return torch.full(shape, SENT32, dtype=dtype, device=device)


def is_sentinel(t):
    """bool tensor: which elements still hold the sentinel, bit for bit"""
    t = t.detach().cpu()
    if t.dtype == BF:
        return bits(t) == SENT16_BITS
    return bits(t) == bits(torch.full((1,), SENT32, dtype=t.dtype))


def few_ops_bound(k, *terms):
    """k * 2^-23 * (|term| + ...), element by element, fp64"""
    s = sum(t.double().abs() if torch.is_tensor(t) else abs(float(t)) for t in terms)
    return k * ULP32 * s


def bf16_of_f32_bound(ref, tol32):
    """|bf16(v) - ref| for any f32 v with |v - ref| <= tol32: the distance v may have from ref plus half a bf16 ulp of v
    (2^-8 relative at worst: 8 significant bits, so an ulp is 2^-7 of the value's power of two, round to nearest)"""
    return tol32 + 2.0 ** -8 * (ref.abs() + tol32)


def rel_to_max(got, ref):
    """max |got - ref| / max |ref| (the measure of tests/test_kernels_gpu.py::_close)"""
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


# ------------------------------------------------------------------------------------------------------------------ usdm_norm
NORM_ROWS = 7                                                  # one workgroup of 4 rows + a tail of 3
NORM_WIDTHS = (4, 64, 260, 768, 1028, 4100, 4352, 5120)        # <2> partial / one piece; <2>; <2> partial; <5> idle; <5>; <MAXP> x3
NORM_LN_TOL = 2e-6          # x max |ref|: the bound of tests/test_kernels_gpu.py::test_layernorm_and_rms, kept (see norm_ln_torch_err)
NORM_EPS = 1e-5


def norm_inputs(rows, C, seed, x_dtype=F32, res_dtype=F32, n_res2=0):
    """x, res [rows, C] in their dtypes, r2 [n_res2, rows, C] f32, gamma, beta [C] f32; rows get different offsets and scales so
    that a wrong mean or a neighbour's row shows"""
    sc = torch.exp(randn((rows, 1), seed + 5) * 0.5)
    x = (randn((rows, C), seed) * sc + randn((rows, 1), seed + 6)).to(x_dtype)
    res = randn((rows, C), seed + 1).to(res_dtype)
    r2 = randn((n_res2, rows, C), seed + 2) if n_res2 else None
    return x, res, r2, 1.0 + 0.5 * randn((C,), seed + 3), randn((C,), seed + 4)


def norm_sum32(x, res=None, r2=None, round_bf16=False):
    """the row the kernel normalises, in its own arithmetic: float32 (((x + res) [-> bf16]) + r2[0]) + r2[1] ..., in that order"""
    v = x.float()
    if res is not None:
        v = v + res.float()
        if round_bf16:
            v = v.to(BF).float()
    if r2 is not None:
        for e in range(r2.shape[0]):
            v = v + r2[e]
    return v


def norm_ref(s, gamma, beta=None, *, rms=False, gelu=False, eps=NORM_EPS, dtype=F64):
    """LayerNorm / RMSNorm (+ GELU) of the rows s in `dtype` (fp64: the reference; float32: torch's own, to size a bound)"""
    s, g = s.to(dtype), gamma.to(dtype)
    if rms:
        y = s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps) * g
        if beta is not None:
            y = y + beta.to(dtype)
    else:
        y = Fn.layer_norm(s, (s.shape[-1],), g, None if beta is None else beta.to(dtype), eps)
    return Fn.gelu(y) if gelu else y


def norm_row_mask(rows, valid_len, rows_per_batch):
    """bool [rows]: the rows at or past their batch's valid_len (the kernel's srow >= vlen)"""
    r = torch.arange(rows)
    return (r % rows_per_batch) >= torch.as_tensor(valid_len)[r // rows_per_batch]


def norm_rms_hf_ref(sum16, gamma_bf):
    """HF MistralRMSNorm on the bf16 residual sum, fp64: gamma_bf16 * normalised (the two bf16 roundings are the bound's business)"""
    s = sum16.double()
    return gamma_bf.double() * (s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + NORM_EPS))


def norm_ln_torch_err():
    """worst max |torch float32 layer_norm - fp64| / max |ref| over the widths of the GPU test (its inputs)"""
    worst = 0.0
    for C in NORM_WIDTHS:
        x, res, _, g, b = norm_inputs(NORM_ROWS, C, 100 + C)
        s = norm_sum32(x, res)
        worst = max(worst, rel_to_max(norm_ref(s, g, b, dtype=F32), norm_ref(s, g, b)))
    return worst


NORM_RMS_C = (260, 1028, 4100)
NORM_RMS_TORCH_FP32_ERR = 1.1e-7     # measured on the CPU: 1.01e-7 (x max |ref|, rms without round_bf16 at C = 260 / 1028 / 4100)
NORM_GELU_TORCH_FP32_ERR = 2.1e-7    # measured on the CPU: 1.95e-7 (x max |ref|, LayerNorm + GELU at C = 768)


def norm_rms_case(C):
    x, _, _, g, _ = norm_inputs(NORM_ROWS, C, 300 + C)
    return x, g


def norm_rms_torch_err():
    return max(rel_to_max(norm_ref(x, g, rms=True, dtype=F32), norm_ref(x, g, rms=True)) for x, g in map(norm_rms_case, NORM_RMS_C))


def norm_gelu_case():
    x, res, _, g, b = norm_inputs(NORM_ROWS, 768, 400)
    return x, res, g, b


def norm_gelu_torch_err():
    x, res, g, b = norm_gelu_case()
    s = norm_sum32(x, res)
    return rel_to_max(norm_ref(s, g, b, gelu=True, dtype=F32), norm_ref(s, g, b, gelu=True))


# ------------------------------------------------------------------------------------------------------------------ w2v_k.hip
def wave(n, seed, dc=0.3):
    """the sinusoid mix of tests/test_tokenizer_gpu._wave on a DC offset (the mean the kernel has to remove)"""
    g = gen(seed)
    t = torch.arange(n) / 16000.0
    w = sum(torch.sin(2 * torch.pi * f * t + p) for f, p in zip((110, 220, 450, 900, 1800, 3100), torch.rand(6, generator=g) * 6.28))
    return (dc + 0.05 * w + 0.02 * torch.randn(n, generator=g)).float()


WAVE_LN_N = (2, 1000, 1024, 1025, 48001)
WAVE_LN_TORCH_FP32_ERR = 2.9e-7      # measured on the CPU: 2.61e-7 (x max |y|; the DC offset costs x - mean three bits)


def wave_layernorm_ref(x, eps=1e-5, dtype=F64):
    return Fn.layer_norm(x.to(dtype), (x.numel(),), None, None, eps)


def wave_layernorm_torch_err():
    return max(rel_to_max(wave_layernorm_ref(x, dtype=F32), wave_layernorm_ref(x)) for x in (wave(n, 7 + n) for n in WAVE_LN_N))


CONV0_C, CONV0_K = 512, 10
CONV0_STRIDES, CONV0_T = (1, 3, 5, 8), (1, 63, 64, 65, 200)
CONV0_TORCH_FP32_ERR = 3.5e-7        # measured on the CPU: 3.19e-7 (x max |ref|, worst of the 40 cases)


def conv0_params():
    C, k = CONV0_C, CONV0_K
    return randn((C, k), 21, 0.4), randn((C,), 22, 0.2), 1.0 + 0.3 * randn((C,), 23), randn((C,), 24, 0.3)


def conv0_cases():
    """(stride, T, n): n = (T-1)*stride + 10 exactly (the last workgroup's staged window runs past n), and 1000 samples longer"""
    for stride in CONV0_STRIDES:
        for T in CONV0_T:
            for extra in (0, 1000):
                yield stride, T, (T - 1) * stride + CONV0_K + extra


def conv0_wave(n):
    """a waveform as the kernel meets it: already normalised by wave_layernorm (zero mean, unit variance); the last sample is loud,
    so that the frame that ends on it depends on it"""
    x = wave_layernorm_ref(wave(max(n, 2), 31 + n)).float()[:n].clone()
    x[-1] = 2.5
    return x


def conv0_ref(x, T, stride, w, b, g, be, eps=1e-5, dtype=F64):
    """Conv1d(1 -> C, k, stride) -> LayerNorm(C) -> GELU, channels-last [T, C]"""
    y = Fn.conv1d(x.to(dtype)[None, None], w.to(dtype)[:, None, :], b.to(dtype), stride=stride)[0, :, :T].T
    return Fn.gelu(Fn.layer_norm(y, (w.shape[0],), g.to(dtype), be.to(dtype), eps))


def conv0_torch_err():
    p = conv0_params()
    return max(rel_to_max(conv0_ref(x, T, s, *p, dtype=F32), conv0_ref(x, T, s, *p)) for s, T, x in
               ((s, T, conv0_wave(n)) for s, T, n in conv0_cases()))


SOFTMAX_SEG_N = (1, 63, 64, 150)
SOFTMAX_SEG_TORCH_FP32_ERR = 2.3e-6  # measured on the CPU: 2.08e-6 relative per weight (|x - max| reaches 55, where one f32 ulp is 3.8e-6)


def softmax_seg_inputs(n, rows=5, nseg=3):
    """scores [rows, nseg, n]: Gaussian * 3, one dominant column (+12) and one far in the tail (-30), as _softmax_alibi_inputs"""
    x = randn((rows, nseg, n), 50 + n, 3.0)
    x[:, :, min(7, n - 1)] += 12.0
    if n > 20:
        x[:, :, n - 2] -= 30.0
    return x


def softmax_seg_ref(x, dtype=F64):
    return torch.softmax(x.to(dtype), -1)


def softmax_seg_torch_err():
    worst = 0.0
    for n in SOFTMAX_SEG_N:
        x = softmax_seg_inputs(n)
        ref = softmax_seg_ref(x)
        assert float(ref.min()) >= 2.0 ** -100, "a weight under the two-sided floor"
        worst = max(worst, float(((softmax_seg_ref(x, F32).double() - ref).abs() / ref).max()))
    return worst


KMEANS_T = 6
KMEANS_PAD = 3


def kmeans_case(D, n_units, seed=0):
    """All-integer inputs (every f32 operation of the kernel is exact) with planted minima, one per frame:
      0: the minimum at unit 0                          3: a tie of units 10 and 40 (two lanes of wave 0)
      1: the minimum at the last unit                   4: a tie of units 100 and 70 (two lanes of wave 1, the later lane lower)
      2: a tie of units 5 and 261 (one thread)          5: a three-way tie of 300, 70, 200: thread 44 of wave 0 (its second unit),
                                                           wave 1 and wave 3 - the lowest index sits in neither the first wave
                                                           nor the first pass (n_units <= 300: of 250, 70, 200)
    A plant whose units do not all exist (small n_units) is left out: the frame keeps its random distances, ties included.
    -> x f32 [T, D], dots f32 [T, n_units + 3] (pad columns would win if read), csq f32 [n_units]."""
    T, g = KMEANS_T, gen(900 + D + n_units + seed)
    x = torch.randint(-3, 4, (T, D), generator=g).double()
    xsq = x.pow(2).sum(1, keepdim=True)
    csq = 2.0 * torch.randint(0, 500, (n_units,), generator=g).double()                 # even: the parity of a distance depends on the frame only
    dist = 2.0 * torch.randint(50, 2500, (T, n_units), generator=g).double() + xsq % 2  # background, >= 100
    plants = {0: (0,), 1: (n_units - 1,), 2: (5, 261), 3: (10, 40), 4: (100, 70), 5: (300, 70, 200) if n_units > 300 else (250, 70, 200)}
    for t, units in plants.items():
        if max(units) < n_units:
            dist[t, list(units)] = 6.0 + 2 * t + float(xsq[t] % 2)
    dots = (xsq + csq - dist) / 2
    full = torch.full((T, n_units + KMEANS_PAD), 1.0e6, dtype=F64)
    full[:, :n_units] = dots
    for v in (xsq, 2 * dots, xsq - 2 * dots, dist, csq):
        assert float(v.abs().max()) < 2 ** 24 and bool((v == v.round()).all()), "not an exact f32 integer"
    return x.float(), full.float(), csq.float()


def kmeans_ref(x, dots, csq):
    """(ids int64 [T], margin f32 [T], dist fp64 [T, n_units]): argmin of (|x|^2 - 2 dots) + csq, the lowest index on a tie;
    margin = second smallest - smallest (duplicates count: 0 at a tie), inf for a single unit"""
    n = csq.numel()
    dist = (x.double().pow(2).sum(1, keepdim=True) - 2 * dots.double()[:, :n]) + csq.double()
    srt = torch.sort(dist, dim=1).values
    second = srt[:, 1] if n > 1 else torch.full((dist.shape[0],), math.inf, dtype=F64)
    return dist.argmin(1), (second - srt[:, 0]).float(), dist


# ------------------------------------------------------------------------------------------------------------------ vb_k.hip
def vb_input_case(E, dtype, B_in=2, S=9, F=5, V=11):
    g = gen(60 + E)
    ids = torch.randint(1, V - 1, (B_in, S), generator=g)
    ids[0, 0], ids[0, 1], ids[1, S - 1] = 0, V - 1, V - 1          # row 0 and the last row (= null_id)
    return ids, randn((B_in, F, S), 61), randn((B_in, F, S), 62), randn((V, E), 63).to(dtype)


def vb_build_input_ref(ids, y, cond, table, *, dup, use_cond, null_id, ldo):
    """[B_in * dup, S, ldo] in the table's dtype: table[id] | y[:, s] | cond[:, s] | 0 ...; dup == 2: the first B_in batches are the
    unconditional copy (null row, zero cond)"""
    B_in, S = ids.shape
    F, E, dt = y.shape[1], table.shape[1], table.dtype
    out = torch.zeros(B_in * dup, S, ldo, dtype=dt)
    for bx in range(B_in * dup):
        b, uncond = bx % B_in, dup == 2 and bx < B_in
        out[bx, :, :E] = table[torch.full((S,), null_id) if uncond else ids[b]]
        out[bx, :, E:E + F] = y[b].T.to(dt)
        if use_cond and not uncond:
            out[bx, :, E + F:E + 2 * F] = cond[b].T.to(dt)
    return out


TIME_TOKEN_TORCH_FP32_ERR = 3.9e-8   # measured on the CPU: 3.54e-8 absolute (sines and cosines of float32 arguments up to 1000)
TIME_TOKEN_T = ((0.0, 1e-3, 0.5), (1.0, 0.5, 0.0))


def time_token_freqs(H):
    half = H // 2
    return torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1)))      # (usdm_amd/voicebox/model/networks.py)


def time_token_arg(t, freqs):
    """(1000 t) * freqs[i] in float32, in the kernel's two multiplications"""
    return (torch.tensor(1000.0) * t.float()).view(-1, 1) * freqs.view(1, -1)


def time_token_ref(t, freqs, dtype=F64):
    a = time_token_arg(t, freqs).to(dtype)
    return torch.cat([a.sin(), a.cos()], -1)


def time_token_torch_err():
    return max(float((time_token_ref(torch.tensor(t), time_token_freqs(H), F32).double() - time_token_ref(torch.tensor(t), time_token_freqs(H))).abs().max())
               for t in TIME_TOKEN_T for H in (16, 1024))


def solver_case(seed, B=2, F=5, S=67):
    n = B * F * S
    return dict(vout=randn((2 * n,), seed), z=randn((n,), seed + 1), eps=randn((n,), seed + 2), cond=randn((n,), seed + 3),
                vout2=randn((2 * n,), seed + 4), B=B, F=F, S=S, n=n)


def solver_ref(vout, z, *, S, mode, dt, cfg=False, gs=0.0, v1=None, eps=None, cond=None, P=0, c_eps=0.0, c_cond=0.0):
    """one pass of vb_solver_kernel in fp64 on flat [B*F*S] tensors -> (zn, v, bound): the new z, the combined velocity, and
    k * 2^-23 * sum|terms| per element.  Roundings counted (every f32 operation once; the scalars dt, gs, c_* are float32 values):
      v:      cfg: vc - vu, gs * (.), vc + (.) -> 3 over |vc| + |gs| (|vc| + |vu|); else a copy -> 0
      Euler:  dt * v, z + (.) -> kv + 2 over |z| + |dt| |v|terms
      Heun corrector: v1 + v, dt * (.), / 2 is exact, z + (.) -> kv + 3 over |z| + |dt| (|v1| + |v|terms) / 2
      re-noised columns (s < P): c_eps * eps, c_cond * cond, their sum -> 3 over |c_eps eps| + |c_cond cond|"""
    f = lambda s: float(torch.tensor(s, dtype=F32))
    dt, gs, c_eps, c_cond = f(dt), f(gs), f(c_eps), f(c_cond)
    n = z.numel()
    vout, z = vout.double(), z.double()
    if cfg:
        vu, vc = vout[:n], vout[n:2 * n]
        v, vterms, kv = vc + gs * (vc - vu), vc.abs() + abs(gs) * (vc.abs() + vu.abs()), 3
    else:
        v, vterms, kv = vout[:n], vout[:n].abs(), 0
    if mode == 0:
        zn, bound = z + dt * v, few_ops_bound(kv + 2, z, abs(dt) * vterms)
    else:
        v1 = v1.double()
        zn, bound = z + (dt * (v1 + v)) / 2, few_ops_bound(kv + 3, z, abs(dt) * (v1.abs() + vterms) / 2)
    if eps is not None:
        col = (torch.arange(n) % S) < P
        rn = c_eps * eps.double() + c_cond * cond.double()
        zn = torch.where(col, rn, zn)
        bound = torch.where(col, few_ops_bound(3, c_eps * eps.double(), c_cond * cond.double()), bound)
    return zn, v, bound, few_ops_bound(kv, vterms)


def mask_time_ref(x, valid_len, off, layout):
    """x [B, T, C] (layout 0) or [B, C, T] (layout 1): zero where t >= valid_len[b] - off"""
    B = x.shape[0]
    T = x.shape[1] if layout == 0 else x.shape[2]
    dead = torch.arange(T).view(1, T) >= (torch.as_tensor(valid_len).view(B, 1) - off)
    dead = dead.view(B, T, 1) if layout == 0 else dead.view(B, 1, T)
    return torch.where(dead.expand_as(x), torch.zeros_like(x), x)


# ------------------------------------------------------------------------------------------------------------------ bigvgan_k.hip
def sum3_scale_ref(a, b, c, scale):
    return ((a + b) + c) * torch.tensor(scale, dtype=F32)


def cf_to_cl_ref(x, Cpad, scale=1.0, shift=0.0):
    """x [B, C, T] -> fp64 [B, T, Cpad] of x * scale + shift (scale, shift as float32 values), pad channels 0, and the k = 2 bound"""
    s, h = float(torch.tensor(scale, dtype=F32)), float(torch.tensor(shift, dtype=F32))
    B, C, T = x.shape
    ref, bound = torch.zeros(B, T, Cpad, dtype=F64), torch.zeros(B, T, Cpad, dtype=F64)
    xt = x.double().transpose(1, 2)
    ref[..., :C] = xt * s + h
    bound[..., :C] = few_ops_bound(2, xt * s, h)
    return ref, bound


def stft_window(n_fft, seed=71):
    """positive and NOT symmetric (a Hann window under a ramp), so that a reversed or shifted frame shows"""
    return (torch.hann_window(n_fft) + 0.05) * torch.linspace(0.5, 1.5, n_fft) + 0.01 * torch.rand(n_fft, generator=gen(seed))


def stft_T(n, n_fft, hop, pad):
    return 1 + (n + 2 * pad - n_fft) // hop


def stft_frames_ref(x, n_fft, hop, pad, window):
    """F.pad(reflect) -> clamp to [-1, 1] -> frames -> * window, float32: [T, n_fft]"""
    xp = Fn.pad(x[None, None], (pad, pad), mode="reflect")[0, 0].clamp(-1.0, 1.0)
    return xp.unfold(0, n_fft, hop) * window


def stft_mag_ref(re_im, nbins, eps, nbins_pad):
    """sqrt(re^2 + im^2 + eps) in fp64 (eps as its float32 value), pad bins 0, and the k = 4 bound.  Every term of the radicand is
    positive, so its relative error is at most that of its four roundings (re^2, im^2, their sum, + eps: 4 * 2^-24), halved by the
    square root, plus sqrtf's own rounding: under 4 * 2^-23 of the result."""
    e = float(torch.tensor(eps, dtype=F32))
    T = re_im.shape[0]
    ref = torch.zeros(T, nbins_pad, dtype=F64)
    re, im = re_im[:, :nbins].double(), re_im[:, nbins:2 * nbins].double()
    ref[:, :nbins] = torch.sqrt((re * re + im * im) + e)
    return ref, few_ops_bound(4, ref)


def frame_signal_ref(x, frame_len, hop, offset, T):
    """frames[t][c] = x[t * hop + c - offset], zero outside [0, n)"""
    j = torch.arange(T).view(T, 1) * hop + torch.arange(frame_len).view(1, frame_len) - offset
    ok = (j >= 0) & (j < x.numel())
    return torch.where(ok, x[j.clamp(0, x.numel() - 1)], torch.zeros((), dtype=x.dtype))


# ------------------------------------------------------------------------------------------------- llm_k.hip, llm_attn_k.hip
def residual_add_case(n):
    """h bf16 [n], delta f32 [n] with, from the front: exact bf16 ties in delta (1 + 2^-8 -> 1, -(1 + 3 * 2^-8) -> -(1 + 2^-6)),
    deltas a hair above 2^-8 on h = 1 (bf16(delta) = 2^-8 makes h + delta the tie 1 + 2^-8 -> 1; the unrounded sum goes up to
    1 + 2^-7) and their mirror images, then Gaussians"""
    h = randn((n,), 80 + n).to(BF)
    d = randn((n,), 81 + n)
    front_h = torch.tensor([0.5, 0.5, 1.0, -1.0, 1.0, 3.0])
    front_d = torch.tensor([1 + 2.0 ** -8, -(1 + 3 * 2.0 ** -8), 2.0 ** -8 + 2.0 ** -20, -(2.0 ** -8 + 2.0 ** -20), 3 * 2.0 ** -8 - 2.0 ** -21,
                            2.0 ** -7 + 2.0 ** -19])
    k = min(n, front_h.numel())
    h[:k], d[:k] = front_h[:k].to(BF), front_d[:k]
    return h, d


def residual_add_ref(h, delta):
    return (h.float() + delta.to(BF).float()).to(BF)


ROPE = dict(Hq=4, Hkv=2, S=37, ctx=128, vt_ld=64)


def rope_case(seed=3):
    """qkv bf16 [S, (Hq + 2 Hkv) * 128], row scales over several binades (tests/test_kv8_gpu.py): the inner roundings matter"""
    Hq, Hkv, S = ROPE["Hq"], ROPE["Hkv"], ROPE["S"]
    g = gen(seed)
    return (torch.randn(S, (Hq + 2 * Hkv) * 128, generator=g) * torch.exp(torch.randn(S, 1, generator=g) * 2)).to(BF)


def rope_tables(ctx):
    """bf16 (cos, sin) [ctx, 128] of oracle.mistral_oracle.rope_tables; the kernel reads the first 64 columns"""
    from oracle import mistral_oracle as MO
    return MO.rope_tables(dict(head_dim=128, rope_theta=10000.0), torch.arange(ctx), BF)


def rope_ref(heads, pos0, cos, sin):
    """HF apply_rotary_pos_emb evaluated by torch IN bfloat16 (every product and the sum round to bf16) on heads [S, H, 128]"""
    from oracle import mistral_oracle as MO
    S = heads.shape[0]
    c, s = cos[pos0:pos0 + S, None, :], sin[pos0:pos0 + S, None, :]
    return (heads * c) + (MO.rotate_half(heads) * s)
