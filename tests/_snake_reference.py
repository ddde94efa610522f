"""Plain references, case tables, checks and a float32 emulation of usdm_aa_snake (usdm_amd/csrc/bigvgan_k.hip, the fused
Activation1d(SnakeBeta) of BigVGAN), shared by tests/test_snake_cpu.py (which checks them against torch and the oracle) and
tests/test_snake_gpu.py (which runs the same checks on the kernel).  Everything here is numpy on [T][C] (channels-last) arrays.

What the kernel computes (x~, v~ index-clamped = replicate padding; a, b = alpha, beta, exp() of them when logscale):

    u[2m]   = 2 * sum_{i=-2..3} fup[5+2i] * x~[m-i]
    u[2m+1] = 2 * sum_{i=-3..2} fup[6+2i] * x~[m-i]          x~[k] = x[clamp(k, 0, T-1)]
    v[n]    = u[n] + 1/(b + 1e-9) * sin(u[n] * a)^2
    o[t]    = sum_{j=0..11} fdn[j] * v~[2t-5+j]              v~[n] = v[clamp(n, 0, 2T-1)]

fup are conv_transpose1d weights, fdn conv1d weights; channels >= Creal are written as zero whatever x, alpha and beta hold there.

The check families (each a check_* function taking a case and a `run` callable, so that the emulation and the device pass through
the same code):
  1 exact     alpha = 0, beta = 1, logscale = 0: sin(0) = 0, the activation is the identity, and with integer x and integer
              asymmetric taps every product and partial sum is an integer below 2^24: out32 == the int64 reference, out16 == its
              bf16 rounding.
  2 one tap   fup = one 0.5 (times the kernel's 2: exactly x on one phase, exactly 0 on the other), fdn = one 1.0 at j0: o[t] is
              exactly v~[2t-5+j0]: one snake evaluation of one known sample, a replicated end sample, or 0.  Compared with
              ref_snake under tol() below.
  3 chunking  real taps and data: every L, and every choice of outputs, gives the same bits; out16 = bf16(out32).
  4 strides   ldx / ldo / an offset view give the same bits as the dense call.

tol(): the bound of family 2, derived, not chosen
  The reference is ref_snake in float64 on the float32 inputs.  In family 2 u == x exactly (0.5 * x * 2 and sums of zeros), and
  the constant is the float32 1e-9f of the kernel (as torch rounds the oracle's 1e-9 to the tensors' float32).  Without logscale
  the reference takes the sine of the float32 product fl(u * a), the kernel's own argument, so the argument carries no error;
  with logscale a = expf(alpha) is off by EXP ulp and the product by another half.  No table of OCML / HIP error bounds ships
  with the ROCm tree this was written against (a search of its headers and documents for "ulp" finds only the OpenCL C header's
  remarks), so the library functions take the OpenCL full-profile bounds: sin 4 ulp, exp 3 ulp, reciprocal 2.5 ulp; every
  float32 +, * takes 0.5 ulp.  With U = 2^-23 (an ulp is at most U times the value), to first order:
      d_arg = (3 + 0.5) U |arg|                          (logscale; 0 otherwise)
      s  = sinf(arg)      d_s  = 4 U |s| + |cos(arg)| d_arg
      s2 = s * s          d_s2 = 2 |s| d_s + 0.5 U s2
      ib = 1 / (b + 1e-9) d_ib = (r_b + 0.5 + 2.5) U ib    r_b = 3 for b = expf(beta), 0 otherwise; 0.5 for the sum
      p  = ib * s2        d_p  = ib d_s2 + s2 d_ib + 0.5 U |p|
      v  = u + p          d_v  = d_p + 0.5 U |v|
      o  = 1.0 * v (+ zeros)  d_o = d_v + 0.5 U |v|      (the output's rounding; the product and the sums of zeros are exact)
  On the empty phase u = 0 and every term is 0: the bound is 0 and the output must be exactly 0.

emulate(): a numpy float32 restatement with the kernel's structure (a thread per channel pair and chunk of L steps, the 7- and
13-sample sliding windows, v_first / v_last substitution at the ends), with the planted DEFECTS the CPU test shows the families
reject.  It is evidence about the checks, not a bit-exact model of the device (numpy's sin and exp are not the device's).
"""
import numpy as np

F32, F64 = np.float32, np.float64
T_LIST = (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 127, 128, 129, 257)
L_LIST = (0, 1, 2, 3, 8, 16, 32)
C_LIST = (2, 32, 34, 66)
C_MAIN, CREAL_MAIN = 34, 33          # a second, mostly idle column block of 16 pairs; the last pair half padding
LD_PADS = (0, 2, 6)
U = 2.0 ** -23
SIN_ULP, EXP_ULP, RCP_ULP, OP_ULP = 4.0, 3.0, 2.5, 0.5
EPS32 = F32(1e-9)

DEFECTS = ("fdn_reversed", "fup_reversed", "phase_swapped", "v_zero_pad", "x_zero_pad", "neighbour_params", "eps_omitted",
           "logscale_ignored", "pad_not_zeroed", "short_window")


def cdiv(a, b):
    return -(-a // b)


def launcher_L(T, C, L):
    """time steps per thread as usdm_aa_snake chooses them for L <= 0"""
    if L > 0:
        return L
    L, cols = 32, cdiv(C, 32)
    while L > 8 and cols * cdiv(T, 16 * L) < 1024:
        L >>= 1
    return L


def bf16_bits(a):
    """round-to-nearest-even bf16 of finite float32 values, as uint16 bit patterns"""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


# ------------------------------------------------------------------------------------------------------------------ references
def _up(x, fup):
    T = x.shape[0]
    m = np.arange(T)
    u = np.zeros((2 * T,) + x.shape[1:], dtype=x.dtype)
    for i in range(-2, 4):
        u[0::2] += fup[5 + 2 * i] * x[np.clip(m - i, 0, T - 1)]
    for i in range(-3, 3):
        u[1::2] += fup[6 + 2 * i] * x[np.clip(m - i, 0, T - 1)]
    return 2 * u


def _down(v, fdn):
    N = v.shape[0]
    t = np.arange(N // 2)
    o = np.zeros((N // 2,) + v.shape[1:], dtype=v.dtype)
    for j in range(12):
        o += fdn[j] * v[np.clip(2 * t - 5 + j, 0, N - 1)]
    return o


def ref_linear(x, fup, fdn):
    """the formulas with v = u: int64 when x and the taps are integers, float64 otherwise"""
    x, fup, fdn = np.asarray(x), np.asarray(fup), np.asarray(fdn)
    dt = np.int64 if all(a.dtype.kind in "iu" for a in (x, fup, fdn)) else F64
    return _down(_up(x.astype(dt), fup.astype(dt)), fdn.astype(dt))


def _live(x, alpha, beta, Creal):
    """float32 x, alpha, beta with everything of the padding channels replaced by 0"""
    x = np.asarray(x, F32)
    live = np.arange(x.shape[1]) < Creal
    return np.where(live, x, F32(0)), np.where(live, np.asarray(alpha, F32), F32(0)), np.where(live, np.asarray(beta, F32), F32(0)), live


def _snake64(u, a32, b32, logscale):
    """-> v, arg, b in float64 from float64 u and the float32 parameters; without logscale the argument is the float32 product"""
    if logscale:
        a, b = np.exp(a32.astype(F64)), np.exp(b32.astype(F64))
        arg = u * a
    else:
        b = b32.astype(F64)
        with np.errstate(over="ignore"):
            arg = (u.astype(F32) * a32).astype(F64)
    return u + 1.0 / (b + F64(EPS32)) * np.sin(arg) ** 2, arg, b


def ref_snake(x, alpha, beta, fup, fdn, logscale, Creal):
    """the full formula in float64 from the float32 inputs; channels >= Creal are 0"""
    x, a32, b32, live = _live(x, alpha, beta, Creal)
    u = _up(x.astype(F64), np.asarray(fup, F32).astype(F64))
    v, _, _ = _snake64(u, a32, b32, logscale)
    o = _down(v, np.asarray(fdn, F32).astype(F64))
    o[:, ~live] = 0.0
    return o


def one_tap(fup, fdn):
    """(phase, j0) of a family-2 filter pair: fup = one 0.5 at index 5 (phase 0) or 6 (phase 1), fdn = one 1.0 at j0"""
    fup, fdn = np.asarray(fup, F64), np.asarray(fdn, F64)
    iu, jd = np.flatnonzero(fup), np.flatnonzero(fdn)
    assert len(iu) == 1 and iu[0] in (5, 6) and fup[iu[0]] == 0.5 and len(jd) == 1 and fdn[jd[0]] == 1.0, "tol() is derived for one-tap filters"
    return int(iu[0]) - 5, int(jd[0])


def tol(x, alpha, beta, fup, fdn, logscale, Creal):
    """the bound on |out32 - ref_snake| of family 2, element by element (the module docstring derives it)"""
    phase, j0 = one_tap(fup, fdn)
    x, a32, b32, live = _live(x, alpha, beta, Creal)
    T = x.shape[0]
    u = x.astype(F64)
    v, arg, b = _snake64(u, a32, b32, logscale)
    d_arg = (EXP_ULP + OP_ULP) * U * np.abs(arg) if logscale else 0.0
    s = np.sin(arg)
    d_s = SIN_ULP * U * np.abs(s) + np.abs(np.cos(arg)) * d_arg
    s2 = s * s
    d_s2 = 2 * np.abs(s) * d_s + OP_ULP * U * s2
    ib = 1.0 / (b + F64(EPS32))
    d_ib = ((EXP_ULP if logscale else 0.0) + OP_ULP + RCP_ULP) * U * ib
    p = ib * s2
    d_p = ib * d_s2 + s2 * d_ib + OP_ULP * U * p
    d_v = d_p + 2 * OP_ULP * U * np.abs(v)
    d_v[:, ~live] = 0.0
    full = np.zeros((2 * T, x.shape[1]))
    full[phase::2] = d_v
    return full[np.clip(2 * np.arange(T) - 5 + j0, 0, 2 * T - 1)]


# ------------------------------------------------------------------------------------------------------------------ emulation
def emulate(x, alpha, beta, fup, fdn, logscale, Creal, L=0, defect=None):
    """-> (out32 float32 [T][C], out16 bf16 bits).  All chunks advance together (axis 0 = chunk, axis 1 = channel): step i of the
    loop is the kernel's iteration m = t0 - 3 + i of every thread."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(x, F32)
    T, C = x.shape
    assert C % 2 == 0
    L = launcher_L(T, C, L)
    fu, fd = np.asarray(fup, F32), np.asarray(fdn, F32)
    if defect == "fup_reversed":
        fu = fu[::-1]
    if defect == "fdn_reversed":
        fd = fd[::-1]
    ch = np.arange(C)
    own = ch ^ 1 if defect == "neighbour_params" else ch       # a thread holds the pair (c, c + 1): the wrong one of its two
    cv = ch < Creal
    zero = np.zeros((1, C), F32)
    with np.errstate(all="ignore"):
        av = np.where(cv, np.asarray(alpha, F32)[own], F32(0))
        bv = np.where(cv, np.asarray(beta, F32)[own], F32(0))
        if logscale and defect != "logscale_ignored":
            av, bv = np.exp(av), np.exp(bv)
        ib = F32(1) / (bv if defect == "eps_omitted" else bv + EPS32)

        def ld(t):
            r = x[np.clip(t, 0, T - 1)]
            if defect == "x_zero_pad":
                r = np.where(((t < 0) | (t > T - 1))[:, None], F32(0), r)
            return r

        def up2(w):
            u0 = F32(2) * (((fu[1] * w[5] + fu[3] * w[4]) + (fu[5] * w[3] + fu[7] * w[2])) + (fu[9] * w[1] + fu[11] * w[0]))
            u1 = F32(2) * (((fu[0] * w[6] + fu[2] * w[5]) + (fu[4] * w[4] + fu[6] * w[3])) + (fu[8] * w[2] + fu[10] * w[1]))
            return (u1, u0) if defect == "phase_swapped" else (u0, u1)

        def snake1(u):
            s = np.sin(u * av)
            return u + ib * (s * s)

        at = np.zeros(1, np.int64)
        v_first = snake1(up2([ld(at + k - 3) for k in range(7)])[0])
        v_last = snake1(up2([ld(at + T - 1 + k - 3) for k in range(7)])[1])
        if defect == "v_zero_pad":
            v_first = v_last = zero

        K = cdiv(T, L)
        t0 = np.arange(K, dtype=np.int64) * L
        tend = np.minimum(t0 + L, T)
        xw = [None] + [ld(t0 - 7 + k + 1) for k in range(6)]
        vw = [np.zeros((K, C), F32)] * 13
        out = np.full((T, C), np.nan, F32)
        for i in range(L + 6):
            m = t0 - 3 + i
            xw = xw[1:] + [ld(m + 3)]
            v0, v1 = (snake1(u) for u in up2(xw))
            n0 = (2 * m)[:, None]
            v0 = np.where(n0 < 0, v_first, np.where(n0 > 2 * T - 1, v_last, v0))
            v1 = np.where(n0 + 1 < 0, v_first, np.where(n0 + 1 > 2 * T - 1, v_last, v1))
            vw = vw[2:] + [v0, v1]
            if i < 6:
                continue
            w = [np.zeros((K, C), F32)] + vw[1:] if defect == "short_window" and i == 6 else vw
            o = ((((fd[0] * w[0] + fd[1] * w[1]) + (fd[2] * w[2] + fd[3] * w[3])) + ((fd[4] * w[4] + fd[5] * w[5]) + (fd[6] * w[6] + fd[7] * w[7])))
                 + ((fd[8] * w[8] + fd[9] * w[9]) + (fd[10] * w[10] + fd[11] * w[11])))
            if defect != "pad_not_zeroed":
                o = np.where(cv, o, F32(0))
            t = m - 3
            sel = t < tend
            out[t[sel]] = o[sel]
    return out, bf16_bits(out)


def emulated_run(defect=None):
    """a `run` for the check_* functions on emulate(); x goes through the same strided, NaN-surrounded buffer as on the device"""
    def run(case, L=None, outs="both", ldx=None, ldo=None, xoff=0):
        T, C = case["x"].shape
        ldx = ldx or case.get("ldx", C)
        buf, start = strided_input(case["x"], ldx, xoff)
        xv = np.lib.stride_tricks.as_strided(buf[start:], (T, C), (4 * ldx, 4))
        o32, o16 = emulate(xv, case["alpha"], case["beta"], case["fup"], case["fdn"], case["logscale"], case["Creal"],
                           case["L"] if L is None else L, defect)
        return (o32 if outs != "out16" else None), (o16 if outs != "out32" else None)
    return run


def strided_input(x, ldx, xoff=0):
    """-> (flat float32 buffer, index of x[0][0]): rows of x at stride ldx between one row of NaN before and after, NaN in the
    stride gaps and in the xoff elements in front"""
    T, C = x.shape
    buf = np.full(xoff + (T + 2) * ldx, np.nan, F32)
    start = xoff + ldx
    np.lib.stride_tricks.as_strided(buf[start:], (T, C), (4 * ldx, 4))[...] = x
    return buf, start


# ------------------------------------------------------------------------------------------------------------------ cases
FUP_INT = (3, -7, 1, 12, -5, 9, -2, 8, -11, 4, -10, 6)
FDN_INT = (-4, 11, -1, 6, -9, 2, 12, -7, 3, -10, 5, -8)
for _f in (FUP_INT, FDN_INT):
    assert sorted(abs(v) for v in _f) == list(range(1, 13)) and _f != _f[::-1]
assert 2 * 3 * max(sum(abs(v) for v in FUP_INT[p::2]) for p in (0, 1)) * sum(abs(v) for v in FDN_INT) < 2 ** 24


def real_taps():
    from oracle import bigvgan_oracle as BO
    return BO.aa_filter_taps().numpy().astype(F32)


def _case(name, x, alpha, beta, fup, fdn, logscale, Creal, L=0, **kw):
    x = np.array(x, F32)
    C = x.shape[1]
    x[:, Creal:] = np.nan                                   # padding channels hold garbage: x, alpha and beta
    alpha = np.array(alpha, F32)
    same = beta is None                                     # Snake: alpha and beta are one tensor
    beta = alpha if same else np.array(beta, F32)
    for p in (alpha,) if same else (alpha, beta):
        assert p.shape == (C,)
        p[Creal:] = np.nan
    return dict(name=name, x=x, alpha=alpha, beta=beta, fup=np.array(fup, F32), fdn=np.array(fdn, F32), logscale=int(logscale),
                Creal=Creal, L=L, **kw)


def _exact_case(T, C, Creal, L=0, **kw):
    rng = np.random.default_rng(1000 * T + C)
    xi = rng.integers(-3, 4, size=(T, C))
    xi[0, 0] = 3
    c = _case(f"exact T={T} C={C} Creal={Creal} L={L} {kw or ''}", xi, np.zeros(C), np.ones(C), FUP_INT, FDN_INT, 0, Creal, L, **kw)
    xi[:, Creal:] = 0
    c["x_int"] = xi
    return c


def exact_cases(T):
    """family 1 over the L grid for one T, at C = 34 with 33 real channels"""
    return [_exact_case(T, C_MAIN, CREAL_MAIN, L) for L in L_LIST]


EXACT_SHAPE_T = (1, 5, 33)


def exact_shape_cases(T):
    """family 1 over C x Creal x strides for one T"""
    return [_exact_case(T, C, Creal, 0, ldx=C + px, ldo=C + po)
            for C in C_LIST for Creal in sorted({C, C - 1, 1}, reverse=True) for px, po in ((0, 0), (2, 6))]


def _spread(C, lo, hi, swap=False, geometric=False):
    """C different values of [lo, hi]; the two channels of a pair half the range apart"""
    base = np.geomspace(lo, hi, C) if geometric else np.linspace(lo, hi, C)
    v = np.empty(C)
    v[0 + swap::2], v[1 - swap::2] = base[:C // 2], base[C // 2:]
    return v


def _filters(phase, j0):
    fup, fdn = np.zeros(12), np.zeros(12)
    fup[5 + phase], fdn[j0] = 0.5, 1.0
    return fup, fdn


ONE_TAP_SETTINGS = ("logscale", "snake", "beta0", "arg1e-3", "arg1", "arg1e4")


def _one_tap_case(setting, phase, j0, T, L, C=C_MAIN, Creal=CREAL_MAIN):
    rng = np.random.default_rng(7 * T + 13 * j0 + phase)
    x = rng.standard_normal((T, C))
    if setting == "logscale":
        ls, alpha, beta = 1, _spread(C, -1.5, 1.5), _spread(C, -1.2, 1.0, swap=True)
        x *= 1.5
    elif setting == "snake":
        ls, alpha, beta = 1, _spread(C, -1.5, 1.5), None
        x *= 1.5
    elif setting == "beta0":                                # 1 / (0 + 1e-9): the only place the constant shows
        ls, alpha, beta = 0, _spread(C, 0.3, 3.0, geometric=True), np.zeros(C)
    elif setting == "arg1e-3":
        ls, alpha, beta = 0, _spread(C, 0.5e-3, 2e-3, geometric=True), _spread(C, 0.2, 5.0, swap=True, geometric=True)
    elif setting == "arg1":
        ls, alpha, beta = 0, _spread(C, 0.3, 3.0, geometric=True), _spread(C, 0.2, 5.0, swap=True, geometric=True)
    else:                                                   # |x a| up to 1e4: sinf needs its full-range argument reduction
        assert setting == "arg1e4"
        ls, alpha, beta = 0, _spread(C, 100.0, 1000.0, geometric=True), _spread(C, 0.2, 5.0, swap=True, geometric=True)
        x = rng.uniform(-10.0, 10.0, size=(T, C))
        x[-1, 0], x[0, 0] = -10.0, 10.0
    fup, fdn = _filters(phase, j0)
    return _case(f"one tap {setting} phase={phase} j0={j0} T={T} L={L}", x, alpha, beta, fup, fdn, ls, Creal, L)


def one_tap_cases(setting):
    """family 2 for one parameter setting: both phases x j0 = 0..11, T and L walking through their lists (16 and 7 are coprime: the
    six settings together meet every T with every L); "logscale" also runs T = 1, 2, 3 (both pads inside one window) with every
    filter pair"""
    s = ONE_TAP_SETTINGS.index(setting)
    cases = []
    for phase in (0, 1):
        for j0 in range(12):
            k = (s * 2 + phase) * 12 + j0
            cases.append(_one_tap_case(setting, phase, j0, T_LIST[k % len(T_LIST)], L_LIST[k % len(L_LIST)]))
            if setting == "logscale":
                cases += [_one_tap_case(setting, phase, j0, T, 0) for T in (1, 2, 3)]
    return cases


def _real_case(T, C, Creal, seed):
    rng = np.random.default_rng(seed)
    taps = real_taps()
    return _case(f"real taps T={T} C={C} Creal={Creal}", 1.5 * rng.standard_normal((T, C)), 0.4 * rng.standard_normal(C),
                 0.4 * rng.standard_normal(C), taps, taps, 1, Creal)


def chunking_case(T):
    return _real_case(T, C_MAIN, CREAL_MAIN, 300 + T)


STRIDE_SHAPES = ((5, 2), (5, 34), (33, 2), (33, 34))


def stride_case(T, C):
    return _real_case(T, C, C - 1, 400 + T + C)


# ------------------------------------------------------------------------------------------------------------------ checks
def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def _same(got, ref, what):
    """equal bit for bit (arrays of one dtype)"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.ascontiguousarray(got).view(np.uint8) != np.ascontiguousarray(ref).view(np.uint8)
    if bad.any():
        bad = bad.reshape(got.shape + (-1,)).any(-1)
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: {got[i]!r} != {ref[i]!r}")


def _rne(o32, o16, what):
    assert np.isfinite(o32).all(), f"{what}: out32 is not finite"
    _same(o16, bf16_bits(o32), f"{what}: out16 vs the bf16 rounding of out32")


def check_exact(case, run):
    """family 1: out32 == the int64 reference, out16 == its bf16 rounding (values: no NaN, padding channels 0)"""
    ref = ref_linear(case["x_int"], np.array(FUP_INT), np.array(FDN_INT))
    assert ref.dtype == np.int64 and np.abs(ref).max() < 2 ** 24 and not ref[:, case["Creal"]:].any()
    o32, o16 = run(case)
    for got, want, name in ((o32, ref.astype(F32), "out32"), (bf16_value(o16), bf16_value(bf16_bits(ref.astype(F32))), "out16")):
        bad = ~(got == want)
        if bad.any():
            i = _first(bad)
            raise AssertionError(f"{case['name']} {name}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: {got[i]!r} != {want[i]!r}")


def check_one_tap(case, run):
    """family 2: |out32 - ref_snake| <= tol element by element, out16 = bf16(out32); -> the worst ratio"""
    args = [case[k] for k in ("x", "alpha", "beta", "fup", "fdn", "logscale", "Creal")]
    ref, bound = ref_snake(*args), tol(*args)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()
    o32, o16 = run(case)
    _rne(o32, o16, case["name"])
    err = np.abs(o32.astype(F64) - ref)
    with np.errstate(over="ignore"):
        ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    if worst > 1.0:
        i = _first(ratio == ratio.max())
        raise AssertionError(f"{case['name']}: {int((ratio > 1).sum())} elements outside the bound, worst ratio {worst:.3g} at {i}: "
                             f"got {o32[i]!r}, ref {ref[i]!r}, bound {bound[i]:.3g}")
    return worst


CHUNK_ALONE_L = (0, 3)


def check_chunking(case, run):
    """family 3: every L and every choice of outputs gives the bits of L = 0 with both outputs; out16 = bf16(out32)"""
    b32, b16 = run(case, L=0)
    _rne(b32, b16, case["name"])
    for L in L_LIST[1:]:
        o32, o16 = run(case, L=L)
        _same(o32, b32, f"{case['name']}: out32 at L={L} vs L=0")
        _same(o16, b16, f"{case['name']}: out16 at L={L} vs L=0")
    for L in CHUNK_ALONE_L:
        o32, none = run(case, L=L, outs="out32")
        assert none is None
        _same(o32, b32, f"{case['name']}: out32 alone at L={L}")
        none, o16 = run(case, L=L, outs="out16")
        assert none is None
        _same(o16, b16, f"{case['name']}: out16 alone at L={L}")


def check_strides(case, run):
    """family 4: ldx, ldo in C + {0, 2, 6} and x two floats into its buffer give the bits of the dense call"""
    C = case["x"].shape[1]
    b32, b16 = run(case)
    _rne(b32, b16, case["name"])
    for px in LD_PADS:
        for po in LD_PADS:
            for xoff in (0, 2):
                if px == po == xoff == 0:
                    continue
                o32, o16 = run(case, ldx=C + px, ldo=C + po, xoff=xoff)
                what = f"{case['name']} ldx=C+{px} ldo=C+{po} xoff={xoff}"
                _same(o32, b32, what + " out32")
                _same(o16, b16, what + " out16")


def families():
    """name -> (check, cases): everything the GPU test runs, for the CPU test's sweep of the emulation"""
    return {
        "1 exact": (check_exact, [c for T in T_LIST for c in exact_cases(T)] + [c for T in EXACT_SHAPE_T for c in exact_shape_cases(T)]),
        "2 one tap": (check_one_tap, [c for s in ONE_TAP_SETTINGS for c in one_tap_cases(s)]),
        "3 chunking": (check_chunking, [chunking_case(T) for T in T_LIST]),
        "4 strides": (check_strides, [stride_case(T, C) for T, C in STRIDE_SHAPES]),
    }
