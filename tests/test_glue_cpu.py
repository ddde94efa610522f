"""CPU: the references of tests/_glue_reference.py are right (against the project's oracles and torch ops), the recorded float32-error
constants still cover their inputs, and the host side of the glue entry points refuses what its kernels cannot handle."""
import ctypes as C_
import math

import torch
import torch.nn.functional as Fn

from tests import _glue_reference as R

BF, F32, F64 = R.BF, R.F32, R.F64


# ------------------------------------------------------------------------------------------------------------------ references
def test_norm_references_are_layer_norm_and_the_oracle_rms():
    from oracle import mistral_oracle as MO
    x, res, r2, g, b = R.norm_inputs(5, 260, 1, BF, F32, n_res2=4)
    s = R.norm_sum32(x, res, r2)
    assert s.dtype == F32 and torch.equal(s, ((((x.float() + res) + r2[0]) + r2[1]) + r2[2]) + r2[3])
    assert torch.equal(R.norm_ref(s, g, b), Fn.layer_norm(s.double(), (260,), g.double(), b.double(), 1e-5))
    mean, var = s.double().mean(-1, keepdim=True), s.double().var(-1, unbiased=False, keepdim=True)
    assert torch.allclose(R.norm_ref(s, g, b), (s.double() - mean) / torch.sqrt(var + 1e-5) * g.double() + b.double(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.norm_ref(s, g, rms=True), MO.rms_norm(s, g, 1e-5).double(), rtol=0, atol=2e-6)       # (the oracle works in float32)
    sd = s.double()
    assert torch.allclose(R.norm_ref(s, g, rms=True), sd / torch.sqrt((sd * sd).mean(-1, keepdim=True) + 1e-5) * g.double(), rtol=1e-12, atol=1e-12)
    # the HF residual form: the oracle's bf16 RMSNorm of the bf16 sum is the fp64 value under two bf16 roundings
    xb, rb = x, res.to(BF)
    s16 = xb + rb
    assert torch.equal(s16, R.norm_sum32(xb, rb, round_bf16=True).to(BF))
    ref = R.norm_rms_hf_ref(s16, g.to(BF))
    hf = MO.rms_norm(s16, g.to(BF), 1e-5)
    assert hf.dtype == BF and bool(((hf.double() - ref).abs() <= 2.0 ** -7 * ref.abs()).all())
    assert R.norm_row_mask(9, [5, 0, 3], 3).tolist() == [False] * 3 + [True] * 3 + [False] * 3
    assert R.norm_row_mask(6, [1, 2], 3).tolist() == [False, True, True, False, False, True]


def test_recorded_float32_errors_still_cover_their_inputs():
    """every *_TORCH_FP32_ERR constant, recomputed: torch's own float32 evaluation against fp64 on the inputs of the GPU tests.  The
    LayerNorm outputs of usdm_norm keep the 2e-6 x max |ref| of test_layernorm_and_rms: torch float32 stays inside it at the new widths."""
    for name, fn, const in (("layer_norm at the new widths", R.norm_ln_torch_err, R.NORM_LN_TOL),
                            ("rms", R.norm_rms_torch_err, R.NORM_RMS_TORCH_FP32_ERR),
                            ("layer_norm + gelu", R.norm_gelu_torch_err, R.NORM_GELU_TORCH_FP32_ERR),
                            ("wave layer_norm", R.wave_layernorm_torch_err, R.WAVE_LN_TORCH_FP32_ERR),
                            ("conv0", R.conv0_torch_err, R.CONV0_TORCH_FP32_ERR),
                            ("softmax", R.softmax_seg_torch_err, R.SOFTMAX_SEG_TORCH_FP32_ERR),
                            ("time token", R.time_token_torch_err, R.TIME_TOKEN_TORCH_FP32_ERR)):
        err = fn()
        print(f"[glue] torch float32 vs fp64, {name}: {err:.3g} (recorded {const:.3g})")
        assert 0 < err <= const, f"{name}: the recorded figure {const:g} no longer describes the inputs ({err:g})"
        assert name.startswith("layer_norm at") or const <= 1.25 * err, f"{name}: the recorded figure {const:g} is far above what is measured ({err:g})"


def test_bounds_of_the_format_roundings():
    x = R.randn((4096,), 3, 5.0)
    err = (x.to(BF).double() - x.double()).abs()
    assert bool((err <= R.bf16_of_f32_bound(x.double(), 0.0)).all()) and float((err / x.double().abs()).max()) > 2.0 ** -8.5
    a, b = R.randn((4096,), 4), R.randn((4096,), 5)
    got = a * torch.tensor(2.5) + b                     # two float32 roundings
    assert bool(((got.double() - (a.double() * 2.5 + b.double())).abs() <= R.few_ops_bound(2, a * 2.5, b)).all())
    s = R.sentinel((3,), BF)
    assert R.bits(s).tolist() == [0x7f7f] * 3 and bool(torch.isfinite(s).all()) and bool(R.is_sentinel(s).all())
    assert bool(R.is_sentinel(R.sentinel((2,), torch.int64)).all()) and not bool(R.is_sentinel(torch.zeros(2)).any())


def test_wave_and_conv0_references_are_the_torch_ops():
    x = R.wave(1000, 1)
    ref = R.wave_layernorm_ref(x)
    xd = x.double()
    assert torch.allclose(ref, (xd - xd.mean()) / torch.sqrt(xd.var(unbiased=False) + 1e-5), rtol=1e-12, atol=1e-12)
    assert abs(float(x.mean()) - 0.3) < 0.05, "the DC offset"
    assert not bool(R.wave_layernorm_ref(R.wave(1, 8)).any()), "one sample normalises to 0"
    w, b, g, be = R.conv0_params()
    for stride, T, n in ((5, 7, 6 * 5 + 10), (8, 3, 2 * 8 + 10 + 1000), (1, 1, 10)):
        x = R.conv0_wave(n)
        ref = R.conv0_ref(x, T, stride, w, b, g, be)
        assert ref.shape == (T, 512)
        # by hand: frame t is the dot product of the taps with x[t * stride : t * stride + 10]
        y = torch.stack([(w.double() * x.double()[t * stride:t * stride + 10]).sum(1) + b.double() for t in range(T)])
        assert torch.allclose(ref, Fn.gelu(Fn.layer_norm(y, (512,), g.double(), be.double(), 1e-5)), rtol=1e-10, atol=1e-12)
    cases = list(R.conv0_cases())
    assert len(cases) == 40 and all(n - (T - 1) * s - 10 in (0, 1000) for s, T, n in cases)


def test_softmax_reference_and_inputs():
    for n in R.SOFTMAX_SEG_N:
        x = R.softmax_seg_inputs(n)
        ref = R.softmax_seg_ref(x)
        e = torch.exp(x.double() - x.double().amax(-1, keepdim=True))
        assert torch.allclose(ref, e / e.sum(-1, keepdim=True), rtol=1e-12, atol=0)
        assert float(ref.min()) >= 2.0 ** -100 and (n < 21 or float(ref.min()) < 1e-15), "a far tail above the two-sided floor"


def test_kmeans_reference_is_the_oracle_and_the_cases_hold_their_plants():
    from oracle import w2v_oracle as WO
    g = R.gen(5)
    x = torch.randint(-3, 4, (6, 40), generator=g).double()
    cen = torch.randint(-3, 4, (300, 40), generator=g).double()
    cen[17] = cen[4]                                    # an exact tie wherever unit 4 wins
    o_ids, o_dist = WO.kmeans_assign(x, cen)
    ids, margin, dist = R.kmeans_ref(x.float(), (x @ cen.T).float(), cen.pow(2).sum(1).float())
    assert torch.equal(ids, o_ids) and torch.equal(dist, o_dist)
    assert torch.equal(margin.double(), torch.sort(o_dist, 1).values[:, 1] - o_dist.min(1).values)
    for D in (3, 1280):
        for n_units in (1, 255, 256, 257, 10000):
            x, dots, csq = R.kmeans_case(D, n_units)
            assert x.dtype == dots.dtype == csq.dtype == F32 and dots.shape == (6, n_units + 3)
            ids, margin, dist = R.kmeans_ref(x, dots, csq)
            d32 = (x.pow(2).sum(1, keepdim=True) - 2.0 * dots[:, :n_units]) + csq       # the kernel's float32 operations: all exact
            assert torch.equal(d32.double(), dist)
            if n_units == 1:
                assert ids.tolist() == [0] * 6 and bool(torch.isinf(margin).all())
            elif n_units == 10000:
                assert ids.tolist() == [0, 9999, 5, 10, 70, 70] and margin.tolist()[2:] == [0.0] * 4 and min(margin.tolist()[:2]) > 50
                assert (dist[5] == dist[5].min()).nonzero().view(-1).tolist() == [70, 200, 300]
            else:
                assert ids.tolist()[3:] == [10, 70, 70] and ids.tolist()[:2] == [0, n_units - 1]
            assert bool((dots[:, n_units:] == 1.0e6).all()), "pad columns that would win if read"


def test_time_token_reference_is_the_oracle():
    from oracle import voicebox_oracle as VO
    for H in (16, 1024):
        for tv in R.TIME_TOKEN_T:
            t = torch.tensor(tv)
            freqs = R.time_token_freqs(H)
            o = VO.time_embedding(t, H)
            assert torch.equal(R.time_token_ref(t, freqs, F32), o), "the float32 evaluation of the reference is the oracle, operation by operation"
            assert float((R.time_token_ref(t, freqs) - o.double()).abs().max()) <= R.TIME_TOKEN_TORCH_FP32_ERR


def test_solver_reference_is_the_oracle_generate():
    """one Euler step, and one Heun step (predictor, corrector) followed by the closing Euler step, of oracle generate() with a stub
    estimator, with CFG and prompt re-noising: chained solver_ref calls give the same z"""
    from oracle import voicebox_oracle as VO
    cfg = dict(sigma_min=0.25, n_tokens=9)
    B, F, S, P, gs = 2, 5, 67, 13, 0.75
    x = torch.zeros(B, S, dtype=torch.int64)
    cond = R.randn((B, F, S), 1).double()
    noise = [R.randn((B, F, S), 10 + i).double() for i in range(4)]
    lengths = torch.full((B,), S)

    def f(xx, z, c, t, ln):          # the halves differ through cond (zero for the unconditional one) and the null token
        return 0.3 * z + 0.2 * c + t + 0.01 * xx.double().view(-1, 1, S)

    def vel(z, t):                   # [vu ; vc] flat, as the estimator leaves it for the kernel
        tt = torch.full((2 * B, 1, 1), t, dtype=F64)
        return f(torch.cat([cfg["n_tokens"] * torch.ones_like(x), x], 0), torch.cat([z, z], 0), torch.cat([torch.zeros_like(cond), cond], 0), tt, None).reshape(-1)

    def step(z, vout, t_next, **kw):
        zn, v, _, _ = R.solver_ref(vout, z.reshape(-1), S=S, cfg=True, gs=gs, eps=kw.pop("eps").reshape(-1), cond=cond.reshape(-1), P=P,
                                   c_eps=1 - (1 - cfg["sigma_min"]) * t_next, c_cond=t_next, **kw)
        return zn.view(B, F, S), v

    ref = VO.generate(None, cfg, x, cond, lengths, 1, noise, "euler", gs, True, [P], f=f)
    z1, _ = step(noise[0], vel(noise[0], 0.0), 1.0, mode=0, dt=1.0, eps=noise[1])
    assert torch.allclose(z1, ref, rtol=1e-13, atol=1e-13)
    ref = VO.generate(None, cfg, x, cond, lengths, 3, noise, "heun", gs, True, [P], f=f)
    z_in, v1 = step(noise[0], vel(noise[0], 0.0), 0.5, mode=0, dt=0.5, eps=noise[1])
    z1, _ = step(noise[0], vel(z_in, 0.5), 0.5, mode=1, dt=0.5, v1=v1, eps=noise[2])
    z2, _ = step(z1, vel(z1, 0.5), 1.0, mode=0, dt=0.5, eps=noise[3])
    assert torch.allclose(z2, ref, rtol=1e-13, atol=1e-13)
    # the bound is what float32 needs: the same step in float32 arithmetic stays inside it
    c = R.solver_case(11)
    n = c["n"]
    zn, v, bound, vbound = R.solver_ref(c["vout"], c["z"], S=c["S"], mode=0, dt=0.125, cfg=True, gs=0.7)
    gsf, dtf = torch.tensor(0.7), torch.tensor(0.125)
    v32 = c["vout"][n:] + gsf * (c["vout"][n:] - c["vout"][:n])
    assert bool(((v32.double() - v).abs() <= vbound).all()) and bool((((c["z"] + dtf * v32).double() - zn).abs() <= bound).all())
    assert float(((c["z"] + dtf * v32).double() - zn).abs().max()) > 0 and float(bound.max()) < 1e-5


def test_mask_build_input_and_bigvgan_references():
    x = R.randn((3, 4, 5), 1)
    m = R.mask_time_ref(x, [4, 3, 0], 1, 0)
    assert torch.equal(m[0, :3], x[0, :3]) and not bool(m[0, 3:].any()) and torch.equal(m[1, :2], x[1, :2]) and not bool(m[1, 2:].any()) and not bool(m[2].any())
    m = R.mask_time_ref(x, [5, 3, 0], 0, 1)
    assert torch.equal(m[0], x[0]) and torch.equal(m[1, :, :3], x[1, :, :3]) and not bool(m[1, :, 3:].any()) and not bool(m[2].any())
    ids, y, cond, table = R.vb_input_case(8, BF)
    assert 0 in ids.tolist()[0] and table.shape[0] - 1 in ids.tolist()[0]
    out = R.vb_build_input_ref(ids, y, cond, table, dup=2, use_cond=True, null_id=10, ldo=32)
    assert out.shape == (4, 9, 32) and out.dtype == BF
    ref = torch.cat([table[ids], y.transpose(1, 2).to(BF), cond.transpose(1, 2).to(BF), torch.zeros(2, 9, 14, dtype=BF)], -1)      # (networks.py:305-307)
    assert torch.equal(out[2:], ref)
    assert torch.equal(out[:2, :, :8], table[10].expand(2, 9, 8)) and torch.equal(out[:2, :, 8:13], out[2:, :, 8:13]) and not bool(out[:2, :, 13:].any())
    assert not bool(R.vb_build_input_ref(ids, y, cond, table, dup=1, use_cond=False, null_id=10, ldo=32)[:, :, 13:].any())
    a, b, c = R.randn((8,), 1), R.randn((8,), 2), R.randn((8,), 3)
    assert torch.allclose(R.sum3_scale_ref(a, b, c, 1 / 3).double(), (a.double() + b.double() + c.double()) / 3, rtol=1e-6)
    x = R.randn((2, 3, 4), 6)
    ref, bound = R.cf_to_cl_ref(x, 8, 2.5, -1.25)
    assert torch.equal(ref[..., :3], x.double().permute(0, 2, 1) * 2.5 - 1.25) and not bool(ref[..., 3:].any()) and not bool(bound[..., 3:].any())
    assert bool((((x * 2.5 - 1.25).double().permute(0, 2, 1) - ref[..., :3]).abs() <= bound[..., :3]).all())


def test_stft_and_framing_references_are_the_mel_oracle():
    from oracle import mel_oracle as MO
    # stft_frames: frames x window, transformed, are torch.stft of the clamped signal as the oracle calls it (hann window, center=False
    # on the reflect-padded signal)
    n, n_fft, hop = 1500, 1024, 256
    pad = (n_fft - hop) // 2
    x = R.randn((n,), 1, 0.8)
    T = R.stft_T(n, n_fft, hop, pad)
    win = torch.hann_window(n_fft)
    fr = R.stft_frames_ref(x, n_fft, hop, pad, win)
    assert fr.shape == (T, n_fft) and T == 5 and fr.dtype == F32
    y = Fn.pad(x.clamp(-1, 1)[None, None], (pad, pad), mode="reflect")[0]
    spec = torch.stft(y.double(), n_fft, hop_length=hop, win_length=n_fft, window=win.double(), center=False, return_complex=True)[0].T
    assert torch.allclose(torch.fft.rfft(fr.double(), dim=-1), spec, rtol=0, atol=1e-4)
    mag, bound = R.stft_mag_ref(torch.cat([spec.real, spec.imag], -1).float(), 513, 1e-9, 520)
    assert torch.allclose(mag[:, :513], torch.sqrt(torch.real(spec * spec.conj()) + 1e-9), rtol=1e-5) and not bool(mag[:, 513:].any())
    ri = torch.cat([spec.real, spec.imag], -1).float()
    m32 = torch.sqrt((ri[:, :513] * ri[:, :513] + ri[:, 513:] * ri[:, 513:]) + torch.tensor(1e-9))
    assert bool(((m32.double() - mag[:, :513]).abs() <= bound[:, :513]).all()), "float32 arithmetic stays inside the k = 4 bound"
    # the tiny case by hand: n = 7, pad = 6 reflects both ends inside the one frame
    x7 = torch.tensor([0.1, 1.7, -0.3, 0.4, -2.0, 0.6, 0.7])
    w16 = R.stft_window(16)
    assert not torch.equal(w16, w16.flip(0))
    idx = [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 5, 4, 3]
    assert R.stft_T(7, 16, 4, 6) == 1 and torch.equal(R.stft_frames_ref(x7, 16, 4, 6, w16)[0], x7.clamp(-1, 1)[idx] * w16)
    # frame_signal: the im2col of the oracle's polyphase resampler (pad (width, width + orig), stride orig)
    k, width, orig, new = MO.resample_kernel(16000, 22050)
    sig = R.randn((700,), 2)
    flen = k.shape[1]
    Tn = (700 + 2 * width + orig - flen) // orig + 1
    frames = R.frame_signal_ref(sig, flen, orig, width, Tn)
    got = (frames.double() @ k.double().T).reshape(-1)[:math.ceil(new * 700 / orig)]
    assert torch.allclose(got, MO.resample(sig, 16000, 22050).double(), rtol=0, atol=1e-5)
    f = R.frame_signal_ref(torch.arange(1.0, 6.0), 4, 2, 1, 3)
    assert f.tolist() == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 0, 0]]


def test_residual_add_and_rope_references():
    from oracle import mistral_oracle as MO
    h, d = R.residual_add_case(4099)
    ref = R.residual_add_ref(h, d)
    assert ref[:6].tolist() == [1.5, -0.515625, 1.0, -1.0, 1.015625, 3.0]
    assert (h.float() + d).to(BF)[2:6].tolist() == [1.0078125, -1.0078125, 1.0078125, 3.015625], "each needs the inner rounding"
    qkv = R.rope_case()
    Hq, Hkv, S = R.ROPE["Hq"], R.ROPE["Hkv"], R.ROPE["S"]
    heads = qkv.view(S, Hq + 2 * Hkv, 128)
    cos, sin = R.rope_tables(128)
    for pos0 in (0, 91):
        got = R.rope_ref(heads[:, :Hq], pos0, cos, sin)
        assert got.dtype == BF
        # HF layout [B, H, S, d] with cos / sin [B, 1, S, d]
        q = heads[:, :Hq].transpose(0, 1)[None]
        c, s = MO.rope_tables(dict(head_dim=128, rope_theta=10000.0), torch.arange(pos0, pos0 + S), BF)
        hf = (q * c[None, None]) + (MO.rotate_half(q) * s[None, None])
        assert torch.equal(R.bits(got), R.bits(hf[0].transpose(0, 1)))
        # and the roundings spelled out: each product and the sum rounded to bf16
        x1, x2 = heads[:, :Hq, :64].float(), heads[:, :Hq, 64:].float()
        cf, sf = c[:, None, :64].float(), s[:, None, :64].float()
        r = lambda t: t.to(BF).float()
        assert torch.equal(got[..., :64].float(), r(r(x1 * cf) + r(-x2 * sf))) and torch.equal(got[..., 64:].float(), r(r(x2 * cf) + r(x1 * sf)))
        once = r(x1 * cf - x2 * sf)
        assert not torch.equal(once, got[..., :64].float()), "the inputs do not tell one rounding from three"
    assert torch.equal(R.rope_ref(heads[:1, :Hq], 0, cos, sin), heads[:1, :Hq]), "position 0 is the identity"


# ------------------------------------------------------------------------------------------------------------------ host refusals
PTR = 0x10000


def _refused(rc, word):
    from usdm_amd import _lib
    msg = _lib.lib.usdm_last_error()
    assert rc == 2 and word in msg, (rc, msg, word)


def _norm_args(**kw):
    from usdm_amd import _lib
    a = _lib.NormArgs()
    a.x, a.gamma, a.out32, a.rows, a.C, a.eps = PTR, PTR, PTR, 7, 1024, 1e-5
    a.x_dtype = a.res_dtype = _lib.F32
    a.ldx = a.ldr = a.ldo = a.lds = 1024
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_usdm_norm_refusals():
    from usdm_amd import _lib
    call = lambda **kw: _lib.lib.usdm_norm(C_.byref(_norm_args(**kw)), None)
    _refused(call(C=5124, ldx=5124, ldr=5124, ldo=5124, lds=5124), b"C=5124")
    _refused(call(C=6), b"C=6")
    for ld in ("ldx", "ldr", "ldo", "lds"):
        _refused(call(**{ld: 1026}), b"strides")
    _refused(call(res2=PTR, n_res2=9, res2_stride=7 * 1024), b"res2")
    _refused(call(res2=PTR, n_res2=2, res2_stride=7 * 1024, round_bf16=1, res=PTR), b"res2")
    _refused(call(res2=PTR, n_res2=2, res2_stride=7 * 1024 + 2), b"res2")


def test_w2v_refusals():
    from usdm_amd import _lib
    lib = _lib.lib
    p, i32, f = C_.c_void_p(PTR), C_.c_int32, C_.c_float

    def conv0(n=1000, T=10, C=512, k=10, stride=5):
        return lib.usdm_w2v_conv0(p, i32(n), i32(T), i32(C), i32(k), i32(stride), p, p, p, p, f(1e-5), p, None)
    _refused(conv0(stride=0), b"stride 0")
    _refused(conv0(stride=9), b"stride 9")
    _refused(conv0(C=256), b"C=256")
    _refused(conv0(k=3), b"k=3")
    _refused(conv0(n=9 * 5 + 9), b"do not fit in n")

    def kmeans(n_units=100, ldd=100):
        return lib.usdm_kmeans_argmin(p, i32(6), i32(8), p, C_.c_int64(ldd), p, i32(n_units), p, p, None)
    _refused(kmeans(ldd=99), b"ldd=99")
    _refused(kmeans(n_units=0, ldd=0), b"bad args")


def test_vb_refusals():
    from usdm_amd import _lib
    lib = _lib.lib
    s = _lib.VbSolverArgs()
    s.vout, s.z, s.z_in, s.B, s.F, s.S, s.mode = PTR, PTR, PTR, 2, 5, 67, 1
    _refused(lib.usdm_vb_solver_step(C_.byref(s), None), b"v1")
    s.mode, s.eps = 0, PTR
    _refused(lib.usdm_vb_solver_step(C_.byref(s), None), b"cond")

    def build(**kw):
        a = _lib.VbInputArgs()
        a.ids, a.y, a.cond, a.table, a.out = PTR, PTR, PTR, PTR, PTR
        a.B_in, a.dup, a.S, a.E, a.F, a.null_id, a.use_cond, a.ldo, a.out_dtype = 2, 1, 9, 8, 5, 10, 1, 32, _lib.BF16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.usdm_vb_build_input(C_.byref(a), None)
    _refused(build(F=-1), b"F=-1")
    _refused(build(null_id=-1), b"null_id=-1")
    _refused(build(F=13), b"bad sizes")


def test_bigvgan_refusals():
    from usdm_amd import _lib
    lib = _lib.lib
    p, i32 = C_.c_void_p(PTR), C_.c_int32
    _refused(lib.usdm_sum3_scale(p, p, p, C_.c_float(1 / 3), C_.c_int64(6), p, p, None), b"n=6")

    def frames(n=1500, n_fft=1024, hop=256, pad=384, T=5):
        return lib.usdm_stft_frames(p, i32(n), i32(n_fft), i32(hop), i32(pad), p, p, i32(T), None)
    _refused(frames(n=384), b"longer than the reflect pad")
    _refused(frames(n=6, n_fft=16, hop=4, pad=6, T=1), b"longer than the reflect pad")
    _refused(frames(T=6), b"T frames")
    _refused(frames(n=7, n_fft=16, hop=4, pad=6, T=2), b"T frames")
    _refused(frames(n_fft=0), b"n_fft=0")
    _refused(frames(n_fft=-8), b"n_fft=-8")
    _refused(frames(hop=0, T=1), b"hop=0")
    _refused(frames(hop=-256, T=2), b"hop=-256")


def test_llm_glue_refusals():
    from usdm_amd import _lib
    lib = _lib.lib
    p, i32 = C_.c_void_p(PTR), C_.c_int32
    _refused(lib.usdm_embed_rows(p, p, None, i32(5), i32(12), p, None), b"Hd=12")

    def rope(**kw):
        a = _lib.RopeArgs()
        a.qkv, a.cos, a.sin, a.kcache, a.vcache = PTR, PTR, PTR, PTR, PTR
        a.ld, a.S, a.pos0, a.Hq, a.Hkv, a.ctx_max, a.max_pos = 1152, 37, 91, 4, 2, 128, 128
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.usdm_rope_cache(C_.byref(a), None)
    _refused(rope(pos0=92), b"positions")
    _refused(rope(vt=PTR, vt_ld=36), b"vt_ld")
