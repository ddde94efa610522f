"""GPU: the small kernels between the GEMMs and the attention, each called directly through its usdm_amd.ops wrapper and compared
with the plain CPU reference of tests/_glue_reference.py (checked itself by tests/test_glue_cpu.py) at the edges where such kernels
go wrong: partial pieces, strides, tails of a grid, ties, pad columns.

Moves and fixed sequences of rounded operations are compared bit for bit; a few f32 operations against fp64 under
k * 2^-23 * sum|terms|; reductions and transcendentals against fp64 under 4 x torch's own float32 error on the same inputs (the
*_TORCH_FP32_ERR constants of _glue_reference.py, recomputed by the CPU test).  No test leaves an element out.
Every output buffer is larger than what the kernel may write and pre-filled with a sentinel (7.0, bf16 bits 0x7f7f) that must
survive bit for bit.

Entry point -> test
  usdm_norm              test_norm_*                      usdm_mask_time       test_mask_time
  usdm_wave_layernorm    test_wave_layernorm              usdm_sum3_scale      test_sum3_scale
  usdm_w2v_conv0         test_w2v_conv0                   usdm_cf_to_cl        test_cf_to_cl
  usdm_softmax_segments  test_softmax_segments            usdm_stft_frames     test_stft_frames
  usdm_kmeans_argmin     test_kmeans_argmin               usdm_stft_mag        test_stft_mag
  usdm_vb_build_input    test_vb_build_input              usdm_frame_signal    test_frame_signal
  usdm_vb_time_token     test_vb_time_token               usdm_embed_rows      test_embed_rows
  usdm_vb_solver_step    test_vb_solver_*                 usdm_residual_add    test_residual_add
                                                          usdm_rope_cache      test_rope_cache
"""
import math

import pytest
import torch

from tests import _attn_probe as P
from tests import _glue_reference as R

pytestmark = pytest.mark.gpu
BF, F32 = R.BF, R.F32
GELU = 1      # USDM_ACT_GELU


# ------------------------------------------------------------------------------------------------------------------ helpers
class Out:
    """an output buffer of [rows + 1, ld] (or flat [n + 16]) elements pre-filled with the sentinel; take() returns the part the
    kernel owns after asserting that everything else - stride gaps, the row past the end - still holds the sentinel bits"""

    def __init__(self, dev, rows, ld, dtype=F32):
        self.t = R.sentinel((rows + 1, ld), dtype, dev)

    def take(self, rows, cols, what):
        torch.cuda.synchronize()
        got = self.t.cpu()
        outside = torch.ones(got.shape, dtype=torch.bool)
        outside[:rows, :cols] = False
        bad = outside & ~R.is_sentinel(got)
        assert not bool(bad.any()), f"{what}: written outside [{rows}, {cols}] at {bad.nonzero()[:4].tolist()}"
        return got[:rows, :cols].contiguous()


def _flat_out(dev, n, dtype=F32):
    return Out(dev, 1, n + 16, dtype)


def _strided(t, ld, dev):
    """rows of t at stride ld, the gaps (and one more row) holding the sentinel"""
    buf = R.sentinel((t.shape[0] + 1, ld), t.dtype)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.to(dev)


def _same_bits(got, ref, what):
    gb, rb = R.bits(got), R.bits(ref)
    if not torch.equal(gb, rb):
        bad = (gb != rb).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {gb.numel()} elements differ, first at {i}: got {got[i].item()!r}, expected {ref[i].item()!r}")


def _within(got, ref, bound, what):
    """|got - ref| <= bound element by element (fp64); prints the worst ratio before asserting"""
    err = (got.double().cpu() - ref.double()).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[glue] {what}: worst |got - ref| / bound = {worst:.3f}")
    if worst > 1.0:
        i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements outside the bound, worst at {i}: got {got[i].item()!r}, "
                             f"ref {ref[i].item()!r}, bound {bound[i].item():.3g}")


def _rel_to_max(got, ref, tol, what):
    """max |got - ref| <= tol * max |ref|; prints the figure before asserting"""
    e = R.rel_to_max(got.cpu(), ref)
    print(f"[glue] {what}: max |got - ref| / max |ref| = {e:.3g} (bound {tol:.3g})")
    assert e <= tol, f"{what}: {e:.3g} > {tol:.3g}"


# ------------------------------------------------------------------------------------------------------------------ usdm_norm
def _norm(dev, x, gamma, beta, *, C, rows, res=None, r2=None, ld=None, want=("out32",), res2_pad=4, **kw):
    """one usdm_norm launch -> {name: [rows, C] on the CPU} for the outputs in `want`.  ld = (ldx, ldr, ldo, lds) or None (all C);
    r2 [n, rows, C]: the addends, laid out res2_stride = rows * ldr + res2_pad apart."""
    from usdm_amd import ops
    ldx, ldr, ldo, lds = ld or (C, C, C, C)
    outs = {n: Out(dev, rows, ldo if n.startswith("out") else lds, F32 if n.endswith("32") else BF) for n in want}
    args = dict(kw)
    if r2 is not None:
        stride = rows * ldr + res2_pad
        flat = R.sentinel((r2.shape[0] * stride,), F32)
        for e in range(r2.shape[0]):
            flat[e * stride:e * stride + rows * ldr].view(rows, ldr)[:, :C] = r2[e]
        args.update(res2=flat.to(dev), n_res2=r2.shape[0], res2_stride=stride)
    ops.norm(_strided(x, ldx, dev), gamma.to(dev), None if beta is None else beta.to(dev), rows=rows, C=C,
             res=None if res is None else _strided(res, ldr, dev), ldx=ldx, ldr=ldr, ldo=ldo, lds=lds,
             **{n: o.t for n, o in outs.items()}, **args)
    return {n: o.take(rows, C, f"usdm_norm {n}") for n, o in outs.items()}


def _check_ln(got, s, g, b, what, **ref_kw):
    """out32 under 2e-6 * max |ref| (the bound of test_layernorm_and_rms); out16 = bf16 of an f32 value under that bound"""
    ref = R.norm_ref(s, g, b, **ref_kw)
    tol = R.NORM_LN_TOL * float(ref.abs().max())
    if "out32" in got:
        _within(got["out32"], ref, tol, f"{what} out32")
    if "out16" in got:
        _within(got["out16"], ref, R.bf16_of_f32_bound(ref, tol), f"{what} out16")


@pytest.mark.parametrize("C", R.NORM_WIDTHS)
def test_norm_widths(dev, C):
    """usdm_norm, LayerNorm of f32 x + f32 res at every instantiation the launcher selects: <2> with one partial piece (C = 4), fewer
    pieces than lanes (64), a partial second piece (260); <5> with idle pieces (768) and a partial fifth (1028); <MAXP> at 4100
    (cdiv 17), 4352 and 5120 (<4> and <16> run in test_norm_addends).  rows = 7: a workgroup of 4 and a tail of 3."""
    rows = R.NORM_ROWS
    x, res, _, g, b = R.norm_inputs(rows, C, 100 + C)
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, want=("out32", "out16", "sum32"))
    s = R.norm_sum32(x, res)
    _same_bits(got["sum32"], s, f"C={C} sum32")
    _check_ln(got, s, g, b, f"LayerNorm C={C}")


@pytest.mark.parametrize("C", [1028, 4100], ids=["narrow", "wide"])
@pytest.mark.parametrize("xdt,rdt", [(BF, F32), (F32, BF), (BF, BF)], ids=["x16_r32", "x32_r16", "x16_r16"])
def test_norm_source_types(dev, C, xdt, rdt):
    """usdm_norm with bf16 x and / or bf16 res in the narrow (NP <= 5) and the wide path: sum32 is the f32 sum of the converted
    values, exactly"""
    rows = R.NORM_ROWS
    x, res, _, g, b = R.norm_inputs(rows, C, 500 + C, xdt, rdt)
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, want=("out32", "sum32"))
    s = R.norm_sum32(x, res)
    _same_bits(got["sum32"], s, f"C={C} sum32")
    _check_ln(got, s, g, b, f"LayerNorm C={C} {xdt} {rdt}")


@pytest.mark.parametrize("C", [260, 4100])
def test_norm_strides(dev, C):
    """usdm_norm with ldx, ldr, ldo, lds = C + 8, C + 12, C + 4, C + 16: the gaps of the four outputs keep their sentinel"""
    rows = R.NORM_ROWS
    x, res, _, g, b = R.norm_inputs(rows, C, 600 + C)
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, ld=(C + 8, C + 12, C + 4, C + 16), want=("out32", "out16", "sum32", "sum16"))
    s = R.norm_sum32(x, res)
    _same_bits(got["sum32"], s, "sum32")
    _same_bits(got["sum16"], s.to(BF), "sum16")
    _check_ln(got, s, g, b, f"strided LayerNorm C={C}")


@pytest.mark.parametrize("C", [1024, 4096])
@pytest.mark.parametrize("n_res2", [1, 3, 4, 8])
def test_norm_addends(dev, C, n_res2):
    """usdm_norm with n_res2 further f32 addends, res2_stride = rows * C + 4: sum32 == (((x + res) + r2[0]) + r2[1]) ... in float32, in
    that order - the three preloaded addends of the narrow path (<4>), its tail loop after them (n_res2 = 4, 8) and the wide path's
    loop (<16>)"""
    rows = R.NORM_ROWS
    x, res, r2, g, b = R.norm_inputs(rows, C, 700 + C + n_res2, n_res2=n_res2)
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, r2=r2, want=("out32", "sum32"))
    s = R.norm_sum32(x, res, r2)
    _same_bits(got["sum32"], s, f"C={C} n_res2={n_res2} sum32")
    _check_ln(got, s, g, b, f"LayerNorm of {n_res2} addends C={C}")


@pytest.mark.parametrize("C", [1028, 4100])
@pytest.mark.parametrize("both", [False, True], ids=["sum16_alone", "sum16_and_sum32"])
def test_norm_sum16(dev, C, both):
    """usdm_norm's sum16 == bf16(sum32) bit for bit, requested alone and together with sum32"""
    rows = R.NORM_ROWS
    x, res, _, g, b = R.norm_inputs(rows, C, 800 + C)
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, want=("out16", "sum16") + (("sum32",) if both else ()))
    s = R.norm_sum32(x, res)
    _same_bits(got["sum16"], s.to(BF), "sum16")
    if both:
        _same_bits(got["sum32"], s, "sum32")
    _check_ln(got, s, g, b, f"LayerNorm C={C}")


@pytest.mark.parametrize("C", [260, 4100])
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rms"])
@pytest.mark.parametrize("premask", [False, True], ids=["mask_outputs", "premask"])
def test_norm_premask(dev, C, rms, premask):
    """usdm_norm with valid_len = [5, 0, 3], rows_per_batch = 3 (rows = 9; batch 1 is all padding): the outputs are exactly 0 on rows
    >= valid_len; sum32 is exactly 0 there with premask and keeps the sum without"""
    rows, vl, rpb = 9, [5, 0, 3], 3
    x, res, _, g, b = R.norm_inputs(rows, C, 900 + C)
    if rms:
        b = None
    got = _norm(dev, x, g, b, C=C, rows=rows, res=res, want=("out32", "out16", "sum32"), rms=rms, premask=premask,
                valid_len=torch.tensor(vl, dtype=torch.int32, device=dev), rows_per_batch=rpb)
    dead = R.norm_row_mask(rows, vl, rpb)
    assert dead.tolist() == [False] * 3 + [True] * 3 + [False] * 3
    s = R.norm_sum32(x, res)
    s_exp = torch.where(dead[:, None] & premask, torch.zeros_like(s), s)
    _same_bits(got["sum32"], s_exp, "sum32")
    for n in ("out32", "out16"):
        assert not bool(R.bits(got[n][dead]).any()), f"{n} is not exactly +0 on the padding rows"
    live = {n: t[~dead] for n, t in got.items()}
    if rms:
        ref = R.norm_ref(s[~dead], g, rms=True)
        tol = 4 * R.NORM_RMS_TORCH_FP32_ERR * float(ref.abs().max())
        _within(live["out32"], ref, tol, "rms out32")
        _within(live["out16"], ref, R.bf16_of_f32_bound(ref, tol), "rms out16")
    else:
        _check_ln(live, s[~dead], g, b, f"masked LayerNorm C={C}")


@pytest.mark.parametrize("C", R.NORM_RMS_C)
def test_norm_rms_f32(dev, C):
    """usdm_norm, rms without round_bf16, f32 in and out, beta = None, against fp64.  Bound: 4 x NORM_RMS_TORCH_FP32_ERR x max |ref|
    (torch's float32 x * rsqrt(mean(x^2) + eps) * g loses 1.01e-7 x max |ref| on these inputs)."""
    x, g = R.norm_rms_case(C)
    got = _norm(dev, x, g, None, C=C, rows=R.NORM_ROWS, rms=True, want=("out32",))
    _rel_to_max(got["out32"], R.norm_ref(x, g, rms=True), 4 * R.NORM_RMS_TORCH_FP32_ERR, f"RMSNorm f32 C={C}")


@pytest.mark.parametrize("C", [1028, 4100], ids=["narrow", "wide"])
def test_norm_rms_hf_residual(dev, C):
    """usdm_norm, rms + round_bf16 + bf16 res (the HF residual form): sum16 == x_bf16 + res_bf16 as torch evaluates it in bfloat16;
    out16 within 2^-7 relative of the fp64 gamma_bf16 * normalised - the two bf16 roundings of HF's form (the normalised value, then its
    product with gamma; each 2^-8 of its value only just above a power of two, 2^-9 on average) with the float32 noise under them;
    a wrong mean, piece or gamma is O(1)"""
    rows = R.NORM_ROWS
    x, res, _, g, _ = R.norm_inputs(rows, C, 1000 + C, BF, BF)
    gb = g.to(BF)
    got = _norm(dev, x, gb.float(), None, C=C, rows=rows, res=res, rms=True, round_bf16=True, want=("out16", "sum16"))
    s16 = x + res
    assert s16.dtype == BF
    _same_bits(got["sum16"], s16, "sum16")
    ref = R.norm_rms_hf_ref(s16, gb)
    _within(got["out16"], ref, 2.0 ** -7 * ref.abs(), f"HF RMSNorm C={C} out16")


def test_norm_gelu_bf16(dev):
    """usdm_norm, LayerNorm + GELU with a bf16 output only, C = 768 (<5> with idle pieces).  Bound: the bf16 rounding of an f32 value
    within 4 x NORM_GELU_TORCH_FP32_ERR x max |ref| of fp64 (torch's float32 layer_norm + gelu loses 1.95e-7 x max |ref| here)."""
    x, res, g, b = R.norm_gelu_case()
    got = _norm(dev, x, g, b, C=768, rows=R.NORM_ROWS, res=res, act=GELU, want=("out16",))
    ref = R.norm_ref(R.norm_sum32(x, res), g, b, gelu=True)
    tol = 4 * R.NORM_GELU_TORCH_FP32_ERR * float(ref.abs().max())
    _within(got["out16"], ref, R.bf16_of_f32_bound(ref, tol), "LayerNorm + GELU out16")


# ------------------------------------------------------------------------------------------------------------------ w2v_k.hip
@pytest.mark.parametrize("n", (1,) + R.WAVE_LN_N)
def test_wave_layernorm(dev, n):
    """usdm_wave_layernorm over n samples of a waveform on a DC offset of 0.3: fewer samples than threads, 1024 +- 1 and 46 passes + 897.
    n = 1: y is exactly 0.  Bound: 4 x WAVE_LN_TORCH_FP32_ERR x max |y| (torch's float32 layer_norm loses 2.61e-7 x max |y|)."""
    from usdm_amd import ops
    x = R.wave(n, 7 + n)
    y = _flat_out(dev, n)
    ops.wave_layernorm(x.to(dev), y.t, n)
    got = y.take(1, n, "usdm_wave_layernorm")[0]
    if n == 1:
        assert not bool(R.bits(got).any()), "one sample normalises to exactly 0"
        return
    _rel_to_max(got, R.wave_layernorm_ref(x), 4 * R.WAVE_LN_TORCH_FP32_ERR, f"wave_layernorm n={n}")


@pytest.mark.parametrize("stride", R.CONV0_STRIDES)
def test_w2v_conv0(dev, stride):
    """usdm_w2v_conv0 (C = 512, k = 10) at strides 1, 3, 5, 8 x T = 1, 63, 64, 65, 200, with n = (T-1)*stride + 10 exactly (the last
    workgroup's staged window runs past n: zero-filled, not read) and with 1000 samples more.  Reference: fp64 conv1d -> layer_norm
    -> gelu.  Bound: 4 x CONV0_TORCH_FP32_ERR x max |ref| (torch's float32 pipeline loses 3.19e-7 x max |ref| at worst)."""
    from usdm_amd import ops
    w, b, g, be = R.conv0_params()
    wd, bd, gd, bed = (t.to(dev) for t in (w, b, g, be))
    for s, T, n in R.conv0_cases():
        if s != stride:
            continue
        x = R.conv0_wave(n)
        out = Out(dev, T, R.CONV0_C)
        ops.w2v_conv0(x.to(dev), wd, bd, gd, bed, out.t, n=n, T=T, C=R.CONV0_C, k=R.CONV0_K, stride=s)
        got = out.take(T, R.CONV0_C, f"usdm_w2v_conv0 T={T} n={n}")
        _rel_to_max(got, R.conv0_ref(x, T, s, w, b, g, be), 4 * R.CONV0_TORCH_FP32_ERR, f"conv0 stride={s} T={T} n={n}")


@pytest.mark.parametrize("n", R.SOFTMAX_SEG_N)
def test_softmax_segments(dev, n):
    """usdm_softmax_segments in place: rows = 5, nseg = 3, npad = n rounded up to 8, ldseg = npad + 24; pad columns exactly 0, columns
    beyond npad untouched.  Every weight against fp64 under 4 x SOFTMAX_SEG_TORCH_FP32_ERR relative (torch's float32 softmax: 2.08e-6)."""
    from usdm_amd import ops
    rows, nseg = 5, 3
    npad = (n + 7) // 8 * 8
    ldseg = npad + 24
    x = R.softmax_seg_inputs(n, rows, nseg)
    buf = R.sentinel((rows + 1, nseg, ldseg), F32)
    buf[:rows, :, :n] = x
    xd = buf.to(dev)
    ops.softmax_segments(xd, rows=rows, nseg=nseg, n=n, npad=npad, ldrow=nseg * ldseg, ldseg=ldseg)
    torch.cuda.synchronize()
    got = xd.cpu()
    assert bool(R.is_sentinel(got[rows:]).all()) and bool(R.is_sentinel(got[:rows, :, npad:]).all()), "written beyond npad or past the last row"
    assert not bool(R.bits(got[:rows, :, n:npad]).any()), "pad columns must be exactly 0"
    ref = R.softmax_seg_ref(x)
    tol = 4 * R.SOFTMAX_SEG_TORCH_FP32_ERR
    st = P.check_weights(lambda: got[:rows, :, :n], ref, torch.ones_like(ref, dtype=torch.bool), tol=tol, floor=P.FLOOR_EXACT, what=f"softmax_segments n={n}")
    print(st.line(f"softmax_seg_kernel n={n} (tol {tol:.2g})"))


@pytest.mark.parametrize("D", [3, 1280])
@pytest.mark.parametrize("n_units", [1, 255, 256, 257, 10000])
def test_kmeans_argmin(dev, D, n_units):
    """usdm_kmeans_argmin on all-integer inputs (every f32 operation exact: no margin excuse), T = 6, ldd = n_units + 3, with the
    planted minima and ties of _glue_reference.kmeans_case: ids == torch.argmin (the lowest index), margin == second - best exactly
    (0 at a tie, inf for one unit); again with margin = None"""
    from usdm_amd import ops
    x, dots, csq = R.kmeans_case(D, n_units)
    T = x.shape[0]
    ref_ids, ref_margin, dist = R.kmeans_ref(x, dots, csq)
    assert torch.equal(ref_ids, dist.argmin(1))
    if n_units > 300:
        assert ref_ids.tolist() == [0, n_units - 1, 5, 10, 70, 70] and ref_margin[2:].tolist() == [0.0] * 4
    xd, dd, cd = x.to(dev), dots.to(dev), csq.to(dev)
    for with_margin in (True, False):
        ids, margin = _flat_out(dev, T, torch.int64), _flat_out(dev, T)
        ops.kmeans_argmin(xd, dd, cd, ids.t, T=T, D=D, n_units=n_units, ldd=n_units + R.KMEANS_PAD, margin=margin.t if with_margin else None)
        got = ids.take(1, T, "usdm_kmeans_argmin ids")[0]
        assert torch.equal(got, ref_ids), f"ids {got.tolist()} != {ref_ids.tolist()} (margin={with_margin})"
        gm = margin.take(1, T if with_margin else 0, "usdm_kmeans_argmin margin")[0]
        if with_margin:
            assert torch.equal(gm, ref_margin), f"margin {gm.tolist()} != {ref_margin.tolist()}"


# ------------------------------------------------------------------------------------------------------------------ vb_k.hip
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("E", [8, 16])
@pytest.mark.parametrize("dup", [1, 2])
@pytest.mark.parametrize("use_cond", [True, False], ids=["cond", "nocond"])
def test_vb_build_input(dev, dtype, E, dup, use_cond):
    """usdm_vb_build_input: B_in = 2, S = 9, F = 5, ldo = 32 (columns E + 2F .. 32 are pad: exactly 0), null_id = the table's last row,
    ids with row 0 and that last row.  A move (+ one conversion to bf16): exact.  dup = 2: the first B_in batches carry the null row
    and zero cond, both halves the same y."""
    from usdm_amd import ops
    ids, y, cond, table = R.vb_input_case(E, dtype)
    B_in, S = ids.shape
    F, null_id, ldo = y.shape[1], table.shape[0] - 1, 32
    rows = B_in * dup * S
    out = Out(dev, rows, ldo, dtype)
    ops.vb_build_input(ids.to(dev), y.to(dev), cond.to(dev), table.to(dev), out.t, B_in=B_in, dup=dup, S=S, E=E, F=F, null_id=null_id,
                       use_cond=use_cond, ldo=ldo)
    got = out.take(rows, ldo, "usdm_vb_build_input").view(B_in * dup, S, ldo)
    ref = R.vb_build_input_ref(ids, y, cond, table, dup=dup, use_cond=use_cond, null_id=null_id, ldo=ldo)
    _same_bits(got, ref, "A")
    assert not bool(R.bits(got[..., E + 2 * F:]).any()), "pad columns"
    if dup == 2:
        _same_bits(got[:B_in, :, E:E + F], got[B_in:, :, E:E + F], "y of the two halves")
        assert not bool(R.bits(got[:B_in, :, E + F:]).any()) and torch.equal(got[:B_in, :, :E], table[null_id].expand(B_in, S, E))


@pytest.mark.parametrize("H", [16, 1024])
@pytest.mark.parametrize("t_stride", [1, 2])
@pytest.mark.parametrize("tvals", R.TIME_TOKEN_T, ids=["t0", "t1"])
@pytest.mark.parametrize("with16", [True, False], ids=["h16", "h32_only"])
def test_vb_time_token(dev, H, t_stride, tvals, with16):
    """usdm_vb_time_token: Bx = 3, rows_per_batch = 5 (rows 1..4 of every batch keep the sentinel), t in {0, 1e-3, 0.5, 1}.  The
    argument (1000 t) * freqs[i] is formed in float32 in the reference as in the kernel, so the bound covers sinf / cosf only:
    4 x TIME_TOKEN_TORCH_FP32_ERR absolute (torch's float32 sin / cos: 3.54e-8).  h16 == bf16(h32) bit for bit."""
    from usdm_amd import ops
    Bx, rpb = 3, 5
    freqs = R.time_token_freqs(H)
    t = torch.tensor(tvals)
    tbuf = R.sentinel((Bx * t_stride,), F32)
    tbuf[::t_stride] = t
    h32, h16 = Out(dev, Bx * rpb, H), Out(dev, Bx * rpb, H, BF)
    ops.vb_time_token(tbuf.to(dev), freqs.to(dev), h32.t, h16.t if with16 else None, Bx=Bx, H=H, rows_per_batch=rpb, t_stride=t_stride)
    g32 = h32.take(Bx * rpb, H, "h32").view(Bx, rpb, H)
    g16 = h16.take(Bx * rpb if with16 else 0, H, "h16")
    assert bool(R.is_sentinel(g32[:, 1:]).all()), "rows 1.. of a batch were written"
    _within(g32[:, 0], R.time_token_ref(t, freqs), 4 * R.TIME_TOKEN_TORCH_FP32_ERR, f"time token H={H}")
    if with16:
        g16 = g16.view(Bx, rpb, H)
        assert bool(R.is_sentinel(g16[:, 1:]).all()), "rows 1.. of a batch were written (h16)"
        _same_bits(g16[:, 0], g32[:, 0].to(BF), "h16")


class _Solver:
    """the buffers of one usdm_vb_solver_step call: inputs on the device, outputs with a sentinel tail"""

    def __init__(self, dev, c):
        self.dev, self.c, self.n = dev, c, c["n"]
        self.d = {k: c[k].to(dev) for k in ("vout", "vout2", "z", "eps", "cond")}

    def run(self, *, vout="vout", cfg=False, outs=("z_in", "z_commit"), v1=None, alias=False, **kw):
        """-> ({name: [n] on the CPU}, the z buffer afterwards).  v1: an Out to store into (mode 0) / read from (mode 1)"""
        from usdm_amd import ops
        c, n = self.c, self.n
        z = self.d["z"].clone()
        bufs = {o: _flat_out(self.dev, n) for o in outs if not (alias and o == "z_commit")}
        ptr = {o: b.t for o, b in bufs.items()}
        if alias:
            ptr["z_commit"] = z
        if "eps" in kw:
            kw = dict(kw, eps=self.d["eps"], cond=self.d["cond"])
        ops.vb_solver_step(self.d[vout] if cfg else self.d[vout][:n].contiguous(), z, B=c["B"], F=c["F"], S=c["S"], cfg=cfg,
                           v1=None if v1 is None else v1.t, **ptr, **kw)
        got = {o: b.take(1, n, f"usdm_vb_solver_step {o}")[0] for o, b in bufs.items()}
        torch.cuda.synchronize()
        return got, z.cpu()

    def ref(self, *, vout="vout", cfg=False, **kw):
        c = self.c
        if "eps" in kw:
            kw = dict(kw, eps=c["eps"], cond=c["cond"])
        return R.solver_ref(c[vout] if cfg else c[vout][:self.n], c["z"], S=c["S"], cfg=cfg, **kw)


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_vb_solver_euler(dev, cfg):
    """usdm_vb_solver_step, Euler, B = 2, F = 5, S = 67 (670 elements: 2 workgroups + 158), without CFG and with gs = 0.7 (vout holds
    both halves; v1 receives the combined velocity).  Against fp64 under k * 2^-23 * sum|terms|: v = vc + gs * (vc - vu) has k = 3
    (a subtraction, a product, a sum) over |vc| + |gs| (|vc| + |vu|), and is a copy (k = 0: exact) without CFG; z + dt * v adds a
    product and a sum: k = 2 / 5 over |z| + |dt| * (the terms of v)."""
    sv = _Solver(dev, R.solver_case(11))
    kw = dict(mode=0, dt=0.125, cfg=cfg, gs=0.7 if cfg else 0.0)
    v1 = _flat_out(dev, sv.n)
    got, z_after = sv.run(v1=v1, **kw)
    zn, v, bound, vbound = sv.ref(**kw)
    _same_bits(z_after, sv.c["z"], "z (not an output)")
    _same_bits(got["z_in"], got["z_commit"], "z_in vs z_commit")
    _within(got["z_in"], zn, bound, f"Euler cfg={cfg} z")
    gv = v1.take(1, sv.n, "v1")[0]
    if cfg:
        _within(gv, v, vbound, "v1 = the combined velocity")
    else:
        _same_bits(gv, sv.c["vout"][:sv.n], "v1 = vout")


@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_vb_solver_heun(dev, cfg):
    """usdm_vb_solver_step, Heun: the predictor (mode 0) stores v1, the corrector (mode 1, a second velocity) reads it back: the
    reference takes the stored v1 as its input.  z + (dt * (v1 + v)) / 2: a sum, a product, an exact halving, a sum -> k = 3 (+ 3
    for v with CFG) over |z| + |dt| (|v1| + terms of v) / 2."""
    sv = _Solver(dev, R.solver_case(12))
    kw = dict(dt=0.25, cfg=cfg, gs=0.7 if cfg else 0.0)
    v1 = _flat_out(dev, sv.n)
    got, _ = sv.run(v1=v1, mode=0, outs=("z_in",), **kw)
    zn, v, bound, vbound = sv.ref(mode=0, **kw)
    _within(got["z_in"], zn, bound, "predictor z_in")
    stored = v1.take(1, sv.n, "v1")[0]
    _within(stored, v, vbound, "stored v1")
    got, z_after = sv.run(v1=v1, mode=1, vout="vout2", outs=("z_commit",), **kw)
    zn, _, bound, _ = sv.ref(mode=1, vout="vout2", v1=stored, **kw)
    _within(got["z_commit"], zn, bound, "corrector z_commit")
    _same_bits(v1.take(1, sv.n, "v1")[0], stored, "the corrector must not write v1")
    _same_bits(z_after, sv.c["z"], "z (not an output)")
    assert float((zn - sv.ref(mode=0, vout="vout2", **kw)[0]).abs().max()) > 1e-3, "the case does not tell the corrector from an Euler step"


@pytest.mark.parametrize("P_", [0, 13, 67])
@pytest.mark.parametrize("mode", [0, 1], ids=["euler", "corrector"])
def test_vb_solver_renoise(dev, P_, mode):
    """usdm_vb_solver_step with re-noising: exactly the columns s < P take c_eps * eps + c_cond * cond (two products and a sum: k = 3
    over |c_eps eps| + |c_cond cond|), the others the step (P = 0: none, P = S = 67: all).  The two values differ by O(1) where the
    bounds are 1e-6, so a column on the wrong side shows."""
    sv = _Solver(dev, R.solver_case(13))
    v1 = _flat_out(dev, sv.n)
    v1.t[0, :sv.n] = sv.c["vout2"][:sv.n].to(dev)
    stored = sv.c["vout2"][:sv.n]
    kw = dict(mode=mode, dt=0.25, eps=True, P=P_, c_eps=0.6, c_cond=0.4)
    got, z_after = sv.run(v1=v1 if mode else None, **kw)
    zn, _, bound, _ = sv.ref(v1=stored if mode else None, **kw)
    _same_bits(got["z_in"], got["z_commit"], "z_in vs z_commit")
    _within(got["z_in"], zn, bound, f"re-noised step P={P_}")
    col = (torch.arange(sv.n) % sv.c["S"]) < P_
    step = sv.ref(mode=mode, dt=0.25, v1=stored if mode else None)[0]
    assert int(col.sum()) == 10 * P_ and (P_ == 0 or float((zn - step).abs()[col].min()) > 100 * float(bound.max())), "the case cannot tell the sides apart"
    _same_bits(z_after, sv.c["z"], "z (not an output)")


@pytest.mark.parametrize("which", ["z_in", "z_commit", "both", "alias"])
def test_vb_solver_outputs(dev, which):
    """usdm_vb_solver_step writes z_in only, z_commit only, or both; z itself is unchanged unless it IS z_commit (alias: every element
    is read before it is written, by its own thread)"""
    sv = _Solver(dev, R.solver_case(14))
    kw = dict(mode=0, dt=0.5)
    outs = dict(z_in=("z_in",), z_commit=("z_commit",), both=("z_in", "z_commit"), alias=("z_in", "z_commit"))[which]
    got, z_after = sv.run(outs=outs, alias=which == "alias", **kw)
    zn, _, bound, _ = sv.ref(**kw)
    for name, t in got.items():
        _within(t, zn, bound, name)
    if which == "alias":
        _same_bits(z_after, got["z_in"], "z as z_commit")
    else:
        _same_bits(z_after, sv.c["z"], "z (not an output)")


def test_vb_solver_t_cur(dev):
    """usdm_vb_solver_step with t_cur: t_count = 2 entries of a 4-entry buffer become t_next, the rest keep the sentinel"""
    sv = _Solver(dev, R.solver_case(15))
    t_cur = Out(dev, 1, 4)
    sv.run(mode=0, dt=0.5, t_cur=t_cur.t, t_count=2, t_next=0.3)
    got = t_cur.take(1, 2, "t_cur")[0]
    _same_bits(got, torch.tensor([0.3, 0.3], dtype=F32), "t_cur")


@pytest.mark.parametrize("layout,B,T,C", [(0, 3, 300, 1024), (1, 3, 3000, 80)], ids=["rows_major", "channels_first"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("which", ["x32", "x16", "both"])
def test_mask_time(dev, layout, B, T, C, off, which):
    """usdm_mask_time: 921 600 / 720 000 elements on the 2048 x 256 = 524 288 threads the launcher caps at, so the grid-stride loop
    iterates; valid_len = [T, 3, 0].  Exact: zero at t >= valid_len[b] - off, untouched elsewhere."""
    from usdm_amd import ops
    vl = [T, 3, 0]
    shape = (B, T, C) if layout == 0 else (B, C, T)
    n = B * T * C
    x = R.randn(shape, 40 + layout) + 3.0
    args = {}
    for name, dt in (("x32", F32), ("x16", BF)):
        if which in (name, "both"):
            buf = R.sentinel((n + 64,), dt)
            buf[:n] = x.to(dt).reshape(-1)
            args[name] = buf.to(dev)
    ops.mask_time(torch.tensor(vl, dtype=torch.int32, device=dev), B=B, T=T, C=C, layout=layout, off=off, **args)
    torch.cuda.synchronize()
    for name, buf in args.items():
        got = buf.cpu()
        assert bool(R.is_sentinel(got[n:]).all()), f"{name}: written past the end"
        _same_bits(got[:n].view(shape), R.mask_time_ref(x.to(got.dtype), vl, off, layout), name)


# ------------------------------------------------------------------------------------------------------------------ bigvgan_k.hip
@pytest.mark.parametrize("which", ["out32", "out16", "both"])
def test_sum3_scale(dev, which):
    """usdm_sum3_scale: n = 4 * (3 * 256 + 5) (three workgroups of float4 and five more), scale = 1/3.  Two sums and a product, each
    rounded, nothing to contract: exact against float32 ((a + b) + c) * scale and its bf16 rounding."""
    from usdm_amd import ops
    n = 4 * (3 * 256 + 5)
    a, b, c = R.randn((n,), 1), R.randn((n,), 2), R.randn((n,), 3)
    o32, o16 = _flat_out(dev, n), _flat_out(dev, n, BF)
    ops.sum3_scale(a.to(dev), b.to(dev), c.to(dev), 1.0 / 3.0, out32=o32.t if which != "out16" else None, out16=o16.t if which != "out32" else None)
    ref = R.sum3_scale_ref(a, b, c, 1.0 / 3.0)
    g32, g16 = o32.take(1, n if which != "out16" else 0, "out32")[0], o16.take(1, n if which != "out32" else 0, "out16")[0]
    if which != "out16":
        _same_bits(g32, ref, "out32")
    if which != "out32":
        _same_bits(g16, ref.to(BF), "out16")


@pytest.mark.parametrize("B,C,T,Cpad", [(2, 80, 45, 96), (1, 33, 31, 40), (1, 32, 64, 32)])
@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (2.5, -1.25)], ids=["move", "affine"])
def test_cf_to_cl(dev, B, C, T, Cpad, scale, shift):
    """usdm_cf_to_cl [B][C][T] -> [B][T][Cpad], f32 only, bf16 only and both.  scale 1 / shift 0: x * 1 + 0 is exact.  Affine: a
    product and a sum -> k = 2 over |x * scale| + |shift| against fp64; the bf16 output is the bf16 rounding of the f32 one (the same
    value of the same kernel), bit for bit.  Pad channels exactly 0."""
    from usdm_amd import ops
    x = R.randn((B, C, T), 5 + C, 2.0)
    ref, bound = R.cf_to_cl_ref(x, Cpad, scale, shift)
    xd, rows = x.to(dev), B * T
    f32_only = None
    for which in ("out32", "out16", "both"):
        o32, o16 = Out(dev, rows, Cpad), Out(dev, rows, Cpad, BF)
        ops.cf_to_cl(xd, B=B, C=C, T=T, Cpad=Cpad, scale=scale, shift=shift, out32=o32.t if which != "out16" else None,
                     out16=o16.t if which != "out32" else None)
        g32 = o32.take(rows if which != "out16" else 0, Cpad, "out32").view(-1, Cpad)
        g16 = o16.take(rows if which != "out32" else 0, Cpad, "out16").view(-1, Cpad)
        if which != "out16":
            if scale == 1.0:
                _same_bits(g32[..., :C], x.transpose(1, 2).reshape(rows, C), f"{which} out32")
            _within(g32, ref.view(rows, Cpad), bound.view(rows, Cpad), f"cf_to_cl {which} out32")
            assert not bool(R.bits(g32[..., C:]).any()), "pad channels"
            f32_only = g32 if f32_only is None else f32_only
            _same_bits(g32, f32_only, "out32 with and without out16")
        if which != "out32":
            _same_bits(g16, f32_only.to(BF), f"{which} out16")
            assert not bool(R.bits(g16[..., C:]).any()), "pad channels"


@pytest.mark.parametrize("n,n_fft,hop,pad", [(7, 16, 4, 6), (1500, 1024, 256, 384)])
def test_stft_frames(dev, n, n_fft, hop, pad):
    """usdm_stft_frames: a signal one sample longer than the pad (both ends reflect inside one frame) and the mel front end's sizes
    (four passes of 256 threads, five frames); samples beyond +-1 (clamped), a window that is not symmetric.  A clamp and one
    product: exact against F.pad(reflect) -> clamp -> unfold -> * window in float32."""
    from usdm_amd import ops
    T = R.stft_T(n, n_fft, hop, pad)
    x, win = R.randn((n,), 70 + n, 0.8), R.stft_window(n_fft)
    x[1], x[n - 2] = 1.7, -1.3
    out = Out(dev, T, n_fft)
    ops.stft_frames(x.to(dev), win.to(dev), out.t, n=n, n_fft=n_fft, hop=hop, pad=pad, T=T)
    _same_bits(out.take(T, n_fft, "usdm_stft_frames"), R.stft_frames_ref(x, n_fft, hop, pad, win), "frames")


def test_stft_mag(dev):
    """usdm_stft_mag: T = 3, nbins = 513, nbins_pad = 520, ld = 1032, ldo = 528, with an all-zero bin (sqrt(1e-9)).  Two squares, a
    sum, + eps (four roundings of positive terms, halved by the root) and sqrtf -> k = 4 over the result; pad bins exactly 0."""
    from usdm_amd import ops
    T, nbins, npad, ld, ldo, eps = 3, 513, 520, 1032, 528, 1e-9
    ri = R.sentinel((T, ld), F32)
    ri[:, :2 * nbins] = R.randn((T, 2 * nbins), 77, 30.0)
    ri[1, 200] = ri[1, nbins + 200] = 0.0
    out = Out(dev, T, ldo)
    ops.stft_mag(ri.to(dev), out.t, ld=ld, T=T, nbins=nbins, eps=eps, ldo=ldo, nbins_pad=npad)
    got = out.take(T, npad, "usdm_stft_mag")
    ref, bound = R.stft_mag_ref(ri, nbins, eps, npad)
    assert abs(float(ref[1, 200]) - math.sqrt(1e-9)) < 1e-12
    _within(got, ref, bound, "stft_mag")
    assert not bool(R.bits(got[:, nbins:]).any()), "pad bins"


def test_frame_signal(dev):
    """usdm_frame_signal: n = 500, frame_len = 300 (two passes of 256 threads), hop = 7, offset = 11, T = 80: the first frames start
    before 0 and the last run past n.  A move: exact."""
    from usdm_amd import ops
    n, fl, hop, off, T = 500, 300, 7, 11, 80
    x = R.randn((n,), 78) + 2.0
    out = Out(dev, T, fl)
    ops.frame_signal(x.to(dev), out.t, n=n, frame_len=fl, hop=hop, offset=off, T=T)
    ref = R.frame_signal_ref(x, fl, hop, off, T)
    assert not bool(ref[0, :off].any()) and not bool(ref[-1, -1:].any()) and bool(ref[0, off:].all())
    _same_bits(out.take(T, fl, "usdm_frame_signal"), ref, "frames")


# ------------------------------------------------------------------------------------------------- llm_k.hip, llm_attn_k.hip
@pytest.mark.parametrize("Hd", [8, 72, 2400])
def test_embed_rows(dev, Hd):
    """usdm_embed_rows: Hd = 8 (one vector), 72, 2400 (300 vectors on 256 threads); the ids path (n = 5: a repeated id, row 0, the last
    row) and the next_token path (n = 1).  A move: exact; rows past n keep the sentinel."""
    from usdm_amd import ops
    V = 9
    table = R.randn((V, Hd), 90 + Hd).to(BF)
    td = table.to(dev)
    ids = torch.tensor([3, 0, V - 1, 3, 1])
    out = Out(dev, 5, Hd, BF)
    ops.embed_rows(td, out.t, Hd=Hd, ids=ids.to(dev), n=5)
    _same_bits(out.take(5, Hd, "usdm_embed_rows ids"), table[ids], "rows")
    out = Out(dev, 1, Hd, BF)
    ops.embed_rows(td, out.t, Hd=Hd, next_token=torch.tensor([V - 1], dtype=torch.int32, device=dev), n=1)
    _same_bits(out.take(1, Hd, "usdm_embed_rows next_token"), table[V - 1:], "row of next_token")


@pytest.mark.parametrize("n", [1, 255, 4099])
def test_residual_add(dev, n):
    """usdm_residual_add h = bf16(h + bf16(delta)): delta with exact bf16 ties, and values whose bf16 rounding makes the sum a tie
    (without the inner rounding the sum lands on the other side).  Two roundings: exact against torch."""
    from usdm_amd import ops
    h, d = R.residual_add_case(n)
    ref = R.residual_add_ref(h, d)
    if n > 5:
        assert not torch.equal(ref[:6], (h.float() + d).to(BF)[:6]), "the case does not need the inner rounding"
    buf = _flat_out(dev, n, BF)
    buf.t[0, :n] = h.to(dev)
    ops.residual_add(buf.t, d.to(dev), n)
    _same_bits(buf.take(1, n, "usdm_residual_add")[0], ref, "h")


@pytest.mark.parametrize("pos0", [0, 91])
@pytest.mark.parametrize("with_vt", [True, False], ids=["vt", "no_vt"])
def test_rope_cache(dev, pos0, with_vt):
    """usdm_rope_cache (bf16): Hq = 4, Hkv = 2, S = 37, ctx_max = max_pos = 128, ld = nq + 128, vt_ld = 64.  Reference: HF's
    q * cos + rotate_half(q) * sin evaluated by torch on the CPU in bfloat16 (every product and the sum round to bf16), tables from
    oracle.mistral_oracle.rope_tables.  Bit-exact: q roped in place; the k and v sections of qkv and the stride gap unchanged; K cache
    rows pos0 .. pos0 + S - 1 = the roped k, every other row the sentinel; V cache = v; vt the transpose, columns >= S untouched."""
    from usdm_amd import ops
    Hq, Hkv, S, ctx, vt_ld = (R.ROPE[k] for k in ("Hq", "Hkv", "S", "ctx", "vt_ld"))
    qkv0 = R.rope_case()
    nq = qkv0.shape[1]
    ld = nq + 128
    cos, sin = R.rope_tables(ctx)
    buf = _strided(qkv0, ld, dev)
    kc, vc, vt = (R.sentinel(s, BF, dev) for s in ((Hkv, ctx, 128), (Hkv, ctx, 128), (Hkv, 128, vt_ld)))
    ops.rope_cache(buf, cos[:, :64].contiguous().to(dev), sin[:, :64].contiguous().to(dev), kc, vc, ld=ld, S=S, pos0=pos0, Hq=Hq, Hkv=Hkv,
                   ctx_max=ctx, max_pos=ctx, vt=vt if with_vt else None, vt_ld=vt_ld)
    torch.cuda.synchronize()
    got, kc, vc, vt = buf.cpu(), kc.cpu(), vc.cpu(), vt.cpu()
    heads = qkv0.view(S, Hq + 2 * Hkv, 128)
    q_ref, k_ref, v = R.rope_ref(heads[:, :Hq], pos0, cos, sin), R.rope_ref(heads[:, Hq:Hq + Hkv], pos0, cos, sin), heads[:, Hq + Hkv:]
    assert q_ref.dtype == BF
    _same_bits(got[:S, :Hq * 128], q_ref.reshape(S, -1), "q roped in place")
    _same_bits(got[:S, Hq * 128:nq], qkv0[:, Hq * 128:], "the k and v sections of qkv")
    assert bool(R.is_sentinel(got[:S, nq:]).all()) and bool(R.is_sentinel(got[S:]).all()), "the stride gap / the row past S"
    _same_bits(kc[:, pos0:pos0 + S], k_ref.transpose(0, 1), "K cache rows")
    _same_bits(vc[:, pos0:pos0 + S], v.transpose(0, 1), "V cache rows")
    for name, c in (("K", kc), ("V", vc)):
        assert bool(R.is_sentinel(c[:, :pos0]).all()) and bool(R.is_sentinel(c[:, pos0 + S:]).all()), f"{name} cache rows outside pos0 .. pos0 + S"
    if with_vt:
        _same_bits(vt[:, :, :S], v.permute(1, 2, 0), "vt")
        assert bool(R.is_sentinel(vt[:, :, S:]).all()), "vt columns >= S"
    else:
        assert bool(R.is_sentinel(vt).all())
