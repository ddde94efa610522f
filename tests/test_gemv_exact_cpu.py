"""tests/_gemv_reference.py checked on the CPU: the reference against torch.nn.functional on float data, the conditions under which
its cases are exact (2^24 headroom, the SwiGLU grid, the exact RMSNorm family, the 2 % cap of the probe), and that every case
reaches the instantiation it is listed under and every instantiation is reached.  The merged-attention input: its two families'
conditions (the exact merge in two float32 orders, the probe's bound against half an ulp), its launch selection and what usdm_gemv
refuses before a launch."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import _gemv_reference as R
from tests._gemv_reference import BF


def test_launch_selection_mirror():
    """the output counts of VALU_INST reach their instantiation; the odd ones leave the last workgroup ragged"""
    for (rw, glu, nwv), nout in R.VALU_INST.items():
        assert R.valu_select(nout * (2 if glu else 1), glu=glu)[:3] == (rw, glu, nwv), (rw, glu, nwv)
    for nout in (37, 4081, 8193, 16369, 5136):
        rw, _, nwv, _ = R.valu_select(nout * (2 if nout == 5136 else 1), glu=nout == 5136)
        assert nout % (rw * nwv) != 0 or nout == 5136                                       # the last workgroup is ragged
    assert R.valu_select(R.LM_N, lm_head=True)[:3] == (4, False, 4) and R.valu_select(4096, lm_head=True)[:3] == (4, False, 4)
    assert R.valu_select(14336, glu=True, batched=True)[:3] != (2, True, 7)                 # batch-1 only
    assert [R.ring_depth(*i[:2]) for i in R.VALU_INST] == [8, 8, 5, 4, 8, 8, 8, 4, 4]
    # matrix cores: rows per tile, the K split
    assert R.mfma_select(6144, 4096)["rt"] == 12 and R.mfma_select(R.N_RAGGED16, 4096)["rt"] == 16 and R.mfma_select(R.N_SMALL, 4096)["rt"] == 8
    assert R.N_RAGGED16 % 16 != 0
    assert [R.mfma_select(R.N_SMALL, K, ks=True)["ksplit"] for K in (6144, 14336, 16384, 4096, 5120)] == [3, 7, 8, 1, 1]
    assert R.mfma_select(R.LM_N, 256, lm_head=True)["grid"] == 63 and R.mfma_select(R.N_SWIGLU, 256, glu=True)["ntiles"] == 6


def test_every_case_reaches_its_instantiation_and_every_instantiation_is_reached():
    cases = R.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    valu, mfma, bans = set(), set(), set()
    for c in cases:
        if c.lm_head:
            bans.add(("matrix cores" if c.mfma else "valu batch" if c.nb else "usdm_gemv", c.ban))
        if c.mfma:
            assert c.selected() == (c.variant, c.rt), c.name
            mfma.add(c.variant)
            continue
        want = (4, False, 4) if c.inst == "lm" else c.inst
        assert c.selected() == want, c.name
        valu.add((c.inst, c.nb))
    assert {i for i, nb in valu if nb == 0} == set(R.VALU_INST) | {"lm"}
    assert {(i, nb) for i, nb in valu if nb} == {(i, nb) for i in R.BATCH_INST + ("lm",) for nb in R.VALU_NB}
    assert mfma == set(R.MFMA_VARIANTS)
    assert bans == {(f, b) for f in ("usdm_gemv", "valu batch", "matrix cores") for b in R.BANS} and len(R.BANS) == 5
    for nb in R.MFMA_NB:                                        # ... in the matrix-core form for every batch size, "none" with a NULL array
        assert {c.ban for c in R.lm_head_cases(nb, mfma=True)} == set(R.BANS)
        assert all((R.build(c).ban is None) == (c.ban == "none") for c in R.lm_head_cases(nb, mfma=True))
    rts = {(c.rt, c.glu, c.lm_head) for c in cases if c.mfma}
    assert {(8, False, False), (12, False, False), (16, False, False), (16, True, False), (16, False, True)} <= rts


def test_sentinels_of_every_output_dtype():
    """the second fill differs from the first in every output dtype, int32 (part_idx) included, and neither is a NaN"""
    for dt in (R.F32, BF, torch.int32):
        a, b = R.sentinel((3,), dt), R.alt_sentinel((3,), dt)
        assert a.dtype == dt and b.dtype == dt and bool(R.is_sentinel(a).all()) and not bool(R.is_sentinel(b).any())
        assert not torch.equal(R.bits(a), R.bits(b)) and bool((a == a).all()) and bool((b == b).all())
    assert R.alt_sentinel((1,), torch.int32).item() == -7 and R.sentinel((1,), torch.int32).item() == 7


def test_k_ladders():
    assert R.k_ladder((1, False, 4), True) == [8, 504, 512, 520, 2048, 2056, 4088, 4096, 4104, 16384]
    assert R.k_ladder("lm", True) == [8, 504, 512, 520, 2040, 2048, 2056, 16384]
    assert R.k_ladder((1, False, 16), False) == [504, 4104, 8200] and R.k_ladder((2, False, 12), False) == [504, 4104, 6152]
    assert R.k_ladder((3, False, 4), False) == [504, 2056, 2568] and R.k_ladder((2, True, 7), False) == [504, 2056, 3592]


def test_quant_ring_mirror_and_k_ladders():
    """the FP8 ring is twice the bf16 one, an MXFP4 slot is a group of four iterations; every ladder has a K above one ring whose last
    iteration is ragged (FP8: the refill meets the redirect to the row start) or whose last group is partial (MXFP4)"""
    assert [R.fmt_ring_depth(*i[:2], "fp8") for i in R.VALU_INST] == [16, 16, 10, 8, 16, 16, 16, 8, 8]
    assert [R.fmt_ring_depth(*i[:2], "mxfp4") for i in R.VALU_INST] == [4, 4, 2, 2, 4, 4, 4, 2, 2]
    assert [R.fmt_ring_depth(*i[:2]) for i in R.VALU_INST] == [R.ring_depth(*i[:2]) for i in R.VALU_INST]
    assert R.k_ladder((1, False, 4), True, "fp8") == [8, 504, 512, 520, 2048, 2056, 8184, 8192, 8200, 16384]
    assert R.k_ladder((3, False, 4), False, "fp8") == [504, 2056, 5128]
    assert R.k_ladder("lm", True, "fp8") == [8, 504, 512, 520, 2048, 2056, 4088, 4096, 4104, 16384]
    assert R.k_ladder((4, False, 4), False, "fp8") == [504, 2056, 4104] and R.k_ladder((2, True, 7), False, "fp8") == [504, 3592, 4104]
    assert R.k_ladder((1, False, 16), False, "fp8") == [504, 8200] and R.k_ladder((2, False, 12), False, "fp8") == [504, 6152, 8200]
    assert R.k_ladder((1, False, 4), True, "mxfp4") == [32, 480, 512, 544, 2016, 2048, 2080, 8160, 8192, 8224, 16384]
    assert R.k_ladder((1, True, 4), True, "mxfp4") == R.k_ladder((1, False, 4), True, "mxfp4")
    assert R.k_ladder((3, False, 4), False, "mxfp4") == [480, 2080, 4128] and R.k_ladder((2, True, 7), False, "mxfp4") == [480, 2080, 3616, 4128]
    assert R.k_ladder((1, False, 16), False, "mxfp4") == [480, 2080, 8224] and R.k_ladder((2, False, 12), False, "mxfp4") == [480, 2080, 6176, 8224]
    assert R.k_ladder((1, False, 4), True) == R.k_ladder((1, False, 4), True, "bf16")
    for fmt in R.FMTS:
        for inst in R.quant_insts(fmt):
            rw, glu, _ = (4, False, 4) if inst == "lm" else inst
            ring = (2048 if fmt == "mxfp4" else 512) * R.fmt_ring_depth(rw, glu, fmt)
            ks = R.k_ladder(inst, R.is_small(inst), fmt)
            assert any(K > ring and K % (2048 if fmt == "mxfp4" else 512) != 0 for K in ks), (fmt, inst)
            assert all(K % R.k_step(fmt) == 0 and K <= 16384 for K in ks)
            assert {c.K for c in R.valu_plain_cases(inst, fmt=fmt)} == set(ks) == {c.K for c in R.valu_norm_exact_cases(inst, fmt=fmt)}


def test_quant_cases_reach_every_format_instantiation_and_variant():
    """every (format, instantiation), every (format, batch size) and every FP8 matrix-core variant has its cases, each in the families
    the issue lists; the quantized cases are new names next to the bf16 ones, which keep theirs"""
    cases = R.quant_cases()
    assert all(c.fmt in R.FMTS and c.name.startswith(c.fmt + " ") and not c.delta for c in cases)
    assert not [c for c in R.all_cases() if c.fmt == "bf16" and c.name.split()[0] in R.FMTS]
    fams = {}
    for c in cases:
        if c.mfma:
            assert c.fmt == "fp8" and c.form in (0, 5) and c.selected() == (c.variant, c.rt) and c.ldw % 16 == 0, c.name
            continue
        assert c.selected() == ((4, False, 4) if c.inst == "lm" else c.inst) and c.form in (0, -1), c.name
        fam = "skip" if c.skip else "probe" if c.kind == "probe" else "norm-exact" if c.norm else "bans" if (c.lm_head and c.ban != "none") else "plain"
        fams.setdefault((c.fmt, c.inst, c.nb), set()).add(fam)
    for fmt in R.FMTS:
        for inst in R.quant_insts(fmt):
            assert {"plain", "norm-exact", "probe"} <= fams[(fmt, inst, 0)], (fmt, inst)
        for nb in R.VALU_NB:
            for inst in R.quant_batch_insts(fmt):
                assert {"plain", "norm-exact", "probe"} <= fams[(fmt, inst, nb)], (fmt, inst, nb)
        assert all("skip" in fams[(fmt, inst, 0)] for inst in R.DELTA_INST)
    assert all("bans" in fams[("fp8", "lm", nb)] for nb in (0,) + R.VALU_NB) and not [k for k in fams if k[0] == "mxfp4" and k[1] == "lm"]
    for nb in (0,) + R.VALU_NB:
        assert {c.ban for c in R.lm_head_cases(nb, fmt="fp8")} == set(R.BANS) and any(c.idx_offset for c in R.lm_head_cases(nb, fmt="fp8"))
    mf = [c for c in cases if c.mfma]
    assert {c.variant for c in mf} == set(R.FP8_MFMA_VARIANTS) and {c.nb for c in mf} == set(R.MFMA_NB)
    for nb in R.MFMA_NB:
        of = [c for c in mf if c.nb == nb]
        assert {c.variant for c in of} == set(R.FP8_MFMA_VARIANTS) and {c.ban for c in of if c.lm_head} == set(R.BANS)
        assert {(c.rt, c.glu, c.lm_head) for c in of} >= {(8, False, False), (12, False, False), (16, False, False), (16, True, False), (16, False, True)}
        assert {(c.N, c.form) for c in of if c.N in (R.N_ROWS12, R.N_RAGGED16)} == {(N, f) for N in (R.N_ROWS12, R.N_RAGGED16) for f in (0, 5)}
        assert {c.kind for c in of if c.norm} == {"int", "swiglu", "probe"} and max(c.K for c in of if c.norm) == 4096
        # the rows of the bf16 ladder that usdm_gemv_fp8_mfma accepts, form 1 as its form 0
        assert [(c.K, c.form, c.ks) for c in R.mfma_ladder_cases(nb, "fp8")] == [(K, 0 if f == 1 else f, ks) for K, f, ks in R.MFMA_LADDER if f != 3]


def _quant_groups():
    out = []
    for fmt in R.FMTS:
        for i in R.quant_insts(fmt):
            out.append((f"{fmt}-{R.inst_id(i)}", lambda i=i, fmt=fmt: R.valu_plain_cases(i, fmt=fmt) + R.valu_norm_exact_cases(i, fmt=fmt) + R.valu_probe_cases(i, fmt=fmt)))
        out.append((f"{fmt}-rest", lambda fmt=fmt: [c for i in R.DELTA_INST for c in R.skip_cases(i, fmt)] + (R.lm_head_cases(fmt="fp8") if fmt == "fp8" else [])))
        for nb in R.VALU_NB:
            out.append((f"{fmt}-nb{nb}", lambda nb=nb, fmt=fmt: [c for i in R.quant_batch_insts(fmt) for c in R.valu_plain_cases(i, nb, fmt) + R.valu_norm_exact_cases(i, nb, fmt)
                                                                + R.valu_probe_cases(i, nb, fmt)] + (R.lm_head_cases(nb, fmt="fp8") if fmt == "fp8" else [])))
    for nb in R.MFMA_NB:
        out.append((f"fp8-mfma-nb{nb}", lambda nb=nb: R.mfma_ladder_cases(nb, "fp8") + R.mfma_tile_cases(nb, "fp8") + R.mfma_swiglu_cases(nb, "fp8") + R.mfma_norm_cases(nb, "fp8")
                    + R.lm_head_cases(nb, mfma=True, fmt="fp8")))
    return out


def test_quant_groups_are_all_the_quantized_cases():
    assert sorted(c.name for g in _quant_groups() for c in g[1]()) == sorted(c.name for c in R.quant_cases())


@pytest.mark.parametrize("group", _quant_groups(), ids=lambda g: g[0])
def test_quant_exactness_conditions(group):
    """per quantized case: dequantize(quantize(W)) is W bit for bit (no MXFP4 code a negative zero), so the fp64 reference of the bf16
    kernels is the exact reference of the quantized ones; rows / blocks carry different scales; sum |W| |x'| + |residual| in units of
    the smallest weight step stays below 2^24 (every partial sum is exact in f32 in any order, and so is the sum with the residual);
    SwiGLU pre-activations stay within +-20; the exact RMSNorm family, the probe's 2 % cap and the SwiGLU rounding cap hold for the
    reference alone"""
    from usdm_amd import quant
    worst, nsw, dsw = 0.0, 0, 0
    for c in group[1]():
        d = R.build(c)
        xb = d.x.view(c.B + 1, c.x_bs)
        assert bool(torch.isnan(xb[:, c.K:]).all()) and bool(torch.isnan(xb[c.B]).all()) and d.W is None
        # ---- lossless, and the buffers as the kernels get them
        W, ldw = R.device_weight(c, d)
        if c.fmt == "fp8":
            assert ldw == c.ldw and W.q.shape == (c.N + 1, ldw) and W.e.shape == (c.N + 1,) and ldw >= c.K + 8
            assert bool((W.q[:, c.K:] == R.FP8_NAN).all()) and bool((W.q[c.N] == R.FP8_NAN).all())
            assert bool(torch.isnan(W.q[c.N:, c.K:].view(torch.float8_e4m3fn).float()).all())
            back, scales = quant.dequantize_rows(W.q[:c.N, :c.K], W.e[:c.N]), W.e[:c.N]
            per_row = 1
        else:
            codes, scales = W.unpack()
            assert ldw is None and W.K == c.K and W.N == c.N and not bool((codes == 8).any()), c.name
            back = quant.dequantize_mxfp4(codes, scales)
            per_row = max(int(r.unique().numel()) for r in scales[:8])
        assert torch.equal(R.bits(back), R.bits(d.Wl)), f"{c.name}: quantization is not lossless"
        wb, _ = R.device_weight(c, d, fmt="bf16")                            # (what the bf16 entry point is given for the comparison)
        wb = wb.view(c.N + 1, c.K + R.PAD)
        assert torch.equal(R.bits(wb[:c.N, :c.K]), R.bits(d.Wl)) and bool(torch.isnan(wb[:, c.K:]).all()) and bool(torch.isnan(wb[c.N]).all())
        # ---- scales that differ between neighbouring rows and blocks
        if c.kind != "probe" and c.N >= 8:
            assert int(scales.unique().numel()) >= 4 and (c.fmt == "fp8" or per_row >= 2 or c.K == 32), (c.name, scales.unique().tolist())   # (K = 32: one block per row)
            # the next row's and the next wave's scale is another one, and most gate / up partners' (16 rows on); MXFP4: and the next block's and the next group's (ring slot's)
            x_ = d.wexp
            assert bool((x_[1:] != x_[:-1]).all()) and bool((x_[4:] != x_[:-4]).all()) and float((x_[16:] != x_[:-16]).float().mean()) > 0.5, c.name
            assert c.fmt == "mxfp4" or bool((scales[1:8] != scales[0:7]).all()), c.name
            if c.fmt == "mxfp4" and c.kind == "int":
                assert bool((x_[:, 1:] != x_[:, :-1]).all()) and bool((x_[:, 64:] != x_[:, :-64]).all()) and bool((x_[:, 128:] != x_[:, :-128]).all()), c.name
                if c.K >= 4096:     # ... in the scale bytes themselves, wherever both blocks hold a 3 (nearly everywhere)
                    assert float((scales[:, 64:] != scales[:, :-64]).float().mean()) > 0.9, c.name
        e = R.expected(c, d, rbf=False)
        if c.kind == "probe":
            assert d.wexp is None and bool(((d.Wl == 0) | (d.Wl == 1)).all())
            lo, hi = R.expected(c, d, rbf=False, scale=1 - R.DELTA)["y"], R.expected(c, d, rbf=False, scale=1 + R.DELTA)["y"]
            share = float((lo.vals != hi.vals)[lo.owned].double().mean())
            worst = max(worst, share)
            assert share <= R.PROBE_CAP, (c.name, share)
            assert bool(((e["y"].vals == lo.vals) | (e["y"].vals == hi.vals)).all())
            continue
        # ---- 2^24 headroom in units of the smallest step: W is a multiple of 2^emin, x' of xu, the residual an integer
        emin = int(d.wexp.min())
        assert (-3 <= emin <= int(d.wexp.max()) <= 0) if c.kind == "swiglu" else (emin == (-3 if c.fmt == "fp8" else 0) and int(d.wexp.max()) == 3)
        xp = R.x_prime(c, d)[0]
        xu = 1.0 / 16 if c.kind == "swiglu" else 1.0
        step = 2.0 ** min(emin, 0) * xu
        Wd = d.Wl.double()
        assert bool((Wd / 2.0 ** emin == (Wd / 2.0 ** emin).round()).all()) and bool((xp / xu == (xp / xu).round()).all()), c.name
        absum = max(float((xp.abs() @ Wd[r0:r0 + 2048].abs().T).max()) for r0 in range(0, c.N, 2048))
        res_max = float(d.rl.abs().max()) if d.rl is not None else 0.0
        assert (absum + res_max) / step < 2.0 ** 24 and d.acc_max <= absum, (c.name, absum, step)
        if c.kind == "swiglu":
            y = e["y"]
            assert float(y.pre[y.owned].abs().max()) <= 20.0 and float(y.up[y.owned].abs().max()) <= 20.0, c.name
            g, u, ref = y.pre[y.owned], y.up[y.owned], R.expected(c, d, rbf=True)["y"].vals[y.owned]
            t32 = R.swiglu_rbf_ref(g, u, dtype=R.F32)
            assert bool(((t32 - ref).abs() <= R.bf16_ulp(ref)).all()) and torch.equal(ref.float().to(BF).double(), ref), c.name
            nsw, dsw = nsw + ref.numel(), dsw + int((t32 != ref).sum())
        if c.norm == "exact":
            a, b = R.x_prime(c, d, 1 - 2.0 ** -10)[0], R.x_prime(c, d, 1 + 2.0 ** -10)[0]    # rstd ~ 1/2: 2^-11 absolute either side
            assert torch.equal(a, b) and torch.equal(a.abs(), d.gl.abs().expand_as(a)), c.name
    if worst:
        print(f"[gemv] {group[0]}: the probe's references differ on at most {100 * worst:.2f} % of a case's elements (cap 2 %)")
    if nsw:
        print(f"[gemv] {group[0]}: torch float32 differs from the fp64 SwiGLU reference with round_bf16 on {dsw} of {nsw} outputs")
        assert dsw <= R.FLIP_CAP * nsw, (group[0], dsw, nsw)


def _float_case(**kw):
    """a small case whose operands are replaced by float data"""
    c = R.Case("float", N=96, K=520, seed=5, **kw)
    d = R.build(c)
    g = R.gen(77)
    d.Wl = (torch.randn(c.N, c.K, generator=g) * c.K ** -0.5).to(BF)
    d.xl = torch.randn(c.B, c.K, generator=g).to(BF).double()
    return c, d


def test_reference_against_torch_functional():
    # plain + residual, both rounding modes
    c, d = _float_case(res=True, nb=3, form=-1)
    lin = Fn.linear(d.xl, d.Wl.double())
    e = R.expected(c, d, rbf=False)["y"]
    assert torch.equal(e.vals[e.owned].view(3, -1), lin + d.rl)
    e = R.expected(c, d, rbf=True)["y"]
    assert torch.equal(e.vals[e.owned].view(3, -1), (lin.to(BF).double() + d.rl).to(BF).double())
    assert int(e.owned.sum()) == 3 * 96 and not bool(e.owned.view(4, -1)[3].any()) and not bool(e.owned.view(4, -1)[:, 96:].any())
    # RMSNorm with HF's rounding points, then the projection
    c, d = _float_case(norm="probe", kind="int")
    xn = (d.xl * torch.rsqrt(d.xl.pow(2).mean(-1, keepdim=True) + R.EPS32)).float().to(BF).double()
    xn = (xn * d.gl).float().to(BF).double()
    e = R.expected(c, d, rbf=False)["y"]
    assert torch.equal(e.vals[e.owned].view(1, -1), Fn.linear(xn, d.Wl.double()))
    # SwiGLU on packed rows
    c, d = _float_case(glu=True, kind="swiglu")
    lin = Fn.linear(d.xl, d.Wl.double()).view(1, 3, 2, 16)
    gate, up = lin[:, :, 0].reshape(1, -1), lin[:, :, 1].reshape(1, -1)
    e = R.expected(c, d, rbf=False)["y"]
    assert torch.equal(e.vals[e.owned].view(1, -1), Fn.silu(gate) * up)
    e = R.expected(c, d, rbf=True)["y"]
    ref = (Fn.silu(gate.to(BF).double()).to(BF).double() * up.to(BF).double()).to(BF).double()
    assert torch.equal(e.vals[e.owned].view(1, -1), ref)
    # x_delta
    c, d = _float_case(delta=True)
    d.dl = torch.randn(c.K, generator=R.gen(3)).float().double()
    xp = (d.xl + d.dl.to(BF).double()).to(BF).double()
    e = R.expected(c, d, rbf=False)
    assert torch.equal(e["x_out"].vals[:c.K], xp[0]) and torch.equal(e["y"].vals[e["y"].owned].view(1, -1), Fn.linear(xp, d.Wl.double()))


@pytest.mark.parametrize("mfma", [False, True])
def test_lm_head_reference(mfma):
    """logits, ban mask and partials: the best partial is the lowest-id arg-max of the masked logits; fully banned blocks say so"""
    for c in R.lm_head_cases(nb=3, mfma=mfma):
        d = R.build(c)
        e = R.expected(c, d, rbf=True)
        lg = Fn.linear(R.x_prime(c, d)[0], d.Wl.double()).to(BF).double()
        lg[:, d.banl.bool()] = -R.INF
        y = e["y"].vals.view(c.B + 1, -1)[:c.B, :c.N]
        assert torch.equal(y, lg)
        pv, pi = e["part_val"].vals.view(c.B + 1, -1)[:c.B], e["part_idx"].vals.view(c.B + 1, -1)[:c.B]
        for b in range(c.B):
            best = pv[b].max()
            assert best == lg[b].max() and int(pi[b][pv[b] == best].min()) - c.idx_offset == int((lg[b] == best).nonzero()[0])
        if c.ban == "workgroup":
            assert bool((pv[:, 1:3] == -R.INF).all()) and bool((pi[:, 1:3] == R.NO_IDX).all()) and pv[0, 62] == -R.INF
        if c.ban == "wave":
            assert bool((pi[:, 1] == 31 + c.idx_offset).all())
        if mfma:
            assert bool((pv[:, c.nparts:] == -R.INF).all()) and bool((pi[:, c.nparts:] == R.NO_IDX).all()) and pv.shape[1] == c.part_bs
        ties = sum(int(((lg[b] == lg[b].max()).sum() > 1)) for b in range(c.B))
        print(f"[gemv] {c.name}: {ties} of {c.B} items have tied maxima")


def test_probe_positions():
    for c in R.valu_probe_cases((1, False, 4)) + R.valu_probe_cases((1, False, 16)) + R.valu_probe_cases((1, True, 4)):
        pos = R.probe_positions(c)
        assert pos.numel() == c.nout and int(pos.min()) >= 0 and int(pos.max()) < c.K
        if c.nout >= c.K:
            assert set(pos.tolist()) == set(range(c.K))
            continue
        assert pos.unique().numel() == pos.numel() and set(range(c.K - 16, c.K)) <= set(pos.tolist())
        step = 8 * c.threads()
        if step < c.K:
            assert {step - 1, step, step + 7} <= set(pos.tolist())


def _groups():
    out = [("valu-" + R.inst_id(i), (lambda i=i: R.valu_plain_cases(i) + R.valu_norm_exact_cases(i) + R.valu_probe_cases(i))) for i in list(R.VALU_INST) + ["lm"]]
    out.append(("valu-rest", lambda: R.lm_head_cases() + [c for i in R.DELTA_INST for c in R.delta_cases(i) + R.skip_cases(i)]))
    for nb in R.VALU_NB:
        out.append((f"valu-nb{nb}", lambda nb=nb: [c for i in R.BATCH_INST + ("lm",) for c in R.valu_plain_cases(i, nb) + R.valu_norm_exact_cases(i, nb) + R.valu_probe_cases(i, nb)]
                    + R.lm_head_cases(nb)))
    for nb in R.MFMA_NB:
        out.append((f"mfma-nb{nb}", lambda nb=nb: R.mfma_ladder_cases(nb) + R.mfma_tile_cases(nb) + R.mfma_swiglu_cases(nb) + R.mfma_norm_cases(nb) + R.lm_head_cases(nb, mfma=True)))
    return out


@pytest.mark.parametrize("group", _groups(), ids=lambda g: g[0])
def test_exactness_conditions(group):
    """per case: max |acc| + max |res| < 2^24; SwiGLU pre-activations are multiples of 1/16 within +-20; the exact RMSNorm family gives
    x' = +-norm_w for any rstd within 2^-11 of 1/2; the probe's two references differ on at most 2 % of the elements"""
    worst = 0.0
    for c in group[1]():
        d = R.build(c)
        e = R.expected(c, d, rbf=False)
        Wb, xb = d.W.view(c.N + 1, c.ldw), d.x.view(c.B + 1, c.x_bs)
        assert bool(torch.isnan(Wb[:, c.K:]).all()) and bool(torch.isnan(Wb[c.N]).all()) and bool(torch.isnan(xb[:, c.K:]).all()) and bool(torch.isnan(xb[c.B]).all())
        if c.kind == "probe":
            lo, hi = R.expected(c, d, rbf=False, scale=1 - R.DELTA)["y"], R.expected(c, d, rbf=False, scale=1 + R.DELTA)["y"]
            share = float((lo.vals != hi.vals)[lo.owned].double().mean())
            worst = max(worst, share)
            assert share <= R.PROBE_CAP, (c.name, share)
            mid = e["y"].vals
            assert bool(((mid == lo.vals) | (mid == hi.vals)).all())
            continue
        res_max = float(d.rl.abs().max()) if d.rl is not None else 0.0
        if c.kind == "swiglu":
            y = e["y"]
            for v in (y.pre[y.owned], y.up[y.owned]):
                assert bool((v * 16 == torch.round(v * 16)).all()) and float(v.abs().max()) <= 20.0, (c.name, float(v.abs().max()))
        else:
            assert d.acc_max + res_max < 2.0 ** 24, c.name
            assert bool((d.Wl.abs() <= 3).all()) and bool((d.Wl == d.Wl.round()).all())
            if c.K >= 504 and not c.norm and not c.lm_head and not c.delta:          # most sums exceed 256: round_bf16 does something
                y = e["y"]
                assert float((y.vals[y.owned].abs() > 256).double().mean()) > 0.5, c.name
        if c.norm == "exact":
            a, b = R.x_prime(c, d, 1 - 2.0 ** -10)[0], R.x_prime(c, d, 1 + 2.0 ** -10)[0]    # rstd ~ 1/2: 2^-11 absolute either side
            assert torch.equal(a, b) and torch.equal(a.abs(), d.gl.abs().expand_as(a)), c.name
    if worst:
        print(f"[gemv] {group[0]}: the probe's references differ on at most {100 * worst:.2f} % of a case's elements (cap 2 %)")


# ------------------------------------------------------------------------------------------------------------------ merged-attention input
def _gemv_threads(c):
    """usdm_gemv_threads on the arguments that make the selection (dummy addresses: nothing is read)"""
    import ctypes
    from usdm_amd import _lib
    kw = dict(mrg_pm=8, mrg_pl=8, mrg_po=8, mrg_ns=c.NS, **(dict(cmb_gran=8, cmb_err=8) if c.merge == "cmb" else {})) if c.merge else {}
    a = _lib.GemvArgs(W=8, x=8, N=c.N, K=c.K, ldw=c.ldw, act=c.act, y32=8, **kw)
    return _lib.lib.usdm_gemv_threads(ctypes.byref(a))


def test_merge_selection_mirror_and_coverage():
    """valu_select's merge row agrees with usdm_gemv_threads, as Run.threads asks of every GPU case; the three instantiations, every
    shape, the NS ladders and the variants of the issue are all there"""
    cases = R.merge_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.selected() == c.inst and _gemv_threads(c) == c.threads() == 64 * c.inst[2], c.name
    assert R.valu_select(4096, merge="mrg") == (1, False, 16, 256) == R.valu_select(4096, merge="cmb") and R.valu_select(37, merge="mrg") == (1, False, 4, 10)
    assert R.valu_select(6144, merge="mrg") == (1, False, 4, 1536) and R.valu_select(16369, merge="mrg")[:3] == (1, False, 4)     # (plain: 2 x 12 waves, 4 rows per wave)
    for N in (37, 4081, 6144, 16369, 4096):
        assert _gemv_threads(R.Case("t", N=N, K=128, seed=0, merge="mrg", NS=2)) == 64 * R.valu_select(N, merge="mrg")[2], N
    for form in R.MERGE_FORMS:
        ex = [c for s in R.MERGE_SHAPES[form] for c in R.merge_exact_cases(form, s)]
        assert {(c.N, c.K) for c in ex} == set(R.MERGE_SHAPES[form]) and all(c.merge == ("cmb" if form == "cmb" else "mrg") for c in ex)
        assert {c.NS for c in ex if (c.N, c.K) == R.MERGE_NS_AT[form]} == set(R.MERGE_NS[form])
        for s in R.MERGE_SHAPES[form]:
            assert set(R.MERGE_NS_PAIR[form]) <= {c.NS for c in ex if (c.N, c.K) == s}
        assert {(c.res, c.inplace) for c in ex} == {(False, False), (True, False), (True, True)}
        assert [c.skip for c in R.merge_skip_cases(form)] == [True] and {(c.N, c.K, c.NS) for c in R.merge_probe_cases(form)} == set(R.MERGE_PROBE[form])
    assert all(N % 4 == 1 for N, _ in R.MERGE_SHAPES["mrg4"]) and max(K for _, K in R.MERGE_SHAPES["mrg4"]) == 16384
    assert max(c.N * c.ldw for c in cases) == 4096 * 8200


def _merge32(d, order):
    """the merge in float32, by hand: "split": one split after the other; "four": groups of four ((a0 w0 + a1 w1) + (a2 w2 + a3 w3))
    and a tail -> (x [K] float32, the weights e [H][NS])"""
    pm, pl, po = d.pm, d.pl, d.po
    NS = pm.shape[1]
    e = torch.exp(pm - pm.max(-1, keepdim=True).values)
    assert e.dtype == R.F32
    o, l = torch.zeros(po.shape[0], 128), torch.zeros(po.shape[0])
    t = lambda s: po[:, s] * e[:, s, None]
    s = 0
    while order == "four" and s + 4 <= NS:
        o, l = o + ((t(s) + t(s + 1)) + (t(s + 2) + t(s + 3))), l + ((pl[:, s] * e[:, s] + pl[:, s + 1] * e[:, s + 1]) + (pl[:, s + 2] * e[:, s + 2] + pl[:, s + 3] * e[:, s + 3]))
        s += 4
    for s in range(s, NS):
        o, l = o + t(s), l + pl[:, s] * e[:, s]
    return (o * (1.0 / l)[:, None]).reshape(-1), e


@pytest.mark.parametrize("form", R.MERGE_FORMS)
def test_merge_case_conditions(form):
    """every case builds with its guards.  Exact family: the merged x is the integer x bit for bit in float32 in two orders of
    summation and in fp64, dead weights are exactly 0 in float32, all magnitudes sum below 2^24, and live counts, places, 2^j and both
    kinds of dead split vary between heads.  Probe family: |pm - max| <= 16, one dead split per head, B below half a bf16 ulp on
    >= 98 % of the elements, and a plain float32 evaluation is inside the bound"""
    nan = lambda t: bool(torch.isnan(t).all())
    for c in [c for c in R.merge_cases() if c.inst == R.MERGE_INST[form] and (c.merge == "cmb") == (form == "cmb")]:
        d = R.build(c)
        H, NS, K = c.K // 128, c.NS, c.K
        assert d.x.shape == (K,) and nan(d.x) and d.pm.shape == (H, NS) == d.pl.shape and d.po.shape == (H, NS, 128)
        for buf, t, pad in ((d.pm_buf, d.pm, R.PAD), (d.pl_buf, d.pl, R.PAD), (d.po_buf, d.po, 128)):
            assert buf.dtype == R.F32 and buf.numel() == t.numel() + pad and nan(buf[t.numel():]) and torch.equal(R.bits(buf[:t.numel()]), R.bits(t.reshape(-1)))
        Wb = d.W.view(c.N + 1, c.ldw)
        assert c.ldw == K + 8 and nan(Wb[:, K:]) and nan(Wb[c.N])
        if c.res:
            rb = d.res.view(2, c.res_bs)
            assert nan(rb[:, c.nout:]) and nan(rb[1])
        assert bool(torch.isfinite(d.po).all()) and bool(d.live.any(-1).all())
        x64, B = R.merge_ref(c, d)
        e = R.expected(c, d, rbf=False)
        if c.mfam == "exact":
            xi = d.xl[0]
            assert torch.equal(x64, xi) and bool((xi == xi.round()).all()) and torch.equal(R.x_prime(c, d)[0][0], xi), c.name
            for order in ("split", "four"):
                x32, w = _merge32(d, order)
                assert torch.equal(R.bits(x32), R.bits(xi.float())), (c.name, order)
            assert bool((w[~d.live] == 0).all()) and bool((w[d.live] == 1).all()) and bool((d.po[~d.live].abs() == R.MRG_DEAD_PO).all())
            live = d.live.double()
            assert float((d.po.double().abs() * live[..., None]).sum(1).max()) < 2.0 ** 20 and float((d.pl.double() * live).sum(-1).max()) <= 2.0 ** 9
            lsum = (d.pl.double() * live).sum(-1)
            assert bool((torch.log2(lsum) == torch.log2(lsum).round()).all()) and bool((d.pl[d.live] >= 1).all())
            assert torch.equal(e["y"].vals[e["y"].owned], (R.ref_acc(d, d.xl) + (d.rl if c.res else 0.0)).reshape(-1)), c.name
            assert d.acc_max + (float(d.rl.abs().max()) if c.res else 0.0) < 2.0 ** 24
            marker, far = ~d.live & (d.pm == R.MRG_DEAD_PM) & (d.pl == 0), ~d.live & (d.pm > -1e3) & (d.pl > 0)
            assert bool((marker | far | d.live).all()) and (NS < 3 or H < 2 or (bool(marker.any()) and bool(far.any()))), c.name
            if H >= 4 and NS >= 7:
                L = d.live.sum(-1)
                assert int(L.max()) == NS and int(L.min()) == 1 and lsum.unique().numel() >= 3 and L.unique().numel() >= 3
                assert len({tuple(r.tolist()) for r in d.live[L < NS]}) >= min(4, int((L < NS).sum()) // 2), c.name     # places of their own
        else:
            dead = ~d.live
            assert bool((dead.sum(-1) == 1).all()) and bool((d.pm[dead] == R.MRG_DEAD_PM).all()) and bool((d.pl[dead] == 0).all()) and bool((d.pl[d.live] > 0).all())
            pmd = d.pm.double()
            gap = torch.where(d.live, pmd.max(-1, keepdim=True).values - pmd, torch.zeros((), dtype=R.F64))
            assert 0 <= float(gap.min()) and 15.99 < float(gap.max()) <= 16.0 and e["y"].owned.sum() == c.N
            k = d.kpos
            ref, Bk = x64[k], B[k]
            h = R.bf16_ulp(ref) / 2
            share = float((Bk < h).double().mean())
            x32 = _merge32(d, "split")[0].double()[k]
            ratio = float(((x32 - ref).abs() / Bk).max())
            print(f"[gemv] {c.name}: B < half an ulp on {100 * share:.2f} % of the elements, largest B {float((Bk / h).max()):.2f} half ulps; float32 on the CPU: {ratio:.3f} B")
            assert share >= 0.98 and ratio <= 1.0, c.name
            assert torch.equal(e["y"].vals[e["y"].owned], R.rbf64(ref)), c.name
            pos = set(k.tolist())
            want = set(range(K)) if c.N >= K else {0, 1, 2, 3, 127, 128, K - 128, K - 4, K - 3, K - 2, K - 1} | set(range(4 * c.threads() - 4, 4 * c.threads() + 4))
            assert want <= pos and len(pos) == min(c.N, K), c.name


def test_merge_refusals():
    """what usdm_gemv refuses before any launch with the mrg_* partials and with cmb_gran, by return code and message.  Where there
    is a GPU every address is a real buffer that holds the launch and *skip is non-zero, should a refusal ever get lost"""
    import ctypes
    from usdm_amd import _lib
    pool = torch.ones(1 << 21, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
    p = 8 if pool is None else pool.data_ptr()

    def refused(match, **kw):
        a = dict(W=p, x=p, N=8, K=128, ldw=128, y32=p, skip=p, mrg_pm=p, mrg_pl=p, mrg_po=p, mrg_ns=2)
        a.update(kw)
        rc = _lib.lib.usdm_gemv(ctypes.byref(_lib.GemvArgs(**a)), ctypes.c_void_p(0))
        msg = _lib.lib.usdm_last_error().decode()
        assert rc == 2 and match in msg, (kw, rc, msg)

    mrg, plain, cmb = "merged-attention input needs", "are for plain projections", "cmb_gran needs"
    for kw in (dict(mrg_ns=0), dict(mrg_ns=65), dict(K=136, ldw=136), dict(norm_w=p), dict(x_delta=p), dict(mrg_pm=0), dict(mrg_pl=0)):
        refused(mrg, **kw)
    refused(plain, act=R.ACT_SWIGLU, N=32)
    refused(plain, part_val=p, part_idx=p)
    hand = dict(N=4096, cmb_gran=p, cmb_err=p)
    for kw in (dict(N=37), dict(N=4080), dict(N=8192), dict(p2p=p, p2p_mode=1, residual=p, y16=p), dict(mrg_po=0), dict(act=R.ACT_SWIGLU, N=8192), dict(part_val=p, part_idx=p)):
        refused(cmb, **dict(hand, **kw))
    for kw in (dict(mrg_pm=0), dict(mrg_pl=0), dict(mrg_ns=0), dict(mrg_ns=65), dict(norm_w=p), dict(x_delta=p)):
        refused(mrg, **dict(hand, **kw))
