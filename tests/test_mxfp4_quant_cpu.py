"""CPU: the weight-only MXFP4 format (quantization="mxfp4", usdm_amd/quant.py): OCP e2m1 elements with one power-of-two scale per
block of 32 consecutive K elements.  The format is fixed by hand-made blocks (scale rule, rounding ties, clamps), by its invariants
(every W' is a bf16 value, quantization is idempotent), by the pack / unpack round trip of the kernels' private layout, by what the
loader builds, by the rejections that need no GPU, and by the asm audit of the new GEMV instantiations' hand-counted loads."""
import importlib.util
import os
import shutil
import subprocess

import pytest
import torch

from usdm_amd.quant import E2M1_VALUES, Fp8Weight, Mxfp4Weight, dequantize_mxfp4, dequantize_rows, quantize_mxfp4, quantize_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf = torch.bfloat16


def _block(vals):
    """one row of one block: the given values, then zeros"""
    w = torch.zeros(1, 32, dtype=torch.float64)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    return w.float()


def _q(vals):
    c, s = quantize_mxfp4(_block(vals))
    return c[0, :len(vals)].tolist(), int(s[0, 0]) - 127


@pytest.mark.parametrize("k", [-100, -3, 0, 5, 90])
def test_scale_rule_on_hand_made_blocks(k):
    p = 2.0 ** k
    assert _q([p]) == ([6], k - 2)                                  # amax = 2^k -> 4 * 2^(k-2) (code 6 is 4.0)
    assert _q([1.5 * p]) == ([7], k - 2)                            # 1.5 * 2^k -> 6 * 2^(k-2)
    assert _q([6 * p]) == ([7], k)                                  # 6 * 2^k: floor(log2) = k + 2
    codes, s = _q([7.96875 * p, -7.5 * p, 5.0 * p, 1.0 * p])        # just under 8 * 2^k: the scale stays 2^k, the value saturates to 6
    assert (codes, s) == ([7, 15, 6, 2], k)
    assert _q([-p, p / 2, p / 4, p / 8, p / 16]) == ([14, 4, 2, 1, 0], k - 2)   # -4, 2, 1, 0.5 and 0.25 -> 0 (tie to even)


def test_zero_block_clamps_and_subnormals():
    c, s = quantize_mxfp4(torch.zeros(2, 64))
    assert (c == 0).all() and (s == 127).all()                      # all-zero block: s = 0
    # upper end: the largest bf16 magnitudes give s = 125 (6 * 2^125 is finite in bf16)
    big = torch.tensor([3.0e38]).to(bf).float().item()
    codes, s = _q([big, -big / 2])
    assert s == 125 and codes[0] in (6, 7) and codes[1] >= 8
    # lower clamp: amax = 3 * 2^-126 would give s = -127; clamped to -125 -> 1.5 * 2^-125
    codes, s = _q([3 * 2.0 ** -126, 2.0 ** -126, 2.0 ** -127, -2.0 ** -128])
    assert (codes, s) == ([3, 1, 0, 0], -125)                       # 0.25 (tie) -> 0; the negative one rounds to 0 -> code 0, not 8
    # bf16 subnormal inputs (below 2^-126): the block's values are all below half the smallest code -> zeros at the clamp
    sub = torch.tensor([[2.0 ** -130, -2.0 ** -133] + [0.0] * 30]).to(bf)
    assert sub[0, 0] != 0
    c, s = quantize_mxfp4(sub)
    assert (c == 0).all() and int(s[0, 0]) == 127 - 125
    d = dequantize_mxfp4(c, s)
    assert (d == 0).all() and not torch.signbit(d.float()).any()
    # the bytes that never occur
    w = torch.randn(64, 256, generator=torch.Generator().manual_seed(1)) * torch.logspace(-40, 38, 64)[:, None]
    s = quantize_mxfp4(w.to(bf))[1]
    assert not any(int(b) in (0, 1, 253, 254, 255) for b in s.unique())


def test_rounding_ties_go_to_the_even_code_and_no_negative_zero():
    # amax 4 -> s = 0, so the values below are the scaled values themselves
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    c, s = quantize_mxfp4(_block([4.0] + ties + [-t for t in ties]))
    assert int(s[0, 0]) == 127
    got = dequantize_mxfp4(c, s)[0, 1:15].float().tolist()
    assert got == want + [-x for x in want]
    assert int(c[0, 8]) == 0                                        # -0.25 -> code 0, not the negative-zero code 8
    # just off the ties
    c, s = quantize_mxfp4(_block([4.0, 0.2501, 0.7499, 1.2501, 1.7499, 2.5001, 3.4999, 5.0001]))
    assert dequantize_mxfp4(c, s)[0, 1:8].float().tolist() == [0.5, 0.5, 1.5, 1.5, 3.0, 3.0, 6.0]
    w = torch.randn(128, 512, generator=torch.Generator().manual_seed(2)).to(bf)
    assert not (quantize_mxfp4(w)[0] == 8).any()
    assert tuple(E2M1_VALUES) == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def test_bad_inputs_raise():
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.tensor([[1.0, float("inf")] * 16]))
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.tensor([[1.0, float("nan")] * 16]))
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, 48))
    with pytest.raises(ValueError):
        Mxfp4Weight.from_matrix(torch.zeros(4, 40))


def _mats():
    g = torch.Generator().manual_seed(3)
    gauss = torch.randn(96, 4096, generator=g) * 4096 ** -0.5
    heavy = torch.distributions.StudentT(4.0).sample((96, 4096)) * 0.02        # (seeded by the call below)
    return {"gauss": gauss.to(bf), "heavy": heavy.to(bf)}


def test_wprime_is_bf16_and_quantization_is_idempotent():
    torch.manual_seed(4)
    for name, w in _mats().items():
        c, s = quantize_mxfp4(w)
        assert c.dtype == torch.uint8 and s.dtype == torch.uint8 and c.shape == w.shape and s.shape == (w.shape[0], w.shape[1] // 32)
        assert int(c.max()) <= 15
        # W' in float64 from the definition, against the bf16 the module returns: the bf16 rounding changed nothing
        tab = torch.tensor(list(E2M1_VALUES) + [-x for x in E2M1_VALUES], dtype=torch.float64)
        w64 = (tab[c.long()].view(w.shape[0], -1, 32) * (2.0 ** (s.double() - 127))[:, :, None]).view(w.shape)
        d = dequantize_mxfp4(c, s)
        assert d.dtype == bf and torch.equal(d.double(), w64), name
        c2, s2 = quantize_mxfp4(d)
        assert torch.equal(c2, c) and torch.equal(s2, s), name
        rel = ((w64 - w.double()).norm() / w.double().norm()).item()
        assert 0.08 < rel < (0.125 if name == "gauss" else 0.15), (name, rel)   # ~0.115 Gaussian, ~0.132 Student-t (4 d.o.f.)
        # element-wise: inside the code range the error is at most half a code step (steps 0.5 / 1 / 2 times the scale)
        sc = (2.0 ** (s.double() - 127))[:, :, None].expand(-1, -1, 32).reshape(w.shape)
        v = w.double().abs() / sc
        step = torch.where(v < 2, 0.5, torch.where(v < 4, 1.0, 2.0))
        inside = v <= 6
        assert ((w64 - w.double()).abs()[inside] <= (0.5 * step * sc)[inside]).all(), name
        assert ((w64.abs() == 6 * sc) | inside).all(), name


@pytest.mark.parametrize("K", [512, 1792, 4096, 14336])
def test_pack_unpack_round_trip_and_nbytes(K):
    N = 13
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(K)) * torch.logspace(-3, 3, N)[:, None]).to(bf)
    c, s = quantize_mxfp4(w)
    W = Mxfp4Weight.from_codes(c, s)
    Kp = -(-K // 2048) * 2048
    assert (W.N, W.K, tuple(W.shape)) == (N, K, (N, K)) and not W.is_cuda
    assert W.q.shape == (N, Kp // 2) and W.s.shape == (N, Kp // 32) and W.nbytes == N * (Kp // 2 + Kp // 32)
    c2, s2 = W.unpack()
    assert torch.equal(c2, c) and torch.equal(s2, s)
    d = W.dequantize()
    assert d.shape == (N, K) and torch.equal(d, dequantize_mxfp4(c, s))             # padding never leaks
    assert torch.equal(Mxfp4Weight.from_matrix(w).q, W.q) and torch.equal(Mxfp4Weight.from_matrix(w).s, W.s)
    # the documented layout, spot-checked: element k of a row sits in group k // 2048, piece (k % 512) // 8, dword (k % 2048) // 512
    for k in (0, 1, 9, 511, K // 2 + 5, K - 1):
        g, i, L, e = k // 2048, (k % 2048) // 512, (k % 512) // 8, k % 8
        byte = int(W.q[3, g * 1024 + L * 16 + i * 4 + e // 2])
        assert (byte >> 4 if e & 1 else byte & 15) == int(c[3, k]), k
        assert int(W.s[3, g * 64 + (L // 4) * 4 + i]) == int(s[3, k // 32]), k
    # padding: zero codes, scale bytes 127
    if Kp != K:
        full = Mxfp4Weight(W.q, W.s, Kp).unpack()
        assert (full[0][:, K:] == 0).all() and (full[1][:, K // 32:] == 127).all()


def test_loader_builds_mxfp4_layers_and_an_fp8_lm_head():
    from usdm_amd.llm import _pack_gate_up, shard_weights
    g = torch.Generator().manual_seed(11)
    H, I = 64, 96
    gate, up = torch.randn(I, H, generator=g).to(bf), (torch.randn(I, H, generator=g) * 3).to(bf)
    dq = lambda t: dequantize_mxfp4(*quantize_mxfp4(t))
    assert torch.equal(dq(_pack_gate_up(gate, up)), _pack_gate_up(dq(gate), dq(up)))
    qm, km, vm = (torch.randn(n, H, generator=g).to(bf) * sc for n, sc in ((64, 1.0), (64, 0.01), (64, 50.0)))
    assert torch.equal(dq(torch.cat([qm, km, vm])), torch.cat([dq(qm), dq(km), dq(vm)]))
    cfg = dict(vocab_size=40, hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1,
               head_dim=64, rms_norm_eps=1e-5)
    sd = {"model.embed_tokens.weight": torch.randn(40, H, generator=g), "lm_head.weight": torch.randn(40, H, generator=g),
          "model.norm.weight": torch.ones(H)}
    p = "model.layers.0."
    sd.update({p + "self_attn.q_proj.weight": qm, p + "self_attn.k_proj.weight": km, p + "self_attn.v_proj.weight": vm,
               p + "self_attn.o_proj.weight": torch.randn(H, 64, generator=g), p + "mlp.gate_proj.weight": gate,
               p + "mlp.up_proj.weight": up, p + "mlp.down_proj.weight": torch.randn(H, I, generator=g),
               p + "input_layernorm.weight": torch.ones(H), p + "post_attention_layernorm.weight": torch.ones(H)})
    W = shard_weights(lambda n: sd[n], cfg, 0, 1, "cpu", quantization="mxfp4")
    L = W["layers"][0]
    assert all(isinstance(L[k], Mxfp4Weight) for k in ("qkv", "o", "gu", "down")) and isinstance(W["lm_head"], Fp8Weight)
    assert W["embed"].dtype == bf and L["ln1"].dtype == torch.float32 and W["norm"].dtype == torch.float32
    assert torch.equal(L["gu"].dequantize(), _pack_gate_up(dq(gate), dq(up)))
    assert torch.equal(L["qkv"].dequantize(), torch.cat([dq(qm), dq(km), dq(vm)]))
    assert torch.equal(L["down"].dequantize(), dq(sd[p + "mlp.down_proj.weight"].to(bf)))
    assert torch.equal(W["lm_head"].dequantize(), dequantize_rows(*quantize_rows(sd["lm_head.weight"].to(bf))))


def test_mxfp4_rejections_before_any_gpu_work():
    from usdm_amd.llm import USDMForCausalLM, check_quantization
    from usdm_amd.serving import LLM
    cfg = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
    check_quantization("mxfp4", False)
    with pytest.raises(ValueError):
        check_quantization("mxfp4", True)
    with pytest.raises(ValueError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", fp8_matrix_cores=True)
    with pytest.raises(ValueError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp6")
    with pytest.raises(NotImplementedError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", tp_size=2, tp_rank=0)
    with pytest.raises(NotImplementedError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", tp_segments=True)
    with pytest.raises(ValueError):
        LLM(model="naver-ai/USDM-DailyTalk", quantization="mxfp4", fp8_matrix_cores=True)
    with pytest.raises(ValueError):
        LLM(model="naver-ai/USDM-DailyTalk", quantization="nvfp4")


# ---- the asm audit of the new instantiations' hand-counted loads (x piece + RMSNorm weights before the ring, one exact wait) -----
def _tool():
    spec = importlib.util.spec_from_file_location("check_mfma_asm", os.path.join(ROOT, "tools", "check_mfma_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from usdm_amd import build
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("hipcc is not installed")
    hipcc = build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")
    out = {}
    for f in ("llm_k", "llm_batch_k"):
        dst = str(tmp_path_factory.mktemp("asm") / (f + ".s"))
        r = subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-S", os.path.join(build.CSRC, f + ".hip"), "-o", dst],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[f] = open(dst).read().split("\n")
    return out


def _mx4_kernels(t, asm):
    """(file, name, first line, end line, holds an asm load) of every MXFP4 instantiation of the two GEMV kernels"""
    out = []
    for f, kern, tag in (("llm_k", "gemv_kernel", "gemv_mx4"), ("llm_batch_k", "gemv_batch_kernel", "gemv_mx4")):
        lines = asm[f]
        for name, i0, i1 in t.kernels(lines, kern):
            if tag in name:
                held = any("ASMSTART" in lines[i] and t.LOAD.search(lines[i + 1].split(";")[0]) for i in range(i0, i1 - 1))
                out.append((f, name, i0, i1, held))
    return out


def test_every_mxfp4_instantiation_with_hand_counted_loads_is_clean(asm):
    t = _tool()
    ks = _mx4_kernels(t, asm)
    # 9 shapes of gemv_kernel (the launcher's variants), 8 shapes x nb = 2, 3, 4 of gemv_batch_kernel
    assert sum(f == "llm_k" for f, *_ in ks) == 9 and sum(f == "llm_batch_k" for f, *_ in ks) == 24, [k[1] for k in ks]
    held = [k for k in ks if k[4]]
    assert len(held) == 9 and all(f == "llm_k" for f, *_ in held)      # gemv_batch_kernel has no hand-counted loads
    for f, name, i0, i1, _ in held:
        nload, bad = t.audit(asm[f], i0, i1)
        assert nload == 3, (name, nload)
        assert not bad, (name, bad[:5])
    # no instantiation spills: the scratch size in the kernel descriptors is zero
    for f, name, i0, i1, _ in ks:
        meta = [l for l in asm[f] if ".private_segment_fixed_size" in l or ".name:" in l]
        i = next(j for j, l in enumerate(meta) if ".name:" in l and l.split()[-1] == name)
        near = [l for l in meta[max(0, i - 3):i + 4] if ".private_segment_fixed_size" in l]
        assert near and all(l.split()[-1] == "0" for l in near), (name, near)


def test_audit_catches_a_seeded_violation_in_the_mxfp4_kernels(asm):
    t = _tool()
    held = [k for k in _mx4_kernels(t, asm) if k[4]]
    assert held
    for f, name, i0, i1, _ in held:
        lines = list(asm[f])
        j = next(i for i in range(i0, i1) if "ASMSTART" in lines[i] and t.LOAD.search(lines[i + 1].split(";")[0]))
        dst = t.REG.findall(lines[j + 1].split(";")[0])[0]
        r0 = min(t.regs(dst))
        end = next(i for i in range(j, i1) if "ASMEND" in lines[i])
        lines.insert(end + 1, f"\tv_mov_b32_e32 v255, v{r0}")
        _, bad = t.audit(lines, i0, i1 + 1)
        assert bad and bad[0][1] == f"v_mov_b32_e32 v255, v{r0}", name
