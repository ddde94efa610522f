"""CPU: the matrix-core image of an MXFP4 matrix (quant.Mxfp4Weight with matrix_cores=True, read by usdm_gemv_mxfp4_mfma) and the
`mxfp4_matrix_cores` flag's refusals that need no device.  The image is a second layout of the SAME logical codes and scales: both
images must unpack to what quantize_mxfp4 produced, and one row is checked against the index formula written out by hand."""
import pytest
import torch

from usdm_amd.quant import MX_GROUP, Mxfp4Weight, quantize_mxfp4

SHAPES = [(16, 256), (37, 512), (5, 1792), (19, 4096), (3, 14336), (1003, 512)]      # N is no multiple of 16 in all but the first


def _matrix(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    w *= torch.exp2(torch.randint(-12, 13, (N, K // 32), generator=g).float()).repeat_interleave(32, dim=1)
    w[torch.rand(N, K, generator=g) < 0.05] = 0.0
    return w.to(torch.bfloat16)


@pytest.mark.parametrize("N,K", SHAPES)
def test_both_images_unpack_to_the_same_codes_and_scales(N, K):
    w = _matrix(N, K, N + K)
    codes, scales = quantize_mxfp4(w)
    W = Mxfp4Weight.from_matrix(w, matrix_cores=True)
    assert W.has_matrix_core_image and W.mq.shape == (N, K // 2) and W.ms.shape == (N, K // 32)      # no padding to groups of 2048
    assert W.q.shape == (N, -(-K // MX_GROUP) * MX_GROUP // 2)
    for mc in (False, True):
        c, s = W.unpack(matrix_cores=mc)
        assert torch.equal(c, codes) and torch.equal(s, scales), mc
    assert torch.equal(W.ms, scales)                                  # plain [N][K / 32] scale bytes
    assert W.nbytes_matrix_cores == N * (K // 2 + K // 32)
    # built later from the first image: the same bytes; and the first image does not depend on the second
    plain = Mxfp4Weight.from_matrix(w)
    assert not plain.has_matrix_core_image and plain.nbytes_matrix_cores == 0
    assert torch.equal(plain.q, W.q) and torch.equal(plain.s, W.s)
    with pytest.raises(ValueError):
        plain.unpack(matrix_cores=True)
    later = plain.with_matrix_core_image()
    assert later is plain and torch.equal(plain.mq, W.mq) and torch.equal(plain.ms, W.ms)
    assert torch.equal(W.dequantize(), plain.dequantize())


def test_index_formula_by_hand_on_one_row():
    """element 128 Q + 32 j + 8 g + e sits in nibble e of dword j of 16-byte piece g of quad Q; the dword at byte 4 Q of the scale row
    holds the four scales of quad Q"""
    N, K, r = 7, 1792, 5
    w = _matrix(N, K, 99)
    codes, scales = quantize_mxfp4(w)
    W = Mxfp4Weight.from_matrix(w, matrix_cores=True)
    row = W.mq[r].tolist()
    seen = 0
    for Q in range(K // 128):
        for g in range(4):
            for j in range(4):
                dword = int.from_bytes(bytes(row[64 * Q + 16 * g + 4 * j: 64 * Q + 16 * g + 4 * j + 4]), "little")
                for e in range(8):
                    assert (dword >> (4 * e)) & 15 == int(codes[r, 128 * Q + 32 * j + 8 * g + e]), (Q, g, j, e)
                    seen += 1
        sd = int.from_bytes(bytes(W.ms[r, 4 * Q:4 * Q + 4].tolist()), "little")
        for j in range(4):
            assert (sd >> (8 * j)) & 255 == int(scales[r, 4 * Q + j]), (Q, j)
    assert seen == K
    assert len(set(codes[r].tolist())) > 8 and len(set(scales[r].tolist())) > 4      # (the row is not trivially uniform)


def test_image_needs_whole_quads():
    w = _matrix(4, 96, 1)
    Mxfp4Weight.from_matrix(w)                       # the first image takes any K % 32
    with pytest.raises(ValueError):
        Mxfp4Weight.from_matrix(w, matrix_cores=True)
    with pytest.raises(ValueError):
        Mxfp4Weight.from_matrix(w).with_matrix_core_image()


def test_gemv_mxfp4_mfma_takes_only_a_weight_with_the_image():
    from usdm_amd import ops
    w = _matrix(16, 256, 2)
    x = torch.zeros(8, 256, dtype=torch.bfloat16)
    for W in (Mxfp4Weight.from_matrix(w), w, None):
        with pytest.raises(TypeError):
            ops.gemv_mxfp4_mfma(W, x, nb=8, N=16, K=256, x_bs=256, y_bs=16, y16=torch.zeros(8, 16, dtype=torch.bfloat16))


def test_shard_weights_builds_the_image_only_when_asked():
    from usdm_amd.llm import shard_weights
    from usdm_amd.quant import Fp8Weight
    H, I = 256, 512
    g = torch.Generator().manual_seed(3)
    cfg = dict(vocab_size=40, hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
               head_dim=128, rms_norm_eps=1e-5)
    p = "model.layers.0."
    shapes = {"model.embed_tokens.weight": (40, H), "lm_head.weight": (40, H), p + "self_attn.q_proj.weight": (256, H),
              p + "self_attn.k_proj.weight": (128, H), p + "self_attn.v_proj.weight": (128, H), p + "self_attn.o_proj.weight": (H, 256),
              p + "mlp.gate_proj.weight": (I, H), p + "mlp.up_proj.weight": (I, H), p + "mlp.down_proj.weight": (H, I)}
    sd = {k: torch.randn(*v, generator=g) for k, v in shapes.items()}
    sd.update({"model.norm.weight": torch.ones(H), p + "input_layernorm.weight": torch.ones(H), p + "post_attention_layernorm.weight": torch.ones(H)})
    a = shard_weights(lambda n: sd[n], cfg, 0, 1, "cpu", quantization="mxfp4")
    b = shard_weights(lambda n: sd[n], cfg, 0, 1, "cpu", quantization="mxfp4", mxfp4_matrix_cores=True)
    for k in ("qkv", "o", "gu", "down"):
        wa, wb = a["layers"][0][k], b["layers"][0][k]
        assert not wa.has_matrix_core_image and wb.has_matrix_core_image
        assert torch.equal(wa.q, wb.q) and torch.equal(wa.s, wb.s)
        ca, cb = wa.unpack(), wb.unpack(matrix_cores=True)
        assert torch.equal(ca[0], cb[0]) and torch.equal(ca[1], cb[1])
    assert isinstance(b["lm_head"], Fp8Weight)


def test_flag_refusals_before_any_gpu_work():
    from usdm_amd.llm import USDMForCausalLM, check_quantization
    from usdm_amd.serving import LLM
    cfg = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
    check_quantization("mxfp4", False, True)
    check_quantization("mxfp4", False)                  # (the two-argument call of before)
    for q in (None, "fp8"):
        with pytest.raises(ValueError):
            check_quantization(q, False, True)
        with pytest.raises(ValueError):
            USDMForCausalLM(cfg, "cuda", quantization=q, mxfp4_matrix_cores=True)
        with pytest.raises(ValueError):
            LLM(model="naver-ai/USDM-DailyTalk", quantization=q, mxfp4_matrix_cores=True)
    with pytest.raises(ValueError):                     # fp8_matrix_cores with mxfp4 stays the error it is, with or without the new flag
        check_quantization("mxfp4", True, True)
    with pytest.raises(ValueError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", fp8_matrix_cores=True, mxfp4_matrix_cores=True)
    with pytest.raises(NotImplementedError):            # tensor parallelism stays refused
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", mxfp4_matrix_cores=True, tp_size=2, tp_rank=0)
    with pytest.raises(NotImplementedError):
        USDMForCausalLM(cfg, "cuda", quantization="mxfp4", mxfp4_matrix_cores=True, tp_segments=True)
