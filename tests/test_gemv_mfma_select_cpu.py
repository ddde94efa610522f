"""CPU: usdm_gemv_mfma_select - the matrix-core launcher's own selection, asked on the host - against the mirror the exact GPU tests
build their cases from (tests/_gemv_reference.py:mfma_select), field by field, over a grid that reaches every variant of every format;
the shapes the launcher refuses are refused with its messages; USDMForCausalLM.max_batch() gives the launcher's answer."""
import itertools
import re

import pytest

from tests import _gemv_reference as R
from usdm_amd import _lib, ops

KS = (256, 512, 1792, 3840, 4096, 6144, 14336, 16384)
NS = (16, 37, 200, 1003, 4096, 6144, 28672, 42003)
MODES = (dict(), dict(glu=True), dict(norm=True), dict(lm_head=True))
FORMS = {"bf16": (1, 3, 5), "fp8": (0, 5), "mxfp4": (0, 5)}
# (hold, cpwt, trl) of the kernel instantiation behind each variant name of the mirror, per format (MXFP4: its image is cut into
# fragments already - no re-cut through LDS, and K = 14336 streams on the generic form)
INSTANTIATION = {
    "bf16": {"hold": (1, 0, 0), "hold16-recut": (1, 16, 1), "hold16-frag": (1, 16, 0), "stream": (0, 0, 0), "stream56-recut": (0, 56, 1),
             "stream56-frag": (0, 56, 0), "ksplit": (1, 8, 1)},
    "fp8": {"hold": (1, 0, 0), "hold16-recut": (1, 16, 1), "stream": (0, 0, 0), "stream56-recut": (0, 56, 1), "ksplit": (1, 8, 1)},
    "mxfp4": {"hold": (1, 0, 0), "hold16-recut": (1, 16, 0), "stream": (0, 0, 0), "stream56-recut": (0, 0, 0), "ksplit": (1, 8, 0)},
}
LDS_DEF = 16 * 8 * 1024 + 4096 * 4 + 8 * 16 * 4 + 64 * 4 + 2 * 16 * 16 * 4      # reduction group of 16 tiles + gam, ssum, tl, sv, si
LDS_TRL = 8 * 8 * 1024 + (LDS_DEF - 16 * 8 * 1024) + 8 * 8192                   # group of 8 + a transposition buffer per wave


def refusal(N, K, glu=False, norm=False, lm_head=False):
    """the launcher's message for a shape it refuses (its checks in its order), or None"""
    if K % 256:
        return "K % 256"
    if norm and K > 4096:
        return "the fused RMSNorm needs K <= 4096"
    if glu and N % 32:
        return "swiglu needs N % 32 == 0"
    return None


def test_select_equals_the_mirror_over_every_variant_of_every_format():
    reached = {f: set() for f in FORMS}
    for fmt, forms in FORMS.items():
        for K, N, mode, form, ks in itertools.product(KS, NS, MODES, forms, (False, True)):
            why = refusal(N, K, **mode)
            if why:
                with pytest.raises(_lib.UsdmError, match=re.escape(why)):
                    ops.gemv_mfma_select(N, K, form=form, fmt=fmt, ks=ks, **mode)
                continue
            p = ops.gemv_mfma_select(N, K, form=form, fmt=fmt, ks=ks, **mode)
            want = R.mfma_select(N, K, form=form, ks=ks, **mode)
            what = (fmt, N, K, mode, form, ks)
            assert (p["hold"], p["cpwt"], p["trl"]) == INSTANTIATION[fmt][want["variant"]], what
            for key in ("rt", "ksplit", "ntiles", "grid", "kwg"):
                assert p[key] == want[key], (what, key)
            assert p["nout"] == (N // 2 if mode.get("glu") else N) and p["cpw"] == (8 if p["ksplit"] > 1 else K // 256), what
            assert p["lds_bytes"] == (LDS_TRL if p["trl"] else LDS_DEF) <= 160 * 1024, what
            reached[fmt].add(want["variant"])
    assert reached["bf16"] == set(R.MFMA_VARIANTS)
    assert reached["fp8"] == reached["mxfp4"] == set(R.FP8_MFMA_VARIANTS)


@pytest.mark.parametrize("fmt", sorted(FORMS))
def test_refused_shapes_carry_the_launchers_messages(fmt):
    f = FORMS[fmt][0]
    for kw, msg in ((dict(N=4096, K=1000), r"usdm_gemv_mfma_select \(matrix-core form\): K % 256, ldw % 8, x stride % 8"),
                    (dict(N=4096, K=128), r"K % 256"),
                    (dict(N=4096, K=6144, norm=True), r"usdm_gemv_mfma_select \(matrix-core form\): the fused RMSNorm needs K <= 4096"),
                    (dict(N=48, K=4096, glu=True), r"swiglu needs N % 32 == 0 \(packed gate/up rows\)"),
                    (dict(N=16 * 64 * 256 + 1, K=256, lm_head=True), r"N too large \(more than 64 tiles per workgroup\)"),
                    (dict(N=16 * 64 * 256 + 1, K=4096), r"N too large \(more than 64 tiles per workgroup\)")):
        with pytest.raises(_lib.UsdmError, match=msg):
            ops.gemv_mfma_select(form=f, fmt=fmt, **kw)
    assert ops.gemv_mfma_select(16 * 64 * 256, 256, lm_head=True, form=f, fmt=fmt)["ntiles"] == 64 * 256      # the bound itself is taken


def _stub(hidden, inter, quantization=None, matrix_cores=False, vocab=42003, heads=32, kv_heads=8):
    from usdm_amd.llm import USDMForCausalLM
    m = object.__new__(USDMForCausalLM)
    m.cfg = dict(hidden_size=hidden, head_dim=128, num_hidden_layers=1)
    m.Hq, m.Hkv, m.I, m.v0, m.v1 = heads, kv_heads, inter, 0, vocab
    m.quantization = quantization
    m.fp8_matrix_cores = matrix_cores and quantization == "fp8"
    m.mxfp4_matrix_cores = matrix_cores and quantization == "mxfp4"
    return m


def _max_batch_before(m):
    """max_batch() of the quantized formats as it stood before it asked the launcher"""
    ks = (m.cfg["hidden_size"], m.Hq * m.cfg["head_dim"], m.I)
    if not (m.fp8_matrix_cores or m.mxfp4_matrix_cores):
        return 4
    return 16 if all(k % 256 == 0 for k in ks) and m.cfg["hidden_size"] <= 4096 and -(-(m.v1 - m.v0) // 16) <= 64 * 256 else 4


def test_max_batch_is_the_launchers_answer():
    assert _stub(4096, 14336).max_batch() == 16
    assert _stub(5120, 13824, heads=40, kv_heads=40).max_batch() == 4        # the fused RMSNorm holds K <= 4096: was 16, then failed in plan build
    assert _stub(4096, 14336 + 128).max_batch() == 4                          # K % 256
    assert _stub(2048, 5632, heads=16, kv_heads=16).max_batch() == 16
    for q in ("fp8", "mxfp4"):
        for mc in (False, True):
            for cfg in (dict(hidden=4096, inter=14336), dict(hidden=5120, inter=13824, heads=40, kv_heads=40), dict(hidden=4096, inter=14336 + 128),
                        dict(hidden=2048, inter=5632, heads=16, kv_heads=16), dict(hidden=4096, inter=14336, vocab=16 * 64 * 256 + 1),
                        dict(hidden=4096, inter=14336, vocab=16 * 64 * 256), dict(hidden=4096, inter=14336, heads=31, kv_heads=8)):
                m = _stub(quantization=q, matrix_cores=mc, **cfg)
                assert m.max_batch() == _max_batch_before(m), (q, mc, cfg)
    assert _stub(4096, 14336, "fp8", True).max_batch() == _stub(4096, 14336, "mxfp4", True).max_batch() == 16
