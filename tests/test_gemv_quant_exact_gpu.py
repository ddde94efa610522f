"""The quantized decode GEMVs against the exact references of tests/_gemv_reference.py: usdm_gemv_fp8 and usdm_gemv_mxfp4 in all nine
(rows per wave, GLU, waves) instantiations (FP8: and lm_head mode) over the K ladder of the format's own ring, their VALU batch forms
(2 ... 4 items), and usdm_gemv_fp8_mfma in every variant, tile height and mode.  The logical weights of a case are bf16 values that
quantize losslessly (tests/test_gemv_exact_cpu.py), scaled so that neighbouring rows (FP8) and blocks (MXFP4) carry different scales:
the fp64 reference of the bf16 kernels is the exact reference of these kernels too.  Run, run_case and every assertion are those of
tests/test_gemv_exact_gpu.py: integer cases compare bit patterns in both round_bf16 settings, e4m3 NaN bytes fill the gaps of the FP8
weights, NaN every other operand gap, the sentinel surrounds every output.  usdm_gemv_mxfp4 has no y32: its y16 must hold the single
bf16 rounding of the exact sum without round_bf16, the reference's two roundings with it.  SwiGLU and probe cases, for which the
reference is a bound, must in addition equal the bf16 entry point on the same weights bit for bit.

Measured on an MI355X: SwiGLU without round_bf16 reaches at most 0.24 of its bound (4 x torch's float32 error) and differs from the
fp64 reference with HF's rounding points on none of its outputs with round_bf16; of the RMSNorm probe's elements at most 1.35 % of a
case equal only the reference at rstd (1 + DELTA).  The slowest id takes 2.2 s (MXFP4, the 7-wave GLU tuple: 14336 x 4128 weights
and its bf16 twin), its bf16 counterpart 0.9 s; the weights are quantized once per case, on the device.

A break tried locally (never committed): without the redirect of the ragged last iteration in the FP8 refill of gemv_kernel,
"fp8 rw1-4waves plain K8200" reads NaN; with the scale dword of the group before for a partial last MXFP4 group in the refill,
"mxfp4 rw1-4waves plain K8224" differs on 24 of 37 outputs.  tests/test_fp8_gpu.py and tests/test_mxfp4_gpu.py pass with both."""
import pytest

from tests import _gemv_reference as R
from tests.test_gemv_exact_gpu import _run_all

pytestmark = pytest.mark.gpu

FMT_INSTS = [(f, i) for f in R.FMTS for i in R.quant_insts(f)]
FMT_SKIP = [(f, i) for f in R.FMTS for i in R.DELTA_INST]
FMT_BATCH = [(f, nb, i) for f in R.FMTS for nb in R.VALU_NB for i in R.quant_batch_insts(f)]
_id = lambda p: "-".join(str(v) if isinstance(v, (int, str)) and v != "lm" else R.inst_id(v) for v in p)


@pytest.mark.parametrize("fmt,inst", FMT_INSTS, ids=[_id(p) for p in FMT_INSTS])
def test_gemv_quant_plain(dev, fmt, inst):
    """integer operands over the K ladder of the format's ring (FP8: 16 / 16 / 10 / 8 iterations; MXFP4: 4 / 2 groups of four): below, at
    and above one iteration, one group, one ring and the workgroup's first pass over x; a refill with a ragged last iteration (FP8: the
    redirect to the row start) or a partial last group (MXFP4) in every instantiation"""
    _run_all(R.valu_plain_cases(inst, fmt=fmt), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("fmt,inst", FMT_INSTS, ids=[_id(p) for p in FMT_INSTS])
def test_gemv_quant_norm_exact(dev, fmt, inst):
    """fused RMSNorm on x = +-2: x' = +-norm_w exactly, so the projection after the norm is an integer case"""
    _run_all(R.valu_norm_exact_cases(inst, fmt=fmt), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("fmt,inst", FMT_INSTS, ids=[_id(p) for p in FMT_INSTS])
def test_gemv_quant_norm_probe(dev, fmt, inst):
    """fused RMSNorm read back through unit-vector rows at the first ragged K and just past 8 x threads"""
    _run_all(R.valu_probe_cases(inst, fmt=fmt), dev, "share of the (1 + DELTA) reference")


def test_gemv_fp8_lm_head_bans(dev):
    """no ban array, a banned workgroup, a banned wave in a live workgroup, scattered bans, the last row; idx_offset != 0"""
    _run_all(R.lm_head_cases(fmt="fp8"), dev, "")


@pytest.mark.parametrize("fmt,inst", FMT_SKIP, ids=[_id(p) for p in FMT_SKIP])
def test_gemv_quant_skip(dev, fmt, inst):
    """*skip = 1: no output is touched"""
    _run_all(R.skip_cases(inst, fmt), dev, "")


@pytest.mark.parametrize("fmt,nb,inst", FMT_BATCH, ids=[_id(p) for p in FMT_BATCH])
def test_gemv_quant_batch_valu(dev, fmt, nb, inst):
    """the VALU batch form (form -1): every item against its own reference (different data per item, strided with NaN between)"""
    _run_all(R.valu_plain_cases(inst, nb, fmt) + R.valu_norm_exact_cases(inst, nb, fmt), dev, "SwiGLU error / bound")
    _run_all(R.valu_probe_cases(inst, nb, fmt), dev, "share of the (1 + DELTA) reference")


@pytest.mark.parametrize("nb", R.VALU_NB)
def test_gemv_fp8_batch_valu_lm_head_bans(dev, nb):
    _run_all(R.lm_head_cases(nb, fmt="fp8"), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_fp8_matrix_cores(dev, nb):
    """N = 37 over every variant of usdm_gemv_fp8_mfma: held and streamed activations, the re-cut loads at K = 4096 and 14336, K split in
    3, 7 and 8 slices (counters back at zero, the same bits on the same scratch); plain + residual, in place in the round_bf16 launch"""
    _run_all(R.mfma_ladder_cases(nb, "fp8"), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_fp8_matrix_cores_tile_rows(dev, nb):
    """12-row tiles (N = 6144) and ragged 16-row tiles (N = 4085) on forms 0 and 5; N = 37 above runs 8-row tiles"""
    _run_all(R.mfma_tile_cases(nb, "fp8"), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_fp8_matrix_cores_swiglu(dev, nb):
    _run_all(R.mfma_swiglu_cases(nb, "fp8"), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_fp8_matrix_cores_norm(dev, nb):
    """both RMSNorm families on the held activations (K <= 4096); the probe covers all of K at K = 4096"""
    cases = R.mfma_norm_cases(nb, "fp8")
    _run_all([c for c in cases if c.kind != "probe"], dev, "SwiGLU error / bound")
    _run_all([c for c in cases if c.kind == "probe"], dev, "share of the (1 + DELTA) reference")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_fp8_matrix_cores_lm_head(dev, nb):
    """N = 1003 with all five ban patterns (no ban array among them): one partial per workgroup, the rest of part_bs reads "no candidate" """
    _run_all(R.lm_head_cases(nb, mfma=True, fmt="fp8"), dev, "")
