"""Weight-only FP8 (opt-in, `quantization="fp8"`): OCP e4m3fn weights with one power-of-two scale per output row.

Row r of a [N][K] matrix is stored as
    e[r]    int8: the smallest integer with max_k |w[r,k]| / 2^e[r] <= 448, clamped to [EXP_MIN, EXP_MAX] (see below);
            an all-zero row gets 0;
    q[r,k]  uint8: the e4m3fn byte of w[r,k] / 2^e[r], rounded to nearest even (OCP e4m3fn, not the fnuz encoding).
The dequantized weight W'[r,k] = e4m3(q[r,k]) * 2^e[r] has at most 4 significant bits and, with e clamped so that the smallest
e4m3 subnormal (2^-9) times 2^e is still a normal bf16 and 448 * 2^e is finite, it is EXACTLY a bf16 value.  An FP8 model is
therefore exactly the bf16 model with weights W': the decode kernels convert q to bf16 in registers (exact) and run the bf16
arithmetic unchanged, and prefill dequantizes into a bf16 scratch for usdm_gemm.

Byte layout (only this module, usdm_dequant_fp8 and the FP8 GEMV kernels know it): q is row-major [N][K] bytes with row stride K
(K a multiple of 8: lane L of the GEMV reads the 8 bytes of the 8 bf16 elements it reads in the bf16 kernel); e is [N].
Quantization runs once, at load time, with torch ops on whatever device the matrix is on; it is deterministic.
"""
import torch

E4M3_MAX = 448.0
EXP_MIN = -117      # 2^-9 * 2^-117 = 2^-126: the smallest nonzero dequantized value is a normal bf16
EXP_MAX = 119       # 448 * 2^119 < the largest finite bf16


def _row_exponents(w32):
    """e[r] for an f32 [N][K] matrix (minimal, clamped)."""
    amax = w32.abs().amax(dim=1)
    nz = amax > 0
    # frexp: amax / 448 = m * 2^x with m in [0.5, 1) -> ceil(log2(amax / 448)) = x - (m == 0.5); then an exact check both ways
    m, x = torch.frexp(torch.where(nz, amax, torch.ones_like(amax)) / E4M3_MAX)
    e = (x - (m == 0.5).to(x.dtype)).to(torch.int32)
    e = torch.where(torch.ldexp(torch.full_like(amax, E4M3_MAX), e.float()) < amax, e + 1, e)
    e = torch.where(torch.ldexp(torch.full_like(amax, E4M3_MAX), (e - 1).float()) >= amax, e - 1, e)
    e = e.clamp(EXP_MIN, EXP_MAX)
    return torch.where(nz, e, torch.zeros_like(e))


def quantize_rows(w):
    """w: [N][K] (bf16 or f32, finite) -> (q uint8 [N][K] e4m3fn bytes, e int8 [N]) on w's device."""
    if w.dim() != 2:
        raise ValueError("quantize_rows takes a [N][K] matrix")
    w32 = w.float()
    if not bool(torch.isfinite(w32).all()):
        raise ValueError("quantize_rows: the matrix holds a non-finite value")
    e = _row_exponents(w32)
    scaled = torch.ldexp(w32, (-e).float()[:, None])        # exact: a power-of-two scaling of a bf16 value
    scaled = scaled.clamp(-E4M3_MAX, E4M3_MAX)               # (only a row clamped at EXP_MAX can exceed 448)
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return q, e.to(torch.int8).contiguous()


def dequantize_rows(q, e):
    """(q uint8 [N][K], e int8 [N]) -> bf16 [N][K] = e4m3(q) * 2^e (exact)."""
    v = q.view(torch.float8_e4m3fn).float()
    return torch.ldexp(v, e.float()[:, None]).to(torch.bfloat16)


# ---- FP8 KV cache (opt-in, kv_cache_dtype="fp8"): the SAME format, one row = the 128 values of one (token, kv head) --------------
# k8 / v8 uint8 [..., ctx_max, 128] with ke / ve int8 [..., ctx_max]: exactly quantize_rows of the bf16 row the bf16 cache would
# hold (K after RoPE, V as it leaves the qkv projection).  Byte 0 with exponent 0 is 0.0, so a zero-initialised cache is a cache
# of zero rows.  The decode kernels (usdm_attn_decode_fp8) and the prefill append (usdm_rope_cache_fp8) write this format on the
# device; these helpers are the one host-side definition that tests and tools share.
def quantize_kv_rows(x):
    """x: [..., D] (bf16 or f32, finite) -> (q uint8 [..., D], e int8 [...]): quantize_rows over the last dimension."""
    q, e = quantize_rows(x.reshape(-1, x.shape[-1]))
    return q.view(x.shape), e.view(x.shape[:-1])


def dequantize_kv_rows(q, e):
    """(q uint8 [..., D], e int8 [...]) -> bf16 [..., D] (exact)."""
    return dequantize_rows(q.reshape(-1, q.shape[-1]), e.reshape(-1)).view(q.shape)


def roundtrip_kv_rows(x):
    """The bf16 rows an FP8 cache returns for the bf16 rows x: dequantize(quantize(x)).  Idempotent in values."""
    return dequantize_kv_rows(*quantize_kv_rows(x)).to(x.dtype)


KV_CACHE_DTYPES = (None, "bf16", "fp8")


def check_kv_cache_dtype(v):
    """Validated kv_cache_dtype -> "bf16" | "fp8" (None = bf16)."""
    if v not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype={v!r}: supported are None / 'bf16' and 'fp8' (e4m3 rows, one power-of-two scale per "
                         "(token, kv head))")
    return v or "bf16"


class Fp8Weight:
    """A quantized matrix as the kernels take it: q uint8 [N][K], e int8 [N].  ops.gemv / ops.gemv_batch dispatch on this type."""
    __slots__ = ("q", "e", "N", "K")

    def __init__(self, q, e):
        if q.dtype != torch.uint8 or e.dtype != torch.int8 or q.dim() != 2 or e.shape != (q.shape[0],) or q.shape[1] % 8:
            raise ValueError("Fp8Weight: q uint8 [N][K] (K a multiple of 8) and e int8 [N]")
        self.q, self.e = q.contiguous(), e.contiguous()
        self.N, self.K = q.shape

    @classmethod
    def from_matrix(cls, w):
        return cls(*quantize_rows(w))

    def dequantize(self):
        return dequantize_rows(self.q, self.e)

    @property
    def is_cuda(self):
        return self.q.is_cuda

    @property
    def shape(self):
        return self.q.shape

    @property
    def nbytes(self):
        """bytes one pass over the matrix streams (e4m3 bytes + row exponents)"""
        return self.q.numel() + self.e.numel()

    def data_ptr(self):
        return self.q.data_ptr()

    def numel(self):
        return self.q.numel()
