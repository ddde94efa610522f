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

Weight-only MXFP4 (opt-in, `quantization="mxfp4"`): OCP MX e2m1 elements with one power-of-two scale per block of 32 consecutive K
elements of a row (quantize_mxfp4 / dequantize_mxfp4 / Mxfp4Weight below).  4.25 bits per weight, and a much coarser grid than fp8:
round-to-nearest MXFP4 has a relative L2 weight error of about 11.5 % on Gaussian rows (fp8 with row scales: 2.7 %).
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


# ---- Weight-only MXFP4 (opt-in, quantization="mxfp4") ---------------------------------------------------------------------------
# Logical format (public; tests and kernels share it).  A [N][K] matrix, K % 32 == 0, is cut into blocks of 32 consecutive K
# elements of one row.
#   scale of a block: s = floor(log2(amax)) - 2 (the OCP MX rule; amax the block's largest magnitude), clamped to
#       [MX_EXP_MIN, MX_EXP_MAX]; an all-zero block gets 0.  Stored as the e8m0 byte s + 127.
#   element: the e2m1 code (bit 3 sign, bits 2:0 index into E2M1_VALUES) of w / 2^s, rounded to nearest, ties to the even code,
#       magnitudes above 6 saturate to 6.  A value that rounds to zero gets code 0 whatever its sign.
#   W'[r][k] = e2m1(code) * 2^s: at most 2 significant bits times a power of two inside the clamp, so exactly a normal bf16 or 0.
# An MXFP4 model is therefore exactly the bf16 model with the weights W'.
# Memory layout (private to Mxfp4Weight, usdm_dequant_mxfp4 and the MXFP4 GEMV kernels; include/usdm_hip.h describes it): nibbles
# and scale bytes are interleaved so that a GEMV lane fetches its codes of four K iterations with one 16-byte load.
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_BLOCK = 32
MX_EXP_MIN = -125     # 0.5 * 2^-125 = 2^-126: the smallest nonzero dequantized value is a normal bf16
MX_EXP_MAX = 125      # 6 * 2^125 < the largest finite bf16
MX_GROUP = 2048       # elements of a row that the packed layout interleaves (four K iterations of 512 of the GEMV)


def quantize_mxfp4(w):
    """w: [N][K] (bf16 or f32, finite), K % 32 == 0 -> (codes uint8 [N][K], one e2m1 code per element; scales uint8 [N][K/32],
    e8m0 bytes) on w's device.  Deterministic: comparisons and integer ops only."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK:
        raise ValueError("quantize_mxfp4 takes a [N][K] matrix with K a multiple of 32")
    w32 = w.float()
    if not bool(torch.isfinite(w32).all()):
        raise ValueError("quantize_mxfp4: the matrix holds a non-finite value")
    N, K = w32.shape
    blk = w32.view(N, K // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(dim=2)
    nz = amax > 0
    _, x = torch.frexp(torch.where(nz, amax, torch.ones_like(amax)))     # amax = m * 2^x, m in [0.5, 1): floor(log2) = x - 1
    e = (x.to(torch.int32) - 3).clamp(MX_EXP_MIN, MX_EXP_MAX)
    e = torch.where(nz, e, torch.zeros_like(e))
    v = torch.ldexp(blk.abs(), (-e).float()[:, :, None])                  # exact: a power-of-two scaling
    code = torch.zeros(blk.shape, dtype=torch.uint8, device=w.device)
    for t, closed in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        code += (v >= t if closed else v > t).to(torch.uint8)             # ties go to the even code
    code |= ((blk < 0) & (code != 0)).to(torch.uint8) << 3                # no negative zero
    return code.view(N, K).contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(codes, scales):
    """(codes uint8 [N][K], scales uint8 [N][K/32]) -> bf16 [N][K] = e2m1(code) * 2^(scale - 127) (exact)."""
    N, K = codes.shape
    lut = torch.tensor(E2M1_VALUES + tuple(-x for x in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    v = lut[codes.long()].view(N, K // MX_BLOCK, MX_BLOCK)
    return torch.ldexp(v, (scales.float() - 127.0)[:, :, None]).view(N, K).to(torch.bfloat16)


MX_QUAD = 128         # elements of a row that the matrix-core image interleaves (four K chunks of 32 of one MFMA wave)


def _mc_swap(byts, N, K):
    """code bytes [N][K / 2]: linear dword 16 Q + 4 j + g (elements 128 Q + 32 j + 8 g ..+7) <-> dword 16 Q + 4 g + j (its own inverse)"""
    return byts.view(N, K // MX_QUAD, 4, 4, 4).permute(0, 1, 3, 2, 4).reshape(N, K // 2)


class Mxfp4Weight:
    """A quantized matrix as the kernels take it: q uint8 [N][Kp / 2] packed codes and s uint8 [N][Kp / 32] scale bytes, Kp = K
    rounded up to whole groups of 2048 (zero codes, scale bytes 127).  ops.gemv / ops.gemv_batch dispatch on this type.
    Only when asked (matrix_cores=True, or with_matrix_core_image()) it also holds a second image of the same logical matrix for
    usdm_gemv_mxfp4_mfma (ops.gemv_mxfp4_mfma), whose waves own contiguous K chunks: mq uint8 [N][K / 2], where 16-byte piece g of
    the quad Q of four chunks holds four dwords, dword j the codes of elements 128 Q + 32 j + 8 g ..+7 (the earlier element in bits
    3:0, as in q), and ms uint8 [N][K / 32], the plain scale bytes.  No padding; K % 128 == 0.  The VALU kernels and
    usdm_dequant_mxfp4 never read it; it costs K / 2 + K / 32 more bytes per row."""
    __slots__ = ("q", "s", "N", "K", "mq", "ms")

    def __init__(self, q, s, K, mq=None, ms=None):
        Kp = -(-K // MX_GROUP) * MX_GROUP
        if q.dtype != torch.uint8 or s.dtype != torch.uint8 or q.dim() != 2 or K % MX_BLOCK or q.shape[1] != Kp // 2 \
                or s.shape != (q.shape[0], Kp // MX_BLOCK):
            raise ValueError("Mxfp4Weight: q uint8 [N][Kp / 2] and s uint8 [N][Kp / 32], Kp = K (a multiple of 32) rounded up to 2048")
        self.q, self.s = q.contiguous(), s.contiguous()
        self.N, self.K = q.shape[0], K
        if (mq is None) != (ms is None):
            raise ValueError("Mxfp4Weight: the matrix-core image is mq AND ms")
        if mq is not None and (K % MX_QUAD or mq.dtype != torch.uint8 or ms.dtype != torch.uint8 or mq.shape != (self.N, K // 2)
                               or ms.shape != (self.N, K // MX_BLOCK) or mq.stride(1) != 1 or ms.stride(1) != 1):
            raise ValueError("Mxfp4Weight: mq uint8 [N][K / 2] and ms uint8 [N][K / 32], K a multiple of 128")
        self.mq, self.ms = mq, ms

    @staticmethod
    def _pack_mc(codes, scales):
        N, K = codes.shape
        if K % MX_QUAD:
            raise ValueError("Mxfp4Weight: the matrix-core image needs K to be a multiple of 128")
        byts = codes[:, 0::2] | (codes[:, 1::2] << 4)
        return _mc_swap(byts, N, K).contiguous(), scales.contiguous()

    @classmethod
    def from_codes(cls, codes, scales, matrix_cores=False):
        """Pack the logical (codes [N][K], scales [N][K/32]) of quantize_mxfp4 into the kernels' layout (matrix_cores: both images)."""
        N, K = codes.shape
        G = -(-K // MX_GROUP)
        c = torch.zeros(N, G * MX_GROUP, dtype=torch.uint8, device=codes.device)
        c[:, :K] = codes
        byts = c[:, 0::2] | (c[:, 1::2] << 4)                             # element 2m in bits 3:0, element 2m+1 in bits 7:4
        # linear dword 256 g + 64 i + L (elements 2048 g + 512 i + 8 L ..+7) -> dword 256 g + 4 L + i
        q = byts.view(N, G, 4, 64, 4).permute(0, 1, 3, 2, 4).reshape(N, G * MX_GROUP // 2)
        sc = torch.full((N, G * MX_GROUP // MX_BLOCK), 127, dtype=torch.uint8, device=codes.device)
        sc[:, :K // MX_BLOCK] = scales
        # block 64 g + 16 i + b -> byte 64 g + 4 b + i
        s = sc.view(N, G, 4, 16).permute(0, 1, 3, 2).reshape(N, G * MX_GROUP // MX_BLOCK)
        return cls(q, s, K, *(cls._pack_mc(codes, scales) if matrix_cores else ()))

    @classmethod
    def from_matrix(cls, w, matrix_cores=False):
        return cls.from_codes(*quantize_mxfp4(w), matrix_cores=matrix_cores)

    @property
    def has_matrix_core_image(self):
        return self.mq is not None

    def with_matrix_core_image(self):
        """Build the matrix-core image (from the first one) if it is not there yet; returns self."""
        if self.mq is None:
            self.mq, self.ms = self._pack_mc(*self.unpack())
        return self

    def unpack(self, matrix_cores=False):
        """-> the logical (codes uint8 [N][K], scales uint8 [N][K/32]); matrix_cores: read from the matrix-core image."""
        if matrix_cores:
            if self.mq is None:
                raise ValueError("Mxfp4Weight.unpack: this matrix holds no matrix-core image")
            byts = _mc_swap(self.mq.contiguous(), self.N, self.K)
            return torch.stack((byts & 15, byts >> 4), dim=2).view(self.N, self.K).contiguous(), self.ms.contiguous()
        N, G = self.N, self.q.shape[1] * 2 // MX_GROUP
        byts = self.q.view(N, G, 64, 4, 4).permute(0, 1, 3, 2, 4).reshape(N, G * MX_GROUP // 2)
        c = torch.stack((byts & 15, byts >> 4), dim=2).view(N, G * MX_GROUP)
        sc = self.s.view(N, G, 16, 4).permute(0, 1, 3, 2).reshape(N, G * MX_GROUP // MX_BLOCK)
        return c[:, :self.K].contiguous(), sc[:, :self.K // MX_BLOCK].contiguous()

    def dequantize(self):
        return dequantize_mxfp4(*self.unpack())

    @property
    def is_cuda(self):
        return self.q.is_cuda

    @property
    def shape(self):
        return torch.Size((self.N, self.K))

    @property
    def nbytes(self):
        """bytes one pass over the matrix streams (packed codes + scale bytes, padding included)"""
        return self.q.numel() + self.s.numel()

    @property
    def nbytes_matrix_cores(self):
        """bytes one pass over the matrix-core image streams (0 without it)"""
        return 0 if self.mq is None else self.N * (self.K // 2 + self.K // MX_BLOCK)

    def data_ptr(self):
        return self.q.data_ptr()

    def numel(self):
        return self.N * self.K
