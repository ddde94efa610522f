"""Lossless 13-bit image of a bf16 weight matrix for the batch-1 decode GEMVs (default on for the 7B's down_proj and gate/up).

The exponent field of a weight matrix is almost constant: of the 8 exponent bits of a bf16 weight the upper seven take, for all but
a few weights in a hundred million, one of 16 neighbouring values.  A weight with the 16 bits b is therefore stored as
    low byte  b & 0xff                      (exponent LSB + mantissa), raw;
    index     ((b >> 8) & 0x7f) - base      4 bits; base = (the matrix's largest upper-seven-bit exponent) - 15 (_pick_base);
    sign      b >> 15                       1 bit;
13 bits instead of 16, and the kernel rebuilds b exactly with integer operations (csrc/gemv_common.h gemv_wpack8).  A row that holds
a weight whose index is outside 0..15 (zeros, denormals, tiny values, inf / NaN) is MARKED: the kernel streams it from the bf16
matrix, which stays resident anyway (prefill, batched and speculative steps read it), so exactness never depends on the data and no
matrix is refused.  The packed bytes of a marked row are don't-care.

Byte layout (include/usdm_hip.h usdm_gemv_wpack states it; only this module and the kernel know it): a row is K / 2048 units of
3328 bytes; in unit u lane L of a wave owns, as in the bf16 kernels, the elements e(i, k) = 2048 u + 512 i + 8 L + k of the K
iterations i = 0..3, and every plane is contiguous over the lanes:
    bytes    0 .. 1023   low bytes, byte 16 L + 8 i + k for i = 0, 1
    bytes 1024 .. 2047   low bytes, byte 16 L + 8 (i - 2) + k for i = 2, 3
    bytes 2048 .. 3071   nibbles: dword 4 L + i, byte k (0..3) = index of e(i, k) | index of e(i, k + 4) << 4
    bytes 3072 .. 3327   signs: dword L, the sign of e(i, k) at bit 8 (k & 3) + 7 - (2 i + (k >> 2))
so that the kernel needs no per-weight shift.  Packing runs once at load, with torch ops on the device the matrix is on.

The interleaved gate/up matrix of a SwiGLU projection (blocks of 16 gate + 16 up rows; PackedWeight.from_matrix(w, glu=True)) is
packed row by row in the same layout.  Its kernel works on OUTPUTS - a wave streams the gate and the up rows of its outputs
together - so the bitmap in the kernel argument is per output there: output o is marked when its gate row or its up row is
(glu_row; csrc/gemv_common.h gemv_glu_row).
"""
import ctypes as C

import torch

UNIT_ELEMS = 2048
UNIT_BYTES = 3328
MAX_ROWS = 14336      # rows (glu: outputs) the kernel argument's bitmap of marked rows covers


def glu_row(o, up):
    """Weight row of SwiGLU output o in the interleaved gate/up matrix (csrc/gemv_common.h gemv_glu_row)."""
    return (o >> 4) * 32 + (o & 15) + (16 if up else 0)


def _i16(w):
    if w.dtype != torch.bfloat16 or w.dim() != 2 or w.shape[1] % UNIT_ELEMS:
        raise ValueError("wpack: a bf16 [N][K] matrix with K a multiple of 2048")
    return w.contiguous().view(torch.int16).to(torch.int32) & 0xffff


def _pick_base(e7):
    """The window's first field: (the matrix's largest upper-seven-bit exponent) - 15 wherever that window marks the fewest rows -
    every ordinary matrix.  A stray inf, NaN or outlier must not lift the window off the bulk (every row would be marked and the
    image would buy nothing), so the rule is stated as what it is for: of the windows base .. base + 15 the one that leaves the
    fewest rows marked, the lowest such on a tie (= largest exponent - 15 when the row that holds the largest exponent fits)."""
    rmin, rmax = e7.amin(dim=1), e7.amax(dim=1)
    cand = torch.arange(0, 0x7f - 15 + 1, device=e7.device)
    fits = ((rmin[None, :] >= cand[:, None]) & (rmax[None, :] <= cand[:, None] + 15)).sum(dim=1)
    best = int(fits.max().item())
    return int(cand[fits == best].min().item())


def pack(w):
    """w bf16 [N][K] -> (planes uint8 [N][K / 2048 * 3328], rowflag uint8 [N rounded up to 4], base)."""
    b = _i16(w)
    N, K = b.shape
    U = K // UNIT_ELEMS
    e7 = (b >> 8) & 0x7f
    base = _pick_base(e7)
    idx = e7 - base
    marked = ((idx < 0) | (idx > 15)).any(dim=1)
    idx = idx & 15                                                    # (marked rows: don't-care)
    v = lambda t: t.view(N, U, 4, 64, 8)                              # [row][unit][iteration i][lane L][k]
    lo, ix, sg = v(b & 0xff), v(idx), v(b >> 15)
    low = lo.permute(0, 1, 3, 2, 4).reshape(N, U, 64, 32)             # per lane: (i, k) -> byte 8 i + k
    la, lb = low[..., :16].reshape(N, U, 1024), low[..., 16:].reshape(N, U, 1024)
    nib = (ix[..., :4] | (ix[..., 4:] << 4)).permute(0, 1, 3, 2, 4).reshape(N, U, 1024)   # per lane: dword i, byte k
    # sign dword of a lane: bit 8 (k & 3) + 7 - (2 i + (k >> 2))
    i_ = torch.arange(4, device=w.device).view(4, 1, 1)
    k_ = torch.arange(8, device=w.device).view(1, 1, 8)
    sh = 8 * (k_ & 3) + 7 - (2 * i_ + (k_ >> 2))                       # [i][1][k]
    sd = (sg.to(torch.int64) << sh).sum(dim=(2, 4))                    # [N][U][L] (distinct bits: the sum is the or)
    sb = torch.stack([(sd >> (8 * j)) & 0xff for j in range(4)], dim=-1).reshape(N, U, 256)
    planes = torch.cat((la, lb, nib, sb.to(torch.int32)), dim=2).to(torch.uint8).reshape(N, U * UNIT_BYTES).contiguous()
    flag = torch.zeros((N + 3) // 4 * 4, dtype=torch.uint8, device=w.device)
    flag[:N] = marked.to(torch.uint8)
    return planes, flag, base


def unpack(planes, base, K):
    """The inverse of pack in plain torch ops: planes uint8 [N][K / 2048 * 3328] -> the 16 bits of every weight, int32 [N][K]
    (rows that were marked come back as whatever their don't-care bytes say)."""
    N, U = planes.shape[0], K // UNIT_ELEMS
    p = planes.view(N, U, UNIT_BYTES).to(torch.int32)
    low = torch.cat((p[..., :1024].reshape(N, U, 64, 16), p[..., 1024:2048].reshape(N, U, 64, 16)), dim=3)    # [lane][8 i + k]
    lo = low.view(N, U, 64, 4, 8).permute(0, 1, 3, 2, 4)                                                       # [i][L][k]
    nb = p[..., 2048:3072].reshape(N, U, 64, 4, 4).permute(0, 1, 3, 2, 4)                                      # [i][L][byte k]
    ix = torch.cat((nb & 15, nb >> 4), dim=4)                                                                  # k = 0..7
    sb = p[..., 3072:].reshape(N, U, 64, 4).to(torch.int64)
    sd = (sb[..., 0] | (sb[..., 1] << 8) | (sb[..., 2] << 16) | (sb[..., 3] << 24)).view(N, U, 1, 64, 1)
    i_ = torch.arange(4, device=planes.device).view(4, 1, 1)
    k_ = torch.arange(8, device=planes.device).view(1, 1, 8)
    sg = ((sd >> (8 * (k_ & 3) + 7 - (2 * i_ + (k_ >> 2)))) & 1).to(torch.int32)
    return (lo | ((ix + base) << 8) | (sg << 15)).reshape(N, K)


class GemvWpack(C.Structure):
    """usdm_gemv_wpack (include/usdm_hip.h)."""
    _fields_ = [("planes", C.c_void_p), ("rowflag", C.c_void_p), ("stride", C.c_int64), ("base", C.c_int32), ("units", C.c_int32),
                ("marked", C.c_uint32 * (MAX_ROWS // 32))]


class PackedWeight:
    """The image of one matrix as ops.gemv(..., wpack=) takes it.  from_matrix verifies its own round trip - unpack(pack(W)) == W
    on the raw bits of every unmarked row - and raises if that fails.  glu: the interleaved gate/up matrix of a SwiGLU call;
    marked_outputs are then the outputs whose gate or up row is marked (the bits of args().marked), else None."""
    __slots__ = ("planes", "rowflag", "base", "N", "K", "marked_rows", "glu", "marked_outputs")

    def __init__(self, planes, rowflag, base, K, glu=False):
        self.planes, self.rowflag, self.base, self.K, self.glu = planes, rowflag, int(base), K, bool(glu)
        self.N = planes.shape[0]
        if glu and self.N % 32:
            raise ValueError("wpack: a gate/up matrix has a multiple of 32 rows")
        if (self.N // 2 if glu else self.N) > MAX_ROWS:
            raise ValueError(f"wpack: at most {MAX_ROWS} {'outputs' if glu else 'rows'}")
        self.marked_rows = torch.nonzero(rowflag[:self.N]).flatten().tolist()
        # rows [block][gate | up][16] -> outputs [block][16]: glu_row's formula
        self.marked_outputs = torch.nonzero(rowflag[:self.N].view(-1, 2, 16).amax(dim=1).flatten()).flatten().tolist() if glu else None

    @classmethod
    def from_matrix(cls, w, glu=False):
        planes, flag, base = pack(w)
        ok = (unpack(planes, base, w.shape[1]) == _i16(w)).all(dim=1) | (flag[:w.shape[0]] != 0)
        if not bool(ok.all()):
            raise RuntimeError("wpack: the packed image does not reproduce the matrix")
        return cls(planes, flag, base, w.shape[1], glu)

    @property
    def is_cuda(self):
        return self.planes.is_cuda

    @property
    def marked_share(self):
        return len(self.marked_rows) / self.N

    @property
    def nbytes(self):
        return self.planes.numel() + self.rowflag.numel()

    def args(self):
        a = GemvWpack()
        a.planes, a.rowflag = C.c_void_p(self.planes.data_ptr()), C.c_void_p(self.rowflag.data_ptr())
        a.stride, a.base, a.units = self.planes.shape[1], self.base, self.K // UNIT_ELEMS
        for r in (self.marked_outputs if self.glu else self.marked_rows):
            a.marked[r >> 5] |= 1 << (r & 31)
        return a
