"""Plain CPU reference of the two bf16 decode-GEMV anchors, usdm_gemv and usdm_gemv_batch, and the inputs of
tests/test_gemv_exact_gpu.py, checked themselves by tests/test_gemv_exact_cpu.py.  Written from the contract in include/usdm_hip.h
(usdm_gemv_args, usdm_gemv_batch_args), not from the kernels:

  x'      = bf16(x + bf16(x_delta))                                   (x_delta given; x_out receives x')
  x'      = bf16(bf16(x' * rstd) * norm_w),  rstd = 1 / sqrt(mean(x'^2) + eps)      (norm_w given)
  acc[n]  = sum_k W[n][k] * x'[k]
  plain   : v = acc [-> bf16]; v += residual [-> bf16]                 ([-> bf16]: with round_bf16)
  SwiGLU  : rows packed in blocks of 16 gate + 16 up rows; v = silu(g) * u, with round_bf16 bf16(bf16(silu(bf16(g))) * bf16(u))
  lm_head : y32 = bf16(acc), -inf on banned rows; one (max, lowest-id arg-max + idx_offset) partial per block of rows, a block
            without a candidate holds (-inf, 0x7fffffff)
  batched : item b at + b * stride of x, y, residual and the partials; W, norm_w and ban are shared

Conventions (those of tests/_gemm_reference.py)
  * integer operands: x in {-1 ... 3} and W in +-{-1 ... 3} (one sign per row), both inside {-3 ... 3}, held as bf16.  With K <= 16384
    every partial sum is an integer below 2^24, so an f32 accumulator holds the TRUE sum in any order (v_dot2 or MFMA), and one
    fp64 matmul is the reference of every kernel bit for bit.  The means are +-1, so most sums are near +-K and round_bf16 does
    something from K = 504 on.  Residuals are integers in {-8 ... 8}.
  * every operand sits in a buffer whose gaps hold NaN: ldw = K + 8 and one row after the last of W, eight elements after x (per
    item: x_bs = K + 8, and one more item row of NaN), norm_w, x_delta and the residual rows.  Bytes 1 follow the ban array.
  * every output sits in a sentinel-filled buffer larger than what the kernel owns (y_bs > nout, part_bs > blocks, one more item
    row; x_out likewise).  What the kernel owns must hold the reference, the rest the sentinel, bit for bit.
  * SwiGLU: x = integers / 16 and W sparse in {-1, 0, 1}: the pre-activations are exact multiples of 1/16 within +-20.
  * fused RMSNorm, family "exact": x = +-2, norm_w small integers (times 1/16 under SwiGLU) and eps = 1e-5 give
    bf16(x * rstd) = +-1 for any rstd within 2^-11 of 1/2 (1 - 2^-9 is the tie below 1), so x' = +-norm_w exactly and the case is an integer case.
    Family "probe": W rows are unit vectors, so y[n] = x'[k_n] with no arithmetic in between, x Gaussian with the last eight
    elements x 16, norm_w = 1 + 0.1 Gaussian.  The reference x' is evaluated at rstd (1 - DELTA) and rstd (1 + DELTA); a GPU element
    must equal one of the two.

Quantized weight formats (Case.fmt = "fp8" | "mxfp4": usdm_gemv_fp8, usdm_gemv_mxfp4, their VALU batch forms, usdm_gemv_fp8_mfma; the
cases of tests/test_gemv_quant_exact_gpu.py).  The logical weights are the same small integers times a power of two per row (FP8)
or per block of 32 (MXFP4) that differs between neighbours (weight_exponents), so that dequantize(quantize(W)) = W bit for bit and
the fp64 reference above is the exact reference of these kernels too; device_weight builds what the entry points take (FP8: NaN
bytes in the gap after every row and in one more row).  Probe rows are not scaled.  The K ladders follow the format's own ring
(fmt_ring_depth, k_ladder).

DELTA.  x is bf16, so every square is exact in f32 and only the additions of the sum of squares round.  All terms are positive: a
sum whose longest chain has n additions is within n 2^-24 of the true sum, relatively.  The longest chain of any instantiation is
the matrix-core kernel's at K = 4096: 128 sequential FMAs per lane (16 held fragments of 8 elements), 2 cross-lane additions and 8
per-wave partials = 138.  (usdm_gemv at K = 16384 with 256 threads: 8 pieces per thread, each four times ss += lo lo + hi hi
without contraction, i.e. 4 additions on the chain and one rounding of the pair sum beside it = 8 x 5 = 40, 6 for the wave, up to
16 wave partials = 62.)  rstd = sum^(-1/2) halves the relative error: 69.  The division by K, the addition of eps
and the device's rsqrt (one ulp) add at most 0.5 + 0.5 + 2, and the f32 rounding of x * rstd before its bf16 rounding acts like
one more 2^-24 on rstd: 73 2^-24 < 128 2^-24 = 2^-17.

Merged-attention input (Case.merge = "mrg" | "cmb": usdm_gemv with mrg_pm / mrg_pl / mrg_po / mrg_ns, and its hand-off form
cmb_gran; the cases of tests/test_gemv_merge_exact_gpu.py).  From usdm_gemv_args and the header of csrc/attn_merge.h: K = heads x 128,
  x[h 128 + d] = bf16(sum_s po[h][s][d] e_s / sum_s pl[h][s] e_s),  e_s = exp(pm[h][s] - max_s pm[h][s])        (merge_ref)
and x is what the projection multiplies; the x pointer is not read (a buffer of NaN).  NaN follows pm, pl (PAD elements) and po
(one more row of 128).  e_s is a float32 number: below the smallest float32 denormal it is 0.
  * family "exact": per head 1 <= L <= NS live splits at places of their own share ONE pm, so their e_s is 1 in any arithmetic;
    their pl are positive integers that sum to 2^j (j differs between heads), their po integers that sum to x 2^j with x the
    integer x of the integer cases, every sum of magnitudes far below 2^24.  The merged x then IS that integer x in float32 in
    any order of summation (fma or not), and everything downstream is the integer case above, bit for bit.  The other splits are
    dead: the kernels' own marker (pm = -1e30, pl = 0), or pm = max - 200 with pl = 3 (e^-200 = 0 in float32).  A dead split's po
    is +-2^100: any weight but an exact 0 shows.
  * family "probe": real softmax weights.  pm Gaussian (sigma 1, 3, 6 by head) clipped to max - 16, one dead split (the marker)
    per head, pl in (0.5, 1.5), po Gaussian; W rows are unit vectors and round_bf16 is off, so y32[n] = x[k_n].  A GPU element must
    be a bf16 value with |got - ref64| <= half a bf16 ulp of ref64 + B,
      B = MERGE_K 2^-24 S / D,  S = sum_s |po_s| e_s,  D = sum_s pl_s e_s.

MERGE_K, in units of u = 2^-24 (one float32 rounding, relative).  e_s: the argument pm_s - max rounds once, and where exp is
exp2(a log2 e) so do the constant and the product: three roundings of an argument of magnitude |a| <= 16 move e^a by 3 |a| u <= 48 u,
and the device's exp2 is good to one ulp = 2 u: 50 u per weight (the maximum's own weight is exactly 1).  Numerator: one rounding per
product (none with fma) and at most 64 additions, each relative to a partial sum of magnitude <= S, and the weights' 50 u: (1 + 64
+ 50) u S = 115 u S absolute.  Denominator, all terms positive: 115 u relative.  One reciprocal (one ulp: 2 u) and one product
(u).  With |ref| = |num| / D <= S / D:  |v - ref| <= (115 + 115 + 2 + 1) u S / D = 233 u S / D < 256 u S / D: MERGE_K = 256.
The bf16 rounding of v: got is the bf16 value nearest to v; if it is not the one nearest to ref, a midpoint m lies between ref and
v, got is half a spacing from m and |m - ref| <= |v - ref|: half an ulp + B.  (The spacing is the one at ref unless v crossed a
power of two upwards by more than half the wider spacing, which takes B above one ulp of ref: the few elements that cancel that
much.  The test keeps half an ulp OF REF there too, the stricter reading.)
S / |num| is the cancellation of an element; B is below half an ulp while it is below 128 (tests/test_gemv_exact_cpu.py: for
>= 98 % of each case's elements, a condition on the seeds).
"""
import torch
import torch.nn.functional as Fn

from tests._glue_reference import BF, F32, F64, SENT32, bits, gen, is_sentinel, sentinel  # noqa: F401
from tests._gemm_reference import (FLIP_CAP, GEMM_SWIGLU_TORCH_FP32_ERR, Exp, bf16_ulp, check_exact, check_guard, rbf64,  # noqa: F401
                                   swiglu_rbf_ref)

NAN, INF = float("nan"), float("inf")
ACT_NONE, ACT_SWIGLU = 0, 3
NO_IDX = 0x7fffffff
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=F32))
DELTA = 2.0 ** -17
PROBE_CAP = 0.02            # share of a probe case's elements on which the two references may differ
PAD = 8                     # elements of 16 bytes: the NaN gap after every operand row
# SwiGLU without round_bf16: 4 x torch's own float32 error per max(|ref|, |u|), as the GEMM test.  The device evaluates e^-g as
# exp2(-g log2 e): the product rounds once (2^-24 of |g| log2 e) and log2 e is held to 2^-25, so e^-g carries about
# 1.5 |g| 2^-24 on top of the exp2's ulp.  silu'(e^-g) turns that into g^2 s (1 - s) 1.5 2^-24 with s = sigmoid(g); g^2 s (1 - s)
# peaks at 0.44 (|g| = 2.4), i.e. 4e-8 per |u|, a sixteenth of the bound: no |g|-proportional term is needed at |g| <= 20.
SWIGLU_TOL = 4.0 * GEMM_SWIGLU_TORCH_FP32_ERR


def cdiv(a, b):
    return -(-a // b)


ALT16_BITS = 0x7e7e     # the second fill of a bf16 buffer (a finite bf16 again); f32 and int32 buffers: -SENT32 in their own dtype


def alt_sentinel(shape, dtype, device=None):
    """a buffer pre-filled with the dtype's second sentinel: an owned element that legitimately holds the first sentinel's bits is
    read again over this fill (a written element holds the same bits again, an unwritten one this fill)"""
    if dtype == BF:
        return torch.full(shape, ALT16_BITS, dtype=torch.int16, device=device).view(BF)
    return torch.full(shape, -int(SENT32) if dtype == torch.int32 else -SENT32, dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------------------------ launch selection
# (rows per wave, GLU, waves): output count at which usdm_gemv reaches each instantiation ("lm": lm_head mode, always 4 rows)
VALU_INST = {(1, False, 4): 37, (2, False, 4): 4081, (3, False, 4): 8193, (4, False, 4): 16369, (1, False, 16): 4096,
             (2, False, 12): 6144, (1, True, 4): 48, (2, True, 4): 5136, (2, True, 7): 7168}
SMALL_INST = ((1, False, 4), (1, True, 4))
LM_N = 1003
BATCH_INST = ((1, False, 4), (1, False, 16), (1, True, 4))


def inst_id(i):
    return "lm_head" if i == "lm" else f"rw{i[0]}{'-glu' if i[1] else ''}-{i[2]}waves"


def pick_rw(nout, glu):
    """gemv_pick_rw: the largest rows-per-wave with >= 1024 workgroups at >= 90 % balance over 256 CUs, else the best score"""
    cands = (2, 1) if glu else (4, 3, 2, 1)
    best, best_score = cands[-1], -1.0
    for rw in cands:
        blocks = cdiv(nout, 4 * rw)
        eff = (blocks / 256.0) / float((blocks + 255) // 256)
        if blocks >= 1024 and eff >= 0.9:
            return rw
        score = eff * (1.0 if blocks >= 512 else 0.5 + blocks / 1024.0)
        if score > best_score:
            best_score, best = score, rw
    return best


def valu_select(N, *, glu=False, lm_head=False, batched=False, merge=None):
    """gemv_select for the single-GPU forms -> (rows per wave, GLU, waves per workgroup, grid).  merge: "mrg" (mrg_po given: the
    16-wave row at 16 rows per CU, else one row per wave whatever the balance rule says) | "cmb" (refused unless N = 4096)"""
    nout = N // 2 if glu else N
    rows_per_cu = nout // 256 if nout % 256 == 0 else 0
    if merge and not batched:
        return (1, False, 16, 256) if (rows_per_cu == 16 or merge == "cmb") else (1, False, 4, cdiv(nout, 4))
    if not glu and not lm_head and rows_per_cu == 16:
        return 1, False, 16, 256
    if not glu and not lm_head and rows_per_cu == 24:
        return 2, False, 12, 256
    if not batched and glu and nout % 14 == 0 and (nout // 14) % 512 == 0:
        return 2, True, 7, nout // 14
    rw = 4 if lm_head else pick_rw(nout, glu)
    return rw, glu, 4, cdiv(nout, 4 * rw)


def ring_depth(rw, glu):
    """gemv_ring_depth of the bf16 format: K iterations of 512 in flight per row"""
    nr = 2 * rw if glu else rw
    return 2 if nr >= 8 else 4 if nr >= 4 else 5 if nr == 3 else 8


FMTS = ("fp8", "mxfp4")     # the quantized weight formats; "bf16" is the default of every case


def fmt_ring_depth(rw, glu, fmt="bf16"):
    """gemv_ring_depth(NR, FP8, MX4): FP8 twice the bf16 depth (8-byte loads); MXFP4: slots of one group = four K iterations"""
    if fmt == "mxfp4":
        return 2 if (2 * rw if glu else rw) >= 3 else 4
    return ring_depth(rw, glu) * (2 if fmt == "fp8" else 1)


MW, CH, KS_K, KS_MAX, MTG_TRL = 8, 16, 2048, 8, 8
MFMA_VARIANTS = ("hold", "hold16-recut", "hold16-frag", "stream", "stream56-recut", "stream56-frag", "ksplit")


def ks_floats(N, K):
    if K <= MW * CH * 32 or K % KS_K != 0 or K // KS_K > KS_MAX or N <= 0:
        return 0
    return cdiv(N, 16) * (K // KS_K) * 256


def mfma_select(N, K, *, glu=False, lm_head=False, norm=False, form=1, ks=False):
    """the matrix-core launcher's decisions -> dict(variant, rt (rows per tile), ksplit, ntiles, grid, kwg (workgroups that share the tiles))"""
    cpw = cdiv(K // 32, MW)
    hold = cpw <= CH
    nout = N // 2 if glu else N
    rt, ksplit = 16, 1
    if ks_floats(N, K) and ks and not glu and not lm_head and not norm and form not in (3, 5):
        ksplit = K // KS_K
        if cdiv(cdiv(N, 16), min(256 // ksplit, cdiv(N, 16))) > MTG_TRL:
            ksplit = 1
    if glu:
        ntiles = cdiv(nout, 8)
    elif lm_head:
        ntiles = cdiv(N, 16)
    else:
        best = 1 << 30
        for r in (16, 12, 8):
            nt = cdiv(N, r)
            per = cdiv(nt, min(nt, 256)) * r
            if per < best:
                best, rt = per, r
        ntiles = cdiv(N, rt)
    grid = kwg = min(ntiles, 256)
    if ksplit > 1:
        rt, ntiles = 16, cdiv(N, 16)
        kwg = min(256 // ksplit, ntiles)
        grid = kwg * ksplit
        variant = "ksplit"
    else:
        variant = "hold" if hold else "stream"
        if cpw == (16 if hold else 56):      # K = 4096 / 14336: chunks per wave as a constant; row-contiguous loads re-cut through LDS unless form 3
            variant += str(cpw) + ("-frag" if form == 3 else "-recut")
    return dict(variant=variant, rt=rt, ksplit=ksplit, ntiles=ntiles, grid=grid, kwg=kwg)


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """one projection.  nb = 0: usdm_gemv; nb >= 1: usdm_gemv_batch with `form`.  kind: "int" | "swiglu" | "probe"; norm: None |
    "exact" | "probe"; ban: None | "none" | "workgroup" | "wave" | "scattered" | "last" (lm_head mode when not None); merge: None |
    "mrg" | "cmb" (x merged from NS attention partials per head; mfam: "exact" with kind "int", "probe" with kind "probe")"""

    def __init__(self, name, *, N, K, seed, nb=0, form=0, glu=False, kind="int", norm=None, res=False, inplace=False, ban=None, idx_offset=0,
                 delta=False, skip=False, ks=False, inst=None, variant=None, rt=None, fmt="bf16", mfma=None, merge=None, NS=0, mfam="exact"):
        self.name, self.N, self.K, self.seed, self.nb, self.form, self.glu = name, N, K, seed, nb, form, glu
        self.merge, self.NS, self.mfam = merge, NS, mfam
        assert merge is None or (merge in ("mrg", "cmb") and 1 <= NS <= 64 and K % 128 == 0 and kind == ("int" if mfam == "exact" else "probe")
                                 and not (nb or glu or norm or delta or ban) and fmt == "bf16"), "the merged input: a plain batch-1 bf16 projection"
        self.kind, self.norm, self.res, self.inplace, self.ban, self.idx_offset = kind, norm, res, inplace, ban, idx_offset
        self.delta, self.skip, self.ks, self.inst, self.variant, self.rt = delta, skip, ks, inst, variant, rt
        self.fmt = fmt
        self.B = max(nb, 1)
        self.lm_head = ban is not None
        # (mfma=True: usdm_gemv_fp8_mfma, which runs the matrix cores at every nb and takes form 0 where usdm_gemv_batch takes 1)
        self.mfma = (nb >= 1 and (form in (1, 3, 5) or (form == 0 and nb > 4))) if mfma is None else mfma
        self.nout = N // 2 if glu else N
        self.ldw = self.x_bs = K + PAD
        if fmt == "fp8" and self.mfma:       # usdm_gemv_fp8_mfma wants 16-byte rows of bytes: a gap of 16
            self.ldw = K + 2 * PAD
        self.y_bs = self.nout + 5
        self.res_bs = self.y_bs if inplace else self.nout + 3
        self.sel = mfma_select(N, K, glu=glu, lm_head=self.lm_head, norm=norm is not None, form=form, ks=ks) if self.mfma else None
        self.nparts = (self.sel["grid"] if self.mfma else cdiv(N, 16)) if self.lm_head else 0
        self.part_bs = self.nparts + 3 if self.lm_head else 0
        assert not (glu and (res or self.lm_head)) and not (delta and nb) and K % 8 == 0
        assert fmt == "bf16" or (fmt in FMTS and not delta and form != 3), "the quantized formats refuse x_delta and have no fragment-shaped form"
        assert fmt != "mxfp4" or (K % 32 == 0 and not self.lm_head and not self.mfma), "MXFP4: whole blocks of 32, no lm_head mode, no matrix cores"

    @property
    def act(self):
        return ACT_SWIGLU if self.glu else ACT_NONE

    def selected(self):
        """what the launch is expected to reach: the VALU tuple, or the matrix-core (variant, rows per tile)"""
        if self.mfma:
            return self.sel["variant"], self.sel["rt"]
        return valu_select(self.N, glu=self.glu, lm_head=self.lm_head, batched=self.nb >= 1, merge=self.merge)[:3]

    def threads(self):
        return MW * 64 if self.mfma else 64 * self.selected()[2]

    def __repr__(self):
        return self.name


class Data:
    pass


def _ints(shape, g, lo, hi, dtype=torch.int8):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=dtype)


def _guarded(vals, stride, rows=None, fill=NAN, dtype=BF):
    """[rows + 1][stride] filled with `fill`, vals [rows][n] in its top left corner, flat"""
    rows = vals.shape[0] if rows is None else rows
    buf = torch.full((rows + 1, stride), fill, dtype=dtype)
    buf[:vals.shape[0], :vals.shape[1]] = vals.to(dtype)
    return buf.reshape(-1)


def probe_positions(c):
    """the K positions the probe's unit rows read: all of K where there are rows enough; else the last and first 16 elements and 16
    either side of every multiple of 8 x threads, then evenly spread ones, as many as there are outputs.
    Merged input (37 outputs must do): a thread stages four elements (the hand-off form: one granule of two) and a head is 128: the
    last and first four elements (whole threads and granules, the last element of the last head), four either side of every pass
    of the workgroup, the last and first element of a head (127, 128) and the first two of the last head, then evenly spread ones"""
    n, K = c.nout, c.K
    if n >= K:
        return torch.arange(n) % K
    if c.merge:
        step = (2 if c.merge == "cmb" else 4) * c.threads()
        pos = list(range(K - 4, K)) + list(range(4)) + [p for m in range(step, K + 4, step) for p in range(m - 4, m + 4)] + [127, 128, K - 128, K - 127]
    else:
        step = 8 * c.threads()
        pos = list(range(K - 16, K)) + [p for m in range(step, K + 16, step) for p in range(m - 16, m + 16)] + list(range(16))
    pos += [(i * K) // n for i in range(n)]
    out = []
    for p in pos:
        if 0 <= p < K and p not in out:
            out.append(p)
    return torch.tensor(out[:n])


def ban_pattern(c):
    """uint8 [N] of the lm_head cases: rows the arg-max must ignore"""
    N, ban = c.N, torch.zeros(c.N, dtype=torch.uint8)
    g = gen(c.seed + 9)
    if c.ban == "workgroup":            # blocks 1 and 2 of 16 rows entirely (a whole workgroup of either form), and the ragged last one
        ban[16:48] = 1
        ban[N - N % 16:] = 1
    elif c.ban == "wave":               # rows 4 ... 7 of block 0 (a whole wave of usdm_gemv), rows 16 ... 30 (all but one of block 1)
        ban[4:8] = 1
        ban[16:31] = 1
    elif c.ban == "scattered":
        ban[torch.rand(N, generator=g) < 0.4] = 1
    elif c.ban == "last":
        ban[N - 1] = 1
    return ban


def weight_exponents(c):
    """int32 [N][1] (FP8: per row) or [N][K / 32] (MXFP4: per block): the power of two each logical weight of an integer or SwiGLU
    case is multiplied by, so that neighbouring rows and blocks have different scales.  Integer cases: -3 ... 3 per row, 0 ... 3 per
    block.  SwiGLU cases shrink only (|g| <= 20 stays true): -3 ... 0, four values, because the sparse +-1 weights have one magnitude
    per scale and the CPU test asks for four distinct exponents (scale bytes) per case.
    The row term is (5 n) mod 7 throughout: its period is odd, so rows 1, 4 or 16 apart (the next row, wave, gate / up partner) differ.
    MXFP4: ((5 n) mod 7 + 3 b + 3 (b div 64)) mod 4 for block b of row n.  With (n + 3 b) mod 4 alone, rows 4 apart and blocks 64
    apart (the same place in the next group, i.e. in the next ring slot) would share their scales, and a kernel that took the scale
    dword of the wrong slot or row would still pass.  The factor 3 keeps blocks 1, 64 and 128 apart different (4 groups apart
    coincide: there are four values)."""
    n = (5 * torch.arange(c.N, dtype=torch.int32).view(-1, 1)) % 7
    if c.fmt == "fp8":
        return -(n % 4) if c.kind == "swiglu" else n - 3
    b = torch.arange(c.K // 32, dtype=torch.int32).view(1, -1)
    e = (n + 3 * b + 3 * (b // 64)) % 4
    return -e if c.kind == "swiglu" else e


FP8_NAN = 0x7f      # e4m3fn NaN: the fill of the gaps of an FP8 weight buffer


def device_weight(c, d, dev="cpu", fmt=None):
    """(W, ldw) as ops.gemv / gemv_batch / gemv_fp8_mfma take it, on dev.  fmt (default: the case's): "bf16" gives the guarded bf16
    buffer of d.Wl (of a quantized case: the operand of the bf16 entry point it is compared with).  "fp8": quantize_rows(d.Wl) with
    q widened to [N + 1][ldw], NaN bytes in the gap and in the extra row (whose exponent is 0).  "mxfp4": Mxfp4Weight.from_matrix;
    its padding to whole groups (zero codes, scale bytes 127) belongs to the format.  Quantization runs on dev (it is deterministic:
    comparisons, frexp and ldexp only), once per case."""
    from usdm_amd import quant
    fmt = c.fmt if fmt is None else fmt
    if fmt == "bf16":
        W = _guarded(d.Wl, c.K + PAD) if d.W is None else d.W
        return W.to(dev), c.K + PAD
    Wl = d.Wl.to(dev)
    if fmt == "mxfp4":
        return quant.Mxfp4Weight.from_matrix(Wl), None
    q, e = quant.quantize_rows(Wl)
    buf = torch.full((c.N + 1, c.ldw), FP8_NAN, dtype=torch.uint8, device=dev)
    buf[:c.N, :c.K] = q
    return quant.Fp8Weight(buf, torch.cat([e, torch.zeros(1, dtype=torch.int8, device=dev)])), c.ldw


def build(c):
    """the case's logical operands (fp64 / bf16) and its guarded flat buffers, all on the CPU"""
    d, g = Data(), gen(c.seed)
    N, K, B = c.N, c.K, c.B
    d.kpos = None
    # ---- x [B][K] (fp64, logical), norm_w [K], W [N][K] (bf16, logical)
    if c.norm == "probe":
        x = torch.randn(B, K, generator=g)
        x[:, K - 8:] *= 16.0
        d.xl = x.to(BF).double()
        d.gl = (1.0 + 0.1 * torch.randn(K, generator=g)).float().double()
    elif c.norm == "exact":
        sgn = (_ints((B, K), g, 0, 1).double() * 2 - 1)
        d.xl = 2.0 * sgn
        if c.kind == "swiglu":
            d.gl = _ints((K,), g, -3, 3).double() / 16
        else:                            # positive x' for item 0 (the sign of norm_w follows item 0's x), so that the sums are near +-2 K
            d.gl = sgn[0] * _ints((K,), g, 1, 3).double()
    else:
        d.gl = None
        d.xl = _ints((B, K), g, -3, 3).double() / 16 if c.kind == "swiglu" else _ints((B, K), g, -1, 3).double()
    if c.kind == "probe":
        pos = probe_positions(c)
        rows = torch.arange(c.nout)
        d.kpos = torch.zeros(N, dtype=torch.int64)
        if c.glu:                        # gate and up row of an output read the same element: y = silu(x'[k]) * x'[k]
            gate = (rows // 16) * 32 + rows % 16
            d.kpos[gate], d.kpos[gate + 16] = pos, pos
        else:
            d.kpos[rows] = pos
        d.Wl = torch.zeros(N, K, dtype=BF)
        d.Wl[torch.arange(N), d.kpos] = 1.0
    elif c.kind == "swiglu":
        keep = torch.rand(N, K, generator=g) < min(1.0, 800.0 / K)
        d.Wl = (_ints((N, K), g, 0, 1) * 2 - 1).to(BF) * keep.to(BF)
    else:
        d.Wl = (_ints((N, K), g, -1, 3) * (_ints((N, 1), g, 0, 1) * 2 - 1)).to(BF)
    d.wexp = None
    if c.fmt != "bf16" and c.kind != "probe":
        d.wexp = weight_exponents(c)
        # exact: small integers x 2^e; + 0.0: the sparse SwiGLU weights hold -0.0, which the MXFP4 codes do not have
        d.Wl = (torch.ldexp(d.Wl.float().view(N, d.wexp.shape[1], -1), d.wexp.float()[:, :, None]).view(N, K) + 0.0).to(BF)
    d.W = _guarded(d.Wl, c.ldw) if c.fmt == "bf16" else None      # (the quantized formats: device_weight)
    d.x = _guarded(d.xl, c.x_bs)
    d.norm_w = None if d.gl is None else _guarded(d.gl.view(1, -1), K + PAD, rows=0, dtype=F32)
    # ---- x_delta: integer-valued f32 (with the exact norm family: zero but for a few elements whose x + delta is again +-2)
    d.dl = d.x_delta = None
    if c.delta:
        if c.norm == "exact":
            d.dl = torch.zeros(K, dtype=F64)
            at = torch.randperm(K, generator=g)[:max(1, K // 5)]
            d.dl[at] = -2.0 * d.xl[0, at]
        else:
            d.dl = _ints((K,), g, -2, 0).double()                 # x + delta stays inside {-3 ... 3}
        d.x_delta = _guarded(d.dl.view(1, -1), K + PAD, rows=0, dtype=F32)
    # ---- residual [B][nout], ban [N]
    d.rl = _ints((B, c.nout), g, -8, 8).double() if c.res else None
    d.res = None if d.rl is None else _guarded(d.rl, c.res_bs)
    d.banl = ban_pattern(c) if c.lm_head else None
    d.ban = None if (d.banl is None or c.ban == "none") else torch.cat([d.banl, torch.ones(16, dtype=torch.uint8)])
    if c.merge:
        _build_merge(c, d, g)
    return d


MRG_DEAD_PM = -1e30         # the marker usdm_attn_decode leaves in an empty split (with pl = 0)
MRG_DEAD_PO = 2.0 ** 100


def _build_merge(c, d, g):
    """d.pm, d.pl [H][NS], d.po [H][NS][128] (float32, logical), their guarded flat buffers d.pm_buf, d.pl_buf, d.po_buf, d.live
    (bool [H][NS]), and d.x = K elements of NaN (the x pointer is not read).  The exact family merges to d.xl (module docstring)"""
    H, NS, K = c.K // 128, c.NS, c.K
    dead_po = MRG_DEAD_PO * (_ints((H, NS, 128), g, 0, 1).float() * 2 - 1)
    if c.mfam == "probe":
        sigma = torch.tensor([1.0, 3.0, 6.0])[torch.arange(H) % 3].view(H, 1)
        pm = (sigma * torch.randn(H, NS, generator=g)).float()
        live = torch.ones(H, NS, dtype=torch.bool)
        live[torch.arange(H), _ints((H,), g, 0, NS - 1, torch.int64)] = False
        mx = torch.where(live, pm, torch.full((), -INF)).max(-1, keepdim=True).values
        pm = torch.maximum(pm, (mx.double() - 16.0).float())
        pm = torch.where(mx.double() - pm.double() > 16.0, torch.nextafter(pm, mx), pm)      # (the float32 of max - 16 may lie below it)
        pl = (0.5 + torch.rand(H, NS, generator=g)).float()
        po = torch.randn(H, NS, 128, generator=g).float()
        pm, pl = torch.where(live, pm, torch.full((), MRG_DEAD_PM)), torch.where(live, pl, torch.zeros(()))
    else:
        x = d.xl[0].view(H, 128)
        pm, pl, live = torch.empty(H, NS), torch.empty(H, NS), torch.zeros(H, NS, dtype=torch.bool)
        po = torch.zeros(H, NS, 128)
        for h in range(H):
            L = NS if h % 4 == 1 else 1 if h % 4 == 2 else int(_ints((1,), g, 1, NS, torch.int64))
            at = torch.randperm(NS, generator=g)[:L]
            live[h, at] = True
            j = (L - 1).bit_length() + h % 4                              # 2^j >= L; j <= 9
            w = torch.rand(L, generator=g).double()
            a = 1 + torch.floor((2 ** j - L) * w / w.sum())              # positive integers ...
            a[0] += 2 ** j - a.sum()                                      # ... that sum to 2^j
            o = _ints((L, 128), g, -2 ** (j + 1), 2 ** (j + 1), torch.int64).double()
            o[L - 1] = x[h] * 2 ** j - o[:L - 1].sum(0)
            pmh = float(3.0 * torch.randn(1, generator=g))
            s = torch.arange(NS)
            pm[h] = torch.where((s + h) % 2 == 0, torch.full((), MRG_DEAD_PM), torch.full((), pmh - 200.0))
            pl[h] = torch.where((s + h) % 2 == 0, torch.zeros(()), torch.full((), 3.0))
            pm[h, at], pl[h, at], po[h, at] = pmh, a.float(), o.float()
    d.live = live
    d.pm, d.pl, d.po = pm.float(), pl.float(), torch.where(live.view(H, NS, 1), po.float(), dead_po)
    nan = lambda n: torch.full((n,), NAN, dtype=F32)
    d.pm_buf, d.pl_buf = torch.cat([d.pm.reshape(-1), nan(PAD)]), torch.cat([d.pl.reshape(-1), nan(PAD)])
    d.po_buf = torch.cat([d.po.reshape(-1), nan(128)])
    d.x = torch.full((K,), NAN, dtype=BF)


MERGE_K = 256.0


def merge_ref(c, d, dtype=F64):
    """the merge of the contract in dtype -> (x [K] before its bf16 rounding, B [K]: the probe family's bound, module docstring)"""
    pm, pl, po = d.pm.to(dtype), d.pl.to(dtype), d.po.to(dtype)
    e = torch.exp(pm - pm.max(-1, keepdim=True).values)
    e = torch.where(e < 2.0 ** -149, torch.zeros((), dtype=dtype), e)      # a float32 number: e^-200 is 0
    den = (pl * e).sum(-1, keepdim=True)
    x = (po * e.unsqueeze(-1)).sum(1) / den
    B = MERGE_K * 2.0 ** -24 * (po.abs() * e.unsqueeze(-1)).sum(1) / den
    return x.reshape(-1), B.reshape(-1)


GRAN_TAIL = (2 << 32) | 0x7e7e7f7f      # the fill of the 16 granules after cmb_gran[K / 2]: not zero, its tag not 1


def granules(x):
    """int64 [K / 2]: the granules {tag 1, bf16 x[2 i], x[2 i + 1]} of the hand-off form for the merged x (fp64, bf16 values)"""
    b = bits(x.to(BF)).to(torch.int64) & 0xffff
    return (1 << 32) | b[0::2] | (b[1::2] << 16)


def x_prime(c, d, scale=1.0):
    """(x' the projection multiplies, x' before the RMSNorm = what x_out receives), fp64 [B][K]; scale: applied to rstd"""
    if c.merge:
        x = rbf64(merge_ref(c, d)[0]).view(1, c.K)
        return x, x
    x = d.xl
    if c.delta:
        x = rbf64(x + rbf64(d.dl))
    pre = x
    if c.norm:
        f32 = lambda t: t.float().double()
        rstd = scale / torch.sqrt((x * x).mean(-1, keepdim=True) + EPS32)
        x = rbf64(f32(rbf64(f32(x * rstd)) * d.gl))
    return x, pre


def ref_acc(d, xp):
    """fp64 [B][N]; rows that are unit vectors: the element they select (a sum of it and exact zeros)"""
    if d.kpos is not None:
        return xp[:, d.kpos]
    out = torch.empty(xp.shape[0], d.Wl.shape[0], dtype=F64)
    for r0 in range(0, d.Wl.shape[0], 2048):
        out[:, r0:r0 + 2048] = xp @ d.Wl[r0:r0 + 2048].double().T
    return out


def part_slot(c):
    """[N]: the partial that row n's logit competes in (usdm_gemv and the VALU form: blocks of 16 rows; matrix cores: 16-row tiles
    dealt round-robin to the workgroups)"""
    blk = torch.arange(c.N) // 16
    return blk % c.sel["kwg"] if c.mfma else blk


def partials(c, logits):
    """(val, idx) fp64 [B][written partials] of logits [B][N] (-inf where banned); the matrix-core form fills all of part_bs"""
    nw = c.part_bs if c.mfma else c.nparts
    val = torch.full((c.B, nw), -INF, dtype=F64)
    idx = torch.full((c.B, nw), float(NO_IDX), dtype=F64)
    slot, ids = part_slot(c), torch.arange(c.N)
    for s in range(c.nparts):
        m = slot == s
        if not bool(m.any()):
            continue
        lg = logits[:, m]
        best = lg.max(-1).values
        first = (lg == best.view(-1, 1)).float().argmax(-1)           # the lowest id among the ties
        val[:, s] = best
        idx[:, s] = torch.where(best > -INF, (ids[m][first] + c.idx_offset).double(), torch.full((), float(NO_IDX), dtype=F64))
    return val, idx


def expected(c, d, *, rbf, scale=1.0):
    """{"y": Exp, "part_val", "part_idx", "x_out"} of one launch with round_bf16 = rbf; d.acc_max for the CPU test"""
    B, nout = c.B, c.nout
    xp, xpre = x_prime(c, d, scale)
    acc = ref_acc(d, xp)
    d.acc_max = float(acc.abs().max())
    e = {"y": Exp((B + 1) * c.y_bs)}
    yi = torch.arange(B).view(-1, 1) * c.y_bs + torch.arange(nout).view(1, -1)
    if c.lm_head:
        logits = rbf64(acc)
        logits[:, d.banl.bool()] = -INF
        e["y"].put(yi, logits)
        val, idx = partials(c, logits)
        pi = torch.arange(B).view(-1, 1) * c.part_bs + torch.arange(val.shape[1]).view(1, -1)
        e["part_val"], e["part_idx"] = Exp((B + 1) * c.part_bs), Exp((B + 1) * c.part_bs)
        e["part_val"].put(pi, val)
        e["part_idx"].put(pi, idx)
    elif c.glu:
        o = torch.arange(nout)
        gate = (o // 16) * 32 + o % 16
        gv, uv = acc[:, gate], acc[:, gate + 16]
        e["y"].put(yi, swiglu_rbf_ref(gv, uv) if rbf else Fn.silu(gv) * uv, gv, uv)
    else:
        v = rbf64(acc) if rbf else acc
        if c.res:
            v = v + d.rl
            v = rbf64(v) if rbf else v
        e["y"].put(yi, v)
    if c.delta:
        e["x_out"] = Exp(c.K + PAD)
        e["x_out"].put(torch.arange(c.K), xpre[0])
    return e


# ---- usdm_gemv: the K ladder of an instantiation (UNR: its ring depth, threads: its workgroup)
def k_ladder(inst, small, fmt="bf16"):
    """u: the elements of one ring; t: the workgroup's first pass over x.  MXFP4 (K % 32 == 0): 2048 is the group boundary"""
    rw, glu, nwv = (4, False, 4) if inst == "lm" else inst
    t = 8 * 64 * nwv
    if fmt == "mxfp4":
        u = 2048 * fmt_ring_depth(rw, glu, fmt)
        ks = (32, 480, 512, 544, 2016, 2048, 2080, u - 32, u, u + 32, t, t + 32, 16384) if small else (480, 2080, u + 32, t + 32)
    else:
        u = 512 * fmt_ring_depth(rw, glu, fmt)
        ks = (8, 504, 512, 520, u - 8, u, u + 8, t, t + 8, 16384) if small else (504, u + 8, t + 8)
    return sorted(set(ks))


def ragged_k(fmt):
    """the first K with a ragged (FP8: redirected) last iteration; one iteration of 512"""
    return 480 if fmt == "mxfp4" else 504


def k_step(fmt):
    return 32 if fmt == "mxfp4" else 8


FMT_SEED = {"bf16": 0, "fp8": 100000, "mxfp4": 200000}
# The probe's cap (2 % of a case's elements may differ between its two references) is less than one element of the 37- and
# 48-output cases, so their seeds are ones at which no element sits on a rounding boundary of the reference (the CPU test checks it)
PROBE_SEED = {"bf16": 0, "fp8": 2, "mxfp4": 5}


def _shape(inst):
    if inst == "lm":
        return dict(N=LM_N, ban="none", inst=inst)
    return dict(N=VALU_INST[inst] * (2 if inst[1] else 1), glu=inst[1], inst=inst)


def is_small(inst):
    return inst == "lm" or inst in SMALL_INST


def _mk(name, inst, K, seed, nb=0, fmt="bf16", **kw):
    a = dict(_shape(inst), **kw)
    if a.get("glu") and a.get("kind", "int") == "int":
        a["kind"] = "swiglu"
    if nb:
        a.update(nb=nb, form=-1)
    return Case(_pre(fmt) + f"{inst_id(inst)} {name} K{K}" + (f" nb{nb}" if nb else ""), K=K, seed=seed + FMT_SEED[fmt], fmt=fmt, **a)


def _pre(fmt):
    return "" if fmt == "bf16" else fmt + " "


def _ks(inst, nb, fmt):
    """the K of a family: the instantiation's ladder; batched: the first ragged K and one step past the first pass over x"""
    if not nb:
        return k_ladder(inst, is_small(inst), fmt)
    return (ragged_k(fmt), 8 * 64 * (4 if inst == "lm" else inst[2]) + k_step(fmt))


def _seed(inst, j):
    return 1000 * (list(VALU_INST).index(inst) + 1 if inst != "lm" else 10) + j


def valu_plain_cases(inst, nb=0, fmt="bf16"):
    """plain with a residual (GLU: SwiGLU; lm_head: no ban) over the K ladder"""
    return [_mk("plain", inst, K, _seed(inst, j) + 50 * nb, nb, fmt, res=inst != "lm" and not inst[1]) for j, K in enumerate(_ks(inst, nb, fmt))]


def valu_norm_exact_cases(inst, nb=0, fmt="bf16"):
    return [_mk("norm-exact", inst, K, _seed(inst, j) + 100 + 50 * nb, nb, fmt, norm="exact", res=inst != "lm" and not inst[1])
            for j, K in enumerate(_ks(inst, nb, fmt))]


def valu_probe_cases(inst, nb=0, fmt="bf16"):
    t = 64 * (4 if inst == "lm" else inst[2])
    return [_mk("norm-probe", inst, K, _seed(inst, j) + 200 + 50 * nb + PROBE_SEED[fmt], nb, fmt, kind="probe", norm="probe")
            for j, K in enumerate((ragged_k(fmt), 8 * t + k_step(fmt)))]


BANS = ("none", "workgroup", "wave", "scattered", "last")           # "none": no ban array at all (a NULL pointer)


def lm_head_cases(nb=0, mfma=False, fmt="bf16"):
    """every ban pattern, in every form: the banning ones at a one-iteration and a ragged multi-iteration K (matrix cores: multiples of
    256), idx_offset != 0 on two; no ban array at K = 520 (matrix cores: K = 4096, the row-contiguous loads)"""
    out = []
    for j, ban in enumerate(BANS[1:]):
        K = (256, 3840)[j % 2] if mfma else (504, 2056)[j % 2]
        kw = dict(nb=nb, variant="hold", rt=16, **_mfma_form(1, fmt)) if mfma else (dict(nb=nb, form=-1) if nb else {})
        out.append(Case(_pre(fmt) + f"lm_head {ban} K{K}" + (f" nb{nb}" if nb else ""), N=LM_N, K=K, seed=11000 + j + 10 * nb + FMT_SEED[fmt], ban=ban,
                        idx_offset=(0, 70000)[j // 2], inst="lm", fmt=fmt, **kw))
    K = 4096 if mfma else 520
    kw = dict(nb=nb, variant="hold16-recut", rt=16, **_mfma_form(1, fmt)) if mfma else (dict(nb=nb, form=-1) if nb else {})
    out.append(Case(_pre(fmt) + f"lm_head none K{K}" + (f" nb{nb}" if nb else ""), N=LM_N, K=K, seed=11005 + 10 * nb + FMT_SEED[fmt], ban="none", idx_offset=123,
                    inst="lm", fmt=fmt, **kw))
    return out


def _mfma_form(form, fmt):
    """the matrix-core form of a case: usdm_gemv_fp8_mfma takes 0 where usdm_gemv_batch takes 1, and 5 as it is"""
    return dict(form=form) if fmt == "bf16" else dict(form=0 if form == 1 else form, mfma=True)


def delta_cases(inst):
    return [_mk("x_delta", inst, 2056, _seed(inst, 300), delta=True, res=True), _mk("x_delta+norm", inst, 2056, _seed(inst, 301), delta=True, norm="exact", res=True),
            _mk("x_delta", inst, 504, _seed(inst, 302), delta=True, res=True), _mk("x_delta+norm", inst, 8200, _seed(inst, 303), delta=True, norm="exact")]


def skip_cases(inst, fmt="bf16"):
    K = 544 if fmt == "mxfp4" else 520
    return [_mk("skip", inst, K, _seed(inst, 310), fmt=fmt, skip=True, res=True, delta=fmt == "bf16"),
            _mk("skip+norm", inst, K, _seed(inst, 311), fmt=fmt, skip=True, norm="exact")]


DELTA_INST = ((1, False, 4), (1, False, 16))
VALU_NB = (2, 3, 4)


# ---- usdm_gemv_batch on the matrix cores
MFMA_NB = (1, 5, 13, 16)
# (K, form, ks): the variant each reaches is asserted by the CPU test
MFMA_LADDER = ((256, 1, False), (3840, 1, False), (4096, 1, False), (4096, 3, False), (6144, 5, False), (16384, 5, False), (14336, 1, False),
               (14336, 3, False), (14336, 5, False), (14336, 1, True), (6144, 1, True), (16384, 1, True))
MFMA_LADDER_VARIANT = ("hold", "hold", "hold16-recut", "hold16-frag", "stream", "stream", "stream56-recut", "stream56-frag", "stream56-recut",
                       "ksplit", "ksplit", "ksplit")
N_SMALL = 37        # plain: five 8-row tiles (the launcher's loop takes the shortest workgroup); K split: three 16-row tiles, the last of 5 rows
N_RAGGED16 = 4085   # 256 tiles of 16 rows, the last of 5 (12-row tiles would need two rounds, 8-row tiles are no shorter)
N_ROWS12 = 6144
# SwiGLU: 48 outputs = six tiles of 8 gate + 8 up rows.  The packed layout has whole blocks of 16 gate + 16 up rows only (N % 32 == 0;
# N = 80, i.e. 40 outputs, would put the last up rows past W and is refused), so the output count is a multiple of 16 and no tile of
# 8 outputs can be ragged: 48 is deliberate, there is no ragged SwiGLU tile to reach
N_SWIGLU = 96


def mfma_ladder_cases(nb, fmt="bf16"):
    """N = 37 with a residual, in place (y16 = residual) in the round_bf16 launch, over every variant (FP8: all but the
    fragment-shaped form 3, which usdm_gemv_fp8_mfma does not have)"""
    return [Case(_pre(fmt) + f"mfma K{K} form{f}{' ks' if ks else ''} nb{nb}", N=N_SMALL, K=K, seed=20000 + 20 * j + nb + FMT_SEED[fmt], nb=nb, ks=ks, res=True,
                 inplace=True, variant=MFMA_LADDER_VARIANT[j], rt=16 if ks else 8, fmt=fmt, **_mfma_form(f, fmt))
            for j, (K, f, ks) in enumerate(MFMA_LADDER) if fmt == "bf16" or f != 3]


def mfma_tile_cases(nb, fmt="bf16"):
    """12-row tiles (N = 6144), ragged 16-row tiles (N = 4085), at a generic held K and on both K = 4096 load patterns (FP8: K = 4096
    on its forms 0 and 5, both with the re-cut loads)"""
    out = []
    third = (4096, 3, "hold16-frag") if fmt == "bf16" else (4096, 5, "hold16-recut")
    for i, (N, rt) in enumerate(((N_ROWS12, 12), (N_RAGGED16, 16))):
        for j, (K, f, v) in enumerate(((256, 1, "hold"), (4096, 1, "hold16-recut"), third)):
            out.append(Case(_pre(fmt) + f"mfma N{N} K{K} form{f} nb{nb}", N=N, K=K, seed=21000 + 10 * i + j + 100 * nb + FMT_SEED[fmt], nb=nb, res=True, inplace=True,
                            variant=v, rt=rt, fmt=fmt, **_mfma_form(f, fmt)))
    return out


def mfma_swiglu_cases(nb, fmt="bf16"):
    return [Case(_pre(fmt) + f"mfma swiglu K{K} form{f} nb{nb}", N=N_SWIGLU, K=K, seed=22000 + j + 10 * nb + FMT_SEED[fmt], nb=nb, glu=True, kind="swiglu", variant=v,
                 rt=16, fmt=fmt, **_mfma_form(f, fmt))
            for j, (K, f, v) in enumerate(((256, 1, "hold"), (4096, 1, "hold16-recut"), (4096, 3, "hold16-frag"), (6144, 5, "stream"))) if fmt == "bf16" or f != 3]


def mfma_norm_cases(nb, fmt="bf16"):
    """both RMSNorm families at K <= 4096 (the matrix-core form fuses the norm into the held activations only)"""
    out, s = [], FMT_SEED[fmt]
    for j, (K, f, v) in enumerate(((256, 1, "hold"), (3840, 1, "hold"), (4096, 1, "hold16-recut"), (4096, 3, "hold16-frag"))):
        if fmt != "bf16" and f == 3:
            continue
        out.append(Case(_pre(fmt) + f"mfma norm-exact K{K} form{f} nb{nb}", N=N_SMALL, K=K, seed=23000 + j + 10 * nb + s, nb=nb, norm="exact", res=True, variant=v,
                        rt=8, fmt=fmt, **_mfma_form(f, fmt)))
        out.append(Case(_pre(fmt) + f"mfma norm-probe K{K} form{f} nb{nb}", N=4096, K=K, seed=23500 + j + 10 * nb + s, nb=nb, kind="probe", norm="probe", variant=v,
                        rt=16, fmt=fmt, **_mfma_form(f, fmt)))   # N >= K: all of K
    out.append(Case(_pre(fmt) + f"mfma swiglu norm-exact K4096 nb{nb}", N=N_SWIGLU, K=4096, seed=23900 + nb + s, nb=nb, glu=True, kind="swiglu", norm="exact",
                    variant="hold16-recut", rt=16, fmt=fmt, **_mfma_form(1, fmt)))
    return out


FP8_MFMA_VARIANTS = ("hold", "hold16-recut", "stream", "stream56-recut", "ksplit")


# ---- usdm_gemv with the merged-attention input: GEMV_MRG on (1, false, 16) and (1, false, 4), GEMV_CMB on (1, false, 16)
MERGE_FORMS = ("mrg16", "mrg4", "cmb")
MERGE_INST = {"mrg16": (1, False, 16), "mrg4": (1, False, 4), "cmb": (1, False, 16)}
# (N, K).  mrg16: 1024 threads x 4 elements = 4096 per pass: one head (most threads idle, zero fill to Kpad), exactly one pass, a
# second pass of 32 threads, two passes.  mrg4: 1024 per pass, the last workgroup ragged (37 = 9 x 4 + 1, 4081 = 1020 x 4 + 1); 16384 is
# the K limit (128 heads).  cmb: the gather takes 1024 granules = 2048 elements per pass; K = 128: workgroup 0 alone combines
MERGE_SHAPES = {"mrg16": ((4096, 128), (4096, 4096), (4096, 4224), (4096, 8192)),
                "mrg4": ((37, 128), (37, 1024), (37, 1152), (37, 16384), (4081, 1024)),
                "cmb": ((4096, 128), (4096, 2048), (4096, 4096), (4096, 4224), (4096, 8192))}
# mrg: chunks of 8 splits with clamped loads; cmb: groups of four and a scalar tail, 64 lanes of weights
MERGE_NS = {"mrg16": (1, 7, 8, 9, 64), "mrg4": (1, 7, 8, 9, 64), "cmb": (1, 3, 4, 5, 21, 64)}
MERGE_NS_PAIR = {"mrg16": (7, 9), "mrg4": (7, 9), "cmb": (3, 5)}       # below and above a chunk / a group: at every shape
MERGE_NS_AT = {"mrg16": (4096, 4224), "mrg4": (37, 1152), "cmb": (4096, 4224)}      # the shape that runs the whole NS ladder
MERGE_VARIANTS = (dict(res=True), dict(res=True, inplace=True), dict())     # in place: y16 = residual in the round_bf16 launch
MERGE_PROBE = {"mrg16": ((4096, 4096, 9), (4096, 4096, 64)), "mrg4": ((37, 1152, 9), (37, 1152, 64), (4081, 1152, 9)),
               "cmb": ((4096, 4096, 5), (4096, 4096, 21), (4096, 4096, 64))}


def _merge_case(form, tag, N, K, NS, seed, **kw):
    return Case(f"{form} {tag} N{N} K{K} NS{NS}", N=N, K=K, seed=seed, merge="cmb" if form == "cmb" else "mrg", NS=NS, inst=MERGE_INST[form], **kw)


def merge_exact_cases(form, shape):
    """the exact family at one (N, K): the two NS either side of a chunk / group, the whole NS ladder at MERGE_NS_AT; plain, with a
    residual and with the residual in place by turns"""
    f, i = MERGE_FORMS.index(form), MERGE_SHAPES[form].index(shape)
    ns = MERGE_NS[form] if shape == MERGE_NS_AT[form] else MERGE_NS_PAIR[form]
    return [_merge_case(form, "exact", *shape, NS, 30000 + 1000 * f + 100 * i + NS, **MERGE_VARIANTS[(i + j) % 3]) for j, NS in enumerate(ns)]


def merge_skip_cases(form):
    N, K = MERGE_SHAPES[form][1]
    return [_merge_case(form, "skip", N, K, MERGE_NS_PAIR[form][1], 33000 + MERGE_FORMS.index(form), skip=True, res=True)]


def merge_probe_cases(form):
    """(the seeds: ones at which B is below half an ulp on >= 98 % of a case's elements, i.e. on all 37 of the small cases; the CPU
    test checks it)"""
    return [_merge_case(form, "probe", N, K, NS, 34000 + 1000 * MERGE_FORMS.index(form) + 100 * j, kind="probe", mfam="probe")
            for j, (N, K, NS) in enumerate(MERGE_PROBE[form])]


def merge_cases():
    """every case of tests/test_gemv_merge_exact_gpu.py"""
    return [c for form in MERGE_FORMS for c in [x for s in MERGE_SHAPES[form] for x in merge_exact_cases(form, s)] + merge_skip_cases(form) + merge_probe_cases(form)]


def quant_insts(fmt):
    """the instantiations a format reaches: MXFP4 has no lm_head mode"""
    return list(VALU_INST) + (["lm"] if fmt == "fp8" else [])


def quant_batch_insts(fmt):
    return BATCH_INST + (("lm",) if fmt == "fp8" else ())


def quant_cases():
    """every case of tests/test_gemv_quant_exact_gpu.py"""
    out = []
    for fmt in FMTS:
        for inst in quant_insts(fmt):
            out += valu_plain_cases(inst, fmt=fmt) + valu_norm_exact_cases(inst, fmt=fmt) + valu_probe_cases(inst, fmt=fmt)
        for inst in DELTA_INST:
            out += skip_cases(inst, fmt)
        for nb in VALU_NB:
            for inst in quant_batch_insts(fmt):
                out += valu_plain_cases(inst, nb, fmt) + valu_norm_exact_cases(inst, nb, fmt) + valu_probe_cases(inst, nb, fmt)
    out += lm_head_cases(fmt="fp8")
    for nb in VALU_NB:
        out += lm_head_cases(nb, fmt="fp8")
    for nb in MFMA_NB:
        out += (mfma_ladder_cases(nb, "fp8") + mfma_tile_cases(nb, "fp8") + mfma_swiglu_cases(nb, "fp8") + mfma_norm_cases(nb, "fp8")
                + lm_head_cases(nb, mfma=True, fmt="fp8"))
    return out


def all_cases():
    """every case of the GPU test, for the CPU test's conditions"""
    out = []
    for inst in list(VALU_INST) + ["lm"]:
        out += valu_plain_cases(inst) + valu_norm_exact_cases(inst) + valu_probe_cases(inst)
    out += lm_head_cases()
    for inst in DELTA_INST:
        out += delta_cases(inst) + skip_cases(inst)
    for nb in VALU_NB:
        for inst in BATCH_INST + ("lm",):
            out += valu_plain_cases(inst, nb) + valu_norm_exact_cases(inst, nb) + valu_probe_cases(inst, nb)
        out += lm_head_cases(nb)
    for nb in MFMA_NB:
        out += mfma_ladder_cases(nb) + mfma_tile_cases(nb) + mfma_swiglu_cases(nb) + mfma_norm_cases(nb) + lm_head_cases(nb, mfma=True)
    return out + quant_cases()
