"""Plain CPU reference of usdm_gemm and the inputs of tests/test_gemm_exact_gpu.py, checked themselves by tests/test_gemm_exact_cpu.py
against torch.nn.functional.  Written from the contract in include/usdm_hip.h (usdm_gemm_args), not from csrc/gemm.hip:

  acc[m][n] = sum_tap sum_c A[row(m, tap)][c + tap * a_tap_stride] * W[n][tap * Kc + c]
  row(m, tap) = m * a_row_mul + a_row_off + tap * a_row_step           (rows outside [0, rowsA) read as zero)
  v = alpha * acc + bias[n];  [round to bf16];  v = act(v);  v += residual;  [round to bf16];  store

Conventions
  * A and W are integers in {-3 ... 3}: every product and every partial sum is an integer far below 2^24, so the f32 accumulator of
    any kernel holds the TRUE sum whatever its accumulation order, and one fp64 reference serves every tile bit for bit.  Bias and
    residual are small integers and alpha = 0.5 in the plain cases, which therefore stay exact through the epilogue
    (tests/test_gemm_exact_cpu.py asserts max |acc| + max |bias| + max |res| < 2^24 for every case).
  * every operand sits in a buffer whose gaps hold NaN (0 * NaN = NaN): the columns past taps * Kc of each A and W row, one row
    after the last valid row of W (per group), bias and residual, and one row before and after the rows of A (per batch and
    source), A being a view that starts one row into its buffer.  A correct kernel touches none of it; all of it is allocated.
  * every output is pre-filled with the sentinel of tests/_glue_reference.py and is larger than what the kernel owns (ldc > N, one
    more row; transposed: one more column and row; split-K: c_split_stride > rows * ldc).  What the kernel owns must hold the
    reference, everything else the sentinel, bit for bit.
  * activations: the pre-activations alpha * acc + bias are exact (alpha = 2^-4, bias multiples of 0.25) multiples of 1/16 within
    +-20; the fp64 activation of them is the reference and the bound is 4 x what torch's own float32 evaluation loses against fp64
    on the whole grid of such values (GEMM_*_TORCH_FP32_ERR below, recomputed by the CPU test; the factor 4 covers the device's
    exp, rcp and log at one to two ulp each, as in tests/_glue_reference.py).
"""
import torch
import torch.nn.functional as Fn

from tests._glue_reference import BF, F32, F64, SENT32, bf16_of_f32_bound, bits, gen, is_sentinel, sentinel  # noqa: F401

NAN = float("nan")
ACT_NONE, ACT_GELU, ACT_SWIGLU, ACT_TANH, ACT_LOGCLAMP = 0, 1, 3, 4, 5
ACT_NAMES = {ACT_GELU: "gelu", ACT_SWIGLU: "swiglu", ACT_TANH: "tanh", ACT_LOGCLAMP: "logclamp"}

# sel: (BM, BN, loader, dtypes) - the dispatch at the end of gemm_impl.  reg: register-staged (reg8: 8 waves); dmaS: LDS-DMA with S
# stages of two 64-byte chunks (dma4x1: four stages of one chunk); pp: the 8-wave ping-pong ring of three 64-deep slots
TILES = {
    0: (128, 128, "reg", (BF, F32)), 1: (128, 64, "reg", (BF, F32)), 2: (64, 64, "reg", (BF, F32)), 3: (128, 128, "reg8", (BF, F32)),
    4: (128, 128, "dma2", (BF, F32)), 5: (64, 64, "dma2", (BF, F32)), 6: (128, 64, "dma2", (BF, F32)), 7: (64, 64, "dma3", (BF, F32)),
    8: (64, 64, "dma4", (BF, F32)), 9: (128, 128, "dma4x1", (BF, F32)), 10: (128, 64, "dma3", (BF, F32)), 11: (128, 128, "dma3", (BF, F32)),
    12: (256, 128, "pp", (BF,)), 13: (288, 128, "pp", (BF,)), 14: (128, 128, "pp", (BF,)),
}
DT_TILES = [(dt, t) for dt in (BF, F32) for t in sorted(TILES) if dt in TILES[t][3]]
PP_TILES = (12, 13, 14)


def dt_name(dt):
    return "bf16" if dt == BF else "f32"


def tile_id(p):
    return f"{dt_name(p[0])}-tile{p[1]:02d}"


def chunk(dt):
    """elements of a 64-byte K chunk; a K-step is two chunks"""
    return 32 if dt == BF else 16


def pad16(dt):
    """elements of 16 bytes: the launcher refuses strides that are no multiple of it"""
    return 8 if dt == BF else 4


def expected_tile(dt, sel, *, multi_tap=False, concat=False, transpose=False, head_split=False):
    """the tile the launcher runs when `sel` is forced (its documented reroutes)"""
    if multi_tap and sel >= 4 and not (sel >= 12 and concat):
        sel = 1 if sel in (6, 10) else (2 if sel in (5, 7, 8) else 0)       # the LDS-DMA tiles are single-tap
    if sel == 13 and (transpose or head_split):
        sel = 12                                                            # the 288-row tile has row-major epilogues only
    if dt == F32 and sel >= 12:
        sel = 2                                                             # the ping-pong tiles are bf16 only
    return sel


def ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen(seed)).double()


def rbf64(x):
    """fp64 -> the nearest bf16 value (8 significant bits, ties to even), exactly, as fp64"""
    _, e = torch.frexp(x)
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    return torch.round(x / ulp) * ulp


def bf16_ulp(x):
    """the spacing of bf16 values at |x| (fp64)"""
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 8)


# ------------------------------------------------------------------------------------------------------------------ activations
LOG_FLOOR = float(torch.tensor(1e-5, dtype=F32))
ACT_GRID = torch.arange(-320, 321, dtype=F64) / 16          # every multiple of 1/16 in [-20, 20]: a superset of the cases' pre-activations
# worst |torch float32 - fp64| / normaliser over ACT_GRID (SwiGLU: over ACT_GRID x ACT_GRID); the normaliser of each is act_norm()
GEMM_GELU_TORCH_FP32_ERR = 2.0e-7       # per max(1, |x|)          measured on the CPU: 1.87e-7
GEMM_TANH_TORCH_FP32_ERR = 3.2e-8       # absolute (|tanh| <= 1)   measured on the CPU: 2.96e-8
GEMM_LOGCLAMP_TORCH_FP32_ERR = 6.4e-8   # per max(1, |ref|)        measured on the CPU: 5.89e-8
GEMM_SWIGLU_TORCH_FP32_ERR = 1.65e-7    # per max(|ref|, |u|)      measured on the CPU: 1.54e-7
ACT_ERR = {ACT_GELU: GEMM_GELU_TORCH_FP32_ERR, ACT_TANH: GEMM_TANH_TORCH_FP32_ERR, ACT_LOGCLAMP: GEMM_LOGCLAMP_TORCH_FP32_ERR,
           ACT_SWIGLU: GEMM_SWIGLU_TORCH_FP32_ERR}
FLIP_CAP = 2e-3                          # share of outputs a chain of bf16 roundings may flip (tests/test_kernels_gpu.py)


def act_ref(act, x, u=None, dtype=F64):
    """the activation of the pre-activation x (SwiGLU: gate x, up u) evaluated by torch in `dtype`"""
    x = x.to(dtype)
    if act == ACT_GELU:
        return Fn.gelu(x)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_LOGCLAMP:
        return torch.log(torch.clamp(x, min=LOG_FLOOR))
    if act == ACT_SWIGLU:
        return Fn.silu(x) * u.to(dtype)
    return x


def act_norm(act, x, ref, u=None):
    """what an activation's error is measured against; depends on the pre-activation and the fp64 reference only"""
    if act == ACT_GELU:
        return x.abs().clamp(min=1.0)                       # max(1, |x|)
    if act == ACT_TANH:
        return torch.ones_like(x)                           # 1
    if act == ACT_LOGCLAMP:
        return ref.abs().clamp(min=1.0)                     # max(1, |ref|)
    if act == ACT_SWIGLU:
        return torch.maximum(ref.abs(), u.abs())            # max(|ref|, |u|)
    raise ValueError(act)


def act_torch_err(act):
    x, u = ACT_GRID, None
    if act == ACT_SWIGLU:
        x, u = ACT_GRID.view(-1, 1).expand(-1, ACT_GRID.numel()), ACT_GRID.view(1, -1).expand(ACT_GRID.numel(), -1)
        keep = u != 0                                       # (u = 0: ref = 0 = the float32 result, and the normaliser is 0)
        x, u = x[keep], u[keep]
    ref = act_ref(act, x, u)
    got = act_ref(act, x, u, dtype=F32).double()
    return float(((got - ref).abs() / act_norm(act, x, ref, u)).max())


def swiglu_rbf_ref(g, u, dtype=F64):
    """silu_mul with round_bf16: bf16(bf16(silu(bf16(g))) * bf16(u)); fp64 with exact roundings, or torch float32 / bfloat16"""
    if dtype == F64:
        g, u = rbf64(g.double()), rbf64(u.double())
        return rbf64(rbf64(g / (1.0 + torch.exp(-g))) * u)
    r = lambda t: t.to(BF).float()
    g, u = r(g.float()), r(u.float())
    return r(r(g / (1.0 + torch.exp(-g))) * u).double()


# ------------------------------------------------------------------------------------------------------------------ cases
class Exp:
    """what one output buffer must hold: vals (fp64, flat), owned (bool, flat: the kernel writes these and nothing else), and for the
    activation cases the exact pre-activation (and SwiGLU's up value) of every owned element"""

    def __init__(self, size):
        self.vals, self.owned = torch.zeros(size, dtype=F64), torch.zeros(size, dtype=torch.bool)
        self.pre, self.up = torch.zeros(size, dtype=F64), torch.zeros(size, dtype=F64)

    def put(self, idx, vals, pre=None, up=None):
        idx = idx.reshape(-1)
        assert not bool(self.owned[idx].any()) and idx.unique().numel() == idx.numel(), "two writers of one output element"
        self.vals[idx], self.owned[idx] = vals.reshape(-1), True
        if pre is not None:
            self.pre[idx] = pre.reshape(-1)
        if up is not None:
            self.up[idx] = up.reshape(-1)


class Case:
    """one launch (or several into one output: launches) with its guarded buffers.  kw: the scalar keywords of ops.gemm."""

    def __init__(self, name, dt):
        self.name, self.dt = name, dt
        self.launches = []          # [(kw, W flat, Wvals logical)]
        self.A = self.bias = self.res = None
        self.A_off = 0
        self.want32 = self.want16 = False
        self.out_size = 0
        self.qkv = None             # dict(B, S, Spad, H, D, q_off, k_off)
        self.stats = False
        self.exact = True
        self._exp = None

    @property
    def kw(self):
        return self.launches[0][0]

    def __repr__(self):
        return self.name


def _a_index(kw, b, g, tap, M):
    """(flat indices [M, Kc] into the A view, validity [M]) of A[row(m, tap)][c + tap * a_tap_stride] for group g of batch b"""
    m, c = torch.arange(M), torch.arange(kw["Kc"])
    row = m * kw["a_row_mul"] + kw["a_row_off"] + tap * kw["a_row_step"]
    ok = (row >= 0) & (row < kw["rowsA"])
    base = kw["a_gstride"] * g + kw["a_bstride"] * b + tap * kw["a_tap_stride"]
    return base + row.clamp(0, kw["rowsA"] - 1).view(-1, 1) * kw["lda"] + c.view(1, -1), ok


def ref_acc(c, kw, W):
    """fp64 [batch, groups, M, N] of the header's sum (products of integers: exact)"""
    A, W = c.A.double()[c.A_off:], W.double()
    B, G, M, N, Kc = kw["batch"], kw["groups"], kw["M"], kw["N"], kw["Kc"]
    acc = torch.zeros(B, G, M, N, dtype=F64)
    n, cc = torch.arange(N), torch.arange(Kc)
    for b in range(B):
        for g in range(G):
            for tap in range(kw["taps"]):
                idx, ok = _a_index(kw, b, g, tap, M)
                a = torch.where(ok.view(-1, 1), A[idx], torch.zeros((), dtype=F64))
                w = W[kw["w_gstride"] * g + n.view(-1, 1) * kw["ldw"] + tap * Kc + cc.view(1, -1)]
                acc[b, g] += a @ w.T
    return acc


def out_rows(kw):
    """[batch, M]: (b * c_bstride + m) * c_row_mul + c_row_off"""
    b, m = torch.arange(kw["batch"]).view(-1, 1), torch.arange(kw["M"]).view(1, -1)
    return (b * kw["c_bstride"] + m) * kw["c_row_mul"] + kw["c_row_off"]


def out_cols(kw):
    """[groups, N]: g * c_gcol + n (bias, residual and output alike)"""
    return torch.arange(kw["groups"]).view(-1, 1) * kw["c_gcol"] + torch.arange(kw["N"]).view(1, -1)


def expected(c):
    """{"out" | "q", "k", "v" | "stats": Exp} of the case, and c.acc_max / c.finite for the CPU test"""
    if c._exp is not None:
        return c._exp
    e = {}
    c.acc_max = 0.0
    for kw, W, _ in c.launches:
        acc = ref_acc(c, kw, W)
        c.acc_max = max(c.acc_max, float(acc.abs().max()))
        rows, cols = out_rows(kw), out_cols(kw)                       # [B, M], [G, N]
        R, Cn = rows.view(kw["batch"], 1, -1, 1), cols.view(1, kw["groups"], 1, -1)
        pre = kw["alpha"] * acc + (c.bias.double()[Cn] if c.bias is not None else 0.0)
        rbf, act = kw["round_bf16"], kw["act"]
        if c.qkv is not None:
            q = c.qkv
            HD = q["H"] * q["D"]
            v = rbf64(pre[0, 0]) if rbf else pre[0, 0]                # [M, 3 H D], m = b * S + s
            v = v.view(q["B"], q["S"], 3, q["H"], q["D"])
            b_, s_, h_, d_ = torch.meshgrid(torch.arange(q["B"]), torch.arange(q["S"]), torch.arange(q["H"]), torch.arange(q["D"]), indexing="ij")
            qk_idx = ((b_ * q["H"] + h_) * q["Spad"] + s_) * q["D"] + d_                 # [B][H][Spad][D]
            v_idx = ((b_ * q["H"] + h_) * q["D"] + d_) * q["Spad"] + s_                  # [B][H][D][Spad]
            for name, part, idx, size in (("q", 0, qk_idx, q["B"] * HD * q["Spad"] + q["D"]), ("k", 1, qk_idx, q["B"] * HD * q["Spad"] + q["D"]),
                                          ("v", 2, v_idx, q["B"] * HD * q["Spad"] + q["Spad"])):
                e[name] = Exp(size)
                e[name].put(idx, v[:, :, part])
            continue
        out = e.setdefault("out", Exp(c.out_size))
        if act == ACT_SWIGLU:
            assert kw["groups"] == 1 and kw["batch"] == 1
            j = torch.arange(kw["N"] // 2)
            gate = (j // 16) * 32 + j % 16                            # blocks of 32 rows of W: 16 gate rows, then their 16 up rows
            gv, uv = pre[0, 0][:, gate], pre[0, 0][:, gate + 16]
            val = swiglu_rbf_ref(gv, uv) if rbf else act_ref(act, gv, uv)
            out.put(rows.view(-1, 1) * kw["ldc"] + j.view(1, -1), val, gv, uv)
            continue
        if rbf:
            pre = rbf64(pre)
        v = act_ref(act, pre)
        if c.res is not None:
            v = v + c.res.double()[R * kw["ldr"] + Cn]
            if rbf:
                v = rbf64(v)
        oi = (Cn * kw["ldc"] + R) if kw["transpose_out"] else (R * kw["ldc"] + Cn)
        out.put(oi.expand_as(v), v, pre)
        if c.stats:                                                   # per row and 128-column tile: (sum, M2 about the tile's mean)
            nt = kw["N"] // 128
            t = v[0, 0].view(kw["M"], nt, 128)
            s1 = t.sum(-1)
            m2 = (t - (s1 / 128).unsqueeze(-1)).pow(2).sum(-1)
            st = e.setdefault("stats", Exp(c.stats_size))
            si = (rows.view(-1, 1) * nt + torch.arange(nt).view(1, -1)) * 2
            st.put(torch.stack([si, si + 1], -1), torch.stack([s1, m2], -1))
    c.finite = all(bool(torch.isfinite(x.vals).all()) for x in e.values())
    c._exp = e
    return e


def make(name, dt, *, M, N, Kc, seed, taps=1, rowsA=None, a_row_mul=1, a_row_off=0, a_row_step=0, sources=1, groups=1, batch=1,
         c_gcol=None, bias=True, bias_q=1.0, bias_hi=8, alpha=0.5, act=ACT_NONE, round_bf16=False, res=None, out32=True, out16=True,
         ldc=None, c_row_mul=1, c_row_off=0, c_bgap=3, transpose=False, split_k=0, qkv=None, stats=False, Avals=None, Wvals=None, phases=None):
    """Build a case.  Avals [sources, batch, rowsA, groups * Kc] and Wvals [groups, N, taps * Kc] (one per phase) are the logical
    operands (random integers in {-3 ... 3} when not given); phases: per-launch overrides of kw (ConvTranspose1d)."""
    c = Case(name, dt)
    rowsA = M if rowsA is None else rowsA
    if sources > 1:
        taps = sources
    p = pad16(dt)
    # ---- A: [1 NaN row] + per (source, batch): rowsA rows + 1 NaN row; columns past groups * Kc are NaN; the view starts at row 1
    ka = groups * Kc
    lda = ka + p
    c.Avals = ints((sources, batch, rowsA, ka), seed) if Avals is None else Avals.double()
    buf = torch.full((1 + sources * batch * (rowsA + 1), lda), NAN, dtype=F64)
    for s in range(sources):
        for b in range(batch):
            r0 = 1 + (s * batch + b) * (rowsA + 1)
            buf[r0:r0 + rowsA, :ka] = c.Avals[s, b]
    c.A, c.A_off = buf.to(dt).reshape(-1), lda
    # ---- W: per group N rows + 1 NaN row; columns past taps * Kc are NaN
    kt = taps * Kc
    ldw = kt + p
    nph = len(phases) if phases else 1
    Wl = [ints((groups, N, kt), seed + 1 + i) for i in range(nph)] if Wvals is None else [w.double() for w in Wvals]
    # ---- output geometry
    c_gcol = (N if c_gcol is None else c_gcol) if groups > 1 else 0
    c_bstride = (M + c_bgap) if batch > 1 else 0
    kw = dict(M=M, N=N, Kc=Kc, taps=taps, lda=lda, rowsA=rowsA, a_row_mul=a_row_mul, a_row_off=a_row_off, a_row_step=a_row_step,
              a_tap_stride=(batch * (rowsA + 1) * lda if sources > 1 else 0), ldw=ldw, groups=groups, batch=batch,
              a_gstride=(Kc if groups > 1 else 0), w_gstride=(N + 1) * ldw, a_bstride=(rowsA + 1) * lda, c_gcol=c_gcol, c_bstride=c_bstride,
              alpha=alpha, act=act, round_bf16=bool(round_bf16), ldr=0, ldc=0, c_row_mul=c_row_mul, c_row_off=c_row_off,
              transpose_out=bool(transpose), split_k=split_k, c_split_stride=0)
    kws = [dict(kw, **ph) for ph in phases] if phases else [kw]
    width = (groups - 1) * c_gcol + N
    nrows = max(int(out_rows(k).max()) for k in kws) + 1
    cols = out_cols(kw)
    if bias:
        c.bias = torch.full((width + 4,), NAN, dtype=F32)
        c.bias[cols.reshape(-1)] = (ints((cols.numel(),), seed + 20, -bias_hi, bias_hi) * bias_q).float()
    if qkv is not None:
        c.qkv = dict(qkv)
        ldc = N
    elif act == ACT_SWIGLU:
        ldc = N // 2 + 4 if ldc is None else ldc
        c.out_size = (nrows + 1) * ldc
    elif transpose:
        assert ldc is not None and ldc > nrows
        c.out_size = (width + 1) * ldc
    else:
        ldc = ((width + 3) // 4 * 4 + 4) if ldc is None else ldc
        c.out_size = (nrows + 1) * ldc
    if res is not None:
        ldr = (width + 3) // 4 * 4 + 4
        rb = torch.full(((nrows + 1) * ldr,), NAN, dtype=F64)
        for k in kws:
            ri = (out_rows(k).view(batch, 1, M, 1) * ldr + cols.view(1, groups, 1, N)).reshape(-1)
            rb[ri] = ints((ri.numel(),), seed + 30, -8, 8)
        c.res = rb.to(res)
        for k in kws:
            k["ldr"] = ldr
    if stats:
        c.stats, c.stats_size = True, (nrows + 1) * (N // 128) * 2
    if split_k:
        c.part_size = c.out_size
        c.out_size = split_k * (c.part_size + 4)
        for k in kws:
            k["c_split_stride"] = c.part_size + 4
    for k, w in zip(kws, Wl):
        k["ldc"] = ldc
        wb = torch.full((groups * (N + 1), ldw), NAN, dtype=F64)
        for g in range(groups):
            wb[g * (N + 1):g * (N + 1) + N, :kt] = w[g]
        c.launches.append((k, wb.to(dt).reshape(-1), w))
    c.want32, c.want16 = out32, out16
    c.exact = act == ACT_NONE
    return c


def _mn(BM, BN):
    return BM + 37, BN + 68


# a. ---- K ladder: 1/2, 1, 1 1/2, 2, 3, 4 1/2, 5 1/2, 7 1/2, 8 1/2 K-steps (below, at and above every pipeline depth; half-step tails on
#         the ring's prologue, steady state and drain)
K_LADDER = (32, 64, 96, 128, 192, 288, 352, 480, 544)       # bf16; f32: half of each


def k_of(dt, k_bf16):
    return k_bf16 if dt == BF else k_bf16 // 2


def k_ladder_cases(dt, BM, BN):
    M, N = _mn(BM, BN)
    return [make(f"K{k_of(dt, k)}", dt, M=M, N=N, Kc=k_of(dt, k), seed=100 + i, res=F32) for i, k in enumerate(K_LADDER)]


# b. ---- edges at 3 1/2 K-steps
def edge_cases(dt, BM, BN):
    K = k_of(dt, 224)
    M, N = _mn(BM, BN)
    mk = lambda name, seed, **kw: make(name, dt, **dict(dict(M=M, N=N, Kc=K, seed=seed, res=F32), **kw))
    return [
        mk("M1", 200, M=1), mk("M=BM", 201, M=BM), mk("M=BM+1", 202, M=BM + 1),
        mk("12tiles", 203, M=2 * BM + 5, N=3 * BN + 4),                      # the XCD remap has q = 1, r = 4
        mk("N+69,ldc=N+3", 204, N=BN + 69, ldc=BN + 72),                     # vectorised; the last thread owns one column
        mk("N+69,ldc=N", 205, N=BN + 69, ldc=BN + 69),                       # the scalar path everywhere
        mk("res16", 206, res=BF),
        # two rounding points; a bias up to +-1000 (11 bits) so that either one changes most outputs, at the short K of f32 as well
        mk("round_bf16+res", 207, res=F32, round_bf16=True, bias_hi=1000), mk("round_bf16+res16", 208, res=BF, round_bf16=True, bias_hi=1000),
        mk("out16-only", 209, out32=False), mk("out32-only", 210, out16=False),
        mk("no-bias-no-res", 211, bias=False, res=None),
        mk("batch2,row_mul2", 212, batch=2, c_row_mul=2, c_row_off=1),       # the even output rows keep the sentinel
        mk("groups2,gcol%4=0", 213, groups=2, c_gcol=N + 4), mk("groups2,gcol%4=2", 214, groups=2, c_gcol=N + 2),
    ]


# c. ---- transposed output
def transposed_cases(dt, BM, BN):
    K = k_of(dt, 224)
    M, N = _mn(BM, BN)                                                       # M % 4 == 1
    return [make(f"T,ldc={ldc}", dt, M=M, N=N, Kc=K, seed=300 + i, res=F32, transpose=True, ldc=ldc) for i, ldc in enumerate((M + 3, M + 2))]


# d. ---- head-split epilogue: H = 3, D = 64 (a 128-column tile straddles the Q / K boundary at 192), B = 2, S = BM / 2 + 21 (odd; the
#         sequence boundary falls inside the first tile)
def head_split_cases(dt, BM, BN, pp=False):
    K = k_of(dt, 224)
    H, D, B, S = 3, 64, 2, BM // 2 + 21
    q = dict(B=B, S=S, Spad=(S + 63) // 64 * 64, H=H, D=D, q_off=0, k_off=0)
    out = [make("qkv+bias", dt, M=B * S, N=3 * H * D, Kc=K, seed=400, qkv=q), make("qkv", dt, M=B * S, N=3 * H * D, Kc=K, seed=401, qkv=q, bias=False),
           make("qkv+round_bf16", dt, M=B * S, N=3 * H * D, Kc=K, seed=402, qkv=q, round_bf16=True, bias_hi=1000)]
    if pp:      # q or k 8 but not 16 bytes aligned: the narrow path of the ping-pong tiles
        out += [make("qkv,q+8B", dt, M=B * S, N=3 * H * D, Kc=K, seed=403, qkv=dict(q, q_off=4)),
                make("qkv,k+8B", dt, M=B * S, N=3 * H * D, Kc=K, seed=404, qkv=dict(q, k_off=4))]
    return out


# e. ---- split-K: equal shares, a short last share, empty shares (chunks of 64 bytes: 8 / 2, 2 / 3, 9 / 3, 5 / 4, 12 / 16)
SPLIT_K = ((2, 256), (3, 64), (3, 288), (4, 160), (16, 384))   # (S, bf16 K); f32: half the K


def split_k_cases(dt, BM, BN):
    M, N = _mn(BM, BN)
    return [make(f"S{S},K{k_of(dt, k)}", dt, M=M, N=N, Kc=k_of(dt, k), seed=500 + i, res=F32, out16=False, split_k=S) for i, (S, k) in enumerate(SPLIT_K)]


# f. ---- multi-tap operands
def conv_case(name, dt, BM, BN, seed, *, k, dil=1, stride=1, same=True, Cin=None, G=1, B=1):
    """Conv1d on channels-last activations; M = output length (two tiles with a ragged end), N = output channels per group"""
    Cin = chunk(dt) * 2 if Cin is None else Cin
    M, N = BM + 37, BN + 4
    pad = (k - 1) * dil // 2 if same else 0
    T = (M - 1) * stride + (k - 1) * dil + 1 - 2 * pad
    c = make(name, dt, M=M, N=N, Kc=Cin, seed=seed, taps=k, rowsA=T, a_row_mul=stride, a_row_off=-pad, a_row_step=dil, groups=G, batch=B, res=F32)
    c.conv = dict(k=k, dil=dil, stride=stride, pad=pad, G=G, Cin=Cin)
    return c


def conv_torch(c):
    """fp64 [B, M, G * N] of the same convolution by torch.nn.functional.conv1d on the logical operands (no bias)"""
    v, kw, W = c.conv, c.kw, c.launches[0][2]
    x = c.Avals[0].permute(0, 2, 1)                                                       # [B, G * Cin, T]
    w = W.view(v["G"] * kw["N"], v["k"], v["Cin"]).permute(0, 2, 1)                       # [G * N, Cin, k]
    return Fn.conv1d(x, w, None, stride=v["stride"], padding=v["pad"], dilation=v["dil"], groups=v["G"]).permute(0, 2, 1)


def conv_transpose_case(dt, BM, BN, seed=610, k=8, u=4):
    """ConvTranspose1d(k = 2 u, stride u, padding (k - u) / 2) as u two-tap phase GEMMs into one buffer of T * u rows"""
    Cin, T, N = chunk(dt), BM + 37, BN + 4
    pad = (k - u) // 2
    w = ints((Cin, N, k), seed + 7)                                                       # torch's [Cin, Cout, k]
    phases, Wl = [], []
    for ph in range(u):
        js = sorted((j for j in range(k) if (ph + pad - j) % u == 0), key=lambda j: (ph + pad - j) // u)   # ascending input offset
        offs = [(ph + pad - j) // u for j in js]
        assert len(js) == 2 and offs[1] - offs[0] == 1
        phases.append(dict(a_row_off=offs[0], c_row_off=ph))
        Wl.append(torch.stack([w[:, :, j].T for j in js], dim=1).reshape(1, N, 2 * Cin))
    c = make("convT k8 u4", dt, M=T, N=N, Kc=Cin, seed=seed, taps=2, rowsA=T, a_row_step=1, c_row_mul=u, res=F32, Wvals=Wl, phases=phases)
    c.convT = dict(w=w, u=u, pad=pad)
    return c


def concat_case(dt, BM, BN, seed=620):
    """Linear over two sources concatenated along K (a_tap_stride, a_row_step = 0); Kc % 64 == 0, so the ping-pong tiles serve it too"""
    M, N = _mn(BM, BN)
    return make("cat2", dt, M=M, N=N, Kc=64, seed=seed, sources=2, res=F32)


def multi_tap_cases(dt, BM, BN):
    return [conv_case("conv k3", dt, BM, BN, 600, k=3), conv_case("conv k7 d3", dt, BM, BN, 601, k=7, dil=3, Cin=chunk(dt)),
            conv_case("conv k3 s2", dt, BM, BN, 602, k=3, stride=2, same=False), conv_transpose_case(dt, BM, BN),
            conv_case("conv k5 G3 B2", dt, BM, BN, 603, k=5, G=3, B=2, Cin=chunk(dt)), concat_case(dt, BM, BN)]


# g. ---- activations: alpha = 2^-4, bias multiples of 0.25 within +-1, K = 128: exact pre-activations, multiples of 1/16, sigma about 2.8
def activation_cases(dt, BM, BN):
    M, N = _mn(BM, BN)                                                       # N % 8 == 4
    mk = lambda name, seed, **kw: make(name, dt, **dict(dict(M=M, N=N, Kc=128, seed=seed, alpha=2.0 ** -4, bias_q=0.25, bias_hi=4), **kw))
    return [
        mk("gelu", 700, act=ACT_GELU),
        mk("gelu,out16,ldc%8=0", 701, act=ACT_GELU, out32=False, ldc=N + 4),   # the packed 16-byte path of the ping-pong tiles (full tiles)
        mk("gelu,out16,ldc%8=4", 702, act=ACT_GELU, out32=False, ldc=N + 8),   # the generic path
        mk("gelu+res", 703, act=ACT_GELU, res=F32), mk("gelu,T", 704, act=ACT_GELU, res=F32, transpose=True, ldc=M + 3),
        mk("tanh", 705, act=ACT_TANH), mk("logclamp", 706, act=ACT_LOGCLAMP), mk("tanh,ldc=N", 707, act=ACT_TANH, N=BN + 69, ldc=BN + 69),
        mk("swiglu", 708, act=ACT_SWIGLU, N=BN + 32), mk("swiglu+round_bf16", 709, act=ACT_SWIGLU, N=BN + 32, round_bf16=True),
    ]


# h. ---- folded-LayerNorm producer (ping-pong tiles): ragged M, N = 256
def stats_cases(dt, BM, BN):
    return [make("stats", dt, M=BM + 37, N=256, Kc=224, seed=800, res=F32, out16=False, stats=True, ldc=260)]


GROUPS = dict(k_ladder=k_ladder_cases, edges=edge_cases, transposed=transposed_cases, head_split=head_split_cases, split_k=split_k_cases,
              multi_tap=multi_tap_cases, activations=activation_cases)
M2_BOUND = 16 * 2.0 ** -24      # x M2_ref: one rounding per square, at most nine per sum of non-negative terms


# ------------------------------------------------------------------------------------------------------------------ checks
def check_exact(what, got, exp):
    """got (a flat CPU tensor, f32 or bf16) holds the reference on every owned element and the sentinel everywhere else, bit for bit"""
    want = exp.vals.to(got.dtype)
    assert bool((want.double() == exp.vals)[exp.owned].all()) or got.dtype == BF, f"{what}: the reference is not exact in float32"
    stray = ~is_sentinel(got) & ~exp.owned
    assert not bool(stray.any()), f"{what}: {int(stray.sum())} elements written outside what the kernel owns, first at {int(stray.nonzero()[0])}"
    kept = is_sentinel(got) & exp.owned & (bits(want) != bits(sentinel((1,), got.dtype)))
    assert not bool(kept.any()), f"{what}: {int(kept.sum())} owned elements never written, first at {int(kept.nonzero()[0])}"
    bad = (bits(got) != bits(want)) & exp.owned
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(exp.owned.sum())} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


def check_guard(what, got, exp, tol=0.0):
    """the sentinel outside the owned elements, none left inside (outputs that are compared within the bound tol: an owned f32 element
    whose reference is within tol of the sentinel's value may hold its bits)"""
    stray = ~is_sentinel(got) & ~exp.owned
    assert not bool(stray.any()), f"{what}: {int(stray.sum())} elements written outside what the kernel owns, first at {int(stray.nonzero()[0])}"
    kept = is_sentinel(got) & exp.owned
    if got.dtype != BF:
        kept &= (exp.vals - SENT32).abs() > tol
    assert not bool(kept.any()), f"{what}: {int(kept.sum())} owned elements never written, first at {int(kept.nonzero()[0])}"


def act_tolerance(act, exp):
    """fp64, flat: 4 x the recorded float32 error x the activation's normaliser, on the owned elements (0 elsewhere)"""
    return 4.0 * ACT_ERR[act] * torch.where(exp.owned, act_norm(act, exp.pre, exp.vals, exp.up), torch.zeros((), dtype=F64))
