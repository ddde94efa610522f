"""Thin per-kernel wrappers over the C-ABI (torch tensors in, device pointers out).

These exist for the parity tests and for the Python drop-ins; they add no arithmetic.
"""
import ctypes as C_      # (C is the channel count in several wrappers' keywords)
import os

import torch

from . import _lib
from ._lib import (BF16, F32, AttnVerifyArgs, AttnVerifyBatchArgs, SpecArgs, SpecBatchArgs, SpecSampleArgs, BeamArgs, KvExpandArgs, KvReorderArgs, AttnArgs, AttnDecodeArgs, AttnDecodeFp8Args, RopeFp8Args, DecodeState, GemmArgs, GemvArgs, GemvBatchArgs, GemvFp8Args, GemvMxfp4Args, GemvMxfp4MfmaArgs, LogitEditArgs, LogprobArgs, NormArgs, PenaltyArgs, PromptLogprobArgs, RopeArgs, SampleArgs, SnakeArgs,
                   VbInputArgs, VbSolverArgs, check, lib)
from .quant import Fp8Weight, Mxfp4Weight
from .wpack import GemvWpack

if lib.usdm_sizeof_gemv_wpack() != C_.sizeof(GemvWpack):
    raise ImportError(f"ABI mismatch: usdm_gemv_wpack is {lib.usdm_sizeof_gemv_wpack()} bytes in the library, {C_.sizeof(GemvWpack)} in Python")


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    """A recorded sequence of C-ABI launches with their argument structs pre-built.

    Python builds the structs once per shape; run() is then a tight loop of ctypes calls on the
    current HIP stream (and is what gets captured into a hipGraph by usdm_amd.graph.GraphedPlan)."""

    def __init__(self):
        self.calls = []
        self.keep = []  # tensors that must outlive the plan (workspaces, packed weights)

    def add(self, what, fn, *args):
        self.calls.append((what, fn, args))

    def hold(self, *tensors):
        self.keep.extend(tensors)
        return tensors[0] if len(tensors) == 1 else tensors

    def run(self):
        st = _stream()
        for what, fn, args in self.calls:
            rc = fn(*args, st)
            if rc != 0:
                check(rc, what)

    def __len__(self):
        return len(self.calls)


def _go(plan, what, fn, *args):
    if plan is not None:
        plan.add(what, fn, *args)
    else:
        check(fn(*args, _stream()), what)


def _ptr(t):
    return C_.c_void_p(t.data_ptr()) if t is not None else C_.c_void_p(0)


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported dtype {t.dtype}")


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.UsdmError("usdm_amd kernels run on the GPU only (no CPU fallback); got a CPU tensor")


def gemm(A, W, *, M, N, Kc, taps=1, lda=None, rowsA=None, a_row_mul=1, a_row_off=0, a_row_step=0,
         a_tap_stride=0, ldw=None, groups=1, batch=1, a_gstride=0, w_gstride=0, a_bstride=0, c_gcol=0,
         c_bstride=0, bias=None, alpha=1.0, act=0, round_bf16=False, residual=None, ldr=0,
         out32=None, out16=None, ldc=None, c_row_mul=1, c_row_off=0, transpose_out=False,
         qkv=None, split_k=0, c_split_stride=0, stats_out=None, ln=None, plan=None, tile_query=False):
    """Raw launch of usdm_gemm; see include/usdm_hip.h for the meaning of every field."""
    _need_cuda(A, W, bias, residual, out32, out16)
    a = GemmArgs()
    a.dtype = _dt(A)
    assert W.dtype == A.dtype
    a.M, a.N, a.taps, a.Kc = M, N, taps, Kc
    a.A, a.lda = _ptr(A), (lda if lda is not None else A.stride(-2))
    a.rowsA = rowsA if rowsA is not None else M
    a.a_row_mul, a.a_row_off, a.a_row_step, a.a_tap_stride = a_row_mul, a_row_off, a_row_step, a_tap_stride
    a.W, a.ldw = _ptr(W), (ldw if ldw is not None else taps * Kc)
    a.groups, a.batch = groups, batch
    a.a_gstride, a.w_gstride, a.a_bstride, a.c_gcol, a.c_bstride = a_gstride, w_gstride, a_bstride, c_gcol, c_bstride
    a.bias, a.alpha, a.act, a.round_bf16 = _ptr(bias), alpha, act, int(round_bf16)
    a.residual = _ptr(residual)
    a.res_dtype = _dt(residual) if residual is not None else F32
    a.ldr = ldr
    a.C32, a.C16 = _ptr(out32), _ptr(out16)
    a.ldc = ldc if ldc is not None else N
    a.c_row_mul, a.c_row_off, a.transpose_out = c_row_mul, c_row_off, int(transpose_out)
    a.split_k, a.c_split_stride = split_k, c_split_stride
    a.stats_out = _ptr(stats_out)
    if ln is not None:      # folded LayerNorm (include/usdm_hip.h): dict(mode, stats, nt, C, eps, c= | gamma=, beta=)
        _need_cuda(ln["stats"], ln.get("c"), ln.get("gamma"), ln.get("beta"))
        a.ln_stats, a.ln_nt, a.ln_mode, a.ln_C, a.ln_eps = _ptr(ln["stats"]), ln["nt"], ln["mode"], ln["C"], ln.get("eps", 1e-5)
        a.ln_c, a.ln_gamma, a.ln_beta = _ptr(ln.get("c")), _ptr(ln.get("gamma")), _ptr(ln.get("beta"))
        if ln.get("guard") is not None:      # device word OR-ed with 1 when a row's |mean| / sigma exceeds guard_ratio
            _need_cuda(ln["guard"])
            a.ln_guard, a.ln_guard_ratio = _ptr(ln["guard"]), float(ln["guard_ratio"])
    tile = os.environ.get("USDM_GEMM_TILE")      # benchmarks / tile-equivalence tests: the library itself reads no environment
    if tile is not None:
        a.tile_sel = int(tile) + 1
    if qkv is not None:
        a.epi = _lib.EPI_QKV_HEADS
        a.qkv_S, a.qkv_Spad, a.qkv_H, a.qkv_D = qkv["S"], qkv["Spad"], qkv["H"], qkv["D"]
        a.qkv_q, a.qkv_k, a.qkv_v = _ptr(qkv["q"]), _ptr(qkv["k"]), _ptr(qkv["v"])
    if tile_query:
        return lib.usdm_gemm_tile_for(C_.byref(a))
    _go(plan, "usdm_gemm", lib.usdm_gemm, C_.byref(a))


def norm(x, gamma, beta=None, *, rows, C, eps=1e-5, res=None, rms=False, act=0, round_bf16=False, premask=False,
         valid_len=None, rows_per_batch=0, out32=None, out16=None, sum32=None, sum16=None,
         ldx=None, ldr=None, ldo=None, lds=None, res2=None, n_res2=0, res2_stride=0, plan=None):
    """usdm_norm: LayerNorm/RMSNorm over the last axis (see include/usdm_hip.h)."""
    _need_cuda(x, gamma, beta, res, out32, out16, sum32, sum16, valid_len)
    a = NormArgs()
    a.x, a.x_dtype, a.ldx = _ptr(x), _dt(x), (ldx if ldx is not None else C)
    a.res, a.res_dtype, a.ldr = _ptr(res), (_dt(res) if res is not None else F32), (ldr if ldr is not None else C)
    a.gamma, a.beta, a.eps = _ptr(gamma), _ptr(beta), eps
    a.rows, a.C = rows, C
    a.rms, a.act, a.round_bf16, a.premask = int(rms), act, int(round_bf16), int(premask)
    a.valid_len, a.rows_per_batch = _ptr(valid_len), rows_per_batch
    a.out32, a.out16, a.ldo = _ptr(out32), _ptr(out16), (ldo if ldo is not None else C)
    a.sum32, a.sum16, a.lds = _ptr(sum32), _ptr(sum16), (lds if lds is not None else C)
    if res2 is not None:     # further f32 addends (split-K partials): res2[i] for i < n_res2, res2_stride elements apart
        _need_cuda(res2)
        a.res2, a.n_res2, a.res2_stride = _ptr(res2), (n_res2 or 1), res2_stride
    _go(plan, "usdm_norm", lib.usdm_norm, C_.byref(a))


def aa_snake(x, alpha, beta, fup, fdn, *, T, C, Creal=None, logscale=True, out32=None, out16=None, ldx=None, ldo=None, L=0, plan=None):
    """usdm_aa_snake: fused Activation1d(SnakeBeta) on channels-last f32 [T][C]."""
    _need_cuda(x, alpha, beta, out32, out16)
    a = SnakeArgs()
    a.x, a.ldx = _ptr(x), (ldx if ldx is not None else C)
    a.T, a.C, a.Creal, a.L = T, C, (Creal if Creal is not None else C), L
    a.alpha, a.beta, a.logscale = _ptr(alpha), _ptr(beta), int(logscale)
    for j in range(12):
        a.fup[j] = float(fup[j])
        a.fdn[j] = float(fdn[j])
    a.out32, a.out16, a.ldo = _ptr(out32), _ptr(out16), (ldo if ldo is not None else C)
    _go(plan, "usdm_aa_snake", lib.usdm_aa_snake, C_.byref(a))


def attention(q, k, vt, o, *, mode, dh, B, Hq, Hkv, Sq, Skv, Skv_alloc, q_strides, k_strides, v_strides, o_strides,
              scale=1.0, q_pos0=0, kv_len=None, slopes=None, alibi_col0_zero=True, window=0, plan=None):
    """usdm_attention (see include/usdm_hip.h for layouts)."""
    _need_cuda(q, k, vt, o, kv_len, slopes)
    a = AttnArgs()
    a.mode, a.dh, a.B, a.Hq, a.Hkv, a.Sq, a.Skv, a.Skv_alloc = mode, dh, B, Hq, Hkv, Sq, Skv, Skv_alloc
    a.q_pos0, a.alibi_col0_zero, a.scale = q_pos0, int(alibi_col0_zero), scale
    a.q, (a.q_bs, a.q_hs, a.q_rs) = _ptr(q), q_strides
    a.k, (a.k_bs, a.k_hs, a.k_rs) = _ptr(k), k_strides
    a.vt, (a.v_bs, a.v_hs, a.v_ds) = _ptr(vt), v_strides
    a.o, (a.o_bs, a.o_rs) = _ptr(o), o_strides
    a.kv_len, a.slopes = _ptr(kv_len), _ptr(slopes)
    a.window = int(window)
    a.variant = 1 if os.environ.get("USDM_ATTN_V16", "1") == "0" else 0      # (tools/attn_bench.py: the 32-query-wave kernel)
    if os.environ.get("USDM_ATTN_ORDER") == "0":
        a.head_order = -1
    _go(plan, "usdm_attention", lib.usdm_attention, C_.byref(a))


def sum3_scale(a, b, c, scale, *, out32=None, out16=None, plan=None):
    _need_cuda(a, b, c, out32, out16)
    n = a.numel()
    _go(plan, "usdm_sum3_scale", lib.usdm_sum3_scale, _ptr(a), _ptr(b), _ptr(c), C_.c_float(scale), C_.c_int64(n),
        _ptr(out32), _ptr(out16))


def cf_to_cl(x, *, B, C, T, Cpad, scale=1.0, shift=0.0, out32=None, out16=None, plan=None):
    """channels-first f32 [B][C][T] -> channels-last [B][T][Cpad]."""
    _need_cuda(x, out32, out16)
    _go(plan, "usdm_cf_to_cl", lib.usdm_cf_to_cl, _ptr(x), C_.c_int32(B), C_.c_int32(C), C_.c_int32(T), C_.c_int32(Cpad),
        C_.c_float(scale), C_.c_float(shift), _ptr(out32), _ptr(out16))


def vb_build_input(ids, y, cond, table, out, *, B_in, dup, S, E, F, null_id, use_cond, ldo, plan=None):
    _need_cuda(ids, y, cond, table, out)
    a = VbInputArgs()
    a.ids, a.y, a.cond, a.table = _ptr(ids), _ptr(y), _ptr(cond), _ptr(table)
    a.B_in, a.dup, a.S, a.E, a.F, a.null_id, a.use_cond = B_in, dup, S, E, F, null_id, int(use_cond)
    a.out, a.ldo, a.out_dtype = _ptr(out), ldo, _dt(out)
    assert table.dtype == out.dtype
    _go(plan, "usdm_vb_build_input", lib.usdm_vb_build_input, C_.byref(a))


def softmax_alibi(x, *, rows, rows_per_batch, nheads, n, npad, ldrow, ldseg, slopes=None, kv_len=None, col0_zero=True, plan=None):
    _need_cuda(x, slopes, kv_len)
    _go(plan, "usdm_softmax_alibi", lib.usdm_softmax_alibi, _ptr(x), C_.c_int32(rows), C_.c_int32(rows_per_batch), C_.c_int32(nheads),
        C_.c_int32(n), C_.c_int32(npad), C_.c_int64(ldrow), C_.c_int32(ldseg), _ptr(slopes), _ptr(kv_len), C_.c_int32(int(col0_zero)))


def vb_time_token(t, freqs, h32, h16, *, Bx, H, rows_per_batch, t_stride=1, plan=None):
    _need_cuda(t, freqs, h32, h16)
    _go(plan, "usdm_vb_time_token", lib.usdm_vb_time_token, _ptr(t), C_.c_int32(t_stride), _ptr(freqs), C_.c_int32(Bx),
        C_.c_int32(H), C_.c_int64(rows_per_batch), _ptr(h32), _ptr(h16))


def vb_solver_step(vout, z, *, B, F, S, mode, dt, cfg=False, gs=0.0, v1=None, eps=None, cond=None, P=0, c_eps=0.0,
                   c_cond=0.0, z_in=None, z_commit=None, t_cur=None, t_count=0, t_next=0.0, plan=None):
    _need_cuda(vout, z, v1, eps, cond, z_in, z_commit, t_cur)
    a = VbSolverArgs()
    a.vout, a.z, a.v1, a.eps, a.cond = _ptr(vout), _ptr(z), _ptr(v1), _ptr(eps), _ptr(cond)
    a.z_in, a.z_commit, a.t_cur = _ptr(z_in), _ptr(z_commit), _ptr(t_cur)
    a.B, a.F, a.S, a.P, a.cfg, a.mode, a.t_count = B, F, S, P, int(cfg), mode, t_count
    a.gs, a.dt, a.c_eps, a.c_cond, a.t_next = gs, dt, c_eps, c_cond, t_next
    _go(plan, "usdm_vb_solver_step", lib.usdm_vb_solver_step, C_.byref(a))


def copy_bytes(dst, src, nbytes, plan=None):
    _need_cuda(dst, src)
    _go(plan, "usdm_copy_bytes", lib.usdm_copy_bytes, _ptr(dst), _ptr(src), C_.c_int64(nbytes))


def process_unit(units, rep, hop):
    """usdm_process_unit: int64 [n] on the GPU -> int64 [floor(n*rep/hop)]."""
    _need_cuda(units)
    if units.dtype != torch.int64 or units.dim() != 1:
        raise TypeError("units must be a 1-D int64 tensor")
    n = units.numel()
    nframes = (n * rep) // hop
    out = torch.empty(nframes, dtype=torch.int64, device=units.device)
    if n == 0 or nframes == 0:
        return out
    check(lib.usdm_process_unit(_ptr(units.contiguous()), C_.c_int32(n), C_.c_int32(rep), C_.c_int32(hop), _ptr(out),
                                C_.c_int32(nframes), _stream()), "usdm_process_unit")
    return out


def _fill_gemv(a, W, x, *, N, K, ldw=None, norm_w=None, eps=1e-5, act=0, round_bf16=True, residual=None, y16=None, y32=None,
               ban=None, part_val=None, part_idx=None, idx_offset=0):
    """The usdm_gemv_args fields that gemv, gemv_batch and gemv_fp8_mfma share (see include/usdm_hip.h)."""
    _need_cuda(W, x, norm_w, residual, y16, y32, ban, part_val, part_idx)
    a.W, a.ldw, a.N, a.K = _ptr(W), (ldw if ldw is not None else K), N, K
    if isinstance(W, Mxfp4Weight):      # (its packed rows: the stride is in bytes and belongs to the weight, not to the caller)
        a.ldw = W.q.shape[1]
    a.x, a.norm_w, a.eps = _ptr(x), _ptr(norm_w), eps
    a.act, a.round_bf16 = act, int(round_bf16)
    a.residual, a.y16, a.y32 = _ptr(residual), _ptr(y16), _ptr(y32)
    a.ban, a.part_val, a.part_idx, a.idx_offset = _ptr(ban), _ptr(part_val), _ptr(part_idx), idx_offset


def gemv(W, x, *, x_delta=None, x_out=None, skip=None, p2p=None, p2p_site=0, p2p_mode=0, merge=None, cmb=None, plan=None,
         only_args=False, resident=None, wpack=None, **common):
    """usdm_gemv: batch-1 weight-streaming GEMV (see include/usdm_hip.h; **common: the keywords of _fill_gemv).
    p2p: a usdm_amd.p2p.P2PComm (fused all-reduce).
    resident: usdm_gemv_args.resident (SwiGLU: 0 the launcher's choice, -1 one tile per workgroup, n > 0 resident on at most n
    workgroups; a plain K = 14336 projection: 0 the launcher's choice, -1 gemv_kernel, n > 0 the straight-line form at any N);
    None: USDM_GEMV_RESIDENT, else 0.
    only_args=True: return the filled usdm_gemv_args instead of launching (a phase of usdm_gemv_chain).
    wpack: a wpack.PackedWeight of W (bf16 W only): usdm_gemv_packed, which streams the 13-bit image where usdm_gemv_packs says
    the call has a packed form (down_proj's straight-line form) and is usdm_gemv everywhere else - identical bits either way.
    A SwiGLU call takes the image of the interleaved gate/up matrix (PackedWeight.from_matrix(W, glu=True)) through
    usdm_gemv_packed_glu / usdm_gemv_packs_glu in the same way (gate/up's straight-line resident form).
    W a quant.Fp8Weight / quant.Mxfp4Weight: usdm_gemv_fp8 / usdm_gemv_mxfp4 (the plain single-GPU forms only; the library refuses
    the others)."""
    _need_cuda(x_delta, x_out, skip)
    if x_out is not None and x_out.data_ptr() == x.data_ptr():
        raise ValueError("usdm_gemv: x_out must not alias x")
    a = GemvArgs()
    _fill_gemv(a, W, x, **common)
    a.x_delta, a.x_out, a.skip = _ptr(x_delta), _ptr(x_out), _ptr(skip)
    if resident is None:        # benchmarks / form-equivalence tests: the library itself reads no environment
        resident = int(os.environ.get("USDM_GEMV_RESIDENT", "0"))
    a.resident = resident
    if merge is not None:      # (pm, pl, po, NS): x is merged from the decode-attention partials in the prologue
        pm, pl, po, ns = merge
        _need_cuda(pm, pl, po)
        a.mrg_pm, a.mrg_pl, a.mrg_po, a.mrg_ns = _ptr(pm), _ptr(pl), _ptr(po), ns
    if cmb is not None:         # (granules int64 [K/2], err int32 [1]): the hand-off form of `merge` (one combine per head, see usdm_hip.h)
        gran, err = cmb
        _need_cuda(gran, err)
        if merge is None or gran.numel() * gran.element_size() < (a.K // 2) * 8:
            raise ValueError("usdm_gemv: cmb needs merge=(pm, pl, po, NS) and K/2 8-byte granules")
        a.cmb_gran, a.cmb_err, a.cmb_timeout_ms = _ptr(gran), _ptr(err), 200
    if p2p is not None and p2p_mode:
        p2p.check_site(p2p_site, a.N)
        a.p2p, a.p2p_site, a.p2p_mode = p2p.dev_ptr, p2p_site, p2p_mode
    if isinstance(W, Fp8Weight):
        if only_args:
            raise ValueError("usdm_gemv: FP8 weights have no chained form")
        f = GemvFp8Args()
        f.b.g, f.b.nb, f.row_exp = a, 1, _ptr(W.e)
        _go(plan, "usdm_gemv_fp8", lib.usdm_gemv_fp8, C_.byref(f))
        return
    if isinstance(W, Mxfp4Weight):
        if only_args:
            raise ValueError("usdm_gemv: MXFP4 weights have no chained form")
        f = GemvMxfp4Args()
        f.b.g, f.b.nb, f.scales, f.lds = a, 1, _ptr(W.s), W.s.shape[1]
        _go(plan, "usdm_gemv_mxfp4", lib.usdm_gemv_mxfp4, C_.byref(f))
        return
    glu = a.act == _lib.ACT_SWIGLU
    packs, packed = (lib.usdm_gemv_packs_glu, lib.usdm_gemv_packed_glu) if glu else (lib.usdm_gemv_packs, lib.usdm_gemv_packed)
    if wpack is not None and not only_args and packs(C_.byref(a)):
        # the 13-bit image of W (usdm_amd.wpack): the same result from 13/16 of the bytes.  Recorded as usdm_gemv with the
        # usdm_gemv_args first: a plan's GEMV launches are counted and grouped by that name and struct.
        if not wpack.is_cuda or (wpack.N, wpack.K, wpack.glu) != (a.N, a.K, glu):
            raise ValueError("usdm_gemv: wpack is the image of another matrix")
        p = wpack.args()
        if plan is not None:
            plan.hold(wpack.planes, wpack.rowflag)
        _go(plan, "usdm_gemv", packed, C_.byref(a), C_.byref(p))
        return
    if only_args:
        return a
    _go(plan, "usdm_gemv", lib.usdm_gemv, C_.byref(a))


def gemv_engine(phases, sync, gran, timeout_ms=2000, plan=None):
    """usdm_gemv_engine: the chained projections on the loader / consumer engine (LDS-DMA weight ring, granule hand-offs).
    gran: >= 24576 int64 words of device scratch."""
    _need_cuda(sync, gran)
    if not (1 <= len(phases) <= 4) or sync.numel() < 8 or sync.element_size() != 4 or gran.numel() * gran.element_size() < 3 * 8192 * 8:
        raise ValueError("gemv_engine: 1..4 phases, an 8-word sync block and 192 KB of granule space")
    c = _lib.GemvChainArgs()
    for i, ph in enumerate(phases):
        c.ph[i] = ph
    c.nph, c.sync, c.timeout_ms, c.gran = len(phases), _ptr(sync), timeout_ms, _ptr(gran)
    _go(plan, "usdm_gemv_engine", _lib.exp().usdm_gemv_engine, C_.byref(c))


def gemv_chain(phases, sync, timeout_ms=2000, plan=None):
    """usdm_gemv_chain: up to 4 consecutive decode projections in one persistent launch.  phases: usdm_gemv_args from
    gemv(..., only_args=True); sync: int32/uint32 device tensor of >= 8 words, zero-initialised once by the caller."""
    _need_cuda(sync)
    if not (1 <= len(phases) <= 4) or sync.numel() < 8 or sync.element_size() != 4:
        raise ValueError("gemv_chain: 1..4 phases and an 8-word sync block")
    c = _lib.GemvChainArgs()
    for i, ph in enumerate(phases):
        c.ph[i] = ph
    c.nph, c.sync, c.timeout_ms = len(phases), _ptr(sync), timeout_ms
    _go(plan, "usdm_gemv_chain", _lib.exp().usdm_gemv_chain, C_.byref(c))


def p2p_reduce(p2p, site, n, h, skip=None, plan=None):
    """usdm_allreduce_p2p_reduce: second half of the split form: h = bf16(h + bf16(sum over ranks of slot[site]))."""
    _need_cuda(h, skip)
    p2p.check_site(site, n)
    _go(plan, "usdm_allreduce_p2p_reduce", lib.usdm_allreduce_p2p_reduce, C_.c_void_p(p2p.dev_ptr), C_.c_int32(site), C_.c_int32(n),
        _ptr(h), _ptr(skip))


def argmax_p2p(part_val, part_idx, nparts, st, p2p, site, phase=0, embed=None, h_out=None, Hd=0, plan=None):
    """usdm_argmax_p2p: vocab-parallel token pick across ranks + decode-state update + epoch advance."""
    _need_cuda(part_val, part_idx, embed, h_out)
    p2p.check_site(site, 2)
    _go(plan, "usdm_argmax_p2p", lib.usdm_argmax_p2p, _ptr(part_val), _ptr(part_idx), C_.c_int32(nparts), C_.byref(st),
        C_.c_void_p(p2p.dev_ptr), C_.c_int32(site), C_.c_int32(phase), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


def decode_state(next_token, out_tokens, step, pos, *, id_offset=0, advance_pos=True, batch=0, done=None, eos=None):
    """batch > 1: next_token / step / pos are [batch] and out_tokens is [batch][max_out].
    done [1] / eos [8] = {n_eos, min_new, ids...}: device words of the optional device-side end of sequence."""
    st = DecodeState()
    st.next_token, st.out_tokens, st.step, st.pos = _ptr(next_token), _ptr(out_tokens), _ptr(step), _ptr(pos)
    st.max_out = out_tokens.shape[-1] if batch > 1 else out_tokens.numel()
    st.id_offset, st.advance_pos, st.batch = id_offset, int(advance_pos), batch
    st.done, st.eos = _ptr(done), _ptr(eos)
    return st


def argmax_final(part_val, part_idx, nparts, st, embed=None, h_out=None, Hd=0, nseg=1, seg_stride=0, plan=None):
    _need_cuda(part_val, part_idx, embed, h_out)
    if nseg > 1:      # [segment (rank)][sequence][nparts]: the gathered partials of a tensor-parallel batched step
        _go(plan, "usdm_argmax_final_seg", lib.usdm_argmax_final_seg, _ptr(part_val), _ptr(part_idx), C_.c_int32(nparts), C_.c_int32(nseg),
            C_.c_int64(seg_stride), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))
        return
    _go(plan, "usdm_argmax_final", lib.usdm_argmax_final, _ptr(part_val), _ptr(part_idx), C_.c_int32(nparts), C_.byref(st),
        _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


def sample_params_tensor(device, n=1):
    """Device block holding n usdm_sample_params (24 bytes each: temperature, top_k, top_p, min_p, seed)."""
    sz = C_.sizeof(_lib.SampleParams)
    return torch.zeros(sz if n == 1 else (n, sz), dtype=torch.uint8, device=device)


def set_sample_params(t, temperature, top_k, top_p, seed, min_p=0.0):
    """t: one 24-byte block (a row of sample_params_tensor(device, n) for slot b of a batch)"""
    p = _lib.SampleParams(float(temperature), int(top_k), float(top_p), float(min_p), int(seed) & 0xFFFFFFFFFFFFFFFF)
    t.copy_(torch.frombuffer(bytearray(bytes(p)), dtype=torch.uint8))


def _logits_row(who, a, logits, st, V, nseg, seg_stride, seg_len):
    """The f32 logits row(s) of a pick kernel (csrc/logits_row.h): checks the tensor, fills a.logits / a.V / a.logits_bs and returns
    whether the segmented entry point (usdm_*_seg) is the one to call."""
    a.logits, a.V = _ptr(logits), logits.shape[-1] if V is None else V
    if logits.dtype != torch.float32 or logits.stride(-1) != 1:
        raise ValueError(f"{who}: logits must be float32 with unit inner stride")
    if seg_len > 0:
        if nseg < 1 or not logits.is_contiguous() or logits.shape[-1] != seg_len or logits.numel() < (nseg - 1) * seg_stride + max(1, st.batch) * seg_len:
            raise ValueError(f"segmented {who}: logits must be a contiguous [nseg][B][seg_len] tensor")
        a.logits_bs = seg_len
        return True
    if logits.dim() > 2 or a.V > logits.shape[-1]:
        raise ValueError(f"{who}: logits must be [V] or [B][>= V] (a segmented row needs seg_len)")
    a.logits_bs = logits.stride(0) if logits.dim() == 2 else logits.numel()
    return False


def sample_final(logits, st, *, temperature=1.0, top_k=0, top_p=1.0, seed=0, min_p=0.0, probs_out=None, embed=None, h_out=None, Hd=0,
                 dev_params=None, V=None, nseg=1, seg_stride=0, seg_len=0, plan=None):
    """usdm_sample_final: temperature / top-k / top-p / min-p sampling of one token from ban-masked f32 logits.
    dev_params (sample_params_tensor): the knobs are read from device memory instead (graph-replayable per request).
    Batched state (decode_state(batch=B)): logits [B][V], dev_params [B][24], h_out [B][Hd]; one workgroup per sequence.
    V: ids drawn from (default logits.shape[-1]; a gathered tensor-parallel row is longer than the vocabulary by the last rank's
    padding slots).  seg_len > 0 (usdm_sample_final_seg): logits is [nseg][B][seg_len], the ranks' shards gathered rank-major;
    sequence b's id i is read at (i // seg_len) * seg_stride + b * seg_len + i % seg_len; probs_out is [B][V]."""
    _need_cuda(logits, probs_out, embed, h_out, dev_params)
    a = SampleArgs()
    seg = _logits_row("sample_final", a, logits, st, V, nseg, seg_stride, seg_len)
    a.temperature, a.top_k, a.top_p, a.min_p = temperature, top_k, top_p, min_p
    a.seed, a.probs_out, a.dev_params = seed, _ptr(probs_out), _ptr(dev_params)
    if probs_out is not None and probs_out.numel() < max(1, st.batch) * a.V:
        raise ValueError("sample_final: probs_out holds fewer than batch * V values")
    if seg:
        _go(plan, "usdm_sample_final_seg", lib.usdm_sample_final_seg, C_.byref(a), C_.c_int32(nseg), C_.c_int64(seg_stride),
            C_.c_int32(seg_len), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))
        return
    _go(plan, "usdm_sample_final", lib.usdm_sample_final, C_.byref(a), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


LOGPROBS_MAX_K = 20     # vLLM's cap on SamplingParams.logprobs


def logprobs(logits, st, *, K, tok_lp, tok_rank, top_id=None, top_lp=None, count=None, V=None, nseg=1, seg_stride=0, seg_len=0, plan=None):
    """usdm_logprobs, launched after the sample_final of the same step on the same row: log-probability and rank of the token that
    was just picked into tok_lp / tok_rank [max_out] at row step - 1, and (K > 0) the K most likely ids and their log-probabilities
    into top_id / top_lp, which the kernel addresses as [max_out][K].  Batched state: every output is [B][...] with its dim-0 stride.
    count (int32 [B]): rows written so far, required with a device-side `done` word (see include/usdm_hip.h).
    V / nseg / seg_stride / seg_len as in sample_final (usdm_logprobs_seg)."""
    _need_cuda(logits, tok_lp, tok_rank, top_id, top_lp, count)
    B = max(1, st.batch)
    a = LogprobArgs()
    seg = _logits_row("logprobs", a, logits, st, V, nseg, seg_stride, seg_len)
    a.K = int(K)
    a.tok_lp, a.tok_rank, a.top_id, a.top_lp, a.count = _ptr(tok_lp), _ptr(tok_rank), _ptr(top_id), _ptr(top_lp), _ptr(count)
    for name, t, dt, per in (("tok_lp", tok_lp, torch.float32, 1), ("tok_rank", tok_rank, torch.int32, 1),
                             ("top_id", top_id, torch.int32, a.K), ("top_lp", top_lp, torch.float32, a.K)):
        if t is None or not 0 <= a.K <= LOGPROBS_MAX_K:
            continue      # (the library refuses a missing output and K outside 0 .. 20)
        rows = t if B == 1 else t[0]
        if t.dtype != dt or not rows.is_contiguous() or rows.numel() < st.max_out * per or (B > 1 and (t.shape[0] < B or t.stride(0) < st.max_out * per)):
            raise ValueError(f"logprobs: {name} must be {dt} with room for [max_out = {st.max_out}][{per}] values per sequence")
    if count is not None and (count.dtype != torch.int32 or count.numel() < B):
        raise ValueError("logprobs: count must be int32 [batch]")
    a.tok_bs = tok_lp.stride(0) if (B > 1 and tok_lp is not None) else 0
    a.top_bs = top_id.stride(0) if (B > 1 and top_id is not None) else 0
    if B > 1 and (tok_rank is not None and tok_rank.stride(0) != a.tok_bs or top_lp is not None and top_lp.stride(0) != a.top_bs):
        raise ValueError("logprobs: tok_lp / tok_rank and top_id / top_lp must share their per-sequence strides")
    if seg:
        _go(plan, "usdm_logprobs_seg", lib.usdm_logprobs_seg, C_.byref(a), C_.c_int32(nseg), C_.c_int64(seg_stride), C_.c_int32(seg_len), C_.byref(st))
        return
    _go(plan, "usdm_logprobs", lib.usdm_logprobs, C_.byref(a), C_.byref(st))


def prompt_logprobs(logits, ids, *, row0, K, tok_lp, tok_rank, top_id=None, top_lp=None, rows=None, V=None, nseg=1, seg_stride=0, seg_len=0,
                    plan=None):
    """usdm_prompt_logprobs: log-probabilities of tokens that were GIVEN.  logits: a chunk of f32 rows, [rows][>= V] with any row
    stride (or one row [V]); row r is prompt row row0 + r, its target ids[row0 + r + 1] (ids: the prompt's int64 ids on the device).
    Outputs are indexed by the target's row t = row0 + r + 1: tok_lp / tok_rank [>= n_ids], top_id / top_lp addressed as [n_ids][K].
    seg_len > 0 (usdm_prompt_logprobs_seg): logits is [nseg][rows][seg_len] with any row stride, the ranks' chunks gathered rank-major,
    seg_stride elements between two segments; V: the ids scored over (default logits.shape[-1])."""
    _need_cuda(logits, ids, tok_lp, tok_rank, top_id, top_lp)
    if logits.dtype != torch.float32 or logits.stride(-1) != 1 or ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("prompt_logprobs: logits must be float32 with unit inner stride, ids a contiguous int64 [n_ids]")
    a = PromptLogprobArgs()
    a.logits, a.V, a.K = _ptr(logits), (logits.shape[-1] if V is None else V), int(K)
    a.ids, a.n_ids, a.row0 = _ptr(ids), ids.numel(), int(row0)
    if seg_len > 0:
        if logits.dim() != 3 or logits.shape[0] != nseg or logits.shape[2] != seg_len or logits.stride(0) != seg_stride:
            raise ValueError("segmented prompt_logprobs: logits must be [nseg][rows][seg_len] with seg_stride elements between segments")
        a.rows, a.logits_bs = (logits.shape[1] if rows is None else rows), logits.stride(1)
        if a.rows > logits.shape[1]:
            raise ValueError("segmented prompt_logprobs: more rows than the chunk holds")
    else:
        if logits.dim() > 2 or a.V > logits.shape[-1]:
            raise ValueError("prompt_logprobs: logits must be [V] or [rows][>= V] (a segmented chunk needs seg_len)")
        have = logits.shape[0] if logits.dim() == 2 else 1
        a.rows = have if rows is None else rows
        a.logits_bs = logits.stride(0) if logits.dim() == 2 else logits.numel()
        if a.rows > have:
            raise ValueError("prompt_logprobs: more rows than the chunk holds")
    a.tok_lp, a.tok_rank, a.top_id, a.top_lp = _ptr(tok_lp), _ptr(tok_rank), _ptr(top_id), _ptr(top_lp)
    for name, t, dt, per in (("tok_lp", tok_lp, torch.float32, 1), ("tok_rank", tok_rank, torch.int32, 1),
                             ("top_id", top_id, torch.int32, a.K), ("top_lp", top_lp, torch.float32, a.K)):
        if t is None or not 0 <= a.K <= LOGPROBS_MAX_K:
            continue      # (the library refuses a missing output and K outside 0 .. 20)
        if t.dtype != dt or not t.is_contiguous() or t.numel() < a.n_ids * per:
            raise ValueError(f"prompt_logprobs: {name} must be {dt} with room for [n_ids = {a.n_ids}][{per}] values")
    if seg_len > 0:
        _go(plan, "usdm_prompt_logprobs_seg", lib.usdm_prompt_logprobs_seg, C_.byref(a), C_.c_int32(nseg), C_.c_int64(seg_stride), C_.c_int32(seg_len))
        return
    _go(plan, "usdm_prompt_logprobs", lib.usdm_prompt_logprobs, C_.byref(a))


BEAM_MAX_KC = 32        # candidates usdm_beam_step keeps per step: KC = max(2, 1 + n_eos) * B
BEAM_MAX_EOS = 3


def beam_candidates(B, n_eos):
    """KC = max(2, 1 + n_eos) * B (HF's beams_to_keep), checked against usdm_beam_step's limits: 1 <= B <= 16, 0 <= n_eos <= 3,
    KC <= 32.  ValueError otherwise."""
    if isinstance(B, bool) or not isinstance(B, int) or not 1 <= B <= 16:
        raise ValueError(f"beam search runs 1 .. 16 beams, got {B!r}")
    if not 0 <= n_eos <= BEAM_MAX_EOS:
        raise ValueError(f"beam search takes 0 .. {BEAM_MAX_EOS} EOS ids, got {n_eos}")
    KC = max(2, 1 + n_eos) * B
    if KC > BEAM_MAX_KC:
        raise ValueError(f"beam search keeps KC = max(2, 1 + n_eos) * num_beams = {KC} candidates per step, at most {BEAM_MAX_KC} are supported")
    return KC


def beam_step(logits, st, *, score, parent, nlive, eos, n_eos, log_score, log_token, log_parent, cand_score, cand_index, embed=None,
              h_out=None, Hd=0, V=None, plan=None):
    """usdm_beam_step: the beam-search pick of B = st.batch rows of ban-masked f32 logits [B][>= V].  score f32 [B] (read and
    rewritten), parent i32 [B] (out), nlive 1 (first step) or B, eos i32 [>= 3] on the device with its first n_eos ids, the step log
    log_score f32 / log_token i32 / log_parent i32 [rows][KC] with KC = beam_candidates(B, n_eos), scratch cand_score f32 / cand_index
    i32 [B][KC].  V: ids ranked (default logits.shape[-1]).  Contiguous rows only: beam search runs on one GPU."""
    _need_cuda(logits, score, parent, eos, log_score, log_token, log_parent, cand_score, cand_index, embed, h_out)
    B = max(1, st.batch)
    KC = beam_candidates(B, n_eos)
    a = BeamArgs()
    _logits_row("beam_step", a, logits, st, V, 1, 0, 0)
    if a.V < KC:
        raise ValueError(f"beam_step: V = {a.V} is smaller than the KC = {KC} candidates kept per step")
    if nlive not in (1, B):
        raise ValueError(f"beam_step: nlive must be 1 or B = {B}, got {nlive}")
    for name, t, dt, n in (("score", score, torch.float32, B), ("parent", parent, torch.int32, B), ("eos", eos, torch.int32, BEAM_MAX_EOS),
                           ("cand_score", cand_score, torch.float32, B * KC), ("cand_index", cand_index, torch.int32, B * KC),
                           ("log_score", log_score, torch.float32, KC), ("log_token", log_token, torch.int32, KC),
                           ("log_parent", log_parent, torch.int32, KC)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"beam_step: {name} must be a contiguous {dt} tensor of at least {n} values")
    rows = min(t.numel() // KC for t in (log_score, log_token, log_parent))
    a.score, a.parent, a.nlive, a.n_eos, a.eos = _ptr(score), _ptr(parent), int(nlive), int(n_eos), _ptr(eos)
    a.log_score, a.log_token, a.log_parent, a.log_rows = _ptr(log_score), _ptr(log_token), _ptr(log_parent), rows
    a.cand_score, a.cand_index = _ptr(cand_score), _ptr(cand_index)
    _go(plan, "usdm_beam_step", lib.usdm_beam_step, C_.byref(a), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


def kv_reorder(arrays, parent, lo, pos, *, B, nblk, ctx_max, plan=None):
    """usdm_kv_reorder: rows [lo[0], pos[0]) of every block of slot b become those of slot parent[b], in place, for each tensor of
    `arrays` (1 .. 4 of them): [>= B][nblk = layers x kv heads][ctx_max][row...] with contiguous slots, any element type (K / V caches,
    bf16 or e4m3, and the fp8 cache's exponents [B][nblk][ctx_max]).  parent i32 [>= B], lo i32 [1], pos i32 [>= 1]: device memory."""
    _need_cuda(parent, lo, pos, *arrays)
    if not 1 <= len(arrays) <= 4:
        raise ValueError("kv_reorder: 1 .. 4 arrays")
    for t in (parent, lo, pos):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("kv_reorder: parent, lo and pos must be contiguous int32 tensors")
    if parent.numel() < B or lo.numel() < 1 or pos.numel() < 1:
        raise ValueError("kv_reorder: parent [B], lo [1], pos [>= 1]")
    a = KvReorderArgs()
    a.n_arrays, a.nblk, a.ctx_max, a.B = len(arrays), int(nblk), int(ctx_max), int(B)
    a.parent, a.lo, a.pos = _ptr(parent), _ptr(lo), _ptr(pos)
    for i, t in enumerate(arrays):
        if t.shape[0] < B or not t[0].is_contiguous() or t[0].numel() % (nblk * ctx_max):
            raise ValueError(f"kv_reorder: array {i} must be [>= B][nblk][ctx_max][row] with contiguous slots")
        a.base[i], a.slot_bytes[i] = t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t[0].numel()) * t.element_size()
        a.row_bytes[i] = t[0].numel() // (nblk * ctx_max) * t.element_size()
    _go(plan, "usdm_kv_reorder", lib.usdm_kv_reorder, C_.byref(a))


def kv_expand(kcache, vcache, vt, *, n, Hkv, ctx_max, vt_ld, kv8=None, kscr=None, kscr_ld=0, plan=None):
    """usdm_kv_expand: rows 0 .. n-1 of one layer's cache of one sequence ([Hkv][ctx_max][128]) as the prefill attention's operands -
    V^T into vt [Hkv][128][vt_ld], and with kv8=(kexp, vexp) (uint8 caches) the dequantized K rows into kscr [Hkv][kscr_ld][128]."""
    _need_cuda(kcache, vcache, vt, kscr)
    a = KvExpandArgs()
    a.kcache, a.vcache, a.vt, a.vt_ld, a.kscr, a.kscr_ld = _ptr(kcache), _ptr(vcache), _ptr(vt), vt_ld, _ptr(kscr), kscr_ld
    a.Hkv, a.ctx_max, a.n = Hkv, ctx_max, n
    if kv8 is not None:
        kexp, vexp = _kv8(kv8, kcache, vcache)
        a.kexp, a.vexp = _ptr(kexp), _ptr(vexp)
    elif kcache.dtype != torch.bfloat16 or vcache.dtype != torch.bfloat16:
        raise TypeError("kv_expand: bf16 caches, or uint8 caches with kv8=(kexp, vexp)")
    _go(plan, "usdm_kv_expand", lib.usdm_kv_expand, C_.byref(a))


PENALTY_PROMPT_BIT = 1 << 30     # usdm_penalize's table word: in_prompt(i) in bit 30, c(i) below it
PENALTY_NEUTRAL = (1.0, 0.0, 0.0)   # repetition, frequency, presence: the knobs that change nothing


def penalty_params_tensor(device, n=1):
    """Device block holding n usdm_penalty_params (16 bytes each: repetition, frequency, presence, reserved); zero-filled = neutral."""
    sz = C_.sizeof(_lib.PenaltyParams)
    return torch.zeros(sz if n == 1 else (n, sz), dtype=torch.uint8, device=device)


def penalty_params(repetition=1.0, frequency=0.0, presence=0.0):
    """One host usdm_penalty_params, filled and range-checked by the library (usdm_penalty_params_init): repetition in (0, 2],
    frequency and presence in [-2, 2]; anything else, NaN included, is a ValueError."""
    p = _lib.PenaltyParams()
    try:
        r, f, q = float(repetition), float(frequency), float(presence)
    except (TypeError, ValueError):
        raise ValueError(f"penalties must be numbers, got {repetition!r}, {frequency!r}, {presence!r}") from None
    if lib.usdm_penalty_params_init(C_.byref(p), C_.c_float(r), C_.c_float(f), C_.c_float(q)) != 0:
        raise ValueError(lib.usdm_last_error().decode())
    return p


def set_penalty_params(block, repetition=1.0, frequency=0.0, presence=0.0):
    """block: one 16-byte block (a row of penalty_params_tensor(device, n) for slot b of a batch)"""
    block.copy_(torch.frombuffer(bytearray(bytes(penalty_params(repetition, frequency, presence))), dtype=torch.uint8))


def penalize(logits, st, *, table, dev_params, count=None, V=None, nseg=1, seg_stride=0, seg_len=0, plan=None):
    """usdm_penalize, launched before the sample_final of the same step on the row it will read: counts the token the previous step
    picked into table (int32 [V], or [B][>= V] with a batched state) and applies the repetition / frequency / presence penalties of
    dev_params (penalty_params_tensor) to the f32 row in place.  count (int32 [B]): the step at the last counting, required with a
    device-side `done` word (see include/usdm_hip.h).  V / nseg / seg_stride / seg_len as in sample_final (usdm_penalize_seg)."""
    _need_cuda(logits, table, dev_params, count)
    B = max(1, st.batch)
    a = PenaltyArgs()
    seg = _logits_row("penalize", a, logits, st, V, nseg, seg_stride, seg_len)
    a.table, a.dev_params, a.count = _ptr(table), _ptr(dev_params), _ptr(count)
    if table is not None:
        rows = table if B == 1 else table[0]
        if table.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < a.V or (B > 1 and (table.dim() != 2 or table.shape[0] < B)):
            raise ValueError(f"penalize: table must be int32 with room for V = {a.V} words per sequence")
        a.table_bs = table.stride(0) if B > 1 else 0
    if dev_params is not None and (dev_params.dtype != torch.uint8 or not dev_params.is_contiguous() or dev_params.numel() < 16 * B):
        raise ValueError("penalize: dev_params must be a penalty_params_tensor of [batch] blocks")
    if count is not None and (count.dtype != torch.int32 or count.numel() < B):
        raise ValueError("penalize: count must be int32 [batch]")
    if seg:
        _go(plan, "usdm_penalize_seg", lib.usdm_penalize_seg, C_.byref(a), C_.c_int32(nseg), C_.c_int64(seg_stride), C_.c_int32(seg_len), C_.byref(st))
        return
    _go(plan, "usdm_penalize", lib.usdm_penalize, C_.byref(a), C_.byref(st))


LOGIT_BIAS_MAX = 1024     # bias entries per sequence: one per thread of usdm_logit_edit's workgroup


def edit_params_tensor(device, n=1):
    """Device block holding n usdm_logit_edit_params (16 bytes each: ngram, prompt_len, n_bias, reserved); zero-filled = neutral."""
    sz = C_.sizeof(_lib.LogitEditParams)
    return torch.zeros(sz if n == 1 else (n, sz), dtype=torch.uint8, device=device)


def set_edit_params(block, ngram=0, prompt_len=0, n_bias=0):
    """block: one 16-byte block (a row of edit_params_tensor(device, n) for slot b of a batch)"""
    if ngram < 0 or prompt_len < 0 or not 0 <= n_bias <= LOGIT_BIAS_MAX:
        raise ValueError(f"set_edit_params: ngram >= 0, prompt_len >= 0, n_bias 0 .. {LOGIT_BIAS_MAX}; got {ngram}, {prompt_len}, {n_bias}")
    p = _lib.LogitEditParams(min(int(ngram), 2 ** 31 - 1), int(prompt_len), int(n_bias), 0)
    block.copy_(torch.frombuffer(bytearray(bytes(p)), dtype=torch.uint8))


def logit_edit(logits, st, *, dev_params, bias_id=None, bias_val=None, prompt=None, V=None, nseg=1, seg_stride=0, seg_len=0, plan=None):
    """usdm_logit_edit, launched before the penalize / sample_final of the same step on the row they will read: adds the sequence's
    logit bias (bias_id int32 / bias_val f32, [<= 1024] or [B][<= 1024]; the first n_bias entries count) and writes -inf over the ids
    HF's no_repeat_ngram_size bans, the history being prompt (int32 [>= prompt_len] or [B][...]) followed by the state's out_tokens.
    dev_params: edit_params_tensor.  V / nseg / seg_stride / seg_len as in sample_final (usdm_logit_edit_seg)."""
    _need_cuda(logits, dev_params, bias_id, bias_val, prompt)
    B = max(1, st.batch)
    a = LogitEditArgs()
    seg = _logits_row("logit_edit", a, logits, st, V, nseg, seg_stride, seg_len)
    a.dev_params, a.bias_id, a.bias_val, a.prompt = _ptr(dev_params), _ptr(bias_id), _ptr(bias_val), _ptr(prompt)
    if dev_params is not None and (dev_params.dtype != torch.uint8 or not dev_params.is_contiguous() or dev_params.numel() < 16 * B):
        raise ValueError("logit_edit: dev_params must be an edit_params_tensor of [batch] blocks")
    if (bias_id is None) != (bias_val is None):
        raise ValueError("logit_edit: bias_id and bias_val go together")

    def rows_of(name, t, dt):      # -> (entries per sequence, per-sequence stride)
        if t is None:
            return 0, 0
        rows = t if B == 1 else t[0]
        if t.dtype != dt or not rows.is_contiguous() or (B > 1 and (t.dim() != 2 or t.shape[0] < B)):
            raise ValueError(f"logit_edit: {name} must be {dt}, [n] or [batch][n] with contiguous rows")
        return rows.numel(), (t.stride(0) if B > 1 else 0)
    a.bias_max, a.bias_bs = rows_of("bias_id", bias_id, torch.int32)
    if rows_of("bias_val", bias_val, torch.float32) != (a.bias_max, a.bias_bs) or a.bias_max > LOGIT_BIAS_MAX:
        raise ValueError(f"logit_edit: bias_id and bias_val must have the same shape, at most {LOGIT_BIAS_MAX} entries per sequence")
    a.prompt_max, a.prompt_bs = rows_of("prompt", prompt, torch.int32)
    if seg:
        _go(plan, "usdm_logit_edit_seg", lib.usdm_logit_edit_seg, C_.byref(a), C_.c_int32(nseg), C_.c_int64(seg_stride), C_.c_int32(seg_len), C_.byref(st))
        return
    _go(plan, "usdm_logit_edit", lib.usdm_logit_edit, C_.byref(a), C_.byref(st))


def logits_p2p(logits, Vloc, st, p2p, site0, row_out, phase=0, plan=None):
    """usdm_logits_p2p: this rank's Vloc f32 logits to every rank, every rank's into row_out [world * Vloc] (global-id order),
    epoch + 1.  The shard spans ceil(Vloc / max_elems) sites from site0.  phase 0: put + get; 1: put; 2: get."""
    _need_cuda(logits, row_out)
    if logits.numel() < Vloc or (phase != 1 and row_out.numel() < p2p.world * Vloc):
        raise ValueError("logits_p2p: logits holds fewer than Vloc values or row_out fewer than world * Vloc")
    p2p.check_site(site0 + (Vloc - 1) // p2p.max_elems, 1)
    _go(plan, "usdm_logits_p2p", lib.usdm_logits_p2p, _ptr(logits), C_.c_int32(Vloc), C_.byref(st) if st is not None else None,
        C_.c_void_p(p2p.dev_ptr), C_.c_int32(site0), C_.c_int32(phase), _ptr(row_out))


def embed_rows(table, out, *, Hd, ids=None, next_token=None, n=1, plan=None):
    _need_cuda(table, out, ids, next_token)
    _go(plan, "usdm_embed_rows", lib.usdm_embed_rows, _ptr(table), _ptr(ids), _ptr(next_token), C_.c_int32(n), C_.c_int32(Hd), _ptr(out))


def _kv8(kv8, kcache, vcache):
    """kv8 = (kexp, vexp) int8 exponent arrays of uint8 e4m3 caches (usdm_amd/quant.py quantize_kv_rows)."""
    kexp, vexp = kv8
    _need_cuda(kexp, vexp)
    if kcache.dtype != torch.uint8 or vcache.dtype != torch.uint8 or kexp.dtype != torch.int8 or vexp.dtype != torch.int8:
        raise TypeError("kv8: uint8 caches [Hkv][ctx_max][128] with int8 exponents [Hkv][ctx_max]")
    return kexp, vexp


def rope_cache(qkv, cos, sin, kcache, vcache, *, ld, S, pos0, Hq, Hkv, ctx_max, max_pos, vt=None, vt_ld=0, kv8=None, kscr=None,
               kscr_ld=0, plan=None):
    """usdm_rope_cache; kv8=(kexp, vexp): usdm_rope_cache_fp8 - kcache / vcache are the uint8 caches, the bf16 roped K rows go to
    kscr [Hkv][kscr_ld][128] and V^T to vt (the prompt's own attention reads those)."""
    _need_cuda(qkv, cos, sin, kcache, vcache, vt, kscr)

    def fill(a):
        a.qkv, a.ld, a.S, a.pos0, a.Hq, a.Hkv, a.ctx_max, a.max_pos = _ptr(qkv), ld, S, pos0, Hq, Hkv, ctx_max, max_pos
        a.cos, a.sin, a.kcache, a.vcache, a.vt, a.vt_ld = _ptr(cos), _ptr(sin), _ptr(kcache), _ptr(vcache), _ptr(vt), vt_ld
    if kv8 is None:
        if kscr is not None:
            raise ValueError("rope_cache: kscr belongs to the fp8 cache form (kv8=)")
        a = RopeArgs()
        fill(a)
        _go(plan, "usdm_rope_cache", lib.usdm_rope_cache, C_.byref(a))
        return
    kexp, vexp = _kv8(kv8, kcache, vcache)
    f = RopeFp8Args()
    fill(f.r)
    f.kexp, f.vexp, f.kscr, f.kscr_ld = _ptr(kexp), _ptr(vexp), _ptr(kscr), kscr_ld
    _go(plan, "usdm_rope_cache_fp8", lib.usdm_rope_cache_fp8, C_.byref(f))


def gemv_batch(W, x, *, nb, x_bs, y_bs=0, res_bs=0, part_bs=0, form=0, ks=None, plan=None, only_args=False, **common):
    """usdm_gemv_batch: the decode projection over nb <= 16 input vectors (x is [nb][x_bs], outputs [nb][y_bs]; **common: the
    keywords of _fill_gemv).
    form 0: VALU kernel for nb <= 4, matrix-core kernel above; 1: matrix cores; -1: VALU; 3 / 5: A/B forms of the matrix-core kernel.
    ks = (part f32 [gemv_batch_ks_floats(N, K)], counters int32 [ceil(N / 16)], zero): K split over workgroups (K > 4096)."""
    b = GemvBatchArgs()
    _fill_gemv(b.g, W, x, **common)
    b.nb, b.x_bs, b.y_bs, b.res_bs, b.part_bs, b.form = nb, x_bs, y_bs, res_bs, part_bs, form
    if ks is not None:
        part, cnt = ks
        _need_cuda(part, cnt)
        if part.dtype != torch.float32 or cnt.dtype != torch.int32 or cnt.numel() < -(-b.g.N // 16):
            raise ValueError("usdm_gemv_batch: ks = (float32 partials, int32 counters [ceil(N / 16)])")
        b.ks_part, b.ks_cnt, b.ks_part_floats = _ptr(part), _ptr(cnt), part.numel()
    if only_args:         # (gemv_fp8_mfma: the filled usdm_gemv_batch_args)
        return b
    if isinstance(W, Fp8Weight):     # usdm_gemv_fp8: nb 1..4, VALU form (bit-identical with the bf16 launch on the dequantized matrix)
        f = GemvFp8Args()
        f.b, f.row_exp = b, _ptr(W.e)
        _go(plan, "usdm_gemv_fp8", lib.usdm_gemv_fp8, C_.byref(f))
        return
    if isinstance(W, Mxfp4Weight):   # usdm_gemv_mxfp4: likewise
        f = GemvMxfp4Args()
        f.b, f.scales, f.lds = b, _ptr(W.s), W.s.shape[1]
        _go(plan, "usdm_gemv_mxfp4", lib.usdm_gemv_mxfp4, C_.byref(f))
        return
    _go(plan, "usdm_gemv_batch", lib.usdm_gemv_batch, C_.byref(b))


def gemv_fp8_mfma(W, x, *, plan=None, **kw):
    """usdm_gemv_fp8_mfma: the matrix-core form (nb <= 16) on a quant.Fp8Weight, opt-in.  Keywords as gemv_batch; form 0 (K split
    where ks is given) or 5 (no split).  Equals gemv_batch(W.dequantize(), ..., form=1 or 5) bit for bit; NOT bit-identical with the
    VALU form that gemv_batch runs on an Fp8Weight (nb <= 4)."""
    if not isinstance(W, Fp8Weight):
        raise TypeError("gemv_fp8_mfma takes a quant.Fp8Weight (bf16 weights: gemv_batch)")
    f = GemvFp8Args()
    f.b, f.row_exp = gemv_batch(W.q, x, **dict(kw, only_args=True)), _ptr(W.e)
    _go(plan, "usdm_gemv_fp8_mfma", lib.usdm_gemv_fp8_mfma, C_.byref(f))


def gemv_mxfp4_mfma(W, x, *, plan=None, **kw):
    """usdm_gemv_mxfp4_mfma: the matrix-core form (nb <= 16) on a quant.Mxfp4Weight that holds the matrix-core image
    (Mxfp4Weight.from_matrix(w, matrix_cores=True) / with_matrix_core_image()), opt-in.  Keywords as gemv_batch; form 0 (K split
    where ks is given) or 5 (no split); y16 only.  Equals gemv_batch(W.dequantize(), ..., form=1 or 5) bit for bit; NOT bit-identical
    with the VALU form that gemv_batch runs on an Mxfp4Weight (nb <= 4)."""
    if not isinstance(W, Mxfp4Weight) or not W.has_matrix_core_image:
        raise TypeError("gemv_mxfp4_mfma takes a quant.Mxfp4Weight that holds the matrix-core image (matrix_cores=True)")
    _need_cuda(W.mq, W.ms)
    f = GemvMxfp4MfmaArgs()
    f.b = gemv_batch(W, x, **dict(kw, only_args=True))
    f.codes, f.ldc, f.scales, f.lds = _ptr(W.mq), W.mq.stride(0), _ptr(W.ms), W.ms.stride(0)
    _go(plan, "usdm_gemv_mxfp4_mfma", lib.usdm_gemv_mxfp4_mfma, C_.byref(f))


def dequant_fp8(W, out, plan=None):
    """usdm_dequant_fp8: a quant.Fp8Weight -> bf16 out [N][>= K] (the prefill operand of usdm_gemm)."""
    _need_cuda(W, out)
    if not isinstance(W, Fp8Weight) or out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape[0] < W.N or out.shape[1] < W.K \
            or out.stride(1) != 1:
        raise ValueError("dequant_fp8: an Fp8Weight and a bf16 [N][>= K] output with unit column stride")
    _go(plan, "usdm_dequant_fp8", lib.usdm_dequant_fp8, _ptr(W.q), _ptr(W.e), C_.c_int32(W.N), C_.c_int32(W.K), C_.c_int64(W.K),
        _ptr(out), C_.c_int64(out.stride(0)))


def dequant_mxfp4(W, out, plan=None):
    """usdm_dequant_mxfp4: a quant.Mxfp4Weight -> bf16 out [N][>= K] (the prefill operand of usdm_gemm)."""
    _need_cuda(W, out)
    if not isinstance(W, Mxfp4Weight) or out.dtype != torch.bfloat16 or out.dim() != 2 or out.shape[0] < W.N or out.shape[1] < W.K \
            or out.stride(1) != 1:
        raise ValueError("dequant_mxfp4: an Mxfp4Weight and a bf16 [N][>= K] output with unit column stride")
    _go(plan, "usdm_dequant_mxfp4", lib.usdm_dequant_mxfp4, _ptr(W.q), C_.c_int64(W.q.shape[1]), _ptr(W.s), C_.c_int64(W.s.shape[1]),
        C_.c_int32(W.N), C_.c_int32(W.K), _ptr(out), C_.c_int64(out.stride(0)))


def gemv_batch_ks_floats(N, K):
    """floats of ks_part usdm_gemv_batch wants for this shape (0: the shape is not split over workgroups)"""
    return int(lib.usdm_gemv_batch_ks_floats(C_.c_int32(N), C_.c_int32(K)))


GEMV_MFMA_FMT = {"bf16": 0, "fp8": 1, "mxfp4": 2}


def gemv_mfma_select(N, K, *, glu=False, norm=False, lm_head=False, ks=False, form=1, fmt="bf16"):
    """usdm_gemv_mfma_select: what the matrix-core launcher decides for this shape (host only, no device needed) -> the
    usdm_gemv_mfma_plan as a dict; UsdmError with the launcher's message for a shape it refuses."""
    p = _lib.GemvMfmaPlan()
    flags = int(bool(glu)) | int(bool(norm)) << 1 | int(bool(lm_head)) << 2 | int(bool(ks)) << 3
    _lib.check(lib.usdm_gemv_mfma_select(C_.c_int32(N), C_.c_int32(K), C_.c_int32(flags), C_.c_int32(form),
                                         C_.c_int32(GEMV_MFMA_FMT[fmt]), C_.byref(p)), "usdm_gemv_mfma_select")
    return {n: getattr(p, n) for n, _ in p._fields_}


def attn_decode(qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, *, Hq, Hkv, ctx_max, NS, scale, counters=None, batch=0,
                qkv_bs=0, out_bs=0, cache_bs=0, skip=None, defer_merge=False, window=0, cmb_gran=None, kv8=None, exp_bs=0, plan=None):
    """usdm_attn_decode; kv8=(kexp, vexp): usdm_attn_decode_fp8 on uint8 e4m3 caches (cache_bs in bytes, exp_bs between the
    sequences' exponent arrays)."""
    _need_cuda(qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, counters)
    if kv8 is not None:
        f = AttnDecodeFp8Args()
        a = f.a       # (a view of f's leading usdm_attn_decode_args)
    else:
        a = AttnDecodeArgs()
    a.qkv, a.pos, a.Hq, a.Hkv, a.ctx_max, a.NS, a.scale = _ptr(qkv), _ptr(pos), Hq, Hkv, ctx_max, NS, scale
    a.cos, a.sin, a.kcache, a.vcache = _ptr(cos), _ptr(sin), _ptr(kcache), _ptr(vcache)
    a.pm, a.pl, a.po, a.out, a.counters = _ptr(pm), _ptr(pl), _ptr(po), _ptr(out), _ptr(counters)
    a.batch, a.qkv_bs, a.out_bs, a.cache_bs, a.skip = batch, qkv_bs, out_bs, cache_bs, _ptr(skip)
    a.defer_merge = int(defer_merge)
    a.window = int(window)
    if cmb_gran is not None:
        _need_cuda(cmb_gran)
        if cmb_gran.numel() * cmb_gran.element_size() < Hq * 64 * 8:
            raise ValueError("usdm_attn_decode: cmb_gran holds Hq*64 8-byte granules")
        a.cmb_gran = _ptr(cmb_gran)
    if kv8 is not None:
        kexp, vexp = _kv8(kv8, kcache, vcache)
        f.kexp, f.vexp, f.exp_bs = _ptr(kexp), _ptr(vexp), exp_bs
        _go(plan, "usdm_attn_decode_fp8", lib.usdm_attn_decode_fp8, C_.byref(f))
        return
    _go(plan, "usdm_attn_decode", lib.usdm_attn_decode, C_.byref(a))


SPEC_MAX_T = 8        # rows of a speculative step (usdm_attn_verify, usdm_spec_commit)
ATTN_VERIFY_TILE = 64  # usdm_attn_verify's key tile: C is a multiple of it, at most ATTN_VERIFY_CMAX
ATTN_VERIFY_CMAX = 256


def attn_verify_splits(ctx_max, C):
    """splits of usdm_attn_verify's grid and of its partial buffers [T][Hq][splits]"""
    return -(-ctx_max // C)


def _attn_verify_args(a, qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, T, Hq, Hkv, ctx_max, C, scale, window, skip, qkv_ld, out_ld):
    _need_cuda(qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, skip)
    a.qkv, a.qkv_ld, a.pos = _ptr(qkv), (Hq + 2 * Hkv) * 128 if qkv_ld is None else qkv_ld, _ptr(pos)
    a.T, a.Hq, a.Hkv, a.ctx_max, a.C, a.window, a.scale = T, Hq, Hkv, ctx_max, C, int(window), scale
    a.cos, a.sin, a.kcache, a.vcache = _ptr(cos), _ptr(sin), _ptr(kcache), _ptr(vcache)
    a.pm, a.pl, a.po, a.out, a.out_ld, a.skip = _ptr(pm), _ptr(pl), _ptr(po), _ptr(out), Hq * 128 if out_ld is None else out_ld, _ptr(skip)


def attn_verify(qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, *, T, Hq, Hkv, ctx_max, C, scale, window=0, skip=None, qkv_ld=None,
                out_ld=None, plan=None):
    """usdm_attn_verify: decode attention for T new tokens of one sequence (qkv [T][qkv_ld], out [T][out_ld], bf16 caches)."""
    a = AttnVerifyArgs()
    _attn_verify_args(a, qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, T, Hq, Hkv, ctx_max, C, scale, window, skip, qkv_ld, out_ld)
    _go(plan, "usdm_attn_verify", lib.usdm_attn_verify, C_.byref(a))


def attn_verify_batch(qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, *, B, T, Hq, Hkv, ctx_max, C, scale, cache_bs, window=0, skip=None,
                      qkv_ld=None, out_ld=None, plan=None):
    """usdm_attn_verify_batch: the same for B slots x T rows (qkv [B*T][qkv_ld], out [B*T][out_ld], pos / skip [B], partials
    [B][T][Hq][splits]); kcache / vcache are slot 0's, slot b's lie b * cache_bs elements behind."""
    a = AttnVerifyBatchArgs()
    _attn_verify_args(a.v, qkv, pos, cos, sin, kcache, vcache, pm, pl, po, out, T, Hq, Hkv, ctx_max, C, scale, window, skip, qkv_ld, out_ld)
    a.B, a.cache_bs = B, cache_bs
    _go(plan, "usdm_attn_verify_batch", lib.usdm_attn_verify_batch, C_.byref(a))


def _spec_args(a, part_val, part_idx, nparts, T, drafts, limit, prompt, prompt_len, prompt_max, params, counters, V, script, propose_only):
    a.part_val, a.part_idx, a.nparts, a.T = _ptr(part_val), _ptr(part_idx), nparts, T
    a.drafts, a.limit, a.prompt, a.prompt_len, a.prompt_max = _ptr(drafts), _ptr(limit), _ptr(prompt), _ptr(prompt_len), prompt_max
    a.script, a.params, a.V, a.counters, a.propose_only = _ptr(script), _ptr(params), V, _ptr(counters), int(propose_only)


def spec_commit(part_val, part_idx, nparts, st, *, T, drafts, limit, prompt, prompt_len, params, counters, V, script=None, embed, h_out, Hd,
                propose_only=False, picks=None, plan=None):
    """usdm_spec_commit: pick, accept, commit, propose and embed at the end of a speculative step (propose_only: after the prefill).
    picks (int32 [T], local ids): usdm_spec_commit_picks - the rows' picks are given (usdm_spec_sample) and the partials not read."""
    _need_cuda(part_val, part_idx, picks, drafts, limit, prompt, prompt_len, params, counters, script, embed, h_out)
    a = SpecArgs()
    _spec_args(a, part_val, part_idx, nparts, T, drafts, limit, prompt, prompt_len, prompt.numel(), params, counters, V, script, propose_only)
    if picks is not None:
        _go(plan, "usdm_spec_commit_picks", lib.usdm_spec_commit_picks, C_.byref(a), _ptr(picks), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))
        return
    _go(plan, "usdm_spec_commit", lib.usdm_spec_commit, C_.byref(a), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


def spec_commit_batch(part_val, part_idx, nparts, st, *, T, drafts, limit, prompt, prompt_len, params, counters, V, script=None, embed, h_out, Hd,
                      slot_lo=0, n=None, propose_only=False, picks=None, plan=None):
    """usdm_spec_commit_batch: usdm_spec_commit on the slots [slot_lo, slot_lo + n) (default: all) of the batched state st (st.batch = B
    slots): part_val / part_idx [B*T][nparts], drafts [B][8], limit / prompt_len [B], prompt [B][prompt_max], script [B][max_out] or
    None, counters [B][3], params [4] shared, h_out [B*T][Hd].  picks (int32 [B*T], local ids): usdm_spec_commit_batch_picks."""
    _need_cuda(part_val, part_idx, picks, drafts, limit, prompt, prompt_len, params, counters, script, embed, h_out)
    a = SpecBatchArgs()
    _spec_args(a.s, part_val, part_idx, nparts, T, drafts, limit, prompt, prompt_len, prompt.shape[-1], params, counters, V, script, propose_only)
    a.slot_lo, a.n = slot_lo, st.batch - slot_lo if n is None else n
    if picks is not None:
        _go(plan, "usdm_spec_commit_batch_picks", lib.usdm_spec_commit_batch_picks, C_.byref(a), _ptr(picks), C_.byref(st), _ptr(embed), C_.c_int32(Hd),
            _ptr(h_out))
        return
    _go(plan, "usdm_spec_commit_batch", lib.usdm_spec_commit_batch, C_.byref(a), C_.byref(st), _ptr(embed), C_.c_int32(Hd), _ptr(h_out))


def spec_sample(logits, picks, *, T, n, dev_params, step, drafts, done=None, V=None, plan=None):
    """usdm_spec_sample: the draws of the n * T rows of a sampled speculative step.  logits f32 [n * T][>= V], dev_params [n][24]
    (sample_params_tensor), step [n], done [n] or None, drafts [n][8], picks int32 [n * T]: picks[b * T + i] = the local id
    usdm_sample_final commits for that row with slot b's knobs at step[b] + i; rows of a done slot or behind a -1 draft are skipped."""
    _need_cuda(logits, picks, dev_params, step, drafts, done)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < n * T:
        raise ValueError("spec_sample: logits must be float32 [n * T][>= V] with unit inner stride")
    if picks.dtype != torch.int32 or picks.numel() < n * T or drafts.numel() < n * SPEC_MAX_T or step.numel() < n or (done is not None and done.numel() < n) or dev_params.numel() < n * C_.sizeof(_lib.SampleParams):
        raise ValueError("spec_sample: picks [n * T] int32, drafts [n][8], step [n] and dev_params [n][24] are required")
    a = SpecSampleArgs()
    a.logits, a.logits_bs, a.V, a.T, a.n = _ptr(logits), logits.stride(0), logits.shape[-1] if V is None else V, T, n
    a.dev_params, a.step, a.done, a.drafts, a.picks = _ptr(dev_params), _ptr(step), _ptr(done), _ptr(drafts), _ptr(picks)
    _go(plan, "usdm_spec_sample", lib.usdm_spec_sample, C_.byref(a))


def residual_add(h, delta, n, plan=None):
    _need_cuda(h, delta)
    _go(plan, "usdm_residual_add", lib.usdm_residual_add, _ptr(h), _ptr(delta), C_.c_int32(n))


def gemv_nblocks(N, act=0):
    return lib.usdm_gemv_nblocks(C_.c_int32(N), C_.c_int32(act))


def wave_layernorm(x, y, n, eps=1e-5, plan=None):
    _need_cuda(x, y)
    _go(plan, "usdm_wave_layernorm", lib.usdm_wave_layernorm, _ptr(x), C_.c_int32(n), C_.c_float(eps), _ptr(y))


def w2v_conv0(x, w, b, g, be, out, *, n, T, C, k, stride, eps=1e-5, plan=None):
    _need_cuda(x, w, b, g, be, out)
    _go(plan, "usdm_w2v_conv0", lib.usdm_w2v_conv0, _ptr(x), C_.c_int32(n), C_.c_int32(T), C_.c_int32(C), C_.c_int32(k),
        C_.c_int32(stride), _ptr(w), _ptr(b), _ptr(g), _ptr(be), C_.c_float(eps), _ptr(out))


def softmax_segments(x, *, rows, nseg, n, npad, ldrow, ldseg, plan=None):
    _need_cuda(x)
    _go(plan, "usdm_softmax_segments", lib.usdm_softmax_segments, _ptr(x), C_.c_int32(rows), C_.c_int32(nseg), C_.c_int32(n),
        C_.c_int32(npad), C_.c_int64(ldrow), C_.c_int32(ldseg))


def kmeans_argmin(x, dots, csq, ids, *, T, D, n_units, ldd, margin=None, plan=None):
    _need_cuda(x, dots, csq, ids, margin)
    _go(plan, "usdm_kmeans_argmin", lib.usdm_kmeans_argmin, _ptr(x), C_.c_int32(T), C_.c_int32(D), _ptr(dots), C_.c_int64(ldd),
        _ptr(csq), C_.c_int32(n_units), _ptr(ids), _ptr(margin))


def stft_frames(x, window, frames, *, n, n_fft, hop, pad, T, plan=None):
    _need_cuda(x, window, frames)
    _go(plan, "usdm_stft_frames", lib.usdm_stft_frames, _ptr(x), C_.c_int32(n), C_.c_int32(n_fft), C_.c_int32(hop), C_.c_int32(pad),
        _ptr(window), _ptr(frames), C_.c_int32(T))


def stft_mag(re_im, out, *, ld, T, nbins, eps, ldo, nbins_pad, plan=None):
    _need_cuda(re_im, out)
    _go(plan, "usdm_stft_mag", lib.usdm_stft_mag, _ptr(re_im), C_.c_int64(ld), C_.c_int32(T), C_.c_int32(nbins), C_.c_float(eps),
        _ptr(out), C_.c_int64(ldo), C_.c_int32(nbins_pad))


def frame_signal(x, frames, *, n, frame_len, hop, offset, T, plan=None):
    _need_cuda(x, frames)
    _go(plan, "usdm_frame_signal", lib.usdm_frame_signal, _ptr(x), C_.c_int32(n), C_.c_int32(frame_len), C_.c_int32(hop),
        C_.c_int32(offset), _ptr(frames), C_.c_int32(T))


def mask_time(valid_len, *, B, T, C, layout, off=0, x32=None, x16=None, plan=None):
    _need_cuda(valid_len, x32, x16)
    _go(plan, "usdm_mask_time", lib.usdm_mask_time, _ptr(x32), _ptr(x16), C_.c_int32(B), C_.c_int32(T), C_.c_int32(C),
        C_.c_int32(layout), _ptr(valid_len), C_.c_int32(off))
