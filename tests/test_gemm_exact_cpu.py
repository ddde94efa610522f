"""The reference, the inputs and the bounds of tests/test_gemm_exact_gpu.py, checked without a GPU: the reference against
torch.nn.functional on the very inputs of the GPU cases, the exactness bound, the recorded activation constants, the guards, and the
host side of usdm_gemm (refusals, usdm_gemm_tile_for, the tile table and the recorded tile choice)."""
import ctypes as C_

import pytest
import torch
import torch.nn.functional as Fn

from tests import _gemm_reference as R
from tests._gemm_reference import BF, F32, F64

SHAPES = sorted({(bm, bn) for bm, bn, _, _ in R.TILES.values()})            # the tile sizes: (64, 64) ... (288, 128)
DT_SHAPES = [(dt, bm, bn) for dt in (BF, F32) for bm, bn in SHAPES if dt == BF or bm <= 128]
ids = lambda p: f"{R.dt_name(p[0])}-{p[1]}x{p[2]}"


def _all_cases(dt, BM, BN):
    for name, fn in R.GROUPS.items():
        kw = dict(pp=True) if name == "head_split" and BM * BN >= 128 * 128 and dt == BF else {}
        if name == "multi_tap" and BM > 128:
            yield name, R.concat_case(dt, BM, BN)
            continue
        for c in fn(dt, BM, BN, **kw):
            yield name, c
    if dt == BF and BN == 128:
        yield "stats", R.stats_cases(dt, BM, BN)[0]


def _gather(c, kw, b, g):
    """the expected [M, N] block of batch b, group g, read back through the output's index formula"""
    e = R.expected(c)["out"]
    rows, cols = R.out_rows(kw)[b].view(-1, 1), R.out_cols(kw)[g].view(1, -1)
    oi = cols * kw["ldc"] + rows if kw["transpose_out"] else rows * kw["ldc"] + cols
    assert bool(e.owned[oi].all())
    return e.vals[oi]


def _epilogue(c, kw, lin, b, g):
    """alpha * lin + bias + residual of a plain case from its buffers by slicing (no index arithmetic shared with the reference)"""
    N = kw["N"]
    v = kw["alpha"] * lin
    if c.bias is not None:
        v = v + c.bias.double()[g * kw["c_gcol"]:g * kw["c_gcol"] + N]
    if kw["round_bf16"]:
        v = v.float().to(BF).double()
    if c.res is not None:
        res = c.res.double().view(-1, kw["ldr"])
        r0 = b * kw["c_bstride"] * kw["c_row_mul"] + kw["c_row_off"]
        v = v + res[r0:r0 + kw["M"] * kw["c_row_mul"]:kw["c_row_mul"], g * kw["c_gcol"]:g * kw["c_gcol"] + N]
        if kw["round_bf16"]:
            v = v.float().to(BF).double()
    return v


@pytest.mark.parametrize("p", DT_SHAPES, ids=ids)
def test_reference_against_torch_functional(p):
    """Fn.linear / conv1d (dilated, strided, grouped) / conv_transpose1d / cat in fp64 on the logical operands of every plain case"""
    dt, BM, BN = p
    n = 0
    for group, c in _all_cases(dt, BM, BN):
        if group in ("activations", "head_split", "stats"):
            continue
        for kw, _, W in c.launches:
            Kc = kw["Kc"]
            for b in range(kw["batch"]):
                for g in range(kw["groups"]):
                    if hasattr(c, "conv"):
                        lin = R.conv_torch(c)[b, :, g * kw["N"]:(g + 1) * kw["N"]]
                    elif hasattr(c, "convT"):
                        continue
                    elif kw["taps"] > 1:        # two sources concatenated along K
                        lin = Fn.linear(torch.cat([c.Avals[0, b], c.Avals[1, b]], -1), W[g])
                    else:
                        lin = Fn.linear(c.Avals[0, b][:, g * Kc:(g + 1) * Kc], W[g])
                    assert torch.equal(_gather(c, kw, b, g), _epilogue(c, kw, lin, b, g)), (group, c.name, b, g)
                    n += 1
        if hasattr(c, "convT"):
            v, kw = c.convT, c.kw
            full = Fn.conv_transpose1d(c.Avals[0].permute(0, 2, 1), v["w"], None, stride=v["u"], padding=v["pad"])[0].T      # [T * u, N]
            e = R.expected(c)["out"]
            got = e.vals.view(-1, kw["ldc"])[:full.shape[0], :kw["N"]]
            res = c.res.double().view(-1, kw["ldr"])[:full.shape[0], :kw["N"]]
            assert bool(e.owned.view(-1, kw["ldc"])[:full.shape[0], :kw["N"]].all()), "not every one of the T * u rows is written"
            assert int(e.owned.sum()) == full.numel()
            assert torch.equal(got, kw["alpha"] * full + c.bias.double()[:kw["N"]] + res)
            n += 1
    assert n > 30


@pytest.mark.parametrize("p", DT_SHAPES, ids=ids)
def test_head_split_and_swiglu_layouts(p):
    """Q, K -> [B][H][Spad][D], V -> [B][H][D][Spad] by reshaping Fn.linear; SwiGLU: blocks of 32 W rows = 16 gate + 16 up rows"""
    dt, BM, BN = p
    for c in R.head_split_cases(dt, BM, BN):
        q, kw = c.qkv, c.kw
        lin = kw["alpha"] * Fn.linear(c.Avals[0, 0], c.launches[0][2][0]) + (c.bias.double()[:kw["N"]] if c.bias is not None else 0.0)
        if kw["round_bf16"]:
            lin = lin.float().to(BF).double()
        lin = lin.view(q["B"], q["S"], 3, q["H"], q["D"])
        e = R.expected(c)
        for i, name in enumerate("qk"):
            t = e[name].vals[:-q["D"]].view(q["B"], q["H"], q["Spad"], q["D"])
            o = e[name].owned[:-q["D"]].view(q["B"], q["H"], q["Spad"], q["D"])
            assert torch.equal(t[:, :, :q["S"]], lin[:, :, i].permute(0, 2, 1, 3)) and bool(o[:, :, :q["S"]].all())
            assert not bool(o[:, :, q["S"]:].any()) and not bool(e[name].owned[-q["D"]:].any())
        t = e["v"].vals[:-q["Spad"]].view(q["B"], q["H"], q["D"], q["Spad"])
        o = e["v"].owned[:-q["Spad"]].view(q["B"], q["H"], q["D"], q["Spad"])
        assert torch.equal(t[..., :q["S"]], lin[:, :, 2].permute(0, 2, 3, 1)) and bool(o[..., :q["S"]].all()) and not bool(o[..., q["S"]:].any())
    for c in R.activation_cases(dt, BM, BN):
        kw = c.kw
        if kw["act"] != R.ACT_SWIGLU or kw["round_bf16"]:
            continue
        W = c.launches[0][2][0].view(kw["N"] // 32, 2, 16, kw["Kc"])
        gate, up = W[:, 0].reshape(-1, kw["Kc"]), W[:, 1].reshape(-1, kw["Kc"])
        b = c.bias.double()[:kw["N"]].view(kw["N"] // 32, 2, 16)
        g = kw["alpha"] * Fn.linear(c.Avals[0, 0], gate) + b[:, 0].reshape(-1)
        u = kw["alpha"] * Fn.linear(c.Avals[0, 0], up) + b[:, 1].reshape(-1)
        e = R.expected(c)["out"]
        assert torch.equal(e.vals.view(-1, kw["ldc"])[:kw["M"], :kw["N"] // 2], Fn.silu(g) * u)
        assert int(e.owned.sum()) == kw["M"] * kw["N"] // 2


@pytest.mark.parametrize("p", DT_SHAPES, ids=ids)
def test_cases_are_exact_and_guarded(p):
    """max |acc| + max |bias| + max |res| < 2^24 and the reference never meets a NaN (so no gap is read); the NaN gaps sit where
    stated; every operand stride keeps 16-byte alignment; the activation cases' pre-activations lie on the grid of the constants"""
    dt, BM, BN = p
    es = 2 if dt == BF else 4
    for group, c in _all_cases(dt, BM, BN):
        e = R.expected(c)
        assert c.finite, (group, c.name, "the reference read a NaN gap")
        mx = lambda t: 0.0 if t is None else float(t.double().nan_to_num(0.0).abs().max())
        assert c.acc_max + mx(c.bias) + mx(c.res) < 2 ** 24, (group, c.name)
        assert c.acc_max > 8, (group, c.name)
        for kw, W, Wv in c.launches:
            for s in ("lda", "ldw", "a_gstride", "w_gstride", "a_bstride", "a_tap_stride"):
                assert kw[s] * es % 16 == 0, (group, c.name, s)
            assert c.A_off * es % 16 == 0 and kw["lda"] > kw["groups"] * kw["Kc"] and kw["ldw"] > kw["taps"] * kw["Kc"]
            # A: a NaN row before the view and after every (source, batch) block, NaN columns past groups * Kc, integers elsewhere
            A = c.A.double().view(-1, kw["lda"])
            nanrow = torch.zeros(A.shape[0], dtype=torch.bool)
            nanrow[0] = True
            nanrow[torch.arange(kw["rowsA"] + 1, A.shape[0], kw["rowsA"] + 1)] = True
            ka = kw["groups"] * kw["Kc"]
            assert bool(A[nanrow].isnan().all()) and bool(A[:, ka:].isnan().all()) and bool(A[-1].isnan().all())
            assert bool((A[~nanrow][:, :ka].abs() <= 3).all())
            Wm = W.double().view(-1, kw["ldw"])
            wnan = torch.zeros(Wm.shape[0], dtype=torch.bool)
            wnan[torch.arange(kw["N"], Wm.shape[0], kw["N"] + 1)] = True
            kt = kw["taps"] * kw["Kc"]
            assert bool(Wm[wnan].isnan().all()) and bool(Wm[:, kt:].isnan().all()) and bool((Wm[~wnan][:, :kt].abs() <= 3).all())
            assert int(wnan.sum()) == kw["groups"]
            if c.bias is not None:
                cols = R.out_cols(kw).reshape(-1)
                isn = c.bias.isnan()
                assert c.bias.numel() > kw["groups"] * kw["N"] and not bool(isn[cols].any()) and int((~isn).sum()) == cols.numel()
            if c.res is not None:
                assert kw["ldr"] > kw["N"] and bool(c.res.double().view(-1, kw["ldr"])[-1].isnan().all())
            if c.qkv is None and "out" in e:
                own = e["out"].owned
                part = c.part_size if kw["split_k"] else c.out_size
                assert kw["ldc"] > (int(R.out_rows(kw).max()) + 1 if kw["transpose_out"] else kw["N"] // 2 if kw["act"] == R.ACT_SWIGLU else kw["N"]) or c.name.endswith("ldc=N")
                assert not bool(own[part - (1 if kw["transpose_out"] else kw["ldc"]):].any()), "no guard row"
                if kw["split_k"]:
                    assert kw["c_split_stride"] > part > kw["M"] * kw["N"]
        if c.kw["round_bf16"] and c.exact and c.qkv is None:       # the inputs tell two roundings from either one alone
            o, kw = e["out"], c.kw
            ri = R.out_rows(kw).view(-1, 1) * kw["ldr"] + R.out_cols(kw).view(1, -1)
            oi = R.out_rows(kw).view(-1, 1) * kw["ldc"] + R.out_cols(kw).view(1, -1)
            pre = kw["alpha"] * R.ref_acc(c, kw, c.launches[0][1])[0, 0] + c.bias.double()[:kw["N"]]
            res = c.res.double()[ri]
            assert torch.equal(R.rbf64(R.rbf64(pre) + res), o.vals[oi])
            for what, v in (("first", R.rbf64(pre + res)), ("second", R.rbf64(pre) + res)):
                assert float((v != o.vals[oi]).double().mean()) > 0.1, (group, c.name, f"without the {what} rounding too few outputs change")
        if not c.exact:
            x = e["out"].pre[e["out"].owned]
            assert bool(((x * 16) == (x * 16).round()).all()) and float(x.abs().max()) <= 20 and x.unique().numel() > 150
            assert float((x.abs() <= 4).double().mean()) > 0.7
            if c.kw["act"] == R.ACT_SWIGLU:
                u = e["out"].up[e["out"].owned]
                assert bool(((u * 16) == (u * 16).round()).all()) and float(u.abs().max()) <= 20


def test_recorded_activation_errors():
    """the GEMM_*_TORCH_FP32_ERR constants, recomputed: each covers what is measured and is at most a quarter above it"""
    for act in (R.ACT_GELU, R.ACT_TANH, R.ACT_LOGCLAMP, R.ACT_SWIGLU):
        err, const = R.act_torch_err(act), R.ACT_ERR[act]
        print(f"[gemm] torch float32 vs fp64, {R.ACT_NAMES[act]}: {err:.3g} (recorded {const:.3g})")
        assert 0 < err <= const <= 1.25 * err, (R.ACT_NAMES[act], err, const)


def test_swiglu_rounding_reference_stays_under_the_cap():
    """torch's float32 / bfloat16 evaluation of silu_mul's four rounding points against the fp64 one, on the GPU cases' inputs: within
    one bf16 ulp everywhere and different on at most FLIP_CAP of the outputs"""
    n = diff = 0
    for dt, BM, BN in DT_SHAPES:
        c = [c for c in R.activation_cases(dt, BM, BN) if c.kw["act"] == R.ACT_SWIGLU and c.kw["round_bf16"]][0]
        e = R.expected(c)["out"]
        g, u, ref = e.pre[e.owned], e.up[e.owned], e.vals[e.owned]
        t32 = R.swiglu_rbf_ref(g, u, dtype=F32)
        assert bool(((t32 - ref).abs() <= R.bf16_ulp(ref)).all())
        assert torch.equal(ref.float().to(BF).double(), ref), "the reference is not a bf16 value"
        n, diff = n + ref.numel(), diff + int((t32 != ref).sum())
    print(f"[gemm] swiglu + round_bf16: torch float32 differs from the fp64 reference on {diff} of {n} outputs")
    assert n > 10000 and diff <= R.FLIP_CAP * n
    x = torch.tensor([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 257.0, 0.0, 3.0e-3], dtype=F64)
    assert torch.equal(R.rbf64(x), x.float().to(BF).double()) and float(R.rbf64(x)[1]) == 1.0 and float(R.rbf64(x)[2]) == 1 + 2.0 ** -6


def test_checks_see_what_they_should():
    """check_exact on a perfect output, a stray write, an unwritten element and a wrong value"""
    c = R.make("t", F32, M=5, N=6, Kc=16, seed=1, res=F32)
    e = R.expected(c)["out"]
    for dtype in (F32, BF):
        good = torch.where(e.owned, e.vals, R.sentinel(e.vals.shape, F64)).to(dtype)
        if dtype == BF:
            good = torch.where(e.owned, good, R.sentinel(good.shape, BF))
        R.check_exact("good", good, e)
        R.check_guard("good", good, e)
        own, free = int(e.owned.nonzero()[3]), int((~e.owned).nonzero()[2])
        for idx, val in ((free, 1.0), (own, None), (own, float(e.vals[own]) + 0.5)):
            bad = good.clone()
            bad[idx] = R.sentinel((1,), dtype)[0] if val is None else val
            with pytest.raises(AssertionError):
                R.check_exact("bad", bad, e)
    assert int(e.owned.sum()) == 30 and e.owned.numel() == 6 * 12


# ------------------------------------------------------------------------------------------------------------------ the host side
PTR = 0x10000


def _args(**kw):
    from usdm_amd import _lib
    a = _lib.GemmArgs()
    a.dtype, a.M, a.N, a.taps, a.Kc = _lib.BF16, 64, 192, 1, 64
    a.A, a.W, a.C32 = PTR, PTR, PTR
    a.lda = a.ldw = 64
    a.rowsA, a.ldc, a.alpha = 64, 192, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(word, **kw):
    from usdm_amd import _lib
    if not (b"stats" in word or b"ln_" in word):       # (usdm_gemm_tile_for launches nothing and skips only the folded-LayerNorm rules)
        assert _lib.lib.usdm_gemm_tile_for(C_.byref(_args(**kw))) == -2, (word, kw)
    rc = _lib.lib.usdm_gemm(C_.byref(_args(**kw)), None)
    msg = _lib.lib.usdm_last_error()
    assert rc == 2 and word in msg, (rc, msg, word, kw)


def test_usdm_gemm_refusals():
    """every USDM_CHECK_ARG of gemm_impl, clause by clause (fake aligned pointers: nothing is launched)"""
    _refused(b"bad dtype", dtype=7)
    for kw in (dict(M=0), dict(N=0), dict(M=-1)):
        _refused(b"bad M/N", **kw)
    _refused(b"Kc=40", Kc=40)
    _refused(b"Kc=0", Kc=0)
    _refused(b"Kc=48", Kc=48)
    _refused(b"Kc=24", Kc=24, dtype=1)
    _refused(b"null operand", A=0)
    _refused(b"null operand", W=0)
    _refused(b"ldw too small", ldw=56)
    _refused(b"ldw too small", taps=2, ldw=64, lda=64)
    _refused(b"16-B aligned", A=PTR + 8)
    _refused(b"16-B aligned", W=PTR + 4)
    for s in ("lda", "ldw", "a_gstride", "w_gstride", "a_bstride", "a_tap_stride"):
        _refused(b"strides", **{s: 68})
        _refused(b"strides", dtype=1, **{s: 66})
    _refused(b"a_tap_stride", a_tap_stride=-64)
    _refused(b"2 GiB", rowsA=2 ** 20, lda=1024)
    _refused(b"2 GiB", N=2 ** 20, ldw=1024)
    _refused(b"2 GiB", taps=2, ldw=128, a_tap_stride=2 ** 30)
    _refused(b"no output", C32=0)
    split = dict(split_k=2, c_split_stride=64 * 192)
    for kw in (dict(split_k=17), dict(taps=2, ldw=128), dict(C32=0, C16=PTR), dict(C16=PTR), dict(act=1), dict(round_bf16=1), dict(transpose_out=1),
               dict(epi=1), dict(c_split_stride=0)):
        _refused(b"split_k", **dict(split, **kw))
    sw = dict(act=3, N=192 - 32, ldc=96)
    for kw in (dict(N=48), dict(transpose_out=1), dict(residual=PTR), dict(ldc=98), dict(groups=2, c_gcol=4), dict(epi=1)):
        _refused(b"swiglu", **dict(sw, **kw))
    qkv = dict(epi=1, C32=0, qkv_q=PTR, qkv_k=PTR, qkv_v=PTR, qkv_S=32, qkv_Spad=64, qkv_H=1, qkv_D=64, N=192, M=64)
    from usdm_amd import _lib
    assert _lib.lib.usdm_gemm_tile_for(C_.byref(_args(**qkv))) >= 0
    for kw in (dict(qkv_q=0), dict(qkv_k=0), dict(qkv_v=0), dict(N=256), dict(qkv_D=32, N=96), dict(qkv_S=0), dict(qkv_Spad=31), dict(qkv_H=32, qkv_D=6, N=576),
               dict(transpose_out=1), dict(residual=PTR), dict(groups=2), dict(batch=2)):
        _refused(b"qkv", **dict(qkv, **kw))
    # stats_out / ln_mode: the ping-pong tiles (forced here: tile_sel = tile + 1) with a row-major bf16 epilogue, N % 128 == 0
    pp = dict(tile_sel=13, N=256, ldc=256, stats_out=PTR)
    for kw in (dict(tile_sel=1), dict(tile_sel=12), dict(tile_sel=0), dict(dtype=1), dict(epi=1, qkv_q=PTR, qkv_k=PTR, qkv_v=PTR, qkv_S=32, qkv_Spad=64, qkv_H=2, qkv_D=64, N=384, ldc=384),
               dict(transpose_out=1), dict(round_bf16=1), dict(N=192), dict(groups=2), dict(ldc=258)):
        _refused(b"stats_out / ln_mode", **dict(pp, **kw))
    _refused(b"stats_out / ln_mode", tile_sel=5, N=256, ldc=256, ln_mode=2, ln_stats=PTR, ln_nt=2, ln_C=256)
    _refused(b"stats_out needs", **dict(pp, act=1))
    _refused(b"stats_out needs", **dict(pp, split_k=2, c_split_stride=64 * 256))
    ln = dict(tile_sel=13, N=256, ldc=256, ln_stats=PTR, ln_nt=2, ln_C=256)
    ln1 = dict(ln, ln_mode=1, ln_c=PTR, act=1, C16=PTR, C32=0)
    ln2 = dict(ln, ln_mode=2, ln_gamma=PTR, ln_beta=PTR, residual=PTR, res_dtype=1, ldr=256)
    for kw in (dict(ln_stats=0), dict(ln_nt=0), dict(ln_nt=65, ln_C=65 * 128), dict(ln_C=0), dict(ln_C=384)):
        _refused(b"ln_stats / ln_nt / ln_C", **dict(ln2, **kw))
    _refused(b"ln_guard", **dict(ln2, ln_guard=PTR))
    for kw in (dict(ln_c=0), dict(act=0), dict(C16=0, C32=PTR), dict(C32=PTR), dict(residual=PTR), dict(alpha=0.5)):
        _refused(b"ln_mode 1", **dict(ln1, **kw))
    for kw in (dict(ln_gamma=0), dict(ln_beta=0), dict(residual=0), dict(res_dtype=0), dict(act=1), dict(ldr=258)):
        _refused(b"ln_mode 2", **dict(ln2, **kw))
    _refused(b"usdm_gemm: ln_mode", **dict(ln, ln_mode=3))
    _refused(b"usdm_gemm: ln_mode", **dict(ln, ln_mode=-1))


def test_usdm_gemm_tile_for_reports_the_tile_that_runs():
    """forced tiles and the launcher's reroutes; an f32 call forced to the (bf16-only) ping-pong tiles reports the 64x64 tile it runs"""
    from usdm_amd import _lib
    tile_for = lambda **kw: _lib.lib.usdm_gemm_tile_for(C_.byref(_args(**kw)))
    conv = dict(taps=3, ldw=192, a_row_off=-1, a_row_step=1)
    cat = dict(taps=2, ldw=128, a_tap_stride=64 * 64)
    qkv = dict(epi=1, C32=0, qkv_q=PTR, qkv_k=PTR, qkv_v=PTR, qkv_S=32, qkv_Spad=64, qkv_H=1, qkv_D=64)
    for dtype, dt in ((_lib.BF16, BF), (_lib.F32, F32)):
        for t in range(15):
            assert tile_for(dtype=dtype, tile_sel=t + 1) == R.expected_tile(dt, t) == (t if dt == BF or t < 12 else 2)
            want = {4: 0, 9: 0, 11: 0, 6: 1, 10: 1, 5: 2, 7: 2, 8: 2}.get(t, t)
            if t >= 12:
                want = 0
            assert tile_for(dtype=dtype, tile_sel=t + 1, **conv) == R.expected_tile(dt, t, multi_tap=True) == want
            want = t if (t < 4 or (t >= 12 and dt == BF)) else (2 if t >= 12 else want)
            assert tile_for(dtype=dtype, tile_sel=t + 1, **cat) == R.expected_tile(dt, t, multi_tap=True, concat=True) == want
            want = (12 if t == 13 else t) if dt == BF or t < 12 else 2
            assert tile_for(dtype=dtype, tile_sel=t + 1, transpose_out=1) == R.expected_tile(dt, t, transpose=True) == want
            assert tile_for(dtype=dtype, tile_sel=t + 1, **qkv) == R.expected_tile(dt, t, head_split=True) == want
    # the heuristic never chooses a ping-pong tile for f32 (the shapes at which it does for bf16)
    for M, N, K in ((2236, 1024, 1024), (4472, 4096, 1024), (100, 14336, 4096)):
        big = dict(M=M, N=N, Kc=K, lda=K, ldw=K, rowsA=M, ldc=N)
        assert tile_for(dtype=_lib.BF16, **big) >= 12 and tile_for(dtype=_lib.F32, **big) < 12
    assert sorted(R.TILES) == list(range(15)) and len(R.DT_TILES) == 27


def test_tile_table_matches_the_mirror():
    """usdm_gemm_tile_info against R.TILES / R.DT_TILES, all 15 ids and both dtypes: the GPU tests choose their K values below, at and
    above the pipeline depth from that mirror"""
    from usdm_amd import _lib
    # the mirror's loader names as (waves, DMA, LDS stages, 64-byte chunks per stage, ping-pong)
    loaders = {"reg": (4, 0, 2, 2, 0), "reg8": (8, 0, 2, 2, 0), "dma2": (4, 1, 2, 2, 0), "dma3": (4, 1, 3, 2, 0), "dma4": (4, 1, 4, 2, 0),
               "dma4x1": (4, 1, 4, 1, 0), "pp": (8, 1, 3, 2, 1)}
    out = (C_.c_int32 * 8)()
    for dtype, dt in ((_lib.BF16, BF), (_lib.F32, F32)):
        for t in range(15):
            rc = _lib.lib.usdm_gemm_tile_info(t, dtype, out)
            assert (rc == 0) == ((dt, t) in R.DT_TILES), (dt, t, rc)
            if rc:
                assert rc == 2 and b"usdm_gemm_tile_info" in _lib.lib.usdm_last_error()
                continue
            BM, BN, loader, _ = R.TILES[t]
            assert list(out) == [BM, BN, *loaders[loader], 0], (t, list(out))
    for t, dtype in ((-1, 0), (15, 0), (0, 2)):
        assert _lib.lib.usdm_gemm_tile_info(t, dtype, out) == 2


# ---- which tile the heuristic chooses: recorded from the library of the commit before the launcher was split into gemm_check /
#      gemm_select / gemm_reroute (tests/golden/make_golden.py make_gemm_tiles), replayed here against the library under test
TILE_VARIANTS = ("plain", "batch 2", "batch 8", "split_k 2", "split_k 4", "transposed", "3 taps", "7 taps", "2 sources along K", "head split")
CHOSEN = {BF: (0, 1, 2, 4, 5, 6, 8, 10, 12, 13, 14), F32: (0, 1, 2, 4, 5, 6, 10, 11)}       # every tile the heuristic can choose


def tile_queries(Ms, Ns, Kcs):
    """(dtype, M, N, Kc, variant, keywords of _args) of every query of the grid, in the fixture's order"""
    for dt in (BF, F32):
        for M in Ms:
            for N in Ns:
                for Kc in Kcs:
                    base = dict(dtype=0 if dt == BF else 1, M=M, N=N, Kc=Kc, lda=Kc, ldw=Kc, rowsA=M, ldc=N)
                    split = dict(c_split_stride=M * N)
                    variants = (dict(), dict(batch=2), dict(batch=8), dict(split, split_k=2), dict(split, split_k=4), dict(transpose_out=1),
                                dict(taps=3, ldw=3 * Kc, a_row_step=1), dict(taps=7, ldw=7 * Kc, a_row_step=1),
                                dict(taps=2, ldw=2 * Kc, a_tap_stride=64),
                                dict(epi=1, C32=0, qkv_q=PTR, qkv_k=PTR, qkv_v=PTR, qkv_S=M, qkv_Spad=M, qkv_D=64, qkv_H=N // 192))
                    for name, kw in zip(TILE_VARIANTS, variants):
                        if name != "head split" or N % 192 == 0:
                            yield dt, M, N, Kc, name, dict(base, **kw)


def tile_sweep(lib, Ms, Ns, Kcs):
    """int8 per query of tile_queries: the tile usdm_gemm_tile_for names, or the negative refusal code"""
    import numpy as np
    return np.array([lib.usdm_gemm_tile_for(C_.byref(_args(**kw))) for *_, kw in tile_queries(Ms, Ns, Kcs)], dtype=np.int8)


def test_tile_choice_is_the_recorded_one():
    """the heuristic's choice on 2 dtypes x 27 M x 17 N x 10 Kc x 10 launch forms, refusals included, is the recorded one entry for entry"""
    import os
    import numpy as np
    from usdm_amd import _lib
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_tiles.npz"))
    axes = [[int(v) for v in d[k]] for k in ("M", "N", "Kc")]
    want, got = d["tile"], tile_sweep(_lib.lib, *axes)
    assert want.dtype == np.int8 and want.shape == got.shape and want.size > 80000
    half = want.size // 2
    for dt, part in ((BF, want[:half]), (F32, want[half:])):
        assert sorted(set(part[part >= 0].tolist())) == list(CHOSEN[dt]), (R.dt_name(dt), "the grid no longer reaches every tile the heuristic chooses")
    assert 0 < int((want < 0).sum()) < want.size // 50 and set(want[want < 0].tolist()) == {-2}
    bad = np.nonzero(got != want)[0]
    if bad.size:
        q = list(tile_queries(*axes))
        first = [(R.dt_name(q[i][0]), *q[i][1:5], f"recorded {int(want[i])}, got {int(got[i])}") for i in bad[:5]]
        raise AssertionError(f"{bad.size} of {want.size} tile choices differ from the recorded ones, first: {first}")
