"""usdm_gemm against the exact integer reference of tests/_gemm_reference.py: every tile instantiation (bf16 0 ... 14, f32 0 ... 11,
forced with USDM_GEMM_TILE and confirmed with usdm_gemm_tile_for before each launch), every loader at K below, at and above its
pipeline depth, every epilogue branch, with NaN in every operand gap and the sentinel around every output.  Plain cases compare bit
patterns; activations compare with the fp64 activation of the exact pre-activation within 4 x torch's own float32 error."""
import pytest
import torch

from tests import _gemm_reference as R
from tests._gemm_reference import BF, F32, F64, TILES

pytestmark = pytest.mark.gpu

MAIN_TILES = [(dt, t) for dt in (BF, F32) for t in range(4)]
DMA_TILES = [(dt, t) for dt in (BF, F32) for t in range(4, 12)]
PP = [(BF, t) for t in R.PP_TILES]


@pytest.fixture
def force(monkeypatch):
    return lambda t: monkeypatch.setenv("USDM_GEMM_TILE", str(t))


def _launch(c, dev, forced, fill=None):
    """run the case's launches into sentinel-filled outputs -> {name: flat CPU tensor}; asserts the tile that runs"""
    from usdm_amd import ops
    up = lambda t: None if t is None else t.to(dev)

    def buf(size, dtype, off=0):
        t = R.sentinel((size + off,), dtype, dev) if fill is None else torch.full((size + off,), fill, dtype=dtype, device=dev)
        return t[off:]
    A, bias, res = c.A.to(dev)[c.A_off:], up(c.bias), up(c.res)
    e = R.expected(c)
    out = {}
    if c.qkv is not None:
        out = {n: buf(e[n].vals.numel(), BF, c.qkv.get(n + "_off", 0)) for n in "qkv"}
    else:
        if c.want32:
            out["out32"] = buf(c.out_size, F32)
        if c.want16:
            out["out16"] = buf(c.out_size, BF)
    if c.stats:
        out["stats"] = buf(c.stats_size, F32)
    for kw, W, _ in c.launches:
        args = dict(kw, bias=bias, residual=res, out32=out.get("out32"), out16=out.get("out16"), stats_out=out.get("stats"))
        if c.qkv is not None:
            args["qkv"] = dict(S=c.qkv["S"], Spad=c.qkv["Spad"], H=c.qkv["H"], D=c.qkv["D"], q=out["q"], k=out["k"], v=out["v"])
        multi = kw["taps"] > 1
        want = R.expected_tile(c.dt, forced, multi_tap=multi, concat=multi and kw["a_row_step"] == 0 and kw["Kc"] % 64 == 0,
                               transpose=kw["transpose_out"], head_split=c.qkv is not None)
        Wd = W.to(dev)
        assert ops.gemm(A, Wd, tile_query=True, **args) == want, f"{c.name}: forced tile {forced} should run as {want}"
        ops.gemm(A, Wd, **args)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in out.items()}


def _check_split(c, dev, forced, got, e):
    """split-K: the exact sum of the partials is the reference (bias and residual counted once), no partial's block keeps a sentinel,
    the gaps between the partials and the guards inside them do"""
    S, part = c.kw["split_k"], c.part_size
    own = e.owned[:part]
    owned = torch.cat([own, torch.zeros(c.kw["c_split_stride"] - part, dtype=torch.bool)]).repeat(S)
    stray = ~R.is_sentinel(got) & ~owned
    assert not bool(stray.any()), f"{c.name}: {int(stray.sum())} elements written outside the partials, first at {int(stray.nonzero()[0])}"
    total = got.double().view(S, -1).sum(0)[:part]
    bad = (total != e.vals[:part]) & own
    assert not bool(bad.any()), f"{c.name}: the partials' sum differs on {int(bad.sum())} of {int(own.sum())} elements, first at {int(bad.nonzero()[0])}"
    kept = R.is_sentinel(got) & owned
    if bool(kept.any()):       # a partial sum may BE 7.0: such an element holds 7.0 again over another fill, an unwritten one does not
        again = _launch(c, dev, forced, fill=-R.SENT32)["out32"]
        assert bool(R.is_sentinel(again)[kept].all()), f"{c.name}: {int((~R.is_sentinel(again)[kept]).sum())} elements of the partials never written"


def _same16(c, got, own):
    """wherever one launch writes out32 and out16, out16 is out32 rounded to bf16, bit for bit"""
    if "out32" in got and "out16" in got:
        assert torch.equal(R.bits(got["out16"])[own], R.bits(got["out32"].to(BF))[own]), f"{c.name}: out16 is not out32 rounded to bf16"


def _check_act(c, got, e):
    act, rbf = c.kw["act"], c.kw["round_bf16"]
    own, ref = e.owned, e.vals
    g32, g16 = got.get("out32"), got.get("out16")
    if rbf:                    # SwiGLU with four bf16 rounding points: within one bf16 ulp, at most FLIP_CAP of the outputs differ at all
        for name, g in got.items():
            R.check_guard(f"{c.name} {name}", g, e, R.bf16_ulp(ref))
            d = (g.double() - ref).abs()[own]
            print(f"[gemm] {c.name} {name}: {int((d != 0).sum())} of {d.numel()} differ, worst {float((d / R.bf16_ulp(ref[own])).max()):.2f} bf16 ulp")
            assert bool((d <= R.bf16_ulp(ref[own])).all()) and int((d != 0).sum()) <= R.FLIP_CAP * d.numel(), (c.name, name)
        return _same16(c, got, own)
    tol = R.act_tolerance(act, e)
    if g32 is not None:
        R.check_guard(f"{c.name} out32", g32, e, tol)
        err = torch.where(own, (g32.double() - ref).abs(), torch.zeros((), dtype=F64))
        worst = float((err[own] / tol[own]).nan_to_num(0.0).max()) * 4
        print(f"[gemm] {c.name} out32: worst error {worst:.2f} x the recorded float32 error of {R.ACT_NAMES[act]} (bound 4)")
        assert bool((err <= tol).all()), f"{c.name}: {worst:.2f} x GEMM_{R.ACT_NAMES[act].upper()}_TORCH_FP32_ERR"
        _same16(c, got, own)
    elif g16 is not None:      # bf16 only: the f32 bound plus half a bf16 ulp of the reference
        R.check_guard(f"{c.name} out16", g16, e, tol)
        err = torch.where(own, (g16.double() - ref).abs(), torch.zeros((), dtype=F64))
        bound = torch.where(own, R.bf16_of_f32_bound(ref, tol), torch.zeros((), dtype=F64))
        print(f"[gemm] {c.name} out16: worst error / bound {float((err[own] / bound[own]).nan_to_num(0.0).max()):.3f}")
        assert bool((err <= bound).all()), c.name


def run_case(c, dev, forced):
    e = R.expected(c)
    got = _launch(c, dev, forced)
    if c.qkv is not None:
        for n in "qkv":
            R.check_exact(f"{c.name} {n}", got[n], e[n])
        return
    o = e["out"]
    if c.kw["split_k"]:
        return _check_split(c, dev, forced, got["out32"], o)
    if not c.exact:
        return _check_act(c, got, o)
    for n in ("out32", "out16"):
        if n in got:
            R.check_exact(f"{c.name} {n}", got[n], o)
    _same16(c, got, o.owned)
    if c.stats:                # (sum, M2) per row and 128-column tile: the sums bit-exact, M2 within M2_BOUND of the reference
        st, g = e["stats"], got["stats"]
        R.check_guard(f"{c.name} stats", g, st, 0.0)
        is_sum = torch.arange(g.numel()) % 2 == 0
        s1 = st.owned & is_sum
        assert torch.equal(R.bits(g[s1]), R.bits(st.vals[s1].float())), f"{c.name}: row sums"
        m2 = st.owned & ~is_sum
        rel = ((g[m2].double() - st.vals[m2]).abs() / st.vals[m2])
        print(f"[gemm] {c.name}: M2 worst relative error {float(rel.max()):.3g} (bound {R.M2_BOUND:.3g})")
        assert bool((rel <= R.M2_BOUND).all()), c.name


def _run_group(group, dev, force, p, **kw):
    dt, t = p
    force(t)
    for c in R.GROUPS[group](dt, *TILES[t][:2], **kw):
        run_case(c, dev, t)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_k_ladder(dev, force, p):
    """a. Linear with bias, alpha, an f32 residual, out32 and out16, at 1/2 ... 8 1/2 K-steps"""
    _run_group("k_ladder", dev, force, p)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_edges(dev, force, p):
    """b. M = 1 / BM / BM + 1, 12 tiles (the XCD remap), ragged N on the vector and the scalar path, bf16 residual, round_bf16's two
    rounding points, one output only, batch with c_row_mul / c_row_off, groups with c_gcol"""
    _run_group("edges", dev, force, p)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_transposed_output(dev, force, p):
    """c. transpose_out with bias and residual, M % 4 != 0, ldc a multiple of 4 and not (tile 13 runs as 12)"""
    _run_group("transposed", dev, force, p)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_head_split(dev, force, p):
    """d. Q, K -> [B][H][Spad][D], V -> [B][H][D][Spad]; the padding keeps the sentinel (tile 13 runs as 12); ping-pong tiles: also
    with q or k off 16-byte alignment (the narrow path)"""
    _run_group("head_split", dev, force, p, pp=p[1] in R.PP_TILES)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_split_k(dev, force, p):
    """e. S = 2, 3, 4, 16 with equal shares, a short last share and empty shares"""
    _run_group("split_k", dev, force, p)


@pytest.mark.parametrize("p", MAIN_TILES, ids=R.tile_id)
def test_multi_tap(dev, force, p):
    """f. Conv1d (k = 3; k = 7 dilated; stride 2), ConvTranspose1d as four phases, grouped batched conv, two sources along K"""
    _run_group("multi_tap", dev, force, p)


@pytest.mark.parametrize("p", PP, ids=R.tile_id)
def test_two_sources_on_the_pingpong_tiles(dev, force, p):
    force(p[1])
    run_case(R.concat_case(p[0], *TILES[p[1]][:2]), dev, p[1])


@pytest.mark.parametrize("p", DMA_TILES + PP + [(F32, t) for t in R.PP_TILES], ids=R.tile_id)
def test_multi_tap_reroutes(dev, force, p):
    """multi-tap operands forced to an LDS-DMA tile run on the register-staged tile of the same size (4 / 9 / 11 -> 0, 6 / 10 -> 1,
    5 / 7 / 8 -> 2), and a convolution forced to a ping-pong tile on tile 0; f32 forced to 12 ... 14 runs tile 2"""
    dt, t = p
    force(t)
    ran = R.expected_tile(dt, t, multi_tap=True)
    assert ran == {4: 0, 9: 0, 11: 0, 6: 1, 10: 1, 5: 2, 7: 2, 8: 2, 12: 0, 13: 0, 14: 0}[t]
    run_case(R.conv_case("conv k3", dt, *TILES[ran][:2], 600, k=3), dev, t)
    if t < 12:
        run_case(R.concat_case(dt, *TILES[ran][:2]), dev, t)
    elif dt == F32:
        assert R.expected_tile(dt, t) == 2
        run_case(R.k_ladder_cases(dt, 64, 64)[5], dev, t)


@pytest.mark.parametrize("p", R.DT_TILES, ids=R.tile_id)
def test_activations(dev, force, p):
    """g. GELU (out32; out16 only on the packed and the generic path; + residual; transposed), TANH, LOGCLAMP, SWIGLU, SWIGLU with
    round_bf16, on exact pre-activations.  Measured on an MI355X, in units of the recorded float32 error (bound 4), the same on
    every tile: GELU 0.69 (2.25 with a residual, whose addition rounds once more), TANH 1.24, LOGCLAMP 1.98, SWIGLU 0.85; the bf16-only
    GELU outputs reach 0.84 of their bound; SWIGLU with round_bf16 differs from the fp64 reference on none of its outputs."""
    _run_group("activations", dev, force, p)


@pytest.mark.parametrize("p", PP, ids=R.tile_id)
def test_layernorm_statistics(dev, force, p):
    """h. stats_out: per row and 128-column tile the sum (bit-exact) and M2 about the tile's mean"""
    dt, t = p
    force(t)
    for c in R.stats_cases(dt, *TILES[t][:2]):
        run_case(c, dev, t)
