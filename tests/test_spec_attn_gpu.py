"""usdm_attn_verify (decode attention for T new tokens of one sequence) through the C-ABI: parity with a float64 reference and with
T successive usdm_attn_decode calls, position invariance (==), exact key visibility and softmax weights (the one-hot V probes of
tests/_attn_probe.py), bounds, skip and the launcher's refusals.  Shapes: ctx_max 256, C = 64 (four splits, tiles = splits), Hkv 2."""
import pytest
import torch

from tests import _attn_probe as P
from tests import _spec_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CM, C, HKV, D = 256, 64, 2, 128
SCALE = D ** -0.5
_CACHE = {}


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables():
    if "tab" not in _CACHE:
        _CACHE["tab"] = R.rope_tables(CM)
    return _CACHE["tab"]


def _dev_tables(dev):
    if "dtab" not in _CACHE:
        cosf, sinf = _tables()
        _CACHE["dtab"] = (cosf[:, :64].contiguous().to(dev), sinf[:, :64].contiguous().to(dev))
    return _CACHE["dtab"]


def _inputs(G):
    """one sequence per G: a qkv row for every position and random caches (bf16), computed once"""
    if ("in", G) not in _CACHE:
        nq = (HKV * G + 2 * HKV) * D
        _CACHE[("in", G)] = (_r((CM, nq), 10 + G).to(BF), _r((HKV, CM, D), 20 + G).to(BF), _r((HKV, CM, D), 30 + G).to(BF))
    return _CACHE[("in", G)]


def _verify(dev, qkv, pos, kc, vc, *, G, T=None, window=0, Cs=C, skip=None, out=None, ctx_max=CM, Hq=None, **kw):
    """one launch on device tensors kc / vc (written in place) -> out [T][Hq*128] bf16 on the device"""
    from usdm_amd import ops
    T = qkv.shape[0] if T is None else T
    Hq = HKV * G if Hq is None else Hq
    ns = ops.attn_verify_splits(ctx_max, Cs) if Cs > 0 else 1
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    out = torch.zeros(max(T, 1), Hq * D, dtype=BF, device=dev) if out is None else out
    cos, sin = _dev_tables(dev)
    args = dict(qkv=qkv.to(dev), pos=torch.tensor([pos], dtype=torch.int32, device=dev), cos=cos, sin=sin, kcache=kc, vcache=vc,
                pm=f32(8 * Hq * ns), pl=f32(8 * Hq * ns), po=f32(8 * Hq * ns * D), out=out)
    args.update(kw)
    ops.attn_verify(args["qkv"], args["pos"], args["cos"], args["sin"], args["kcache"], args["vcache"], args["pm"], args["pl"], args["po"],
                    args["out"], T=T, Hq=Hq, Hkv=HKV, ctx_max=ctx_max, C=Cs, scale=SCALE, window=window, skip=skip)
    return out


POSITIONS = lambda T: (0, 1, 62, 63, 64, 65, 125, CM - T)


@pytest.mark.parametrize("G", [1, 2, 4])
def test_parity_with_fp64_and_with_successive_decode_steps(dev, G):
    """out vs the float64 reference at the tolerance tests/test_llm_gpu.py::test_attn_decode uses for usdm_attn_decode (2e-2 of the
    largest reference value); the appended K / V rows == those of T successive usdm_attn_decode calls, every other row untouched."""
    from usdm_amd import ops
    qa, kc0, vc0 = _inputs(G)
    Hq, worst = HKV * G, 0.0
    cos, sin = _dev_tables(dev)
    for T in (1, 2, 4, 8):
        for pos in POSITIONS(T):
            qkv = qa[pos:pos + T]
            for window in (0, 40, 69):
                kc, vc = kc0.to(dev), vc0.to(dev)
                out = _verify(dev, qkv, pos, kc, vc, G=G, window=window)
                ref, _, kr, vr = R.attn_verify_ref(qkv, kc0, vc0, pos, Hq=Hq, Hkv=HKV, window=window, scale=SCALE, tables=_tables())
                err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
                worst = max(worst, err)
                assert err <= 2e-2, (T, pos, window, err)
                # T successive single-token steps on a copy of the same cache
                kd, vd = kc0.to(dev), vc0.to(dev)
                o1 = torch.zeros(Hq * D, dtype=BF, device=dev)
                pm, pl, po = (torch.zeros(Hq * 2 * n, device=dev) for n in (1, 1, D))
                for i in range(T):
                    ops.attn_decode(qkv[i].to(dev), torch.tensor([pos + i], dtype=torch.int32, device=dev), cos, sin, kd, vd, pm, pl, po, o1,
                                    Hq=Hq, Hkv=HKV, ctx_max=CM, NS=2, scale=SCALE, window=window)
                assert torch.equal(kc, kd) and torch.equal(vc, vd), (T, pos, "appended rows differ from usdm_attn_decode's")
                assert torch.equal(kc[:, pos:pos + T].cpu(), kr.transpose(0, 1)) and torch.equal(vc[:, pos:pos + T].cpu(), vr.transpose(0, 1))
                keep = torch.ones(CM, dtype=torch.bool)
                keep[pos:pos + T] = False
                assert torch.equal(kc.cpu()[:, keep], kc0[:, keep]) and torch.equal(vc.cpu()[:, keep], vc0[:, keep])
    print(f"[spec-attn] G={G}: worst |out - ref| / max|ref| = {worst:.2e} (bound 2e-2)")


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("window", [0, 40])
def test_position_invariance(dev, G, window):
    """The token at absolute position p, computed as row i of a step based at p - i for every i < T and every T: outputs and appended
    rows are equal with ==.  The cache holds the sequence's own rows below the base and 1e3 from the base on (never read)."""
    qa, _, _ = _inputs(G)
    Hq, tab = HKV * G, _tables()
    rows = qa.view(CM, Hq + 2 * HKV, D)
    K_all = torch.stack([R.rope_rows(rows[p, Hq:Hq + HKV], p, tab) for p in range(CM)], 1)      # [Hkv, CM, 128]
    V_all = rows[:, Hq + HKV:].transpose(0, 1).contiguous()
    for p in (63, 64, 130):
        first = None
        for T in (1, 2, 4, 8):
            for i in range(T):
                base = p - i
                kc, vc = K_all.clone(), V_all.clone()
                kc[:, base:], vc[:, base:] = P.PAD_BIG, P.PAD_BIG
                kc, vc = kc.to(dev), vc.to(dev)
                out = _verify(dev, qa[base:base + T], base, kc, vc, G=G, window=window)
                got = (out[i].cpu(), kc[:, p].cpu(), vc[:, p].cpu())
                if first is None:
                    first = got
                    assert torch.equal(got[1], K_all[:, p]) and torch.equal(got[2], V_all[:, p])
                for a, b, what in zip(got, first, ("out", "K row", "V row")):
                    assert torch.equal(a, b), f"p={p} T={T} row {i}: {what} differs from the T=1 step's"


@pytest.mark.parametrize("G", [1, 2, 4])
def test_visibility_and_weights(dev, G):
    """One-hot V probes (tests/_attn_probe.py): column c of output row i is the softmax weight of key j0 + c.  Every row's visible
    key set is exact - the step's own earlier rows and the window's lower edge included - and the weights match fp64 at that file's
    tolerance.  The cache rows the step writes hold 1e3 before the launch: own rows must come from LDS."""
    qa, kc0, _ = _inputs(G)
    Hq = HKV * G
    tot = P.Stats()
    cols = torch.arange(D)
    for T, pos in ((8, 0), (8, 60), (3, 125), (8, CM - 8), (1, 64)):
        for window in (0, 40, 69):
            qkv = qa[pos:pos + T].clone()
            q3 = qkv.view(T, Hq + 2 * HKV, D)
            kc_in = kc0.clone()
            kc_in[:, pos:pos + T] = P.PAD_BIG
            parts = []
            for j0 in range(0, CM, D):
                vc = torch.zeros(HKV, CM, D)
                vc[:, j0 + cols, cols] = 1.0
                vc[:, pos:pos + T] = P.PAD_BIG
                q3[:, Hq + HKV:] = 0
                for i in range(T):
                    if j0 <= pos + i < j0 + D:
                        q3[i, Hq + HKV:, pos + i - j0] = 1.0
                out = _verify(dev, qkv, pos, kc_in.to(dev), vc.to(BF).to(dev), G=G, window=window)
                parts.append(out.view(T, Hq, D).float().cpu())
            _, wts, _, _ = R.attn_verify_ref(qkv, kc0, torch.zeros_like(kc0), pos, Hq=Hq, Hkv=HKV, window=window, scale=SCALE, tables=_tables())
            j = torch.arange(CM).view(1, 1, CM)
            p = (pos + torch.arange(T)).view(T, 1, 1)
            vis = (j <= p) & ((j > p - window) if window > 0 else torch.ones_like(j, dtype=torch.bool))
            vis = vis.expand(T, Hq, CM)
            assert bool((wts[~vis] == 0).all())
            tot.add(P.check_weights(lambda: torch.cat(parts, -1), wts, vis, what=f"verify G={G} T={T} pos={pos} window={window}"))
    print(tot.line(f"usdm_attn_verify G={G}"))


def test_bounds_rows_past_the_cache_are_neither_appended_nor_computed(dev):
    """The caches sit inside a larger buffer of sentinels, *pos = ctx_max - 2, T = 4: rows 0 and 1 are correct and appended, rows 2 and
    3 are not computed, and no sentinel - around the caches, in out rows 2 / 3 - is touched."""
    G, T, pos, pad = 4, 4, CM - 2, 4096
    qa, kc0, vc0 = _inputs(G)
    Hq, SENT = HKV * G, 777.0
    bufs = []
    for c0 in (kc0, vc0):
        b = torch.full((pad + c0.numel() + pad,), SENT, dtype=BF)
        b[pad:pad + c0.numel()] = c0.reshape(-1)
        bufs.append(b.to(dev))
    kc, vc = (b[pad:pad + kc0.numel()].view(HKV, CM, D) for b in bufs)
    qkv = torch.cat([qa[pos:pos + 2], qa[:2]])
    out = torch.full((T, Hq * D), SENT, dtype=BF, device=dev)
    _verify(dev, qkv, pos, kc, vc, G=G, out=out)
    ref, _, kr, vr = R.attn_verify_ref(qkv, kc0, vc0, pos, Hq=Hq, Hkv=HKV, window=0, scale=SCALE, tables=_tables())
    assert ref.shape[0] == 2
    assert (out[:2].cpu().double() - ref).abs().max() <= 2e-2 * ref.abs().max()
    assert bool((out[2:] == SENT).all()), "a row at a position >= ctx_max was computed"
    for b in bufs:
        assert bool((b[:pad] == SENT).all()) and bool((b[-pad:] == SENT).all()), "a sentinel outside the cache was written"
    assert torch.equal(kc[:, pos:].cpu(), kr.transpose(0, 1)) and torch.equal(vc[:, pos:].cpu(), vr.transpose(0, 1))
    assert torch.equal(kc[:, :pos].cpu(), kc0[:, :pos]) and torch.equal(vc[:, :pos].cpu(), vc0[:, :pos])


def test_skip_leaves_cache_and_output_unchanged(dev):
    G, T, pos = 2, 4, 70
    qa, kc0, vc0 = _inputs(G)
    kc, vc = kc0.to(dev), vc0.to(dev)
    out = torch.full((T, HKV * G * D), 5.0, dtype=BF, device=dev)
    _verify(dev, qa[pos:pos + T], pos, kc, vc, G=G, out=out, skip=torch.ones(1, dtype=torch.int32, device=dev))
    assert torch.equal(kc.cpu(), kc0) and torch.equal(vc.cpu(), vc0) and bool((out == 5.0).all())
    _verify(dev, qa[pos:pos + T], pos, kc, vc, G=G, out=out, skip=torch.zeros(1, dtype=torch.int32, device=dev))
    assert not torch.equal(kc.cpu(), kc0) and not bool((out == 5.0).any())


def test_launcher_refusals(dev):
    """every refusal is an error (no fall-back): T outside 1 .. 8, unsupported G, NULL or misaligned pointers, C no multiple of the
    key tile / out of range"""
    from usdm_amd._lib import UsdmError
    G = 2
    qa, kc0, vc0 = _inputs(G)
    kc, vc = kc0.to(dev), vc0.to(dev)
    ok = lambda **kw: _verify(dev, qa[:kw.pop("rows", 2)], 0, kw.pop("kc", kc), kw.pop("vc", vc), G=kw.pop("G", G), **kw)
    ok()
    q3 = _r((2, (6 + 4) * D), 3).to(BF)
    odd = torch.zeros(kc0.numel() + 8, dtype=BF, device=dev)[1:1 + kc0.numel()].view(HKV, CM, D)      # 2-byte aligned only
    bad = [("T = 0", dict(T=0)), ("T = 9", dict(rows=9)), ("C = 48", dict(Cs=48)), ("C = 32", dict(Cs=32)), ("C = 320", dict(Cs=320)),
           ("C = 0", dict(Cs=0)), ("window < 0", dict(window=-1)), ("NULL cache", dict(kcache=None)), ("NULL pm", dict(pm=None)),
           ("NULL sin", dict(sin=None)), ("misaligned K cache", dict(kc=odd)), ("misaligned V cache", dict(vc=odd))]
    for what, kw in bad:
        with pytest.raises(UsdmError):
            ok(**kw)
            pytest.fail(f"{what} was accepted")
    with pytest.raises(UsdmError):      # G = 3
        _verify(dev, q3, 0, kc, vc, G=3, Hq=6)
    with pytest.raises(UsdmError):      # more than 64 splits
        _verify(dev, qa[:2], 0, kc, vc, G=G, ctx_max=64 * 65)
    assert torch.equal(kc.cpu()[:, 2:], kc0[:, 2:])
