"""usdm_attn_verify_batch (verify attention for B slots x T rows) through the C-ABI: every slot's out rows and WHOLE cache equal (==)
usdm_attn_verify on a copy of that slot's cache - which carries over that kernel's position invariance, key visibility and fp64 parity
(tests/test_spec_attn_gpu.py) - plus a direct float64 comparison, the per-slot skip, the context end next to another slot, and the
launcher's refusals.  Shapes: ctx_max 256, C = 64 (four splits), Hkv 2, head_dim 128."""
import numpy as np
import pytest
import torch

from tests import _spec_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CM, C, HKV, D = 256, 64, 2, 128
SCALE = D ** -0.5
SENT = 777.0
SHAPES = ((2, 8), (4, 4), (8, 2), (3, 5), (16, 1), (1, 8))
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
    """per G: 16 x 8 qkv rows and 16 slots' random caches (bf16, host), computed once and never changed"""
    if G not in _CACHE:
        nq = (HKV * G + 2 * HKV) * D
        _CACHE[G] = (_r((16 * 8, nq), 40 + G).to(BF), _r((16, HKV, CM, D), 50 + G).to(BF), _r((16, HKV, CM, D), 60 + G).to(BF))
    return _CACHE[G]


def _positions(B, T, seed):
    choices = (0, 1, 62, 63, 64, 65, 125, CM - T)
    return [int(p) for p in np.random.default_rng(seed).choice(choices, B)]


def _scratch(dev, rows, Hq):
    ns = CM // C
    return [torch.zeros(rows * Hq * ns * n, dtype=torch.float32, device=dev) for n in (1, 1, D)]


def _batch(dev, qkv, pos, kc, vc, *, G, B, T, window=0, skip=None, out=None, **kw):
    """one batched launch on the device caches kc / vc [B][Hkv][CM][D] (written in place) -> out [B*T][Hq*128]"""
    from usdm_amd import ops
    Hq = HKV * G
    cos, sin = _dev_tables(dev)
    pm, pl, po = _scratch(dev, 16, Hq)
    out = torch.full((max(B * T, 1), Hq * D), SENT, dtype=BF, device=dev) if out is None else out
    a = dict(qkv=qkv.to(dev), pos=torch.tensor(pos, dtype=torch.int32, device=dev), cos=cos, sin=sin, kcache=kc, vcache=vc, pm=pm, pl=pl, po=po,
             out=out, B=B, T=T, Hq=Hq, Hkv=HKV, ctx_max=CM, C=C, scale=SCALE, cache_bs=HKV * CM * D, window=window,
             skip=None if skip is None else torch.tensor(skip, dtype=torch.int32, device=dev))
    a.update(kw)
    ops.attn_verify_batch(a.pop("qkv"), a.pop("pos"), a.pop("cos"), a.pop("sin"), a.pop("kcache"), a.pop("vcache"), a.pop("pm"), a.pop("pl"),
                          a.pop("po"), a.pop("out"), **a)
    return out


def _single(dev, qkv, pos, kc, vc, *, G, window=0):
    """the single-sequence kernel on one slot's device cache (written in place) -> out [T][Hq*128], sentinel-filled before"""
    from usdm_amd import ops
    Hq, T = HKV * G, qkv.shape[0]
    cos, sin = _dev_tables(dev)
    pm, pl, po = _scratch(dev, 8, Hq)
    out = torch.full((T, Hq * D), SENT, dtype=BF, device=dev)
    ops.attn_verify(qkv.to(dev), torch.tensor([pos], dtype=torch.int32, device=dev), cos, sin, kc, vc, pm, pl, po, out, T=T, Hq=Hq, Hkv=HKV,
                    ctx_max=CM, C=C, scale=SCALE, window=window)
    return out


@pytest.mark.parametrize("G", [1, 2, 4])
def test_every_slot_equals_the_single_sequence_kernel(dev, G):
    """(B, T) x window, every slot with its own random cache and its own position (different splits and tiles in one launch): out rows
    and the slot's whole cache == usdm_attn_verify's on a copy of that slot's cache."""
    qa, kc0, vc0 = _inputs(G)
    for n, (B, T) in enumerate(SHAPES):
        pos = _positions(B, T, 100 * G + n)
        qkv = qa[:B * T]
        for window in (0, 40, 69):
            kc, vc = kc0[:B].to(dev), vc0[:B].to(dev)
            out = _batch(dev, qkv, pos, kc, vc, G=G, B=B, T=T, window=window)
            for b in range(B):
                k1, v1 = kc0[b].to(dev), vc0[b].to(dev)
                o1 = _single(dev, qkv[b * T:(b + 1) * T], pos[b], k1, v1, G=G, window=window)
                what = (B, T, window, b, pos[b])
                assert torch.equal(out[b * T:(b + 1) * T], o1), ("out rows", what)
                assert torch.equal(kc[b], k1) and torch.equal(vc[b], v1), ("cache", what)
                assert not bool((o1 == SENT).all())


@pytest.mark.parametrize("G", [1, 2, 4])
def test_parity_with_fp64(dev, G):
    """one case per G against the float64 reference directly, at the project's tolerance for decode attention (2e-2 of the largest
    reference value, tests/test_spec_attn_gpu.py)"""
    B, T, window = 2, 8, 40
    qa, kc0, vc0 = _inputs(G)
    pos = [65, 125]
    kc, vc = kc0[:B].to(dev), vc0[:B].to(dev)
    out = _batch(dev, qa[:B * T], pos, kc, vc, G=G, B=B, T=T, window=window).cpu().double()
    for b in range(B):
        ref, _, kr, vr = R.attn_verify_ref(qa[b * T:(b + 1) * T], kc0[b], vc0[b], pos[b], Hq=HKV * G, Hkv=HKV, window=window, scale=SCALE,
                                           tables=_tables())
        err = (out[b * T:(b + 1) * T] - ref).abs().max().item() / ref.abs().max().item()
        print(f"[spec-batch-attn] G={G} slot {b}: |out - ref| / max|ref| = {err:.2e} (bound 2e-2)")
        assert err <= 2e-2, (G, b, err)
        assert torch.equal(kc[b, :, pos[b]:pos[b] + T].cpu(), kr.transpose(0, 1)) and torch.equal(vc[b, :, pos[b]:pos[b] + T].cpu(), vr.transpose(0, 1))


def test_per_slot_skip(dev):
    """skip[b] != 0: slot b keeps its cache and its sentinel-filled out rows; its neighbours equal the launch without the skip"""
    G, B, T = 2, 4, 4
    qa, kc0, vc0 = _inputs(G)
    pos = [63, 64, 0, 125]
    kf, vf = kc0[:B].to(dev), vc0[:B].to(dev)
    full = _batch(dev, qa[:B * T], pos, kf, vf, G=G, B=B, T=T, skip=[0, 0, 0, 0])
    for skipped in ([0, 1, 0, 0], [1, 0, 0, 1]):
        kc, vc = kc0[:B].to(dev), vc0[:B].to(dev)
        out = _batch(dev, qa[:B * T], pos, kc, vc, G=G, B=B, T=T, skip=skipped)
        for b in range(B):
            rows = slice(b * T, (b + 1) * T)
            if skipped[b]:
                assert bool((out[rows] == SENT).all()) and torch.equal(kc[b].cpu(), kc0[b]) and torch.equal(vc[b].cpu(), vc0[b]), b
            else:
                assert torch.equal(out[rows], full[rows]) and torch.equal(kc[b], kf[b]) and torch.equal(vc[b], vf[b]), b


def test_context_end_stays_inside_its_slot(dev):
    """slot 0 at pos = ctx_max - 1 with T = 4 appends one row and writes one out row; the NEXT slot's cache and out rows equal those of
    a launch in which slot 0 is skipped, and no sentinel around the caches is touched"""
    G, B, T, pad = 4, 2, 4, 4096
    qa, kc0, vc0 = _inputs(G)
    pos = [CM - 1, 64]
    n = kc0[:B].numel()

    def padded(c0):
        buf = torch.full((pad + n + pad,), SENT, dtype=BF)
        buf[pad:pad + n] = c0[:B].reshape(-1)
        buf = buf.to(dev)
        return buf, buf[pad:pad + n].view(B, HKV, CM, D)

    (kb, kc), (vb, vc) = padded(kc0), padded(vc0)
    out = _batch(dev, qa[:B * T], pos, kc, vc, G=G, B=B, T=T)
    k2, v2 = kc0[:B].to(dev), vc0[:B].to(dev)
    out2 = _batch(dev, qa[:B * T], pos, k2, v2, G=G, B=B, T=T, skip=[1, 0])
    assert torch.equal(out[T:], out2[T:]) and torch.equal(kc[1], k2[1]) and torch.equal(vc[1], v2[1]), "slot 1 depends on slot 0's rows"
    assert bool((out[1:T] == SENT).all()) and not bool((out[0] == SENT).any()), "exactly one out row of slot 0 is written"
    k1, v1 = kc0[0].to(dev), vc0[0].to(dev)
    o1 = _single(dev, qa[:T], CM - 1, k1, v1, G=G)
    assert torch.equal(out[:T], o1) and torch.equal(kc[0], k1) and torch.equal(vc[0], v1)
    assert torch.equal(kc[0, :, :CM - 1].cpu(), kc0[0, :, :CM - 1]) and not torch.equal(kc[0, :, CM - 1].cpu(), kc0[0, :, CM - 1])
    for buf in (kb, vb):
        assert bool((buf[:pad] == SENT).all()) and bool((buf[-pad:] == SENT).all()), "a sentinel outside the caches was written"


def test_launcher_refusals(dev):
    """every refusal is an error (no fall-back): B < 1, T outside 1 .. 8, B * T > 16, a slot stride smaller than one slot's cache, and
    what usdm_attn_verify refuses"""
    from usdm_amd._lib import UsdmError
    G = 2
    qa, kc0, vc0 = _inputs(G)
    kc, vc = kc0.to(dev), vc0.to(dev)

    def go(B=2, T=2, **kw):
        return _batch(dev, qa, [0] * max(B, 1), kw.pop("kc", kc), kw.pop("vc", vc), G=kw.pop("G", G), B=B, T=T, **kw)

    go()
    odd = torch.zeros(kc0.numel() + 8, dtype=BF, device=dev)[1:1 + kc0.numel()].view(16, HKV, CM, D)      # 2-byte aligned only
    bad = [("B = 0", dict(B=0)), ("B = -1", dict(B=-1)), ("T = 0", dict(T=0)), ("T = 9", dict(B=1, T=9)), ("B * T = 18", dict(B=3, T=6)),
           ("B * T = 17", dict(B=17, T=1)), ("slot stride below a slot's cache", dict(cache_bs=HKV * CM * D - 8)),
           ("slot stride 0", dict(cache_bs=0)), ("misaligned slot stride", dict(cache_bs=HKV * CM * D + 4)),
           ("C = 48", dict(C=48)), ("C = 320", dict(C=320)), ("C = 0", dict(C=0)), ("window < 0", dict(window=-1)),
           ("NULL cache", dict(kcache=None)), ("NULL pm", dict(pm=None)), ("NULL sin", dict(sin=None)), ("misaligned K cache", dict(kc=odd)),
           ("G = 3", dict(Hq=6)), ("more than 64 splits", dict(ctx_max=64 * 65))]
    for what, kw in bad:
        with pytest.raises(UsdmError):
            go(**kw)
            pytest.fail(f"{what} was accepted")
    assert torch.equal(kc.cpu()[:, :, 2:], kc0[:, :, 2:])
