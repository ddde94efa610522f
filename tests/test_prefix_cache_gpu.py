"""GPU: usdm_kv_expand (prefix caching where the prefill attention's V^T is per-plan scratch: batch slots, FP8 cache).  The kernel
moves and converts exactly - every dequantized e4m3 row is a bf16 value - so every check is bit equality: against the transpose of a
bf16 cache, against quant.dequantize_kv_rows evaluated on the CPU for an FP8 cache, and, fed to usdm_attention next to the rope
launch's new rows, against the single sequence's cache + persistent V^T holding the same values."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HKV, CTX = 2, 192
SENT = 0x7B5A      # the sentinel, as bf16 bits (a finite value no test row holds)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _guarded(dev, *shape, guard=512):
    """a bf16 [shape] view in the middle of a sentinel-filled buffer -> (whole buffer, view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((guard + n + guard,), SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return buf, buf[guard:guard + n].view(*shape)


def _is_sent(t):
    return bool((_bits(t) == SENT).all())


def _corner_rows():
    """bf16 [n][128] rows at the quantizer's corners: a zero row, both exponent clamps (the upper one saturating at 448), a row whose
    maximum lands on the largest byte (448 = 0x7e) exactly, bf16 subnormals, -0.0 and a lone outlier."""
    g = torch.Generator().manual_seed(7)
    base = torch.randn(128, generator=g).clamp(-1.5, 1.5) * 0.4
    top = base.clone(); top[9] = -448.0 * 2.0 ** -3                  # amax = 448 * 2^e exactly: the byte 0x7e / 0xfe
    big = base * 2.0e38; big[3], big[77] = 3.3e38, -3.0e38            # above 448 * 2^119: the upper clamp, saturated
    tiny = torch.zeros(128); tiny[5] = 9.2e-41                        # the smallest bf16 subnormal alone: the lower clamp
    lone = torch.zeros(128); lone[100], lone[101], lone[102] = 449.0, 1e-3, -0.0
    rows = [torch.zeros(128), top, big, base * 1e-36, base * 1e-38, base * 3e-39, base * 1e-40, tiny, lone, base * 2.0 ** 60]
    return torch.stack(rows).to(torch.bfloat16)


def _bf16_cache(seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(HKV, CTX, 128, generator=g) * torch.exp(torch.randn(HKV, CTX, 1, generator=g))).to(torch.bfloat16)
    adv = _corner_rows()
    for i in range(len(adv)):      # spread over both heads, the first rows, a tile boundary and the last rows
        x[i % HKV, (0, 1, 14, 62, 63, 64, 65, 129, 190, 191)[i]] = adv[i]
    return x


@pytest.fixture(scope="module")
def caches(dev):
    """One K and one V cache, as bf16 rows and as their FP8 form, with the CPU's dequantization of the latter (quant.py's definition
    is exact arithmetic, and only on the CPU is torch.ldexp trusted to be - DESIGN.md 8d); shared by the tests, never written."""
    from usdm_amd.quant import dequantize_kv_rows, quantize_kv_rows
    k, v = _bf16_cache(1), _bf16_cache(2).flip(0)
    c = dict(k=k, v=v)
    for name, x in (("k", k), ("v", v)):
        q, e = quantize_kv_rows(x)
        assert int(e.max()) == 119 and int(e.min()) == -117 and bool((q == 0x7E).any() or (q == 0xFE).any())      # the corners are met
        c[name + "8"], c[name + "e"], c[name + "d"] = q, e, dequantize_kv_rows(q, e)
    return {n: t.to(dev) for n, t in c.items()}


@pytest.mark.parametrize("ld", [192, 256])
@pytest.mark.parametrize("n", [1, 15, 63, 64, 65, 130, 192])
def test_kv_expand_bf16_cache_is_the_transpose(dev, caches, n, ld):
    from usdm_amd import ops
    kc, vc = caches["k"].clone(), caches["v"].clone()
    buf, vt = _guarded(dev, HKV, 128, ld)
    ops.kv_expand(kc, vc, vt, n=n, Hkv=HKV, ctx_max=CTX, vt_ld=ld)
    torch.cuda.synchronize()
    assert torch.equal(_bits(vt[:, :, :n]), _bits(caches["v"][:, :n].transpose(1, 2)))
    assert _is_sent(vt[:, :, n:]) and _is_sent(buf[:512]) and _is_sent(buf[-512:])      # columns >= n, the heads' padding, the neighbours
    assert torch.equal(_bits(kc), _bits(caches["k"])) and torch.equal(_bits(vc), _bits(caches["v"]))


@pytest.mark.parametrize("ld", [192, 256])
@pytest.mark.parametrize("n", [1, 15, 63, 64, 65, 130, 192])
def test_kv_expand_fp8_cache_is_the_exact_dequantization(dev, caches, n, ld):
    from usdm_amd import ops
    k8, v8, ke, ve = (caches[x].clone() for x in ("k8", "v8", "ke", "ve"))
    vbuf, vt = _guarded(dev, HKV, 128, ld)
    kbuf, kscr = _guarded(dev, HKV, ld, 128)
    ops.kv_expand(k8, v8, vt, n=n, Hkv=HKV, ctx_max=CTX, vt_ld=ld, kv8=(ke, ve), kscr=kscr, kscr_ld=ld)
    torch.cuda.synchronize()
    assert torch.equal(_bits(kscr[:, :n]), _bits(caches["kd"][:, :n]))
    assert torch.equal(_bits(vt[:, :, :n]), _bits(caches["vd"][:, :n].transpose(1, 2)))
    assert _is_sent(vt[:, :, n:]) and _is_sent(vbuf[:512]) and _is_sent(vbuf[-512:])
    assert _is_sent(kscr[:, n:]) and _is_sent(kbuf[:512]) and _is_sent(kbuf[-512:])
    for got, want in ((k8, "k8"), (v8, "v8"), (ke, "ke"), (ve, "ve")):
        assert torch.equal(got, caches[want])


def test_kv_expand_unaligned_destinations_take_the_narrow_stores(dev, caches):
    """vt / kscr only 4-byte aligned, vt_ld no multiple of 8: the same values, the same untouched surroundings"""
    from usdm_amd import ops
    n, ld = 77, 194
    vbuf, vt = _guarded(dev, HKV, 128, ld, guard=514)
    kbuf, kscr = _guarded(dev, HKV, ld, 128, guard=514)
    assert vt.data_ptr() % 16 == 4 and kscr.data_ptr() % 16 == 4
    ops.kv_expand(caches["k8"], caches["v8"], vt, n=n, Hkv=HKV, ctx_max=CTX, vt_ld=ld, kv8=(caches["ke"], caches["ve"]), kscr=kscr, kscr_ld=ld)
    torch.cuda.synchronize()
    assert torch.equal(_bits(kscr[:, :n]), _bits(caches["kd"][:, :n])) and torch.equal(_bits(vt[:, :, :n]), _bits(caches["vd"][:, :n].transpose(1, 2)))
    assert _is_sent(vt[:, :, n:]) and _is_sent(kscr[:, n:])
    assert all(_is_sent(b[:514]) and _is_sent(b[-514:]) for b in (vbuf, kbuf))


def test_kv_expand_refusals(dev, caches):
    """every refusal returns its error without a launch: the sentinel-filled destinations stay as they are"""
    from usdm_amd import _lib, ops
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    vbuf, vt = _guarded(dev, HKV, 128, 192)
    kbuf, kscr = _guarded(dev, HKV, 192, 128)
    k, v, k8, v8, ke, ve = (caches[x] for x in ("k", "v", "k8", "v8", "ke", "ve"))
    base = dict(n=64, Hkv=HKV, ctx_max=CTX, vt_ld=192)
    bf = lambda kc=k, vc=v, t=vt, **kw: ops.kv_expand(kc, vc, t, **dict(base, **kw))
    f8 = lambda kc=k8, vc=v8, t=vt, kx=ke, vx=ve, ks=kscr, **kw: ops.kv_expand(kc, vc, t, kv8=(kx, vx), kscr=ks, **dict(dict(base, kscr_ld=192), **kw))
    for call, kw, what in ((bf, dict(n=0), "n <= ctx_max"), (bf, dict(n=193), "n <= ctx_max"), (bf, dict(n=64, vt_ld=63), "vt_ld"),
                           (f8, dict(n=64, kscr_ld=63), "kscr_ld"), (f8, dict(n=-1), "n <= ctx_max"),
                           (bf, dict(kscr=kscr, kscr_ld=192), "kscr belongs to the fp8 cache"), (f8, dict(ks=None), "kscr"),
                           (bf, dict(vc=z(HKV * CTX * 128 + 8)[4:]), "16-byte"), (f8, dict(kc=z(HKV * CTX * 128 + 16, dt=torch.uint8)[8:]), "16-byte"),
                           (f8, dict(kx=z(HKV * CTX + 4, dt=torch.int8)[1:]), "4-byte"), (f8, dict(vx=z(HKV * CTX + 4, dt=torch.int8)[2:]), "4-byte"),
                           (bf, dict(t=vbuf[513:]), "4-byte"), (f8, dict(ks=kbuf[513:]), "4-byte")):
        with pytest.raises(_lib.UsdmError, match=what):
            call(**kw)
    with pytest.raises(TypeError):
        bf(kc=k8, vc=v8)                                   # byte caches without their exponents
    with pytest.raises(TypeError):
        f8(kc=k, vc=v)
    a = _lib.KvExpandArgs()                                # null pointers, and one exponent array only
    assert _lib.lib.usdm_kv_expand(None, None) == 2
    a.kcache, a.vcache, a.Hkv, a.ctx_max, a.n, a.vt_ld = k.data_ptr(), v.data_ptr(), HKV, CTX, 64, 192
    assert _lib.lib.usdm_kv_expand(_lib.C.byref(a), None) == 2 and b"null" in _lib.lib.usdm_last_error()
    a.kcache, a.vcache, a.vt, a.kexp = k8.data_ptr(), v8.data_ptr(), vt.data_ptr(), ke.data_ptr()
    a.kscr, a.kscr_ld = kscr.data_ptr(), 192
    assert _lib.lib.usdm_kv_expand(_lib.C.byref(a), None) == 2 and b"exponent" in _lib.lib.usdm_last_error()
    torch.cuda.synchronize()
    assert _is_sent(vbuf) and _is_sent(kbuf)
    bf()                                                   # ... and the good calls run
    f8()
    torch.cuda.synchronize()
    assert not _is_sent(vt[:, :, :64]) and not _is_sent(kscr[:, :64])


def _rope_tables(dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2).float() / 128))
    fr = torch.arange(CTX).float()[:, None] * inv[None, :]
    return fr.cos().to(torch.bfloat16).to(dev).contiguous(), fr.sin().to(torch.bfloat16).to(dev).contiguous()


@pytest.mark.parametrize("window", [0, 40])
@pytest.mark.parametrize("fp8", [False, True])
def test_prefill_attention_over_expanded_scratch_equals_the_single_path(dev, caches, fp8, window):
    """usdm_attention mode 1 over (past = 70, S = 9): fed by usdm_kv_expand's scratch + the rope launch's new rows at offset past (a
    batch slot's / an fp8 cache's prefill with a past), and fed by the single sequence's bf16 cache + persistent V^T holding the
    same values (the fp8 cache's: its dequantized rows).  Bit-identical outputs."""
    from usdm_amd import ops
    past, S, Hq, Spad = 70, 9, 4, 128
    nq = (Hq + 2 * HKV) * 128
    g = torch.Generator().manual_seed(11)
    qkv0 = torch.randn(S, nq, generator=g).to(torch.bfloat16).to(dev)
    cos, sin = _rope_tables(dev)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=dev)
    common = dict(mode=1, dh=128, B=1, Hq=Hq, Hkv=HKV, Sq=S, Skv=past + S, q_pos0=past, q_strides=(0, 128, nq), o_strides=(0, Hq * 128),
                  scale=128 ** -0.5, window=window)
    rope = dict(ld=nq, S=S, pos0=past, Hq=Hq, Hkv=HKV, ctx_max=CTX, max_pos=CTX)
    # the single path: a bf16 cache holding the past rows (fp8: as the fp8 cache returns them) and their V^T in the persistent image
    kb, vb = (caches["kd" if fp8 else "k"].clone(), caches["vd" if fp8 else "v"].clone())
    kb[:, past:], vb[:, past:] = 0, 0
    vtc = z(HKV, 128, CTX)
    vtc[:, :, :past] = vb[:, :past].transpose(1, 2)
    qb, ob = qkv0.clone(), z(S, Hq * 128)
    ops.rope_cache(qb, cos, sin, kb, vb, vt=vtc[:, :, past:], vt_ld=CTX, **rope)
    ops.attention(qb, kb, vtc, ob, Skv_alloc=CTX, k_strides=(0, CTX * 128, 128), v_strides=(0, 128 * CTX, CTX), **common)
    # the scratch path
    qa, oa, vt = qkv0.clone(), z(S, Hq * 128), z(HKV, 128, Spad)
    if fp8:
        k8, v8, ke, ve = (caches[x].clone() for x in ("k8", "v8", "ke", "ve"))
        for t in (k8, v8, ke, ve):
            t[:, past:] = 0
        kscr = z(HKV, Spad, 128)
        ops.kv_expand(k8, v8, vt, n=past, Hkv=HKV, ctx_max=CTX, vt_ld=Spad, kv8=(ke, ve), kscr=kscr, kscr_ld=Spad)
        ops.rope_cache(qa, cos, sin, k8, v8, vt=vt[:, :, past:], vt_ld=Spad, kv8=(ke, ve), kscr=kscr[:, past:], kscr_ld=Spad, **rope)
        ops.attention(qa, kscr, vt, oa, Skv_alloc=Spad, k_strides=(0, Spad * 128, 128), v_strides=(0, 128 * Spad, Spad), **common)
    else:
        ka, va = kb.clone(), vb.clone()
        ka[:, past:], va[:, past:] = 0, 0
        ops.kv_expand(ka, va, vt, n=past, Hkv=HKV, ctx_max=CTX, vt_ld=Spad)
        ops.rope_cache(qa, cos, sin, ka, va, vt=vt[:, :, past:], vt_ld=Spad, **rope)
        ops.attention(qa, ka, vt, oa, Skv_alloc=Spad, k_strides=(0, CTX * 128, 128), v_strides=(0, 128 * Spad, Spad), **common)
    torch.cuda.synchronize()
    assert bool(ob.any()) and torch.equal(_bits(oa), _bits(ob)) and torch.equal(_bits(qa), _bits(qb))
    assert torch.equal(_bits(vt[:, :, :past + S]), _bits(vtc[:, :, :past + S])) and not bool(vt[:, :, past + S:].any())
