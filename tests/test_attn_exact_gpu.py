"""GPU: key visibility and softmax weights of every attention kernel, read out exactly (tests/_attn_probe.py: one-hot V probes, an
fp64 CPU reference, every invisible weight == 0.0, every visible weight within TOL = 2^-6 relative).  The test id names the kernel,
the merge path and the cache format; every test prints the (query, key) pairs it checked, the exact-zero checks among them and the
worst |p - p_ref| / (TOL * p_ref)."""
import pytest
import torch

from tests import _attn_probe as P

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------ usdm_attention
def _prefill_weights(dev, mode, c, *, dh, window=0, kv_len=None):
    """the probe launches of one prefill_case -> weights [B, Hq, Sq, Skv] (f32, on the CPU).  Padding keys [Skv, Skv_alloc) hold large
    finite values in K and V^T: a leak shows in every column."""
    from usdm_amd import ops
    q, k = c["q"], c["k"]
    B, Hq, Sq, _ = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    Sa = (Skv + 63) // 64 * 64
    kd = torch.full((B, Hkv, Sa, dh), P.PAD_BIG, dtype=BF, device=dev)
    kd[:, :, Skv:, 1::2] = -P.PAD_BIG
    kd[:, :, :Skv] = k.to(dev)
    qd = q.to(dev).contiguous()
    vt = torch.zeros(B, Hkv, dh, Sa, dtype=BF, device=dev)
    vt[..., Skv:] = P.PAD_BIG
    o = torch.empty(B, Sq, Hq * dh, dtype=BF, device=dev)
    cols = torch.arange(dh, device=dev)
    parts = []
    for j0 in range(0, Skv, dh):
        n = min(dh, Skv - j0)
        vt[:, :, cols[:n], j0 + cols[:n]] = 1.0
        o.fill_(7.0)
        ops.attention(qd, kd, vt, o, mode=mode, dh=dh, B=B, Hq=Hq, Hkv=Hkv, Sq=Sq, Skv=Skv, Skv_alloc=Sa,
                      q_strides=(Hq * Sq * dh, Sq * dh, dh), k_strides=(Hkv * Sa * dh, Sa * dh, dh),
                      v_strides=(Hkv * dh * Sa, dh * Sa, Sa), o_strides=(Sq * Hq * dh, Hq * dh), scale=c["scale"], q_pos0=c["q_pos0"],
                      kv_len=torch.tensor(kv_len, dtype=torch.int32, device=dev) if kv_len is not None else None,
                      slopes=c["slopes"].to(dev) if mode == 0 else None, alibi_col0_zero=c["col0_zero"], window=window)
        w = o.view(B, Sq, Hq, dh).permute(0, 2, 1, 3)
        parts.append(w[..., :n].float())
        if n < dh:      # columns without a probe key see only zeros of V (and nothing of the padding)
            assert not bool(w[..., n:].any()), "probe-less output columns must be exactly 0"
        vt[:, :, cols[:n], j0 + cols[:n]] = 0.0
    return torch.cat(parts, -1).cpu()


_BIDIR_REF = {}


def _bidir_ref(dh, Sq, fam):
    key = (dh, Sq, fam)
    if key not in _BIDIR_REF:
        c = P.prefill_case(0, fam, dh=dh, B=3, Hq=2, Hkv=2, Sq=Sq, Skv=Sq)
        _BIDIR_REF[key] = (c,) + P.prefill_reference(0, c, kv_len=P.bidir_kv_len(Sq))[:2]
    return _BIDIR_REF[key]


@pytest.mark.parametrize("Sq", P.BIDIR_SQ)
@pytest.mark.parametrize("kernel", ["attn16_kernel-dh64", "attn_kernel-dh64-mode0", "attn_kernel-dh128-mode0"])
def test_bidirectional_weights(dev, monkeypatch, kernel, Sq):
    """usdm_attention mode 0 (ALiBi, kv_len = [Sq, Sq - 37, 1]): the 16-query-wave kernel, the 32-query-wave kernel at dh 64
    (USDM_ATTN_V16=0) and at dh 128.  Weights under 2^-24 are only bounded from above (far-tile skipping); none in the uniform family."""
    dh = 128 if "dh128" in kernel else 64
    monkeypatch.setenv("USDM_ATTN_V16", "1" if kernel.startswith("attn16") else "0")
    tot = P.Stats()
    for fam in P.PREFILL_FAMILIES_BIDIR:
        c, ref, vis = _bidir_ref(dh, Sq, fam)
        st = P.check_weights(lambda: _prefill_weights(dev, 0, c, dh=dh, kv_len=P.bidir_kv_len(Sq)), ref, vis, floor=P.FLOOR_BIDIR,
                             tail_ok=True, what=f"{kernel} Sq {Sq} {fam}")
        assert fam != "uniform" or st.tail == 0
        tot.add(st)
    print(tot.line(f"{kernel} Sq {Sq}"))


@pytest.mark.parametrize("cfg", range(len(P.CAUSAL_CONFIGS)), ids=["attn_kernel-dh128-mode1-gqa4", "attn_kernel-dh128-mode1-mha",
                                                                   "attn_kernel-dh64-mode1"])
def test_causal_weights(dev, cfg):
    """usdm_attention mode 1: q_pos0 = 0 and the prefix-reuse form (Skv = q_pos0 + Sq), windows shorter than / equal to / not a
    multiple of the 64-key tile (rows whose first tiles are masked entirely), GQA 4 and 1.  Two-sided bound on every visible weight."""
    dh, B, Hq, Hkv = P.CAUSAL_CONFIGS[cfg]
    tot = P.Stats()
    for q_pos0, Sq, window, fams in P.causal_cases(cfg):
        for fam in fams:
            c = P.prefill_case(1, fam, dh=dh, B=B, Hq=Hq, Hkv=Hkv, Sq=Sq, Skv=q_pos0 + Sq, q_pos0=q_pos0)
            ref, vis, _ = P.prefill_reference(1, c, window=window)
            tot.add(P.check_weights(lambda: _prefill_weights(dev, 1, c, dh=dh, window=window), ref, vis,
                                    what=f"mode 1 dh {dh} Hq/Hkv {Hq}/{Hkv} q_pos0 {q_pos0} Sq {Sq} window {window} {fam}"))
    assert tot.tail == 0
    print(tot.line(f"attn_kernel<{dh}, 1> Hq/Hkv {Hq}/{Hkv}"))


# ------------------------------------------------------------------------------------------------------------------ usdm_attn_decode
class _DecodeRig:
    """device buffers of one (Hq, Hkv, NS, batch) decode configuration, reused over the probe launches"""

    def __init__(self, dev, Hq, Hkv, NS, batch, fp8, merge):
        self.dev, self.Hq, self.Hkv, self.NS, self.B, self.fp8, self.merge = dev, Hq, Hkv, NS, max(1, batch), fp8, merge
        self.batch = batch
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        n = self.B * Hq * max(NS, 1)
        self.pm, self.pl, self.po = z(n), z(n), z(n * 128)
        self.cnt = z(self.B * Hkv, dt=torch.int32) if merge == "counters" else None
        self.cos, self.sin = (t.to(dev) for t in P.rope_tables64(P.DECODE_CTX_MAX))
        self.eye = torch.eye(Hq * 128, dtype=BF, device=dev) if merge == "gemv" else None

    def launch(self, qkv, pos_t, kc, vc, exps, window, skip=None):
        """one usdm_attn_decode(_fp8) launch (+ the merging GEMV); returns out [B, Hq*128] bf16"""
        from usdm_amd import ops
        Hq, Hkv, cm = self.Hq, self.Hkv, P.DECODE_CTX_MAX
        out = torch.full((self.B, Hq * 128), 7.0, dtype=BF, device=self.dev)
        nq = (Hq + 2 * Hkv) * 128
        ops.attn_decode(qkv, pos_t, self.cos, self.sin, kc, vc, self.pm, self.pl, self.po, None if self.merge == "gemv" else out,
                        Hq=Hq, Hkv=Hkv, ctx_max=cm, NS=self.NS, scale=0.5, counters=self.cnt, batch=self.batch, qkv_bs=nq,
                        out_bs=Hq * 128, cache_bs=Hkv * cm * 128, skip=skip, defer_merge=self.merge == "gemv", window=window,
                        kv8=exps, exp_bs=Hkv * cm)
        if self.merge == "gemv":    # identity weights: the GEMV returns the merged, bf16-rounded attention output (x is ignored)
            ops.gemv(self.eye, out[0].clone(), N=Hq * 128, K=Hq * 128, y16=out[0], merge=(self.pm, self.pl, self.po, self.NS))
        if self.cnt is not None:
            assert not bool(self.cnt.any()), "the merge counters must be left zero"
        return out


_PROBE_V = {}


def _probe_v(dev, fp8, j0):
    """the one-hot V cache [2, ctx_max, 128] whose rows j0 .. j0+127 carry the probes (fp8: its bytes and exponents), on the device"""
    from usdm_amd.quant import quantize_kv_rows
    if (fp8, j0) not in _PROBE_V:
        v = torch.zeros(2, P.DECODE_CTX_MAX, 128)
        cols = torch.arange(128)
        v[:, j0 + cols, cols] = 1.0
        v = v.to(BF)
        _PROBE_V[(fp8, j0)] = tuple(t.to(dev) for t in quantize_kv_rows(v)) if fp8 else (v.to(dev),)
    return _PROBE_V[(fp8, j0)]


def _decode_weights(rig, cases, window, check_side_effects=True):
    """the probe launches of len(cases) sequences (decode_case dicts, one per batch item) -> weights [B, Hq, ctx_max] f32 on the CPU,
    plus the (dequantized) cached keys the kernel read.  The cache rows at pos hold large values before the launch (the new token's
    own row must come from LDS, not from the cache); after it they must equal the roped k / the probe v, all other rows untouched."""
    from usdm_amd.quant import dequantize_kv_rows, quantize_kv_rows
    dev, Hq, Hkv, B, cm = rig.dev, rig.Hq, rig.Hkv, rig.B, P.DECODE_CTX_MAX
    assert len(cases) == B and Hkv == 2
    pos = [c["pos"] for c in cases]
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    kc = torch.stack([c["kc"] for c in cases])                         # [B, Hkv, cm, 128] bf16
    for b in range(B):
        kc[b, :, pos[b]] = P.PAD_BIG
    kread = kc
    if rig.fp8:
        k8, ke = quantize_kv_rows(kc)
        kread = dequantize_kv_rows(k8, ke)
        kbase = (k8.to(dev), ke.to(dev))
        pad8, pade = (t.to(dev) for t in quantize_kv_rows(torch.full((128,), P.PAD_BIG, dtype=BF)))
    else:
        kbase = (kc.to(dev),)
    qkv = torch.stack([c["qkv"] for c in cases]).clone()               # [B, nq], v = 0
    krs = [P.rope_rows(c["qkv"].view(-1, 128)[Hq:Hq + Hkv], c["pos"], cm) for c in cases]
    others = torch.ones(B, 1, cm, 1, dtype=torch.bool, device=dev)     # every cache row but the sequences' own
    for b in range(B):
        others[b, 0, pos[b]] = False
    parts = []
    for j0 in range(0, cm, 128):
        vnew = torch.zeros(B, Hkv, 128)
        for b in range(B):
            if j0 <= pos[b] < j0 + 128:
                vnew[b, :, pos[b] - j0] = 1.0
        qkv.view(B, Hq + 2 * Hkv, 128)[:, Hq + Hkv:] = vnew.to(BF)
        vbase = tuple(t[None].expand(B, *t.shape).clone() for t in _probe_v(dev, rig.fp8, j0))
        for b in range(B):
            if rig.fp8:
                vbase[0][b, :, pos[b]], vbase[1][b, :, pos[b]] = pad8, pade
            else:
                vbase[0][b, :, pos[b]] = P.PAD_BIG
        kcl, vcl = tuple(t.clone() for t in kbase), tuple(t.clone() for t in vbase)
        out = rig.launch(qkv.to(dev), pos_t, kcl[0], vcl[0], (kcl[1], vcl[1]) if rig.fp8 else None, window)
        parts.append(out.view(B, Hq, 128).float().cpu())
        if check_side_effects and j0 == 0:
            for after, before in zip(kcl + vcl, kbase + vbase):
                m = others if after.dim() == 4 else others[..., 0]
                assert torch.equal(after * m, before * m), "a cache row other than the new token's was written"
            for b in range(B):
                p = pos[b]
                for got, row in ((kcl, krs[b]), (vcl, vnew[b].to(BF))):
                    if rig.fp8:
                        q_, e_ = quantize_kv_rows(row)
                        assert torch.equal(got[0][b, :, p].cpu(), q_) and torch.equal(got[1][b, :, p].cpu(), e_), f"sequence {b}: appended fp8 row"
                    else:
                        assert torch.equal(got[0][b, :, p].cpu(), row), f"sequence {b}: appended row"
    return torch.cat(parts, -1), kread


def _run_decode_cases(dev, fp8, merge, ns_list, offset, what):
    tot = P.Stats()
    rigs = {}
    for pos, NS, window, G, fams in P.decode_cases(ns_list, offset):
        rig = rigs.setdefault((G, NS), _DecodeRig(dev, 2 * G, 2, NS, 0, fp8, merge))
        for fam in fams:
            c = P.decode_case(fam, Hq=2 * G, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=pos, NS=NS, window=window)
            got, kread = _decode_weights(rig, [c], window, check_side_effects=fam == "uniform")
            ref, vis, _, _ = P.decode_reference(c, window=window, k_cached=kread[0])
            tot.add(P.check_weights(lambda: got[0], ref, vis, what=f"{what} pos {pos} NS {NS} window {window} G {G} {fam}"))
    assert tot.tail == 0
    print(tot.line(what))


@pytest.mark.parametrize("merge", ["combine", "counters", "gemv"])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
def test_decode_split_weights(dev, cache, merge):
    """attn_decode_kernel<G, false, FP8> with NS in {2, 3, 8}: every pos x NS, every (window, pos) x NS, G in {1, 2, 4}; merged by
    attn_combine_kernel, by the last-arriving workgroup (counters) or by usdm_gemv's merge prologue (defer_merge)."""
    _run_decode_cases(dev, cache == "fp8", merge, P.DECODE_NS, ["combine", "counters", "gemv"].index(merge),
                      f"attn_decode_kernel {cache} cache, merge by {merge}")


def test_decode1_weights(dev):
    """attn_decode1_kernel<G> (NS = 1, one workgroup per kv head, bf16 cache), every pos, G in {1, 2, 4}"""
    for off in (0, 1, 2):       # every pos with every G
        _run_decode_cases(dev, False, "none", (1,), off, "attn_decode1_kernel (NS = 1)")


@pytest.mark.parametrize("cache", ["bf16", "fp8"])
def test_decode_refuses_window_without_splits(dev, cache):
    from usdm_amd import _lib
    rig = _DecodeRig(dev, 4, 2, 1, 0, cache == "fp8", "none")
    c = P.decode_case("uniform", Hq=4, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=300, NS=1, window=100)
    with pytest.raises(_lib.UsdmError):
        _decode_weights(rig, [c], 100)


BATCH_POS = (0, P.DECODE_CTX_MAX - 1, 699, 31, 32, 63, 64, 255, 256, 1, 100, 299, 300, 301, 511, 512)


@pytest.mark.parametrize("merge", ["combine", "counters"])
@pytest.mark.parametrize("batch,NS,window", [(3, 8, 0), (3, 16, 0), (16, 3, 300), (16, 2, 100), (16, 8, 0)],
                         ids=["b3-ns8-PIPE", "b3-ns16-plain", "b16-ns3-w300-PIPE", "b16-ns2-w100-plain", "b16-ns8-PIPE"])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
def test_decode_batched_weights(dev, cache, batch, NS, window, merge):
    """the batched launch: a different pos per sequence (0 and ctx_max - 1 among them); ceil(span / NS) > 64 selects the pipelined
    instantiation attn_decode_kernel<G, true, FP8>, <= 64 the plain one."""
    G = 4 if batch == 16 else 2
    rig = _DecodeRig(dev, 2 * G, 2, NS, batch, cache == "fp8", merge)
    tot = P.Stats()
    for rnd in range(2):
        fams = [P.DECODE_FAMILIES[(b + 2 * rnd + (0 if rnd == 0 else 1)) % 5] if rnd else "uniform" for b in range(batch)]
        cases = [P.decode_case(fams[b], Hq=2 * G, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=BATCH_POS[b], NS=NS, window=window, seed=b)
                 for b in range(batch)]
        got, kread = _decode_weights(rig, cases, window, check_side_effects=rnd == 0)
        for b, c in enumerate(cases):
            ref, vis, _, _ = P.decode_reference(c, window=window, k_cached=kread[b])
            tot.add(P.check_weights(lambda: got[b], ref, vis, what=f"batch {batch} sequence {b} pos {c['pos']} NS {NS} window {window} {fams[b]}"))
    assert tot.tail == 0
    pipe = "true" if -(-(window or P.DECODE_CTX_MAX) // NS) > 64 else "false"
    print(tot.line(f"attn_decode_kernel<{G}, {pipe}> {cache} cache, batch {batch}, merge by {merge}"))


@pytest.mark.parametrize("merge", ["combine", "counters"])
@pytest.mark.parametrize("cache", ["bf16", "fp8"])
def test_decode_skip_touches_nothing(dev, cache, merge):
    """*skip != 0: the sequence has ended - no cache row is appended and `out` keeps its contents"""
    from usdm_amd.quant import quantize_kv_rows
    fp8 = cache == "fp8"
    rig = _DecodeRig(dev, 8, 2, 8, 0, fp8, merge)
    c = P.decode_case("ramp_up", Hq=8, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=300, NS=8, window=0)
    kc, vc = c["kc"].clone(), torch.ones(2, P.DECODE_CTX_MAX, 128, dtype=BF)
    if fp8:
        (k8, ke), (v8, ve) = quantize_kv_rows(kc), quantize_kv_rows(vc)
        bufs = [k8.to(dev), v8.to(dev), ke.to(dev), ve.to(dev)]
    else:
        bufs = [kc.to(dev), vc.to(dev)]
    before = [t.clone() for t in bufs]
    out = rig.launch(c["qkv"].to(dev)[None], torch.tensor([300], dtype=torch.int32, device=dev), bufs[0], bufs[1],
                     (bufs[2], bufs[3]) if fp8 else None, 0, skip=torch.ones(1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "out was written"
    for a, b in zip(bufs, before):
        assert torch.equal(a, b), "a cache was written"


# ------------------------------------------------------------------------------------------------------------------ usdm_softmax_alibi
def _softmax_alibi_inputs():
    B, rpb, H, n, npad, ldseg = 3, 70, 3, 150, 160, 200
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * rpb, H, ldseg, generator=g) * 3.0
    x[:, :, 7] += 12.0                                                       # one dominant key and a far tail
    kv_len = [n, 97, 1]
    return B, rpb, H, n, npad, ldseg, x, kv_len, P.alibi_slopes(H)


def _softmax_alibi_ref(x, col0, dtype):
    """softmax_j(x - slope * |i - j|) over j < kv_len[b] in `dtype` (fp64: the reference; fp32: torch's own, to size the bound)"""
    B, rpb, H, n, npad, ldseg, _, kv_len, slopes = _softmax_alibi_inputs()
    i = torch.arange(rpb).repeat(B).view(-1, 1, 1)
    j = torch.arange(n).view(1, 1, -1)
    bias = -slopes.to(dtype).view(1, H, 1) * (i - j).abs().to(dtype)
    if col0:
        bias[..., 0] = 0
    s = x[..., :n].to(dtype) + bias
    vis = (j < torch.tensor(kv_len).repeat_interleave(rpb).view(-1, 1, 1)).expand_as(s)
    return torch.softmax(s.masked_fill(~vis, -float("inf")), -1), vis


SOFTMAX_ALIBI_TORCH_FP32_ERR = 1.0e-5     # measured on the CPU: 9.73e-6 / 9.59e-6 (col0_zero on / off); recomputed and asserted by the test itself


@pytest.mark.parametrize("col0", [True, False], ids=["col0_zero", "col0_biased"])
def test_softmax_alibi_weights(dev, col0):
    """softmax_alibi_kernel (the exact-f32 Voicebox plan), in place on f32 scores: n = 150 (not a multiple of 64), npad = 160 (pad
    columns exactly 0), ldseg = 200 (neighbours beyond npad untouched), kv_len = [150, 97, 1], 3 heads.  Every weight against fp64.
    Bound: torch's own fp32 softmax of the same biased scores differs from fp64 by 9.73e-6 relative at worst on these inputs (weights
    >= 2^-100; scores reach |x + bias| ~ 120, where one f32 ulp is 7.6e-6; measured on the CPU, recomputed below, recorded as 1.0e-5);
    the kernel may take 4x that = 4e-5 (a 64-lane tree sum and expf differ from
    torch's order by a few ulp)."""
    from usdm_amd import ops
    B, rpb, H, n, npad, ldseg, x, kv_len, slopes = _softmax_alibi_inputs()
    ref, vis = _softmax_alibi_ref(x, col0, torch.float64)
    t32, _ = _softmax_alibi_ref(x, col0, torch.float32)
    big = vis & (ref >= P.FLOOR_EXACT)
    torch_err = float(((t32.double() - ref).abs() / ref.clamp_min(1e-300))[big].max())
    print(f"[attn-probe] torch fp32 softmax vs fp64 on these inputs: {torch_err:.3g} relative")
    assert torch_err <= SOFTMAX_ALIBI_TORCH_FP32_ERR, "the recorded fp32 figure no longer describes the inputs"
    tol = 4 * SOFTMAX_ALIBI_TORCH_FP32_ERR
    xd = x.to(dev).contiguous()
    ops.softmax_alibi(xd, rows=B * rpb, rows_per_batch=rpb, nheads=H, n=n, npad=npad, ldrow=H * ldseg, ldseg=ldseg, slopes=slopes.to(dev),
                      kv_len=torch.tensor(kv_len, dtype=torch.int32, device=dev), col0_zero=col0)
    got = xd.cpu()
    assert torch.equal(got[..., npad:], x[..., npad:]), "columns beyond npad inside ldseg were touched"
    assert not bool(got[..., n:npad].any()), "pad columns must be exactly 0"
    st = P.check_weights(lambda: got[..., :n], ref, vis, tol=tol, floor=P.FLOOR_EXACT, tail_ok=True, what=f"softmax_alibi col0_zero={col0}")
    print(st.line(f"softmax_alibi_kernel col0_zero={col0} (tol {tol:.2g})"))
