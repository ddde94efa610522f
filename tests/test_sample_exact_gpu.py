"""The sampling head (usdm_sample_final / usdm_sample_final_seg) against tests/_sample_reference.py, the kernel's arithmetic restated
in Python integers, on rows built so that every decision is decidable although the kernel's fast exp and numpy's differ by a few ulp
(tests/test_sample_reference_cpu.py proves every row's stated property on the CPU):

  exact rows: every logit is one value or -inf, so every mass is 2^32 or 0 under any exp.  probs_out and every token bit for bit, at
              the vocabulary sizes where the draw's thread ranges change shape, with (seed, step) pairs chosen so that the targets
              fall on the first and the last kept id and on both sides of every thread-range boundary that has kept ids next to it;
  level rows: a handful of tied levels.  Equal logits have equal masses under any exp, so tie decisions are exact, and every other
              threshold has a relative margin of 1e-3 in mass: kept sets identical, probabilities to rtol 3e-6 (the tolerance
              test_sampling_gpu.py uses for the same f32 exp difference), tokens equal for pairs with a slack of 1e-4;
  the batched, the segmented and the device-parameter forms, every row against the reference.

Measured on the MI355X: the largest relative difference of probs_out against the reference over all level rows is 4.5e-7 (the T=0.05
row, whose lowest kept level sits 7.5 below the maximum; 1.5e-7 on every other row), against the bound of 3e-6.

Before -0.0 was made equal to +0.0 in the sampler (csrc/sample_k.hip), the two signed-zero rows failed here: the kernel dropped the
four -0.0 ids of the zero block at the k-th rank, which HF and the reference keep.
"""
import numpy as np
import pytest
import torch

from tests import _sample_reference as R

pytestmark = pytest.mark.gpu

RTOL = 3e-6
OFF, HD, MAX_OUT = 1000, 64, 64
JUNK = 1.0e4                    # what every slot holds that no row owns: it would take all the mass if it were read


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _draws(dev, logits, pairs, probs=None, **knobs):
    """one launch per (seed, step) pair on the same row, every pair with state words of its own, one synchronisation at the end
    -> tokens; probs_out is written by the first launch"""
    from usdm_amd import ops
    n = len(pairs)
    steps = torch.tensor([t for _, t, *_ in pairs], dtype=torch.int32)
    nxt, out, pos = (torch.full((n,), v, dtype=torch.int32, device=dev) for v in (-3, -5, 7))
    stp = steps.to(dev)
    for i, (seed, *_) in enumerate(pairs):
        st = ops.decode_state(nxt[i:i + 1], out[i:i + 1], stp[i:i + 1], pos[i:i + 1])
        ops.sample_final(logits, st, seed=seed, probs_out=probs if i == 0 else None, **knobs)
    torch.cuda.synchronize()
    nxt, out, stp, pos = nxt.cpu(), out.cpu(), stp.cpu(), pos.cpu()
    ok = steps < 2 ** 31 - 1
    assert torch.equal(stp[ok], steps[ok] + 1) and (pos == 8).all()
    assert torch.equal(out, torch.where(steps == 0, nxt, torch.full_like(nxt, -5)))      # max_out = 1: only step 0 has an output row
    return nxt.tolist()


# ------------------------------------------------------------------------------------------------------------------- exact rows
@pytest.mark.parametrize("V", R.EXACT_V + (R.BIG_V,))
def test_exact_rows(dev, V):
    for name, kept in R.exact_patterns(V):
        F, pairs = R.exact_pairs(V, kept)
        assert len(pairs) >= 64
        probs = torch.full((V,), -1.0, device=dev)
        toks = _draws(dev, torch.from_numpy(R.exact_row(V, kept)).to(dev), pairs, probs)
        want = np.zeros(V, np.float32)
        want[kept] = np.float32(1.0 / kept.size)
        assert np.array_equal(_bits(probs.cpu().numpy()), _bits(want)), name
        bad = [(s, t, w, g) for (s, t, w), g in zip(pairs, toks) if g != w]
        assert not bad, (name, len(bad), bad[:4])


# ------------------------------------------------------------------------------------------------------------------- level rows
def _check_probs(got, F, what):
    """kept set identical, probabilities within RTOL -> the largest relative difference"""
    want = R.probs(F)
    got = got.astype(np.float64)
    assert np.array_equal(got > 0, want > 0), f"{what}: kept set differs: {np.flatnonzero((got > 0) != (want > 0))[:8]}"
    on = want > 0
    rel = float(np.abs(got[on] / want[on] - 1).max())
    print(f"probs_out max rel diff {rel:.3e}  [{what}]")
    assert rel <= RTOL, (what, rel)
    return rel


@pytest.mark.parametrize("i", range(len(R.LEVEL_CASES)), ids=[c["name"] for c in R.LEVEL_CASES])
def test_level_rows(dev, i):
    c, row, F, pairs = R.level_case(i)
    probs = torch.full((R.LV,), -1.0, device=dev)
    toks = _draws(dev, torch.tensor(row).to(dev), pairs, probs, temperature=c["T"], top_k=c["k"], top_p=c["p"], min_p=c["min_p"])
    got = probs.cpu().numpy()
    _check_probs(got, F, c["name"])
    assert np.array_equal(got > 0, R.keep_mask(c, row))
    if c.get("lowest"):           # k = 1 keeps the whole tie block (HF keeps ties): uniform over it, and the lowest id is taken
        assert set(_bits(got[got > 0]).tolist()) == set(_bits(np.float32(1.0 / 3)).tolist())
    assert toks == [w for _, _, w in pairs]


# ------------------------------------------------------------------------------------------- batched, segmented, device parameters
BATCH_CASES = (13, 17, 0, 3, 5, 9, 10, 12, 15, 16, 20, 22, 24, 25, 26, 27)      # indices into LEVEL_CASES, one per sequence


def _batch(dev, B, done, nseg=1):
    """sequence b = level row BATCH_CASES[b] with its own knobs, seed and step, in one launch; rows with done[b] != 0 must be left alone.
    nseg = 1: logits [B][V + 5]; nseg > 1: [nseg][B][seg_len] with seg_len not dividing V.  Junk wherever no row owns a slot."""
    from usdm_amd import ops
    V = R.LV
    cases = [R.level_case(i) for i in BATCH_CASES[:B]]
    picks = [ps[0] if b % 4 == 3 else ps[-1 - b % 3] for b, (_, _, _, ps) in enumerate(cases)]      # (step 0 or 2^31 - 1, else a small step)
    if nseg == 1:
        host = torch.full((B, V + 5), JUNK)
        for b, (_, row, _, _) in enumerate(cases):
            host[b, :V] = torch.tensor(row)
        seg = dict(V=V)
    else:
        sl = -(-V // nseg)
        assert V % sl and nseg * sl >= V
        host = torch.full((nseg, B, sl), JUNK)
        for b, (_, row, _, _) in enumerate(cases):
            for s in range(nseg):
                part = torch.tensor(row[s * sl:(s + 1) * sl])
                host[s, b, :part.numel()] = part
        seg = dict(V=V, nseg=nseg, seg_stride=B * sl, seg_len=sl)
    logits = host.to(dev)
    sp = ops.sample_params_tensor(dev, B).view(B, -1)
    for b, ((c, _, _, _), (seed, _, _)) in enumerate(zip(cases, picks)):
        ops.set_sample_params(sp[b], c["T"], c["k"], c["p"], seed, c["min_p"])
    E = torch.randn(V + OFF, HD, generator=torch.Generator().manual_seed(B)).to(torch.bfloat16).to(dev)
    steps = [t for _, t, _ in picks]
    nxt0 = torch.arange(-7, -7 - B, -1, dtype=torch.int32)
    out0 = -(100 + torch.arange(B * MAX_OUT, dtype=torch.int32)).view(B, MAX_OUT)
    stp0, pos0 = torch.tensor(steps, dtype=torch.int32), 40 + torch.arange(B, dtype=torch.int32)
    nxt, out, stp, pos = nxt0.to(dev), out0.to(dev), stp0.to(dev), pos0.to(dev)
    dn = torch.tensor(done, dtype=torch.int32, device=dev)
    h = torch.full((B, HD), 768.0, dtype=torch.bfloat16, device=dev)
    probs = torch.full((B, V), -1.0, device=dev)
    if B == 1:
        st = ops.decode_state(nxt, out[0], stp, pos, id_offset=OFF, done=dn)
        ops.sample_final(logits, st, dev_params=sp[0], probs_out=probs, embed=E, h_out=h, Hd=HD, **seg)
    else:
        st = ops.decode_state(nxt, out, stp, pos, id_offset=OFF, batch=B, done=dn)
        ops.sample_final(logits, st, dev_params=sp, probs_out=probs, embed=E, h_out=h, Hd=HD, **seg)
    torch.cuda.synchronize()
    nxt, out, stp, pos, h, probs, E = (t.cpu() for t in (nxt, out, stp, pos, h, probs, E))
    assert dn.cpu().tolist() == list(done)
    for b, ((c, row, F, _), (seed, step, tok)) in enumerate(zip(cases, picks)):
        what = f"B={B} nseg={nseg} b={b}: {c['name']}"
        if done[b]:
            assert int(nxt[b]) == int(nxt0[b]) and torch.equal(out[b], out0[b]) and int(stp[b]) == step and int(pos[b]) == int(pos0[b]), what
            assert (h[b] == 768.0).all() and (probs[b] == -1.0).all(), what
            continue
        _check_probs(probs[b].numpy(), F, what)
        assert int(nxt[b]) == tok + OFF, (what, int(nxt[b]) - OFF, tok)
        want_out = out0[b].clone()
        if step < MAX_OUT:
            want_out[step] = tok + OFF
        assert torch.equal(out[b], want_out), what
        assert int(pos[b]) == int(pos0[b]) + 1 and (step == 2 ** 31 - 1 or int(stp[b]) == step + 1), what
        assert torch.equal(h[b], E[tok + OFF]), what
    assert any(t < MAX_OUT for t in steps) and (B == 1 or len(set(steps)) > 1)


@pytest.mark.parametrize("B,done", [(2, (0, 1)), (2, (1, 0)), (16, (0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0))])
def test_batched_contiguous_form(dev, B, done):
    _batch(dev, B, done)


@pytest.mark.parametrize("nseg", [2, 8])
@pytest.mark.parametrize("B", [1, 6])
def test_segmented_form(dev, nseg, B):
    _batch(dev, B, (0,) * B, nseg=nseg)


NAN = float("nan")


@pytest.mark.parametrize("raw", [(0.0, 6, 0.5), (-2.0, 6, 0.5), (NAN, 6, 0.5), (0.7, 6, 0.0), (0.7, 6, 1.5), (0.7, 6, NAN), (0.7, -3, 0.4)],
                         ids=lambda r: "T=%g k=%d p=%g" % r)
def test_dev_params_sanitising(dev, raw):
    """a device block holding an out-of-range knob gives, bit for bit, what the sanitised values give as host arguments, and that is
    what the reference gives"""
    from usdm_amd import ops
    _, row, _, _ = R.level_case(16)
    T, k, p, _ = R.sanitize(*raw)
    F = R.filter_ref(row, T, k, p)
    assert R.margin(F) >= R.MARGIN
    pairs = R.pairs_for(F, [], n_min=4, slack=R.SLACK)
    logits = torch.tensor(row).to(dev)
    sp = ops.sample_params_tensor(dev)
    res = []
    for form in ("dev", "host"):
        probs = torch.full((R.LV,), -1.0, device=dev)
        toks = []
        for seed, step, _ in pairs:
            nxt, out, stp, pos = (torch.full((n,), v, dtype=torch.int32, device=dev) for n, v in ((1, -3), (MAX_OUT, -5), (1, step), (1, 7)))
            st = ops.decode_state(nxt, out, stp, pos)
            if form == "dev":
                ops.set_sample_params(sp, raw[0], raw[1], raw[2], seed)
                ops.sample_final(logits, st, dev_params=sp, probs_out=probs)
            else:
                ops.sample_final(logits, st, temperature=T, top_k=k, top_p=p, seed=seed, probs_out=probs)
            torch.cuda.synchronize()
            toks.append(int(nxt.item()))
        res.append((toks, probs.cpu().numpy()))
    assert res[0][0] == res[1][0] == [w for _, _, w in pairs]
    assert np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
    _check_probs(res[0][1], F, "dev_params %r" % (raw,))
