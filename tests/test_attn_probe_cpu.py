"""CPU: the probe method of tests/_attn_probe.py can fail.  (a) An fp64 attention with exactly the two bf16 roundings of a correct
flash-attention kernel (P before P.V, the output) passes the checker on every case list of tests/test_attn_exact_gpu.py with room to
spare - the worst |p - p_ref| / (TOL * p_ref) is printed and must stay under 0.5, i.e. the roundings alone need less than 2^-7 and
TOL = 2^-6 leaves the factor 2 its derivation promises; and no visible weight of a causal / decode case lies under 2^-100.
(b) Deliberately wrong emulations - one mask bit at a tile edge, a key counted twice or not at all, an ALiBi distance off by one, a
missing key-0 exception, a window edge off by one - are every one rejected.  This is the only place a wrong mask is built."""
import pytest
import torch

from tests import _attn_probe as P


def _emul_check(sc, vis, ref, **kw):
    return P.check_weights(lambda: P.emulate_weights(sc, vis), ref, vis, **kw)


def test_emulated_kernel_passes_bidirectional_cases():
    tot = P.Stats()
    for Sq in P.BIDIR_SQ:
        for fam in P.PREFILL_FAMILIES_BIDIR:
            c = P.prefill_case(0, fam, dh=64, B=3, Hq=2, Hkv=2, Sq=Sq, Skv=Sq)
            ref, vis, sc = P.prefill_reference(0, c, kv_len=P.bidir_kv_len(Sq))
            st = _emul_check(sc, vis, ref, floor=P.FLOOR_BIDIR, tail_ok=True, what=f"mode 0 Sq {Sq} {fam}")
            assert fam != "uniform" or st.tail == 0
            tot.add(st)
    print(P.Stats.line(tot, "emulation, bidirectional"))
    assert tot.worst < 0.5 and tot.zeros > 0


def test_emulated_kernel_passes_causal_cases():
    tot = P.Stats()
    for ci, (dh, B, Hq, Hkv) in enumerate(P.CAUSAL_CONFIGS):
        for q_pos0, Sq, window, fams in P.causal_cases(ci):
            for fam in fams:
                c = P.prefill_case(1, fam, dh=dh, B=B, Hq=Hq, Hkv=Hkv, Sq=Sq, Skv=q_pos0 + Sq, q_pos0=q_pos0)
                ref, vis, sc = P.prefill_reference(1, c, window=window)
                assert P.min_visible(ref, vis) >= P.FLOOR_EXACT
                tot.add(_emul_check(sc, vis, ref, what=f"mode 1 dh {dh} q_pos0 {q_pos0} Sq {Sq} window {window} {fam}"))
    print(P.Stats.line(tot, "emulation, causal"))
    assert tot.worst < 0.5 and tot.tail == 0 and tot.zeros > 0


def test_emulated_kernel_passes_decode_cases():
    tot = P.Stats()
    for ns_list in ((1,), P.DECODE_NS):
        for pos, NS, window, G, fams in P.decode_cases(ns_list):
            for fam in fams:
                c = P.decode_case(fam, Hq=2 * G, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=pos, NS=NS, window=window)
                ref, vis, sc, _ = P.decode_reference(c, window=window)
                assert P.min_visible(ref, vis) >= P.FLOOR_EXACT
                tot.add(_emul_check(sc, vis, ref, what=f"decode pos {pos} NS {NS} window {window} {fam}"))
    print(P.Stats.line(tot, "emulation, decode"))
    assert tot.worst < 0.5 and tot.tail == 0 and tot.zeros > 0


# ------------------------------------------------------------------------------------------------------------------ mutations
def _causal(fam, window=0, Sq=577):
    c = P.prefill_case(1, fam, dh=128, B=1, Hq=4, Hkv=1, Sq=Sq, Skv=Sq)
    return P.prefill_reference(1, c, window=window)


def _rejected(sc_bad, vis_bad, ref, vis, mult=None, **kw):
    with pytest.raises(AssertionError):
        P.check_weights(lambda: P.emulate_weights(sc_bad, vis_bad, mult), ref, vis, **kw)


@pytest.mark.parametrize("fam", ["uniform", "ramp_up", "ramp_down"])
def test_wrong_masks_are_rejected_causal(fam):
    ref, vis, sc = _causal(fam)
    i = torch.arange(577).view(-1, 1)
    j = torch.arange(577).view(1, -1)
    _emul_check(sc, vis, ref)                                            # the unmutated emulation passes
    _rejected(sc, vis & ~((j == 64) & (i >= 128)), ref, vis)             # key 64 (first key of tile 1) hidden from rows >= 128
    _rejected(sc, vis | ((j == i + 1) & (i >= 64)), ref, vis)            # rows >= 64 also see key i + 1
    _rejected(sc, vis | ((j == i + 1) & (i >= 128)), ref, vis)           # ... rows of the second workgroup only
    _rejected(sc, vis | ((j == i + 1) & (i == 576 - 1)), ref, vis)       # ... one row only
    for w in (64, 100):
        ref, vis, sc = _causal(fam, window=w, Sq=300)
        _emul_check(sc, vis, ref)
        _rejected(sc, P.visibility(1, 1, 300, 300, 0, w + 1).expand_as(sc), ref, vis)     # far edge: one key too many
        _rejected(sc, P.visibility(1, 1, 300, 300, 0, w - 1).expand_as(sc), ref, vis)     # ... one too few


@pytest.mark.parametrize("fam", ["uniform", "ramp_up", "ramp_down", "spike_split_first"])
def test_wrong_splits_are_rejected_decode(fam):
    pos, NS = 699, 8
    c = P.decode_case(fam, Hq=4, Hkv=2, ctx_max=P.DECODE_CTX_MAX, pos=pos, NS=NS, window=0)
    ref, vis, sc, _ = P.decode_reference(c)
    _emul_check(sc, vis, ref)
    _, sp = P.decode_splits(pos, NS, 0)
    for k0, k1 in (sp[0], sp[3], sp[NS - 1]):
        for key, times in ((k1 - 1, 2.0), (k1 - 1, 0.0), (k0, 2.0)):       # a key counted in two splits; a split that drops its last key
            mult = torch.ones(P.DECODE_CTX_MAX, dtype=torch.float64)
            mult[key] = times
            _rejected(sc, vis, ref, vis, mult)
    vis_bad = vis.clone(); vis_bad[:, pos + 1] = True                     # a cache row beyond pos
    _rejected(sc, vis_bad, ref, vis)


@pytest.mark.parametrize("Sq", [65, 300])
def test_wrong_alibi_is_rejected(Sq):
    kw = dict(floor=P.FLOOR_BIDIR, tail_ok=True)
    kv_len = P.bidir_kv_len(Sq)
    c = P.prefill_case(0, "alibi", dh=64, B=3, Hq=2, Hkv=2, Sq=Sq, Skv=Sq)
    ref, vis, sc = P.prefill_reference(0, c, kv_len=kv_len)
    _emul_check(sc, vis, ref, **kw)
    for off in (1, -1):                                                   # ALiBi distance off by one
        _rejected(P.scores_fp64(c["q"], c["k"], c["scale"], c["slopes"], 0, True, dist_off=off), vis, ref, vis, **kw)
    _rejected(P.scores_fp64(c["q"], c["k"], c["scale"], c["slopes"], 0, False), vis, ref, vis, **kw)     # key-0 exception missing
    c2 = P.prefill_case(0, "alibi_nocol0", dh=64, B=3, Hq=2, Hkv=2, Sq=Sq, Skv=Sq)
    ref2, vis2, sc2 = P.prefill_reference(0, c2, kv_len=kv_len)
    _rejected(sc, vis, ref2, vis2, **kw)                                  # ... applied where it is switched off
    bad = P.visibility(0, 3, Sq, Sq, kv_len=[Sq, max(1, Sq - 36), 1]).expand_as(sc)       # kv_len off by one in the second batch item
    _rejected(sc, bad, ref, vis, **kw)
