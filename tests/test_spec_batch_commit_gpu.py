"""usdm_spec_commit_batch through the C-ABI against tests/_spec_reference.py's numpy restatement applied slot by slot
(tests/_spec_batch_reference.py): every word of every buffer ==, over hand-built multi-slot states and 200 seeded random ones
(B in 2 .. 8, T in 1 .. 8); a propose_only launch over one slot of four leaves the other three untouched."""
import numpy as np
import pytest
import torch

from tests import _spec_batch_reference as RB
from tests import _spec_reference as R

pytestmark = pytest.mark.gpu
HD = 16      # embedding row: E[t][c] = bit c of t, so a row of h_out names the token it was copied from


def _launch(dev, states, slot_lo=0, n=None, **over):
    """one usdm_spec_commit_batch launch on the batch `states` -> the states after it, in the reference's form"""
    from usdm_amd import ops
    RB.check_batch(states)
    s0, B = states[0], len(states)
    T, V, off = s0["T"], s0["V"], s0["id_offset"]
    t32 = lambda a: torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=dev).contiguous()
    stack = lambda k: t32(np.stack([np.asarray(s[k], np.int32) for s in states]))
    has_parts = s0["part_val"] is not None
    nparts = s0["part_val"].shape[1] if has_parts else 1
    pv = torch.tensor(np.concatenate([s["part_val"] for s in states]), dtype=torch.float32, device=dev) if has_parts else None
    pi = t32(np.concatenate([s["part_idx"] for s in states])) if has_parts else None
    pmax = max(len(s["prompt"]) for s in states) + 1
    prompt = t32(np.stack([np.concatenate([s["prompt"], np.full(pmax - len(s["prompt"]), -7)]) for s in states]))
    drafts, limit, plen, counters = stack("drafts"), stack("limit"), stack("prompt_len"), stack("counters")
    params = t32(s0["params"])
    script = None if s0["script"] is None else stack("script")
    nxt, out, step, pos, done, eos = stack("next_token"), stack("out_tokens"), stack("step"), stack("pos"), stack("done"), stack("eos")
    E = ((torch.arange(V + off)[:, None] >> torch.arange(HD)[None]) & 1).to(torch.bfloat16).contiguous().to(dev)
    h = torch.full((B * T, HD), -1.0, dtype=torch.bfloat16, device=dev)
    st = ops.decode_state(nxt, out, step, pos, id_offset=off, batch=over.pop("batch", B), done=over.pop("done", done), eos=eos)
    st.max_out = out.shape[-1]
    kw = dict(T=T, drafts=drafts, limit=limit, prompt=prompt, prompt_len=plen, params=params, counters=counters, V=V, script=script, embed=E,
              h_out=h, Hd=HD, slot_lo=slot_lo, n=n, propose_only=s0["propose_only"])
    kw.update(over)
    ops.spec_commit_batch(pv, pi, nparts, st, **kw)
    res = []
    for b in range(B):
        rows = h[b * T:(b + 1) * T].float().cpu()
        rows = None if bool((rows == -1).all()) else [int(x) for x in (rows.long() << torch.arange(HD)[None]).sum(1).tolist()]
        res.append(dict(drafts=drafts[b].cpu().numpy(), out_tokens=out[b].cpu().numpy(), counters=counters[b].cpu().numpy(), step=int(step[b]),
                        pos=int(pos[b]), next_token=int(nxt[b]), done=int(done[b]), rows=rows))
    return res


def _same(name, got, ref):
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        for k in ("step", "pos", "next_token", "done", "rows"):
            assert g[k] == r[k], (name, b, k, g[k], r[k])
        for k in ("drafts", "out_tokens", "counters"):
            assert np.array_equal(g[k], r[k]), (name, b, k, g[k], r[k])


def _check(name, states, **kw):
    ref = RB.spec_commit_batch_ref(states, **kw)
    _same(name, _launch(torch.device("cuda"), states, **kw), ref)
    return ref


P10 = [5, 6, 7, 8, 5, 6, 9, 5, 6, 7]
PICKS, ALL = [11, 12, 13, 14], [11, 12, 13]


def hand_batches():
    """(name, states, what a reader can check by eye: per slot the tokens emitted and / or the done word)"""
    fp = lambda **kw: R.from_picks(4, PICKS, **dict(dict(drafts=ALL, out_tokens=[3]), **kw))
    c = []
    c.append(("a slot done on entry", [fp(), fp(done=1, counters=(4, 5, 6)), fp(drafts=[11, 2, 13])],
              dict(emitted=[PICKS, [], [11, 12]], done=[0, 1, 0])))
    c.append(("limit inside the accepted run, the neighbour accepts everything", [fp(limit=3), fp(), fp(out_tokens=[3, 4], limit=2)],
              dict(emitted=[[11, 12], PICKS, []], done=[1, 0, 1])))
    c.append(("a stop id before and after min_new", [fp(eos=[12], min_new=4), fp(eos=[12], min_new=3), fp(eos=[12]), fp(eos=[99, 13])],
              dict(emitted=[PICKS, [11, 12], [11, 12], [11, 12, 13]], done=[0, 1, 1, 1])))
    c.append(("a slot with no lookup match", [R.from_picks(3, [6, 7, 1], drafts=[6, 2], prompt=P10[:4], out_tokens=[5]),
                                               R.from_picks(3, [40, 41, 42], drafts=[1, 2], prompt=[1, 2, 3], out_tokens=[4])],
              dict(emitted=[[6, 7], [40]], drafts=[[8, 5], [-1, -1]])))
    sc = [0, 0, 31, 32, 33, 34] + [0] * 58
    c.append(("script mode", [fp(script=sc, drafts=[11, 2, 13]), fp(script=[1000, -5, 999, 7] + [0] * 60, drafts=[1, 2, 3])],
              dict(emitted=[[11, 12], [11]], drafts=[[32, 33, 34], [999, 7, 0]])))
    c.append(("draft ids outside [0, V)", [fp(script=[0, 1000, -5, 999] + [0] * 60, drafts=[1000, -5, 12], V=1000),
                                            fp(script=[0, 0, 5, 1000, 2] + [0] * 59, drafts=[11, 1000, 13], V=1000)],
              dict(emitted=[[11], [11, 12]], drafts=[[-1, 999, 0], [-1, 2, 0]])))
    return c


def test_hand_built_states(dev):
    for name, states, exp in hand_batches():
        ref = _check(name, states)
        for b, (s, r) in enumerate(zip(states, ref)):      # the reference itself, against what a reader can check by eye
            if "emitted" in exp:
                assert R.emitted(s, r) == exp["emitted"][b], (name, b, R.emitted(s, r))
            if "done" in exp:
                assert r["done"] == exp["done"][b], (name, b)
            if "drafts" in exp:
                assert r["drafts"][1:s["T"]].tolist() == exp["drafts"][b], (name, b, r["drafts"])


def test_random_states(dev):
    seen = set()
    for seed in range(200):
        states = RB.random_batch(seed)
        ref = _check(f"seed {seed}", states)
        seen.add((len(states), states[0]["T"], max(r["step"] - s["step"] for s, r in zip(states, ref))))
    assert {b for b, _, _ in seen} == set(range(2, 9)) and {t for _, t, _ in seen} == set(range(1, 9))
    assert max(m for _, _, m in seen) >= 3      # the cases do accept runs


def test_propose_only_over_one_slot_of_four(dev):
    """an admitted request gets its first drafts and input rows; every word of the other three slots stays as it was"""
    mk = lambda prompt, out, **kw: R.new_state(4, prompt=prompt, out_tokens=out, propose_only=True, next_token=out[-1], **kw)
    states = [mk(P10[:7], [5, 6], counters=(1, 2, 3)), mk(P10, [7]), mk([1, 2, 3], [4], done=1), mk([9, 9, 9], [9], drafts=[4, 4, 4])]
    for b in range(4):
        ref = _check(f"slot {b}", states, slot_lo=b, n=1)
        for o in range(4):
            touched = o == b and not states[o]["done"]
            assert (ref[o]["rows"] is not None) == touched
            if not touched:
                assert np.array_equal(ref[o]["drafts"], states[o]["drafts"])
    assert _check("slot 0", states, slot_lo=0, n=1)[0]["drafts"][1:4].tolist() == [9, 5, 6]
    _check("slots 1 and 2", states, slot_lo=1, n=2)


def test_refusals(dev):
    from usdm_amd._lib import UsdmError
    ok = [R.from_picks(4, PICKS, drafts=ALL, out_tokens=[3]) for _ in range(2)]
    _launch(dev, ok)
    bad = [("T = 0", dict(T=0)), ("T = 9", dict(T=9)), ("V = 0", dict(V=0)), ("slots past the state", dict(slot_lo=1, n=2)),
           ("slot_lo < 0", dict(slot_lo=-1, n=1)), ("n = 0", dict(n=0)), ("no done words", dict(done=None)), ("B * T = 20", dict(batch=5)),
           ("B = 0", dict(batch=0))]
    for what, kw in bad:
        with pytest.raises(UsdmError):
            _launch(dev, ok, **kw)
            pytest.fail(what)
