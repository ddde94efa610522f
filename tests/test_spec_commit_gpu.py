"""usdm_spec_commit through the C-ABI against the numpy restatement of tests/_spec_reference.py: every output word ==, over the
hand-built cases of tests/test_spec_cpu.py and 200 seeded random ones (T in {2, 4, 8}); a launch with `done` set changes nothing."""
import numpy as np
import pytest
import torch

from tests import _spec_reference as R

pytestmark = pytest.mark.gpu
HD = 16      # embedding row: E[t][c] = bit c of t, so a row of h_out names the token it was copied from


def _launch(dev, s):
    """one usdm_spec_commit launch on the state dict s -> the state after it, in the reference's form"""
    from usdm_amd import ops
    T, V, off = s["T"], s["V"], s["id_offset"]
    t32 = lambda a: torch.tensor(np.asarray(a, np.int32).reshape(-1), dtype=torch.int32, device=dev)
    nparts = 1 if s["part_val"] is None else s["part_val"].shape[1]
    pv = None if s["part_val"] is None else torch.tensor(s["part_val"], dtype=torch.float32, device=dev)
    pi = None if s["part_idx"] is None else t32(s["part_idx"])
    drafts, limit, prompt = t32(s["drafts"]), t32([s["limit"]]), t32(np.concatenate([s["prompt"], [0]]))
    plen, params, counters = t32([s["prompt_len"]]), t32(s["params"]), t32(s["counters"])
    script = None if s["script"] is None else t32(s["script"])
    nxt, out, step, pos, done, eos = t32([s["next_token"]]), t32(s["out_tokens"]), t32([s["step"]]), t32([s["pos"]]), t32([s["done"]]), t32(s["eos"])
    E = ((torch.arange(V + off)[:, None] >> torch.arange(HD)[None]) & 1).to(torch.bfloat16).contiguous().to(dev)
    h = torch.full((T, HD), -1.0, dtype=torch.bfloat16, device=dev)
    st = ops.decode_state(nxt, out, step, pos, id_offset=off, done=done, eos=eos)
    ops.spec_commit(pv, pi, nparts, st, T=T, drafts=drafts, limit=limit, prompt=prompt, prompt_len=plen, params=params, counters=counters,
                    V=V, script=script, embed=E, h_out=h, Hd=HD, propose_only=s["propose_only"])
    rows = h.float().cpu()
    rows = None if bool((rows == -1).all()) else [int(x) for x in (rows.long() << torch.arange(HD)[None]).sum(1).tolist()]
    return dict(drafts=drafts.cpu().numpy(), out_tokens=out.cpu().numpy(), counters=counters.cpu().numpy(), step=int(step.item()),
                pos=int(pos.item()), next_token=int(nxt.item()), done=int(done.item()), rows=rows)


def _same(name, got, ref):
    for k in ("step", "pos", "next_token", "done", "rows"):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    for k in ("drafts", "out_tokens", "counters"):
        assert np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])


def test_hand_cases(dev):
    for name, s, _ in R.hand_cases():
        _same(name, _launch(dev, s), R.spec_commit_ref(s))


def test_random_cases(dev):
    seen = set()
    for seed in range(200):
        s = R.random_case(seed)
        ref = R.spec_commit_ref(s)
        _same(f"seed {seed}", _launch(dev, s), ref)
        seen.add((s["T"], ref["step"] - s["step"]))
    assert {t for t, _ in seen} == {2, 4, 8} and max(m for _, m in seen) >= 3      # the cases do accept runs


def test_done_launch_is_a_noop(dev):
    s = R.from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], done=1, prompt=[1, 2, 3], counters=(4, 5, 6))
    got = _launch(dev, s)
    assert got["rows"] is None and got["step"] == 1 and got["done"] == 1 and got["next_token"] == s["next_token"]
    assert np.array_equal(got["drafts"], s["drafts"]) and np.array_equal(got["out_tokens"], s["out_tokens"])
    assert np.array_equal(got["counters"], s["counters"])


def test_refusals(dev):
    from usdm_amd._lib import UsdmError
    ok = R.from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3])
    _launch(dev, ok)
    for what, kw in (("T = 0", dict(T=0)), ("T = 9", dict(T=9)), ("V = 0", dict(V=0))):
        with pytest.raises(UsdmError):
            _launch(dev, dict(ok, **kw))
            pytest.fail(what)
