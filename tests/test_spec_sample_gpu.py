"""usdm_spec_sample and the commit from given picks (sampled speculation) through the C-ABI.  Every comparison is ==.

  usdm_spec_sample against usdm_sample_final, kernel against kernel: picks[b * T + i] must be the token that usdm_sample_final commits
  for the same row with slot b's parameter block at step = s0[b] + i.  Both run the same text, so nothing about the fast exp enters:
  the rows may be anything - tests/_sample_reference.py's level rows (each with its case's knobs) and exact rows, seeded random rows,
  an all-banned row, NaN rows - at V in {1, 63, 1025, 3001, 42003}, (B, T) in {(1, 1), (1, 8), (2, 8), (4, 4), (8, 2)}, step offsets
  0, 1 and 2^31 - 9, per-slot knobs and seeds, unsanitised blocks included.
  Skipping: a done slot and the rows behind a -1 draft keep the sentinel their picks were filled with.
  usdm_spec_commit_picks / usdm_spec_commit_batch_picks against tests/_spec_reference.py's spec_commit_ref word for word, the picks
  being what the reference's own pick stage takes from the state's partials (from_picks states and the seeded random ones); the
  partials themselves are not passed."""
import numpy as np
import pytest
import torch

from tests import _sample_reference as SR
from tests import _spec_batch_reference as RB
from tests import _spec_reference as R

pytestmark = pytest.mark.gpu

VS = (1, 63, 1025, 3001, 42003)
SHAPES = ((1, 1), (1, 8), (2, 8), (4, 4), (8, 2))
S0 = (0, 1, 2 ** 31 - 9)
SENTINEL = -77
NAN = float("nan")
# (temperature, top_k, top_p, min_p): plain, every filter, greedy, and blocks the kernel has to sanitise
KNOBS = ((0.8, 20, 1.0, 0.0), (1.0, 0, 0.9, 0.05), (0.7, 50, 0.95, 0.0), (1.0, 1, 1.0, 0.0), (0.0, -1, 1.5, NAN), (1.3, 0, 1.0, 0.1),
         (NAN, 3, -0.5, 2.0), (2.0, 0, 1.0, 0.0))
SEEDS = (0, 7, 2 ** 32 + 3, 2 ** 40 + 7, 12345, 2 ** 63 + 5, 99, 31337)


def _block(dev, knobs, seeds):
    """[n][24] device parameter blocks, written as they are (no host-side check)"""
    from usdm_amd import ops
    t = ops.sample_params_tensor(dev, max(2, len(knobs)))[:len(knobs)]
    for b, ((temp, k, p, mp), seed) in enumerate(zip(knobs, seeds)):
        ops.set_sample_params(t[b], temp, k, p, seed, min_p=mp)
    return t


def _reference_tokens(dev, rows, block, steps):
    """usdm_sample_final's batched form over the n rows, row r with block[r] at steps[r] -> the n tokens it commits"""
    from usdm_amd import ops
    n = rows.shape[0]
    nxt, out, pos = (torch.full((n,), v, dtype=torch.int32, device=dev) for v in (-3, -5, 7))
    stp = torch.tensor(steps, dtype=torch.int32, device=dev)
    if n == 1:
        ops.sample_final(rows[0], ops.decode_state(nxt, out, stp, pos), dev_params=block[0])
    else:
        ops.sample_final(rows, ops.decode_state(nxt, out.view(n, 1), stp, pos, batch=n), dev_params=block)
    assert stp.tolist() == [s + 1 for s in steps]
    return nxt.tolist()


def _check(dev, rows, B, T, knobs, seeds, s0, drafts=None, done=None, what=""):
    """one usdm_spec_sample launch over rows [B * T][V] against usdm_sample_final row by row; skipped rows keep the sentinel"""
    from usdm_amd import ops
    rows = torch.as_tensor(np.asarray(rows, np.float32)).to(dev)
    block = _block(dev, knobs, seeds)
    d = np.zeros((B, 8), np.int32) if drafts is None else np.asarray(drafts, np.int32)
    dn = np.zeros(B, np.int32) if done is None else np.asarray(done, np.int32)
    step = torch.tensor(s0, dtype=torch.int32, device=dev)
    picks = torch.full((B * T,), SENTINEL, dtype=torch.int32, device=dev)
    ops.spec_sample(rows, picks, T=T, n=B, dev_params=block, step=step, done=torch.tensor(dn, device=dev), drafts=torch.tensor(d, device=dev))
    assert step.tolist() == list(s0)                                          # no state word moves
    per_row = block.repeat_interleave(T, 0).contiguous()
    ref = _reference_tokens(dev, rows, per_row, [s0[b] + i for b in range(B) for i in range(T)])
    live = [not dn[b] and all(d[b, j] >= 0 for j in range(1, i + 1)) for b in range(B) for i in range(T)]
    want = [t if ok else SENTINEL for t, ok in zip(ref, live)]
    assert picks.tolist() == want, (what, B, T, s0, picks.tolist(), want)
    return live


def _pool(V):
    """the rows of vocabulary size V: exact rows, seeded random rows with bans, an all-banned row, NaN rows (V = 3001: + the level rows)"""
    g = np.random.default_rng(V)
    rows = [SR.exact_row(V, kept) for _, kept in SR.exact_patterns(V)]
    for scale in (1.0, 4.0, 12.0):
        x = (g.standard_normal(V) * scale).astype(np.float32)
        x[g.random(V) < 0.2] = -np.inf
        rows.append(x)
    x = g.standard_normal(V).astype(np.float32)
    x[g.random(V) < 0.5] = np.nan                                             # some NaN among finite logits
    rows += [np.full(V, -np.inf, np.float32), np.full(V, np.nan, np.float32), x]
    if V == SR.LV:
        rows += [SR.level_case(i)[1] for i in range(len(SR.LEVEL_CASES))]
    return rows


@pytest.mark.parametrize("V", VS)
def test_rows_equal_sample_final(dev, V):
    pool, r0, seen = _pool(V), 0, 0
    while seen < len(pool):                                                   # every row of the pool at least once
        for B, T in SHAPES:
            for j, s in enumerate(S0):
                rows = [pool[(r0 + r) % len(pool)] for r in range(B * T)]
                knobs = [KNOBS[(r0 + b + j) % len(KNOBS)] for b in range(B)]
                seeds = [SEEDS[(r0 + 3 * b) % len(SEEDS)] for b in range(B)]
                _check(dev, rows, B, T, knobs, seeds, [s + (b if s == 1 else 0) for b in range(B)], what=f"V={V} rows from {r0}")
                r0, seen = r0 + B * T, seen + B * T


def test_level_rows_with_their_knobs(dev):
    """every level row of tests/_sample_reference.py drawn with its own case's knobs, in every shape and at every step offset"""
    n = len(SR.LEVEL_CASES)
    for i in range(n):
        c = SR.level_case(i)[0]
        B, T = SHAPES[i % len(SHAPES)]
        rows = [SR.level_case((i + r) % n if r % T else i)[1] for r in range(B * T)]      # row 0 of every slot: the case's own row
        knobs = [(c["T"], c["k"], c["p"], c["min_p"])] * B
        _check(dev, rows, B, T, knobs, [SEEDS[(i + b) % len(SEEDS)] for b in range(B)], [S0[(i + b) % len(S0)] for b in range(B)], what=c["name"])


def test_draws_differ_by_position_and_seed(dev):
    """the comparison above is not vacuous: one flat row drawn at 16 counters / with 2 seeds gives more than a few distinct tokens"""
    from usdm_amd import ops
    V = 3001
    rows = torch.zeros(16, V, device=dev)
    block = _block(dev, [(1.0, 0, 1.0, 0.0)] * 2, [5, 6])
    picks = torch.full((16,), SENTINEL, dtype=torch.int32, device=dev)
    ops.spec_sample(rows, picks, T=8, n=2, dev_params=block, step=torch.zeros(2, dtype=torch.int32, device=dev),
                    drafts=torch.zeros(2, 8, dtype=torch.int32, device=dev))
    p = picks.tolist()
    assert len(set(p)) >= 8 and all(0 <= t < V for t in p) and p[:8] != p[8:]
    want = [SR.sample_ref(np.zeros(V, np.float32), i, seed=s)[2] for s in (5, 6) for i in range(8)]      # exact row: no exp involved
    assert p == want


def test_done_slots_and_rows_behind_a_missing_draft_are_skipped(dev):
    g = np.random.default_rng(3)
    V, B, T = 1025, 2, 8
    rows = (g.standard_normal((B * T, V)) * 3).astype(np.float32)
    d = np.full((B, 8), 5, np.int32)
    d[:, 0] = -1                                                              # word 0 is not a draft: never read
    d[0, 4] = -1                                                              # slot 0: rows 0 .. 3 are reachable, 4 .. 7 are not
    live = _check(dev, rows, B, T, KNOBS[:2], SEEDS[:2], [3, 9], drafts=d)
    assert live == [True] * 4 + [False] * 4 + [True] * 8
    d[1, 1] = -1                                                              # slot 1: only row 0
    live = _check(dev, rows, B, T, KNOBS[:2], SEEDS[:2], [3, 9], drafts=d)
    assert live == [True] * 4 + [False] * 4 + [True] + [False] * 7
    live = _check(dev, rows, B, T, KNOBS[:2], SEEDS[:2], [3, 9], drafts=np.full((B, 8), 5, np.int32), done=[1, 0])
    assert live == [False] * 8 + [True] * 8
    B, T = 4, 4
    live = _check(dev, rows, B, T, KNOBS[:4], SEEDS[:4], [0, 1, 2, 3], drafts=np.full((B, 8), -1, np.int32), done=[0, 1, 0, 1])
    assert live == [True, False, False, False] + [False] * 4 + [True, False, False, False] + [False] * 4


def test_refusals(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    rows, block = torch.zeros(16, 64, device=dev), _block(dev, KNOBS[:2], SEEDS[:2])
    ok = dict(T=4, n=2, dev_params=block, step=z(2), drafts=z(2, 8))
    ops.spec_sample(rows, z(8), **ok)
    big = torch.zeros(32, 64, device=dev)
    for what, kw in (("T = 0", dict(T=0)), ("T = 9", dict(T=9, n=1)), ("18 rows", dict(T=6, n=3, dev_params=_block(dev, KNOBS[:3], SEEDS[:3]),
                                                                                  step=z(3), drafts=z(3, 8)))):
        with pytest.raises(UsdmError):
            ops.spec_sample(big, z(32), **dict(ok, **kw))
            pytest.fail(what)


# ------------------------------------------------------------------------------------------------ the commit from given picks
HD = 16      # embedding row: E[t][c] = bit c of t, so a row of h_out names the token it was copied from


def _commit(dev, states, batch, slot_lo=0, n=None):
    """one usdm_spec_commit_picks (batch False: one state) or usdm_spec_commit_batch_picks launch; the picks are what the reference's
    pick stage takes from each state's partials, and the partials are NOT passed -> the states after it, in the reference's form"""
    from usdm_amd import ops
    s0, B = states[0], len(states)
    T, V, off = s0["T"], s0["V"], s0["id_offset"]
    t32 = lambda a: torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=dev).contiguous()
    stack = lambda k: t32(np.stack([np.asarray(s[k], np.int32) for s in states]))
    if s0["part_val"] is not None:
        picks = t32([R.pick_row(s["part_val"][i], s["part_idx"][i]) for s in states for i in range(T)])
    else:                            # propose_only states without partials: the picks are never read
        assert s0["propose_only"]
        picks = t32([SENTINEL] * B * T)
    pmax = max(len(s["prompt"]) for s in states) + 1
    prompt = t32(np.stack([np.concatenate([s["prompt"], np.full(pmax - len(s["prompt"]), -7)]) for s in states]))
    drafts, limit, plen, counters = stack("drafts"), stack("limit"), stack("prompt_len"), stack("counters")
    params = t32(s0["params"])
    script = None if s0["script"] is None else stack("script")
    nxt, out, step, pos, done, eos = stack("next_token"), stack("out_tokens"), stack("step"), stack("pos"), stack("done"), stack("eos")
    E = ((torch.arange(V + off)[:, None] >> torch.arange(HD)[None]) & 1).to(torch.bfloat16).contiguous().to(dev)
    h = torch.full((B * T, HD), -1.0, dtype=torch.bfloat16, device=dev)
    kw = dict(T=T, drafts=drafts, limit=limit, prompt_len=plen, params=params, counters=counters, V=V, script=script, embed=E, h_out=h, Hd=HD,
              propose_only=s0["propose_only"], picks=picks)
    if batch:
        st = ops.decode_state(nxt, out, step, pos, id_offset=off, batch=B, done=done, eos=eos)
        st.max_out = out.shape[-1]
        ops.spec_commit_batch(None, None, 0, st, prompt=prompt, slot_lo=slot_lo, n=n, **kw)
    else:
        assert B == 1
        st = ops.decode_state(nxt[0:1], out[0], step[0:1], pos[0:1], id_offset=off, done=done[0:1], eos=eos[0])
        ops.spec_commit(None, None, 0, st, prompt=prompt[0], **dict(kw, drafts=drafts[0], limit=limit[0:1], prompt_len=plen[0:1],
                                                                   counters=counters[0], script=None if script is None else script[0]))
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


def test_commit_from_picks_single(dev):
    """the hand-built cases (accept counts, a stop id inside an accepted run, a limit inside a run, id_offset, propose_only, the
    lookup and the script) and 100 seeded random states"""
    names = set()
    for name, s, _ in R.hand_cases():
        _same(name, _commit(dev, [s], False), [R.spec_commit_ref(s)])
        names.add(name)
    assert {"stop id inside the accepted run", "limit cuts the run", "script replaces the lookup", "id_offset"} <= names
    s = R.from_picks(8, list(range(20, 28)), drafts=[20, 21, 22, 9, 24, 25, 26], out_tokens=[1], prompt=[20, 21, 22, 23])
    ref = R.spec_commit_ref(s)
    assert R.emitted(s, ref) == [20, 21, 22, 23]
    _same("from_picks, T = 8", _commit(dev, [s], False), [ref])
    for seed in range(100):
        s = R.random_case(seed)
        _same(f"seed {seed}", _commit(dev, [s], False), [R.spec_commit_ref(s)])


def test_commit_from_picks_batch(dev):
    fp = lambda **kw: R.from_picks(4, [11, 12, 13, 14], **dict(dict(drafts=[11, 12, 13], out_tokens=[3]), **kw))
    hand = [("done, partial accept", [fp(), fp(done=1, counters=(4, 5, 6)), fp(drafts=[11, 2, 13])]),
            ("a limit inside the run", [fp(limit=3), fp(), fp(out_tokens=[3, 4], limit=2)]),
            ("a stop id inside the run, before and after min_new", [fp(eos=[12], min_new=4), fp(eos=[12], min_new=3), fp(eos=[12]), fp(eos=[99, 13])]),
            ("propose_only", [fp(propose_only=True, prompt=[3, 11, 12, 3]), fp(propose_only=True, prompt=[1, 2])])]
    for name, states in hand:
        _same(name, _commit(dev, states, True), RB.spec_commit_batch_ref(states))
    states = hand[0][1]
    _same("one slot of three", _commit(dev, states, True, slot_lo=2, n=1), RB.spec_commit_batch_ref(states, 2, 1))
    po = [dict(s, propose_only=True) for s in states]
    _same("propose_only over one slot", _commit(dev, po, True, slot_lo=0, n=1), RB.spec_commit_batch_ref(po, 0, 1))
    for seed in range(100):
        states = RB.random_batch(seed)
        _same(f"seed {seed}", _commit(dev, states, True), RB.spec_commit_batch_ref(states))


def test_commit_from_picks_refusals(dev):
    from usdm_amd import _lib, ops
    import ctypes as C
    s = R.from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3])
    _commit(dev, [s], False)
    with pytest.raises(_lib.UsdmError):
        _commit(dev, [R.from_picks(9, list(range(9)), out_tokens=[3])], False)      # T = 9
    # picks == NULL without propose_only, straight through the C-ABI
    a, st = _lib.SpecArgs(), ops.decode_state(*(torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(4)))
    a.T, a.V = 4, 10
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    for f in ("drafts", "limit", "prompt_len", "params", "counters"):
        setattr(a, f, z.data_ptr())
    E, h = torch.zeros(16, 16, dtype=torch.bfloat16, device=dev), torch.zeros(4, 16, dtype=torch.bfloat16, device=dev)
    rc = _lib.lib.usdm_spec_commit_picks(C.byref(a), C.c_void_p(0), C.byref(st), C.c_void_p(E.data_ptr()), C.c_int32(16), C.c_void_p(h.data_ptr()), ops._stream())
    assert rc != 0 and b"picks" in _lib.lib.usdm_last_error()
