"""The batched speculative commit (usdm_spec_commit_batch) restated with tests/_spec_reference.py: that file's spec_commit_ref applied
slot by slot.  A batch is a list of its state dicts that agree in what the launch shares: T, the partials' width, V, max_out,
id_offset, the lookup params (use_script included) and the prompt row's width."""
import numpy as np

from tests import _spec_reference as R

SHARED = ("T", "V", "id_offset", "propose_only")


def check_batch(states):
    s0 = states[0]
    for s in states:
        assert all(s[k] == s0[k] for k in SHARED) and np.array_equal(s["params"], s0["params"])
        assert len(s["out_tokens"]) == len(s0["out_tokens"]) and (s["script"] is None) == (s0["script"] is None)
        assert (s["part_val"] is None) == (s0["part_val"] is None) and (s["part_val"] is None or s["part_val"].shape == s0["part_val"].shape)
    assert 1 <= len(states) and len(states) * s0["T"] <= 16


def spec_commit_batch_ref(states, slot_lo=0, n=None):
    """-> the states after one launch over the slots [slot_lo, slot_lo + n): spec_commit_ref on those, the others as they were (rows None)"""
    n = len(states) - slot_lo if n is None else n
    return [R.spec_commit_ref(s) if slot_lo <= b < slot_lo + n else dict(s, rows=None) for b, s in enumerate(states)]


def random_batch(seed):
    """a seeded random multi-slot state: B in 2 .. 8, T in 1 .. 8 with B * T <= 16, a small vocabulary so that drafts match, per-slot
    stop ids, limits, histories, done words and counters"""
    g = np.random.default_rng(1000 + seed)
    B = int(g.integers(2, 9))
    T = int(g.integers(1, min(8, 16 // B) + 1))
    V, nparts, max_out = 12, int(g.integers(1, 7)), int(g.integers(4, 40))
    use_script = g.random() < 0.3
    lookup = (int(g.integers(1, 5)), int(g.integers(1, 3)))
    states = []
    for _ in range(B):
        nout = int(g.integers(1, max_out + 1))
        picks = g.integers(0, V, T)
        drafts = np.where(g.random(T - 1) < 0.6, picks[:T - 1], g.integers(-1, V, T - 1))
        val = g.integers(-3, 3, (T, nparts)).astype(np.float32)
        idx = g.integers(0, V, (T, nparts)).astype(np.int32)
        for i in range(T):
            if g.random() < 0.7:
                j = int(g.integers(0, nparts))
                val[i, j], idx[i, j] = 5.0, picks[i]
        states.append(R.new_state(T, part_val=val, part_idx=idx, drafts=drafts.tolist(), limit=int(g.integers(1, max_out + 4)),
                                  prompt=g.integers(0, V, int(g.integers(0, 30))).tolist(),
                                  script=g.integers(-1, V + 1, max_out).tolist() if use_script else None, lookup=lookup, V=V, max_out=max_out,
                                  out_tokens=g.integers(0, V, nout).tolist(), pos=int(g.integers(0, 100)), next_token=int(g.integers(0, V)),
                                  done=int(g.random() < 0.15), eos=g.integers(0, V, int(g.integers(0, 3))).tolist(),
                                  min_new=int(g.integers(0, max_out)), counters=g.integers(0, 50, 3).tolist()))
    return states
