"""tests/_sample_reference.py proven on the CPU: pinned to oracle/sampling_oracle.py (itself pinned to HF's warpers in
test_oracle_cpu.py) on random rows, and every hand-built row of tests/test_sample_exact_gpu.py checked against the property it is
stated to have, before a GPU sees it."""
import math

import numpy as np
import pytest

from oracle import sampling_oracle as so
from tests import _sample_reference as R


# ------------------------------------------------------------------------------------------------------------ against the oracle
def _random_row(g, V):
    x = (g.standard_normal(V) * g.choice([0.5, 3.0])).astype(np.float32)
    x = (x.view(np.uint32) & 0xFFFF0000).view(np.float32)      # bf16-valued: ties do occur
    x[g.integers(0, V, V // 10)] = R.NINF
    return x


def test_reference_equals_the_oracle_on_random_rows():
    g = np.random.default_rng(20)
    n_tok = n_slack = 0
    for it in range(300):
        V = int(g.choice([5, 48, 517, 1000, 1025, 4099]))
        x = _random_row(g, V)
        T = float(g.choice([0.5, 0.7, 1.0, 1.3, 2.0]))
        k = int(g.choice([0, 0, 1, 2, 10, V // 2, V - 1, V, V + 3]))
        p = float(g.choice([1.0, 0.97, 0.9, 0.5, 0.1]))
        F = R.filter_ref(x, T, k, p)
        want = so.filtered_probs(x, T, k, p)
        got = R.probs(F)
        assert ((got > 0) == (want > 0)).all(), (it, V, T, k, p)
        assert (F.kept >= (got > 0)).all()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        for step, seed in ((0, 0), (3, 12345), (2 ** 31 - 1, 2 ** 40 + 7)):
            if k == 1:
                continue                  # (u = 0 is the kernel's greedy slot; the oracle draws)
            tok, slack = R.draw_ref(F, seed, step)
            n_tok += 1
            if slack >= R.SLACK:          # (the oracle walks float64 probabilities: within the slack both name the same id)
                n_slack += 1
                assert tok == so.sample(x, step, T, k, p, seed)[0], (it, step, seed)
    assert n_slack > 0.9 * n_tok


def test_reference_returns_kept_masses_token_slack():
    x = np.array([0.0, 1.0, R.NINF, 1.0], np.float32)
    kept, mass, tok, slack = R.sample_ref(x, 5, seed=9)
    assert kept.tolist() == [True, True, False, True]
    assert mass.tolist() == [int(math.floor(float(np.exp(np.float32(-1))) * 2 ** 32)), 2 ** 32, 0, 2 ** 32]
    u = so.philox_uniform(9, 5) * float(mass.sum())
    assert tok == [i for i in (0, 1, 3) if u < float(np.cumsum(mass)[i])][0] and 0 < slack < 0.5
    # min-p: e >= f32(min_p)
    assert R.filter_ref(x, min_p=0.5).kept.tolist() == [False, True, False, True]
    assert R.filter_ref(x, min_p=float(np.exp(np.float32(-1)))).kept.tolist() == [True, True, False, True]
    # zero-mass fallback: lowest-index arg-max of the finite logits, else 0
    assert R.sample_ref(np.full(7, R.NINF, np.float32), 0)[2] == 0
    assert R.sample_ref(np.full(7, np.nan, np.float32), 0)[2] == 0
    y = np.full(7, np.nan, np.float32)
    y[[2, 4, 6]] = -5.0, -3.0, -3.0
    assert R.fallback(y) == 4
    # sanitising of a device parameter block
    assert R.sanitize(0.0, -3, 0.0, -0.1) == (1.0, 0, 1.0, 0.0)
    assert R.sanitize(-2.0, 5, 1.5, 1.5) == (1.0, 5, 1.0, 0.0)
    assert R.sanitize(math.nan, 0, math.nan, math.nan) == (1.0, 0, 1.0, 0.0)
    assert R.sanitize(0.7, 3, 0.5, 0.25) == (float(np.float32(0.7)), 3, 0.5, 0.25)


def test_vectorised_philox_equals_the_oracles():
    for seed in (0, 12345, 2 ** 40 + 7, 2 ** 63 + 5):
        ctrs = [0, 1, 17, 2 ** 31 - 1, 2 ** 32 - 1]
        assert R.philox_uniform_np(seed, ctrs).tolist() == [so.philox_uniform(seed, c) for c in ctrs]


def test_reference_keeps_negative_zero_tied_with_positive_zero():
    x = np.array([2.0, -0.0, 0.0, -0.0, -1.0, 0.0, -1.0], np.float32)
    for T in (1.0, 0.7):
        F = R.filter_ref(x, T, 2)         # the 2nd largest is a zero: HF's `scores < kth` removes neither sign
        assert F.kept.tolist() == [True, True, True, True, False, True, False]
        assert (so.filtered_probs(x, T, 2) > 0).tolist() == F.kept.tolist()


# ------------------------------------------------------------------------------------------------------------------- exact rows
@pytest.mark.parametrize("V", R.EXACT_V + (R.BIG_V,))
def test_exact_rows(V):
    pats = R.exact_patterns(V)
    names = [n for n, _ in pats]
    if V == R.BIG_V:
        assert names == ["none banned", "every second id banned"] and pats[1][1].size == V // 2
    elif V > 2:
        assert {"only id 0", "only id V - 1", "only the last thread's range"} <= set(names)
        if V >= 63:
            assert "only ranges between empty neighbours" in names
    per = -(-V // R.NT)
    for name, kept in pats:
        n = kept.size
        if name == "only the last thread's range":
            assert kept[0] // per == kept[-1] // per == (V - 1) // per and kept[-1] == V - 1
        if name == "only ranges between empty neighbours":
            ts = set((kept // per).tolist())
            assert all(t - 1 not in ts and t + 1 not in ts for t in ts)
        F, pairs = R.exact_pairs(V, kept)
        assert F.kept.nonzero()[0].tolist() == kept.tolist() and set(F.mass[kept].tolist()) == {R.Q1} and F.Zk == n * R.Q1
        assert len(pairs) >= 64 and len(set((s, t) for s, t, _ in pairs)) == len(pairs)
        steps, seeds = {t for _, t, _ in pairs}, {s for s, _, _ in pairs}
        assert 0 in steps and 2 ** 31 - 1 in steps and max(seeds) > 2 ** 32
        for seed, step, tok in pairs[:64] + pairs[64::max(1, len(pairs) // 200)]:      # (every pair at small V, a sample of them at large V)
            assert tok == int(kept[int(so.philox_uniform(seed, step) * n)]) == R.draw_ref(F, seed, step)[0]
        drawn = {tok for _, _, tok in pairs}
        # the first and the last kept id, and both sides of every thread-range boundary that has kept ids next to it
        want = {int(kept[0]), int(kept[-1])}
        for a, b in zip(kept[:-1].tolist(), kept[1:].tolist()):
            if a // per != b // per:
                want |= {a, b}
        assert want <= drawn and want == set(R.edge_ids(V, kept))


# ------------------------------------------------------------------------------------------------------------------- level rows
@pytest.mark.parametrize("i", range(len(R.LEVEL_CASES)), ids=[c["name"] for c in R.LEVEL_CASES])
def test_level_rows(i):
    c, row, F, pairs = R.level_case(i)
    p = R.probs(F)
    stated = R.keep_mask(c, row)
    assert ((p > 0) == stated).all(), "the stated kept levels are not what the reference keeps"
    assert stated.any() and (F.kept >= stated).all()
    want = so.filtered_probs(row, c["T"], c["k"], c["p"])
    if c["min_p"] == 0:
        assert ((want > 0) == stated).all()
        np.testing.assert_allclose(p, want, rtol=0, atol=1e-12)
    if c.get("equal_R"):
        # the masses below 2^21 are small integers, each at least 1e-3 of itself away from the next integer: exact under any exp
        small = np.unique(F.e[(F.q > 0) & (F.q < 2 ** 21)]).astype(np.float64) * 2.0 ** 32
        assert sorted(np.floor(small).tolist()) == [1, 8, 24] and F.R == 256 and F.Ztot == 2 ** 32 + 96 + 160 + 240
        assert (np.minimum(small - np.floor(small), np.ceil(small) - small) / small).min() >= 1e-3
        assert [cum for _, _, cum in F.blocks] == [96, 256, 496, F.Ztot]
    else:
        assert R.margin(F, c["min_p"]) >= R.MARGIN
        # every mass that counts is far above the 2^-32 grain of the fixed point (so a few ulp of exp stay a few ulp of probability) ...
        assert F.mass[F.mass > 0].min() >= 2 ** 21
    # ... and every removed level is removed as a whole, every kept level kept as a whole
    for v in np.unique(row[np.isfinite(row)]):
        assert len(set((p[row == v] > 0).tolist())) == 1
    if "digits" in c:
        key = R.fkey(F.kth)
        assert {s: (key >> s) & 255 for s in (24, 16, 8, 0)} == c["digits"], hex(key)
    if c["k"] and c["k"] < R.LV:
        x = np.sort(F.x)[::-1]
        assert x[c["k"] - 1] == F.kth
    if "straddle" in c:
        blk = {v: (m, cum) for v, m, cum in F.blocks}
        e_of = lambda v: float(F.e[row == np.float32(v)][0])
        m, cum = blk[e_of(c["straddle"])]
        assert cum - m <= F.R < cum and m > 0
        if m < F.Ztot and c["straddle"] != max(c["keep"]):
            assert (row == np.float32(c["straddle"])).sum() > 1          # a tie block, kept as a whole
        if "fits" in c:
            m, cum = blk[e_of(c["fits"])]
            assert cum <= F.R and not p[row == np.float32(c["fits"])].any()
    if "zero_mass" in c:
        z = row == np.float32(c["zero_mass"])
        assert (F.e[z] > 0).all() and not F.q[z].any() and not p[z].any()
        assert c["p"] < 1 or F.kept[z].all()                            # kept by the filters, yet never drawn
    if c.get("signed_zero"):
        z = F.x[(F.x == 0)]
        assert np.signbit(z).any() and not np.signbit(z).all() and F.kth == 0 and c["k"] < (F.x >= 0).sum()
        assert (p[row == 0] > 0).all()
    if c.get("lowest"):
        assert {tok for _, _, tok in pairs} == {int(np.flatnonzero(row == row.max())[0])}
        assert np.flatnonzero(p).size == 3 and set(p[p > 0].tolist()) == {1 / 3}
    # the pairs: enough of them, none below the slack, the first and the last id with mass among the draws
    assert len(pairs) >= R.LEVEL_PAIRS
    for seed, step, tok in pairs:
        t, slack = R.draw_ref(F, seed, step)
        assert t == tok and slack >= R.SLACK and p[tok] > 0
    if not c.get("lowest"):
        has = np.flatnonzero(p)
        assert {int(i) for i in (has[0], has[-1]) if p[i] >= 4 * R.SLACK} <= {tok for _, _, tok in pairs}


def test_level_rows_cover_the_digit_edges():
    """digit 0x00 and digit 0xFF of the k-th key at each of the four shifts of the radix select"""
    seen = {(s, d) for c in R.LEVEL_CASES for s, d in c.get("digits", {}).items()}
    assert {(s, d) for s in (24, 16, 8, 0) for d in (0x00, 0xFF)} <= seen
