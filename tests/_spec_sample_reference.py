"""Shared pieces of the sampled-speculation tests (tests/test_spec_sample_*.py; TEST INFRASTRUCTURE ONLY): the two knob sets of the
model tests, the seed of the replay test with the oracle trajectory that justifies it, and the two token laws of DESIGN.md 8k-3 in
exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import torch

from tests import _sample_reference as SR
from tests import _spec_reference as R

BANNED = 5                                                        # the all-wrong script's id: banned, so no draw can equal it
KNOBS_TK = dict(temperature=0.8, top_k=20)                        # top-k is exact on keys: only the fast exp's few ulp can move a draw
KNOBS_ALL = dict(temperature=0.8, top_k=20, top_p=0.9, min_p=0.05)
# The replay test's seed: the first of 0, 1, 2, ... for which every draw of the oracle's own sampled trajectory (KNOBS_TK, the small
# model, tests/_spec_reference.py's prompt, BANNED banned) has slack >= 10 * SR.SLACK; tests/test_spec_sample_cpu.py re-derives that.
REPLAY_SEED = 2
REPLAY_SLACK = 10 * SR.SLACK


def oracle_trajectory(seed, new=R.NEW, **knobs):
    """The oracle model sampling `new` tokens with tests/_sample_reference.py's sampler, the draw of output s at Philox counter s, every
    row computed from the tokens drawn so far (teacher-forced on its own trajectory) -> (tokens, slacks)"""
    from oracle import mistral_oracle as MO
    sd = MO.random_state_dict(R.SMALL_CFG, R.MODEL_SEED)
    logits, cache = MO.forward(sd, R.SMALL_CFG, R.small_prompt())
    toks, slacks = [], []
    for s in range(new):
        row = logits[-1].float().numpy().copy()
        row[BANNED] = -np.inf
        _, _, tok, slack = SR.sample_ref(row, s, seed=seed, **knobs)
        toks.append(tok)
        slacks.append(slack)
        logits, cache = MO.forward(sd, R.SMALL_CFG, torch.tensor([tok]), cache)
    return toks, slacks


# ------------------------------------------------------------------------------------------------ the two laws, in rationals
def law_accept_if_equal(p, d):
    """Draw x ~ p with the position's own uniform, accept the draft d iff x == d, else emit x -> {token: probability} of the token
    emitted at the position, and the probability that the draft was accepted.  This side is p whatever d is, by its definition: the
    content of the equivalence test is the rejection side below, which has to come out as the same pair for every draft."""
    return {x: px for x, px in enumerate(p) if px}, (p[d] if 0 <= d < len(p) else Fraction(0))


def law_rejection_sampling(p, d):
    """Textbook speculative rejection sampling against the one-hot proposal q = delta_d: accept d with probability min(1, p(d) / q(d))
    = p(d); on rejection draw from the residual max(0, p - q) renormalised, which is p restricted to the ids other than d -> the same
    pair"""
    V = len(p)
    q = [Fraction(int(x == d)) for x in range(V)]
    acc = min(Fraction(1), p[d] / q[d]) if 0 <= d < V else Fraction(0)
    res = [max(Fraction(0), px - qx) for px, qx in zip(p, q)]
    z = sum(res)
    law = {}
    if 0 <= d < V and acc:
        law[d] = acc
    if z:
        for x, r in enumerate(res):
            if r:
                law[x] = law.get(x, Fraction(0)) + (1 - acc) * r / z
    return law, acc
