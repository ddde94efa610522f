"""usdm_beam_step and usdm_kv_reorder through usdm_amd.ops, against tests/_beam_reference.beam_step (float64) and a numpy gather.

Tolerance of a candidate's value: tests/_logprob_reference.kernel_tolerance() for the log-probability (the kernel's arithmetic is
usdm_logprobs') plus half an ulp of the float32 sum score + lp.  The seeds below were chosen on the CPU so that the float64
reference's gaps between consecutive kept candidates, and between the last kept and the first dropped one, exceed twice that
tolerance (asserted in every test): the device's list must then be the reference's, id for id and in its order.  Exact ties are
made on purpose in tests of their own."""
import numpy as np
import pytest
import torch

from tests import _beam_reference as R
from tests import _logprob_reference as LR

pytestmark = pytest.mark.gpu

HD, PAD, MAX_OUT = 64, 5, 6
VS, BS, PATTERNS = (42003, 1000, 64), (1, 2, 4, 5, 16), ("none", "range")
SEEDS = {(42003, 2, 'none'): 2, (42003, 4, 'none'): 2, (42003, 4, 'range'): 3, (42003, 5, 'none'): 3, (42003, 5, 'range'): 3,
         (42003, 16, 'none'): 196, (42003, 16, 'range'): 30, (1000, 1, 'range'): 2, (1000, 2, 'range'): 2, (1000, 4, 'none'): 16,
         (1000, 5, 'range'): 9}      # (V, B, pattern) -> seed; anything not listed uses seed 1 (all were checked on the CPU: _case asserts the gaps)


def _n_eos_for(B, k):
    """n_eos cycles through 0, 1, 3 over the cases; 16 beams leave room for at most one EOS id (KC <= 32)"""
    return (0, 1, 3)[k % 3] if B < 16 else (0, 1)[k % 2]


GENERIC = [(V, B, p, _n_eos_for(B, k)) for k, (V, B, p) in enumerate((V, B, p) for V in VS for B in BS for p in PATTERNS)]


def tol_of(ref_scores):
    fin = np.isfinite(ref_scores)
    t = np.zeros(ref_scores.shape)
    t[fin] = LR.kernel_tolerance() + 0.5 * np.spacing(np.abs(ref_scores[fin]).astype(np.float32)).astype(np.float64)
    return t


def _rows(V, B, pattern, seed):
    rows = np.stack([LR.banned(LR.bf16_row(V, 1000 * seed + 31 * V + b), pattern) for b in range(B)])
    scores = (-np.random.default_rng(seed + 7).uniform(0.0, 6.0, B)).astype(np.float32)
    return rows, scores


def _gaps_ok(rows, scores, nlive, eos, B):
    """the precondition: every gap of the float64 reference around the kept candidates exceeds twice the tolerance"""
    V, KC = rows.shape[1], R.candidates(B, len(eos))
    s = np.stack([np.float64(scores[b]) + R.log_softmax64(rows[b]) for b in range(nlive)]).reshape(-1)
    top = np.sort(s)[::-1][:KC + 1]
    fin = np.isfinite(top)
    if not fin.all():
        return False
    return bool((-(np.diff(top)) > 2 * tol_of(top)[:-1]).all())


def _case(V, B, pattern, n_eos, nlive=None):
    seed = SEEDS.get((V, B, pattern), 1)
    rows, scores = _rows(V, B, pattern, seed)
    nlive = B if nlive is None else nlive
    plain = R.beam_step(rows, scores, nlive, [-1, -2, -3][:n_eos], B)      # (the candidates do not depend on which ids are EOS)
    eos = [int(t) for t in dict.fromkeys(plain["cand_token"].tolist())][1:1 + n_eos]      # (not the best one: the first beam survives)
    assert len(eos) == n_eos
    assert _gaps_ok(rows, scores, nlive, eos, B), "choose another seed for this case"
    return rows, scores, eos


class _Dev:
    """Device buffers of one usdm_beam_step call over rows [B][V] (held with logits_bs = V + PAD, the padding poisoned)"""

    def __init__(self, dev, rows, scores, eos, step=2, pos=9, Vtab=None):
        from usdm_amd import ops
        B, V = rows.shape
        self.B, self.V, self.KC, self.eos = B, V, R.candidates(B, len(eos)), eos
        lg = np.full((B, V + PAD), 1e30, dtype=np.float32)
        lg[:, :V] = rows
        self.logits = torch.from_numpy(lg).to(dev)
        i32 = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device=dev)
        self.score = torch.from_numpy(np.asarray(scores, dtype=np.float32)).to(dev)
        self.parent, self.nxt, self.step, self.pos = i32(B, v=-7), i32(B, v=-7), i32(B, v=step), i32(B, v=pos)
        self.out = i32(B, MAX_OUT, v=-7)
        self.eos_t = torch.tensor((list(eos) + [0, 0, 0])[:3], dtype=torch.int32, device=dev)
        self.log_score = torch.full((MAX_OUT, self.KC), 12345.0, device=dev)
        self.log_token, self.log_parent = i32(MAX_OUT, self.KC, v=-7), i32(MAX_OUT, self.KC, v=-7)
        self.cand_score, self.cand_index = torch.zeros(B, self.KC, device=dev), i32(B, self.KC)
        g = torch.Generator().manual_seed(3)
        self.E = torch.randn(V if Vtab is None else Vtab, HD, generator=g).to(torch.bfloat16).to(dev)
        self.h = torch.zeros(B, HD, dtype=torch.bfloat16, device=dev)
        self.st = ops.decode_state(self.nxt, self.out if B > 1 else self.out[0], self.step, self.pos, batch=B if B > 1 else 0)

    def run(self, nlive=None):
        from usdm_amd import ops
        ops.beam_step(self.logits, self.st, V=self.V, score=self.score, parent=self.parent, nlive=self.B if nlive is None else nlive,
                      eos=self.eos_t, n_eos=len(self.eos), log_score=self.log_score, log_token=self.log_token, log_parent=self.log_parent,
                      cand_score=self.cand_score, cand_index=self.cand_index, embed=self.E, h_out=self.h, Hd=HD)
        torch.cuda.synchronize()
        return self

    def bits(self):
        return [t.clone().view(torch.int32).cpu() if t.dtype == torch.float32 else t.clone().cpu()
                for t in (self.log_score, self.log_token, self.log_parent, self.score, self.parent, self.nxt, self.step, self.pos, self.out)]


def _check(d, rows, scores, nlive, step=2, pos=9, exact=True):
    """everything one launch wrote, against the float64 reference"""
    B, V, KC = d.B, d.V, d.KC
    ref = R.beam_step(rows, scores, nlive, d.eos, B)
    cs = d.log_score[step].cpu().numpy().astype(np.float64)
    ct, cp = d.log_token[step].cpu().numpy(), d.log_parent[step].cpu().numpy()
    flat = cp.astype(np.int64) * V + ct
    assert ((0 <= ct) & (ct < V) & (0 <= cp) & (cp < nlive)).all() and len(set(flat.tolist())) == KC
    # sorted by the device's own values under the total order
    for a in range(KC - 1):
        assert cs[a] > cs[a + 1] or (cs[a] == cs[a + 1] and flat[a] < flat[a + 1]), (a, cs[a:a + 2], flat[a:a + 2])
    # values against float64
    s_all = np.stack([np.float64(scores[b]) + R.log_softmax64(rows[b]) for b in range(nlive)])
    want = s_all[cp, ct]
    fin = np.isfinite(want)
    assert (cs[~fin] == want[~fin]).all()
    t = tol_of(want)
    assert (np.abs(cs[fin] - want[fin]) <= t[fin]).all(), float(np.abs(cs[fin] - want[fin]).max())
    # complete: nothing unlisted beats the last listed one by more than the tolerance
    rest = s_all.copy().reshape(-1)
    rest[flat] = -np.inf
    if np.isfinite(cs[-1]):
        assert rest.max() <= cs[-1] + t[-1]
    if exact:
        assert ct.tolist() == ref["cand_token"].tolist() and cp.tolist() == ref["cand_parent"].tolist()
    # the next running beams: the first B candidates that are no EOS, their embedding rows, the counters
    sel = [r for r in range(KC) if int(ct[r]) not in d.eos][:B]
    assert len(sel) == B
    assert d.nxt.cpu().tolist() == ct[sel].tolist() and d.parent.cpu().tolist() == cp[sel].tolist()
    assert torch.equal(d.score.cpu().view(torch.int32), d.log_score[step].cpu()[sel].view(torch.int32))
    assert torch.equal(d.h.cpu().view(torch.int16), d.E.cpu()[ct[sel]].view(torch.int16))
    assert d.out[:, step].cpu().tolist() == ct[sel].tolist()
    assert d.step.cpu().tolist() == [step + 1] * B and d.pos.cpu().tolist() == [pos + 1] * B
    # nothing else: the other log rows and out_tokens columns keep their fill
    other = [r for r in range(MAX_OUT) if r != step]
    assert (d.log_score[other] == 12345.0).all() and (d.log_token[other] == -7).all() and (d.log_parent[other] == -7).all()
    assert (d.out[:, other] == -7).all()
    return ref, sel


@pytest.mark.parametrize("V,B,pattern,n_eos", GENERIC)
def test_beam_step_matches_float64(dev, V, B, pattern, n_eos):
    rows, scores, eos = _case(V, B, pattern, n_eos)
    d = _Dev(dev, rows, scores, eos).run()
    _check(d, rows, scores, B)
    again = _Dev(dev, rows, scores, eos).run()
    assert all(torch.equal(a, b) for a, b in zip(d.bits(), again.bits()))      # bit-identical run to run


@pytest.mark.parametrize("V", VS)
def test_first_step_reads_row_0_only(dev, V):
    B = 4
    rows, scores, eos = _case(V, B, "none", 1, nlive=1)
    rows[1:] = 1e30      # rows that are not live must not be read
    scores[1:] = 1e30
    d = _Dev(dev, rows, scores, eos).run(nlive=1)
    ref, _ = _check(d, rows, scores, 1)
    assert d.parent.cpu().tolist() == [0] * B


@pytest.mark.parametrize("score0", [0.0, -3.25])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("V,B,n_eos", [(42003, 5, 3), (1000, 4, 0), (64, 5, 3)])      # KC = 20, 8, 20
def test_row_scores_are_usdm_logprobs_bits(dev, V, B, n_eos, pattern, score0):
    """one live row: the step's candidates are usdm_logprobs' top KC of that row, id for id, and their scores are its
    log-probabilities plus one float32 addition, bit for bit (both kernels run the row passes of csrc/logprob_row.h)"""
    from usdm_amd import ops
    rows, scores = _rows(V, B, pattern, seed=1)
    scores[0] = score0
    KC, step = R.candidates(B, n_eos), 2
    # the beam row orders by s = score + lp, usdm_logprobs by the logit: the two orders agree when logits that differ give sums that
    # differ.  Over the KC + 1 largest logits in (logit descending, id ascending) order: equal logits, or a float64 gap above 2 tol
    x = rows[0]
    order = np.lexsort((np.arange(V), -x.astype(np.float64)))[:KC + 1]
    s = np.float64(score0) + R.log_softmax64(x)[order]
    assert np.isfinite(s).all()
    same = x[order][:-1] == x[order][1:]
    assert (same | (-np.diff(s) > 2 * tol_of(s)[:-1])).all(), "choose another seed for this case"
    d = _Dev(dev, rows, scores, list(range(V - n_eos, V)))
    i32 = lambda *sh: torch.full(sh, -7, dtype=torch.int32, device=dev)
    nxt, lstep, lpos, out = i32(1), torch.ones(1, dtype=torch.int32, device=dev), i32(1), i32(MAX_OUT)      # step = 1: row 0
    tok_lp, tok_rank = torch.zeros(MAX_OUT, device=dev), i32(MAX_OUT)
    top_id, top_lp = i32(MAX_OUT * KC), torch.zeros(MAX_OUT * KC, device=dev)
    ops.logprobs(d.logits[0], ops.decode_state(nxt, out, lstep, lpos), K=KC, V=V, tok_lp=tok_lp, tok_rank=tok_rank, top_id=top_id, top_lp=top_lp)
    d.run(nlive=1)
    assert torch.equal(d.log_token[step].cpu(), top_id[:KC].cpu())
    want = np.float32(score0) + top_lp[:KC].cpu().numpy()      # float32 + float32
    assert want.dtype == np.float32
    assert d.log_score[step].cpu().numpy().view(np.int32).tolist() == want.view(np.int32).tolist()


@pytest.mark.parametrize("V,B", [(42003, 2), (1000, 4), (64, 5)])
def test_all_of_the_best_B_are_eos(dev, V, B):
    """EOS ids placed on the tokens of the first B candidates (at most 3 distinct ones): the running beams come from ranks B .. 2B-1"""
    rows, scores = _rows(V, B, "none", 1)
    free = R.beam_step(rows, scores, B, [], B)
    for b in range(B):      # the same best token in every row, far ahead: the first B candidates are that token, once per beam
        rows[b, 11] = rows[b].max() + 8.0 + 0.5 * b
    eos = [11]
    assert _gaps_ok(rows, scores, B, eos, B)
    d = _Dev(dev, rows, scores, eos).run()
    ref, sel = _check(d, rows, scores, B)
    assert ref["cand_token"][:B].tolist() == [11] * B and sel == list(range(B, 2 * B))
    assert free["cand_token"][:B].tolist() != [11] * B


def test_all_but_one_row_lists_banned_ids_in_flat_order(dev):
    """B = 2, every id but one banned in both rows, that id an EOS: the two finite candidates finish, the candidates behind them are
    -inf in flat-index order, and the beams continue with score -inf"""
    V, B = 1000, 2
    rows, scores = _rows(V, B, "all_but_one", 1)
    keep = (2 * V) // 3
    d = _Dev(dev, rows, scores, [keep]).run()
    cs, ct, cp = d.log_score[2].cpu().numpy(), d.log_token[2].cpu().tolist(), d.log_parent[2].cpu().tolist()
    order = np.argsort(-scores.astype(np.float64), kind="stable").tolist()
    assert ct == [keep, keep, 0, 1] and cp == order + [0, 0]
    assert cs[:2].tolist() == scores[order].tolist() and np.isneginf(cs[2:]).all()      # lp = 0 exactly: the score itself
    assert d.nxt.cpu().tolist() == [0, 1] and d.parent.cpu().tolist() == [0, 0] and torch.isneginf(d.score).all()
    # the next step from -inf scores: still no NaN, flat-index order
    d2 = _Dev(dev, rows, np.full(B, -np.inf, dtype=np.float32), []).run()
    assert d2.log_token[2].cpu().tolist() == [0, 1, 2, 3] and d2.log_parent[2].cpu().tolist() == [0] * 4
    assert torch.isneginf(d2.log_score[2]).all() and torch.isneginf(d2.score).all()


@pytest.mark.parametrize("V,B", [(42003, 4), (64, 16)])
def test_exact_ties_between_slots_go_by_flat_index(dev, V, B):
    """two slots with the same row and the same score: bit-equal candidate values, the lower slot first; -0.0 ties with +0.0"""
    rows, scores = _rows(V, B, "range", 1)
    rows[B - 1] = rows[0]
    scores[[0, B - 1]] = [0.0, -0.0] if B == 4 else [-0.25, -0.25]
    d = _Dev(dev, rows, scores, []).run()
    _check(d, rows, scores, B, exact=False)
    cs, ct, cp = d.log_score[2].cpu().view(torch.int32).tolist(), d.log_token[2].cpu().tolist(), d.log_parent[2].cpu().tolist()
    firsts = [r for r in range(d.KC - 1) if cp[r] == 0]
    assert firsts, "slot 0 has no candidate in the list: choose other scores"
    for r in firsts:      # its twin of the last slot follows it directly, with the same bits
        assert (cp[r + 1], ct[r + 1]) == (B - 1, ct[r]) and cs[r + 1] == cs[r], (r, cp, ct)
    assert all(cp[r - 1] == 0 and ct[r - 1] == ct[r] for r in range(d.KC) if cp[r] == B - 1)


def test_refusals(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError
    rows, scores = _rows(64, 4, "none", 1)
    d = _Dev(dev, rows, scores, [1])
    with pytest.raises(ValueError):
        ops.beam_step(d.logits, d.st, V=7, score=d.score, parent=d.parent, nlive=4, eos=d.eos_t, n_eos=1, log_score=d.log_score,
                      log_token=d.log_token, log_parent=d.log_parent, cand_score=d.cand_score, cand_index=d.cand_index)      # V < KC
    with pytest.raises(ValueError):
        ops.beam_step(d.logits, d.st, V=64, score=d.score, parent=d.parent, nlive=2, eos=d.eos_t, n_eos=1, log_score=d.log_score,
                      log_token=d.log_token, log_parent=d.log_parent, cand_score=d.cand_score, cand_index=d.cand_index)      # nlive
    big = _Dev(dev, *_rows(64, 16, "none", 1), [1])
    with pytest.raises(ValueError):
        ops.beam_step(big.logits, big.st, V=64, score=big.score, parent=big.parent, nlive=16, eos=big.eos_t, n_eos=2, log_score=big.log_score,
                      log_token=big.log_token, log_parent=big.log_parent, cand_score=big.cand_score, cand_index=big.cand_index)   # KC = 48
    # the library's own checks (the launcher), below the wrapper
    import ctypes as C
    from usdm_amd._lib import BeamArgs, lib
    a = BeamArgs()
    a.logits, a.V, a.logits_bs, a.score, a.parent = d.logits.data_ptr(), 7, 64 + PAD, d.score.data_ptr(), d.parent.data_ptr()
    a.nlive, a.n_eos, a.eos = 4, 1, d.eos_t.data_ptr()
    a.log_score, a.log_token, a.log_parent, a.log_rows = d.log_score.data_ptr(), d.log_token.data_ptr(), d.log_parent.data_ptr(), MAX_OUT
    a.cand_score, a.cand_index = d.cand_score.data_ptr(), d.cand_index.data_ptr()
    null = C.c_void_p(0)
    assert lib.usdm_beam_step(C.byref(a), C.byref(d.st), null, 0, null, null) == 2 and b"KC" in lib.usdm_last_error()
    a.V, a.n_eos = 64, 3
    bst = big.st
    a.nlive = 16
    assert lib.usdm_beam_step(C.byref(a), C.byref(bst), null, 0, null, null) == 2 and b"at most 32" in lib.usdm_last_error()
    assert UsdmError is not None and (d.log_token == -7).all() and (big.log_token == -7).all()      # nothing ran


# ---------------------------------------------------------------------------------------------- usdm_kv_reorder
L_, HKV, CTX, D = 2, 2, 64, 128
MAPS = {4: {"identity": [0, 1, 2, 3], "swap": [1, 0, 2, 3], "cycle3_dup": [1, 2, 0, 0], "all_from_one": [1, 1, 1, 1], "all_from_last": [3, 3, 3, 3]},
        16: {"identity": list(range(16)), "swap": [0, 1, 9, 3, 4, 5, 6, 7, 8, 2, 10, 11, 12, 13, 14, 15],
             "cycle3_dup": [5, 1, 2, 3, 4, 11, 6, 7, 8, 9, 10, 0, 0, 13, 5, 15], "all_from_one": [1] * 16, "all_from_last": [15] * 16}}
RANGES = [(0, 0), (0, 64), (5, 5), (5, 6), (17, 63)]


def _caches(dev, B, fp8, extra=2):
    """K, V (and the fp8 cache's exponents) of B + extra slots, a distinct pattern per (array, slot, layer, head, row, element)"""
    n = (B + extra) * L_ * HKV * CTX
    g = torch.Generator().manual_seed(17 + B)
    if fp8:
        mk = lambda: torch.randint(0, 256, (B + extra, L_ * HKV, CTX, D), generator=g, dtype=torch.int32).to(torch.uint8)
        ex = lambda: torch.randint(-100, 100, (B + extra, L_ * HKV, CTX), generator=g, dtype=torch.int32).to(torch.int8)
        arrays = [mk(), mk(), ex(), ex()]
    else:
        mk = lambda: torch.randint(-32768, 32767, (B + extra, L_ * HKV, CTX, D), generator=g, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
        arrays = [mk(), mk()]
    for a in arrays:      # (random rows could repeat; a counter in the first element of every row makes each row unique)
        flat = a.view(torch.uint8).view(n, -1)
        flat[:, 0] = (torch.arange(n) % 251).to(torch.uint8)
    return [a.to(dev) for a in arrays]


def _gather(arrays, parent, lo, pos, B):
    out = []
    for a in arrays:
        w = a.cpu().clone()
        src = a.cpu()
        for b in range(B):
            w[b, :, lo:pos] = src[parent[b], :, lo:pos]
        out.append(w)
    return out


def _raw(t):
    return t.cpu().contiguous().view(torch.uint8)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", [4, 16])
def test_kv_reorder_equals_numpy_gather(dev, B, fp8):
    from usdm_amd import ops
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    for name, parent in MAPS[B].items():
        for lo, pos in RANGES:
            arrays = _caches(dev, B, fp8)
            want = _gather(arrays, parent, lo, pos, B)
            ops.kv_reorder(arrays, i32(parent), i32([lo]), i32([pos] * B), B=B, nblk=L_ * HKV, ctx_max=CTX)
            torch.cuda.synchronize()
            for a, w in zip(arrays, want):      # bit for bit, rows outside the range and the slots beyond B included
                assert torch.equal(_raw(a), _raw(w)), (name, lo, pos)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_kv_reorder_replays_in_a_graph_with_new_parents(dev, fp8):
    """parent, lo and pos live on the device: one captured launch follows them"""
    from usdm_amd import ops
    from usdm_amd.graph import GraphedPlan
    B = 4
    arrays = _caches(dev, B, fp8)
    parent, lo, pos = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (B, 1, B))
    plan = ops.Plan()
    ops.kv_reorder(arrays, parent, lo, pos, B=B, nblk=L_ * HKV, ctx_max=CTX, plan=plan)
    g = GraphedPlan(plan, enabled=True)
    for par, (a, b) in ((MAPS[B]["swap"], (5, 6)), (MAPS[B]["cycle3_dup"], (17, 63)), (MAPS[B]["all_from_last"], (0, 64))):
        want = _gather(arrays, par, a, b, B)
        parent.copy_(torch.tensor(par, dtype=torch.int32))
        lo.fill_(a)
        pos.fill_(b)
        g.run()      # eager, capture + replay, replay
        torch.cuda.synchronize()
        for arr, w in zip(arrays, want):
            assert torch.equal(_raw(arr), _raw(w)), (par, a, b)
    assert g.graph is not None
