"""usdm_logprobs / usdm_logprobs_seg through usdm_amd.ops: log-probability and rank of the picked token and the top-K list of a
ban-masked logits row, against torch.log_softmax in float64 plus a stable sort by (-value, id).

Ids and ranks must match exactly; values within tests/_logprob_reference.kernel_tolerance(): four times the largest error of a numpy
f32 emulation of the kernel's arithmetic against float64 on these same rows (8.50e-07 -> 3.40e-06, derivation in that module;
asserted <= 1e-4).  The kernel runs after the pick, which has advanced the step counter: a state with step = t + 1 and
next_token = the pick writes row t."""
import numpy as np
import pytest
import torch

from tests import _logprob_reference as R

pytestmark = pytest.mark.gpu

MAX_OUT, KMAX = 8, 20
SENT_F, SENT_I = 12345.0, -7


class _Out:
    """The four output buffers for B sequences, pre-filled with a sentinel."""

    def __init__(self, dev, B=1, max_out=MAX_OUT):
        self.B, self.max_out = B, max_out
        self.tok_lp = torch.full((B, max_out), SENT_F, device=dev)
        self.tok_rank = torch.full((B, max_out), SENT_I, dtype=torch.int32, device=dev)
        self.top_id = torch.full((B, max_out * KMAX), SENT_I, dtype=torch.int32, device=dev)
        self.top_lp = torch.full((B, max_out * KMAX), SENT_F, device=dev)

    def kw(self, K):
        f = (lambda t: t[0]) if self.B == 1 else (lambda t: t)
        return dict(K=K, tok_lp=f(self.tok_lp), tok_rank=f(self.tok_rank), top_id=f(self.top_id), top_lp=f(self.top_lp))

    def row(self, b, t, K):
        """(lp, rank, ids [K], lps [K]) of row t of sequence b, on the host"""
        torch.cuda.synchronize()
        ids = self.top_id[b, :self.max_out * K].view(self.max_out, K)[t].cpu() if K else torch.zeros(0)
        lps = self.top_lp[b, :self.max_out * K].view(self.max_out, K)[t].cpu() if K else torch.zeros(0)
        return self.tok_lp[b, t].item(), self.tok_rank[b, t].item(), ids, lps

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.tok_lp == SENT_F).all() and (self.tok_rank == SENT_I).all() and (self.top_id == SENT_I).all()
                    and (self.top_lp == SENT_F).all())

    def bits(self):
        torch.cuda.synchronize()
        return [t.clone().view(torch.int32) for t in (self.tok_lp, self.tok_rank, self.top_id, self.top_lp)]


def _state(dev, toks, steps, max_out=MAX_OUT, **kw):
    """The decode state as the pick leaves it: next_token = the picked ids, step = row + 1"""
    from usdm_amd import ops
    B = len(toks)
    nxt = torch.tensor(toks, dtype=torch.int32, device=dev)
    stp = torch.tensor(steps, dtype=torch.int32, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.zeros(B, max_out, dtype=torch.int32, device=dev)
    st = ops.decode_state(nxt, out[0] if B == 1 else out, stp, pos, batch=B if B > 1 else 0, **kw)
    return st, (nxt, out, stp, pos)


@pytest.fixture(scope="module")
def tol():
    return R.kernel_tolerance()


@pytest.mark.parametrize("pattern", R.BANS)
@pytest.mark.parametrize("V,Ks", R.CASES)
def test_logprobs_match_float64(dev, tol, V, Ks, pattern):
    from usdm_amd import ops
    x = R.case_row(V, pattern)
    xd = torch.from_numpy(x).to(dev)
    _, order, _ = R.reference(x)
    allowed = int(np.isfinite(x).sum())
    picks = [int(order[0]), int(order[allowed // 2]), int(order[allowed - 1])]     # arg-max, a mid-rank id, the least likely allowed id
    for K in Ks:
        o = _Out(dev)
        for t, tok in enumerate(picks):
            st, keep = _state(dev, [tok], [t + 1])
            ops.logprobs(xd, st, **o.kw(K))
            R.check_row(x, tok, *o.row(0, t, K), K, tol)
        lp, rk, ids, lps = o.row(0, 0, K)
        assert rk == 1 and (K == 0 or int(ids[0]) == picks[0])
        assert (o.tok_lp[0, len(picks):] == SENT_F).all() and (o.top_id[0, len(picks) * K:] == SENT_I).all()      # nothing past its rows


def test_edge_rows(dev):
    from usdm_amd import ops
    V, K = 777, 5
    # every id banned: the sampler falls back to id 0, which must be reported; -inf everywhere, no NaN
    x = torch.full((V,), float("-inf"), device=dev)
    o = _Out(dev)
    st, (nxt, out, stp, pos) = _state(dev, [99], [0])
    ops.sample_final(x, st, temperature=1.0, top_k=0, top_p=0.9, seed=3)
    ops.logprobs(x, st, **o.kw(K))
    lp, rk, ids, lps = o.row(0, 0, K)
    assert int(nxt.item()) == 0 and int(stp.item()) == 1
    assert lp == float("-inf") and rk == 1 and ids.tolist() == [0, 1, 2, 3, 4] and torch.isneginf(lps).all()
    # a single finite id: lp = 0 exactly, rank 1, and it leads the list
    x[500] = -3.25
    st, _ = _state(dev, [500], [2])
    ops.logprobs(x, st, **o.kw(K))
    lp, rk, ids, lps = o.row(0, 1, K)
    assert lp == 0.0 and rk == 1 and ids.tolist() == [500, 0, 1, 2, 3] and lps[0].item() == 0.0 and torch.isneginf(lps[1:]).all()
    # two exact ties at the maximum, the pick being the higher id: rank 1 (nothing is strictly greater), second in the list
    xr = R.bf16_row(V, 5)
    xr[[40, 600]] = xr.max() + 1.0
    st, _ = _state(dev, [600], [3])
    ops.logprobs(torch.from_numpy(xr).to(dev), st, **o.kw(K))
    lp, rk, ids, lps = o.row(0, 2, K)
    assert rk == 1 and ids[:2].tolist() == [40, 600] and lps[0].item() == lps[1].item() == lp
    R.check_row(xr, 600, lp, rk, ids, lps, K, R.kernel_tolerance())
    assert not any(torch.isnan(t).any() for t in (o.tok_lp, o.top_lp))


def _batch_rows(B, V):
    rows = np.stack([R.banned(R.bf16_row(V, 100 + b), R.BANS[b % 3]) for b in range(B)])
    if B > 3:
        rows[3] = -np.inf
    toks = [int(np.nanargmax(np.where(np.isfinite(r), r, -1e30))) if b % 2 else (b * 37) % V for b, r in enumerate(rows)]
    steps = [1 + (3 * b) % MAX_OUT for b in range(B)]
    return rows, toks, steps


@pytest.mark.parametrize("B", [1, 6, 16])
def test_batched_is_bit_identical_with_single(dev, tol, B):
    from usdm_amd import ops
    V, K = 42003, 20
    rows, toks, steps = _batch_rows(B, V)
    xd = torch.from_numpy(rows).to(dev)
    ob = _Out(dev, B)
    st, keep = _state(dev, toks, steps)
    ops.logprobs(xd[0] if B == 1 else xd, st, **ob.kw(K))
    os_ = _Out(dev, B)
    for b in range(B):
        st1, keep1 = _state(dev, [toks[b]], [steps[b]])
        ops.logprobs(xd[b], st1, K=K, tok_lp=os_.tok_lp[b], tok_rank=os_.tok_rank[b], top_id=os_.top_id[b], top_lp=os_.top_lp[b])
    for x, y in zip(ob.bits(), os_.bits()):
        assert torch.equal(x, y)
    for b in (0, B - 1):
        R.check_row(rows[b], toks[b], *ob.row(b, steps[b] - 1, K), K, tol)


@pytest.mark.parametrize("nseg", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 6])
def test_segmented_is_bit_identical_with_contiguous(dev, nseg, B):
    from usdm_amd import ops
    from usdm_amd.llm import vocab_shard
    V, K = 42003, 20
    Vloc = vocab_shard(V, 0, nseg)[0]
    rows, toks, steps = _batch_rows(B, V)
    seg = torch.randn(nseg, B, Vloc, generator=torch.Generator().manual_seed(nseg)) * 1e3      # finite junk in the padding slots too
    for s in range(nseg):
        n = min(V, (s + 1) * Vloc) - s * Vloc
        seg[s, :, :n] = torch.from_numpy(rows[:, s * Vloc:s * Vloc + n])
    xd, seg = torch.from_numpy(rows).to(dev), seg.to(dev)
    oc, og = _Out(dev, B), _Out(dev, B)
    st, keep = _state(dev, toks, steps)
    ops.logprobs(xd[0] if B == 1 else xd, st, **oc.kw(K))
    ops.logprobs(seg, st, V=V, nseg=nseg, seg_stride=B * Vloc, seg_len=Vloc, **og.kw(K))
    for x, y in zip(oc.bits(), og.bits()):
        assert torch.equal(x, y)
    assert not og.untouched()


def test_state_handling(dev, tol):
    """The row of the step whose pick sets the device-side `done` word is written; replays after it write nothing; a step at
    max_out writes nothing; two identical launches give identical bytes."""
    from usdm_amd import ops
    V, K = 1000, 5
    x = R.case_row(V, "range")
    xd = torch.from_numpy(x).to(dev)
    top = int(R.reference(x)[1][0])
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    eos = torch.tensor([1, 2, top, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)     # stop id = the greedy pick, at least 2 tokens
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    o = _Out(dev)
    st, (nxt, out, stp, pos) = _state(dev, [0], [0], done=done, eos=eos)
    plan = ops.Plan()
    ops.sample_final(xd, st, temperature=1.0, top_k=1, top_p=1.0, seed=0, plan=plan)
    ops.logprobs(xd, st, count=count, plan=plan, **o.kw(K))
    plan.run()
    assert int(done.item()) == 0
    plan.run()                                       # this pick sets `done`: its row must be there
    assert int(done.item()) == 1 and int(stp.item()) == 2 and int(count.item()) == 2
    for t in (0, 1):
        R.check_row(x, top, *o.row(0, t, K), K, tol)
    o.tok_lp[0, :2] = SENT_F; o.tok_rank[0, :2] = SENT_I; o.top_id[0, :2 * K] = SENT_I; o.top_lp[0, :2 * K] = SENT_F
    plan.run(); plan.run()                           # replays after the end: nothing is written, earlier rows stay
    assert o.untouched() and int(stp.item()) == 2 and int(count.item()) == 2
    # the library refuses a `done` state without the count (the final row could not be told from a replay)
    from usdm_amd._lib import UsdmError
    with pytest.raises(UsdmError, match="count"):
        ops.logprobs(xd, st, **o.kw(K))
    # step == max_out: the pick stores no token, and there is no row for it
    st2, (nxt2, out2, stp2, pos2) = _state(dev, [0], [MAX_OUT])
    ops.sample_final(xd, st2, temperature=1.0, top_k=1, top_p=1.0, seed=0)
    ops.logprobs(xd, st2, **o.kw(K))
    assert int(stp2.item()) == MAX_OUT + 1 and o.untouched()
    # two identical launches: identical bytes
    st3, keep3 = _state(dev, [top], [4])
    ops.logprobs(xd, st3, **o.kw(K))
    a = o.bits()
    o2 = _Out(dev)
    ops.logprobs(xd, st3, **o2.kw(K))
    for p, q in zip(a, o2.bits()):
        assert torch.equal(p, q)


def test_bad_arguments_are_refused_on_the_host(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError, lib
    x = torch.zeros(100, device=dev)
    o = _Out(dev)
    st, keep = _state(dev, [3], [1])
    for kw, msg in ((dict(o.kw(21)), "K must be 0 .. 20"), (dict(o.kw(5), V=0), "logits / V"),
                    (dict(o.kw(5), top_id=None), "top_id / top_lp missing")):
        with pytest.raises(UsdmError, match=msg):
            ops.logprobs(x, st, **kw)
        assert msg in lib.usdm_last_error().decode()
    assert o.untouched()
