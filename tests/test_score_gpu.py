"""usdm_prompt_logprobs / usdm_prompt_logprobs_seg through usdm_amd.ops: log-probability, rank and top-K list of GIVEN target ids over
chunks of logits rows, against the float64 reference of tests/_logprob_reference (torch.log_softmax in float64 plus a stable sort by
(-value, id)) on that module's rows, with its derived tolerance: ids and ranks exactly, values within kernel_tolerance().

Row r of a chunk is prompt row row0 + r; its target is ids[row0 + r + 1]; outputs are indexed by the target's row."""
import numpy as np
import pytest
import torch

from tests import _logprob_reference as R

pytestmark = pytest.mark.gpu

KMAX = 20
SENT_F, SENT_I = 12345.0, -7
N_IDS, ROW0, ROWS = 9, 2, 5


class _Out:
    """The four output buffers for n target rows, pre-filled with a sentinel."""

    def __init__(self, dev, n=N_IDS):
        self.n = n
        self.tok_lp = torch.full((n,), SENT_F, device=dev)
        self.tok_rank = torch.full((n,), SENT_I, dtype=torch.int32, device=dev)
        self.top_id = torch.full((n * KMAX,), SENT_I, dtype=torch.int32, device=dev)
        self.top_lp = torch.full((n * KMAX,), SENT_F, device=dev)

    def kw(self, K):
        return dict(K=K, tok_lp=self.tok_lp, tok_rank=self.tok_rank, top_id=self.top_id, top_lp=self.top_lp)

    def row(self, t, K):
        """(lp, rank, ids [K], lps [K]) of target row t, on the host"""
        torch.cuda.synchronize()
        ids = self.top_id[:self.n * K].view(self.n, K)[t].cpu() if K else torch.zeros(0)
        lps = self.top_lp[:self.n * K].view(self.n, K)[t].cpu() if K else torch.zeros(0)
        return self.tok_lp[t].item(), self.tok_rank[t].item(), ids, lps

    def untouched(self, K=KMAX, lo=0, hi=0):
        """every row outside lo .. hi-1 (and everything past the [n][K] area of the top lists) still holds the sentinel"""
        torch.cuda.synchronize()
        keep = torch.ones(self.n, dtype=torch.bool, device=self.tok_lp.device)
        keep[lo:hi] = False
        ok = bool((self.tok_lp[keep] == SENT_F).all() and (self.tok_rank[keep] == SENT_I).all())
        if K:
            ok = ok and bool((self.top_id[:self.n * K].view(self.n, K)[keep] == SENT_I).all() and (self.top_lp[:self.n * K].view(self.n, K)[keep] == SENT_F).all())
        return ok and bool((self.top_id[self.n * K:] == SENT_I).all() and (self.top_lp[self.n * K:] == SENT_F).all())

    def bits(self):
        torch.cuda.synchronize()
        return [t.clone().view(torch.int32) for t in (self.tok_lp, self.tok_rank, self.top_id, self.top_lp)]


@pytest.fixture(scope="module")
def tol():
    return R.kernel_tolerance()


def _rows_and_targets(V):
    """5 rows with mixed ban patterns and their targets: the arg-max id, a banned (-inf) id, an id tied with others, id V - 1, and a
    mid-rank id.  Row 2 holds an exact three-way tie; its target is the highest of the tied ids."""
    patterns = ("none", "range", "none", "all_but_one", "range")
    rows = np.stack([R.banned(R.bf16_row(V, 7 * V + 1 + r), p) for r, p in enumerate(patterns)])      # (row 0 is R.case_row(V, "none"))
    tie_ids = sorted({1, V // 2, V - 2})
    rows[2][tie_ids] = np.float32(0.5)
    assert len(tie_ids) == 3 and np.isneginf(rows[1]).any() and np.isneginf(rows[3][V - 1])
    allowed = int(np.isfinite(rows[4]).sum())
    targets = [int(np.argmax(rows[0])), int(np.flatnonzero(np.isneginf(rows[1]))[0]), tie_ids[-1], V - 1,
               int(R.reference(rows[4])[1][allowed // 2])]
    return rows, targets


def _prompt(dev, targets, fill=0):
    """a 9-id prompt whose ids ROW0 + 1 .. ROW0 + ROWS are the rows' targets"""
    ids = [fill] * N_IDS
    ids[ROW0 + 1:ROW0 + 1 + ROWS] = targets
    return torch.tensor(ids, dtype=torch.int64, device=dev)


@pytest.mark.parametrize("V,Ks", R.CASES)
def test_rows_match_float64(dev, tol, V, Ks):
    from usdm_amd import ops
    rows, targets = _rows_and_targets(V)
    chunk = torch.full((ROWS, V + 3), float("nan"), device=dev)          # logits_bs = V + 3; the gap is never read
    chunk[:, :V] = torch.from_numpy(rows).to(dev)
    ids = _prompt(dev, targets)
    for K in Ks:
        o = _Out(dev)
        ops.prompt_logprobs(chunk[:, :V], ids, row0=ROW0, **o.kw(K))
        for r in range(ROWS):
            R.check_row(rows[r], targets[r], *o.row(ROW0 + 1 + r, K), K, tol)
        assert o.untouched(K, ROW0 + 1, ROW0 + 1 + ROWS)                   # nothing outside its rows
        lp, rk, _, _ = o.row(ROW0 + 1, K)
        assert rk == 1                                                     # the arg-max target
        assert o.row(ROW0 + 2, K)[0] == float("-inf")                      # the banned target: -inf, not NaN
        assert not any(torch.isnan(t).any() for t in (o.tok_lp, o.top_lp))


def _decode_state(dev, tok):
    from usdm_amd import ops
    nxt = torch.tensor([tok], dtype=torch.int32, device=dev)
    stp = torch.ones(1, dtype=torch.int32, device=dev)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros(N_IDS, dtype=torch.int32, device=dev)
    return ops.decode_state(nxt, out, stp, pos), (nxt, stp, pos, out)


@pytest.mark.parametrize("V,K", [(42003, 20), (1000, 5), (7, 20)])
def test_same_bits_as_the_decode_kernel(dev, V, K):
    """the same row and target through usdm_logprobs (decode state: next_token = target, step = 1 -> row 0) and through
    usdm_prompt_logprobs (a one-row chunk, target row 1): the same bits in all four outputs"""
    from usdm_amd import ops
    rows, targets = _rows_and_targets(V)
    for r in range(ROWS):
        x = torch.from_numpy(rows[r]).to(dev)
        od, op = _Out(dev), _Out(dev)
        st, keep = _decode_state(dev, targets[r])
        ops.logprobs(x, st, **od.kw(K))
        ops.prompt_logprobs(x, torch.tensor([0, targets[r]], dtype=torch.int64, device=dev), row0=0, **op.kw(K))
        torch.cuda.synchronize()
        assert od.tok_lp[0].view(torch.int32) == op.tok_lp[1].view(torch.int32) and od.tok_rank[0] == op.tok_rank[1]
        assert torch.equal(od.top_id[:K], op.top_id[K:2 * K]) and torch.equal(od.top_lp[:K].view(torch.int32), op.top_lp[K:2 * K].view(torch.int32))
    # an id outside [0, V): both report lp = -inf and the rank of -inf
    x = torch.from_numpy(rows[0]).to(dev)
    od, op = _Out(dev), _Out(dev)
    st, keep = _decode_state(dev, V + 5)
    ops.logprobs(x, st, **od.kw(K))
    ops.prompt_logprobs(x, torch.tensor([0, V + 5], dtype=torch.int64, device=dev), row0=0, **op.kw(K))
    o2 = _Out(dev)
    ops.prompt_logprobs(x, torch.tensor([0, -(2 ** 40)], dtype=torch.int64, device=dev), row0=0, **o2.kw(K))      # (not truncated to 32 bits)
    torch.cuda.synchronize()
    assert od.tok_lp[0].item() == op.tok_lp[1].item() == o2.tok_lp[1].item() == float("-inf")
    assert od.tok_rank[0].item() == op.tok_rank[1].item() == o2.tok_rank[1].item() == 1 + int(np.isfinite(rows[0]).sum())


def test_empty_row_gives_minus_infinity_not_nan(dev):
    from usdm_amd import ops
    V, K = 777, 5
    x = torch.full((2, V), float("-inf"), device=dev)
    x[1, 500] = -3.25                                        # row 1: a single finite id
    o = _Out(dev, 3)
    ops.prompt_logprobs(x, torch.tensor([0, 99, 500], dtype=torch.int64, device=dev), row0=0, **o.kw(K))
    lp, rk, ids, lps = o.row(1, K)
    assert lp == float("-inf") and rk == 1 and ids.tolist() == [0, 1, 2, 3, 4] and torch.isneginf(lps).all()
    lp, rk, ids, lps = o.row(2, K)
    assert lp == 0.0 and rk == 1 and ids.tolist() == [500, 0, 1, 2, 3] and lps[0].item() == 0.0 and torch.isneginf(lps[1:]).all()
    assert not any(torch.isnan(t).any() for t in (o.tok_lp, o.top_lp))


def test_segmented_is_bit_identical_with_contiguous(dev):
    """V = 1003 as 2 segments of 502 ids (the vocab-parallel lm_head of two ranks), 3 rows; the padding slot past V is NaN"""
    from usdm_amd import ops
    V, K, nseg, slen, rows_n = 1003, 20, 2, 502, 3
    rows = np.stack([R.banned(R.bf16_row(V, 50 + r), R.BANS[r]) for r in range(rows_n)])
    targets = [int(np.argmax(rows[0])), 700, V - 1]
    ids = torch.tensor([5] + targets + [6], dtype=torch.int64, device=dev)
    seg = torch.full((nseg, rows_n, slen), float("nan"))
    for s in range(nseg):
        n = min(V, (s + 1) * slen) - s * slen
        seg[s, :, :n] = torch.from_numpy(rows[:, s * slen:s * slen + n])
    oc, og = _Out(dev, 5), _Out(dev, 5)
    ops.prompt_logprobs(torch.from_numpy(rows).to(dev), ids, row0=0, **oc.kw(K))
    ops.prompt_logprobs(seg.to(dev), ids, row0=0, V=V, nseg=nseg, seg_stride=rows_n * slen, seg_len=slen, **og.kw(K))
    for x, y in zip(oc.bits(), og.bits()):
        assert torch.equal(x, y)
    assert not og.untouched() and og.untouched(K, 1, 4)
    for r in range(rows_n):
        R.check_row(rows[r], targets[r], *og.row(1 + r, K), K, R.kernel_tolerance())


def test_two_runs_are_bit_identical(dev):
    from usdm_amd import ops
    V, K = 42003, 20
    rows, targets = _rows_and_targets(V)
    chunk, ids = torch.from_numpy(rows).to(dev), _prompt(dev, targets)
    a, b = _Out(dev), _Out(dev)
    ops.prompt_logprobs(chunk, ids, row0=ROW0, **a.kw(K))
    ops.prompt_logprobs(chunk, ids, row0=ROW0, **b.kw(K))
    for x, y in zip(a.bits(), b.bits()):
        assert torch.equal(x, y)


def test_bad_arguments_are_refused_on_the_host(dev):
    from usdm_amd import ops
    from usdm_amd._lib import UsdmError, lib
    x = torch.zeros(ROWS, 100, device=dev)
    ids = torch.zeros(N_IDS, dtype=torch.int64, device=dev)
    o = _Out(dev)
    for kw, msg in ((dict(o.kw(21), row0=ROW0), "K must be 0 .. 20"), (dict(o.kw(5), row0=ROW0 + 2), "n_ids"),
                    (dict(o.kw(5), row0=ROW0, V=101), None), (dict(o.kw(5), row0=ROW0, top_lp=None), "top_id / top_lp missing"),
                    (dict(o.kw(5), row0=ROW0, tok_lp=None), "tok_lp / tok_rank missing")):
        if msg is None:      # logits_bs < V: the wrapper already refuses a row shorter than V ...
            with pytest.raises(ValueError, match="logits"):
                ops.prompt_logprobs(x, ids, **kw)
            continue
        with pytest.raises(UsdmError, match=msg):
            ops.prompt_logprobs(x, ids, **kw)
        assert msg in lib.usdm_last_error().decode()
    # ... and the library refuses it by return code
    from usdm_amd import _lib
    import ctypes as C
    a = _lib.PromptLogprobArgs(logits=x.data_ptr(), V=100, K=5, logits_bs=99, ids=ids.data_ptr(), n_ids=N_IDS, row0=ROW0, rows=ROWS,
                               tok_lp=o.tok_lp.data_ptr(), tok_rank=o.tok_rank.data_ptr(), top_id=o.top_id.data_ptr(), top_lp=o.top_lp.data_ptr())
    assert lib.usdm_prompt_logprobs(C.byref(a), None) == 2 and "logits_bs" in lib.usdm_last_error().decode()
    assert o.untouched()
