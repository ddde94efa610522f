"""usdm_penalize / usdm_penalize_seg through usdm_amd.ops against the numpy float32 restatement (tests/_penalty_reference.py): the
penalised row and the table after the launch are compared as int32 bit patterns.  The kernel runs BEFORE the pick of step `step`: it
first counts out_tokens[step - 1], then penalises the row."""
import numpy as np
import pytest
import torch

from tests import _penalty_reference as P

pytestmark = pytest.mark.gpu

MAX_OUT = 48
KNOBS = [(1.3, 0.7, -0.5), (1.0, 0.0, 0.0), (0.8, -2.0, 2.0), (2.0, 0.0, 0.0), (1.0, 1.5, 0.0), (1.0, 0.0, -1.25)]     # (r, f, p); [1] is neutral
SENT = 12345.0


def _knobs(b):
    return KNOBS[b % len(KNOBS)]


def _case(V, B, seed):
    """B sequences: rows, prompts, output histories (the last id of each history is the one the launch has to count)"""
    rows = np.stack([P.bf16_row(V, seed + 7 * b) for b in range(B)])
    hist = [P.history(V, seed + 100 + b, n_out=20 + b) for b in range(B)]
    return rows, [h[0] for h in hist], [h[1] for h in hist]


class _Dev:
    """Decode state, tables (holding everything but the last output id), knobs and count words of B sequences on the device"""

    def __init__(self, dev, V, prompts, outs, count=None, done=None, table_pad=0):
        from usdm_amd import ops
        B = self.B = len(prompts)
        self.out = torch.zeros(B, MAX_OUT, dtype=torch.int32, device=dev)
        for b, o in enumerate(outs):
            self.out[b, :len(o)] = torch.from_numpy(np.asarray(o)).to(dev, torch.int32)
        self.step = torch.tensor([len(o) for o in outs], dtype=torch.int32, device=dev)
        self.nxt, self.pos = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        self.table = torch.full((B, V + table_pad), -1, dtype=torch.int32, device=dev)
        for b in range(B):
            self.table[b, :V] = torch.from_numpy(P.table(V, prompts[b], outs[b][:-1])).to(dev)
        self.params = ops.penalty_params_tensor(dev, B).view(B, -1)
        for b in range(B):
            ops.set_penalty_params(self.params[b], *_knobs(b))
        self.count = None if count is None else torch.tensor(count, dtype=torch.int32, device=dev)
        self.done = None if done is None else torch.tensor(done, dtype=torch.int32, device=dev)
        one = B == 1
        self.eos = None if done is None else torch.zeros(8, dtype=torch.int32, device=dev)
        self.st = ops.decode_state(self.nxt, self.out[0] if one else self.out, self.step, self.pos, batch=0 if one else B, done=self.done,
                                   eos=self.eos)
        self.kw = dict(table=self.table[0, :V] if one else self.table, dev_params=self.params[0] if one else self.params, count=self.count)


def _want(V, rows, prompts, outs):
    tbls = [P.table(V, p, o) for p, o in zip(prompts, outs)]
    return np.stack([P.penalize_table(rows[b], tbls[b], *_knobs(b)) for b in range(len(tbls))]), np.stack(tbls)


@pytest.mark.parametrize("B", [1, 4, 16])
@pytest.mark.parametrize("V", [1000, 32003])
def test_row_and_table_match_the_reference_bit_for_bit(dev, V, B):
    from usdm_amd import ops
    rows, prompts, outs = _case(V, B, 3 * V + B)
    d = _Dev(dev, V, prompts, outs, count=[len(o) - 1 for o in outs] if B == 1 else None, table_pad=5 if B > 1 else 0)
    x = torch.from_numpy(rows).to(dev)
    ops.penalize(x[0] if B == 1 else x, d.st, **d.kw)
    torch.cuda.synchronize()
    want_rows, want_tbl = _want(V, rows, prompts, outs)
    assert np.array_equal(P.bits(x.cpu().numpy()), P.bits(want_rows))
    assert np.array_equal(d.table[:, :V].cpu().numpy(), want_tbl) and bool((d.table[:, V:] == -1).all())
    if B > 1:       # the neutral slot: every bit of its row stays, its token is still counted
        assert _knobs(1) == (1.0, 0.0, 0.0) and np.array_equal(P.bits(x[1].cpu().numpy()), P.bits(rows[1]))
        assert not np.array_equal(P.bits(x[0].cpu().numpy()), P.bits(rows[0]))
    else:
        assert int(d.count.item()) == len(outs[0])


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("nseg", [2, 3])
def test_segmented_form_equals_the_contiguous_call(dev, nseg, B):
    from usdm_amd import ops
    V = 32003
    seg_len = -(-V // nseg) + 37            # the last segment is only partly inside V
    assert (nseg - 1) * seg_len < V < nseg * seg_len
    rows, prompts, outs = _case(V, B, 11 * nseg + B)
    want_rows, want_tbl = _want(V, rows, prompts, outs)
    # [nseg][B][seg_len], padding slots (ids >= V) filled with a sentinel
    pad = np.full((B, nseg * seg_len), SENT, dtype=np.float32)
    pad[:, :V] = rows
    seg = torch.from_numpy(np.ascontiguousarray(pad.reshape(B, nseg, seg_len).transpose(1, 0, 2))).to(dev)
    d = _Dev(dev, V, prompts, outs)
    if B == 1:
        ops.penalize(seg.view(-1), d.st, V=V, **d.kw)      # one sequence: the gathered row is contiguous
    else:
        ops.penalize(seg, d.st, V=V, nseg=nseg, seg_stride=B * seg_len, seg_len=seg_len, **d.kw)
    torch.cuda.synchronize()
    got = seg.cpu().numpy().transpose(1, 0, 2).reshape(B, nseg * seg_len)
    assert np.array_equal(P.bits(got[:, :V]), P.bits(want_rows)) and bool((got[:, V:] == SENT).all())
    assert np.array_equal(d.table[:, :V].cpu().numpy(), want_tbl)
    # the segmented form on ONE sequence as well (nseg segments of one row)
    d1 = _Dev(dev, V, prompts[:1], outs[:1])
    seg1 = torch.from_numpy(pad[:1].reshape(nseg, 1, seg_len).copy()).to(dev)
    ops.penalize(seg1, d1.st, V=V, nseg=nseg, seg_stride=seg_len, seg_len=seg_len, **d1.kw)
    torch.cuda.synchronize()
    got1 = seg1.cpu().numpy().reshape(-1)
    assert np.array_equal(P.bits(got1[:V]), P.bits(want_rows[0])) and bool((got1[V:] == SENT).all())
    assert np.array_equal(d1.table[0, :V].cpu().numpy(), want_tbl[0])


def test_counting_over_six_steps_replays_and_done(dev):
    """out_tokens / step set as the sampler would: after each launch the table is the histogram of out[0 .. step - 1] plus the prompt
    flags; a replay at the same step changes neither table nor count; done = 1 leaves row, table and count alone; step 0 counts nothing."""
    from usdm_amd import ops
    V = 1000
    row = P.bf16_row(V, 21)
    prompt = np.array([5, 9, 9, 700, 999])
    picks = [17, 5, 17, 999, 17, 0]
    d = _Dev(dev, V, [prompt], [np.array([0])], count=[0], done=[0])      # (the history is overwritten below)
    d.table[0, :V] = torch.from_numpy(P.table(V, prompt, [])).to(dev)
    d.out.zero_()
    knobs = _knobs(0)
    for step in range(len(picks) + 1):
        d.step.fill_(step)
        if step:
            d.out[0, step - 1] = picks[step - 1]
        for replay in range(2):
            x = torch.from_numpy(row).to(dev)
            ops.penalize(x, d.st, **d.kw)
            torch.cuda.synchronize()
            want_tbl = P.table(V, prompt, picks[:step])
            assert np.array_equal(d.table[0].cpu().numpy(), want_tbl), (step, replay)
            assert int(d.count.item()) == step
            assert np.array_equal(P.bits(x.cpu().numpy()), P.bits(P.penalize_table(row, want_tbl, *knobs))), (step, replay)
    assert int(d.table[0, 17].item()) == 3 and int(d.table[0, 5].item()) == P.PROMPT_BIT + 1 and int(d.table[0, 9].item()) == P.PROMPT_BIT
    # device-side end of sequence: one more token in out_tokens, but done is set - nothing moves
    d.out[0, 6] = 123
    d.step.fill_(7)
    d.done.fill_(1)
    before = d.table.clone()
    x = torch.from_numpy(row).to(dev)
    ops.penalize(x, d.st, **d.kw)
    torch.cuda.synchronize()
    assert torch.equal(d.table, before) and int(d.count.item()) == 6 and np.array_equal(P.bits(x.cpu().numpy()), P.bits(row))


def test_batch_form_without_count_counts_at_every_launch(dev):
    from usdm_amd import ops
    V, B = 1000, 4
    rows, prompts, outs = _case(V, B, 77)
    d = _Dev(dev, V, prompts, outs)
    d.step[2] = 0                                    # a freshly admitted slot: nothing to count
    x = torch.from_numpy(rows).to(dev)
    for n in (1, 2):
        ops.penalize(x, d.st, **d.kw)
        torch.cuda.synchronize()
        for b in range(B):
            want = P.table(V, prompts[b], outs[b][:-1])
            if b != 2:
                want[outs[b][-1]] += n               # no count word: every launch counts out[step - 1] again
            assert np.array_equal(d.table[b].cpu().numpy(), want), (n, b)


def test_ops_refuses_what_the_library_would_misread(dev):
    from usdm_amd import _lib, ops
    V = 1000
    rows, prompts, outs = _case(V, 1, 5)
    d = _Dev(dev, V, prompts, outs, done=[0])        # a `done` word but no count
    x = torch.from_numpy(rows[0]).to(dev)
    with pytest.raises(_lib.UsdmError, match="done"):
        ops.penalize(x, d.st, **d.kw)
    d = _Dev(dev, V, prompts, outs)
    with pytest.raises(ValueError, match="table"):
        ops.penalize(x, d.st, table=d.table[0, :V - 1], dev_params=d.params[0])
    with pytest.raises(ValueError, match="float32"):
        ops.penalize(x.double(), d.st, **d.kw)
    torch.cuda.synchronize()
    assert np.array_equal(P.bits(x.cpu().numpy()), P.bits(rows[0]))
