"""GPU: the two pieces of code that end every decode step, launched alone through their usdm_amd.ops wrappers and compared word for
word with the plain reference of tests/_pick_reference.py (checked itself by tests/test_pick_cpu.py): the greedy pick over the
lm_head's partials (argmax_final_kernel, csrc/llm_k.hip) and the commit of the token to the device-side decode state (pick_commit and
pick_embed_row, csrc/pick_commit.h) through the greedy and the sampling entry points.

Every comparison is between integers or bit patterns; no test leaves a case out.  Every buffer a kernel may write is longer than what
it owns and pre-filled with a sentinel (int32 0x5a5a5a5a, bf16 / f32 bits 0x7f7f / 0x7f7f7f7f) that must survive bit for bit;
out_tokens is passed as a view of the first max_out (B * max_out) words of such a buffer.  Every input gap (between segments, behind
the last sequence's partials, a logits row's padding) holds (+inf, id -1), which would win if it were read; the eos words behind the
ids in use hold the token itself, a hit if they were read.  Row t of the embedding table spells t in its 16 elements, so a copied row
names the token it was copied from.

Entry point -> test
  usdm_argmax_final        test_pick_single, test_pick_batched[plain], test_commit[argmax], test_embed_row_widths, test_replay
  usdm_argmax_final_seg    test_pick_segmented, test_pick_batched[seg], test_commit[argmax_seg]
  usdm_sample_final        test_commit[sample], test_sampled_commit, test_embed_row_widths
  usdm_sample_final_seg    test_commit[sample_seg]

Where nparts has no such position a placement is not built (one partial has no partner to tie with, 63 partials have no second wave);
tests/test_pick_cpu.py::test_pick_cases_place_what_they_promise checks what is built at every size.

Breaks tried locally, never committed, and the tests that caught each:
  pick_better's tie rule flipped to the higher id          every id of test_pick_single and test_pick_segmented (36): the ties, the
                                                           +0.0 / -0.0 pair and "a real (-inf, 5) among no candidates" (token 0)
  pick_commit: `step + 1 >= mn` -> `step >= mn`            test_commit, all four ids ("hit at step 0, min_new 1": done stays 0)
  pick_commit: EOS loop bound `i < 6` -> `i < 5`           test_commit, all four ids ("n_eos 6, hit at the sixth": done stays 0)
(The sampler's top_k = 1 pick is a scan in index order, not pick_better: the first break leaves test_commit[sample*] passing.)

Measured on an MI355X: the 60 ids take 2.8 s together; the slowest is test_pick_segmented[1003-*] with 0.08 s (about 200 launches of
up to 8 x 1003 partials), behind the one id that pays for the first launch of the process (0.18 s).
"""
import functools

import numpy as np
import pytest
import torch

from tests import _pick_reference as R

pytestmark = pytest.mark.gpu
HD = 16       # embedding row: E[t][c] = bit c of t
PAD = 5       # sentinel words behind every state array
BF_SENT = 0x7F7F


# ------------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _table(dev, rows):
    assert rows <= 1 << HD
    return ((torch.arange(rows)[:, None] >> torch.arange(HD)[None]) & 1).to(torch.bfloat16).contiguous().to(dev)


def _words(dev, vals, pad=PAD):
    """int32 device words: vals, then `pad` sentinel words"""
    return torch.tensor(list(vals) + [R.SENT] * pad, dtype=torch.int32, device=dev)


class Dev:
    """the device side of a host state: every array with sentinel words behind it, h_out with a sentinel row behind it"""

    def __init__(self, dev, s, Hd=HD, table=None):
        from usdm_amd import ops
        B, mo = s["B"], s["max_out"]
        self.s, self.B, self.Hd = s, B, Hd
        self.nxt, self.step, self.pos = _words(dev, s["next_token"]), _words(dev, s["step"]), _words(dev, s["pos"])
        self.out = _words(dev, [w for row in s["out_tokens"] for w in row])
        self.done = None if s["done"] is None else _words(dev, s["done"])
        self.eos = None if s["eos"] is None else _words(dev, s["eos"], 0)
        self.h = torch.full((B + 1, Hd), BF_SENT, dtype=torch.int16, device=dev).view(torch.bfloat16)
        self.E = _table(dev, R.PICK_V + s["id_offset"]) if table is None else table
        out_view = self.out[:mo] if B == 1 else self.out[:B * mo].view(B, mo)
        self.st = ops.decode_state(self.nxt, out_view, self.step, self.pos, id_offset=s["id_offset"], advance_pos=bool(s["advance_pos"]),
                                   batch=B if B > 1 else 0, done=self.done, eos=self.eos)
        assert self.st.max_out == mo
        self.embed = dict(embed=self.E, h_out=self.h, Hd=Hd)

    def read(self, what):
        """-> the state in the reference's form, after asserting that every sentinel survived"""
        torch.cuda.synchronize()
        B, mo, s = self.B, self.s["max_out"], self.s
        got = {}
        for k, t, n in (("next_token", self.nxt, B), ("out_tokens", self.out, B * mo), ("step", self.step, B), ("pos", self.pos, B), ("done", self.done, B)):
            if t is None:
                got[k] = None
                continue
            w = t.cpu().tolist()
            assert w[n:] == [R.SENT] * PAD, f"{what}: {k} written behind its {n} words: {w[n:]}"
            got[k] = w[:n]
        got["out_tokens"] = [got["out_tokens"][b * mo:(b + 1) * mo] for b in range(B)]
        if self.eos is not None:
            assert self.eos.cpu().tolist() == s["eos"], f"{what}: eos is an input"
        h = self.h.cpu()
        bits = h.view(torch.int16)
        assert bool((bits[B] == BF_SENT).all()), f"{what}: h_out written behind its {B} rows"
        self.h_rows = h[:B]
        got["rows"] = []
        for b in range(B):
            if bool((bits[b] == BF_SENT).all()):
                got["rows"].append(None)
            elif self.Hd == HD:
                f = h[b].float()
                assert bool(((f == 0) | (f == 1)).all()), f"{what}: h_out[{b}] is no row of the table: {f.tolist()}"
                got["rows"].append(int((f.long() << torch.arange(HD)).sum()))
            else:
                got["rows"].append("row")
        return got


def _same(what, got, ref):
    for k in ("next_token", "out_tokens", "step", "pos", "done", "rows"):
        assert got[k] == ref[k], f"{what}: {k} = {got[k]}, expected {ref[k]}"


def _argmax(dev, s, vals, ids, what, gap=0, seg=False, plan=None, **dkw):
    """one usdm_argmax_final(_seg) launch on the partials vals / ids [nseg][B][nparts] -> (Dev, the expected state)"""
    from usdm_amd import ops
    nseg, B, nparts = vals.shape
    assert B == s["B"] and (nseg == 1 or seg)
    pv, pi, ss = R.lay_out(vals, ids, gap)
    d = Dev(dev, s, **dkw)
    d.pv, d.pi = torch.from_numpy(pv).to(dev), torch.from_numpy(pi).to(dev)
    toks = [R.pick_ref(vals[:, b], ids[:, b]) for b in range(B)]
    assert all(0 <= t and t + s["id_offset"] < d.E.shape[0] for t in toks), what
    if seg and nseg == 1:      # (ops.argmax_final takes nseg = 1 to the plain entry point)
        from usdm_amd import _lib
        import ctypes as C
        _lib.check(_lib.lib.usdm_argmax_final_seg(C.c_void_p(d.pv.data_ptr()), C.c_void_p(d.pi.data_ptr()), C.c_int32(nparts), C.c_int32(1), C.c_int64(0),
                                                  C.byref(d.st), C.c_void_p(d.E.data_ptr()), C.c_int32(d.Hd), C.c_void_p(d.h.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "usdm_argmax_final_seg")
    else:
        ops.argmax_final(d.pv, d.pi, nparts, d.st, nseg=nseg, seg_stride=ss if nseg > 1 else 0, plan=plan, **d.embed)
    return d, R.expected(s, toks)


def _sample(dev, s, x, what, seg=False, params=None, **dkw):
    """one usdm_sample_final(_seg) launch on the logits x [B][V] -> (Dev, probs_out [B][V] and the words behind it).  params: B x
    (temperature, top_k, top_p, seed); the batched form reads them from the device.  The contiguous rows are V + 5 apart; the
    segmented row is cut into two segments of 32 ids with one more row per segment, and all of that padding is +inf."""
    from usdm_amd import ops
    B, V = x.shape
    d = Dev(dev, s, **dkw)
    if seg:
        sl, nseg = 32, -(-V // 32)
        lg = np.full((nseg, B + 1, sl), R.POISON_V, np.float32)
        for k in range(nseg):
            lg[k, :B, :min(sl, V - k * sl)] = x[:, k * sl:(k + 1) * sl]
        kw = dict(V=V, nseg=nseg, seg_stride=(B + 1) * sl, seg_len=sl)
    else:
        lg = np.full((B, V + 5), R.POISON_V, np.float32)
        lg[:, :V] = x
        kw = dict(V=V)
        if B == 1:
            lg = lg[0]
    d.lg = torch.from_numpy(lg).to(dev)
    d.probs = torch.full((B * V + 16,), 0x7F7F7F7F, dtype=torch.int32, device=dev).view(torch.float32)
    if B > 1:
        d.params = ops.sample_params_tensor(dev, B)
        for b, (T, k, p, seed) in enumerate(params):
            ops.set_sample_params(d.params[b], T, k, p, seed)
        kw.update(dev_params=d.params)
    else:
        T, k, p, seed = params[0]
        kw.update(temperature=T, top_k=k, top_p=p, seed=seed)
    ops.sample_final(d.lg, d.st, probs_out=d.probs, **kw, **d.embed)
    return d


def _probs_rows(d, V, what):
    """-> per sequence: was its probs_out row written?  (asserting that a row is written whole or not at all, and nothing behind:
    probs_out is [B][V] also where the logits rows are further apart than V)"""
    torch.cuda.synchronize()
    w = d.probs.view(torch.int32).cpu() != 0x7F7F7F7F
    assert not bool(w[d.B * V:].any()), f"{what}: probs_out written behind its {d.B} rows"
    rows = w[:d.B * V].view(d.B, V)
    assert bool((rows.all(1) | ~rows.any(1)).all()), f"{what}: a probs_out row written in part"
    return rows.all(1).tolist()


# ------------------------------------------------------------------------------------------------------------------ a. the pick
@pytest.mark.parametrize("off", R.OFFSETS)
@pytest.mark.parametrize("nparts", R.PICK_NPARTS)
def test_pick_single(dev, nparts, off):
    """usdm_argmax_final on one sequence: every placement of _pick_reference.pick_cases == pick_ref, the token carries id_offset and
    h_out is the table's row of that token (all no-candidate: token id_offset and its row)"""
    for name, v, i in R.pick_cases(nparts):
        what = f"nparts {nparts}, id_offset {off}, {name}"
        s = R.state(1, step=2, id_offset=off)
        d, ref = _argmax(dev, s, v[:, None], i[:, None], what)
        _same(what, d.read(what), ref)
        assert ref["rows"] == [R.pick_ref(v, i) + off] == ref["next_token"]


@pytest.mark.parametrize("off", R.OFFSETS)
@pytest.mark.parametrize("nparts", R.PICK_NPARTS)
def test_pick_segmented(dev, nparts, off):
    """usdm_argmax_final_seg, nseg in {2, 8} (and 1, which the plain entry point forwards), seg_stride = nparts and nparts + 5 with
    poison in the gap: the same placements with the winner in the first, a middle and the last segment, the tie's partners in later
    segments"""
    for nseg in (1, 2, 8):
        for gap in ((0, 5) if nseg > 1 else (0,)):
            for name, v, i in R.pick_cases(nparts, nseg):
                what = f"nparts {nparts}, nseg {nseg}, gap {gap}, id_offset {off}, {name}"
                d, ref = _argmax(dev, R.state(1, step=2, id_offset=off), v[:, None], i[:, None], what, gap=gap, seg=True)
                _same(what, d.read(what), ref)


@pytest.mark.parametrize("form", ["plain", "seg"])
@pytest.mark.parametrize("nparts", [67, 300])
@pytest.mark.parametrize("B", [2, 5, 16, 64])
def test_pick_batched(dev, B, nparts, form):
    """the batched form (one workgroup per sequence), plain and with nseg = 2 (seg_stride = B * nparts + 5): every sequence has a winner
    and a position of its own; b = 1 and b = B - 1 are done beforehand and keep every word, their h_out row included"""
    nseg = 2 if form == "seg" else 1
    v, i = R.batch_case(B, nparts, nseg)
    done = [int(b in (1, B - 1)) for b in range(B)]
    s = R.state(B, step=[b % 11 for b in range(B)], pos=[7 + 2 * b for b in range(B)], done=done, id_offset=32002)
    what = f"B {B}, nparts {nparts}, {form}"
    d, ref = _argmax(dev, s, v, i, what, gap=5 if nseg > 1 else 0, seg=nseg > 1)
    assert ref["rows"] == [None if done[b] else R.ID0 + b + 32002 for b in range(B)] and ref["step"][1] == s["step"][1]
    _same(what, d.read(what), ref)


# ------------------------------------------------------------------------------------------------------------------ b. the commit
ENTRIES = ("argmax", "argmax_seg", "sample", "sample_seg")


def _commit_launch(dev, entry, s, toks, what):
    """the launch of `entry` in which sequence b picks raw id toks[b] -> (the state read back, the expected state, Dev)"""
    if entry.startswith("argmax"):
        nseg = 2 if entry == "argmax_seg" else 1
        v, i = R.parts_for(toks, nseg=nseg)
        d, ref = _argmax(dev, s, v, i, what, gap=5 if nseg > 1 else 0, seg=nseg > 1)
        return d.read(what), ref, d
    x = R.logits_for(toks)
    d = _sample(dev, s, x, what, seg=entry == "sample_seg", params=[(1.0, 1, 1.0, 5)] * len(toks))
    return d.read(what), R.expected(s, toks), d


@pytest.mark.parametrize("entry", ENTRIES)
def test_commit(dev, entry):
    """the case table of _pick_reference.commit_cases (step at and past max_out, advance_pos, up to six EOS ids and a seventh, min_new,
    null done / eos, id_offset) and the B = 5 batch through usdm_argmax_final(_seg), whose partials encode the token, and
    usdm_sample_final(_seg) with top_k = 1, whose logits have the token as the lowest id of a three-way exact maximum: == commit_ref"""
    for name, tok, s in R.commit_cases():
        what = f"{entry}, {name}"
        got, ref, d = _commit_launch(dev, entry, s, [tok], what)
        _same(what, got, ref)
        if entry.startswith("sample"):
            assert _probs_rows(d, R.COMMIT_V, what) == [True]
    toks, s = R.commit_batch_case()
    what = f"{entry}, batched"
    got, ref, d = _commit_launch(dev, entry, s, toks, what)
    _same(what, got, ref)
    if entry.startswith("sample"):
        assert _probs_rows(d, R.COMMIT_V, what) == [True, True, False, True, True], "the done sequence's probs_out row"


# ------------------------------------------------------------------------------------------------------------------ c. the sampled commit
def test_sampled_commit(dev):
    """usdm_sample_final, top_k = 0, top_p = 0.9, V = 517, B = 3 with dev_params per sequence: the token is the oracle's for (the
    sequence's seed, the sequence's own step) - one step is past max_out - and the state follows commit_ref; sequence 1 draws its EOS
    id (the oracle's token, put into eos)"""
    c = R.SAMPLED
    x, toks, s = R.sampled_case()
    d = _sample(dev, s, x, "sampled", params=[(1.0, 0, c["top_p"], seed) for seed in c["seeds"]], table=_table(dev, c["V"] + c["off"]))
    ref = R.expected(s, toks)
    assert ref["done"] == [0, 1, 0] and ref["out_tokens"][2] == s["out_tokens"][2]
    _same("sampled", d.read("sampled"), ref)
    assert _probs_rows(d, c["V"], "sampled") == [True] * 3


# ------------------------------------------------------------------------------------------------------------------ d. replay
def test_replay(dev):
    """an ops.Plan of one usdm_argmax_final run four times on fixed partials with max_out = 3: step 0 -> 4, the token stored three
    times, the word behind out_tokens still the sentinel, pos advanced four times"""
    from usdm_amd import ops
    v, i = R.parts_for([23])
    s = R.state(1, max_out=3, step=0, pos=7)
    plan = ops.Plan()
    d, ref = _argmax(dev, s, v, i, "replay", plan=plan)
    assert len(plan) == 1
    for _ in range(3):
        ref = R.expected(ref, [23])
    for _ in range(4):
        plan.run()
    got = d.read("replay")
    _same("replay", got, ref)
    assert got["step"] == [4] and got["pos"] == [11] and got["out_tokens"] == [[23, 23, 23]] and got["rows"] == [23]


# ------------------------------------------------------------------------------------------------------------------ embedding rows
@pytest.mark.parametrize("Hd", [8, 4096])
def test_embed_row_widths(dev, Hd):
    """pick_embed_row at Hd = 8 (one 16-byte vector) and 4096 (two turns of the 256 threads of the pick, half a turn of the sampler's
    1024): a table of 100 random bf16 rows, id_offset 39, one sequence and B = 5 with b = 2 done; h_out[b] == table[token], bit for
    bit, and the row of the done sequence and the row behind the last keep the sentinel"""
    table = torch.randn(100, Hd, generator=torch.Generator().manual_seed(Hd)).to(torch.bfloat16).to(dev)
    toks5, s5 = R.commit_batch_case()
    for entry in ("argmax", "sample"):
        for toks, s in (([23], R.state(1)), (toks5, s5)):
            s = dict(s, id_offset=39)
            what = f"Hd {Hd}, {entry}, B {len(toks)}"
            if entry == "argmax":
                v, i = R.parts_for(toks)
                d, ref = _argmax(dev, s, v, i, what, Hd=Hd, table=table)
            else:
                d, ref = _sample(dev, s, R.logits_for(toks), what, params=[(1.0, 1, 1.0, 5)] * len(toks), Hd=Hd, table=table), R.expected(s, toks)
            got = d.read(what)
            _same(what, dict(got, rows=None), dict(ref, rows=None))
            for b, t in enumerate(ref["rows"]):
                assert (got["rows"][b] is None) == (t is None), f"{what}: h_out[{b}]"
                if t is not None:
                    assert torch.equal(d.h_rows[b].view(torch.int16), table[t].cpu().view(torch.int16)), f"{what}: h_out[{b}] != table[{t}]"
