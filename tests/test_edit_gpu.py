"""usdm_logit_edit / usdm_logit_edit_seg through usdm_amd.ops against the numpy restatement (tests/_edit_reference.py): the edited
rows are compared as int32 bit patterns.  And min_p through usdm_sample_final's probs_out: the kept set against the float64
reference, exactly - which rests on a condition on the inputs that is asserted on the CPU before every launch (no id's p / p_max
within relative 1e-4 of min_p: the kernel's f32 ratio is off by less than 2e-5, see min_p_band_empty)."""
import numpy as np
import pytest
import torch

from tests import _edit_reference as E

pytestmark = pytest.mark.gpu

MAX_OUT, PMAX = 2304, 2048
SENT = 12345.0
NEUTRAL = dict(bias={}, n=0, prompt=[], out=[])


def _hist(V, seed, L, alphabet=3):
    """L ids over a small alphabet that includes 0 and V - 1 (n-grams repeat, and the ends of the row get banned)"""
    ids = np.array([0, V - 1, V // 2, 1, V // 3][:alphabet])
    return ids[np.random.default_rng(seed).integers(0, len(ids), L)].tolist()


def _bias(V, seed, count):
    """count distinct ids, ids 0 and V - 1 among them when count >= 2, with values in [-100, 100]"""
    g = np.random.default_rng(seed)
    ids = g.permutation(V)[:count].tolist()
    if count >= 2:
        ids = list(dict.fromkeys([0, V - 1] + ids))[:count]
    return {int(i): float(np.float32(g.uniform(-100, 100))) for i in ids}


def _spec(V, b, seed):
    """Slot b of a batch: [1] is neutral, [2] has its `done` word set, the others mix bias lists of 0 / 1 / a few / min(V, 1024)
    entries with n = 0, 1, 2, 3, 5 over prompts and outputs of several lengths (P = 0 and step = 0 among them)"""
    if b == 1:
        return dict(NEUTRAL, prompt=_hist(V, seed, 9), out=_hist(V, seed + 1, 4))      # a history, but nothing to do with it
    n = (2, 0, 3, 0, 1, 5, 2, 3)[b % 8]
    nb = (3, 0, 5, min(V, 1024), 0, 1, min(V, 6), 0)[b % 8]
    P, G = ((21, 13), (0, 0), (30, 9), (5, 5), (0, 17), (40, 0), (7, 33), (60, 60))[b % 8]
    if b >= 8:
        n, nb = (5, 1, 2, 3, 2, 0, 3, 1)[b % 8], (0, 2, 1024 if V >= 1024 else 1, 0, 4, 7, 0, 1)[b % 8]
    return dict(bias=_bias(V, seed + b, nb), n=n, prompt=_hist(V, seed + 2 * b, P), out=_hist(V, seed + 2 * b + 1, G), done=(b == 2))


class _Dev:
    """Decode state, edit blocks, bias rows and prompt rows of the sequences `specs` on the device"""

    def __init__(self, dev, specs, id_offset=0):
        from usdm_amd import ops
        B = self.B = len(specs)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        self.out, self.step, self.nxt, self.pos = i32(B, MAX_OUT), i32(B), i32(B), i32(B)
        self.params = ops.edit_params_tensor(dev, B).view(B, -1)
        self.bias_id, self.bias_val = torch.full((B, ops.LOGIT_BIAS_MAX), -7, dtype=torch.int32, device=dev), torch.full((B, ops.LOGIT_BIAS_MAX), 999.0, device=dev)
        self.prompt = torch.full((B, PMAX), -3, dtype=torch.int32, device=dev)
        for b, s in enumerate(specs):
            assert len(s["out"]) <= MAX_OUT and len(s["prompt"]) <= PMAX
            if s["out"]:
                self.out[b, :len(s["out"])] = torch.tensor(s["out"], dtype=torch.int32) + id_offset
            self.step[b] = len(s["out"])
            if s["prompt"]:
                self.prompt[b, :len(s["prompt"])] = torch.tensor(s["prompt"], dtype=torch.int32)
            if s["bias"]:
                self.bias_id[b, :len(s["bias"])] = torch.tensor(list(s["bias"]), dtype=torch.int32)
                self.bias_val[b, :len(s["bias"])] = torch.tensor(list(s["bias"].values()), dtype=torch.float32)
            ops.set_edit_params(self.params[b], s["n"], len(s["prompt"]), len(s["bias"]))
        done = [int(bool(s.get("done"))) for s in specs]
        self.done = torch.tensor(done, dtype=torch.int32, device=dev) if any(done) else None
        self.eos = None if self.done is None else i32(8)
        one = B == 1
        self.st = ops.decode_state(self.nxt, self.out[0] if one else self.out, self.step, self.pos, id_offset=id_offset, batch=0 if one else B,
                                   done=self.done, eos=self.eos)
        pick = (lambda t: t[0]) if one else (lambda t: t)
        self.kw = dict(dev_params=pick(self.params), bias_id=pick(self.bias_id), bias_val=pick(self.bias_val), prompt=pick(self.prompt))


def _want(rows, specs, id_offset=0):
    return np.stack([x.copy() if s.get("done") else E.edit_row(x, s["bias"], s["n"], s["prompt"], [t + id_offset for t in s["out"]], id_offset)
                     for x, s in zip(rows, specs)])


def _rows(V, B, seed):
    rows = np.stack([E.bf16_row(V, seed + 7 * b) for b in range(B)])
    rows[:, V // 5:V // 5 + max(1, V // 10)] = -np.inf      # a banned range, as the lm_head writes it
    return rows


def _run(dev, rows, specs, id_offset=0):
    from usdm_amd import ops
    d = _Dev(dev, specs, id_offset)
    x = torch.from_numpy(rows).to(dev)
    ops.logit_edit(x[0] if len(specs) == 1 else x, d.st, **d.kw)
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize("B", [1, 4, 16])
@pytest.mark.parametrize("V", [7, 1000, 42003])
def test_rows_match_the_reference_bit_for_bit(dev, V, B):
    rows = _rows(V, B, 3 * V + B)
    specs = [_spec(V, b, 11 * V + B) for b in range(B)] if B > 1 else [_spec(V, 0, 11 * V)]
    got, want = _run(dev, rows, specs), _want(rows, specs)
    for b in range(B):
        assert np.array_equal(E.bits(got[b]), E.bits(want[b])), (b, specs[b]["n"], len(specs[b]["bias"]))
    assert not np.array_equal(E.bits(got[0]), E.bits(rows[0]))                   # slot 0 was edited
    if B > 1:
        assert np.array_equal(E.bits(got[1]), E.bits(rows[1]))                   # the neutral slot: every bit stays
        assert specs[2]["done"] and (specs[2]["bias"] or specs[2]["n"]) and np.array_equal(E.bits(got[2]), E.bits(rows[2]))
        assert len(specs[3]["bias"]) == min(V, 1024) and {0, V - 1} <= set(specs[3]["bias"])
        assert not np.array_equal(E.bits(got[3]), E.bits(rows[3]))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("V,nseg,seg_len", [(1003, 2, 502), (42003, 8, 5251)])
def test_segmented_form_equals_the_reference(dev, V, nseg, seg_len, B):
    from usdm_amd import ops
    assert (nseg - 1) * seg_len < V < nseg * seg_len            # the last segment is only partly inside V
    rows = _rows(V, B, 5 * V + B)
    specs = [_spec(V, b, 13 * V + B) for b in (range(B) if B > 1 else [0])]
    want = _want(rows, specs)
    pad = np.full((B, nseg * seg_len), SENT, dtype=np.float32)      # [nseg][B][seg_len], padding slots (ids >= V) hold a sentinel
    pad[:, :V] = rows
    seg = torch.from_numpy(np.ascontiguousarray(pad.reshape(B, nseg, seg_len).transpose(1, 0, 2))).to(dev)
    d = _Dev(dev, specs)
    ops.logit_edit(seg, d.st, V=V, nseg=nseg, seg_stride=B * seg_len, seg_len=seg_len, **d.kw)
    torch.cuda.synchronize()
    got = seg.cpu().numpy().transpose(1, 0, 2).reshape(B, nseg * seg_len)
    assert np.array_equal(E.bits(got[:, :V]), E.bits(want)) and bool((got[:, V:] == SENT).all())
    assert not np.array_equal(E.bits(got[0, :V]), E.bits(rows[0]))
    if B == 1:      # one sequence's gathered row is also a contiguous row that is longer than V
        flat = torch.from_numpy(pad[0].copy()).to(dev)
        ops.logit_edit(flat, d.st, V=V, **d.kw)
        torch.cuda.synchronize()
        assert np.array_equal(E.bits(flat.cpu().numpy()[:V]), E.bits(want[0])) and bool((flat[V:] == SENT).all())


@pytest.mark.parametrize("id_offset", [0, 32002])
def test_ngram_sizes_and_history_lengths(dev, id_offset):
    """n in {0, 1, 2, 3, 5} x Lh in {n - 1, n, n + 1}, the history all generated (P = 0), all prompt (step = 0) and split; an all-equal
    history (many writers of one id); one launch of 16 sequences per group of cases"""
    V = 1000
    specs = []
    for n in (0, 1, 2, 3, 5):
        for Lh in (n - 1, n, n + 1):
            if Lh < 0:
                continue
            h = [V - 1] * Lh if n in (1, 3) else _hist(V, 100 * n + Lh, Lh, alphabet=2)
            for P in sorted({0, Lh, Lh // 2}):
                specs.append(dict(bias={}, n=n, prompt=h[:P], out=h[P:]))
    specs.append(dict(bias={5: 1.0}, n=3, prompt=[5] * 300, out=[5] * 200))         # all equal: 498 threads store to id 5
    specs.append(dict(bias={}, n=2, prompt=[], out=[]))                               # nothing at all
    changed, equal_row = 0, None
    for g0 in range(0, len(specs), 16):
        grp = specs[g0:g0 + 16]
        assert len(grp) >= 2
        rows = _rows(V, len(grp), g0 + 1)
        rows[:, V - 1] = 1.5
        got, want = _run(dev, rows, grp, id_offset), _want(rows, grp, id_offset)
        for b, s in enumerate(grp):
            assert np.array_equal(E.bits(got[b]), E.bits(want[b])), (s["n"], s["prompt"], s["out"])
            Lh = len(s["prompt"]) + len(s["out"])
            if Lh < s["n"] or s["n"] == 0:
                assert np.array_equal(E.bits(got[b]), E.bits(rows[b]))
            changed += int(not np.array_equal(E.bits(got[b]), E.bits(rows[b])))
            if s["bias"]:
                equal_row = got[b]
    assert changed >= 12 and np.isneginf(equal_row[5])


@pytest.mark.parametrize("id_offset", [0, 7])
def test_matches_across_the_prompt_boundary_and_long_histories(dev, id_offset):
    V = 1000
    a, b_, c = 700, 701, 702
    g = np.random.default_rng(5)
    filler = lambda L: g.integers(10, 600, L).tolist()
    specs = [
        # n = 5, history ... a b a b | a b: the tail a b a b straddles the boundary; the window starting 4 ids before it matches with its
        # first four ids in the prompt and bans the id it ends on, the first GENERATED token (a); one step earlier ... a b a b bans b too
        dict(bias={}, n=5, prompt=filler(20) + [a, b_, a, b_], out=[a, b_]),
        # n = 3: the only earlier occurrence of the tail (a b) ends the prompt, the id it bans (c) is the first generated one
        dict(bias={}, n=3, prompt=filler(30) + [a, b_], out=[c] + filler(9) + [a, b_]),
        # 1025 and 2100 tokens: a thread handles more than one j; the only match sits past j = 1024 (2100: past j = 2048)
        dict(bias={}, n=3, prompt=filler(1000), out=filler(12) + [a, b_, c] + filler(8) + [a, b_]),
        dict(bias={c: 50.0}, n=3, prompt=filler(2040), out=filler(15) + [a, b_, c] + filler(40) + [a, b_]),
    ]
    assert len(specs[2]["prompt"]) + len(specs[2]["out"]) == 1025 and len(specs[3]["prompt"]) + len(specs[3]["out"]) == 2100
    rows = _rows(V, len(specs), 17)
    rows[:, 690:710] = 2.0
    got, want = _run(dev, rows, specs, id_offset), _want(rows, specs, id_offset)
    for i in range(len(specs)):
        assert np.array_equal(E.bits(got[i]), E.bits(want[i])), i
    assert np.isneginf(got[0][a]) and not np.isneginf(got[0][b_])
    assert all(np.isneginf(got[i][c]) and not np.isneginf(got[i][a]) for i in (1, 2, 3))      # (3: biased AND banned ends at -inf)
    assert all(int(np.isneginf(got[i]).sum()) == int(np.isneginf(rows[i]).sum()) + 1 for i in range(4))


def test_bias_special_values_and_the_barrier(dev):
    """A bias on a -inf logit stays -inf, on a NaN logit stays NaN; an id that is biased and banned ends at -inf on every one of 16
    sequences (the barrier between the two phases); entries outside [0, V) are ignored; bias_val beyond n_bias is never read"""
    from usdm_amd import ops
    V, B = 1000, 16
    rows = _rows(V, B, 23)
    rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6] = -np.inf, np.nan, 1.25, -0.0
    bias = {3: 100.0, 4: -3.0, 5: 100.0, 6: 0.0, 999: -100.0, 0: 0.5}
    specs = [dict(bias=bias, n=1, prompt=[5, 5, 999], out=[5]) for _ in range(B)]
    d = _Dev(dev, specs)
    d.bias_id[:, 2] = torch.tensor([V, -1, 1 << 20, -(1 << 31)] * 4, dtype=torch.int32, device=dev)      # entry 2 (id 5's bias) now out of range
    x = torch.from_numpy(rows).to(dev)
    ops.logit_edit(x, d.st, **d.kw)
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    want = np.stack([E.edit_row(r, {k: v for k, v in bias.items() if k != 5}, 1, [5, 5, 999], [5]) for r in rows])
    cols = np.arange(V) != 4                                  # (the NaN column: NaN-ness below, not its payload)
    assert np.array_equal(E.bits(got[:, cols]), E.bits(want[:, cols]))
    assert np.isneginf(got[:, 3]).all() and np.isnan(got[:, 4]).all() and np.isneginf(got[:, 5]).all() and np.isneginf(got[:, 999]).all()
    assert (E.bits(got[:, 6]) == E.bits(np.float32(0.0))).all() and np.array_equal(got[:, 0], rows[:, 0] + np.float32(0.5))


# ---------------------------------------------------------------------------------------------- min_p (usdm_sample_final)
MINP_V, MINP_SEED = 42003, 4
MINP_CASES = [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.3, 0, 0.95), (1.0, 200, 1.0), (0.7, 0, 1.0), (1.3, 2000, 0.99)]      # T, top_k, top_p


def _minp_row():
    x = E.bf16_row(MINP_V, MINP_SEED)
    x[np.random.default_rng(MINP_SEED).integers(0, MINP_V, MINP_V // 10)] = -np.inf
    return x


def _state(dev, step, B=0):
    from usdm_amd import ops
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
    n = max(1, B)
    nxt, out, stp, pos = i32(n), torch.zeros(n, 64, dtype=torch.int32, device=dev), i32(n, step), i32(n)
    return ops.decode_state(nxt, out[0] if B == 0 else out, stp, pos, batch=B), nxt


def _segmented(x, nseg, dev):
    seg_len = -(-x.shape[0] // nseg)
    pad = np.full(nseg * seg_len, SENT, dtype=np.float32)
    pad[:x.shape[0]] = x
    return torch.from_numpy(pad.reshape(nseg, 1, seg_len)).to(dev), seg_len


@pytest.mark.parametrize("min_p", [0.05, 0.3])
@pytest.mark.parametrize("T,k,p", MINP_CASES)
def test_min_p_kept_set_equals_the_float64_reference(dev, T, k, p, min_p):
    from oracle import sampling_oracle as so
    from usdm_amd import ops
    x, V = _minp_row(), MINP_V
    assert E.min_p_band_empty(x, T, min_p), "an id's p / p_max is within 1e-4 of min_p: choose another seed"
    base = so.filtered_probs(x, T, k, p)                  # temperature / top-k / top-p (what tests/test_sampling_gpu.py pins)
    keep = (base > 0) & E.min_p_keep(x, T, min_p)
    assert 1 <= keep.sum() < (base > 0).sum()             # min_p drops something on top of the other filters
    ref = np.where(keep, base, 0.0)
    ref /= ref.sum()
    step, seed = 5, 1234
    xd, probs = torch.from_numpy(x).to(dev), torch.zeros(V, device=dev)
    st, nxt = _state(dev, step)
    ops.sample_final(xd, st, temperature=T, top_k=k, top_p=p, seed=seed, min_p=min_p, probs_out=probs)      # the knobs as host arguments
    torch.cuda.synchronize()
    got = probs.cpu().numpy()
    print(f"T={T} k={k} p={p} min_p={min_p}: kept {int((got > 0).sum())} (reference {int(keep.sum())}) of {int((base > 0).sum())}")
    assert np.array_equal(got > 0, keep)
    np.testing.assert_allclose(got.astype(np.float64), ref, rtol=1e-5, atol=1e-10)
    tok = int(nxt.item())
    assert keep[tok]
    # segmented, the knobs in the device block: the same bits, the same draw
    seg, seg_len = _segmented(x, 8, dev)
    sp = ops.sample_params_tensor(dev)
    ops.set_sample_params(sp, T, k, p, seed, min_p=min_p)
    probs2 = torch.zeros(V, device=dev)
    st2, nxt2 = _state(dev, step)
    ops.sample_final(seg, st2, V=V, nseg=8, seg_stride=seg_len, seg_len=seg_len, dev_params=sp, probs_out=probs2)
    torch.cuda.synchronize()
    assert np.array_equal(E.bits(probs2.cpu().numpy()), E.bits(got)) and int(nxt2.item()) == tok


@pytest.mark.parametrize("T", [1.0, 1.5])
def test_min_p_one_keeps_the_maximum_and_its_exact_ties(dev, T):
    from usdm_amd import ops
    x, V = _minp_row(), MINP_V
    top = np.float32(x[np.isfinite(x)].max())
    x[[17, 4000, V - 1]] = top
    assert E.min_p_band_empty(x, T, 1.0)
    keep = x == top
    assert keep.sum() >= 3 and np.array_equal(keep, E.min_p_keep(x, T, 1.0))
    toks = set()
    for form in ("contiguous", "segmented"):
        for step in range(6):
            probs = torch.zeros(V, device=dev)
            st, nxt = _state(dev, step)
            if form == "contiguous":
                ops.sample_final(torch.from_numpy(x).to(dev), st, temperature=T, seed=3, min_p=1.0, probs_out=probs)
            else:
                seg, seg_len = _segmented(x, 8, dev)
                ops.sample_final(seg, st, V=V, nseg=8, seg_stride=seg_len, seg_len=seg_len, temperature=T, seed=3, min_p=1.0, probs_out=probs)
            torch.cuda.synchronize()
            got = probs.cpu().numpy()
            assert np.array_equal(got > 0, keep) and np.allclose(got[keep], 1.0 / keep.sum(), rtol=1e-6)
            assert keep[int(nxt.item())]
            toks.add((step, int(nxt.item())))
    assert len(toks) == 6      # (step, token) pairs: both forms drew the same token at every step


def test_min_p_zero_is_the_call_that_never_sets_it(dev):
    """min_p = 0 as a host argument and in the device block, and a device block holding NaN / a negative value / a value above 1
    (taken as 0): probs_out and token bit-identical with the call without min_p; with top_k = 1 any min_p changes nothing"""
    from usdm_amd import ops
    x, V = _minp_row(), MINP_V
    xd = torch.from_numpy(x).to(dev)

    def run(step, **kw):
        probs = torch.zeros(V, device=dev)
        st, nxt = _state(dev, step)
        ops.sample_final(xd, st, probs_out=probs, **kw)
        torch.cuda.synchronize()
        return E.bits(probs.cpu().numpy()), int(nxt.item())

    for T, k, p in MINP_CASES[:3]:
        for step in (0, 9):
            plain = run(step, temperature=T, top_k=k, top_p=p, seed=77)
            zero = run(step, temperature=T, top_k=k, top_p=p, seed=77, min_p=0.0)
            assert np.array_equal(plain[0], zero[0]) and plain[1] == zero[1]
            sp = ops.sample_params_tensor(dev)
            for raw in (0.0, float("nan"), -0.25, 1.5, -0.0):
                ops.set_sample_params(sp, T, k, p, 77)
                sp[12:16] = torch.from_numpy(np.frombuffer(np.float32(raw).tobytes(), dtype=np.uint8).copy()).to(dev)
                blk = run(step, dev_params=sp)
                assert np.array_equal(plain[0], blk[0]) and plain[1] == blk[1], raw
    greedy, with_min_p = run(0, top_k=1), run(0, top_k=1, min_p=0.9)
    assert np.array_equal(with_min_p[0], greedy[0]) and with_min_p[1] == greedy[1] == int(np.argmax(np.where(np.isfinite(x), x, -np.inf)))
