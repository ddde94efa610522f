"""The end of a decode step in plain Python / numpy (TEST INFRASTRUCTURE ONLY): the greedy pick over the lm_head's partials
(`pick_ref`) and the commit of the picked token to the device-side decode state (`commit_ref`), written from the contract in
include/usdm_hip.h (usdm_decode_state, usdm_argmax_final), plus the case builders that tests/test_pick_cpu.py and
tests/test_pick_gpu.py share.  Everything here is integers and bit patterns: no tolerance anywhere."""
import copy

import numpy as np

NO_ID = 0x7FFFFFFF                    # the id of the "no candidate" partial, which carries the value -inf
NINF, PINF = float("-inf"), float("inf")
POISON_V, POISON_I = PINF, -1         # what every input gap holds: it would win if it were read
SENT = 0x5A5A5A5A                     # what every int32 word around an output holds
ID0 = 10                              # ordinary partials carry ids >= ID0: ids 0 .. 9 are free for the placements that need the lowest
MAX_OUT = 8
EOS_WORDS = 10                        # eos buffers: {n, min_new, ids ...} with room for a seventh id and poison behind it
PICK_NPARTS = (1, 2, 63, 64, 65, 255, 256, 257, 1003)
PICK_V = ID0 + 8 * 1003 + 6           # ids of the pick cases are < PICK_V (8 segments of 1003 partials)
OFFSETS = (0, 32002)


# ------------------------------------------------------------------------------------------------------------------ the reference
def pick_ref(part_val, part_idx):
    """All partials of one sequence, in any layout -> the picked id (before id_offset).  Among the entries that are not NaN the
    largest value (compared as floats: +0.0 == -0.0), among equal values the lowest id.  (-inf, NO_ID) is no entry at all, so a real
    (-inf, id) beats it; with nothing real left the result is 0."""
    best = None
    for v, i in zip(np.asarray(part_val, np.float32).reshape(-1).tolist(), np.asarray(part_idx).reshape(-1).tolist()):
        if v != v or (v == NINF and i == NO_ID):
            continue
        if best is None or v > best[0] or (v == best[0] and i < best[1]):
            best = (v, i)
    return 0 if best is None else best[1]


def state(B=1, *, max_out=MAX_OUT, step=0, pos=7, done=None, eos=None, advance_pos=1, id_offset=0):
    """A decode state on the host.  step / pos / done: one int for every sequence or a list; done / eos None = a null pointer.
    rows[b] is the token whose embedding row h_out[b] holds (None: untouched)."""
    per = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * B
    return dict(B=B, max_out=max_out, advance_pos=advance_pos, id_offset=id_offset, next_token=[-3 - b for b in range(B)],
                out_tokens=[[-(100 + b * max_out + i) for i in range(max_out)] for b in range(B)], step=per(step), pos=per(pos),
                done=None if done is None else per(done), eos=None if eos is None else list(eos), rows=[None] * B)


def commit_ref(s, b, tok):
    """-> the state after sequence b committed token `tok` (id_offset already added); s itself is left alone"""
    s = copy.deepcopy(s)
    if s["done"] is not None and s["done"][b] != 0:
        return s
    step = s["step"][b]
    s["next_token"][b] = tok
    if step < s["max_out"]:
        s["out_tokens"][b][step] = tok
    s["step"][b] = step + 1
    if s["advance_pos"]:
        s["pos"][b] += 1
    if s["done"] is not None and s["eos"] is not None:
        n, min_new = s["eos"][0], s["eos"][1]
        if tok in s["eos"][2:2 + max(0, min(n, 6))] and step + 1 >= min_new:
            s["done"][b] = 1
    s["rows"][b] = tok
    return s


def expected(s, toks):
    """the state after one launch in which sequence b picked raw id toks[b]"""
    for b, t in enumerate(toks):
        s = commit_ref(s, b, t + s["id_offset"])
    return s


def eos_words(n, min_new, ids, tok):
    """{n, min_new, ids ...}; every word behind the ids given holds `tok`: a hit if the kernel read it"""
    return [n, min_new] + list(ids) + [tok] * (EOS_WORDS - 2 - len(ids))


# ------------------------------------------------------------------------------------------------------------------ the pick's cases
def background(n, seed):
    """n losing partials: negative values with many ties among them, distinct ids >= ID0 in an order unrelated to position"""
    g = np.random.default_rng(seed)
    return (-(1.0 + g.integers(0, 1000, n) / 8.0)).astype(np.float32), (g.permutation(n) + ID0).astype(np.int32)


def winner_positions(nparts):
    """position 0 and the last, lane 0 of waves 1, 2 and 3, position 255, and the second pass of the stride-256 loop (256, and one
    before the last), as far as nparts has them"""
    return sorted({p for p in (0, 64, 128, 192, 255, 256, nparts - 2, nparts - 1) if 0 <= p < nparts and (p in (0, nparts - 1) or p >= 64)})


def tie_slots(nparts, nseg):
    """up to three (segment, position) slots in launch order for entries that meet only late in the reduction: different waves where
    nparts has them (the last one in the second pass where there is one), and with segments the first, a middle and the last"""
    ps = [3, 64 + 3, max(p for p in range(nparts) if p % 256 >= 128)] if nparts >= 132 else [0, nparts // 2, nparts - 1]
    sg = [0, nseg // 2, nseg - 1]
    slots = []
    for s_, p in list(zip(sg, ps)) + [(s_, p) for s_ in sg for p in ps]:
        if (s_, p) not in slots and len(slots) < 3:
            slots.append((s_, p))
    return sorted(slots)


def pick_cases(nparts, nseg=1):
    """-> [(name, vals [nseg][nparts] float32, ids [nseg][nparts] int32)]: the placements of one sequence's partials"""
    n, out, k = nseg * nparts, [], [0]

    def bg():
        k[0] += 1
        v, i = background(n, 100000 * nseg + 100 * nparts + k[0])
        return v.reshape(nseg, nparts), i.reshape(nseg, nparts)

    for sg in sorted({0, nseg // 2, nseg - 1}):
        for p in winner_positions(nparts):
            v, i = bg()
            v[sg, p] = 3.5
            out.append((f"winner in segment {sg} at {p}", v, i))
    slots = tie_slots(nparts, nseg)
    if len(slots) > 1:
        v, i = bg()      # exact tie, ids descending in launch order: the lowest id sits last
        for (s_, p), id_ in zip(slots, sorted((int(i[s]) for s in slots), reverse=True)):
            v[s_, p], i[s_, p] = 2.25, id_
        out.append((f"{len(slots)}-way tie, ids descending", v, i))
        v, i = bg()      # +0.0 with the higher id first, -0.0 with the lower id later; everything else negative
        (a, b), (lo, hi) = slots[:2], sorted(int(i[s]) for s in slots[:2])
        v[a], i[a], v[b], i[b] = 0.0, hi, -0.0, lo
        out.append(("+0.0 against -0.0", v, i))
    v, i = bg()          # NaN on the lowest ids next to a finite winner (one partial only: no NaN)
    for id_, s in enumerate(slots[:n - 1]):
        v[s], i[s] = np.nan, id_
    free = next((s_, p) for s_ in range(nseg) for p in range(nparts) if (s_, p) not in slots[:n - 1])
    v[free] = 1.5
    out.append(("NaN on the lowest ids", v, i))
    v, i = bg()
    v[:], i[:] = np.nan, np.arange(n, dtype=np.int32).reshape(nseg, nparts)
    out.append(("NaN everywhere", v, i))
    v, i = bg()
    v[slots[len(slots) // 2]] = PINF
    out.append(("+inf wins", v, i))
    v, i = np.full((nseg, nparts), NINF, np.float32), np.full((nseg, nparts), NO_ID, np.int32)
    out.append(("no candidate anywhere", v.copy(), i.copy()))
    i[slots[-1]] = 5
    out.append(("a real (-inf, 5) among no candidates", v, i))
    return out


def batch_case(B, nparts, nseg):
    """-> vals, ids [nseg][B][nparts]: sequence b's unique winner has id ID0 + b and sits in segment b % nseg at (11 + 29 b) % nparts
    (nparts prime to 29 and >= B: all positions differ)"""
    vals, ids = np.empty((nseg, B, nparts), np.float32), np.empty((nseg, B, nparts), np.int32)
    for b in range(B):
        v, i = background(nseg * nparts, 7000 + 100 * B + b)
        at, slot = int(np.nonzero(i == ID0 + b)[0][0]), (b % nseg) * nparts + (11 + 29 * b) % nparts
        i[at], i[slot] = i[slot], i[at]
        v[slot] = 1.0 + b
        vals[:, b], ids[:, b] = v.reshape(nseg, nparts), i.reshape(nseg, nparts)
    return vals, ids


def lay_out(vals, ids, gap=0, tail=7):
    """vals / ids [nseg][B][nparts] -> (flat values, flat ids, seg_stride) with seg_stride = B * nparts + gap; the gaps and `tail`
    words behind the last sequence hold the poison"""
    nseg, B, nparts = vals.shape
    ss = B * nparts + gap
    pv, pi = np.full((nseg - 1) * ss + B * nparts + tail, POISON_V, np.float32), np.full((nseg - 1) * ss + B * nparts + tail, POISON_I, np.int32)
    for s_ in range(nseg):
        pv[s_ * ss:s_ * ss + B * nparts], pi[s_ * ss:s_ * ss + B * nparts] = vals[s_].reshape(-1), ids[s_].reshape(-1)
    return pv, pi, ss


def parts_for(toks, nparts=5, nseg=1):
    """partials [nseg][B][nparts] that encode toks[b]: a unique winner with that id in segment b % nseg"""
    B = len(toks)
    vals, ids = np.empty((nseg, B, nparts), np.float32), np.empty((nseg, B, nparts), np.int32)
    for b, t in enumerate(toks):
        v, i = background(nseg * nparts, 9000 + b)
        i += 1000      # (the losers' ids stay clear of every token and EOS id of the commit cases)
        slot = (b % nseg) * nparts + (2 + b) % nparts
        v[slot], i[slot] = 2.0, t
        vals[:, b], ids[:, b] = v.reshape(nseg, nparts), i.reshape(nseg, nparts)
    return vals, ids


COMMIT_V = 61


def logits_for(toks, V=COMMIT_V):
    """[B][V] bf16-valued logits whose maximum sits at toks[b], and again exactly at toks[b] + 3 and V - 1; a few ids banned"""
    g = np.random.default_rng(77)
    x = -(1.0 + g.integers(0, 64, (len(toks), V)) / 16.0).astype(np.float32)
    x[:, ::7] = NINF
    for b, t in enumerate(toks):
        assert t + 3 < V - 1
        x[b, [t, t + 3, V - 1]] = 4.0
    return x


# ------------------------------------------------------------------------------------------------------------------ the commit's cases
def commit_cases():
    """-> [(name, raw id, state of one sequence)], max_out = 8"""
    C, T = [], 23

    def add(name, ids=None, n=None, min_new=0, *, off=0, **kw):
        eos = None if ids is None else eos_words(len(ids) if n is None else n, min_new, ids, T + off)
        C.append((name, T, state(1, eos=eos, id_offset=off, **{"done": 0, **kw})))

    others = [90, 91, 92, 93, 94, 95]
    for step in (0, MAX_OUT - 1, MAX_OUT, MAX_OUT + 3):
        add(f"step {step}, no hit", [90], step=step)
        add(f"step {step}, hit", [T], step=step)
    for adv in (0, 1):
        add(f"advance_pos {adv}", [90], advance_pos=adv)
    add("n_eos 0", [])
    add("n_eos 1, hit", [T])
    add("n_eos 6, hit at the first", [T] + others[:5])
    add("n_eos 6, hit at the sixth", others[:5] + [T])
    add("n_eos 6, no hit", others)
    add("n_eos 7, the token in the seventh slot only", others + [T])
    add("n_eos 2, the token in the third id word", others[:2] + [T], n=2)
    for step in (0, 3):
        for mn in sorted({0, step, step + 1, step + 2}):
            add(f"hit at step {step}, min_new {mn}", [90, T], min_new=mn, step=step)
    add("eos given, done null", [T], done=None)
    add("done given, eos null", None)
    add("both null", None, done=None)
    add("id_offset: only the offset token matches", [T + 32002], off=32002)
    add("id_offset: only the raw id matches", [T], off=32002)
    return C


def commit_batch_case():
    """B = 5: a step, a pos and an EOS outcome of its own for every sequence; b = 2 is done before the launch -> (raw ids, state)"""
    toks = [23, 24, 25, 26, 27]
    eos = eos_words(2, 9, [24, 27], 23)      # b = 1: a hit below min_new; b = 4: a hit past it (and past max_out)
    return toks, state(5, step=[0, 7, 3, 8, 11], pos=[7, 0, 40, 5, 100], done=[0, 0, 1, 0, 0], eos=eos)


# ------------------------------------------------------------------------------------------------------------------ the sampled commit
SAMPLED = dict(V=517, B=3, top_p=0.9, seeds=(2 ** 40 + 7, 12345, 99), steps=(0, 5, MAX_OUT + 1), off=11)


def sampled_case():
    """-> (logits [3][517], oracle tokens, state): every sequence draws with its own seed at its own step (one of them past max_out);
    the EOS id is what the oracle draws for sequence 1"""
    from oracle import sampling_oracle as so
    c = SAMPLED
    g = np.random.default_rng(517)
    x = (g.standard_normal((c["B"], c["V"])) * 3).astype(np.float32)
    x = (x.view(np.uint32) & 0xFFFF0000).view(np.float32)      # bf16-valued (truncated)
    x[:, g.integers(0, c["V"], 50)] = NINF
    toks = [so.sample(x[b], c["steps"][b], 1.0, 0, c["top_p"], c["seeds"][b])[0] for b in range(c["B"])]
    assert toks[0] != toks[1] != toks[2], "the seeds must give sequence 1 a token of its own"
    s = state(c["B"], step=list(c["steps"]), pos=[7, 8, 9], done=0, eos=eos_words(1, 0, [toks[1] + c["off"]], -1), id_offset=c["off"])
    return x, toks, s
