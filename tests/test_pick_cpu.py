"""CPU: the reference of tests/test_pick_gpu.py checked on its own, and the refusals of usdm_argmax_final(_seg).
  * pick_ref == torch.argmax of the dense masked logits row, over 2000 seeded rows full of ties whose partials are permuted;
  * commit_ref == a second, naive statement of the commit on the hand-built cases, and the cases are the ones the issue lists;
  * the case builders give the placements they promise (the tie's lowest id sits last, the poison would win if it were read);
  * usdm_argmax_final(_seg) refuses bad arguments with a message; nothing is launched."""
import ctypes

import numpy as np
import torch

from tests import _pick_reference as R


# ------------------------------------------------------------------------------------------------------------------ pick_ref
def _partials(row):
    """the lm_head's partials of a masked row: the first maximum of every block of 16 ids, (-inf, NO_ID) for a fully banned block"""
    pv, pi = [], []
    for b0 in range(0, len(row), 16):
        blk = row[b0:b0 + 16]
        if np.all(blk == R.NINF):
            pv.append(R.NINF), pi.append(R.NO_ID)
        else:
            pv.append(blk.max()), pi.append(b0 + int(np.argmax(blk)))
    return np.array(pv, np.float32), np.array(pi, np.int64)


def test_pick_ref_is_torch_argmax():
    g = np.random.default_rng(2024)
    levels = np.array([-2.0, -0.5, 0.0, 0.5, 3.0], np.float32)
    n_tied = n_banned_blocks = n_all_banned = 0
    for r in range(2000):
        V = int(g.integers(37, 1101))
        row = levels[g.integers(0, 5 if r % 3 else 3, V)]
        row[g.random(V) < 0.2] = R.NINF
        for b0 in g.integers(0, V // 16 + 1, 3) * 16:      # whole blocks banned (every 50th row: all of them)
            row[b0:b0 + 16] = R.NINF
        if r % 50 == 0:
            row[:] = R.NINF
        pv, pi = _partials(row)
        n_tied += int((pv == pv.max()).sum() > 1)
        n_banned_blocks += int((pi == R.NO_ID).any())
        n_all_banned += int((pi == R.NO_ID).all())
        perm = g.permutation(len(pv))
        want = int(torch.argmax(torch.from_numpy(row)))
        assert R.pick_ref(pv[perm], pi[perm]) == want, (r, V)
    assert n_tied > 1500 and n_banned_blocks > 1500 and n_all_banned >= 10, (n_tied, n_banned_blocks, n_all_banned)


def test_pick_ref_edges():
    nan = float("nan")
    assert R.pick_ref([R.NINF, R.NINF], [R.NO_ID, 5]) == 5                     # a real -inf beats "no candidate"
    assert R.pick_ref([R.NINF, R.NINF], [R.NO_ID, R.NO_ID]) == 0
    assert R.pick_ref([nan, 1.0, nan], [0, 9, 1]) == 9 and R.pick_ref([nan], [4]) == 0
    assert R.pick_ref([0.0, -0.0, -1.0], [8, 3, 1]) == 3 and R.pick_ref([-0.0, 0.0], [8, 3]) == 3
    assert R.pick_ref([R.PINF, 1e38], [7, 2]) == 7
    assert R.pick_ref(np.array([[2.0, 1.0], [2.0, 2.0]]), np.array([[30, 1], [20, 10]])) == 10      # any layout


# ------------------------------------------------------------------------------------------------------------------ the case builders
def test_pick_cases_place_what_they_promise():
    seen = set()
    for nseg in (1, 2, 8):
        for nparts in R.PICK_NPARTS:
            for name, v, i in R.pick_cases(nparts, nseg):
                assert v.shape == i.shape == (nseg, nparts) and v.dtype == np.float32 and i.dtype == np.int32
                real = ~((v == R.NINF) & (i == R.NO_ID))
                assert int(i[real].min(initial=0)) >= 0 and int(i[real].max(initial=0)) < R.PICK_V
                want = R.pick_ref(v, i)
                kind = "winner" if name.startswith("winner") else "tie" if "-way tie" in name else name
                seen.add(kind)
                flat_v, flat_i = v.reshape(-1), i.reshape(-1)
                if kind == "winner":
                    sg, p = int(name.split()[3]), int(name.split()[5])
                    assert int(i[sg, p]) == want and int((v == v.max()).sum()) == 1
                elif kind == "tie":
                    at = np.nonzero(flat_v == flat_v.max())[0]
                    assert len(at) == min(3, nseg * nparts) and list(flat_i[at]) == sorted(flat_i[at], reverse=True) and want == flat_i[at[-1]]
                    if nparts >= 132:      # partners in different waves, with segments in different segments
                        assert len({(a % nparts % 256) // 64 for a in at}) == 3
                    if nseg > 1 and nparts > 1:
                        assert len({a // nparts for a in at}) == min(3, nseg)
                elif kind == "+0.0 against -0.0":
                    z = np.nonzero(flat_v == 0)[0]
                    assert len(z) == 2 and not np.signbit(flat_v[z[0]]) and np.signbit(flat_v[z[1]]) and flat_i[z[1]] < flat_i[z[0]]
                    assert want == flat_i[z[1]] and (np.delete(flat_v, z) < 0).all()
                elif kind == "NaN on the lowest ids":
                    nn = np.isnan(flat_v)
                    assert int(nn.sum()) == min(3, nseg * nparts - 1) and sorted(flat_i[nn]) == list(range(int(nn.sum())))
                    assert want >= R.ID0 and flat_v[flat_i == want][0] == 1.5
                elif kind == "+inf wins":
                    assert flat_v[flat_i == want][0] == R.PINF
                elif kind == "a real (-inf, 5) among no candidates":
                    assert want == 5 and (flat_v == R.NINF).all() and int((flat_i != R.NO_ID).sum()) == 1
                else:
                    assert kind in ("NaN everywhere", "no candidate anywhere") and want == 0
                # the poison of the gaps would win if it were read
                assert R.pick_ref(np.r_[flat_v, R.POISON_V], np.r_[flat_i, R.POISON_I]) == R.POISON_I or kind == "+inf wins"
    assert len(seen) == 8, seen
    assert R.winner_positions(1003) == [0, 64, 128, 192, 255, 256, 1001, 1002] and R.winner_positions(1) == [0]


def test_batch_case_and_layout():
    for B in (2, 5, 16, 64):
        for nseg in (1, 2):
            for nparts in (67, 300):
                v, i = R.batch_case(B, nparts, nseg)
                wins = [R.pick_ref(v[:, b], i[:, b]) for b in range(B)]
                assert wins == [R.ID0 + b for b in range(B)]
                where = [int(np.argmax(v[:, b].reshape(-1))) for b in range(B)]
                assert len({w % nparts for w in where}) == B and all(w // nparts == b % nseg for b, w in enumerate(where))
    v, i = R.batch_case(2, 67, 2)
    pv, pi, ss = R.lay_out(v, i, gap=5)
    assert ss == 139 and len(pv) == 139 + 134 + 7
    assert (pv[134:139] == R.POISON_V).all() and (pi[134:139] == -1).all() and (pv[-7:] == R.POISON_V).all() and (pi[-7:] == -1).all()
    assert np.array_equal(pv[139 + 67:139 + 134], v[1, 1]) and np.array_equal(pi[:67], i[0, 0])
    x = R.logits_for([23, 0])
    assert x.argmax(1).tolist() == [23, 0] and (x == 4.0).sum(1).tolist() == [3, 3]
    assert np.array_equal(torch.from_numpy(x).bfloat16().float().numpy(), x)


# ------------------------------------------------------------------------------------------------------------------ commit_ref
def _naive_commit(s, toks):
    """one launch, stated once more as a loop over the sequences on flat lists of words, as the device holds them"""
    B, mo = s["B"], s["max_out"]
    nxt, out, step, pos = list(s["next_token"]), [w for row in s["out_tokens"] for w in row], list(s["step"]), list(s["pos"])
    done, eos, rows = None if s["done"] is None else list(s["done"]), s["eos"], list(s["rows"])
    for b in range(B):
        if done is not None and done[b]:
            continue
        tok, at = toks[b] + s["id_offset"], step[b]
        nxt[b] = rows[b] = tok
        if at < mo:
            out[b * mo + at] = tok
        step[b] = at + 1
        pos[b] = pos[b] + (1 if s["advance_pos"] else 0)
        if done is None or eos is None:
            continue
        hit = False
        for k in range(6):
            if k < eos[0] and eos[2 + k] == tok:
                hit = True
        if hit and not (step[b] < eos[1]):
            done[b] = 1
    return dict(next_token=nxt, out_tokens=out, step=step, pos=pos, done=done, rows=rows)


def _flat(s):
    return dict(next_token=s["next_token"], out_tokens=[w for row in s["out_tokens"] for w in row], step=s["step"], pos=s["pos"],
                done=s["done"], rows=s["rows"])


def test_commit_ref_against_the_naive_statement():
    cases = [(n, [t], s) for n, t, s in R.commit_cases()] + [("batched",) + R.commit_batch_case(), ("sampled",) + R.sampled_case()[1:]]
    for name, toks, s in cases:
        before = repr(s)
        assert _flat(R.expected(s, toks)) == _naive_commit(s, toks), name
        assert repr(s) == before, "commit_ref must leave its argument alone"


def test_commit_cases_are_the_listed_ones():
    got = {n: R.expected(s, [t]) for n, t, s in R.commit_cases()}
    init = {n: s for n, _, s in R.commit_cases()}
    T = 23
    for n, e in got.items():
        off, step = init[n]["id_offset"], init[n]["step"][0]
        assert e["next_token"] == [T + off] and e["rows"] == [T + off] and e["step"] == [step + 1], n
        assert e["pos"] == [7 + init[n]["advance_pos"]], n
        stored = [k for k in range(R.MAX_OUT) if e["out_tokens"][0][k] != init[n]["out_tokens"][0][k]]
        assert stored == ([step] if step < R.MAX_OUT else []), n
    done = {n: (e["done"] or [None])[0] for n, e in got.items()}
    for step in (0, 7, 8, 11):
        assert done[f"step {step}, no hit"] == 0 and done[f"step {step}, hit"] == 1
    assert got["advance_pos 0"]["pos"] == [7] and got["advance_pos 1"]["pos"] == [8]
    assert [done[k] for k in ("n_eos 0", "n_eos 1, hit", "n_eos 6, hit at the first", "n_eos 6, hit at the sixth", "n_eos 6, no hit",
                              "n_eos 7, the token in the seventh slot only", "n_eos 2, the token in the third id word")] == [0, 1, 1, 1, 0, 0, 0]
    for step in (0, 3):
        for mn in sorted({0, step, step + 1, step + 2}):
            assert done[f"hit at step {step}, min_new {mn}"] == int(mn <= step + 1)
    assert done["eos given, done null"] is None and done["done given, eos null"] == 0 and done["both null"] is None
    assert done["id_offset: only the offset token matches"] == 1 and done["id_offset: only the raw id matches"] == 0
    toks, s = R.commit_batch_case()
    e = R.expected(s, toks)
    assert e["done"] == [0, 0, 1, 0, 1] and e["step"] == [1, 8, 3, 9, 12] and e["pos"] == [8, 1, 40, 6, 101]
    assert e["rows"] == [23, 24, None, 26, 27] and e["next_token"][2] == s["next_token"][2] and e["out_tokens"][2] == s["out_tokens"][2]
    assert e["out_tokens"][1][7] == 24 and e["out_tokens"][3] == s["out_tokens"][3] and e["out_tokens"][4] == s["out_tokens"][4]
    _, toks, s = R.sampled_case()
    assert R.expected(s, toks)["done"] == [0, 1, 0]


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(lib, rc):
    assert rc != 0 and len(lib.usdm_last_error()) > 0, rc


def test_argmax_final_refuses_bad_arguments():
    from usdm_amd import _lib
    lib = _lib.lib
    words = (ctypes.c_int32 * 16)()
    p = ctypes.cast(words, ctypes.c_void_p)      # a dummy for every pointer: every call below is refused before any launch

    def st(batch=0, **null):
        s = _lib.DecodeState()
        s.next_token, s.out_tokens, s.step, s.pos, s.max_out, s.batch = p, p, p, p, 4, batch
        for k in null:
            setattr(s, k, None)
        return s

    def single(nparts=4, s=None, E=None, Hd=0, h=None):
        return lib.usdm_argmax_final(p, p, ctypes.c_int32(nparts), ctypes.byref(s or st()), E, ctypes.c_int32(Hd), h, None)

    def seg(nparts, nseg, stride, s=None, E=None, Hd=0, h=None):
        return lib.usdm_argmax_final_seg(p, p, ctypes.c_int32(nparts), ctypes.c_int32(nseg), ctypes.c_int64(stride), ctypes.byref(s or st()),
                                         E, ctypes.c_int32(Hd), h, None)

    _refused(lib, single(nparts=0))
    _refused(lib, seg(0, 2, 16))
    _refused(lib, seg(4, 0, 16))
    _refused(lib, seg(4, 2, 3))                       # seg_stride < nparts
    assert b"overlap" in lib.usdm_last_error()
    _refused(lib, seg(4, 2, 11, s=st(batch=3)))       # seg_stride < nparts * batch
    assert b"overlap" in lib.usdm_last_error()
    for batch in (65, -1):
        _refused(lib, single(s=st(batch=batch)))
        _refused(lib, seg(4, 2, 4 * 65, s=st(batch=batch)))
        assert b"batch" in lib.usdm_last_error()
    for Hd, h in ((16, None), (0, p), (12, p)):       # an embedding table without h_out, with Hd = 0, with Hd = 12
        _refused(lib, single(E=p, Hd=Hd, h=h))
        _refused(lib, seg(4, 2, 4, E=p, Hd=Hd, h=h))
        assert b"embedding" in lib.usdm_last_error()
    _refused(lib, single(s=st(step=None)))
    _refused(lib, seg(4, 2, 4, s=st(step=None)))
