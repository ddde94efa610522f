"""Shared references of the speculative-decoding tests (tests/test_spec_*.py): a numpy restatement of usdm_spec_commit (pick, accept,
commit, propose, the ids of the next step's input rows: all int32, so the kernel must equal it word for word) and a float64
multi-row decode attention for usdm_attn_verify (rope in bf16 as HF and the decode kernels do it)."""
import numpy as np
import torch

NO_ID = 0x7fffffff
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ usdm_spec_commit
def pick_row(val, idx):
    """arg-max of one row's partials: the larger value, among equal values the lower id, NaN never wins; nothing -> id 0"""
    bv, bi = -np.inf, NO_ID
    for v, i in zip(np.asarray(val, np.float32).tolist(), np.asarray(idx).tolist()):
        if v > bv or (v == bv and i < bi):
            bv, bi = v, i
    return 0 if bi == NO_ID else int(bi)


def history(s):
    P = min(max(int(s["prompt_len"]), 0), len(s["prompt"]))
    step = min(max(int(s["step"]), 0), len(s["out_tokens"]))
    return [int(t) + s["id_offset"] for t in s["prompt"][:P]] + [int(t) for t in s["out_tokens"][:step]]


def propose(hist, k, lookup_max, lookup_min):
    """prompt lookup: for n from lookup_max down to lookup_min the MOST RECENT earlier occurrence of the last n tokens; the up to k
    tokens behind it, -1 where the history ends or nothing matched"""
    Lh = len(hist)
    for n in range(min(lookup_max, 16), max(lookup_min, 1) - 1, -1):
        if Lh < n + 1:
            continue
        tail = hist[Lh - n:]
        for j in range(Lh - n - 1, -1, -1):
            if hist[j:j + n] == tail:
                return [hist[j + n + i] if j + n + i < Lh else -1 for i in range(k)]
    return [-1] * k


def new_state(T, *, part_val=None, part_idx=None, drafts=(), limit=1 << 30, prompt=(), script=None, lookup=(3, 1), V=1000, max_out=64,
              out_tokens=(), pos=0, next_token=0, done=0, eos=(), min_new=0, id_offset=0, counters=(0, 0, 0), propose_only=False):
    """the words usdm_spec_commit reads, as a dict of Python / numpy values (drafts: the ids fed as rows 1 .. T-1)"""
    d = np.full(8, -1, np.int32)
    d[1:1 + len(drafts)] = drafts
    out = np.zeros(max_out, np.int32)
    out[:len(out_tokens)] = out_tokens
    e = np.zeros(8, np.int32)
    e[0], e[1] = len(eos), min_new
    e[2:2 + len(eos)] = eos
    return dict(T=T, part_val=None if part_val is None else np.asarray(part_val, np.float32),
                part_idx=None if part_idx is None else np.asarray(part_idx, np.int32), drafts=d, limit=int(limit),
                prompt=np.asarray(prompt, np.int32), prompt_len=len(prompt), script=None if script is None else np.asarray(script, np.int32),
                params=np.array([lookup[0], lookup[1], int(script is not None), 0], np.int32), V=V, out_tokens=out, step=len(out_tokens),
                pos=int(pos), next_token=int(next_token), done=int(done), eos=e, id_offset=id_offset,
                counters=np.asarray(counters, np.int32).copy(), propose_only=bool(propose_only))


def from_picks(T, picks, nparts=5, **kw):
    """a state whose row i picks picks[i]: the winner sits in one partial, the others hold lower values and other ids"""
    val = np.full((T, nparts), -1.0, np.float32)
    idx = np.zeros((T, nparts), np.int32)
    for i, g in enumerate(picks):
        idx[i] = [(g + 7 * (j + 1)) % 997 for j in range(nparts)]
        val[i, (i * 3) % nparts], idx[i, (i * 3) % nparts] = 2.0, g
    return new_state(T, part_val=val, part_idx=idx, **kw)


def spec_commit_ref(s):
    """-> the state after one usdm_spec_commit launch (a new dict; `rows`: the token ids of the T rows written to h_out, None when the
    launch returned before writing them)"""
    s = dict(s, drafts=s["drafts"].copy(), out_tokens=s["out_tokens"].copy(), counters=s["counters"].copy(), rows=None)
    T, off = s["T"], s["id_offset"]
    if s["done"]:
        return s
    if not s["propose_only"]:
        g = [pick_row(s["part_val"][i], s["part_idx"][i]) + off for i in range(T)]
        s0, lim = s["step"], min(s["limit"], len(s["out_tokens"]))
        if s0 >= lim:
            s["done"] = 1
            return s
        n = 0
        while n < T - 1 and s["drafts"][n + 1] == g[n]:
            n += 1
        drafted = int((s["drafts"][1:T] >= 0).sum())
        neos, mn = min(int(s["eos"][0]), 6), int(s["eos"][1])
        m, done = 0, 0
        for i in range(n + 1):
            if s0 + m >= lim:
                break
            s["out_tokens"][s0 + m] = g[i]
            m += 1
            if g[i] in s["eos"][2:2 + neos].tolist() and s0 + m >= mn:
                done = 1
                break
        if s0 + m >= lim:
            done = 1
        s["step"], s["pos"], s["next_token"] = s0 + m, s["pos"] + m, int(s["out_tokens"][s0 + m - 1])
        s["done"] = done
        s["counters"] += np.array([1, drafted, m - 1], np.int32)
    step = min(max(s["step"], 0), len(s["out_tokens"]))
    if s["script"] is not None and s["params"][2]:
        d = [int(s["script"][step + i]) if step + i < len(s["out_tokens"]) else -1 for i in range(T - 1)]
    else:
        d = propose(history(s), T - 1, int(s["params"][0]), int(s["params"][1]))
    d = [x if 0 <= x - off < s["V"] else -1 for x in d]
    s["drafts"][1:T] = d
    s["rows"] = [s["next_token"]] + [x if x >= 0 else off for x in d]
    return s


# ------------------------------------------------------------------------------------------------ usdm_attn_verify
def rope_tables(ctx_max):
    from oracle import mistral_oracle as MO
    return MO.rope_tables(dict(head_dim=128, rope_theta=10000.0), torch.arange(ctx_max), BF)


def rope_rows(x, p, tables):
    """HF apply_rotary_pos_emb in bf16 on rows x [n, 128] at position p"""
    from oracle import mistral_oracle as MO
    cosf, sinf = tables
    return (x * cosf[p]) + (MO.rotate_half(x) * sinf[p])


def lo_of(p, window):
    return p + 1 - window if (window > 0 and p + 1 > window) else 0


def attn_verify_ref(qkv, kc, vc, pos, *, Hq, Hkv, window, scale, tables):
    """float64 attention of the T rows of qkv [T, (Hq+2Hkv)*128] (bf16) at positions pos .. pos+T-1 over bf16 caches kc / vc
    [Hkv, ctx_max, 128] whose rows < pos are the context.  -> (out fp64 [Tl, Hq*128], weights fp64 [Tl, Hq, ctx_max] (0 where
    invisible), roped K rows bf16 [Tl, Hkv, 128], V rows bf16 [Tl, Hkv, 128]); Tl = the rows at positions < ctx_max."""
    T, ctx_max, G = qkv.shape[0], kc.shape[1], Hq // Hkv
    Tl = min(T, ctx_max - pos)
    rows = qkv.view(T, Hq + 2 * Hkv, 128)
    K, V = kc.clone(), vc.clone()
    kr = torch.stack([rope_rows(rows[i, Hq:Hq + Hkv], pos + i, tables) for i in range(Tl)])
    vr = rows[:Tl, Hq + Hkv:].clone()
    for i in range(Tl):
        K[:, pos + i], V[:, pos + i] = kr[i], vr[i]
    out = torch.zeros(Tl, Hq * 128, dtype=torch.float64)
    wts = torch.zeros(Tl, Hq, ctx_max, dtype=torch.float64)
    for i in range(Tl):
        p = pos + i
        lo = lo_of(p, window)
        q = rope_rows(rows[i, :Hq], p, tables).double()                       # [Hq, 128]
        Kd = K[:, lo:p + 1].double().repeat_interleave(G, 0)                  # [Hq, n, 128]
        Vd = V[:, lo:p + 1].double().repeat_interleave(G, 0)
        w = torch.softmax((q[:, None] @ Kd.transpose(1, 2))[:, 0] * scale, -1)   # [Hq, n]
        wts[i, :, lo:p + 1] = w
        out[i] = (w[:, None] @ Vd)[:, 0].reshape(-1)
    return out, wts, kr, vr


# ------------------------------------------------------------------------------------------------ shared cases
def hand_cases():
    """(name, state, expected) of the hand-built commit / propose cases: expected = the words a reader can check by eye
    (emitted: the tokens written by this launch)"""
    c = []
    P10 = [5, 6, 7, 8, 5, 6, 9, 5, 6, 7]      # history for the lookup cases
    add = lambda name, st, **exp: c.append((name, st, exp))
    # accept counts
    add("no draft matches", from_picks(4, [11, 12, 13, 14], drafts=[1, 2, 3], out_tokens=[3]), emitted=[11], accepted=0, drafted=3)
    add("first of three", from_picks(4, [11, 12, 13, 14], drafts=[11, 2, 13], out_tokens=[3]), emitted=[11, 12], accepted=1)
    add("all three", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3]), emitted=[11, 12, 13, 14], accepted=3)
    add("a later match does not count", from_picks(4, [11, 12, 13, 14], drafts=[9, 12, 13], out_tokens=[3]), emitted=[11], accepted=0)
    add("-1 drafts never match", from_picks(4, [11, 0, 0, 0], drafts=[11, -1, -1], out_tokens=[3]), emitted=[11, 0], accepted=1, drafted=1)
    add("T = 1 is the plain step", from_picks(1, [42], out_tokens=[3, 4]), emitted=[42], accepted=0, drafted=0)
    add("T = 8, seven accepted", from_picks(8, list(range(20, 28)), drafts=list(range(20, 27)), out_tokens=[1]), emitted=list(range(20, 28)), accepted=7)
    # stop ids, min_new, limits
    add("stop id inside the accepted run", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], eos=[12]),
        emitted=[11, 12], done=1, accepted=1)
    add("stop id under min_new is passed", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], eos=[12], min_new=4),
        emitted=[11, 12, 13, 14], done=0)
    add("stop id exactly at min_new", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], eos=[12], min_new=3),
        emitted=[11, 12], done=1)
    add("second stop id of two", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], eos=[99, 13]), emitted=[11, 12, 13], done=1)
    add("limit cuts the run", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], limit=3), emitted=[11, 12], done=1, accepted=1)
    add("max_out cuts the run", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3] * 6, max_out=8), emitted=[11, 12], done=1)
    add("no room on entry", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3, 4], limit=2), emitted=[], done=1, steps=0)
    add("done on entry", from_picks(4, [11, 12, 13, 14], drafts=[11, 12, 13], out_tokens=[3], done=1), emitted=[], steps=0)
    # ties and empty rows
    tie = new_state(2, part_val=[[1.0, 3.0, 3.0, -np.inf], [np.nan, 2.0, 2.0, 2.0]], part_idx=[[5, 9, 7, NO_ID], [1, 30, 20, 40]],
                    drafts=[7], out_tokens=[3])
    add("ties go to the lowest id, NaN never wins", tie, emitted=[7, 20], accepted=1)
    none = new_state(2, part_val=[[-np.inf] * 3] * 2, part_idx=[[NO_ID] * 3] * 2, drafts=[0], out_tokens=[3])
    add("no candidate is id 0", none, emitted=[0, 0], accepted=1)
    add("id_offset", from_picks(2, [11, 12], drafts=[111], out_tokens=[103], id_offset=100, prompt=[1, 2]), emitted=[111, 112], accepted=1)
    # the proposer (propose_only: the history is prompt + out_tokens as they stand)
    pr = lambda T, prompt, out, **kw: new_state(T, prompt=prompt, out_tokens=out, propose_only=True, next_token=(out or prompt)[-1], **kw)
    add("no match", pr(4, [1, 2, 3], [4]), drafts=[-1, -1, -1])
    add("two matches, the most recent wins", pr(4, P10[:7], [5, 6]), drafts=[9, 5, 6])
    add("longest n first", pr(4, P10, []), drafts=[8, 5, 6])
    add("n = 1 only", pr(4, P10, [], lookup=(1, 1)), drafts=[8, 5, 6])
    add("lookup_min above the only match", pr(4, [1, 2, 3, 9, 3], [], lookup=(3, 2)), drafts=[-1, -1, -1])
    add("continuation runs off the end", pr(4, [1, 2, 3, 4, 3], [4]), drafts=[3, 4, -1])
    add("history shorter than n", pr(3, [7], [7], lookup=(3, 3)), drafts=[-1, -1])
    add("history of one", pr(3, [], [7]), drafts=[-1, -1])
    add("script replaces the lookup", pr(4, P10, [5, 6], script=[0, 0, 31, 32, 33, 34] + [0] * 58), drafts=[31, 32, 33])
    add("script runs off max_out", pr(4, [1], [5] * 7, script=[9] * 8, max_out=8), drafts=[9, -1, -1])
    add("ids outside the vocabulary are no drafts", pr(4, [1], [5], script=[0, 1000, -5, 999] + [0] * 60), drafts=[-1, -1, 999])
    add("commit then propose from the new history", from_picks(3, [6, 7, 1], drafts=[6, 2], prompt=P10[:4], out_tokens=[5]),
        emitted=[6, 7], drafts=[8, 5])
    return c


def random_case(seed):
    """a seeded random state: small vocabulary so that drafts match, stop ids, limits and histories of every kind"""
    g = np.random.default_rng(seed)
    T = int(g.choice([2, 4, 8]))
    V, nparts, max_out = 12, int(g.integers(1, 7)), int(g.integers(4, 40))
    nout = int(g.integers(1, max_out + 1))
    picks = g.integers(0, V, T)
    drafts = np.where(g.random(T - 1) < 0.6, picks[:T - 1], g.integers(-1, V, T - 1))
    val = g.integers(-3, 3, (T, nparts)).astype(np.float32)
    idx = g.integers(0, V, (T, nparts)).astype(np.int32)
    for i in range(T):
        if g.random() < 0.7:
            j = int(g.integers(0, nparts))
            val[i, j], idx[i, j] = 5.0, picks[i]
    use_script = g.random() < 0.3
    return new_state(T, part_val=val, part_idx=idx, drafts=drafts.tolist(), limit=int(g.integers(1, max_out + 4)),
                     prompt=g.integers(0, V, int(g.integers(0, 30))).tolist(), script=g.integers(-1, V + 1, max_out).tolist() if use_script else None,
                     lookup=(int(g.integers(1, 5)), int(g.integers(1, 3))), V=V, max_out=max_out, out_tokens=g.integers(0, V, nout).tolist(),
                     pos=int(g.integers(0, 100)), next_token=int(g.integers(0, V)), done=int(g.random() < 0.05),
                     eos=g.integers(0, V, int(g.integers(0, 3))).tolist(), min_new=int(g.integers(0, max_out)),
                     counters=g.integers(0, 50, 3).tolist())


def emitted(before, after):
    return after["out_tokens"][before["step"]:after["step"]].tolist()


# ------------------------------------------------------------------------------------------------ the model tests' fixed inputs
SMALL_CFG = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                 num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=32768)
MODEL_SEED, PROMPT_SEED, PROMPT_LEN = 7, 11, 24
NEW = 49                      # the prefill's pick + 48 tokens from speculative steps
LOOKUP_KEEP = (17, 401, 888)  # the lookup test's ban mask allows these three ids only
LOOKUP_K = 3


def small_prompt():
    return torch.randint(0, SMALL_CFG["vocab_size"], (PROMPT_LEN,), generator=torch.Generator().manual_seed(PROMPT_SEED))


def lookup_bad_words():
    return [[i] for i in range(SMALL_CFG["vocab_size"]) if i not in LOOKUP_KEEP]


def simulate_lookup(prompt, output, k, lookup_max=3, lookup_min=1):
    """The speculative steps over a FIXED greedy output (the ids do not depend on the drafts): output[0] is the prefill's pick, every
    step proposes from prompt + the output so far and accepts the leading drafts that equal the output.  -> (steps, drafted, accepted)"""
    s, steps, drafted, accepted = 1, 0, 0, 0
    while s < len(output):
        d = propose(list(prompt) + list(output[:s]), k, lookup_max, lookup_min)
        n = 0
        while n < k and s + n < len(output) and d[n] == output[s + n]:
            n += 1
        m = min(n + 1, len(output) - s)
        steps, drafted, accepted, s = steps + 1, drafted + sum(x >= 0 for x in d), accepted + m - 1, s + m
    return steps, drafted, accepted
