"""The decode slots: B sequences that decode in lockstep (generate_batch, serving.LLM's continuous batching, beam search) - their
buffers and the host protocol around them: which knob block is written when, where an idle slot is parked, which arrays make up "the
cache".  The model (usdm_amd/llm.py) states the launches; the schedulers talk to the methods here.  What a step kind adds (log-probability
rows, penalty tables, logit-edit state) is built here for the single sequence too (B=None)."""
from collections import deque

import torch

from . import ops
from .plancache import LRU
from .prefix import PrefixIndex

CHUNK = 8           # decode steps between two scheduling points (host sync: stop checks, slot turnover)
NO_CANDIDATE_IDX = 0x7fffffff      # the id of an arg-max partial that saw no allowed row
GREEDY_KNOBS = (1.0, 1, 1.0, 0)      # temperature, top_k, top_p, seed: greedy on the sampling step (top_k = 1); harmless on an idle slot


def stop_index(toks, stops, min_new):
    """How many of `toks` a sequence keeps when it ends at its first stop id that is at least its min_new-th token; None: no stop."""
    return next((i + 1 for i, t in enumerate(toks) if t in stops and i + 1 >= min_new), None)


def stop_block(stops, min_new):
    """The device stop block {n, min_new, ids...} of a sequence that ends at one of `stops` -> (its 8 int32 words, the ids the device
    checks: sorted; none where there are more than the block's 6, which leaves the check to the host)."""
    dev = sorted(stops) if len(stops) <= 6 else []
    return torch.tensor(([len(dev), int(min_new)] + dev + [0] * 6)[:8], dtype=torch.int32), dev


def penalty_buffers(device, V, B=None):
    """usdm_penalize's state for one sequence (B=None: plus its tokens-counted word) or B batch slots: the table of V words per
    sequence (count of generated occurrences, bit 30 = in the prompt) and the device block of the knobs (zero-filled = neutral)."""
    lead = () if B is None else (B,)
    bufs = dict(table=torch.zeros(*lead, V, dtype=torch.int32, device=device), dev_params=ops.penalty_params_tensor(device, B or 1).view(*lead, -1))
    if B is None:
        bufs["count"] = torch.zeros(1, dtype=torch.int32, device=device)
    return bufs


def seed_penalties(bufs, prompt_ids, knobs):
    """A new request for this sequence / slot: its knobs, an empty table with every prompt id flagged (prompt ids whose K/V were
    reused from the cache included), nothing counted yet.  Plain torch calls, outside the captured graphs."""
    ops.set_penalty_params(bufs["dev_params"], *(knobs or ops.PENALTY_NEUTRAL))
    tbl = bufs["table"]
    tbl.zero_()
    tbl[prompt_ids.to(tbl.device, torch.long)] = ops.PENALTY_PROMPT_BIT
    if "count" in bufs:
        bufs["count"].zero_()


def edit_buffers(device, ctx_max, B=None):
    """usdm_logit_edit's state for one sequence (B=None) or B batch slots: the device block of the knobs (zero-filled = neutral), the
    bias rows of ops.LOGIT_BIAS_MAX entries and the prompt row of ctx_max ids."""
    lead = () if B is None else (B,)
    return dict(dev_params=ops.edit_params_tensor(device, B or 1).view(*lead, -1),
                bias_id=torch.zeros(*lead, ops.LOGIT_BIAS_MAX, dtype=torch.int32, device=device),
                bias_val=torch.zeros(*lead, ops.LOGIT_BIAS_MAX, dtype=torch.float32, device=device),
                prompt=torch.zeros(*lead, ctx_max, dtype=torch.int32, device=device))


def seed_edits(bufs, prompt_ids, knobs):
    """A new request for this sequence / slot: its bias list, n-gram size and prompt (ids whose K/V were reused from the cache
    included); knobs = check_edits()'s (bias, n) or None: a request without, neutral.  Plain torch calls, outside the captured graphs."""
    bias, n = knobs or ((), 0)
    P = int(prompt_ids.shape[0]) if n else 0      # (the bias needs no history)
    if P > bufs["prompt"].shape[-1]:
        raise ValueError(f"the prompt of {P} ids does not fit the prompt row of {bufs['prompt'].shape[-1]}")
    if bias:
        bufs["bias_id"][:len(bias)] = torch.tensor([i for i, _ in bias], dtype=torch.int32)
        bufs["bias_val"][:len(bias)] = torch.tensor([v for _, v in bias], dtype=torch.float32)
    if P:
        bufs["prompt"][:P] = prompt_ids.to(bufs["prompt"].device, torch.int32)
    ops.set_edit_params(bufs["dev_params"], n, P, len(bias))


class TokenLogprobs:
    """Log-probabilities of one generated sequence of n tokens (host tensors): token_logprobs [n] f32 and ranks [n] i32 of the picked
    tokens, top_ids [n][K] i32 / top_logprobs [n][K] f32 in descending log-probability (exact ties: lowest id first), cumulative = the
    float64 sum of token_logprobs.  lp(i) = x_i - logsumexp(x) over the ban-masked logits row the token was picked from: the model's
    distribution over the allowed ids, before temperature / top-k / top-p (usdm_logprobs)."""
    __slots__ = ("token_logprobs", "ranks", "top_ids", "top_logprobs", "cumulative")

    def __init__(self, token_logprobs, ranks, top_ids, top_logprobs):
        self.token_logprobs, self.ranks, self.top_ids, self.top_logprobs = token_logprobs, ranks, top_ids, top_logprobs
        self.cumulative = float(token_logprobs.double().sum())

    def trimmed(self, n, k):
        """The first n tokens with the k most likely ids each (a request served inside a group whose step carries a larger K)"""
        return TokenLogprobs(self.token_logprobs[:n], self.ranks[:n], self.top_ids[:n, :k], self.top_logprobs[:n, :k])


def logprob_buffers(device, max_out, B=None):
    """The four output buffers of usdm_logprobs for one sequence (B=None: plus its rows-written count) or B batch slots, sized for
    K = 20 so that K never re-allocates; the kernel addresses the top lists as [max_out][K]."""
    lead = () if B is None else (B,)
    z = lambda n, dt: torch.zeros(*lead, n, dtype=dt, device=device)
    bufs = dict(tok_lp=z(max_out, torch.float32), tok_rank=z(max_out, torch.int32), top_id=z(max_out * ops.LOGPROBS_MAX_K, torch.int32),
                top_lp=z(max_out * ops.LOGPROBS_MAX_K, torch.float32))
    if B is None:
        bufs["count"] = torch.zeros(1, dtype=torch.int32, device=device)
    return bufs


def read_logprobs(bufs, n, K, b=None):
    """Rows 0 .. n-1 of a sequence's log-probability buffers (slot b of a batch's) as a TokenLogprobs on the host."""
    row = (lambda t: t) if b is None else (lambda t: t[b])
    top = lambda t: row(t)[:n * K].view(n, K).cpu()
    return TokenLogprobs(row(bufs["tok_lp"])[:n].cpu(), row(bufs["tok_rank"])[:n].cpu(), top(bufs["top_id"]), top(bufs["top_lp"]))


class _Slot:
    """Views of the slots' buffers that stand in for the model's single-sequence attributes during a per-item prefill (batch = 0), or,
    as the "all" view, during the lm_head + pick of the batched step (batch = B).  No device-side end of sequence."""
    batch, st_done, st_eos = 0, None, None


class DecodeSlots:
    """B slots in lockstep on `model` (its shapes, weights and plan builders): caches kc / vc (fp8 cache: + exponents ke / ve), decode
    state nxt / step / pos / out, input rows h, arg-max partials pv / pi, logits rows, sample knobs sp; `slots` the per-slot views and
    `all` the whole batch's; `prefill` the slots' prefill plans (an LRU keyed (S, past, slot, *kind)), `steps` the decode step per kind.
    lp / pen / edt (require()) and prefix (the PrefixIndex of enable_prefix_caching) are None until a step kind or the option needs them."""

    def __init__(self, model, B):
        m, c, dev, bf = model, model.cfg, model.device, torch.bfloat16
        L, d, H = c["num_hidden_layers"], c["head_dim"], c["hidden_size"]
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        rows = lambda: torch.zeros(B, L, m.Hkv, m.ctx_max, d, dtype=torch.uint8 if m.kv8 else bf, device=dev)
        exps = lambda: torch.zeros(B, L, m.Hkv, m.ctx_max, dtype=torch.int8, device=dev) if m.kv8 else None      # fp8 cache: one exponent per row
        self.model, self.B = m, B
        self.kc, self.vc, self.ke, self.ve = rows(), rows(), exps(), exps()
        self.nxt, self.step, self.pos, self.out = i32(B), i32(B), i32(B), i32(B, m.max_out)
        self.h = torch.zeros(B, H, dtype=bf, device=dev)
        self.pv, self.pi, self.logits = f32(B, m.nparts), i32(B, m.nparts), f32(B, m.Vloc)
        self.sp = ops.sample_params_tensor(dev, B).view(B, -1)
        self.prefill, self.steps = LRU(16), {}
        self.lp = self.pen = self.edt = self.prefix = None
        self.pvg = self.pig = self.pvs = self.pis = self.lg = self.lrow = None
        if m.tp_path:
            # tensor parallel: pv / pi hold THIS rank's partials; the decode step gathers them rank-major into pvg / pig
            # [rank][sequence][nparts] (usdm_argmax_final_seg), a slot's prefill into its own row of pvs / pis [sequence][rank * nparts]
            tp = m.tp_size
            self.pvg, self.pig, self.pvs, self.pis = f32(tp, B, m.nparts), i32(tp, B, m.nparts), f32(B, tp * m.nparts), i32(B, tp * m.nparts)
            # sampled: the ranks' [B][Vloc] logits gathered rank-major into lg [rank][sequence][Vloc] (usdm_sample_final_seg); a
            # slot's sampled prefill gathers its row into lrow [tp * Vloc] (prefills run one at a time)
            self.lg, self.lrow = f32(tp, B, m.Vloc), f32(tp * m.Vloc)
        if m.prefix_caching:      # the index (usdm_amd/prefix.py) and the three device words of its usdm_kv_reorder copies
            self.prefix, self.px_parent, self.px_lo, self.px_pos = PrefixIndex(B, m.ctx_max, CHUNK), i32(B), i32(1), i32(1)
        self.slots = []
        for b in range(B):
            sl = _Slot()
            sl.kcache, sl.vcache = self.kc[b], self.vc[b]
            sl.kexp, sl.vexp = (self.ke[b], self.ve[b]) if m.kv8 else (None, None)
            sl.st_next, sl.st_step, sl.st_pos, sl.st_out = self.nxt[b:b + 1], self.step[b:b + 1], self.pos[b:b + 1], self.out[b]
            sl.h_dec = self.h[b]
            sl.part_val_loc, sl.part_idx_loc = self.pv[b], self.pi[b]
            sl.part_val, sl.part_idx = (self.pvs[b], self.pis[b]) if m.tp_path else (self.pv[b], self.pi[b])
            sl.logits, sl.sample_params, sl.logits_row = self.logits[b], self.sp[b], self.lrow
            self.slots.append(sl)
        al = self.all = _Slot()      # the whole batch, for the batched step's lm_head + pick
        al.batch, al.st_next, al.st_step, al.st_pos, al.st_out, al.h_dec = B, self.nxt, self.step, self.pos, self.out, self.h
        al.part_val_loc, al.part_idx_loc = self.pv, self.pi
        al.part_val, al.part_idx = (self.pvg, self.pig) if m.tp_path else (self.pv, self.pi)
        al.logits, al.sample_params, al.logits_row = self.logits, self.sp, self.lg

    def require(self, kind):
        """What a step of this kind needs beyond the sampler's state (allocated at first use): lp, the slots' log-probability buffers
        next to `out`, pen, their penalty state, and edt, their logit-edit state; every slot views its own row as sl.lp / sl.pen /
        sl.edt.  No rows-written / tokens-counted word: batch slots have no device-side `done` word, every step writes its row and
        counts the token of the step before, and the host ignores rows past a request's end."""
        m, new = self.model, {}
        if kind.logprobs is not None and self.lp is None:
            new["lp"] = logprob_buffers(m.device, m.max_out, self.B)
        if kind.penalties and self.pen is None:
            new["pen"] = penalty_buffers(m.device, m.cfg["vocab_size"], self.B)
        if kind.edits and self.edt is None:
            new["edt"] = edit_buffers(m.device, m.ctx_max, self.B)
        for name, bufs in new.items():
            setattr(self, name, bufs)
            setattr(self.all, name, bufs)
            for b, sl in enumerate(self.slots):
                setattr(sl, name, {k: v[b] for k, v in bufs.items()})

    def step_plan(self, kind):
        """The replayable decode step of the slots (built at first use), a plan / graph of its own per kind: greedy, sampled, the
        sampled step followed by usdm_logprobs (per K), and each of the latter two with usdm_logit_edit and / or usdm_penalize in front
        of the pick."""
        self.require(kind)
        if kind not in self.steps:
            self.steps[kind] = self.model._graphed(self.model._build_decode_batch(self.B, *kind))
        return self.steps[kind]

    def admit(self, b, ids, kind, knobs=None, edits=None, sampling=None):
        """Admit a prompt (ids [L]) into slot b, whose batch runs on the step `kind`: its sample knobs (sampling = (temperature, top_k,
        top_p, seed, min_p); None: greedy, which the arg-max step never reads and is spared), its step / position counters, then the
        per-item prefill into the slot's cache, which also picks the first token as that step would (sampled; with row 0 of the slot's
        log-probabilities).  On the penalised step the slot's table is reset and seeded from the prompt and the request's knobs; on the
        step with logit edits its edit state is written from the prompt and the request's check_edits() value (None: neutral, both).
        Returns (source slot, past): the rows [0, past) reused instead of prefilled and their slot (_reuse), or (None, 0)."""
        m, L = self.model, int(ids.shape[0])
        self.require(kind)
        if kind.sampling or sampling is not None:
            ops.set_sample_params(self.sp[b], *(sampling or GREEDY_KNOBS))
        self.step[b] = 0
        self.pos[b] = L
        if kind.penalties:
            seed_penalties(self.slots[b].pen, ids, knobs)
        if kind.edits:
            seed_edits(self.slots[b].edt, ids, edits)
        src, past = self._reuse(b, ids) if m.prefix_caching else (None, 0)
        S = L - past
        segs, io = self.prefill.get_or_build((S, past, b, *kind), lambda: m._build_prefill(S, kind.sampling or None, slot=self.slots[b], past=past,
                                                                                           logprobs=kind.logprobs, penalties=kind.penalties,
                                                                                           edits=kind.edits))
        io["ids"].copy_(ids[past:])
        m._run_segs(segs)
        return src, past

    def _reuse(self, b, ids):
        """enable_prefix_caching: the slots' rows that the prompt `ids`, about to be prefilled into slot b, can reuse -> (source slot or
        None, past).  Rows [0, past) of another slot are copied into slot b (usdm_kv_reorder with parent[b] = source and the identity
        elsewhere, lo = 0, pos = past: K, V and the fp8 cache's exponents in one launch); slot b's entry becomes the prompt.  Counted
        in model.stats: prefix_hits, prefix_rows_reused, prefix_copies, prefill_rows."""
        m, prompt = self.model, ids.tolist()
        src, past = self.prefix.match(prompt, b)
        copied = src is not None and src != b
        if copied:
            self.px_parent.copy_(torch.tensor([src if s == b else s for s in range(self.B)], dtype=torch.int32))
            self.px_pos.fill_(past)
            ops.kv_reorder(self.cache_arrays(), self.px_parent, self.px_lo, self.px_pos, B=self.B, nblk=m.cfg["num_hidden_layers"] * m.Hkv, ctx_max=m.ctx_max)
        self.prefix.admit(b, prompt)
        for k, v in (("prefix_hits", int(past > 0)), ("prefix_rows_reused", past), ("prefix_copies", int(copied)), ("prefill_rows", len(prompt) - past)):
            m.stats[k] = m.stats.get(k, 0) + v
        return src, past

    def reset_knobs(self, b):
        """Slot b is idle and keeps decoding garbage: greedy sample knobs, neutral penalty and edit knobs where those are allocated."""
        ops.set_sample_params(self.sp[b], *GREEDY_KNOBS)
        if self.pen is not None:
            ops.set_penalty_params(self.pen["dev_params"][b])
        if self.edt is not None:
            ops.set_edit_params(self.edt["dev_params"][b])

    def park(self, b):
        """Idle slot b decodes garbage into row 0 of its own cache - with enable_prefix_caching behind the rows its index records, which
        the garbage would destroy (the idle slot's attention then runs over those rows)."""
        self.step[b] = 0
        self.pos[b] = self.prefix.park(b) if self.model.prefix_caching else 0

    def tokens(self, n=None):
        """The slots' first n (None: all max_out) output ids as lists: the host sync of a scheduling point."""
        return self.out[:, :n].tolist()

    def logprobs(self, b, n, K):
        """Rows 0 .. n-1 of slot b's log-probabilities, read before a refill restarts the slot's step at 0 and overwrites them."""
        return read_logprobs(self.lp, n, K, b)

    def cache_arrays(self):
        """Every array that holds cache rows [B][layers x kv heads][ctx_max][...]: what usdm_kv_reorder moves between slots."""
        return [self.kc, self.vc] + ([self.ke, self.ve] if self.model.kv8 else [])

    def reset_prefix(self):
        """Forget every reusable row (nothing on the device changes)."""
        if self.prefix is not None:
            self.prefix.reset()


class BeamSlots(DecodeSlots):
    """The state of a search with B beams and n_eos EOS ids, in a cache of its own (generate_batch's slots and plans
    are not touched): the B slots plus the running scores, the parents, the EOS ids, `lo` (first cache row the reorder moves),
    usdm_beam_step's scratch and its step log [max_out][KC]; per prompt length one prefill plan; the step, eager and captured."""

    def __init__(self, model, B, n_eos):
        super().__init__(model, B)
        dev, KC, T = model.device, ops.beam_candidates(B, n_eos), model.max_out
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.n_eos, self.KC, self.score, self.parent, self.eos, self.lo = n_eos, KC, f32(B), i32(B), i32(ops.BEAM_MAX_EOS), i32(1)
        self.cand_score, self.cand_index = f32(B, KC), i32(B, KC)
        self.log_score, self.log_token, self.log_parent = f32(T, KC), i32(T, KC), i32(T, KC)
        self.beam_graph = self.beam_eager = None


class SpecState:
    """The host side of speculative greedy decoding for n sequences on `model`: per sequence the words of
    usdm_spec_commit - drafts [8], limit, the prompt row, a script row, the three counters - and the shared lookup params; per
    T = k + 1 the n * T rows the step runs on (h, the arg-max partials), the captured step (model._build_spec_step) and the
    one-sequence propose_only launches.  A holder adds where its sequences live, as the step's two launches that differ:
    attn(l, qkv, pm, pl, po, ao, **shape), the verify attention of layer l on its caches, and commit(T, plan, b, propose_only), the
    commit over all its sequences (b = None) or sequence b alone, on its decode state.
    Sampled requests: per T also the rows' f32 logits and their picks (sample_rows), a second captured step under
    (T, "sampled"), and from the holder sample_block(), its sequences' usdm_sample_params [n][24], and step_words(), their step and
    done words, which usdm_spec_sample reads."""

    def __init__(self, model, n=1):
        i32 = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device=model.device)
        self.model, self.n = model, n
        self.drafts, self.limit, self.counters, self.params = i32(n, ops.SPEC_MAX_T, v=-1), i32(n), i32(n, 3), i32(4)
        self.prompt, self.prompt_len, self.script = i32(n, model.ctx_max), i32(n), i32(n, model.max_out, v=-1)
        self.rows, self.spec_steps, self.inits = {}, {}, {}

    def spec_rows(self, T):
        """h [n*T][H] and the arg-max partials [n*T][nparts] of the step with T rows per sequence"""
        if T not in self.rows:
            m, rows = self.model, self.n * T
            self.rows[T] = dict(h=torch.zeros(rows, m.cfg["hidden_size"], dtype=torch.bfloat16, device=m.device),
                                pv=torch.full((rows, m.nparts), float("-inf"), dtype=torch.float32, device=m.device),
                                pi=torch.full((rows, m.nparts), NO_CANDIDATE_IDX, dtype=torch.int32, device=m.device))
        return self.rows[T]

    def sample_rows(self, T):
        """What the SAMPLED step with T rows per sequence adds (allocated at first use): the rows' f32 logits
        [n*T][Vloc], which the lm_head materialises, and their picks [n*T], usdm_spec_sample's draws"""
        r = self.spec_rows(T)
        if "logits" not in r:
            m, rows = self.model, self.n * T
            r["logits"] = torch.zeros(rows, m.Vloc, dtype=torch.float32, device=m.device)
            r["picks"] = torch.zeros(rows, dtype=torch.int32, device=m.device)
        return r

    def commit_words(self, T, sampled=False):
        """What both commit launches take besides their decode state: the rows' partials (sampled: their picks too) and the words above"""
        m, r = self.model, self.sample_rows(T) if sampled else self.spec_rows(T)
        return (r["pv"], r["pi"], m.nparts), dict(T=T, drafts=self.drafts, limit=self.limit, prompt=self.prompt, prompt_len=self.prompt_len,
                                                  params=self.params, counters=self.counters, V=m.cfg["vocab_size"], script=self.script,
                                                  embed=m.W["embed"], h_out=r["h"], Hd=m.cfg["hidden_size"],
                                                  **(dict(picks=r["picks"]) if sampled else {}))

    def sample(self, T, plan):
        """usdm_spec_sample over the n * T logits rows of the sampled step: row b * T + i drawn with sequence b's knobs (the holder's
        sample_block(): [n][24]) at the holder's step[b] + i, sequences that are done and rows behind a -1 draft skipped"""
        r, (step, done) = self.sample_rows(T), self.step_words()
        ops.spec_sample(r["logits"], r["picks"], T=T, n=self.n, dev_params=self.sample_block(), step=step, done=done, drafts=self.drafts,
                        V=self.model.v1 - self.model.v0, plan=plan)

    def spec_step(self, T, sampled=False):
        """The replayable speculative step of the n sequences x T rows (built and captured at first use); sampled: the variant
        whose picks are drawn (usdm_spec_sample), a graph of its own under the key (T, "sampled")"""
        key = (T, "sampled") if sampled else T
        if key not in self.spec_steps:
            self.spec_steps[key] = self.model._graphed(self.model._build_spec_step(self, T, sampled))
        return self.spec_steps[key]

    def set_lookup(self, lookup_max, lookup_min, use_script):
        self.params.copy_(torch.tensor([lookup_max, lookup_min, int(bool(use_script)), 0], dtype=torch.int32))

    def seed(self, b, ids, limit, script=None):
        """A new request for sequence b behind its prefill: limit, the prompt row (ids [L]), zeroed counters, no drafts, the script
        (cut at max_out; None: none)."""
        m, L = self.model, int(ids.shape[0])
        self.limit[b] = int(limit)
        self.prompt[b, :L] = ids.to(m.device, torch.int32)
        self.prompt_len[b] = L
        self.counters[b] = 0
        self.drafts[b] = -1
        self.script[b] = -1
        if script is not None:
            sc = torch.as_tensor(script).to(torch.int32).reshape(-1)[:m.max_out]
            self.script[b, :sc.numel()] = sc.to(m.device)

    def propose(self, T, b):
        """Sequence b's first drafts and input rows behind its prefill, whose pick is already committed: a propose_only commit of
        that sequence alone (one plan per (T, b), built at first use)"""
        if (T, b) not in self.inits:
            self.inits[T, b] = ops.Plan()
            self.commit(T, self.inits[T, b], b, propose_only=True)
        self.inits[T, b].run()

    def stats(self, b):
        """Sequence b's counters: the speculative steps, the drafts fed (ids, not the -1 of "no draft") and the drafts accepted"""
        c = self.counters[b].tolist()
        return dict(steps=c[0], drafted=c[1], accepted=c[2])


class SpecSequence(SpecState):
    """The single sequence's speculative state (n = 1): the model's own caches, decode state and prefix bookkeeping."""

    def attn(self, l, qkv, *bufs, **kw):
        m = self.model
        ops.attn_verify(qkv, m.st_pos, m.cos, m.sin, m.kcache[l], m.vcache[l], *bufs, skip=m.st_done, **kw)

    def commit(self, T, plan, b=None, propose_only=False, sampled=False):
        """usdm_spec_commit over the T rows: the end of the step, or (propose_only) the first drafts and the first T input rows;
        sampled: usdm_spec_commit_picks on the rows' draws"""
        m, (parts, words) = self.model, self.commit_words(T, sampled)
        st = ops.decode_state(m.st_next, m.st_out, m.st_step, m.st_pos, advance_pos=True, done=m.st_done, eos=m.st_eos)
        ops.spec_commit(*parts, st, **words, propose_only=propose_only, plan=plan)
        plan.hold(st)

    def sample_block(self):
        """The call's knobs and seed: the single sequence's sampler block, which generate() writes and the prefill's pick reads"""
        return self.model.sample_params.view(1, -1)

    def step_words(self):
        return self.model.st_step, self.model.st_done


class SpecSlots(DecodeSlots, SpecState):
    """B slots of batched speculative greedy decoding, in a cache of their own (generate_batch's slots and plans are not
    touched): the B slots plus SpecState's words with n = B and, per slot, done and a stop block {n, min_new, ids}; one prefill plan
    cache (DecodeSlots').  A slot without a request has done = 1: the verify attention skips it and the commit changes nothing, so it
    never decodes garbage and needs no parking.  Not on a model with enable_prefix_caching (whose index protocol assumes parked,
    decoding idle slots)."""

    def __init__(self, model, B, kind):
        if model.prefix_caching:
            raise NotImplementedError("batched speculative decoding on a model built with enable_prefix_caching=True: the prefix index "
                                      "assumes idle slots are parked and decoding; the single-sequence speculative path works there")
        DecodeSlots.__init__(self, model, B)
        SpecState.__init__(self, model, B)
        self.kind = kind      # llm.step_kind(): the ban-masked arg-max pick of the slots' prefills
        self.done = torch.ones(B, dtype=torch.int32, device=model.device)
        self.eos = torch.zeros(B, 8, dtype=torch.int32, device=model.device)

    def attn(self, l, qkv, *bufs, **kw):
        m = self.model
        ops.attn_verify_batch(qkv, self.pos, m.cos, m.sin, self.kc[0, l], self.vc[0, l], *bufs, B=self.B, cache_bs=self.kc.stride(0),
                              skip=self.done, **kw)

    def sample_block(self):
        """Per-slot knobs and seeds: the slots' sampler blocks, which admit() writes and a slot's prefill pick reads"""
        return self.sp

    def step_words(self):
        return self.step, self.done

    def commit(self, T, plan, b=None, propose_only=False, sampled=False):
        """usdm_spec_commit_batch over all slots or (b) slot b alone: the end of the step, or (propose_only) an admitted slot's first
        drafts and input rows; sampled: usdm_spec_commit_batch_picks on the rows' draws"""
        parts, words = self.commit_words(T, sampled)
        st = ops.decode_state(self.nxt, self.out, self.step, self.pos, advance_pos=True, batch=self.B, done=self.done, eos=self.eos)
        st.max_out = self.model.max_out
        lo, n = (0, None) if b is None else (b, 1)
        ops.spec_commit_batch(*parts, st, **words, slot_lo=lo, n=n, propose_only=propose_only, plan=plan)
        plan.hold(st)

    def admit_spec(self, b, ids, T, limit, stops=(), min_new=0, script=None, sampled=False, sampling=None):
        """Admit a prompt (ids [L]) into slot b: DecodeSlots.admit's per-slot prefill, whose pick is committed as step 1, then the
        slot's stop block (the host checks every id anyway), its speculative words (seed), done = 0, and its first drafts and input
        rows (propose).  sampled (the slots run the sampled step): the prefill is the sampling kind's, so the first
        token is usdm_sample_final's draw at counter 0 with the slot's knobs - sampling = (temperature, top_k, top_p, seed, min_p), or
        None: a greedy request, which carries top_k = 1."""
        if sampled:
            self.admit(b, ids, self.kind._replace(sampling=True), sampling=sampling or GREEDY_KNOBS)
        else:
            self.admit(b, ids, self.kind)
        self.eos[b] = stop_block(stops, min_new)[0]
        self.seed(b, ids, limit, script)
        self.done[b] = 0
        self.propose(T, b)

    def release(self, b):
        """Slot b has no request: every launch of the step leaves it alone"""
        self.done[b] = 1

    def serve(self, requests, T, stops_of=None, sampled=False):
        """Run `requests` - dicts with ids [L] (a tensor), limit (tokens to emit, <= ctx_max - L and max_out), stops (a set), min_new
        and optionally script and (sampled: the sampled step; a request without is greedy inside it) sampling = (temperature, top_k,
        top_p, seed, min_p) - through the slots with turnover: a finished slot is refilled from the queue at the next scheduling
        point.  The captured step is replayed in chunks; the host reads step / done / out at each scheduling point and never
        runs more replays than the slot with the most tokens left needs at one token per step.  Replays past a slot's device-side
        stop change nothing of that slot.  -> ([(tokens, dict(steps=, drafted=, accepted=)) per request], most slots active at once)"""
        step = self.spec_step(T, sampled)
        queue, slots, results, max_active = deque(enumerate(requests)), [None] * self.B, [None] * len(requests), 0
        while queue or any(s is not None for s in slots):
            for b in range(self.B):
                if slots[b] is None and queue:
                    i, r = queue.popleft()
                    self.admit_spec(b, r["ids"], T, r["limit"], r["stops"], r["min_new"], r.get("script"), sampled, r.get("sampling"))
                    slots[b] = (i, r)
            active = [b for b in range(self.B) if slots[b] is not None]
            max_active = max(max_active, len(active))
            steps, done, toks = self.step.tolist(), self.done.tolist(), self.tokens()      # host sync = scheduling point
            left, freed = 0, False
            for b in active:
                i, r = slots[b]
                seq = toks[b][:min(steps[b], r["limit"])]
                end = stop_index(seq, r["stops"], r["min_new"])
                if end is not None or done[b] or len(seq) >= r["limit"]:
                    results[i] = (seq[:end], self.stats(b))
                    self.release(b)
                    slots[b], freed = None, True
                else:
                    left = max(left, r["limit"] - len(seq))
            if not left or (freed and queue):
                continue                                             # refill the freed slot(s) before spending more steps
            for _ in range(min(CHUNK, left)):
                step.run()
        return results, max_active
