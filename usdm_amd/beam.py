"""Host side of beam search: the finished-hypotheses bookkeeping, replayed from the step log that usdm_beam_step writes on the device.

The device runs the search itself - per step the KC = max(2, 1 + n_eos) * B best continuations of the B running beams and the next
running beams (the first B that are no EOS) - and logs every step's candidates as (score, token, parent beam).  What remains is what HF
transformers does with those candidates on the side: _update_finished_beams, _check_early_stop_heuristic and
_beam_search_has_unfinished_sequences of the installed transformers' GenerationMixin._beam_search.  BeamReplay is that bookkeeping,
fed one log row per step at the decode loop's sync points; it says when HF would have stopped (rows the device ran past that point
are never fed) and recovers the sequences by backtracking the parents.  Pure Python / numpy: no torch, no device.

HF's arithmetic is kept in float32 with its -1e9 placeholders, because the order of the finished list is decided by those values;
torch.topk is restated as a stable descending sort (among equal scores the earlier entry wins)."""
import numpy as np

NEG = np.float32(-1.0e9)
EARLY_STOPPING = (False, True, "never")


def check_beam_args(num_beams, num_return_sequences=None, length_penalty=1.0, early_stopping=False, n_eos=0, vocab=None):
    """generate()'s / BeamSearchParams' beam knobs -> (B, n, length_penalty, early_stopping, KC).  ValueError for anything outside
    usdm_beam_step's limits (1 <= B <= 16, at most 3 EOS ids, KC = max(2, 1 + n_eos) * B <= 32, vocab >= KC) or HF's rules
    (1 <= num_return_sequences <= num_beams, early_stopping in False / True / "never", a finite length_penalty)."""
    from .ops import beam_candidates
    KC = beam_candidates(num_beams, n_eos)
    if vocab is not None and vocab < KC:
        raise ValueError(f"beam search keeps KC = {KC} candidates per step, the vocabulary has only {vocab} ids")
    n = 1 if num_return_sequences is None else num_return_sequences
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= num_beams:
        raise ValueError(f"num_return_sequences must be an integer 1 .. num_beams = {num_beams}, got {num_return_sequences!r}")
    if not any(early_stopping is v or (isinstance(v, str) and early_stopping == v) for v in EARLY_STOPPING):
        raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
    try:
        lp = float(length_penalty)
    except (TypeError, ValueError):
        lp = float("nan")
    if isinstance(length_penalty, bool) or not np.isfinite(lp):
        raise ValueError(f"length_penalty must be a finite number, got {length_penalty!r}")
    return num_beams, n, lp, early_stopping, KC


def check_beam_call(do_sample=False, logprobs=None, penalties=None, edits=None, min_p=0.0, logits_hook=None, min_new_tokens=0,
                    tensor_parallel=False):
    """What generate(num_beams > 1) cannot be combined with: NotImplementedError, each with its reason.  penalties / edits are
    llm.check_penalties' / llm.check_edits' values (None = neutral)."""
    reasons = (
        (do_sample, "do_sample: beam-search multinomial sampling is not built; the search ranks exact log-probabilities"),
        (logprobs is not None, "logprobs: the step log holds the hypotheses' cumulative scores; rescore the list with score()"),
        (penalties is not None, "repetition / presence / frequency penalties: the penalty table is per slot and is not reordered with the beams"),
        (edits is not None, "logit_bias / no_repeat_ngram_size: the edit state is per slot and is not reordered with the beams"),
        (bool(min_p), "min_p: a sampling filter, meaningless for a ranked search"),
        (logits_hook is not None, "_logits_hook: Python logits processors cannot run inside the captured beam step"),
        (bool(min_new_tokens), "min_new_tokens > 0: the device-side candidate selection does not mask EOS by length"),
        (tensor_parallel, "tensor parallelism: the beam step and the KV reorder run on one GPU"),
    )
    for hit, why in reasons:
        if hit:
            raise NotImplementedError("num_beams > 1 with " + why)


def _stable_top(scores, k):
    return np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")[:k]


class BeamReplay:
    """HF's finished-beam bookkeeping over the step log.  feed(score [KC], token [KC], parent [KC]) takes the log row of the next
    step and returns True when the search is over (HF's loop condition turned False, or max_new steps were fed); results(n) then
    gives HF's sequences (generated tokens only, padded) and sequences_scores."""

    def __init__(self, B, eos=(), max_new=1, length_penalty=1.0, early_stopping=False):
        self.B, self.eos, self.max_new = B, set(int(e) for e in eos), int(max_new)
        self.eos_first = int(list(eos)[0]) if len(list(eos)) else -1
        self.KC = max(2, 1 + len(self.eos)) * B
        self.length_penalty, self.early_stopping = float(length_penalty), early_stopping
        self.tokens, self.parents, self.sels = [], [], []        # per step: the log row's tokens and parents, the running beams' ranks
        self.fin = [None] * B                                    # finished hypotheses as (step, rank); None = HF's empty placeholder
        self.fin_score = np.full(B, NEG, dtype=np.float32)
        self.fin_done = np.zeros(B, dtype=bool)
        self.unsat, self.over = True, False

    @property
    def steps(self):
        return len(self.tokens)

    def feed(self, score, token, parent):
        if self.over:
            raise RuntimeError("BeamReplay: the search is already over")
        B, KC, t = self.B, self.KC, self.steps
        cs = np.asarray(score, dtype=np.float32).reshape(KC)
        tok = [int(k) for k in np.asarray(token).reshape(KC)]
        self.tokens.append(tok)
        self.parents.append([int(p) for p in np.asarray(parent).reshape(KC)])
        hits = np.asarray([k in self.eos for k in tok]) | (t + 1 >= self.max_new)
        # _get_running_beams_for_next_iteration: the first B candidates that did not finish (what the device continued with)
        run = cs + hits.astype(np.float32) * NEG
        sel = _stable_top(run, B)
        self.sels.append([int(r) for r in sel])
        # _update_finished_beams: only the best B candidates can finish; score / length ** length_penalty
        did = hits & (np.arange(KC) < B)
        lp = cs / np.float32((t + 1) ** self.length_penalty)
        lp = lp + (~did).astype(np.float32) * NEG
        merged = np.concatenate([self.fin_score, lp])
        keep = _stable_top(merged, B)
        refs = self.fin + [(t, r) for r in range(KC)]
        done = np.concatenate([self.fin_done, did])
        self.fin, self.fin_score, self.fin_done = [refs[i] for i in keep], merged[keep].astype(np.float32), done[keep]
        # _check_early_stop_heuristic (at the new length) and _beam_search_has_unfinished_sequences
        best_len = self.max_new if (self.early_stopping == "never" and self.length_penalty > 0.0) else t + 1
        best_possible = np.float32(run[sel[0]]) / np.float32(best_len ** self.length_penalty)
        worst = np.where(self.fin_done, self.fin_score.min(), NEG)
        self.unsat = self.unsat and bool((best_possible > worst).any())
        open_beam = not (bool(self.fin_done.all()) and self.early_stopping is True)
        self.over = not (self.unsat and open_beam and not bool(hits.all()))
        return self.over

    def running_parents(self, t):
        """parent beam of each running beam after step t (what usdm_kv_reorder applied)"""
        return [self.parents[t][r] for r in self.sels[t]]

    def backtrack(self, ref):
        """The generated tokens of candidate (step, rank): its token, then its parent beam's, which was the running beam of the step
        before, and so on."""
        if ref is None:
            return []
        t, r = ref
        out = []
        while True:
            out.append(self.tokens[t][r])
            if t == 0:
                break
            r = self.sels[t - 1][self.parents[t][r]]
            t -= 1
        return out[::-1]

    def results(self, n=1, pad=None):
        """(sequences [n][width] as lists, padded with pad (default: the first EOS id, -1 without one), scores float32 [n])"""
        if pad is None:
            pad = self.eos_first
        seqs = [self.backtrack(ref) for ref in self.fin[:n]]
        width = max(len(s) for s in seqs)
        return [s + [pad] * (width - len(s)) for s in seqs], self.fin_score[:n].copy()
