"""Prefix caching for the batch slots (enable_prefix_caching): which cache rows of which slot a new prompt may reuse.

Pure host bookkeeping, no torch: per slot the ids whose rows [0, L) of that slot's cache were written by PREFILL launches, or copied
from such rows (the project's "exact" rule, as generate()'s reuse_prefix="exact": a row of the prefill path does not depend on how
many rows were prefilled with it, so reusing it is bit-identical with recomputing it).  Rows appended by decode steps are never
recorded: a slot's entry is its prompt, whatever it generates afterwards.  A slot that is still decoding keeps its entry - decode
appends at positions >= L, its rows [0, L) are stable - so it can serve as a source while it runs.
"""

MIN_MATCH = 16      # a common prefix below this counts as none (generate()'s rule)


def common_prefix(a, b, limit):
    """Length of the common prefix of the id sequences a and b, at most `limit`."""
    n = min(len(a), len(b), limit)
    i = 0
    while i < n and a[i] == b[i]:
        i += 1
    return i


def reusable_past(ids, cached_ids, cap, written_upto, exact):
    """The single sequence's rule (generate(), score()): how many leading tokens of the prompt `ids` are not prefilled again when the
    cache holds the rows of `cached_ids` (None / empty: nothing cached) - their common prefix, at most `cap` (generate(): L - 1, the
    last token's row yields the first pick; score(): start - 1); exact: at most the `written_upto` rows that prefill launches wrote
    (rows beyond that were appended by decode steps).  Below MIN_MATCH tokens: 0."""
    if not cached_ids:
        return 0
    past = common_prefix(ids, cached_ids, cap)
    if exact:
        past = min(past, written_upto)
    return past if past >= MIN_MATCH else 0


class PrefixIndex:
    """The index of one set of batch buffers: `nslots` slots of `ctx_max` rows whose idle slots are stepped `chunk` rows at a time."""

    def __init__(self, nslots, ctx_max, chunk=8):
        self.nslots, self.ctx_max, self.chunk = int(nslots), int(ctx_max), int(chunk)
        self.entries = [None] * self.nslots

    def reset(self):
        """Forget every entry (vLLM's reset_prefix_cache; also what new buffers start from)."""
        self.entries = [None] * self.nslots

    def length(self, slot):
        """Rows of `slot` that are recorded as reusable."""
        e = self.entries[slot]
        return 0 if e is None else len(e)

    def match(self, prompt, target):
        """(source slot, past) for a prompt about to be admitted into slot `target`: the longest common prefix with any slot's entry,
        capped at len(prompt) - 1 (the last token is always prefilled: its row yields the first pick); ties go to the target itself
        (no copy needed), then to the lowest slot.  Below MIN_MATCH tokens: (None, 0)."""
        cap = len(prompt) - 1
        best, src = 0, None
        for s in [target] + [s for s in range(self.nslots) if s != target]:
            e = self.entries[s]
            if e is None:
                continue
            n = common_prefix(prompt, e, cap)
            if n > best:
                best, src = n, s
        return (src, best) if best >= MIN_MATCH else (None, 0)

    def admit(self, target, prompt):
        """The prompt was admitted into `target`: rows [0, len(prompt)) of that slot are now reused, copied or prefilled rows of it."""
        self.entries[target] = tuple(prompt)

    def drop(self, slot):
        self.entries[slot] = None

    def park(self, slot):
        """The position an idle slot is parked at: behind its recorded rows, so that the garbage it decodes while idle (one row per
        step, `chunk` steps between two looks of the scheduler) lands where nothing is recorded.  With fewer than chunk + 1 rows left
        up to ctx_max the entry is dropped and the slot parks at 0."""
        n = self.length(slot)
        if n and self.ctx_max - n < self.chunk + 1:
            self.entries[slot] = None
            n = 0
        return n
