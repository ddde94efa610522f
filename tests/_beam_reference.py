"""Numpy restatement of beam search as the installed transformers runs it (generate(num_beams=B, do_sample=False,
renormalize_logits=True)), for usdm_beam_step, usdm_amd.beam and generate(num_beams=).

beam_step(rows, scores, nlive, eos, B): one step.  lp_b = float64 log-softmax of the live rows (banned ids are -inf and carry no
mass), s(b, i) = scores[b] + lp_b(i) in float64, the KC = max(2, 1 + n_eos) * B best under the total order: value descending, then
flat index b * V + i ascending (-0.0 equals +0.0 in the comparison).  The next running beams are the first B candidates whose token is
no EOS id.

beam_search(row_fn, ...): the whole search.  It keeps explicit token lists per running beam and per finished hypothesis, as HF keeps
tensors of sequences (the product backtracks parent pointers instead), and HF's finished-beam bookkeeping in HF's float32 arithmetic:
_update_finished_beams, _check_early_stop_heuristic and _beam_search_has_unfinished_sequences, with max_length as the stopping
criterion that "finishes" the best B candidates of the last step.  torch.topk over HF's score lists is restated as a stable
descending sort: among equal scores the earlier entry wins (the -1e9 placeholders tie with each other and with nothing real)."""
import numpy as np

NEG = np.float32(-1.0e9)


def candidates(B, n_eos):
    return max(2, 1 + n_eos) * B


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isneginf(x).all():
        return np.full(x.shape, -np.inf)
    m = x.max()
    with np.errstate(divide="ignore"):
        return (x - m) - np.log(np.exp(x - m).sum())


def beam_step(rows, scores, nlive, eos, B):
    """rows [B][V] (only the first nlive are read), scores [B] -> dict of cand_score f64 [KC], cand_token, cand_parent i64 [KC], and
    the next running beams next_token, parent i64 [B], score f64 [B], sel = their ranks in the candidate list."""
    rows = np.asarray(rows)
    V = rows.shape[1]
    eos = list(eos)
    KC = candidates(B, len(eos))
    assert V >= KC and nlive in (1, B)
    s = np.stack([np.float64(scores[b]) + log_softmax64(rows[b, :V]) for b in range(nlive)]).reshape(-1)
    order = np.lexsort((np.arange(s.shape[0]), -(s + 0.0)))[:KC]      # stable: by -value, then flat index
    cs, ct, cp = s[order], order % V, order // V
    sel = [r for r in range(KC) if int(ct[r]) not in eos][:B]
    assert len(sel) == B
    return dict(cand_score=cs, cand_token=ct, cand_parent=cp, sel=np.asarray(sel), next_token=ct[sel], parent=cp[sel], score=cs[sel])


def stable_top(scores, k):
    """torch.topk(scores, k)[1] with ties resolved to the earlier entry"""
    return np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")[:k]


def beam_search(row_fn, B, max_new, eos=(), length_penalty=1.0, early_stopping=False, num_return_sequences=1, pad=None, step_fn=None):
    """row_fn(list of the B running beams' generated tokens) -> logits rows [B][V] (on the first call every list is empty and only
    row 0 is read).  step_fn: a replacement of beam_step with the same signature (recorded device output, for instance).
    Returns (sequences: list of num_return_sequences token lists, padded with `pad` to the longest; scores: float32 array; trace: per
    step the beam_step dict).  Sequences hold the generated tokens only."""
    eos = list(eos)
    KC = candidates(B, len(eos))
    pad = (eos[0] if eos else -1) if pad is None else pad
    step_fn = step_fn or beam_step
    running = [[] for _ in range(B)]
    run_scores = np.zeros(B)
    fin_seq, fin_score, fin_done = [[] for _ in range(B)], np.full(B, NEG, dtype=np.float32), np.zeros(B, dtype=bool)
    unsat, trace = True, []
    top_mask = np.arange(KC) < B
    for t in range(max_new):
        st = step_fn(row_fn(running), run_scores, 1 if t == 0 else B, eos, B)
        trace.append(st)
        cs32 = np.asarray(st["cand_score"], dtype=np.float32)
        cand_seq = [running[int(p)] + [int(k)] for p, k in zip(st["cand_parent"], st["cand_token"])]
        hits = np.asarray([int(k) in eos for k in st["cand_token"]]) | (t + 1 >= max_new)
        # the running beams of the next iteration (on the last step every candidate "hits": the loop ends there)
        sel = stable_top(cs32 + hits.astype(np.float32) * NEG, B)
        if not hits.all():
            assert sel.tolist() == np.asarray(st["sel"]).tolist()
            run_scores = np.asarray(st["score"]).copy()
        running = [cand_seq[r] for r in sel]
        best_running = np.float32((cs32 + hits.astype(np.float32) * NEG)[sel[0]])
        # _update_finished_beams
        did = hits & top_mask
        lp = cs32 / np.float32((t + 1) ** length_penalty)
        lp = lp + (~did).astype(np.float32) * NEG
        merged = np.concatenate([fin_score, lp])
        keep = stable_top(merged, B)
        all_seq, all_done = fin_seq + cand_seq, np.concatenate([fin_done, did])
        fin_seq, fin_score, fin_done = [all_seq[i] for i in keep], merged[keep].astype(np.float32), all_done[keep]
        # _check_early_stop_heuristic at cur_len + 1
        best_len = max_new if (early_stopping == "never" and length_penalty > 0.0) else t + 1
        best_possible = best_running / np.float32(best_len ** length_penalty)
        worst = np.where(fin_done, fin_score.min(), NEG)
        unsat = unsat and bool((best_possible > worst).any())
        if not (unsat and not (fin_done.all() and early_stopping is True) and not hits.all()):
            break
    n = num_return_sequences
    seqs, scores = fin_seq[:n], fin_score[:n]
    width = max(len(s) for s in seqs)
    return [s + [pad] * (width - len(s)) for s in seqs], scores, trace
