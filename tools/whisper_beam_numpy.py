"""A numpy statement of Whisper's beam search under the timestamp rules (openai-whisper's BeamSearchDecoder.update / finalize and
MaximumLikelihoodRanker with length_penalty=None), in fp64 by default: the yardstick of `us_whisper_decode_beam` and `us_whisper_beam_select`
(csrc/whisper.hip).  The masks are tools/whisper_decode_numpy.py's `allowed`; a layout is that module's dict.

Per item: n rows, each with a sampled sequence, a score and a live flag (row 0 alone is live at the start), and a pool of finished
(sequence, score) pairs of capacity max(C, n), C = max_candidates = round(n * patience).  One step (`beam_step`):
 1. every live row offers its top n + 1 survivors by log-softmax over the survivors, the lower id first on equal values; a token at -inf is
    never offered; a row with no survivor offers (eos, 0.0);
 2. the candidates, in (row, rank) order, are sorted descending by score + log-probability, stably;
 3. the sorted list is walked: an eos candidate is newly finished (the row's sequence, the total), any other becomes the next new row; the walk
    stops once n new rows exist and everything behind the stop is ignored; rows that were not filled are dead;
 4. the newly finished entries join the pool in walk order while it holds fewer than C;
 5. the item ends when the pool holds C entries or no row is live.
`finalise` tops a pool of fewer than n entries up with the live rows in descending score (the lower row first on a tie); `rank` picks the
entry with the largest score / length (length 0: -inf), the earlier entry on a tie.  Three departures from openai: -inf tokens are never
candidates, an item's end depends on that item alone, and length 0 ranks at -inf.
"""
import numpy as np

import whisper_decode_numpy as rules


def max_candidates(beam_size, patience=None):
    """openai's round(beam_size * patience), patience 1.0 by default"""
    return int(round(beam_size * (1.0 if patience is None else patience)))


def row_candidates(x, sampled, layout, suppress=None, begin_suppress=None, k=2, dtype=np.float64):
    """One live row: logits x [V] and its sampled tokens -> ([(token, logprob)] of at most k entries, info: dict(d, free, decided,
    tail_gap = the gap between the k-th and the (k + 1)-th surviving logit, inf when there is no (k + 1)-th, max_logit))."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    V = x.shape[0]
    eos, tb = int(layout["eos"]), int(layout["no_timestamps"]) + 1
    ok = rules.allowed(V, sampled, layout, suppress, begin_suppress)
    text, ts = x[:tb][ok[:tb]], x[tb:][ok[tb:]]
    lse_ts = rules._lse(ts, dtype)
    max_text = text.max() if text.size else dtype(-np.inf)
    decided = bool(lse_ts > max_text)
    free = bool(np.isfinite(lse_ts) and np.isfinite(max_text))
    info = dict(d=float(lse_ts - max_text) if free else float("nan"), free=free, decided=decided, tail_gap=float("inf"), max_logit=float(np.abs(x).max()))
    if decided:
        ok = ok.copy()
        ok[:tb] = False
    y = np.where(ok, x, dtype(-np.inf))
    idx = np.flatnonzero(y > -np.inf)
    if idx.size == 0:
        return [(eos, 0.0)], info
    lse = rules._lse(y[ok], dtype)
    order = idx[np.lexsort((idx, -y[idx]))]              # descending value, the lower id first
    if order.size > k:
        info["tail_gap"] = float(y[order[k - 1]] - y[order[k]])
    return [(int(t), float(y[t] - lse)) for t in order[:k]], info


def walk(cands, n, C, eos, pool_count):
    """cands: [(row, token, total)] in (row, rank) order -> dict(rows [(parent, token, score)], finished [(parent, score)] in walk order,
    added: how many of them the pool takes, walked: candidates looked at, order: the sorted candidate indices)"""
    order = sorted(range(len(cands)), key=lambda c: -cands[c][2])           # stable: equal totals keep (row, rank) order
    rows, fin, walked = [], [], 0
    for c in order:
        if len(rows) >= n:
            break
        walked += 1
        row, tok, total = cands[c]
        if tok == eos:
            fin.append((row, total))
        else:
            rows.append((row, tok, total))
    return dict(rows=rows, finished=fin, added=max(0, min(len(fin), C - pool_count)), walked=walked, order=order)


def beam_step(logits, seqs, scores, live, pool, n, C, layout, suppress=None, begin_suppress=None, dtype=np.float64):
    """logits [n][V] (rows that are not live are not read), seqs / scores / live: the n rows, pool: [(sequence tuple, score)] ->
    dict(seqs, scores, live, parents [n] (-1: dead), tokens [n], pool, ended, rows, finished, added, cands, order, walked, info [per live row],
    sort_gap: the smallest distance of two neighbours of the sorted list up to (last walked, first ignored))."""
    eos = int(layout["eos"])
    cands, info = [], []
    for j in range(n):
        if not live[j]:
            continue
        top, inf = row_candidates(logits[j], seqs[j], layout, suppress, begin_suppress, n + 1, dtype)
        info.append(inf)
        cands += [(j, tok, scores[j] + lp) for tok, lp in top]
    w = walk(cands, n, C, eos, len(pool))
    totals = [cands[c][2] for c in w["order"]][:w["walked"] + 1]
    gaps = [a - b for a, b in zip(totals, totals[1:])]
    new_pool = list(pool) + [(tuple(seqs[j]), s) for j, s in w["finished"][:w["added"]]]
    rows = w["rows"]
    out = dict(seqs=[list(seqs[p]) + [t] for p, t, _ in rows] + [[] for _ in range(n - len(rows))],
               scores=[s for _, _, s in rows] + [0.0] * (n - len(rows)), live=[True] * len(rows) + [False] * (n - len(rows)),
               parents=[p for p, _, _ in rows] + [-1] * (n - len(rows)), tokens=[t for _, t, _ in rows] + [eos] * (n - len(rows)),
               pool=new_pool, ended=len(new_pool) >= C or not rows, rows=rows, finished=w["finished"], added=w["added"], cands=cands,
               order=w["order"], walked=w["walked"], info=info, sort_gap=min(gaps) if gaps else float("inf"))
    return out


def finalise(pool, seqs, scores, live, n):
    """a pool of fewer than n entries takes live rows in descending score, the lower row first on a tie, until it holds n"""
    pool = list(pool)
    for j in sorted((j for j in range(len(live)) if live[j]), key=lambda j: -scores[j]):
        if len(pool) >= n:
            break
        pool.append((tuple(seqs[j]), scores[j]))
    return pool


def value(entry):
    seq, score = entry
    return score / len(seq) if len(seq) else float("-inf")


def rank(pool):
    """the index of the entry with the largest score / length, the earlier one on a tie"""
    best = 0
    for i in range(1, len(pool)):
        if value(pool[i]) > value(pool[best]):
            best = i
    return best


def beam_search(logits_fn, n, C, max_new, layout, V, dtype=np.float64):
    """The loop of one item.  logits_fn(step, tokens, parents) -> logits [n][V]: `tokens` the n rows' last tokens (None at step 0: the prompt's
    last token for every row) and `parents` the row each one continues (None at step 0; a dead row has token eos and parent 0).
    -> dict(tokens [max_new] with eos at and after the end, length, sum_logprob, pool, winner, steps: beam_step's dicts,
    ended_by: 'pool' | 'dead' | 'max_new', runner_gap: the winner's value minus the runner-up's, inf with one entry)."""
    sup, beg = rules.masks(layout, V)
    eos = int(layout["eos"])
    seqs, scores, live, pool = [[] for _ in range(n)], [0.0] * n, [True] + [False] * (n - 1), []
    steps, tokens, parents, ended_by = [], None, None, "max_new"
    for i in range(max_new):
        r = beam_step(logits_fn(i, tokens, parents), seqs, scores, live, pool, n, C, layout, sup, beg, dtype)
        steps.append(r)
        seqs, scores, live, pool = r["seqs"], r["scores"], r["live"], r["pool"]
        tokens, parents = r["tokens"], [max(p, 0) for p in r["parents"]]
        if r["ended"]:
            ended_by = "pool" if len(pool) >= C else "dead"
            break
    pool = finalise(pool, seqs, scores, live, n)
    win = rank(pool)
    vals = sorted((value(e) for e in pool), reverse=True)
    seq, score = pool[win]
    out = np.full(max_new, eos, dtype=np.int64)
    out[:len(seq)] = seq
    return dict(tokens=out, length=len(seq), sum_logprob=float(score), pool=pool, winner=win, steps=steps, ended_by=ended_by,
                runner_gap=float(vals[0] - vals[1]) if len(vals) > 1 else float("inf"))
