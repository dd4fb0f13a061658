"""The CTC loss, its gradient and the forced alignment restated in fp64 numpy: the yardstick of csrc/ctc_train.hip and of
`asr.ctc_loss` / `asr.forced_align` (the role tools/ctc_numpy.py has for the decoding and the edit distance).

An item with target l[0..L) has the extended sequence of S = 2 L + 1 states: blank, l[0], blank, ..., l[L - 1], blank.  A path starts in
state 0 or 1, ends in state S - 1 or S - 2, and moves from s to s, s + 1, or s + 2 when state s + 2 is a label that differs from the
label of s.

* `alpha_beta`: log alpha[t, s] = log p(frames 0..t end in s), log beta[t, s] = log p(frames t.. start in s); both include frame t's
  emission, so occupancy[t, s] = exp(alpha + beta - emission - log p(target)).
* `ctc_loss`: -log p(target) and its gradient with respect to the LOGITS: softmax - sum of the occupancies of the states that emit the
  entry.  An infeasible item (no path: T < L + number of adjacent equal pairs) has loss +inf and gradient 0.
* `forced_align`: the best path (Viterbi: max in place of logsumexp).  Tie rule: among equal predecessors staying in s wins over s - 1,
  and s - 1 over s - 2; of the two end states the last label wins over the final blank.
"""
from __future__ import annotations

import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def extended(target, blank: int):
    """-> (labels [S], skip [S]): the entry each state emits, and whether state s may be entered from s - 2."""
    l = np.asarray(target, dtype=np.int64).reshape(-1)
    if np.any(l == blank):
        raise ValueError("the target holds the blank")
    lab = np.full(2 * l.size + 1, blank, dtype=np.int64)
    lab[1::2] = l
    skip = np.zeros(lab.size, dtype=bool)
    skip[3::2] = l[1:] != l[:-1]
    return lab, skip


def _shift(a, k):
    """a[s - k] with -inf where s < k (k >= 0), or a[s + |k|] with -inf beyond the end (k < 0)."""
    out = np.full_like(a, -np.inf)
    if k > 0:
        out[k:] = a[:-k]
    elif k < 0:
        out[:k] = a[-k:]
    else:
        out[:] = a
    return out


def _lse3(a, b, c):
    with np.errstate(invalid="ignore"):
        m = np.maximum(a, np.maximum(b, c))
        safe = np.where(np.isfinite(m), m, 0.0)
        s = np.exp(a - safe) + np.exp(b - safe) + np.exp(c - safe)
        return np.where(np.isfinite(m), safe + np.log(np.where(s > 0, s, 1.0)), -np.inf)


def alpha_beta(log_probs, target, blank: int = 0):
    """log_probs [T, V] (T >= 1) -> (alpha [T, S], beta [T, S], log p(target))."""
    lp = np.asarray(log_probs, dtype=np.float64)
    lab, skip = extended(target, blank)
    T, S = lp.shape[0], lab.size
    e = lp[:, lab]                                       # [T, S]
    skip_out = _shift(skip.astype(np.float64), -2) > 0   # s -> s + 2 exists
    alpha = np.full((T, S), -np.inf)
    beta = np.full((T, S), -np.inf)
    alpha[0, :2] = e[0, :2]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = _lse3(a, _shift(a, 1), np.where(skip, _shift(a, 2), -np.inf)) + e[t]
    beta[T - 1, max(0, S - 2):] = e[T - 1, max(0, S - 2):]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = _lse3(b, _shift(b, -1), np.where(skip_out, _shift(b, -2), -np.inf)) + e[t]
    ll = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2] if S > 1 else -np.inf)
    return alpha, beta, float(ll)


def ctc_loss(logits, target, blank: int = 0):
    """logits [T, V] -> (loss, grad [T, V]): -log p(target | logits) and its gradient with respect to the logits."""
    x = np.asarray(logits, dtype=np.float64)
    T, V = x.shape
    l = np.asarray(target, dtype=np.int64).reshape(-1)
    if T == 0:
        return (0.0 if l.size == 0 else np.inf), np.zeros((0, V))
    lp = log_softmax(x)
    alpha, beta, ll = alpha_beta(lp, l, blank)
    if not np.isfinite(ll):
        return np.inf, np.zeros((T, V))
    lab, _ = extended(l, blank)
    with np.errstate(invalid="ignore"):
        occ = np.exp(np.where(np.isfinite(alpha) & np.isfinite(beta), alpha + beta - lp[:, lab] - ll, -np.inf))   # [T, S]
    per_entry = np.zeros((T, V))
    for s in range(lab.size):                            # ascending s: the order the library adds in
        per_entry[:, lab[s]] += occ[:, s]
    return -ll, np.exp(lp) - per_entry


def ctc_loss_batch(logits, targets, frame_lengths, target_lengths, blank: int = 0, zero_infinity: bool = False):
    """logits [B, Tmax, V], targets [B, Lmax] -> (loss [B], grad [B, Tmax, V]); rows at or beyond frame_lengths[b] get gradient 0."""
    x = np.asarray(logits, dtype=np.float64)
    B = x.shape[0]
    loss = np.zeros(B)
    grad = np.zeros_like(x)
    for b in range(B):
        T, L = int(frame_lengths[b]), int(target_lengths[b])
        loss[b], grad[b, :T] = ctc_loss(x[b, :T], np.asarray(targets)[b, :L], blank)
        if zero_infinity and not np.isfinite(loss[b]):
            loss[b] = 0.0
    return loss, grad


def reduce_loss(loss, target_lengths, reduction: str = "mean"):
    """torch's three reductions: `mean` divides each item by its target length (clamped to 1), then averages."""
    loss = np.asarray(loss, dtype=np.float64)
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    if reduction == "mean":
        return (loss / np.maximum(np.asarray(target_lengths, dtype=np.float64), 1.0)).mean()
    raise ValueError(f"reduction = {reduction!r}")


def forced_align(scores, target, blank: int = 0):
    """scores [T, V] -> (path [T] int64, score, start [L] int64, frames [L] int64); an infeasible item: (all -1, -inf, zeros, zeros)."""
    x = np.asarray(scores, dtype=np.float64)
    l = np.asarray(target, dtype=np.int64).reshape(-1)
    T, L = x.shape[0], l.size
    none = (np.full(T, -1, dtype=np.int64), -np.inf, np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64))
    if T == 0:
        return (none[0], 0.0, none[2], none[3]) if L == 0 else none
    lab, skip = extended(l, blank)
    S = lab.size
    e = x[:, lab]
    d = np.full(S, -np.inf)
    d[:2] = e[0, :2]
    back = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        cand = np.stack([d, _shift(d, 1), np.where(skip, _shift(d, 2), -np.inf)])
        back[t] = np.argmax(cand, axis=0)                # the first maximum: stay, then s - 1, then s - 2
        d = cand[back[t], np.arange(S)] + e[t]
    s = S - 1
    if S > 1 and not d[S - 1] > d[S - 2]:                # the last label wins over the final blank
        s = S - 2
    if not np.isfinite(d[s]):
        return none
    score = float(d[s])
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= back[t, s]
    start, frames = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for i in range(L):
        on = np.flatnonzero(states == 2 * i + 1)
        start[i], frames[i] = on[0], on.size
    return lab[states], score, start, frames
