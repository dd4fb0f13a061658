"""A numpy statement of Whisper's token selection under the timestamp rules (openai's SuppressTokens, SuppressBlank, ApplyTimestampRules and
GreedyDecoder.update at temperature 0; transformers' WhisperTimeStampLogitsProcessor is the same rule text), in fp64 by default: the yardstick
of `us_whisper_select` and of the selection stage inside `us_whisper_decode` (csrc/whisper.hip).

A layout is a dict: `eos`, `no_timestamps`, `max_initial_timestamp_index` (-1: none), and optionally `no_speech`, `suppress`,
`begin_suppress` (lists of ids).  `tb = no_timestamps + 1` is the first timestamp token.
"""
import numpy as np


def masks(layout, V):
    """(suppress, begin_suppress) as bool [V]"""
    out = []
    for k in ("suppress", "begin_suppress"):
        m = np.zeros(V, dtype=bool)
        ids = np.asarray(layout.get(k, ()), dtype=np.int64).reshape(-1)
        m[ids] = True
        out.append(m)
    return out


def allowed(V, sampled, layout, suppress=None, begin_suppress=None):
    """bool [V]: what survives every mask in front of the decision, given the tokens sampled so far"""
    eos, nt, cap = int(layout["eos"]), int(layout["no_timestamps"]), int(layout.get("max_initial_timestamp_index", -1))
    tb = nt + 1
    seq = [int(t) for t in sampled]
    ok = np.ones(V, dtype=bool)
    if suppress is not None:
        ok &= ~suppress
    if begin_suppress is not None and not seq:
        ok &= ~begin_suppress
    ok[nt] = False
    last_ts = len(seq) >= 1 and seq[-1] >= tb
    pen_ts = len(seq) < 2 or seq[-2] >= tb
    if last_ts and pen_ts:
        ok[tb:] = False
    if last_ts and not pen_ts:
        ok[:eos] = False
    stamps = [t for t in seq if t >= tb]
    if stamps:
        ok[tb:stamps[-1] if last_ts and not pen_ts else stamps[-1] + 1] = False
    if not seq:
        ok[:tb] = False
        if cap >= 0:
            ok[tb + cap + 1:] = False
    return ok


def _lse(v, dtype):
    if v.size == 0 or not np.isfinite(v.max()):
        return dtype(-np.inf)
    m = v.max()
    return dtype(m + np.log(np.exp(v - m, dtype=dtype).sum(dtype=dtype), dtype=dtype))


def select(x, sampled, layout, suppress=None, begin_suppress=None, dtype=np.float64):
    """One step: logits x [V] and the tokens sampled so far -> dict(token, logprob, decided (the timestamps won), d = lse_ts - max_text
    (nan unless both sides are finite), free (both sides finite), gap (top-1 minus top-2 of the surviving logits, inf with one survivor))."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    V = x.shape[0]
    eos, tb = int(layout["eos"]), int(layout["no_timestamps"]) + 1
    ok = allowed(V, sampled, layout, suppress, begin_suppress)
    text, ts = x[:tb][ok[:tb]], x[tb:][ok[tb:]]
    lse_ts = _lse(ts, dtype)
    max_text = text.max() if text.size else dtype(-np.inf)
    decided = bool(lse_ts > max_text)
    free = bool(np.isfinite(lse_ts) and np.isfinite(max_text))
    if decided:
        ok = ok.copy()
        ok[:tb] = False
    y = np.where(ok, x, dtype(-np.inf))
    if not ok.any() or not np.isfinite(y.max()):
        return dict(token=eos, logprob=0.0, decided=decided, d=float("nan"), free=False, gap=float("inf"))      # nothing survives: the item ends
    token = int(np.argmax(y))                           # the lower index on an exact tie
    top = np.sort(y[ok])[::-1]
    return dict(token=token, logprob=float(y[token] - _lse(y[ok], dtype)), decided=decided, d=float(lse_ts - max_text) if free else float("nan"),
                free=free, gap=float(top[0] - top[1]) if top.size > 1 else float("inf"))


def history(sampled, layout, done=False):
    """the five numbers the library keeps per item: (n_sampled, last, penultimate, last_timestamp, done)"""
    tb = int(layout["no_timestamps"]) + 1
    seq = [int(t) for t in sampled]
    stamps = [t for t in seq if t >= tb]
    return (len(seq), seq[-1] if seq else -1, seq[-2] if len(seq) > 1 else -1, stamps[-1] if stamps else -1, int(bool(done)))


def decode(logits, layout, dtype=np.float64):
    """The loop of one item over given per-step logits [steps][V] (as the model produced them while it followed these very choices):
    -> dict(tokens [steps] with eos at and after the end, length, logprobs [steps] (0 after the end), sum_logprob, steps: select()'s dicts
    up to and including the step that emitted eos)."""
    logits = np.asarray(logits)
    steps, V = logits.shape
    sup, beg = masks(layout, V)
    eos = int(layout["eos"])
    tokens, lps, sampled, recs, length = np.full(steps, eos, dtype=np.int64), np.zeros(steps), [], [], None
    for i in range(steps):
        r = select(logits[i], sampled, layout, sup, beg, dtype)
        recs.append(r)
        tokens[i], lps[i] = r["token"], r["logprob"]
        sampled.append(r["token"])
        if r["token"] == eos:
            length = i
            break
    return dict(tokens=tokens, length=steps if length is None else length, logprobs=lps, sum_logprob=float(lps.sum()), steps=recs)


def no_speech_prob(x, no_speech, dtype=np.float64):
    """softmax(unmasked logits)[no_speech]"""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    return float(np.exp(x[no_speech] - _lse(x, dtype)))
