"""Greedy CTC decoding, the Levenshtein distance and the two error rates restated in numpy: the exactness yardstick of csrc/ctc.hip
and unitspeech_amd/asr.py (the role tools/units_numpy.py has for the unit extraction).

* `ctc_collapse`: merge equal neighbours, then drop the blank -> (tokens, first_frame): the kept tokens and the frame at which the run of
  each starts.
* `edit_distance`: Levenshtein distance with unit costs by the row DP.  Row i of D (hyp[:i] against every prefix of ref) comes from row
  i - 1 in two vectorised steps: the substitution / deletion candidates c_j, then the insertion chain D[i][j] = min(c_j, D[i][j - 1] + 1),
  which is min_k<=j (c_k - k) + j: one `np.minimum.accumulate`.
* `error_rates`: corpus CER / WER, sum of distances over sum of reference lengths, characters with spaces and words by `str.split`.
"""
from __future__ import annotations

import numpy as np


def ctc_collapse(ids, blank: int):
    u = np.asarray(ids, dtype=np.int64)
    if u.size == 0:
        return u.copy(), u.copy()
    heads = np.flatnonzero(np.concatenate(([True], u[1:] != u[:-1])) & (u != blank))
    return u[heads], heads.astype(np.int64)


def edit_distance(hyp, ref) -> int:
    a, b = np.asarray(hyp, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    m = b.size
    j = np.arange(m + 1, dtype=np.int64)
    row = j.copy()
    for i in range(1, a.size + 1):
        c = np.empty(m + 1, dtype=np.int64)
        c[0] = i
        c[1:] = np.minimum(row[:-1] + (b != a[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(c - j) + j
    return int(row[m])


def error_rates(hyps, refs):
    """-> {"cer", "wer", "per_utterance": [{"cer", "wer", "char_distance", "chars", "word_distance", "words"}]}; an utterance with an
    empty reference has nan rates; ValueError when the references hold no character or no word at all."""
    if len(hyps) != len(refs):
        raise ValueError("error_rates: hyps and refs differ in length")
    per = []
    for h, r in zip(hyps, refs):
        words = {w: i for i, w in enumerate(sorted(set(h.split()) | set(r.split())))}
        cd = edit_distance([ord(c) for c in h], [ord(c) for c in r])
        wd = edit_distance([words[w] for w in h.split()], [words[w] for w in r.split()])
        nc, nw = len(r), len(r.split())
        per.append({"cer": cd / nc if nc else float("nan"), "wer": wd / nw if nw else float("nan"), "char_distance": cd, "chars": nc,
                    "word_distance": wd, "words": nw})
    chars, words = sum(p["chars"] for p in per), sum(p["words"] for p in per)
    if chars == 0 or words == 0:
        raise ValueError("error_rates: the references are empty")
    return {"cer": sum(p["char_distance"] for p in per) / chars, "wer": sum(p["word_distance"] for p in per) / words, "per_utterance": per}
