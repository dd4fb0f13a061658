"""The unit extraction restated in numpy: the exactness yardstick of csrc/units.hip (the role tools/mas_numpy.py has for the
alignment search).

* `kmeans_argmin`: units[t] = argmin_k sum_d (x[t, d] - c[k, d])^2 with the fp32 inputs taken to fp64 and the sum in fp64; numpy's
  argmin keeps the first index on exact ties.  A row with a non-finite feature gets -1.
* `run_lengths`: `unique_consecutive(return_counts=True)`.
* `process_unit`: the reference's `process_unit(encoded, sampling_rate, hop_length)` in closed form.  With spf = sampling_rate // 50,
  the 50 Hz frame f occupies samples [f spf, (f + 1) spf); output frame j covers samples [j hop, (j + 1) hop); there are
  (T spf) // hop of them; frame j's unit is the one with the most samples in it, the smallest unit value on ties (`torch.mode` on the
  CPU); the frames are run-length encoded again.  Nothing is expanded to samples.
* `process_unit_expanded`: the same by brute force, one array entry per sample, to check the closed form against.
"""
from __future__ import annotations

import numpy as np


def kmeans_argmin(x: np.ndarray, centers: np.ndarray, chunk: int = 16) -> np.ndarray:
    x64, c64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(centers, dtype=np.float32).astype(np.float64)
    out = np.empty(x64.shape[0], dtype=np.int64)
    for s in range(0, x64.shape[0], chunk):
        d = x64[s:s + chunk, None, :] - c64[None, :, :]
        out[s:s + chunk] = np.argmin(np.einsum("tkd,tkd->tk", d, d), axis=1)
    out[~np.isfinite(x64).all(axis=1)] = -1
    return out


def run_lengths(u: np.ndarray):
    u = np.asarray(u, dtype=np.int64)
    if u.size == 0:
        return u.copy(), u.copy()
    heads = np.flatnonzero(np.concatenate(([True], u[1:] != u[:-1])))
    return u[heads], np.diff(np.concatenate((heads, [u.size]))).astype(np.int64)


def frame_units(units: np.ndarray, durations: np.ndarray, sampling_rate: int, hop_length: int) -> np.ndarray:
    """The unit of every output frame, before the second run-length encoding."""
    units, durations = np.asarray(units, dtype=np.int64), np.asarray(durations, dtype=np.int64)
    spf = sampling_rate // 50
    ends = np.cumsum(durations) * spf                       # sample at which each run ends
    starts = ends - durations * spf
    n = int(ends[-1] // hop_length) if ends.size else 0
    out = np.empty(n, dtype=np.int64)
    for j in range(n):
        a, e = j * hop_length, (j + 1) * hop_length
        first = int(np.searchsorted(ends, a, side="right"))
        last = int(np.searchsorted(starts, e, side="left"))
        weight = {}
        for r in range(first, last):
            w = min(e, int(ends[r])) - max(a, int(starts[r]))
            if w > 0:
                weight[int(units[r])] = weight.get(int(units[r]), 0) + w
        top = max(weight.values())
        out[j] = min(u for u, w in weight.items() if w == top)
    return out


def process_unit(units, durations, sampling_rate: int, hop_length: int):
    return run_lengths(frame_units(units, durations, sampling_rate, hop_length))


def process_unit_expanded(units, durations, sampling_rate: int, hop_length: int):
    units, durations = np.asarray(units, dtype=np.int64), np.asarray(durations, dtype=np.int64)
    samples = np.repeat(units, durations * (sampling_rate // 50))
    n = samples.size // hop_length
    frames = np.empty(n, dtype=np.int64)
    for j, row in enumerate(samples[:n * hop_length].reshape(n, hop_length)):
        values, counts = np.unique(row, return_counts=True)      # ascending values: argmax keeps the smallest on ties
        frames[j] = values[np.argmax(counts)]
    return run_lengths(frames)
