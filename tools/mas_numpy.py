"""Monotonic alignment search (glow-tts `maximum_path`, called by train_STEP1.py:343) restated in numpy.

The reference imports it from an external compiled module; this is the repository's own statement of the algorithm, the one
`us_maximum_path` must reproduce bit for bit:

* the value table is fp32; for each frame y in order and each row x in [max(0, tx + y - ty), min(tx, y + 1)):
  value[x, y] += max(v_prev, v_cur), v_cur = value[x, y-1] (-1e9 when x == y), v_prev = value[x-1, y-1] (-1e9 when x == 0 and
  y > 0, 0 at x == y == 0); every other cell keeps its input value;
* the path starts at row tx - 1 on frame ty - 1 and walks back: mark (index, y), then step down iff index != 0 and
  (index == y or value[index, y-1] < value[index-1, y-1]) -- strict, so a tie stays on the row.

With tx > ty the sweep visits nothing and the walk compares input values.  The decision at y == 0 is never used (the walk ends).
"""
from __future__ import annotations

import numpy as np

NEG = np.float32(-1e9)


def maximum_path_each(value: np.ndarray, tx: int, ty: int) -> np.ndarray:
    """value [>= tx, >= ty] (any float dtype: taken as fp32) -> path [same shape] int32 0/1."""
    v = np.array(value, dtype=np.float32, copy=True)
    path = np.zeros(v.shape, dtype=np.int32)
    if tx <= 0 or ty <= 0:
        return path
    for y in range(ty):
        lo, hi = max(0, tx + y - ty), min(tx, y + 1)
        if lo >= hi:
            continue
        xs = np.arange(lo, hi)
        if y == 0:
            v_cur = np.full(hi - lo, NEG, np.float32)
            v_prev = np.zeros(hi - lo, np.float32)
        else:
            v_cur = np.where(xs == y, NEG, v[lo:hi, y - 1]).astype(np.float32)
            v_prev = np.where(xs == 0, NEG, v[np.maximum(xs - 1, 0), y - 1]).astype(np.float32)
        v[lo:hi, y] = v[lo:hi, y] + np.maximum(v_prev, v_cur)
    index = tx - 1
    for y in range(ty - 1, -1, -1):
        path[index, y] = 1
        if y > 0 and index != 0 and (index == y or v[index, y - 1] < v[index - 1, y - 1]):
            index -= 1
    return path


def maximum_path(value: np.ndarray, x_lengths, y_lengths) -> np.ndarray:
    """value [B, Tx, Ty] -> attn [B, Tx, Ty] float32 0/1 (rows tx.., columns ty.. zero)."""
    out = np.zeros(value.shape, dtype=np.float32)
    for b in range(value.shape[0]):
        out[b] = maximum_path_each(value[b], int(x_lengths[b]), int(y_lengths[b]))
    return out


def maximum_path_masked(value: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The call form of train_STEP1.py:343: value [B, Tx, Ty] times mask [B, Tx, Ty]; tx / ty read off the mask's first
    column / row."""
    value = (value * mask).astype(np.float32)
    tx = mask.sum(1)[:, 0].astype(np.int64)
    ty = mask.sum(2)[:, 0].astype(np.int64)
    return maximum_path(value, tx, ty)
