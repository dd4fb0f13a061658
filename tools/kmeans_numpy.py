"""The codebook fit restated in fp64 numpy: the yardstick of csrc/units_fit.hip (the role tools/units_numpy.py has for the unit
extraction, whose `kmeans_argmin` is the assignment here).

* `lloyd_step`: labels = fp64 argmin (first index on ties, -1 on a row with a non-finite feature or a row masked out), fp64 sums and
  counts per centre, c_k = fp32(sum_k / count_k); a centre without rows keeps its value.  The record holds the inertia
  sum_rows sum_d (x_d - c_label,d)^2 against the centres the labels were taken with, shift2 = sum (c_new - c_old)^2 in fp64 over the fp32
  values, the number of empty centres, the rows used and the rows skipped.
* `partial_fit_step`: the same assignment, c_k = fp32((c_k total_k + sum_k) / (total_k + count_k)), total_k += count_k: scikit-learn's
  `MiniBatchKMeans.partial_fit` with `reassignment_ratio = 0`.
* `kmeans_plusplus`: plain D^2 seeding with the uniforms given by the caller: step 0 takes valid row floor(u_0 n_valid); step j sets
  mind_i = min(mind_i, |x_i - c_{j-1}|^2), takes the inclusive cumulative sum P over the valid rows and picks the smallest valid i with
  P_i > u_j P_last, or valid row floor(u_j n_valid) when P_last = 0.
* `fit`: `lloyd_step` until shift2 <= tol or max_iter; with tol = 0 it stops exactly when the labels stop changing, which is
  scikit-learn's strict convergence and gives its `n_iter_`.

Not scikit-learn's: its greedy k-means++ and RNG stream, the relocation of empty clusters, sample weights, `tol` scaled by the data's
variance, `MiniBatchKMeans.fit`'s sampler and early stopping, Elkan.
"""
from __future__ import annotations

import numpy as np

from units_numpy import kmeans_argmin


def seed_uniforms(K: int, seed: int) -> np.ndarray:
    """The K doubles in [0, 1) that `kmeans_plusplus(seed=...)` of the library draws."""
    return np.random.Generator(np.random.Philox(key=[int(seed), 0x6b2b])).random(K)


def random_rows(n_rows: int, seed: int) -> np.ndarray:
    """The permutation of the rows whose first K valid entries `init="random"` of the library takes."""
    return np.random.Generator(np.random.Philox(key=[int(seed), 0x7270])).permutation(n_rows)


def assign(x, centers, valid=None):
    labels = kmeans_argmin(x, centers)
    if valid is not None:
        labels[~np.asarray(valid, dtype=bool)] = -1
    return labels


def accumulate(x, labels, centers):
    """-> (fp64 sums [K, D], int64 counts [K], fp64 inertia) over the rows with labels >= 0."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(centers, dtype=np.float32).astype(np.float64)
    K = c64.shape[0]
    use = labels >= 0
    sums = np.zeros_like(c64)
    np.add.at(sums, labels[use], x64[use])
    counts = np.bincount(labels[use], minlength=K).astype(np.int64)
    diff = x64[use] - c64[labels[use]]
    return sums, counts, float(np.einsum("td,td->", diff, diff))


def _record(inertia, new, old, counts, labels):
    d = new.astype(np.float64) - old.astype(np.float64)
    return dict(inertia=inertia, shift2=float(np.einsum("kd,kd->", d, d)), n_empty=int((counts == 0).sum()), rows_used=int((labels >= 0).sum()),
                rows_skipped=int((labels < 0).sum()))


def lloyd_step(x, centers, valid=None):
    """-> (new centres fp32 [K, D], counts int64 [K], record dict, labels)."""
    centers = np.asarray(centers, dtype=np.float32)
    labels = assign(x, centers, valid)
    sums, counts, inertia = accumulate(x, labels, centers)
    new = centers.copy()
    live = counts > 0
    new[live] = (sums[live] / counts[live, None].astype(np.float64)).astype(np.float32)
    return new, counts, _record(inertia, new, centers, counts, labels), labels


def partial_fit_step(x, centers, totals, valid=None):
    """-> (new centres fp32 [K, D], new totals int64 [K], record dict, labels)."""
    centers = np.asarray(centers, dtype=np.float32)
    totals = np.asarray(totals, dtype=np.int64)
    labels = assign(x, centers, valid)
    sums, counts, inertia = accumulate(x, labels, centers)
    new = centers.copy()
    live = counts > 0
    t = totals[live, None].astype(np.float64)
    new[live] = ((centers[live].astype(np.float64) * t + sums[live]) / (t + counts[live, None].astype(np.float64))).astype(np.float32)
    return new, totals + counts, _record(inertia, new, centers, counts, labels), labels


def kmeans_plusplus(x, n_clusters: int, uniforms, valid=None, margins=None):
    """-> (centres fp32 [K, D], row indices int64 [K]).  `margins`, a list, receives for every D^2 step the distance of u_j P_last to
    the nearest cumulative sum, relative to P_last (the golden generator's guard)."""
    x = np.asarray(x, dtype=np.float32)
    x64 = x.astype(np.float64)
    ok = np.isfinite(x64).all(axis=1)
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool)
    rows = np.flatnonzero(ok)
    if rows.size == 0:
        raise ValueError("kmeans_plusplus: no valid row")
    picks = np.empty(n_clusters, dtype=np.int64)
    mind = np.full(x.shape[0], np.inf)
    for j in range(n_clusters):
        u = float(uniforms[j])
        if j > 0:
            d = x64[rows] - x64[picks[j - 1]]
            mind[rows] = np.minimum(mind[rows], np.einsum("td,td->t", d, d))
            P = np.cumsum(mind[rows])
        if j == 0 or not P[-1] > 0.0:
            picks[j] = rows[min(int(np.floor(u * rows.size)), rows.size - 1)]
            continue
        t = u * P[-1]
        i = int(np.searchsorted(P, t, side="right"))          # the first i with P_i > t
        i = min(i, rows.size - 1)
        if margins is not None:
            margins.append(float(np.abs(P[max(i - 1, 0):i + 1] - t).min() / P[-1]))
        picks[j] = rows[i]
    return x[picks].copy(), picks


def fit(x, init, max_iter: int = 100, tol: float = 0.0, valid=None):
    """-> dict(centers, labels, inertia, n_iter, counts, history).  `labels` and `inertia` belong to the returned centres."""
    centers = np.asarray(init, dtype=np.float32).copy()
    history = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        centers, counts, rec, labels = lloyd_step(x, centers, valid)
        history.append(rec)
        if rec["shift2"] <= tol:
            break
    if not history or history[-1]["shift2"] != 0.0:
        labels = assign(x, centers, valid)
        _, counts, inertia = accumulate(x, labels, centers)
    else:
        inertia = history[-1]["inertia"]
    return dict(centers=centers, labels=labels, inertia=inertia, n_iter=n_iter, counts=counts, history=history)


def min_gap(x, centers) -> float:
    """The smallest fp64 gap between the best and the second-best squared distance over the rows (inf for K = 1)."""
    x64, c64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(centers, dtype=np.float32).astype(np.float64)
    if c64.shape[0] < 2:
        return float("inf")
    gap = np.inf
    for s in range(0, x64.shape[0], 64):
        d = x64[s:s + 64, None, :] - c64[None, :, :]
        two = np.partition(np.einsum("tkd,tkd->tk", d, d), 1, axis=1)[:, :2]
        gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
    return gap
