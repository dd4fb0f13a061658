#!/usr/bin/env python3
"""Writes tests/golden/kmeans_fit_{a,b}.npz: what scikit-learn computes from given initial centres on seeded synthetic features, beside
the measured distance of the fp64 statement (tools/kmeans_numpy.py) from it.  CPU only; needs scikit-learn.

    python tools/make_goldens_kmeans.py

Each file holds the seeds and sizes the inputs are regenerated from (`synthetic_centers` / `synthetic_dense`), the initial centres,
scikit-learn's `KMeans(init=array, n_init=1, algorithm="lloyd", tol=0)` result (centres, labels, inertia, n_iter_), the centres and
counts after each of six `MiniBatchKMeans(init=array, reassignment_ratio=0).partial_fit` calls on batches of unequal size, the statement's
distance from each of these, the smallest fp64 gap between the best and the second-best squared distance met in any iteration, and the
rows the statement's k-means++ picks for a stored seed (with the n_iter of the statement's fit from them).

An input is refused (nothing is written) when the statement and scikit-learn disagree on a label or on n_iter_, when an iteration of
the statement has an empty centre, when the smallest gap is below 1e-6 of the mean squared distance, or when some u_j P_last of the
seeding lies within 1e-9 P_last of a neighbouring cumulative sum: those conditions make the exact comparisons of the tests legitimate.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kmeans_numpy as KN  # noqa: E402
from unitspeech_amd.units import synthetic_centers, synthetic_dense  # noqa: E402

CASES = {
    "a": dict(K=16, D=32, N=1500, noise=0.5, seed_centers=11, seed_dense=12, seed_init=13, seed_pp=14, batches=[130, 410, 77, 333, 256, 294]),
    "b": dict(K=64, D=64, N=4000, noise=1.0, seed_centers=21, seed_dense=22, seed_init=23, seed_pp=24, batches=[900, 333, 1200, 257, 640, 670]),
}
MAX_ITER = 100


def inputs(c):
    """-> (features [N, D] fp32, initial centres [K, D] fp32: the rows the statement's k-means++ picks for seed_init)."""
    x = synthetic_dense(synthetic_centers(c["K"], c["D"], c["seed_centers"]), c["N"], c["seed_dense"], noise=c["noise"])
    return x, KN.kmeans_plusplus(x, c["K"], KN.seed_uniforms(c["K"], c["seed_init"]))[0]


def make(name, c):
    from sklearn.cluster import KMeans, MiniBatchKMeans
    x, init = inputs(c)
    K = c["K"]
    assert sum(c["batches"]) == c["N"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=K, init=init, n_init=1, algorithm="lloyd", tol=0, max_iter=MAX_ITER).fit(x)
    st = KN.fit(x, init, max_iter=MAX_ITER, tol=0.0)
    gap = np.inf
    centers = init
    for rec in st["history"]:
        if rec["n_empty"]:
            raise SystemExit(f"{name}: an iteration of the statement has an empty centre")
        gap = min(gap, KN.min_gap(x, centers))
        centers = KN.lloyd_step(x, centers)[0]
    gap = min(gap, KN.min_gap(x, st["centers"]))
    if st["n_iter"] >= MAX_ITER or st["n_iter"] != km.n_iter_ or not np.array_equal(st["labels"], km.labels_):
        raise SystemExit(f"{name}: the statement and scikit-learn disagree (n_iter {st['n_iter']} / {km.n_iter_})")
    lloyd_abs = float(np.abs(st["centers"].astype(np.float64) - km.cluster_centers_).max())
    lloyd_rel = abs(st["inertia"] - km.inertia_) / km.inertia_

    mb = MiniBatchKMeans(n_clusters=K, init=init, n_init=1, reassignment_ratio=0)
    centers, totals = init, np.zeros(K, dtype=np.int64)
    mb_centers, mb_counts, mb_abs, s = [], [], [], 0
    for n in c["batches"]:
        batch = x[s:s + n]
        s += n
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mb.partial_fit(batch)
        gap = min(gap, KN.min_gap(batch, centers))
        centers, totals, rec, _ = KN.partial_fit_step(batch, centers, totals)
        if not np.array_equal(totals, np.asarray(mb._counts).astype(np.int64)):
            raise SystemExit(f"{name}: the statement's and MiniBatchKMeans' counts disagree")
        mb_centers.append(mb.cluster_centers_.astype(np.float32))
        mb_counts.append(totals.copy())
        mb_abs.append(float(np.abs(centers.astype(np.float64) - mb.cluster_centers_).max()))

    mean_dist = st["inertia"] / x.shape[0]
    if not gap >= 1e-6 * mean_dist:
        raise SystemExit(f"{name}: the smallest gap {gap:.3e} is below 1e-6 of the mean squared distance {mean_dist:.3e}")
    margins = []
    _, pp_rows = KN.kmeans_plusplus(x, K, KN.seed_uniforms(K, c["seed_pp"]), margins=margins)
    if min(margins) < 1e-9:
        raise SystemExit(f"{name}: a seeding threshold lies within {min(margins):.3e} P_last of a cumulative sum")
    if len(set(pp_rows.tolist())) != K:
        raise SystemExit(f"{name}: the seeding repeated a row")
    pp = KN.fit(x, x[pp_rows], max_iter=MAX_ITER, tol=0.0)          # the fit from that seeding is compared exactly too
    centers, pp_gap = x[pp_rows], KN.min_gap(x, pp["centers"])
    for rec in pp["history"]:
        pp_gap = min(pp_gap, KN.min_gap(x, centers))
        centers = KN.lloyd_step(x, centers)[0]
    if pp["n_iter"] >= MAX_ITER or any(r["n_empty"] for r in pp["history"]) or not pp_gap >= 1e-6 * mean_dist:
        raise SystemExit(f"{name}: the fit from the seeding does not converge, empties a centre or has a gap of {pp_gap:.3e}")
    gap = min(gap, pp_gap)

    out = os.path.join(ROOT, "tests", "golden", f"kmeans_fit_{name}.npz")
    np.savez_compressed(
        out, K=K, D=c["D"], N=c["N"], noise=c["noise"], seed_centers=c["seed_centers"], seed_dense=c["seed_dense"], seed_init=c["seed_init"], seed_pp=c["seed_pp"],
        batches=np.asarray(c["batches"], dtype=np.int64), init=init, sk_centers=km.cluster_centers_.astype(np.float32),
        sk_labels=km.labels_.astype(np.int32), sk_inertia=float(km.inertia_), sk_n_iter=int(km.n_iter_),
        mb_centers=np.stack(mb_centers), mb_counts=np.stack(mb_counts), stmt_vs_sklearn_max_abs=lloyd_abs,
        stmt_vs_sklearn_rel_inertia=lloyd_rel, mb_stmt_vs_sklearn_max_abs=max(mb_abs), min_gap=gap, mean_dist=mean_dist,
        pp_rows=pp_rows, pp_min_margin=min(margins), pp_fit_n_iter=pp["n_iter"])
    import sklearn
    print(f"{out}: sklearn {sklearn.__version__}, n_iter {km.n_iter_}, inertia {km.inertia_:.6f}, statement vs sklearn: centres {lloyd_abs:.2e}, "
          f"inertia {lloyd_rel:.2e} rel, mini-batch centres {max(mb_abs):.2e}; min gap {gap:.2e} (mean distance {mean_dist:.2e}), "
          f"seeding margin {min(margins):.2e}; {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    for name, c in CASES.items():
        make(name, c)
