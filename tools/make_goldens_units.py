#!/usr/bin/env python3
"""Golden vectors of the unit extraction from the REFERENCE's own code (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_units.py

Drives `textless.data.kmeans_quantizer.KMeansQuantizer.forward` (scikit-learn `KMeans.predict` on a model with planted
`cluster_centers_`, saved with joblib and loaded by the reference class), `torch.unique_consecutive` as speech_encoder.py:40-41 calls
it, and `unitspeech.util.process_unit`, with the missing-module stubs of tools/make_goldens.py.  Inputs are
`unitspeech_amd.units.synthetic_centers` / `synthetic_dense` (centres plus noise on a sticky unit stream); the full case stores the
seeds and sizes, not the 3 MB of centres, and the tests regenerate them.  Writes tests/golden/units_<name>.npz with
  K, D, T, seed, noise      the recipe
  units                     the reference's `predict` (int64 [T])
  dedup_units, dedup_durations     `unique_consecutive(return_counts=True)`
  rates [n, 2]              (sampling_rate, hop_length) pairs, and for pair i  proc_unit_i / proc_duration_i from `process_unit`
  tiny only: centers, dense
A golden is written only if the reference's fp32 `predict` agrees with the fp64 argmin (tools/units_numpy.py) on every row: the
library is held to the fp64 argmin, so a case on which the reference itself rounds differently would be no yardstick.
"""
from __future__ import annotations

import importlib
import importlib.machinery
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import units_numpy as UN  # noqa: E402
from make_goldens import REF, save  # noqa: E402
from unitspeech_amd.units import synthetic_centers, synthetic_dense  # noqa: E402

CASES = [("tiny", 50, 16, 61, 3, 0.5, True), ("full", 1000, 768, 500, 4, 0.5, False)]
RATES = [(16000, 256), (16000, 320), (16000, 512), (16000, 1000), (22050, 256)]


def import_reference(name):
    """Import a module of the reference checkout, replacing third-party modules that are not installed by stubs."""
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    for _ in range(80):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            if e.name.startswith(("unitspeech", "conf")):
                raise
            m = MagicMock()
            m.__spec__ = importlib.machinery.ModuleSpec(e.name, None)
            m.__path__ = []
            sys.modules[e.name] = m
            for k in [k for k in sys.modules if k.startswith(("unitspeech", "conf"))]:
                del sys.modules[k]
    raise RuntimeError(f"could not import {name} of the reference")


def planted_kmeans(centers, path):
    import joblib
    from sklearn.cluster import KMeans
    km = KMeans(n_clusters=centers.shape[0], n_init=1, max_iter=1, random_state=0).fit(centers)
    km.cluster_centers_ = np.ascontiguousarray(centers, dtype=np.float32)
    joblib.dump(km, path)


def main():
    torch.set_num_threads(8)
    Q = import_reference("unitspeech.textlesslib.textless.data.kmeans_quantizer")
    util = import_reference("unitspeech.util")
    for name, K, D, T, seed, noise, store in CASES:
        centers = synthetic_centers(K, D, seed)
        dense = synthetic_dense(centers, T, seed, noise)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "km.bin")
            planted_kmeans(centers, path)
            quantizer = Q.KMeansQuantizer(path)
            assert quantizer.vocab_size == K
            units = quantizer(torch.from_numpy(dense))
        want = UN.kmeans_argmin(dense, centers)
        if not np.array_equal(units.numpy(), want):
            raise SystemExit(f"units_{name}: the reference's predict differs from the fp64 argmin on "
                             f"{int((units.numpy() != want).sum())} rows; pick another seed")
        du, dd = torch.unique_consecutive(units, return_counts=True)
        arrs = dict(K=np.array(K), D=np.array(D), T=np.array(T), seed=np.array(seed), noise=np.array(noise), units=units.numpy(),
                    dedup_units=du.numpy(), dedup_durations=dd.numpy(), rates=np.array(RATES))
        for i, (sr, hop) in enumerate(RATES):
            pu, pd = util.process_unit({"units": du, "durations": dd}, sr, hop)
            arrs[f"proc_unit_{i}"], arrs[f"proc_duration_{i}"] = pu.numpy(), pd.numpy()
        if store:
            arrs.update(centers=centers, dense=dense)
        save(f"units_{name}", **arrs)
        print(f"units_{name}: {T} frames -> {len(du)} runs -> {len(arrs['proc_unit_0'])} mel-rate units at {RATES[0]}")


if __name__ == "__main__":
    main()
