"""Codebook fit, the parts that need no GPU: the fp64 statement (tools/kmeans_numpy.py) against the scikit-learn goldens
(tools/make_goldens_kmeans.py) and against scikit-learn itself where it is installed, the statement's edge cases, and the C ABI's
sizes and refusals."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kmeans_numpy as KN  # noqa: E402
from unitspeech_amd import _build, _lib  # noqa: E402
from unitspeech_amd import units as U  # noqa: E402

FIT_SYMBOLS = ["us_units_fit_workspace_bytes", "us_units_fit_state_bytes", "us_units_fit_state_clear", "us_units_fit_accumulate",
               "us_units_fit_update", "us_units_fit_seed_step"]


def load_golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"kmeans_fit_{name}.npz")) as g:
        d = {k: g[k] for k in g.files}
    d["x"] = U.synthetic_dense(U.synthetic_centers(int(d["K"]), int(d["D"]), int(d["seed_centers"])), int(d["N"]), int(d["seed_dense"]),
                               noise=float(d["noise"]))
    return d


@pytest.fixture(scope="module", params=["a", "b"])
def golden(request):
    return load_golden(request.param)


def test_statement_reproduces_the_sklearn_lloyd_golden(golden):
    g = golden
    st = KN.fit(g["x"], g["init"], max_iter=100, tol=0.0)
    assert st["n_iter"] == int(g["sk_n_iter"])
    assert np.array_equal(st["labels"], g["sk_labels"])
    assert np.abs(st["centers"] - g["sk_centers"]).max() <= 10 * float(g["stmt_vs_sklearn_max_abs"])
    assert abs(st["inertia"] - float(g["sk_inertia"])) <= 10 * float(g["stmt_vs_sklearn_rel_inertia"]) * float(g["sk_inertia"])
    assert len(st["history"]) == st["n_iter"] and st["history"][-1]["shift2"] == 0.0
    inertias = [r["inertia"] for r in st["history"]]
    assert all(b <= a for a, b in zip(inertias, inertias[1:]))
    assert np.array_equal(st["counts"], np.bincount(st["labels"], minlength=int(g["K"])))


def test_statement_reproduces_the_sklearn_minibatch_golden(golden):
    g = golden
    centers, totals, s = g["init"], np.zeros(int(g["K"]), dtype=np.int64), 0
    for i, n in enumerate(g["batches"]):
        centers, totals, rec, _ = KN.partial_fit_step(g["x"][s:s + n], centers, totals)
        s += int(n)
        assert np.array_equal(totals, g["mb_counts"][i])
        assert np.abs(centers - g["mb_centers"][i]).max() <= 10 * float(g["mb_stmt_vs_sklearn_max_abs"])
        assert rec["rows_used"] == n and rec["rows_skipped"] == 0


def test_statement_seeding_matches_the_golden_rows(golden):
    g = golden
    K = int(g["K"])
    centers, rows = KN.kmeans_plusplus(g["x"], K, KN.seed_uniforms(K, int(g["seed_pp"])))
    assert np.array_equal(rows, g["pp_rows"]) and np.array_equal(centers, g["x"][rows])
    assert np.array_equal(KN.seed_uniforms(K, int(g["seed_pp"])), U.seed_uniforms(K, int(g["seed_pp"])))
    assert KN.fit(g["x"], g["x"][rows], max_iter=100)["n_iter"] == int(g["pp_fit_n_iter"])


def test_statement_against_sklearn_live(golden):
    cluster = pytest.importorskip("sklearn.cluster")
    g = golden
    K = int(g["K"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = cluster.KMeans(n_clusters=K, init=g["init"], n_init=1, algorithm="lloyd", tol=0, max_iter=100).fit(g["x"])
    st = KN.fit(g["x"], g["init"], max_iter=100, tol=0.0)
    assert st["n_iter"] == km.n_iter_ and np.array_equal(st["labels"], km.labels_)
    assert np.abs(st["centers"] - km.cluster_centers_).max() <= 10 * float(g["stmt_vs_sklearn_max_abs"])
    assert abs(st["inertia"] - km.inertia_) <= 10 * float(g["stmt_vs_sklearn_rel_inertia"]) * km.inertia_
    mb = cluster.MiniBatchKMeans(n_clusters=K, init=g["init"], n_init=1, reassignment_ratio=0)
    centers, totals, s = g["init"], np.zeros(K, dtype=np.int64), 0
    for n in g["batches"]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mb.partial_fit(g["x"][s:s + n])
        centers, totals, _, _ = KN.partial_fit_step(g["x"][s:s + n], centers, totals)
        s += int(n)
        assert np.array_equal(totals, np.asarray(mb._counts).astype(np.int64))
        assert np.abs(centers - mb.cluster_centers_).max() <= 10 * float(g["mb_stmt_vs_sklearn_max_abs"])


# ---- the statement's edge cases -----------------------------------------------------------------------------------------------------
def test_empty_centre_keeps_its_value():
    x = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float32)
    centers = np.array([[0.25, 0.25, 0, 0], [100, 100, 100, 100]], dtype=np.float32)
    new, counts, rec, labels = KN.lloyd_step(x, centers)
    assert counts.tolist() == [3, 0] and rec["n_empty"] == 1 and labels.tolist() == [0, 0, 0]
    assert np.array_equal(new[1], centers[1])
    assert np.array_equal(new[0], (x.astype(np.float64).sum(0) / 3).astype(np.float32))
    new, totals, rec, _ = KN.partial_fit_step(x, centers, np.array([5, 7]))
    assert totals.tolist() == [8, 7] and np.array_equal(new[1], centers[1])
    assert np.array_equal(new[0], ((centers[0].astype(np.float64) * 5 + x.astype(np.float64).sum(0)) / 8).astype(np.float32))


def test_skipped_rows_are_ignored():
    g = np.random.default_rng(0)
    x = g.standard_normal((50, 8)).astype(np.float32)
    centers = x[:5].copy()
    valid = np.ones(50, dtype=bool)
    valid[[3, 17, 40]] = False
    bad = x.copy()
    bad[20, 2], bad[33, 0] = np.nan, np.inf
    valid[[20, 33]] = False                                  # the same rows, once masked and once non-finite
    a = KN.lloyd_step(bad, centers, valid)
    keep = np.flatnonzero(valid)
    b = KN.lloyd_step(x[keep], centers)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2]["rows_skipped"] == 5 and a[2]["rows_used"] == 45 and b[2]["rows_skipped"] == 0
    assert a[2]["inertia"] == pytest.approx(b[2]["inertia"], rel=1e-14)
    assert (a[3][~valid] == -1).all() and np.array_equal(a[3][keep], b[3])
    rows = KN.kmeans_plusplus(bad, 10, KN.seed_uniforms(10, 1), valid)[1]
    assert valid[rows].all()


def test_seeding_never_repeats_a_row_while_distinct_rows_remain():
    g = np.random.default_rng(1)
    x = g.standard_normal((60, 4)).astype(np.float32)
    for seed in range(5):
        rows = KN.kmeans_plusplus(x, 60, KN.seed_uniforms(60, seed))[1]
        assert sorted(rows.tolist()) == list(range(60))


def test_seeding_falls_back_to_the_uniform_pick_without_distinct_rows():
    g = np.random.default_rng(2)
    base = g.standard_normal((10, 4)).astype(np.float32)
    x = np.tile(base, (4, 1))                                # 40 rows, 10 distinct vectors
    u = KN.seed_uniforms(12, 3)
    centers, rows = KN.kmeans_plusplus(x, 12, u)
    assert len({tuple(c) for c in centers[:10]}) == 10
    assert rows[10] == int(np.floor(u[10] * 40)) and rows[11] == int(np.floor(u[11] * 40))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unitspeech_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(us_[a-z_0-9]+)\s*\(", txt))
    lib = C.CDLL(_build.build_library())
    for s in FIT_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert "units_fit.hip" in _build.SOURCES
    assert {"lloyd_step", "kmeans_plusplus", "KMeansQuantizer"} <= set(U.__all__)


def test_size_functions_return_zero_for_unsupported_sizes():
    lib = _lib.load()
    assert lib.us_units_fit_workspace_bytes(1000, 64, 32) > 0 and lib.us_units_fit_state_bytes(64, 32) > 0
    assert lib.us_units_fit_workspace_bytes(1 << 24, 2048, 1024) > 0 and lib.us_units_fit_state_bytes(2048, 1024) >= 2048 * 1024 * 8
    for rows, K, D in ((1000, 2049, 32), (1000, 64, 770), ((1 << 24) + 1, 64, 32), (1000, 0, 32), (1000, 64, 0), (0, 64, 32), (1000, 64, 1028)):
        assert lib.us_units_fit_workspace_bytes(rows, K, D) == 0, (rows, K, D)
    for K, D in ((2049, 32), (64, 770), (0, 32), (64, 2)):
        assert lib.us_units_fit_state_bytes(K, D) == 0, (K, D)


def test_library_refuses_unsupported_sizes_with_a_message():
    lib = _lib.load()
    for K, D in ((2049, 32), (64, 770)):
        assert lib.us_units_fit_state_clear(None, 0, K, D, None) == -1          # US_EINVAL
        assert b"K must be in [1, 2048]" in lib.us_last_error(None)
    assert lib.us_units_fit_accumulate(None, None, None, (1 << 24) + 1, 64, 32, None, 0, None, 0, None) == -1
    assert b"rows" in lib.us_last_error(None)
    assert lib.us_units_fit_update(7, None, None, None, None, 64, 32, None, 0, None, None) == -1
    assert lib.us_units_fit_seed_step(None, None, 1, 10, 2049, 32, 0, 0.5, None, None, None, None, 0, None) == -1


def test_python_refuses_unsupported_sizes_and_cpu_tensors():
    x = torch.zeros(100, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.KMeansQuantizer.fit(x, n_clusters=8)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.lloyd_step(x, None, torch.zeros(8, 32))
    with pytest.raises(RuntimeError, match="GPU only"):
        U.kmeans_plusplus(x, None, 8, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.KMeansQuantizer.from_centers(torch.zeros(8, 32)).partial_fit(x)
    with pytest.raises(ValueError, match="1 to 2048"):
        U.KMeansQuantizer.fit(torch.zeros(3000, 32), n_clusters=2049)
    with pytest.raises(ValueError, match="multiple of 4"):
        U.KMeansQuantizer.fit(torch.zeros(100, 770), n_clusters=8)
    with pytest.raises(ValueError, match="2\\^24"):
        U.KMeansQuantizer.fit(torch.zeros(1, 4).expand((1 << 24) + 1, 4), n_clusters=8)
    with pytest.raises(ValueError, match="init must be"):
        U.KMeansQuantizer.fit(x, init=torch.zeros(8, 16))
    with pytest.raises(ValueError, match="init must be"):
        U.KMeansQuantizer.fit(x, n_clusters=9, init=torch.zeros(8, 32))
    with pytest.raises(ValueError, match="init must be"):
        U.KMeansQuantizer.fit(x, n_clusters=8, init="greedy")
    with pytest.raises(ValueError, match="larger than the 100 rows"):
        U.KMeansQuantizer.fit(x, n_clusters=101)
    with pytest.raises(ValueError, match="larger than the 100 rows"):
        U.kmeans_plusplus(x, None, 101, 0)
    with pytest.raises(ValueError, match="n_clusters is needed"):
        U.KMeansQuantizer.fit(x)


def test_save_without_a_fit_round_trips_the_centres(tmp_path):
    centers = torch.from_numpy(U.synthetic_centers(12, 16, 0))
    q = U.KMeansQuantizer.from_centers(centers)
    q.save(tmp_path / "codebook.pt")
    assert torch.equal(U.KMeansQuantizer(str(tmp_path / "codebook.pt")).centers, centers)
    assert torch.equal(U.KMeansQuantizer.from_centers(torch.load(tmp_path / "codebook.pt")["centers"]).centers, centers)
    pytest.importorskip("sklearn")
    pytest.importorskip("joblib")
    q.save(tmp_path / "codebook.bin")
    assert torch.equal(U.KMeansQuantizer(str(tmp_path / "codebook.bin")).centers, centers)
