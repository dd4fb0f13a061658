"""Codebook fit on the device (csrc/units_fit.hip) against the fp64 statement tools/kmeans_numpy.py.

What depends on the labelling alone (counts, empty centres, skipped rows, chosen rows, n_iter, final labels) is compared exactly.  New
centres are compared within 1 fp32 ulp: the fp64 sums differ from the statement's only by the order of addition, at most N 2^-53
relative, and are rounded once.  Inertia and shift2 of one step are compared within 1e-11 relative ((N + D + 2) 2^-53 < 3e-12 at these
sizes); a fit's `inertia_` within 1e-5 relative (centres one ulp apart move a squared distance of unit-scale data by under 1e-6)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kmeans_numpy as KN  # noqa: E402
from unitspeech_amd import units as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ulps(a, b):
    """Elementwise distance of two fp32 arrays in units in the last place (monotone integer map of the bit patterns)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def gemm_labels(x, centers):
    """The statement's labels by the fp64 expansion |c|^2 - 2 x.c (a BLAS call, for the shape whose brute-force statement takes
    minutes).  The gap between the two best scores is asserted to be far above the expansion's rounding, so the argmin is the
    statement's."""
    x64, c64 = x.astype(np.float64), centers.astype(np.float64)
    s = (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T)
    two = np.partition(s, 1, axis=1)[:, :2]
    scale = (x64 * x64).sum(1) + (c64 * c64).sum(1).max()
    assert ((two[:, 1] - two[:, 0]) > 1e-9 * scale).all()
    return np.argmin(s, axis=1)


def statement_step(x, centers, valid=None, labels=None):
    if labels is None:
        return KN.lloyd_step(x, centers, valid)
    sums, counts, inertia = KN.accumulate(x, labels, centers)
    new = centers.copy()
    live = counts > 0
    new[live] = (sums[live] / counts[live, None].astype(np.float64)).astype(np.float32)
    return new, counts, KN._record(inertia, new, centers, counts, labels), labels


def check_step(got, want, N):
    new, counts, rec = got
    w_new, w_counts, w_rec, _ = want
    assert np.array_equal(counts.cpu().numpy(), w_counts)
    assert rec["n_empty"] == w_rec["n_empty"] and rec["rows_used"] == w_rec["rows_used"] and rec["rows_skipped"] == w_rec["rows_skipped"]
    worst = int(ulps(new.cpu().numpy(), w_new).max())
    print(f"centres: max {worst} ulp; inertia rel {abs(rec['inertia'] - w_rec['inertia']) / w_rec['inertia']:.2e}; "
          f"shift2 rel {abs(rec['shift2'] - w_rec['shift2']) / max(w_rec['shift2'], 1e-300):.2e}")
    assert worst <= 1
    assert abs(rec["inertia"] - w_rec["inertia"]) <= 1e-11 * w_rec["inertia"]
    assert abs(rec["shift2"] - w_rec["shift2"]) <= 1e-11 * w_rec["shift2"]


def same_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[:2], b[:2])) and a[2] == b[2]


def step_case(name):
    if name == "odd":                      # nothing a multiple of a tile
        K, D, N = 37, 36, 3000
        planted = U.synthetic_centers(K, D, 1)
        x = U.synthetic_dense(planted, N, 2, noise=0.5)
        centers = planted + 0.1 * U.synthetic_centers(K, D, 3)
    elif name == "sparse":                 # most centres empty or with a handful of rows
        K, D, N = 2048, 1024, 5000
        planted = U.synthetic_centers(K, D, 4)
        x = U.synthetic_dense(planted, N, 5, noise=0.5)
        centers = planted
    elif name == "skewed":                 # one centre owns 90 % of the rows: its list is many pieces long
        K, D, N = 8, 64, 20000
        planted = U.synthetic_centers(K, D, 6)
        g = np.random.Generator(np.random.Philox(key=7))
        ids = np.where(g.random(N) < 0.9, 0, g.integers(1, K, size=N))
        x = (planted[ids] + 0.5 * g.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
        centers = planted + 0.1 * U.synthetic_centers(K, D, 8)
    else:                                  # the smallest sizes
        K, D, N = 1, 4, 70
        x = U.synthetic_dense(U.synthetic_centers(3, D, 9), N, 10, noise=0.5)
        centers = U.synthetic_centers(K, D, 11)
    return x, centers.astype(np.float32)


@pytest.mark.parametrize("name", ["odd", "sparse", "skewed", "tiny"])
def test_lloyd_step(name):
    x, centers = step_case(name)
    want = statement_step(x, centers, labels=gemm_labels(x, centers) if name == "sparse" else None)
    if name == "skewed":
        assert want[1][0] >= 0.89 * x.shape[0]
    if name == "sparse":
        assert want[2]["n_empty"] > 0.3 * centers.shape[0]
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(centers).to(DEV)
    got = U.lloyd_step(xd, None, cd)
    check_step(got, want, x.shape[0])
    assert torch.equal(cd.cpu(), torch.from_numpy(centers))          # the input centres are not touched
    assert same_bits(got, U.lloyd_step(xd, None, cd))


@pytest.fixture(scope="module")
def ragged():
    B, T, D, K = 8, 120, 256, 50
    planted = U.synthetic_centers(K, D, 20)
    x = np.stack([U.synthetic_dense(planted, T, 21 + b, noise=0.5) for b in range(B)])
    lengths = np.array([120, 1, 77, 120, 33, 64, 5, 101])
    x[2, 10, 7] = np.nan
    x[5, 63, 0] = np.inf
    valid = np.arange(T)[None, :] < lengths[:, None]
    centers = (planted + 0.1 * U.synthetic_centers(K, D, 30)).astype(np.float32)
    want = KN.lloyd_step(x.reshape(B * T, D), centers, valid.reshape(-1))
    return x, lengths, valid, centers, want


def test_ragged_batch_with_bad_rows(ragged):
    x, lengths, valid, centers, want = ragged
    B, T, D = x.shape
    assert want[2]["rows_skipped"] == B * T - lengths.sum() + 2 and 1 in lengths and T in lengths
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(centers).to(DEV)
    got = U.lloyd_step(xd, torch.from_numpy(lengths).to(DEV), cd)
    check_step(got, want, B * T)
    flat = U.lloyd_step(torch.from_numpy(x[valid]).to(DEV), None, cd)      # the valid rows alone, the two bad ones still among them
    assert torch.equal(flat[1], got[1]) and flat[2]["rows_skipped"] == 2 and flat[2]["rows_used"] == got[2]["rows_used"]
    assert int(ulps(flat[0].cpu().numpy(), want[0]).max()) <= 1


def test_two_chunk_accumulate(ragged):
    x, lengths, valid, centers, want = ragged
    xd, cd, ld = torch.from_numpy(x).to(DEV), torch.from_numpy(centers).to(DEV), torch.from_numpy(lengths).to(DEV)
    one = U.lloyd_step(xd, ld, cd)
    two = U.lloyd_step([xd[:3], xd[3:]], [ld[:3], ld[3:]], cd)
    assert torch.equal(one[1], two[1])
    assert int(ulps(one[0].cpu().numpy(), two[0].cpu().numpy()).max()) <= 1
    assert two[2]["rows_used"] == one[2]["rows_used"] and two[2]["rows_skipped"] == one[2]["rows_skipped"]
    assert abs(two[2]["inertia"] - one[2]["inertia"]) <= 1e-11 * one[2]["inertia"]
    check_step(two, want, x.shape[0] * x.shape[1])


def load_golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"kmeans_fit_{name}.npz")) as g:
        d = {k: g[k] for k in g.files}
    d["x"] = U.synthetic_dense(U.synthetic_centers(int(d["K"]), int(d["D"]), int(d["seed_centers"])), int(d["N"]), int(d["seed_dense"]),
                               noise=float(d["noise"]))
    d["fit"] = KN.fit(d["x"], d["init"], max_iter=100, tol=0.0)
    return d


@pytest.fixture(scope="module")
def goldens():
    return {n: load_golden(n) for n in ("a", "b")}


def test_partial_fit_follows_the_statement_and_sklearn(goldens):
    g = goldens["a"]
    K = int(g["K"])
    q = U.KMeansQuantizer.from_centers(g["init"].copy()).to(DEV)
    centers, totals, s = g["init"], np.zeros(K, dtype=np.int64), 0
    for i, n in enumerate(g["batches"]):
        batch = g["x"][s:s + n]
        s += int(n)
        centers, totals, rec, _ = KN.partial_fit_step(batch, centers, totals)
        assert q.partial_fit(torch.from_numpy(batch).to(DEV)) is q
        assert np.array_equal(q.counts_.cpu().numpy(), totals) and np.array_equal(totals, g["mb_counts"][i])
        got = q.centers.cpu().numpy()
        assert int(ulps(got, centers).max()) <= 1
        assert np.abs(got - g["mb_centers"][i]).max() <= 10 * float(g["mb_stmt_vs_sklearn_max_abs"])
        assert abs(q.inertia_ - rec["inertia"]) <= 1e-11 * rec["inertia"]
        assert torch.equal(q.quantize(torch.from_numpy(batch).to(DEV).unsqueeze(0))[0].cpu(),
                           torch.from_numpy(KN.assign(batch, centers)))          # the packed form follows the update
    assert len(q.history_) == 6


@pytest.mark.parametrize("name", ["a", "b"])
def test_kmeans_plusplus_picks_the_statements_rows(goldens, name):
    g = goldens[name]
    K = int(g["K"])
    _, want = KN.kmeans_plusplus(g["x"], K, KN.seed_uniforms(K, int(g["seed_pp"])))
    xd = torch.from_numpy(g["x"]).to(DEV)
    centers, rows = U.kmeans_plusplus(xd, None, K, int(g["seed_pp"]))
    assert rows.dtype == torch.int64 and np.array_equal(rows.cpu().numpy(), want) and np.array_equal(want, g["pp_rows"])
    assert torch.equal(centers.cpu(), torch.from_numpy(g["x"][want]))
    again = U.kmeans_plusplus(xd, None, K, int(g["seed_pp"]))
    assert torch.equal(again[0], centers) and torch.equal(again[1], rows)


def test_kmeans_plusplus_skips_padding_and_bad_rows(ragged):
    x, lengths, valid, centers, _ = ragged
    B, T, D = x.shape
    ok = valid.reshape(-1) & np.isfinite(x.reshape(B * T, D)).all(1)
    c, rows = U.kmeans_plusplus(torch.from_numpy(x).to(DEV), torch.from_numpy(lengths).to(DEV), 40, 5)
    rows = rows.cpu().numpy()
    assert ok[rows].all() and len(set(rows.tolist())) == 40
    assert torch.equal(c.cpu(), torch.from_numpy(x.reshape(B * T, D)[rows]))
    with pytest.raises(ValueError, match="valid rows"):
        U.kmeans_plusplus(torch.from_numpy(x[1:2]).to(DEV), torch.tensor([1]), 2, 0)


def test_kmeans_plusplus_on_duplicated_rows():
    base = np.random.default_rng(2).standard_normal((10, 4)).astype(np.float32)
    x = np.tile(base, (4, 1))                                # 40 rows, 10 distinct vectors
    u = KN.seed_uniforms(12, 3)
    centers, rows = U.kmeans_plusplus(torch.from_numpy(x).to(DEV), None, 12, 3)
    rows, centers = rows.cpu().numpy(), centers.cpu().numpy()
    assert len({tuple(c) for c in centers[:10]}) == 10
    assert rows[10] == int(np.floor(u[10] * 40)) and rows[11] == int(np.floor(u[11] * 40))
    assert np.array_equal(centers, x[rows])


def check_fit(q, want, x):
    K = want["centers"].shape[0]
    assert q.n_iter_ == want["n_iter"]
    labels = q.quantize(torch.from_numpy(x).to(DEV).unsqueeze(0))[0].cpu().numpy()
    assert np.array_equal(labels, want["labels"])
    assert int(ulps(q.centers.cpu().numpy(), want["centers"]).max()) <= 1
    assert abs(q.inertia_ - want["inertia"]) <= 1e-5 * want["inertia"]
    assert np.array_equal(q.counts_.cpu().numpy(), np.bincount(want["labels"], minlength=K))
    assert len(q.history_) == q.n_iter_
    inertias = [r["inertia"] for r in q.history_]
    assert all(np.isfinite(inertias)) and all(b <= a for a, b in zip(inertias, inertias[1:]))
    assert [r["n_empty"] for r in q.history_] == [r["n_empty"] for r in want["history"]]


@pytest.mark.parametrize("name", ["a", "b"])
def test_fit_from_the_golden_init(goldens, name):
    g = goldens[name]
    xd, init = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["init"]).to(DEV)
    q = U.KMeansQuantizer.fit(xd, init=init)
    assert q.n_iter_ == int(g["sk_n_iter"]) and torch.equal(init.cpu(), torch.from_numpy(g["init"]))
    check_fit(q, g["fit"], g["x"])
    assert np.abs(q.centers.cpu().numpy() - g["sk_centers"]).max() <= 10 * float(g["stmt_vs_sklearn_max_abs"])
    again = U.KMeansQuantizer.fit(xd, init=init)
    assert torch.equal(again.centers, q.centers) and again.inertia_ == q.inertia_ and again.history_ == q.history_
    assert torch.equal(again.counts_, q.counts_)
    chunks = U.KMeansQuantizer.fit([xd[:1000], xd[1000:]], init=init)      # the same rows in two chunks
    check_fit(chunks, g["fit"], g["x"])
    capped = U.KMeansQuantizer.fit(xd, init=init, max_iter=2)
    assert capped.n_iter_ == 2 and len(capped.history_) == 2
    assert abs(capped.inertia_ - g["fit"]["history"][2]["inertia"]) <= 1e-5 * capped.inertia_


def test_fit_from_kmeans_plusplus(goldens):
    g = goldens["a"]
    K = int(g["K"])
    want = KN.fit(g["x"], g["x"][g["pp_rows"]], max_iter=100, tol=0.0)
    assert want["n_iter"] == int(g["pp_fit_n_iter"])
    q = U.KMeansQuantizer.fit(torch.from_numpy(g["x"]).to(DEV), n_clusters=K, init="k-means++", seed=int(g["seed_pp"]))
    check_fit(q, want, g["x"])
    r = U.KMeansQuantizer.fit(torch.from_numpy(g["x"]).to(DEV), n_clusters=K, init="random", seed=1, max_iter=0)
    assert r.n_iter_ == 0 and r.history_ == [] and np.array_equal(r.centers.cpu().numpy(), g["x"][KN.random_rows(g["x"].shape[0], 1)[:K]])
    assert abs(r.inertia_ - KN.fit(g["x"], r.centers.cpu().numpy(), max_iter=0)["inertia"]) <= 1e-11 * r.inertia_


def test_save_round_trip(goldens, tmp_path):
    g = goldens["a"]
    xd = torch.from_numpy(g["x"]).to(DEV)
    q = U.KMeansQuantizer.fit(xd, init=torch.from_numpy(g["init"]))
    units = q.quantize(xd.unsqueeze(0))
    q.save(tmp_path / "km.pt")
    d = torch.load(tmp_path / "km.pt")
    assert d["n_iter"] == q.n_iter_ and d["inertia"] == q.inertia_ and torch.equal(d["counts"], q.counts_.cpu())
    assert torch.equal(U.KMeansQuantizer.from_centers(d["centers"]).to(DEV).quantize(xd.unsqueeze(0)), units)
    pytest.importorskip("sklearn")
    pytest.importorskip("joblib")
    q.save(tmp_path / "km.bin")
    back = U.KMeansQuantizer(str(tmp_path / "km.bin")).to(DEV)
    assert torch.equal(back.centers, q.centers) and torch.equal(back.quantize(xd.unsqueeze(0)), units)


def test_command_line(tmp_path):
    out = tmp_path / "codebook.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fit_units.py"), "--synthetic", "2000", "--n_clusters", "32", "--max_iter", "5",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("iter")]
    assert 1 <= len(lines) <= 5
    inertias = [float(ln.split("inertia")[1].split()[0]) for ln in lines]
    assert all(np.isfinite(inertias)) and all(b <= a for a, b in zip(inertias, inertias[1:]))
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("K 32  D 64  rows used 2000  skipped 0  n_iter")
    q = U.KMeansQuantizer(str(out))                          # finetune.py's --kmeans_checkpoint path
    assert tuple(q.centers.shape) == (32, 64)
    assert torch.equal(U.KMeansQuantizer.from_centers(torch.load(out)["centers"]).centers, q.centers)
