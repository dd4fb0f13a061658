#!/usr/bin/env python3
"""Codebook fit benchmark: one Lloyd iteration over dense features, N = 200,000 x D = 768 with K = 1000 and N = 50,000 x D = 256 with
K = 100.

    python bench_unit_fit.py [--runs 10] [--warmup 3] [--quick] [--no-host] [--json PATH]

  library leg   the iteration of `KMeansQuantizer.fit`, timed with device events and split into its three parts: assignment
                (us_units_quantize: the exact fp64 argmin), accumulate (us_units_fit_accumulate: inverted index + fp64 gather-sum) and
                update (us_units_fit_update, with the 40-byte read-back of the record).
  eager leg     the same GPU through torch: fp32 `matmul` scores + `argmin` + `index_add_` + `bincount` + a division.  Neither exact
                (fp32 scores) nor reproducible (`index_add_` adds with float atomics).
  sklearn leg   when scikit-learn is importable: `KMeans(init=centres, n_init=1, max_iter=1, algorithm="lloyd").fit` on the host's
                16 threads (it includes scikit-learn's final labelling pass), the features already on the host.
  copy          a device-to-device copy of the feature bytes the accumulate pass reads, timed in the same run: the accumulate pass's
                achieved bytes/s stand beside the copy's.
  skewed        the accumulate pass on a labelling in which one centre owns 90 % of the rows, beside the even labelling.
All legs run interleaved, run by run, after the warm-up; median [min, max].  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd import units as U  # noqa: E402

CASES = [dict(N=200_000, D=768, K=1000), dict(N=50_000, D=256, K=100)]
QUICK = [dict(N=20_000, D=256, K=100), dict(N=5_000, D=64, K=16)]


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def features(N, D, K, dev):
    planted = U.synthetic_centers(K, D, 0)
    x = np.concatenate([U.synthetic_dense(planted, min(20_000, N - s), 1 + s, noise=1.0) for s in range(0, N, 20_000)])
    centers = x[np.random.Generator(np.random.Philox(key=3)).permutation(N)[:K]].copy()       # an early iteration: K rows as centres
    return torch.from_numpy(x).to(dev), torch.from_numpy(centers).to(dev)


def run_case(c, runs, warmup, host, dev):
    N, D, K = c["N"], c["D"], c["K"]
    x, centers = features(N, D, K, dev)
    x3 = x.unsqueeze(0)
    lens = torch.full((1,), N, dtype=torch.int64, device=dev)
    q = U.KMeansQuantizer.from_centers(centers.clone()).to(dev)
    st = U._FitState(K, D, dev)
    new, junk = torch.empty_like(centers), torch.empty_like(centers)
    counts = torch.zeros(K, dtype=torch.int64, device=dev)
    box = {}
    g = torch.Generator(device="cpu").manual_seed(0)
    skew = torch.where(torch.rand(N, generator=g) < 0.9, torch.zeros(N, dtype=torch.int64), torch.randint(1, max(K, 2), (N,), generator=g))
    skew = skew.clamp(max=K - 1).to(dev)
    dst = torch.empty_like(x)

    def assign():
        box["labels"] = q.quantize(x3, lens)

    def accumulate():
        st.accumulate(x3, box["labels"], q.centers)

    def update():
        box["rec"] = st.update(0, q.centers, new, None, counts)

    def accumulate_skewed():
        st.accumulate(x3, skew, q.centers)

    def discard():
        st.update(0, q.centers, junk, None, None)

    def eager():
        s = (centers * centers).sum(1)[None, :] - 2.0 * (x @ centers.T)
        lab = s.argmin(1)
        sums = torch.zeros(K, D, device=dev).index_add_(0, lab, x)
        n = torch.bincount(lab, minlength=K)
        box["eager"] = torch.where(n[:, None] > 0, sums / n[:, None].clamp(min=1), centers)
        box["eager_labels"] = lab

    def copy():
        dst.copy_(x)

    km, xh = None, None
    if host:
        try:
            from sklearn.cluster import KMeans
            xh, ch = x.cpu().numpy(), centers.cpu().numpy()
            km = lambda: KMeans(n_clusters=K, init=ch, n_init=1, max_iter=1, algorithm="lloyd", tol=0).fit(xh)      # noqa: E731
        except ImportError:
            print("scikit-learn is not installed: host leg not measured", flush=True)

    def sklearn_leg():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            km()
            return 1e3 * (time.perf_counter() - t0)

    for _ in range(warmup):
        assign(), accumulate(), update(), accumulate_skewed(), discard(), eager(), copy()
    if km is not None:
        sklearn_leg()
    names = ("assign", "accumulate", "update", "accumulate_skewed", "eager", "copy")
    ts = {k: [] for k in names + (("sklearn",) if km is not None else ())}
    for _ in range(runs):
        ts["assign"].append(events(assign))
        ts["accumulate"].append(events(accumulate))
        ts["update"].append(events(update))
        ts["accumulate_skewed"].append(events(accumulate_skewed))
        discard()
        ts["eager"].append(events(eager))
        ts["copy"].append(events(copy))
        if km is not None:
            ts["sklearn"].append(sklearn_leg())
    row = dict(N=N, D=D, K=K, **{k: stats(v) for k, v in ts.items()})
    med = {k: statistics.median(v) for k, v in ts.items()}
    row["iteration_ms"] = round(med["assign"] + med["accumulate"] + med["update"], 4)
    row["assign_tflops"] = round(2.0 * N * K * D / (med["assign"] * 1e-3) / 1e12, 2)
    nbytes = N * D * 4
    row["accumulate_read_GBps"] = round(nbytes / (med["accumulate"] * 1e-3) / 1e9, 1)
    row["copy_read_GBps"] = round(nbytes / (med["copy"] * 1e-3) / 1e9, 1)
    row["skewed_over_even"] = round(med["accumulate_skewed"] / med["accumulate"], 3)
    row["speedup_vs_eager"] = round(med["eager"] / row["iteration_ms"], 2)
    rec = box["rec"]
    row["n_empty"], row["rows_used"] = rec["n_empty"], rec["rows_used"]
    row["eager_labels_differ"] = int((box["eager_labels"] != box["labels"][0]).sum())
    row["eager_centres_max_abs_diff"] = float((box["eager"] - new).abs().max())
    if km is not None:
        row["speedup_vs_sklearn"] = round(med["sklearn"] / row["iteration_ms"], 1)
    line = (f"N={N} D={D} K={K}: iteration {row['iteration_ms']:.3f} ms = assign {med['assign']:.3f} ({row['assign_tflops']:.1f} TFLOP/s) + "
            f"accumulate {med['accumulate']:.3f} ({row['accumulate_read_GBps']:.0f} GB/s; copy {med['copy']:.3f} ms, {row['copy_read_GBps']:.0f} GB/s) + "
            f"update {med['update']:.3f};  skewed accumulate {med['accumulate_skewed']:.3f} ({row['skewed_over_even']:.2f}x);  eager {med['eager']:.3f} ms")
    if km is not None:
        line += f";  sklearn {med['sklearn']:.1f} ms"
    print(line, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes: a functional check, not a measurement")
    ap.add_argument("--no-host", action="store_true", help="no scikit-learn leg")
    ap.add_argument("--json", type=str, default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the codebook fit has no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.set_num_threads(16)
    rows = [run_case(c, max(a.runs, 1), a.warmup, not a.no_host, dev) for c in (QUICK if a.quick else CASES)]
    out = {"bench": "unit_fit", "runs": a.runs, "warmup": a.warmup, "quick": a.quick, "device": torch.cuda.get_device_name(0), "cases": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
