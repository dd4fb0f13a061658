#!/usr/bin/env python3
"""Unit extraction benchmark: dense features [B, T, 768] -> mel-rate (unit, duration), K = 1000 centres.

    python bench_unit_quantizer.py [--runs 10] [--warmup 3] [--quick] [--no-host]

Three cases: B = 1 at T = 500 and T = 1500 (10 s and 30 s of speech at 50 Hz), and B = 32 with ragged lengths up to 1500.
  library leg   `KMeansQuantizer.encode` (one us_units_encode call: score GEMM, decision, fp64 re-evaluation of the flagged rows,
                process_unit), inputs and outputs on the device, no host synchronisation inside.
  host leg      the reference's path restated (finetune.py:112-128): device -> host copy of the features, scikit-learn
                `KMeans.predict` (16 threads), `torch.unique_consecutive`, a process_unit that expands the units to one list entry
                per 16 kHz sample and takes `torch.mode` per hop, and the copy of (unit, duration) back to the device; item by item
                for the batch.  `copies` is that leg's two copies alone.
Both legs are timed with a host clock between device synchronisations, interleaved run by run after the warm-up; median [min, max].
`quantize` times the us_units_quantize call alone with device events; its rate is 2 rows K D over that time (the call's three kernels
and one memset, so a lower bound on the GEMM kernel's own rate, which the rocprofv3 summary under profiles/ gives).
The last line is one JSON object.
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
from unitspeech_amd.units import KMeansQuantizer, synthetic_centers, synthetic_dense  # noqa: E402

K, D, RATE, HOP = 1000, 768, 16000, 256
PEAK_F32_MFMA_TFLOPS = 157.3


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_process_unit(units, durations, sampling_rate, hop_length):
    """The reference's algorithm at the reference's cost: a Python list with one entry per sample, `torch.mode` per hop, a Python loop
    for the run lengths."""
    spf = sampling_rate // 50
    samples = []
    for u, d in zip(units.tolist(), durations.tolist()):
        samples.extend([u] * (d * spf))
    n = len(samples) // hop_length
    frames = torch.LongTensor(samples)[:n * hop_length].reshape(-1, hop_length).mode(1)[0].tolist()
    out_u, out_d = [], []
    for u in frames:
        if out_u and out_u[-1] == u:
            out_d[-1] += 1
        else:
            out_u.append(u)
            out_d.append(1)
    return torch.LongTensor(out_u), torch.LongTensor(out_d)


def planted_kmeans(centers):
    from sklearn.cluster import KMeans
    km = KMeans(n_clusters=centers.shape[0], n_init=1, max_iter=1, random_state=0).fit(centers)
    km.cluster_centers_ = np.ascontiguousarray(centers, dtype=np.float32)
    km._n_threads = 16
    return km


def run_case(name, q, km, dense, lengths, runs, warmup):
    dev = dense.device
    B, T = dense.shape[:2]
    lens = torch.tensor(lengths, dtype=torch.int64, device=dev)
    box = {}

    def library():
        box["lib"] = q.encode(dense, lens, RATE, HOP)

    def host():
        out = []
        for b in range(B):
            x = dense[b, :lengths[b]].cpu().numpy()
            units = torch.from_numpy(km.predict(x))
            u, d = torch.unique_consecutive(units, return_counts=True)
            pu, pd = host_process_unit(u, d, RATE, HOP)
            out.append((pu.to(dev), pd.to(dev)))
        box["host"] = out

    def copies():
        for b in range(B):
            x = dense[b, :lengths[b]].cpu()
            n = max(1, lengths[b] * (RATE // 50) // HOP)
            torch.zeros(n, dtype=torch.int64).to(dev), torch.zeros(n, dtype=torch.int64).to(dev)
            del x

    legs = {"library": library, "copies": copies}
    if km is not None:
        legs["host"] = host
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            ts[k].append(wall(fn))
    tq = []
    for _ in range(runs):
        tq.append(events(lambda: q.quantize(dense, lens)))
    rows = int(sum(lengths))
    bad, flagged = (int(v) for v in q.last_counters.cpu())
    row = dict(case=name, B=B, T=T, rows=rows, flagged_rows=flagged, flagged_share=round(flagged / rows, 5), nonfinite_rows=bad,
               quantize=stats(tq), quantize_tflops=round(2.0 * B * T * K * D / (statistics.median(tq) * 1e-3) / 1e12, 2),
               **{k: stats(v) for k, v in ts.items()})
    row["quantize_share_of_f32_mfma_peak"] = round(row["quantize_tflops"] / PEAK_F32_MFMA_TFLOPS, 4)
    if km is not None:
        unit, dur, n = box["lib"]
        same = all(torch.equal(unit[b, :int(n[b])], box["host"][b][0]) and torch.equal(dur[b, :int(n[b])].long(), box["host"][b][1])
                   for b in range(B))
        row["equal_to_host_leg"] = bool(same)
        row["speedup_vs_host"] = round(row["host"]["median_ms"] / row["library"]["median_ms"], 1)
    line = f"{name:>12}: library {row['library']['median_ms']:8.3f} ms [{row['library']['min_ms']:.3f}, {row['library']['max_ms']:.3f}]"
    if km is not None:
        line += f"  host {row['host']['median_ms']:9.2f} ms [{row['host']['min_ms']:.2f}, {row['host']['max_ms']:.2f}]"
    line += (f"  copies {row['copies']['median_ms']:7.3f} ms  quantize {row['quantize']['median_ms']:.3f} ms = {row['quantize_tflops']:.1f} TFLOP/s"
             f"  flagged {100 * row['flagged_share']:.2f} %")
    print(line, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="T = 100 / 200 and B = 4: a functional check, not a measurement")
    ap.add_argument("--no-host", action="store_true", help="library leg only (profiling runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the unit extraction has no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.set_num_threads(16)
    centers = synthetic_centers(K, D, 0)
    q = KMeansQuantizer.from_centers(centers).to(dev)
    km = None
    if not a.no_host:
        try:
            km = planted_kmeans(centers)
        except ImportError:
            print("scikit-learn is not installed: host leg not measured", flush=True)
    t1, t2, bn = (100, 200, 4) if a.quick else (500, 1500, 32)
    g = np.random.default_rng(0)
    ragged = [int(v) for v in g.integers(t2 // 3, t2 + 1, size=bn)]
    ragged[0] = t2
    cases = [(f"B=1 T={t1}", 1, t1, [t1]), (f"B=1 T={t2}", 1, t2, [t2]), (f"B={bn} ragged", bn, t2, ragged)]
    rows = []
    for name, B, T, lengths in cases:
        dense = torch.from_numpy(np.stack([synthetic_dense(centers, T, 1 + b) for b in range(B)])).to(dev)
        rows.append(run_case(name, q, km, dense, lengths, a.runs, a.warmup))
    print(json.dumps({"bench": "unit_quantizer", "K": K, "D": D, "sampling_rate": RATE, "hop_length": HOP, "runs": a.runs, "warmup": a.warmup,
                      "quick": a.quick, "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS, "cases": rows}))


if __name__ == "__main__":
    main()
