#!/usr/bin/env python3
"""Level-normalisation benchmark: active speech level + gain (us_level_measure + us_level_apply) at 22050 Hz, int16 in and out.

    python bench_level.py [--runs 10] [--warmup 3] [--quick] [--json PATH]

  hip calls     the two library calls back to back on buffers allocated once (six launches), timed with device events
  hip python    `unitspeech_amd.level.normalize_level(..., out_int16=True)` as the scripts call it: the same plus its allocations
  host route    what leaving the device costs: the batch copied to the host, the fp64 numpy yardstick item by item (tools/level_numpy.py,
                its envelope by scipy.signal.lfilter when scipy is importable), the result copied back; wall clock
  device copy   a plain device copy of the same bytes: the floor of one read and one write
at B = 1 x 10 s and B = 32 ragged, 2.5 to 5 s.  The legs run interleaved, run by run, after the warm-up; median [min, max].  The hip
output is compared with the host route's (equal samples expected).  The last line is one JSON object.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import level_numpy as L  # noqa: E402
from unitspeech_amd import _lib, level  # noqa: E402

RATE, NDB = 22050, -26.0
SHAPES = {"B1x10s": [10.0], "B32x5s_ragged": [5.0 - 2.5 * i / 31 for i in range(32)]}
QUICK = {"B3x0.5s_ragged": [0.5, 0.2, 0.35]}

try:
    from scipy.signal import lfilter
except ImportError:                      # the yardstick's own sequential envelope then
    lfilter = None


def host_envelope(x):
    if lfilter is None:
        return L.envelope(x, RATE)
    g, _ = L.constants(RATE)
    return lfilter([1.0 - g], [1.0, -g], lfilter([1.0 - g], [1.0, -g], np.abs(x)))


def host_normalize(x):
    """One item on the host: int16 -> int16, the yardstick's steps."""
    v = L.to_full_scale(x)
    a = L.activity_counts(host_envelope(v), L.constants(RATE)[1])
    lv, _, _ = L.level_from_counts(float(np.sum(v * v)), len(v), a)
    return L.round_saturate(L.scaled_lsb(x, L.gain_factor(lv, NDB)))[0]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def walled(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def case(name, seconds, runs, warmup, dev):
    lens = [int(s * RATE) for s in seconds]
    B, T = len(lens), max(lens)
    host = np.zeros((B, T), dtype=np.int16)
    for b, n in enumerate(lens):
        host[b, :n] = L.burst_signal(n, RATE, seed=b)
    x = torch.from_numpy(host).to(dev)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    lib = _lib.load()
    nws = int(lib.us_level_workspace_bytes(B, T))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    st = torch.empty(B, 8, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 15, dtype=torch.int64, device=dev)
    gain = torch.empty(B, dtype=torch.float64, device=dev)
    clipped = torch.empty(B, dtype=torch.int64, device=dev)
    out, copy = torch.empty_like(x), torch.empty_like(x)
    box = {}

    def hip_calls():
        s = torch.cuda.current_stream().cuda_stream
        rc = lib.us_level_measure(x.data_ptr(), _lib.US_LEVEL_I16, 0, ln.data_ptr(), B, T, RATE, st.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                  nws, s)
        _lib.check(rc, None, "us_level_measure")
        rc = lib.us_level_apply(x.data_ptr(), _lib.US_LEVEL_I16, 0, ln.data_ptr(), B, T, st.data_ptr(), NDB, out.data_ptr(), _lib.US_LEVEL_I16,
                                gain.data_ptr(), clipped.data_ptr(), ws.data_ptr(), nws, s)
        _lib.check(rc, None, "us_level_apply")

    def hip_python():
        box["hip"] = level.normalize_level(x, RATE, NDB, lengths=ln, out_int16=True)[0]

    def host_route():
        h = x.cpu().numpy()
        y = np.zeros_like(h)
        for b, n in enumerate(lens):
            y[b, :n] = host_normalize(h[b, :n])
        box["host"] = torch.from_numpy(y).to(dev)

    def device_copy():
        copy.copy_(x)

    legs = dict(hip_calls=(hip_calls, timed), hip_python=(hip_python, timed), host_route=(host_route, walled), device_copy=(device_copy, timed))
    for _ in range(warmup):
        for fn, _ in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k, (fn, clock) in legs.items():
            ts[k].append(clock(fn))
    med = {k: statistics.median(v) for k, v in ts.items()}
    differing = int((box["hip"] != box["host"]).sum()) + int((out != box["host"]).sum())
    row = dict(shape=name, B=B, samples=T, total_samples=sum(lens), chunks_per_item=-(-T // level.chunk()), workspace_bytes=nws,
               **{k: stats(v) for k, v in ts.items()}, speedup_vs_host_route=round(med["host_route"] / med["hip_calls"], 2),
               times_device_copy=round(med["hip_calls"] / med["device_copy"], 2), samples_differing_from_host_route=differing,
               host_envelope="scipy.signal.lfilter" if lfilter is not None else "python loop")
    print(f"{name:16s} hip calls {med['hip_calls']:8.4f} ms  python {med['hip_python']:8.4f} ms  host route {med['host_route']:9.3f} ms  "
          f"device copy {med['device_copy']:7.4f} ms  x{row['speedup_vs_host_route']:.1f} vs host  ({differing} samples differ)", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes: a functional check, not a measurement")
    ap.add_argument("--json", type=str, default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the level has no CPU fallback")
    dev = torch.device("cuda", 0)
    rows = [case(name, seconds, max(a.runs, 1), a.warmup, dev) for name, seconds in (QUICK if a.quick else SHAPES).items()]
    out = {"bench": "level_measure_apply", "rate": RATE, "ndb": NDB, "chunk": level.chunk(), "runs": a.runs, "warmup": a.warmup, "quick": a.quick,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
