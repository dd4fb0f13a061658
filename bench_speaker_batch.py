#!/usr/bin/env python3
"""ECAPA-TDNN speaker encoder throughput over a set of utterances of different lengths: one call per utterance against ragged batches
(unitspeech_amd.speaker_encoder.ECAPA_TDNN.forward_features with `lengths`).

    python bench_speaker_batch.py [--utterances 64] [--reps 10] [--out profiles/bench_speaker_batch.json]

Reference-size trunk (WavLM-large hidden states: L = 25, C = 1024; channels 512, emb 256) with seeded weights; 64 seeded utterances of
99 to 499 frames (2 to 10 s).  Three legs, interleaved repetition by repetition in this process, each after one untimed pass over every
shape it uses:
  (a) one forward_features call per utterance (the only way before the trunk took lengths);
  (b) ragged batches of 8, the utterances sorted by length;
  (c) ragged batches of 32, sorted likewise.
The padded batches are built before the clock starts (in a pipeline the upstream writes them); device events surround each whole leg,
host work of the calls included.  Printed: utterances per second as median [min, max] over the repetitions, the kernel launches of a
leg, and the largest difference between the embeddings of (a) and (c), which is 0.  The last line is one JSON object; --out also writes
it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.speaker_encoder import synthetic_speaker_embedder  # noqa: E402

L, C = 25, 1024
# kernel launches of one forward without global context (bench_speaker_encoder.py), per launch group of 32 items
LAUNCHES = 2 + 1 + 3 * 6 + 1 + 2 + 1 + 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--min_frames", type=int, default=99)
    ap.add_argument("--max_frames", type=int, default=499)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP speaker encoder has no CPU fallback and this benchmark measures nothing without one")
    if args.reps < 10:
        raise SystemExit("--reps: at least 10 repetitions")
    dev = torch.device("cuda", 0)
    model = synthetic_speaker_embedder(256).to(dev)
    n = args.utterances
    frames = [int(t) for t in np.random.Generator(np.random.Philox(key=8000 + args.seed)).integers(args.min_frames, args.max_frames + 1, size=n)]
    g = torch.Generator(device=dev).manual_seed(args.seed)
    utts = [torch.randn(L, 1, t, C, device=dev, generator=g) for t in frames]
    order = sorted(range(n), key=lambda i: (frames[i], i))

    def batches(size):
        out = []
        for k in range(0, n, size):
            idx = order[k:k + size]
            lens = [frames[i] for i in idx]
            x = torch.zeros(L, len(idx), max(lens), C, device=dev)
            for b, i in enumerate(idx):
                x[:, b, :lens[b]] = utts[i][:, 0]
            out.append((idx, lens, x))
        return out

    def run_alone():
        return torch.cat([model.forward_features(u) for u in utts])

    def run_batched(bs):
        emb = torch.empty(n, model.emb_dim, device=dev)
        for idx, lens, x in bs:
            emb[idx] = model.forward_features(x, lens)
        return emb

    b8, b32 = batches(8), batches(32)
    legs = [("alone", run_alone, n * LAUNCHES),
            ("batch8", lambda: run_batched(b8), len(b8) * LAUNCHES),
            ("batch32", lambda: run_batched(b32), sum(-(-len(idx) // 32) for idx, _, _ in b32) * LAUNCHES)]
    times = {name: [] for name, _, _ in legs}
    outs = {}
    with torch.no_grad():
        for name, fn, _ in legs:                           # every shape once, untimed: the workspace has its final size afterwards
            outs[name] = fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn, _ in legs:
                dt, outs[name] = timed(fn)
                times[name].append(dt)
    diff8 = float((outs["alone"] - outs["batch8"]).abs().max())
    diff32 = float((outs["alone"] - outs["batch32"]).abs().max())
    total = sum(frames)
    result = {"bench": "speaker_batch", "device": torch.cuda.get_device_name(0), "utterances": n, "frames_min_max": [min(frames), max(frames)],
              "frames_total": total, "reps": args.reps, "max_abs_diff_alone_vs_batch8": diff8, "max_abs_diff_alone_vs_batch32": diff32, "legs": {}}
    base = statistics.median(times["alone"])
    for name, _, launches in legs:
        t = times[name]
        med = statistics.median(t)
        padded = {"alone": total, "batch8": sum(len(i) * max(l) for i, l, _ in b8), "batch32": sum(len(i) * max(l) for i, l, _ in b32)}[name]
        result["legs"][name] = {"utterances_per_s": n / med, "utterances_per_s_min_max": [n / max(t), n / min(t)], "leg_ms": med * 1e3,
                                "leg_ms_min_max": [min(t) * 1e3, max(t) * 1e3], "launches": launches, "padded_frames": padded,
                                "speedup_vs_alone": base / med}
        print(f"{name:8s}: {n / med:8.1f} utterances/s [{n / max(t):.1f}, {n / min(t):.1f}]  leg {med * 1e3:8.3f} ms  {launches:5d} launches  "
              f"{total} frames padded to {padded}  {base / med:.2f}x", flush=True)
    print(f"largest |alone - batch8| = {diff8:.1e}, |alone - batch32| = {diff32:.1e}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
