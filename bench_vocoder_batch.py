#!/usr/bin/env python3
"""BigVGAN vocoder throughput over a set of mels of different lengths: one call per utterance against ragged batches
(unitspeech_amd.vocoder.BigVGAN.forward with `lengths`).

    python bench_vocoder_batch.py [--utterances 64] [--reps 10] [--out profiles/bench_vocoder_batch.json]

The 22 kHz / 80-band large generator with seeded weights.  Two workloads of 64 seeded mels each: 2 to 10 s (172 to 861 frames), and 1 to
3 s (86 to 258 frames), where the single-item launches fill the GPU worst.  Three legs per workload, interleaved repetition by repetition
in this process after two untimed passes over every leg:
  (a) one forward call per utterance (the only correct way before the vocoder took lengths);
  (b) ragged batches of 8, the utterances sorted by length;
  (c) ragged batches of 32, sorted likewise.
The padded batches are built before the clock starts (in a pipeline the decoder writes them); device events surround each whole leg, host
work of the calls included.  Printed: utterances per second as median [min, max] over the repetitions, each ragged leg's ratio to (a),
and whether the samples of (b) and (c) are those of (a) bit for bit.  The last line is one JSON object, also written to --out.
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
from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BigVGAN, synthetic_bigvgan_state_dict  # noqa: E402

WORKLOADS = (("2-10s", 172, 861), ("1-3s", 86, 258))
WARMUP = 2


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3, out


def workload(model, dev, name, lo, hi, n, reps, seed):
    frames = [int(t) for t in np.random.Generator(np.random.Philox(key=8100 + seed)).integers(lo, hi + 1, size=n)]
    g = torch.Generator(device=dev).manual_seed(seed)
    mels = [torch.randn(1, 80, t, device=dev, generator=g) * 2 - 5 for t in frames]
    order = sorted(range(n), key=lambda i: (frames[i], i))
    hop = model.hop

    def batches(size):
        out = []
        for k in range(0, n, size):
            idx = order[k:k + size]
            lens = [frames[i] for i in idx]
            x = torch.zeros(len(idx), 80, max(lens), device=dev)
            for b, i in enumerate(idx):
                x[b, :, :lens[b]] = mels[i][0]
            out.append((idx, lens, x))
        return out

    def run_alone():
        return [model(m) for m in mels]

    def run_batched(bs):
        wavs = [None] * n
        for idx, lens, x in bs:
            out = model(x, lengths=lens)
            for b, i in enumerate(idx):
                wavs[i] = out[b:b + 1, :, :lens[b] * hop]
        return wavs

    b8, b32 = batches(8), batches(32)
    legs = [("alone", run_alone), ("batch8", lambda: run_batched(b8)), ("batch32", lambda: run_batched(b32))]
    times = {name: [] for name, _ in legs}
    outs = {}
    with torch.no_grad():
        for _ in range(WARMUP):
            for leg, fn in legs:
                outs[leg] = fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for leg, fn in legs:
                dt, outs[leg] = timed(fn)
                times[leg].append(dt)
    same = {leg: all(torch.equal(a, b) for a, b in zip(outs["alone"], outs[leg])) for leg in ("batch8", "batch32")}
    total = sum(frames)
    padded = {"alone": total, "batch8": sum(len(i) * max(l) for i, l, _ in b8), "batch32": sum(len(i) * max(l) for i, l, _ in b32)}
    res = {"frames_min_max": [min(frames), max(frames)], "frames_total": total, "audio_s": total * hop / 22050.0,
           "bit_identical_to_alone": same, "legs": {}}
    base = statistics.median(times["alone"])
    print(f"workload {name}: {n} mels, {min(frames)} to {max(frames)} frames, {total * hop / 22050.0:.1f} s of audio")
    for leg, _ in legs:
        t = times[leg]
        med = statistics.median(t)
        res["legs"][leg] = {"utterances_per_s": n / med, "utterances_per_s_min_max": [n / max(t), n / min(t)], "leg_ms": med * 1e3,
                            "leg_ms_min_max": [min(t) * 1e3, max(t) * 1e3], "padded_frames": padded[leg], "ratio_vs_alone": base / med}
        print(f"  {leg:8s}: {n / med:8.2f} utterances/s [{n / max(t):.2f}, {n / min(t):.2f}]  leg {med * 1e3:9.2f} ms  {total} frames padded to "
              f"{padded[leg]}  {base / med:.3f}x", flush=True)
    print(f"  samples of batch8 / batch32 equal to alone bit for bit: {same['batch8']} / {same['batch32']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workloads", default=",".join(w[0] for w in WORKLOADS), help="comma-separated subset of " + ", ".join(w[0] for w in WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_vocoder_batch.json"), help="where the JSON object is also written")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP vocoder has no CPU fallback and this benchmark measures nothing without one")
    if args.reps < 10:
        raise SystemExit("--reps: at least 10 repetitions")
    dev = torch.device("cuda", 0)
    model = BigVGAN(BIGVGAN_22KHZ_80BAND)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(BIGVGAN_22KHZ_80BAND, 0).items()})
    model = model.to(dev).eval()
    model.remove_weight_norm()
    result = {"bench": "vocoder_batch", "device": torch.cuda.get_device_name(0), "config": "BIGVGAN_22KHZ_80BAND", "utterances": args.utterances,
              "reps": args.reps, "warmup": WARMUP, "workloads": {}}
    want = args.workloads.split(",")
    for name, lo, hi in WORKLOADS:
        if name in want:
            result["workloads"][name] = workload(model, dev, name, lo, hi, args.utterances, args.reps, args.seed)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
