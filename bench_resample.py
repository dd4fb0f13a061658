#!/usr/bin/env python3
"""Resampler latency: the HIP library (unitspeech_amd.resample.Resample) against torchaudio's strided convolution restated with eager
`F.conv1d` (tools/resample_torch.py, fp32) on the same GPU.

    python bench_resample.py [--runs 50] [--warmup 5] [--inner 20] [--out profiles/bench_resample.json]

Cases: 22050 -> 16000 at B = 1 x 10 s (one reference utterance, finetune.py:113) and B = 32 x 2 s (a batch of crops), and 16000 -> 22050 at
B = 1 x 10 s (data.py:75).  Both legs run in this process on the same seeded waveforms, alternating run by run; a run is `--inner`
back-to-back calls between two device events (host work of the calls included), so one timed window is milliseconds and not one launch; the
median over the runs is reported per call.  The kernel of the eager leg lives on the device, as torchaudio's module keeps it.  The last
line printed is one JSON object with every row; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resample_torch import resample_torch  # noqa: E402

from unitspeech_amd.mel import synthetic_waveform  # noqa: E402
from unitspeech_amd.resample import Resample  # noqa: E402

HIP_LAUNCHES = 2                   # fold, GEMM (per 64 batch items)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / inner, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP resampler has no CPU fallback and this benchmark measures nothing without one")
    dev = torch.device("cuda", 0)
    rows = []
    for name, of, nf, B, seconds in (("22k_16k_utterance_10s", 22050, 16000, 1, 10), ("22k_16k_crops_32x2s", 22050, 16000, 32, 2),
                                     ("16k_22k_utterance_10s", 16000, 22050, 1, 10)):
        T = seconds * of
        model = Resample(of, nf).to(dev)
        wav = torch.stack([torch.from_numpy(synthetic_waveform(T, b, of)) for b in range(B)]).to(dev)
        t_hip, t_eager = [], []
        with torch.no_grad():
            for i in range(args.warmup + args.runs):
                dt, y_hip = timed(lambda: model(wav), args.inner)
                if i >= args.warmup:
                    t_hip.append(dt)
                dt, y_eager = timed(lambda: resample_torch(wav, model.kernel, model.width, model.orig, model.new, torch.float32), args.inner)
                if i >= args.warmup:
                    t_eager.append(dt)
        hip, eager = statistics.median(t_hip), statistics.median(t_eager)
        K = model.orig + 2 * model.width
        flops = 2.0 * B * y_hip.shape[-1] * K              # algorithmic: K multiply-adds per output sample
        nbytes = 4.0 * B * (T + y_hip.shape[-1])            # the waveform in, the waveform out
        diff = float((y_hip.double() - y_eager.double()).abs().max())
        rows.append({"case": name, "orig_freq": of, "new_freq": nf, "B": B, "T": T, "out": int(y_hip.shape[-1]), "K": K, "hip_us": hip * 1e6,
                     "hip_us_min_max": [min(t_hip) * 1e6, max(t_hip) * 1e6], "eager_us": eager * 1e6,
                     "eager_us_min_max": [min(t_eager) * 1e6, max(t_eager) * 1e6], "speedup_vs_eager": eager / hip, "runs": args.runs,
                     "calls_per_run": args.inner, "gflop": flops / 1e9, "mbytes_in_out": nbytes / 1e6, "hip_tflops_end_to_end": flops / hip / 1e12,
                     "hip_launches_per_call": HIP_LAUNCHES * ((B + 63) // 64), "max_abs_diff_hip_vs_eager": diff})
        print(f"{name}: HIP {hip * 1e6:8.1f} us/call ({flops / 1e9:.2f} GFLOP, {flops / hip / 1e12:.2f} TFLOP/s end to end) | eager F.conv1d "
              f"{eager * 1e6:8.1f} us/call  speed-up {eager / hip:.2f}x  max |diff| {diff:.2e}", flush=True)
    result = {"bench": "resample", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
