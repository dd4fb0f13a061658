#!/usr/bin/env python3
"""Mel front end latency: the HIP library (unitspeech_amd.mel.MelSpectrogram) against the reference's function restated with eager
`torch.stft` (tools/mel_torch.py, fp32) on the same GPU.

    python bench_mel.py [--runs 50] [--warmup 5] [--inner 20] [--out profiles/bench_mel.json]

Cases: B = 1 at 10 s (one reference utterance, finetune.py:86-104) and B = 32 at 2 s crops (a training batch), 22050 Hz, the reference's
configuration (1024 / 256 / 1024 / 80 / 0-8000).  Both legs run in this process on the same seeded waveforms, alternating run by run; a run is
`--inner` back-to-back calls between two device events (host work of the calls included), so one timed window is milliseconds and not one
launch; the median over the runs is reported per call.  The filter bank and window of the eager leg live on the device, as the reference
caches them.  The last line printed is one JSON object with every row; --out also writes it to a file.
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
from mel_torch import mel_spectrogram_torch  # noqa: E402

from unitspeech_amd.mel import MelSpectrogram, synthetic_waveform  # noqa: E402

SR, N_FFT, HOP, WIN, MELS = 22050, 1024, 256, 1024, 80
HIP_LAUNCHES = 3                   # framing, windowed DFT, mel projection (per 64 batch items)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / inner, out


def mel_flops(B: int, T: int, live: int) -> float:
    """Algorithmic FLOPs (2 x multiply-adds) of the two matrix products as the library runs them: 2 `live` DFT rows of n_fft terms and
    num_mels rows of `live` terms per frame."""
    return 2.0 * B * (T // HOP) * (2 * live * N_FFT + MELS * live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP mel front end has no CPU fallback and this benchmark measures nothing without one")
    dev = torch.device("cuda", 0)
    model = MelSpectrogram(N_FFT, MELS, SR, HOP, WIN, 0, 8000).to(dev)
    live = int(model.mel_basis.any(dim=0).nonzero().max()) + 1
    rows = []
    for name, B, T in (("utterance_10s", 1, 10 * SR), ("crops_32x2s", 32, 2 * SR)):
        wav = torch.stack([torch.from_numpy(synthetic_waveform(T, b, SR)) for b in range(B)]).to(dev)
        t_hip, t_eager = [], []
        with torch.no_grad():
            for i in range(args.warmup + args.runs):
                dt, y_hip = timed(lambda: model(wav), args.inner)
                if i >= args.warmup:
                    t_hip.append(dt)
                dt, y_eager = timed(lambda: mel_spectrogram_torch(wav, model.mel_basis, model.window, N_FFT, HOP, WIN, dtype=torch.float32),
                                    args.inner)
                if i >= args.warmup:
                    t_eager.append(dt)
        hip, eager = statistics.median(t_hip), statistics.median(t_eager)
        flops = mel_flops(B, T, live)
        diff = float((y_hip.double() - y_eager.double()).abs().max())
        rows.append({"case": name, "B": B, "T": T, "frames": T // HOP, "live_bins": live, "hip_us": hip * 1e6,
                     "hip_us_min_max": [min(t_hip) * 1e6, max(t_hip) * 1e6], "eager_us": eager * 1e6,
                     "eager_us_min_max": [min(t_eager) * 1e6, max(t_eager) * 1e6], "speedup_vs_eager": eager / hip, "runs": args.runs,
                     "calls_per_run": args.inner, "gflop": flops / 1e9, "hip_tflops_end_to_end": flops / hip / 1e12,
                     "hip_launches_per_call": HIP_LAUNCHES * ((B + 63) // 64), "max_abs_diff_hip_vs_eager": diff})
        print(f"{name}: HIP {hip * 1e6:8.1f} us/call ({flops / 1e9:.2f} GFLOP, {flops / hip / 1e12:.2f} TFLOP/s end to end) | eager torch.stft "
              f"{eager * 1e6:8.1f} us/call  speed-up {eager / hip:.2f}x  max |diff| {diff:.2e}", flush=True)
    result = {"bench": "mel", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
