#!/usr/bin/env python3
"""BigVGAN vocoder throughput: the HIP library (unitspeech_amd.vocoder.BigVGAN) against eager PyTorch on the same GPU.

    python bench_vocoder.py [--configs large,base] [--batches 1,8] [--frames 1024] [--runs 10] [--warmup 2]

For every (config, batch) both paths run on the same seeded weights and mel, interleaved run by run; each run is timed with device
events and the median is reported.  The eager leg is tools/vocoder_torch.py (the reference's forward restated in torch ops, weight
norm folded beforehand, i.e. what the reference's get_vocoder() runs).  Printed per row: mel frames/s, the real-time factor
(seconds of compute per second of 22.05 kHz audio), algorithmic FLOPs (bigvgan_flops) and the share of the fp32 matrix-core peak,
the speed-up over eager, and the relative L2 distance between the two outputs on the timed inputs.  The last line is one JSON
object with every row.
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
from vocoder_torch import bigvgan_forward, weights  # noqa: E402

from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BIGVGAN_BASE_22KHZ_80BAND, BigVGAN, bigvgan_flops, synthetic_bigvgan_state_dict  # noqa: E402

CONFIGS = {"large": BIGVGAN_22KHZ_80BAND, "base": BIGVGAN_BASE_22KHZ_80BAND}
FP32_MFMA_PEAK = 157.3e12           # MI355X, v_mfma_f32_32x32x2_f32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="large,base")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_eager", action="store_true", help="time the HIP path only (e.g. under a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP vocoder has no CPU fallback and this benchmark measures nothing without one")
    dev = torch.device("cuda", 0)
    rows = []
    for name in args.configs.split(","):
        h = CONFIGS[name]
        sd_np = synthetic_bigvgan_state_dict(h, 0)
        model = BigVGAN(h)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
        model = model.to(dev).eval()
        sd = {k: torch.from_numpy(v).to(dev) for k, v in sd_np.items()}
        for k in [k[:-9] for k in sd if k.endswith(".weight_g")]:                # fold once, as remove_weight_norm() would
            sd[k + ".weight"] = weights(sd, k)
            del sd[k + ".weight_g"], sd[k + ".weight_v"]
        hop, sr = int(torch.tensor(h["upsample_rates"]).prod()), h["sampling_rate"]
        for B in (int(b) for b in args.batches.split(",")):
            T = args.frames
            g = torch.Generator().manual_seed(B)
            mel = (torch.randn(B, h["num_mels"], T, generator=g) * 2 - 5).to(dev)
            t_hip, t_eager = [], []
            with torch.no_grad():
                for i in range(args.warmup + args.runs):
                    dt, y_hip = timed(lambda: model(mel))
                    if i >= args.warmup:
                        t_hip.append(dt)
                    if not args.no_eager:
                        dt, y_eager = timed(lambda: bigvgan_forward(h, sd, mel))
                        if i >= args.warmup:
                            t_eager.append(dt)
            hip = statistics.median(t_hip)
            flops = bigvgan_flops(h, T) * B
            row = {"config": name, "B": B, "T": T, "hip_ms": hip * 1e3, "hip_frames_per_s": B * T / hip,
                   "hip_rtf": hip / (B * T * hop / sr), "gflop": flops / 1e9, "hip_tflops": flops / hip / 1e12,
                   "hip_share_of_fp32_mfma_peak": flops / hip / FP32_MFMA_PEAK, "runs": args.runs,
                   "hip_ms_min_max": [min(t_hip) * 1e3, max(t_hip) * 1e3]}
            if not args.no_eager:
                eager = statistics.median(t_eager)
                rel = float((y_hip.double() - y_eager.double()).norm() / y_eager.double().norm())
                row.update({"eager_ms": eager * 1e3, "eager_frames_per_s": B * T / eager, "eager_rtf": eager / (B * T * hop / sr),
                            "speedup_vs_eager": eager / hip, "rel_l2_hip_vs_eager": rel,
                            "eager_ms_min_max": [min(t_eager) * 1e3, max(t_eager) * 1e3]})
            rows.append(row)
            line = (f"{name:5s} B={B} T={T}: HIP {hip * 1e3:8.2f} ms  {B * T / hip:9.0f} frames/s  RTF {row['hip_rtf']:.2e}  "
                    f"{row['hip_tflops']:6.1f} TFLOP/s ({100 * row['hip_share_of_fp32_mfma_peak']:.1f} % of fp32 MFMA peak, {flops / 1e9:.0f} GFLOP)")
            if not args.no_eager:
                line += f" | eager {row['eager_ms']:8.2f} ms  speed-up {row['speedup_vs_eager']:.2f}x  rel-L2 {row['rel_l2_hip_vs_eager']:.2e}"
            print(line, flush=True)
    print(json.dumps({"bench": "vocoder", "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
