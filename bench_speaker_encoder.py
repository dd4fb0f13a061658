#!/usr/bin/env python3
"""ECAPA-TDNN speaker encoder latency: the HIP library (unitspeech_amd.speaker_encoder.ECAPA_TDNN.forward_features) against eager
PyTorch on the same GPU.

    python bench_speaker_encoder.py [--frames 149,499,1499] [--runs 20] [--warmup 3] [--out profiles/speaker_encoder_bench.json]

Reference size (WavLM-large hidden states: L = 25, C = 1024; channels 512, emb 256), B = 1.  Both legs run in this process on the same
seeded weights and hidden states, interleaved run by run; each run is timed with device events around the whole call (host work of the
call included) and the median is reported.  The eager leg is tools/speaker_encoder_torch.py (the reference's forward restated in
torch ops).  `--kernel_stats CSV` (a `rocprofv3 --kernel-trace --stats` summary of a `--no_eager --frames N` run) adds the combine
kernel's average time and the fraction of the HBM peak its L*T*C*4-byte read reaches.  The last line printed is one JSON object with
every row; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402

from unitspeech_amd.speaker_encoder import synthetic_ecapa_state_dict, synthetic_hidden_states, synthetic_speaker_embedder  # noqa: E402

HBM_PEAK = 8.0e12                # MI355X HBM3E, bytes/s (specification)
# kernel launches of one us_speaker_forward without global context: combine, instance norm, layer1, 3 x (conv, Res2 chain, conv, row
# mean, SE, scale + residual), conv, 2 pooling convolutions, pooling, linear
HIP_LAUNCHES = 2 + 1 + 3 * 6 + 1 + 2 + 1 + 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3, out


def ecapa_flops(T: int, L: int = 25, C: int = 1024, ch: int = 512, emb: int = 256) -> float:
    """Algorithmic FLOPs (2 x multiply-adds) of one forward, batch 1: the combine and every convolution / linear."""
    w = ch // 8
    f = 2.0 * L * T * C + 2.0 * C * ch * 5 * T
    f += 3 * (2 * 2.0 * ch * ch * T + 7 * 2.0 * w * w * 3 * T + 2 * 2.0 * ch * 128)
    f += 2.0 * 3 * ch * 1536 * T + 2 * 2.0 * 1536 * 128 * T + 2.0 * 3072 * emb
    return f


def combine_time_from_stats(path):
    with open(path) as f:
        for row in csv.DictReader(f):
            if "sp_combine_kernel" in row.get("Name", ""):
                return float(row["AverageNs"]) * 1e-9, int(row["Calls"])
    return None, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="149,499,1499")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_eager", action="store_true", help="time the HIP path only (e.g. under a kernel trace)")
    ap.add_argument("--kernel_stats", default=None, help="rocprofv3 kernel stats CSV of a --no_eager run at --stats_frames")
    ap.add_argument("--stats_frames", type=int, default=499)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP speaker encoder has no CPU fallback and this benchmark measures nothing without one")
    dev = torch.device("cuda", 0)
    model = synthetic_speaker_embedder(256).to(dev)
    cfg = model.config()
    sd = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_ecapa_state_dict(cfg, 0).items() if v.dtype.kind == "f"}
    rows = []
    for T in (int(t) for t in args.frames.split(",")):
        hid = torch.from_numpy(synthetic_hidden_states(25, 1, T, 1024, T)).to(dev)
        t_hip, t_eager = [], []
        with torch.no_grad():
            for i in range(args.warmup + args.runs):
                dt, y_hip = timed(lambda: model.forward_features(hid))
                if i >= args.warmup:
                    t_hip.append(dt)
                if not args.no_eager:
                    dt, y_eager = timed(lambda: ecapa_forward(cfg, sd, hid))
                    if i >= args.warmup:
                        t_eager.append(dt)
        hip = statistics.median(t_hip)
        flops = ecapa_flops(T)
        row = {"B": 1, "T": T, "L": 25, "C": 1024, "hip_ms": hip * 1e3, "hip_ms_min_max": [min(t_hip) * 1e3, max(t_hip) * 1e3], "runs": args.runs,
               "gflop": flops / 1e9, "hip_tflops": flops / hip / 1e12, "hip_launches_per_forward": HIP_LAUNCHES,
               "hidden_state_bytes": 25 * T * 1024 * 4}
        line = f"T={T:5d}: HIP {hip * 1e3:7.3f} ms ({flops / 1e9:5.1f} GFLOP, {row['hip_tflops']:5.1f} TFLOP/s, {HIP_LAUNCHES} launches)"
        if not args.no_eager:
            eager = statistics.median(t_eager)
            rel = float((y_hip.double() - y_eager.double()).norm() / y_eager.double().norm())
            row.update({"eager_ms": eager * 1e3, "eager_ms_min_max": [min(t_eager) * 1e3, max(t_eager) * 1e3], "speedup_vs_eager": eager / hip,
                        "rel_l2_hip_vs_eager": rel})
            line += f" | eager {eager * 1e3:7.3f} ms  speed-up {eager / hip:.2f}x  rel-L2 {rel:.2e}"
        if args.kernel_stats and T == args.stats_frames:
            t_c, calls = combine_time_from_stats(args.kernel_stats)
            if t_c:
                row.update({"combine_kernel_us": t_c * 1e6, "combine_kernel_calls_traced": calls,
                            "combine_fraction_of_hbm_peak": row["hidden_state_bytes"] / t_c / HBM_PEAK})
                line += f" | combine {t_c * 1e6:.1f} us = {100 * row['combine_fraction_of_hbm_peak']:.0f} % of {HBM_PEAK / 1e12:.0f} TB/s"
        rows.append(row)
        print(line, flush=True)
    result = {"bench": "speaker_encoder", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
    if not args.no_eager and any(r["speedup_vs_eager"] < 1.0 for r in rows):
        raise SystemExit("the HIP path is slower than eager PyTorch at one of the lengths")


if __name__ == "__main__":
    main()
