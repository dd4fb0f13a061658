#!/usr/bin/env python3
"""HuBERT-base encoder benchmark: the HIP library against the eager torch restatement (tools/hubert_torch.py, fp32) on the same GPU.

    python bench_hubert.py [--runs 10] [--warmup 3] [--only NAME] [--no-eager]

Shapes: B = 1 x 10 s, B = 1 x 2 s and B = 8 x 2 s ragged (lengths from 0.6 s to 2 s), seeded base-size weights, all 12 layers.  The two legs
run interleaved, run by run, each timed with device events after the warm-up; median [min, max] of both are printed, then one JSON line.
--only / --no-eager serve a kernel trace of one shape.
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
from hubert_torch import base_config, frames, hubert_forward_torch, synthetic_hubert_state_dict  # noqa: E402

from unitspeech_amd.hubert import HubertModel  # noqa: E402

SHAPES = {
    "B1x10s": [160000],
    "B1x2s": [32000],
    "B8x2s_ragged": [32000, 9600, 20800, 31999, 16000, 27000, 12345, 24000],
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = base_config()
    sd = synthetic_hubert_state_dict(cfg, 0)
    model = HubertModel.base()
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    for name, lens in SHAPES.items():
        if a.only and name != a.only:
            continue
        g = torch.Generator().manual_seed(len(lens))
        wav = (0.3 * torch.randn(len(lens), max(lens), generator=g)).to(dev)
        lengths = lens if len(lens) > 1 else None

        def hip():
            return model(wav, lengths)

        def eager():
            return hubert_forward_torch(sd_dev, cfg, wav, lengths, torch.float32)[-1]

        for _ in range(a.warmup):
            hip()
            if not a.no_eager:
                eager()
        th, te = [], []
        for _ in range(a.runs):
            th.append(timed(hip))
            if not a.no_eager:
                te.append(timed(eager))
        row = dict(shape=name, B=len(lens), samples=max(lens), frames=frames(cfg, max(lens)), hip=stats(th))
        line = f"{name:13s} hip {row['hip']['median_ms']:8.3f} ms [{row['hip']['min_ms']:.3f}, {row['hip']['max_ms']:.3f}]"
        if te:
            row["eager"] = stats(te)
            row["speedup"] = round(statistics.median(te) / statistics.median(th), 2)
            diff = float((hip() - eager()).abs().max())
            row["max_abs_diff"] = diff
            line += (f"  eager {row['eager']['median_ms']:8.3f} ms [{row['eager']['min_ms']:.3f}, {row['eager']['max_ms']:.3f}]  x{row['speedup']:.2f}"
                     f"  max |hip - eager| {diff:.2e}")
        print(line, flush=True)
        rows.append(row)
    print(json.dumps({"bench": "hubert_base", "runs": a.runs, "warmup": a.warmup, "rows": rows}))


if __name__ == "__main__":
    main()
