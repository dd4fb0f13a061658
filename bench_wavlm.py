#!/usr/bin/env python3
"""WavLM-large encoder benchmark: the HIP library against the eager torch restatement (tools/wavlm_torch.py, fp32) on the same GPU.

    python bench_wavlm.py [--runs 10] [--warmup 3] [--only NAME] [--no-eager] [--json PATH]

Shapes: B = 1 x 10 s, B = 1 x 3 s and B = 8 x 2 s ragged (lengths from 0.6 s to 2 s), seeded large-size weights drawn on the device, all 24
layers and every hidden state; and `spk_B1x3s`, the whole wav -> WavLM -> ECAPA-TDNN -> spk_emb chain at B = 1 x 3 s (the eager leg is the
WavLM restatement followed by tools/speaker_encoder_torch.py).  The two legs run interleaved, run by run, each timed with device events
after the warm-up; median [min, max] of both are printed, then one JSON line (also written to --json).  --only / --no-eager serve a kernel
trace of one shape.
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
from speaker_encoder_torch import ecapa_forward  # noqa: E402
from wavlm_torch import frames, large_config, synthetic_wavlm_state_dict, wavlm_forward_torch  # noqa: E402

from unitspeech_amd.speaker_encoder import ECAPA_TDNN_SMALL, synthetic_ecapa_state_dict  # noqa: E402
from unitspeech_amd.wavlm import WavLMModel  # noqa: E402

SHAPES = {
    "B1x10s": [160000],
    "B1x3s": [48000],
    "B8x2s_ragged": [32000, 9600, 20800, 31999, 16000, 27000, 12345, 24000],
    "spk_B1x3s": [48000],
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
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = large_config()
    sd_dev = synthetic_wavlm_state_dict(cfg, 0, device=dev)
    model = WavLMModel.large()
    model.load_state_dict(sd_dev, assign=True)
    model = model.eval()
    spk = ECAPA_TDNN_SMALL(feat_dim=1024, emb_dim=256, feat_type="wavlm_large")
    spk_cfg = spk.config()
    ssd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(spk_cfg, 0).items()}
    spk.load_state_dict(ssd)
    spk = spk.eval().attach_upstream(model, normalize=True).to(dev)
    ssd_dev = {k: v.to(dev) for k, v in ssd.items()}
    rows = []
    for name, lens in SHAPES.items():
        if a.only and name != a.only:
            continue
        g = torch.Generator().manual_seed(len(lens))
        wav = (0.3 * torch.randn(len(lens), max(lens), generator=g)).to(dev)
        lengths = lens if len(lens) > 1 else None
        chain = name.startswith("spk_")

        def hip():
            return spk(wav) if chain else model(wav, lengths, output_hidden_states=True)[0]

        def eager():
            hs = wavlm_forward_torch(sd_dev, cfg, wav, lengths, torch.float32, normalize=chain)
            return ecapa_forward(spk_cfg, ssd_dev, torch.stack(hs), torch.float32) if chain else hs[-1]

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
    result = json.dumps({"bench": "wavlm_large", "runs": a.runs, "warmup": a.warmup, "rows": rows})
    print(result)
    if a.json:
        with open(a.json, "w") as f:
            f.write(result + "\n")


if __name__ == "__main__":
    main()
