#!/usr/bin/env python3
"""Voice-conversion benchmark: per-stage device times of `wav -> Resample -> HubertModel (ContentVec) -> ContentVec encoder ->
us_vc_align -> reverse diffusion (50 steps) -> BigVGAN` on the HIP library, and the two new stages (encoder + align) against the eager
torch restatement (tools/encoder_torch.py in fp32, F.interpolate per item) on the same GPU.

    python bench_voice_conversion.py [--runs 5] [--warmup 2] [--steps 50] [--only NAME] [--no-eager]

Shapes: B = 1 x 10 s, and B = 8 ragged from 2 to 10 s (22050 Hz sources).  Seeded weights of every module at the sizes of
checkpoints/voice-conversion.json (HuBERT-base, 768 -> 192 encoder, the full decoder, the base BigVGAN).  Every stage is warmed up on the
shape it is timed on, then timed with device events; the HIP and eager legs of encoder + align run interleaved, run by run.  Median
[min, max] are printed, then one JSON line, which is also written to profiles/bench_voice_conversion.json.
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
import encoder_torch as ET  # noqa: E402
from voice_conversion import SAMPLING_RATE, VC_ENCODER, build_synthetic  # noqa: E402

from unitspeech_amd.encoder import EncoderConfig, synthetic_encoder_state_dict  # noqa: E402
from unitspeech_amd.mel import synthetic_waveform  # noqa: E402
from unitspeech_amd.unitspeech import vc_align  # noqa: E402
from unitspeech_amd.util import fix_len_compatibility  # noqa: E402

SHAPES = {
    "B1x10s": [10.0],
    "B8_ragged_2to10s": [10.0, 2.0, 7.3, 4.1, 8.8, 3.2, 5.9, 6.6],
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def measure(fns, warmup, runs):
    """fns: name -> callable; run interleaved, run by run -> (name -> times, name -> last result)."""
    out = {}
    for _ in range(warmup):
        for n, f in fns.items():
            out[n] = f()
    ts = {n: [] for n in fns}
    for _ in range(runs):
        for n, f in fns.items():
            t, out[n] = timed(f)
            ts[n].append(t)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_voice_conversion.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pipe = build_synthetic(dev, 0)
    e = VC_ENCODER
    ecfg = EncoderConfig(150, 80, e["n_channels"], e["filter_channels"], e["n_heads"], e["n_layers"], e["kernel_size"], e["window_size"],
                         e["n_contentvec"])
    sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_encoder_state_dict(ecfg, 0).items()}
    r16 = pipe.resampler(SAMPLING_RATE, 16000)
    rows = []
    for name, seconds in SHAPES.items():
        if a.only and name != a.only:
            continue
        lens = [int(s * SAMPLING_RATE) for s in seconds]
        B = len(lens)
        wav = torch.zeros(B, max(lens))
        for b, n in enumerate(lens):
            wav[b, :n] = torch.from_numpy(synthetic_waveform(n, b, SAMPLING_RATE))
        wav = wav.to(dev)
        mel_lengths = [n // pipe.hop for n in lens]
        lens16 = [r16.out_length(n) for n in lens]
        cv = [pipe.contentvec.frames(n) for n in lens16]
        cv_dev = torch.tensor(cv, dtype=torch.long, device=dev)
        Tp = fix_len_compatibility(max(mel_lengths), pipe.n_down)
        spk = pipe.spk_emb.expand(B, -1, -1).contiguous()
        row = dict(shape=name, B=B, samples=lens, contentvec_frames=cv, mel_frames=mel_lengths, steps=a.steps, stages={})

        def stage(label, fn):
            ts, out = measure({label: fn}, a.warmup, a.runs)
            row["stages"][label] = stats(ts[label])
            s = row["stages"][label]
            print(f"{name:17s} {label:10s} {s['median_ms']:10.3f} ms [{s['min_ms']:.3f}, {s['max_ms']:.3f}]", flush=True)
            return out[label]

        wav16 = stage("resample", lambda: r16(wav, lens))
        feats = stage("contentvec", lambda: pipe.contentvec(wav16, lens16))
        cond_x = stage("encoder", lambda: pipe.encoder(feats, cv_dev)[0])
        cond_y, y_mask, _ = stage("align", lambda: vc_align(cond_x, cv, mel_lengths, Tp))
        z = torch.randn_like(cond_y)
        mel = stage("sampler", lambda: pipe.decoder.forward(z, y_mask, cond_y, spk, n_timesteps=a.steps, text_gradient_scale=1.0,
                                                            spk_gradient_scale=1.0, mel_range=pipe.mel_range, rng="philox", seed=1))
        stage("vocoder", lambda: pipe.vocoder.forward(mel[:, :, :max(mel_lengths)], lengths=mel_lengths))
        row["total_median_ms"] = round(sum(s["median_ms"] for s in row["stages"].values()), 3)
        row["audio_seconds"] = round(sum(mel_lengths) * pipe.hop / SAMPLING_RATE, 2)

        if not a.no_eager:
            def hip():
                cx = pipe.encoder(feats, cv_dev)[0]
                return vc_align(cx, cv, mel_lengths, Tp)[0]

            def eager():
                cx = ET.encoder_forward(sd_dev, ecfg.n_heads, feats, cv_dev)[0]
                out = torch.zeros(B, cx.shape[1], Tp, device=dev)
                for b in range(B):
                    out[b, :, :mel_lengths[b]] = torch.nn.functional.interpolate(cx[b:b + 1, :, :cv[b]], size=mel_lengths[b], mode="linear")[0]
                return out

            ts, out = measure({"hip": hip, "eager": eager}, a.warmup, a.runs)
            row["encoder_align"] = dict(hip=stats(ts["hip"]), eager=stats(ts["eager"]),
                                        speedup=round(statistics.median(ts["eager"]) / statistics.median(ts["hip"]), 2),
                                        max_abs_diff=float((out["hip"] - out["eager"]).abs().max()))
            ea = row["encoder_align"]
            print(f"{name:17s} encoder+align hip {ea['hip']['median_ms']:.3f} ms  eager {ea['eager']['median_ms']:.3f} ms  x{ea['speedup']:.2f}  "
                  f"max |hip - eager| {ea['max_abs_diff']:.2e}", flush=True)
        rows.append(row)
    result = {"bench": "voice_conversion", "runs": a.runs, "warmup": a.warmup, "rows": rows}
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
