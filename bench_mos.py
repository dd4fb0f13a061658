#!/usr/bin/env python3
"""MOS predictor benchmark at the base size: 13 hidden states of width 768, a connector of 256, seeded weights.

    python bench_mos.py [--runs 10] [--warmup 3] [--quick] [--head_only] [--json PATH]

  head        `us_mos_score` (MOSHead.forward: two launches) on resident hidden states [B, 13, F, 768] at B = 1 x 10 s (F = 499) and at
              B = 8 ragged, 2 to 10 s, timed with device events over 100 back-to-back calls.  Beside it, on the same GPU: the eager fp32 head (the list of hidden
              states stacked, the weighted sum, the connector, masked attention pooling, the linear), and a plain device copy of as many
              bytes as the kernel reads (the valid frames of every state), which is what one read of the hidden states costs with a write
              added.  The eager leg's launches are counted once, outside the timed runs, with torch's profiler.
  wav->score  `MOSPredictor` (encoder with every hidden state, then the head) at the same shapes, beside the encoder alone, whose
              difference is the share of the call spent outside the encoder, and the eager restatement (tools/hubert_torch.py in fp32
              and the eager head).
The legs run interleaved, run by run, after the warm-up; median [min, max].  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hubert_torch import base_config, frames, hubert_forward_torch, synthetic_hubert_state_dict  # noqa: E402
from mos_torch import ATT, MEAN, synthetic_mos_weights  # noqa: E402

from unitspeech_amd.hubert import HubertModel  # noqa: E402
from unitspeech_amd.mos import MOSHead, MOSPredictor  # noqa: E402

P = 256
SHAPES = {
    "B1x10s": [160000],
    "B8x2-10s_ragged": [160000, 32000, 96000, 143999, 64000, 120000, 48123, 80000],
}
QUICK = {"B1x1s": [16000], "B3x1s_ragged": [16000, 4000, 9999]}
HIP_LAUNCHES = 2                 # mos_frame_kernel, mos_pool_kernel
HEAD_REPS = 100                  # calls per timed window of the head legs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def eager_head(states, fr, w):
    """states: the list of n tensors [B, F, H] as an encoder hands them over; fr [B] frames per item -> scores [B], in fp32 torch ops"""
    hs = torch.stack(states, 0)
    s = torch.softmax(w["featurizer.weights"], -1)
    x = (s.view(-1, 1, 1, 1) * hs).sum(0)
    z = F.linear(x, w["connector.weight"], w["connector.bias"])
    live = torch.arange(z.shape[1], device=z.device)[None, :] < fr[:, None]
    e = F.linear(z, w[ATT + "weight"], w[ATT + "bias"])[..., 0].masked_fill(~live, float("-inf"))
    u = (torch.softmax(e, -1)[..., None] * z.masked_fill(~live[..., None], 0.0)).sum(1)
    return F.linear(u, w[MEAN + "weight"], w[MEAN + "bias"])[:, 0]


def count_launches(fn):
    """Device kernels of one call, from torch's profiler; None where it cannot be had."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def run_legs(legs, reps, runs, warmup):
    """legs[k] is called reps.get(k, 1) times inside one timed window (a head call is tens of microseconds: one call alone would time the
    events); the figure kept is the window over the calls."""
    def window(k):
        for _ in range(reps.get(k, 1)):
            legs[k]()

    for _ in range(warmup):
        for k in legs:
            window(k)
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k in legs:
            ts[k].append(timed(lambda: window(k)) / reps.get(k, 1))
    return ts


def case(name, lens, predictor, sd_dev, cfg, w_dev, runs, warmup, dev, head_only):
    g = torch.Generator().manual_seed(len(lens))
    wav = (0.3 * torch.randn(len(lens), max(lens), generator=g)).to(dev)
    lengths = lens if len(lens) > 1 else None
    nfr = [frames(cfg, n) for n in lens]
    fr = torch.tensor(nfr, dtype=torch.int64, device=dev)
    _, hs = predictor.upstream(wav, lengths, output_hidden_states=True)          # [B, 13, F, 768], resident
    states = [hs[:, l].contiguous() for l in range(hs.shape[1])]
    n, H = hs.shape[1], hs.shape[3]
    read_bytes = 4 * n * H * sum(nfr)
    src = torch.empty(read_bytes // 4, device=dev).normal_()
    dst = torch.empty_like(src)
    box = {}

    def hip_head():
        box["hip"] = predictor.head(hs, fr)

    def eager_head_leg():
        box["eager"] = eager_head(states, fr, w_dev)

    def copy():
        dst.copy_(src)

    legs = dict(hip_head=hip_head, eager_head=eager_head_leg, copy=copy)
    if not head_only:
        def hip():
            box["hip_e2e"] = predictor(wav, lengths)

        def encoder():
            predictor.upstream(wav, lengths, output_hidden_states=True)

        def eager():
            box["eager_e2e"] = eager_head(hubert_forward_torch(sd_dev, cfg, wav, lengths, torch.float32), fr, w_dev)

        legs.update(hip=hip, encoder=encoder, eager=eager)
    ts = run_legs(legs, dict(hip_head=HEAD_REPS, eager_head=HEAD_REPS, copy=HEAD_REPS), runs, warmup)
    med = {k: statistics.median(v) for k, v in ts.items()}
    row = dict(shape=name, B=len(lens), frames=max(nfr), valid_frames=sum(nfr), read_mbytes=round(read_bytes / 1e6, 3),
               **{k: stats(v) for k, v in ts.items()})
    row["head_speedup_vs_eager"] = round(med["eager_head"] / med["hip_head"], 2)
    row["head_read_gbytes_per_s"] = round(read_bytes / (med["hip_head"] * 1e-3) / 1e9, 1)
    row["copy_gbytes_per_s_read_plus_write"] = round(2 * read_bytes / (med["copy"] * 1e-3) / 1e9, 1)
    row["head_time_over_copy_time"] = round(med["hip_head"] / med["copy"], 2)
    row["launches"] = dict(hip_head=HIP_LAUNCHES, eager_head=None)
    count = lambda: count_launches(eager_head_leg)  # noqa: E731
    row["head_max_diff_vs_eager"] = float((box["hip"] - box["eager"]).abs().max())
    print(f"{name:16s} head {med['hip_head']:8.4f} ms ({row['head_read_gbytes_per_s']:.0f} GB/s read)   eager head {med['eager_head']:8.4f} ms "
          f"x{row['head_speedup_vs_eager']:.2f}   copy of the same bytes {med['copy']:.4f} ms   "
          f"max |diff| {row['head_max_diff_vs_eager']:.2e}", flush=True)
    if not head_only:
        row["outside_encoder_share"] = round((med["hip"] - med["encoder"]) / med["hip"], 4)
        row["head_share_of_encoder_plus_head"] = round(med["hip_head"] / (med["encoder"] + med["hip_head"]), 4)
        row["speedup_vs_eager"] = round(med["eager"] / med["hip"], 2)
        row["max_diff_vs_eager"] = float((box["hip_e2e"] - box["eager_e2e"]).abs().max())
        print(f"{'':16s} wav->score {med['hip']:8.3f} ms  (encoder alone {med['encoder']:.3f} ms; outside the encoder "
              f"{100 * row['outside_encoder_share']:.2f} %; head / (encoder + head) {100 * row['head_share_of_encoder_plus_head']:.2f} %)   "
              f"eager {med['eager']:8.3f} ms  x{row['speedup_vs_eager']:.2f}   max |diff| {row['max_diff_vs_eager']:.2e}", flush=True)
    return row, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes: a functional check, not a measurement")
    ap.add_argument("--head_only", action="store_true", help="leave out the wav -> score legs (the run a kernel trace is taken of)")
    ap.add_argument("--json", type=str, default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the MOS predictor has no CPU fallback")
    dev = torch.device("cuda", 0)
    cfg = base_config()
    sd = synthetic_hubert_state_dict(cfg, 0)
    n = cfg["num_hidden_layers"] + 1
    w = synthetic_mos_weights(n, cfg["hidden_size"], P, seed=0)
    upstream = HubertModel.base()
    upstream.load_state_dict(sd)
    head = MOSHead(cfg["hidden_size"], n, P)
    head.load_state_dict(w)
    predictor = MOSPredictor(upstream, head).to(dev).eval()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    w_dev = {k: v.to(dev) for k, v in w.items()}
    runs = max(a.runs, 1)
    cases = [case(name, lens, predictor, sd_dev, cfg, w_dev, runs, a.warmup, dev, a.head_only) for name, lens in (QUICK if a.quick else SHAPES).items()]
    rows = [row for row, _ in cases]
    if not a.head_only:                  # after every timed run: the profiler slows the host
        for row, count in cases:
            row["launches"]["eager_head"] = count()
            print(f"{row['shape']:16s} launches per head call: {HIP_LAUNCHES} against eager's {row['launches']['eager_head']}", flush=True)
    out = {"bench": "mos_wav2vec2_base", "n_states": n, "H": cfg["hidden_size"], "P": P, "runs": a.runs, "warmup": a.warmup, "quick": a.quick,
           "head_only": a.head_only, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
