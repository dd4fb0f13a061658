#!/usr/bin/env python3
"""STEP1 (text-to-speech pre-training) step benchmark.

    python bench_tts_step.py [--runs 10] [--warmup 3] [--quick]

(a) DurationPredictor(trainable=True) forward + backward at the reference size (192 + 256 input channels, 256 filter channels, k = 3,
    p_dropout 0.1) at B = 32, L in {128, 400}, against the eager restatement (tools/duration_torch.py, fp32, the same dropout masks as
    inputs) on the same GPU, interleaved run by run, each run timed with device events after warm-up; median and min / max reported.
(b) One full STEP1 iteration (train_tts.py: three modules, three losses, backward, clip + Adam over three groups) at B = 32,
    out_size 176, ragged text lengths up to about 300 symbols and mels up to about 900 frames; and its per-stage split, measured
    stage by stage with device events in a second pass (encoder forward, predictor forward, alignment, decoder loss, backward,
    optimiser).
--quick shrinks (a) to B = 4, L = 64 and (b) to B = 2 with a dim-16 decoder.  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from duration_torch import duration_forward  # noqa: E402

from train_tts import build_modules, synthetic_batch  # noqa: E402
from unitspeech_amd import DecoderConfig, FusedAdam  # noqa: E402
from unitspeech_amd.encoder import DurationPredictorConfig, EncoderConfig  # noqa: E402
from unitspeech_amd.tts_train import align, compute_train_step_loss, duration_loss  # noqa: E402
from unitspeech_amd.unit_encoder_train import align_segment, prior_loss  # noqa: E402
from unitspeech_amd.util import fix_len_compatibility  # noqa: E402

P = 0.1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def predictor_rows(dp, pc, shapes, runs, warmup):
    dev = torch.device("cuda")
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in dp.state_dict().items()}
    rows = []
    for B, L in shapes:
        g = torch.Generator().manual_seed(B * 7 + L)
        x = torch.randn(B, pc.in_channels, L, generator=g).to(dev)
        spk = torch.randn(B, 1, pc.spk_emb_dim, generator=g).to(dev)
        mask = torch.ones(B, 1, L, device=dev)
        gl = torch.randn(B, 1, L, generator=g).to(dev)
        masks = {s: (torch.rand(B, pc.filter_channels, L, device=dev) >= P).float() / (1 - P) for s in (0, 1)}

        def hip():
            (dp(x, mask, g=spk, reverse=True) * gl).sum().backward()

        def eager():
            (duration_forward(sd, x, mask, spk, masks) * gl).sum().backward()

        for _ in range(warmup):
            hip()
            eager()
        th, te = [], []
        for _ in range(runs):
            dp.zero_grad(set_to_none=True)
            for t in sd.values():
                t.grad = None
            th.append(timed(hip))
            te.append(timed(eager))
        row = dict(B=B, L=L, hip=stats(th), eager=stats(te), speedup=round(statistics.median(te) / statistics.median(th), 2))
        print(f"predictor B={B:3d} L={L:4d}  hip {row['hip']['median_ms']:7.3f} ms [{row['hip']['min_ms']:.3f}, {row['hip']['max_ms']:.3f}]  "
              f"eager {row['eager']['median_ms']:7.3f} ms [{row['eager']['min_ms']:.3f}, {row['eager']['max_ms']:.3f}]  x{row['speedup']:.2f}",
              flush=True)
        rows.append(row)
    return rows


def step1(enc, dp, dec, dc, ec, B, symbols, runs, warmup):
    opt = FusedAdam([{"params": list(enc.parameters()), "max_norm": 5.0}, {"params": list(dp.parameters()), "max_norm": 5.0},
                     {"params": list(dec.parameters()), "max_norm": 2.0}], lr=1e-4)
    out_size = fix_len_compatibility(2 * 22050 // 256, len(dc.dim_mults) - 1)
    x, xl, y, yl, spk = synthetic_batch(B, dc.n_feats, dc.spk_emb_dim, ec.n_vocab, 1, symbols=symbols)

    def it():
        for m in (enc, dp, dec):
            m.zero_grad(set_to_none=True)
        dur, prior, diff = compute_train_step_loss(enc, dp, dec, x, xl, y, yl, spk, out_size)
        (dur + prior + diff).backward()
        opt.step()

    for _ in range(warmup):
        it()
    total = stats([timed(it) for _ in range(runs)])
    # the same statements, stage by stage
    split = {k: [] for k in ("encoder_fwd", "predictor_fwd", "alignment", "decoder_loss", "backward", "optimiser")}
    for _ in range(runs):
        for m in (enc, dp, dec):
            m.zero_grad(set_to_none=True)
        box = {}
        split["encoder_fwd"].append(timed(lambda: box.update(e=enc(x, xl))))
        mu_x, h, x_mask = box["e"]
        split["predictor_fwd"].append(timed(lambda: box.update(logw=dp(h.detach(), x_mask, g=spk, reverse=True))))
        y_mask = (torch.arange(y.shape[-1], device=y.device)[None] < yl[:, None]).unsqueeze(1).float()

        def ali():
            attn, d = align(mu_x, y, x_mask, y_mask, xl, yl)
            box.update(attn=attn, dur=duration_loss(box["logw"], d, x_mask, xl))
        split["alignment"].append(timed(ali))

        def decl():
            y_seg, seg_mask, mu_y = align_segment(mu_x, y, yl, box["attn"], out_size)
            diff, _ = dec.compute_loss(y_seg, seg_mask, mu_y, spk_emb=spk)
            box.update(loss=box["dur"] + prior_loss(y_seg, mu_y, seg_mask) + diff)
        split["decoder_loss"].append(timed(decl))
        split["backward"].append(timed(lambda: box["loss"].backward()))
        split["optimiser"].append(timed(lambda: opt.step()))
    return dict(B=B, out_size=out_size, max_symbols=int(xl.max()), max_frames=int(yl.max()), **total,
                stages_ms={k: round(statistics.median(v), 3) for k, v in split.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    random.seed(0)
    dc = DecoderConfig(dim=16) if a.quick else DecoderConfig()
    ec = EncoderConfig(n_feats=dc.n_feats)
    pc = DurationPredictorConfig(in_channels=ec.n_channels, spk_emb_dim=dc.spk_emb_dim)
    enc, dp, dec = build_modules(ec, pc, dc, 0, P)
    enc, dp, dec = enc.cuda().train(), dp.cuda().train(), dec.cuda().train()
    runs, warmup = (3, 1) if a.quick else (a.runs, a.warmup)
    rows = predictor_rows(dp, pc, [(4, 64)] if a.quick else [(32, 128), (32, 400)], runs, warmup)
    s1 = step1(enc, dp, dec, dc, ec, 2 if a.quick else 32, (90, 121) if a.quick else (150, 301), runs, warmup)
    print(f"STEP1 iteration B={s1['B']}: {s1['median_ms']:.2f} ms [{s1['min_ms']:.2f}, {s1['max_ms']:.2f}]  stages {s1['stages_ms']}", flush=True)
    print(json.dumps({"bench": "tts_step1", "config": "quick" if a.quick else "reference", "p_dropout": P, "predictor": rows, "step1": s1}))


if __name__ == "__main__":
    main()
