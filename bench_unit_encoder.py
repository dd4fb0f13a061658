#!/usr/bin/env python3
"""Encoder training step throughput: forward + backward of unitspeech_amd.encoder.Encoder(trainable=True) against eager PyTorch on
the same GPU.

    python bench_unit_encoder.py [--batches 1,32] [--lengths 128,400] [--runs 10] [--warmup 3]

At the reference size (192 channels, 768 filter channels, 6 layers, 2 heads, W = 4, 1000 units, p_dropout 0.1) and for every
(B, L): all items full length, both paths run forward + backward of sum(mu_x * g_mu) + sum(x * g_x) on the same seeded weights,
interleaved run by run, each run timed with device events after warm-up; the median is reported.  The eager leg is
tools/encoder_torch.py in fp32 with the same dropout masks as inputs.  Per row: milliseconds, speed-up, the convolutions'
algorithmic FLOPs (forward, data and weight gradients: 3x the forward) and their share of the fp32 matrix-core peak if the whole
step were convolution time (a lower bound on the convolutions' own share).  Then one full STEP2 iteration at B = --step2_batch
(train_unit_encoder.py's synthetic batch, full-size frozen decoder, 176-frame crop, prior + diffusion backward, FusedAdam step).
The last line is one JSON object.
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
from encoder_torch import encoder_forward  # noqa: E402

from unitspeech_amd.encoder import Encoder, EncoderConfig, synthetic_encoder_state_dict  # noqa: E402

FP32_MFMA_PEAK = 157.3e12           # MI355X, v_mfma_f32_32x32x2_f32
CFG = EncoderConfig(n_vocab=1000)
P = 0.1


def conv_flops(cfg, rows):
    c, f, k = cfg.n_channels, cfg.filter_channels, cfg.kernel_size
    per_row = 3 * c * c * 5 + c * c + cfg.n_layers * (4 * c * c + 2 * c * f * k) + cfg.n_feats * c
    return 3 * 2 * per_row * rows


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--lengths", default="128,400")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step2_batch", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda")
    enc = Encoder(CFG.n_vocab, CFG.n_feats, CFG.n_channels, CFG.filter_channels, CFG.n_heads, CFG.n_layers, CFG.kernel_size, P,
                  window_size=CFG.window_size, trainable=True)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(CFG, 0).items()})
    enc = enc.to(dev).train()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    rows = []
    for B in [int(v) for v in a.batches.split(",")]:
        for L in [int(v) for v in a.lengths.split(",")]:
            g = torch.Generator().manual_seed(B * 7 + L)
            ids = torch.randint(0, CFG.n_vocab, (B, L), generator=g).to(dev)
            lens = torch.full((B,), L, dtype=torch.int64, device=dev)
            g_mu = torch.randn(B, CFG.n_feats, L, generator=g).to(dev)
            g_x = torch.randn(B, CFG.n_channels, L, generator=g).to(dev)
            masks = {}
            for site in range(3 + 4 * CFG.n_layers):
                w, p = (site - 3) % 4, (0.5 if site < 3 else P)
                shape = (B, CFG.n_heads, L, L) if site >= 3 and w == 0 else \
                    (B, CFG.filter_channels if site >= 3 and w == 2 else CFG.n_channels, L)
                masks[site] = (torch.rand(shape, device=dev) >= p).float() / (1 - p)

            def hip():
                mu, x, _ = enc(ids, lens)
                ((mu * g_mu).sum() + (x * g_x).sum()).backward()

            def eager():
                mu, x, _ = encoder_forward(sd, CFG.n_heads, ids, lens, masks)
                ((mu * g_mu).sum() + (x * g_x).sum()).backward()

            for _ in range(a.warmup):
                hip()
                eager()
            th, te = [], []
            for _ in range(a.runs):
                enc.zero_grad(set_to_none=True)
                for t in sd.values():
                    t.grad = None
                th.append(timed(hip))
                te.append(timed(eager))
            mh, me = statistics.median(th), statistics.median(te)
            fl = conv_flops(CFG, B * L)
            row = dict(B=B, L=L, hip_ms=round(mh * 1e3, 3), eager_ms=round(me * 1e3, 3), speedup=round(me / mh, 2),
                       conv_gflop=round(fl / 1e9, 2), conv_share_of_fp32_mfma_peak_lower_bound=round(fl / mh / FP32_MFMA_PEAK, 4))
            print(f"B={B:3d} L={L:4d}  hip {row['hip_ms']:8.2f} ms  eager {row['eager_ms']:8.2f} ms  x{row['speedup']:5.2f}  "
                  f"conv {row['conv_gflop']:7.1f} GFLOP  >= {100 * row['conv_share_of_fp32_mfma_peak_lower_bound']:.1f} % of fp32 MFMA peak",
                  flush=True)
            rows.append(row)
    step2 = step2_iteration(enc, a)
    print(f"STEP2 iteration B={a.step2_batch}: {step2['ms']:.2f} ms", flush=True)
    print(json.dumps({"bench": "unit_encoder_fwd_bwd", "config": "reference", "p_dropout": P, "rows": rows, "step2": step2}))


def step2_iteration(enc, a):
    from train_unit_encoder import synthetic_batch
    from unitspeech_amd import DecoderConfig, FusedAdam, UnitSpeech, synthetic_state_dict
    from unitspeech_amd.unit_encoder_train import compute_train_step_loss
    from unitspeech_amd.util import fix_len_compatibility
    dc = DecoderConfig()
    dec = UnitSpeech(dc.n_feats, dc.dim, list(dc.dim_mults), dc.beta_min, dc.beta_max, dc.pe_scale, dc.spk_emb_dim)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(dc, 0).items()})
    dec = dec.cuda().eval()
    dec.requires_grad_(False)
    opt = FusedAdam(enc.parameters(), lr=1e-4)
    out_size = fix_len_compatibility(2 * 22050 // 256, len(dc.dim_mults) - 1)
    x, xl, dur, y, yl, spk = synthetic_batch(a.step2_batch, dc.n_feats, dc.spk_emb_dim, CFG.n_vocab, 1)

    def it():
        enc.zero_grad(set_to_none=True)
        prior, diff = compute_train_step_loss(enc, dec, x, xl, dur, y, yl, spk, out_size)
        (prior + diff).backward()
        opt.step(max_norm=5)

    for _ in range(a.warmup):
        it()
    ts = [timed(it) for _ in range(a.runs)]
    return dict(B=a.step2_batch, out_size=out_size, ms=round(statistics.median(ts) * 1e3, 3))


if __name__ == "__main__":
    main()
