#!/usr/bin/env python3
"""`train_STEP2.py`'s loop on the library: train a unit encoder against a frozen, pre-trained decoder.

    python train_unit_encoder.py --synthetic [--n_iters 20] [--batch_size 8] [--log_dir DIR]
    python train_unit_encoder.py --decoder_checkpoint ckpt.pt [--unit_encoder_checkpoint ue.pt] --synthetic_data ...

Each iteration is `compute_train_step_loss` (train_STEP2.py:238-305): the HIP `Encoder(trainable=True)` on the units, the
duration path, a random 176-frame window (fix_len_compatibility(2 * 22050 // 256)), the frozen HIP decoder's diffusion loss and
the prior loss; then (prior + diffusion).backward() and FusedAdam(lr=1e-4).step(max_norm=5) on the encoder's parameters.
--synthetic gives seeded decoder and encoder weights and a seeded batch (B utterances of varied lengths: units, durations, mel,
speaker embeddings); --decoder_checkpoint / --unit_encoder_checkpoint start from files.  The encoder is saved as
{"model": state_dict} (train_STEP2.py:233-236).  Losses are printed per iteration as the reference logs them.
"""
from __future__ import annotations

import argparse
import os
import random

import numpy as np
import torch

from unitspeech_amd import DecoderConfig, FusedAdam, UnitSpeech, synthetic_state_dict
from unitspeech_amd.encoder import Encoder, EncoderConfig, synthetic_encoder_state_dict
from unitspeech_amd.unit_encoder_train import compute_train_step_loss
from unitspeech_amd.util import fix_len_compatibility


def synthetic_batch(B, n_feats, spk_dim, n_units, seed):
    """B utterances of 40-120 units, 1-4 frames per unit (0 on padding), a mel of sum(durations) frames, unit-norm speaker
    embeddings.  The mel is a smooth function of the units, so the prior loss has something to learn."""
    g = np.random.Generator(np.random.Philox(key=seed))
    units = g.integers(40, 121, size=B)
    L = int(units.max())
    x = g.integers(0, n_units, size=(B, L)).astype(np.int64)
    dur = g.integers(1, 5, size=(B, L)).astype(np.float32)
    for b, n in enumerate(units):
        dur[b, n:] = 0
    ylen = dur.sum(1).astype(np.int64)
    table = g.standard_normal((n_units, n_feats), dtype=np.float32)
    y = np.zeros((B, n_feats, int(ylen.max())), dtype=np.float32)
    for b in range(B):
        frames = np.repeat(x[b, :units[b]], dur[b, :units[b]].astype(np.int64))
        y[b, :, :len(frames)] = table[frames].T
    spk = g.standard_normal((B, 1, spk_dim), dtype=np.float32)
    spk /= np.linalg.norm(spk, axis=-1, keepdims=True)
    t = lambda a: torch.from_numpy(a).cuda()
    return t(x), t(units.astype(np.int64)), t(dur), t(y), t(ylen), t(spk)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--synthetic", action="store_true", help="seeded decoder / encoder weights (unless checkpoints are given) and batch")
    ap.add_argument("--decoder_checkpoint", default=None, help="pre-trained decoder ({'model': state_dict} or a bare state_dict)")
    ap.add_argument("--unit_encoder_checkpoint", default=None, help="unit encoder to continue from ({'model': state_dict})")
    ap.add_argument("--n_iters", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--n_units", type=int, default=1000)
    ap.add_argument("--decoder_dim", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_dir", default=None, help="save unit_encoder.pt here after the last iteration")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("only --synthetic data is built (the reference's filelists are not read); give --synthetic")
    torch.manual_seed(args.seed)
    random.seed(args.seed)
    dev = torch.device("cuda")
    dc = DecoderConfig(dim=args.decoder_dim)
    decoder = UnitSpeech(dc.n_feats, dc.dim, list(dc.dim_mults), dc.beta_min, dc.beta_max, dc.pe_scale, dc.spk_emb_dim)
    if args.decoder_checkpoint:
        sd = torch.load(args.decoder_checkpoint, map_location="cpu")
        decoder.load_state_dict(sd.get("model", sd))
    else:
        decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(dc, 0).items()})
    decoder = decoder.to(dev).eval()
    decoder.requires_grad_(False)                                      # frozen, train_STEP2.py
    ec = EncoderConfig(n_vocab=args.n_units, n_feats=dc.n_feats)
    enc = Encoder(ec.n_vocab, ec.n_feats, ec.n_channels, ec.filter_channels, ec.n_heads, ec.n_layers, ec.kernel_size, 0.1,
                  window_size=ec.window_size, trainable=True)
    if args.unit_encoder_checkpoint:
        enc.load_state_dict(torch.load(args.unit_encoder_checkpoint, map_location="cpu")["model"])
    else:
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(ec, args.seed).items()})
    enc = enc.to(dev).train()
    opt = FusedAdam(enc.parameters(), lr=args.learning_rate)
    out_size = fix_len_compatibility(2 * 22050 // 256, len(dc.dim_mults) - 1)
    batch = synthetic_batch(args.batch_size, dc.n_feats, dc.spk_emb_dim, args.n_units, args.seed + 1)
    for it in range(args.n_iters):
        x, xl, dur, y, yl, spk = batch
        enc.zero_grad(set_to_none=True)
        prior, diff = compute_train_step_loss(enc, decoder, x, xl, dur, y, yl, spk, out_size)
        (prior + diff).backward()
        opt.step(max_norm=5)
        print(f"iter {it}: prior_loss {prior.item():.6f} diffusion_loss {diff.item():.6f}", flush=True)
    if args.log_dir:
        os.makedirs(args.log_dir, exist_ok=True)
        torch.save({"model": enc.state_dict()}, os.path.join(args.log_dir, "unit_encoder.pt"))


if __name__ == "__main__":
    main()
