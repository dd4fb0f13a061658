#!/usr/bin/env python3
"""`train_STEP1.py`'s loop on the library: train the text encoder, the duration predictor and the decoder together.

    python train_tts.py --synthetic [--n_iters 20] [--batch_size 8] [--log_dir DIR]

Each iteration is `compute_train_step_loss` (train_STEP1.py:307-387): the HIP `Encoder(trainable=True)` on the phonemes, the HIP
`DurationPredictor(trainable=True)` on its detached output, monotonic alignment search on the device, the duration loss, a random
176-frame window (fix_len_compatibility(2 * 22050 // 256)), the decoder's diffusion loss and the prior loss; then
(dur + prior + diff).backward() and one FusedAdam(lr=1e-4) step over three parameter groups clipped at 5 / 5 / 2 (:243-249).
--synthetic gives seeded weights for the three modules and a seeded batch: phonemes with planted durations and a mel that is a
smooth function of the phonemes, so all three losses have something to learn.  The checkpoints start from files when given.  Reading
the reference's file lists (the data loader) is out of scope: only --synthetic data is built.  At the end text_encoder.pt and
duration_predictor.pt are saved as {"model": state_dict} and pretrained_decoder.pt in the trainer's layout (:289-304).
"""
from __future__ import annotations

import argparse
import os
import random

import numpy as np
import torch

from unitspeech_amd import DecoderConfig, FusedAdam, UnitSpeech, synthetic_state_dict
from unitspeech_amd.checkpoint import save_pretrained_checkpoint
from unitspeech_amd.encoder import (DurationPredictor, DurationPredictorConfig, Encoder, EncoderConfig,
                                    synthetic_duration_predictor_state_dict, synthetic_encoder_state_dict)
from unitspeech_amd.tts_train import compute_train_step_loss
from unitspeech_amd.util import fix_len_compatibility


def synthetic_batch(B, n_feats, spk_dim, n_vocab, seed, symbols=(40, 121)):
    """B utterances of symbols[0] .. symbols[1]-1 phonemes with planted durations of 1-4 frames; the mel repeats a smooth per-phoneme
    pattern (a random table, low-pass filtered along the mel axis) for the planted number of frames, plus a little noise."""
    g = np.random.Generator(np.random.Philox(key=seed))
    n = g.integers(symbols[0], symbols[1], size=B)
    L = int(n.max())
    x = g.integers(0, n_vocab, size=(B, L)).astype(np.int64)
    dur = g.integers(1, 5, size=(B, L))
    for b, k in enumerate(n):
        dur[b, k:] = 0
    ylen = dur.sum(1).astype(np.int64)
    table = g.standard_normal((n_vocab, n_feats), dtype=np.float32)
    table = (table + np.roll(table, 1, 1) + np.roll(table, -1, 1)) / 3
    y = np.zeros((B, n_feats, int(ylen.max())), dtype=np.float32)
    for b in range(B):
        frames = np.repeat(x[b, :n[b]], dur[b, :n[b]])
        y[b, :, :len(frames)] = table[frames].T + 0.05 * g.standard_normal((n_feats, len(frames)), dtype=np.float32)
    spk = g.standard_normal((B, 1, spk_dim), dtype=np.float32)
    spk /= np.linalg.norm(spk, axis=-1, keepdims=True)
    t = lambda a: torch.from_numpy(a).cuda()
    return t(x), t(n.astype(np.int64)), t(y), t(ylen), t(spk)


def build_modules(ec, pc, dc, seed=0, p_dropout=0.1):
    enc = Encoder(ec.n_vocab, ec.n_feats, ec.n_channels, ec.filter_channels, ec.n_heads, ec.n_layers, ec.kernel_size, p_dropout,
                  window_size=ec.window_size, trainable=True)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(ec, seed).items()})
    dp = DurationPredictor(pc.in_channels, pc.filter_channels, pc.kernel_size, p_dropout, spk_emb_dim=pc.spk_emb_dim, trainable=True)
    dp.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_duration_predictor_state_dict(pc, seed).items()})
    dec = UnitSpeech(dc.n_feats, dc.dim, list(dc.dim_mults), dc.beta_min, dc.beta_max, dc.pe_scale, dc.spk_emb_dim)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(dc, seed).items()})
    return enc, dp, dec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="Reading the reference's file lists is out of scope: only --synthetic data is built.")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights (unless checkpoints are given) and a seeded batch")
    ap.add_argument("--text_encoder_checkpoint", default=None, help="{'model': state_dict} to continue from")
    ap.add_argument("--duration_predictor_checkpoint", default=None, help="{'model': state_dict} to continue from")
    ap.add_argument("--decoder_checkpoint", default=None, help="{'model': state_dict} or a bare state_dict to continue from")
    ap.add_argument("--n_iters", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--decoder_dim", type=int, default=128)
    ap.add_argument("--with_uncond_score_estimator", action="store_true",
                    help="replace int(0.25 B) speaker embeddings per step by the unconditional one (train_STEP1.py:325-326)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_dir", default=None, help="save text_encoder.pt, duration_predictor.pt and pretrained_decoder.pt here")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("only --synthetic data is built (the reference's filelists are not read); give --synthetic")
    torch.manual_seed(args.seed)
    random.seed(args.seed)
    dev = torch.device("cuda")
    dc = DecoderConfig(dim=args.decoder_dim)
    ec = EncoderConfig(n_feats=dc.n_feats)
    pc = DurationPredictorConfig(in_channels=ec.n_channels, spk_emb_dim=dc.spk_emb_dim)
    enc, dp, dec = build_modules(ec, pc, dc, args.seed)
    if args.text_encoder_checkpoint:
        enc.load_state_dict(torch.load(args.text_encoder_checkpoint, map_location="cpu")["model"])
    if args.duration_predictor_checkpoint:
        dp.load_state_dict(torch.load(args.duration_predictor_checkpoint, map_location="cpu")["model"])
    if args.decoder_checkpoint:
        sd = torch.load(args.decoder_checkpoint, map_location="cpu")
        dec.load_state_dict(sd.get("model", sd))
    enc, dp, dec = enc.to(dev).train(), dp.to(dev).train(), dec.to(dev).train()
    # train_STEP1.py:243-249 (the non-fp16 branch): one Adam over the three modules, each clipped on its own norm
    opt = FusedAdam([{"params": list(enc.parameters()), "max_norm": 5.0}, {"params": list(dp.parameters()), "max_norm": 5.0},
                     {"params": list(dec.parameters()), "max_norm": 2.0}], lr=args.learning_rate)
    out_size = fix_len_compatibility(2 * 22050 // 256, len(dc.dim_mults) - 1)
    x, xl, y, yl, spk = synthetic_batch(args.batch_size, dc.n_feats, dc.spk_emb_dim, ec.n_vocab, args.seed + 1)
    spk_uncond = None
    if args.with_uncond_score_estimator:
        spk_uncond = dec.spk_uncon.detach().reshape(1, -1)
        spk_uncond = spk_uncond / spk_uncond.norm()                    # :158
    for it in range(args.n_iters):
        for m in (enc, dp, dec):
            m.zero_grad(set_to_none=True)
        dur, prior, diff = compute_train_step_loss(enc, dp, dec, x, xl, y, yl, spk, out_size, spk_uncond=spk_uncond)
        (dur + prior + diff).backward()
        opt.step()
        n = [float(opt.last_grad_norms[i]) for i in range(3)]
        print(f"iter {it}: dur_loss {dur.item():.6f} prior_loss {prior.item():.6f} diff_loss {diff.item():.6f} "
              f"grad_norm text_encoder {n[0]:.4f} duration_predictor {n[1]:.4f} decoder {n[2]:.4f}", flush=True)
    if args.log_dir:
        os.makedirs(args.log_dir, exist_ok=True)
        torch.save({"model": enc.state_dict()}, os.path.join(args.log_dir, "text_encoder.pt"))
        torch.save({"model": dp.state_dict()}, os.path.join(args.log_dir, "duration_predictor.pt"))
        speakers = torch.nn.Embedding(args.batch_size, dc.spk_emb_dim)
        speakers.weight.data.copy_(spk.reshape(args.batch_size, -1).cpu())
        save_pretrained_checkpoint(os.path.join(args.log_dir, "pretrained_decoder.pt"), dec, speakers, y.min().cpu(), y.max().cpu(),
                                   args.n_iters)


if __name__ == "__main__":
    main()
