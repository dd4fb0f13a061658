#!/usr/bin/env python3
"""Fitting a CTC head on a frozen HuBERT / ContentVec / wav2vec2 encoder on the HIP library: what a language without a ready-made
fine-tuned CTC checkpoint needs before `evaluate.py` can score it.

    python train_ctc_head.py --filelist LIST --vocab_path vocab.json --encoder_path ENCODER.pt [--config_path config.json]
                             [--epochs 10] [--batch 16] [--lr 1e-3] [--optimizer fused|torch] --out CTC.pt
    python train_ctc_head.py --synthetic 8 --epochs 30 --out CTC.pt

LIST holds one `wav|transcript` line per sample (evaluate.py's format; a third column is ignored).  ENCODER.pt is a `torch.save`d state
dict of the base-form encoder: `transformers.HubertModel` / `Wav2Vec2Model` keys, bare or under `hubert.` / `wav2vec2.` (a whole CTC
checkpoint is taken too: its head is then the starting point).  The transcripts are brought to the vocabulary by `normalize_text`.  The
encoder runs without gradients; `CTCHead(trainable=True)` is fitted with the library's CTC loss (`asr.ctc_loss`, mean reduction,
zero_infinity: a transcript too long for its audio is skipped, not poison) by `FusedAdam` or `torch.optim.Adam`.  After every epoch the
mean loss and the greedy CER over the training files are printed.  --out receives a state dict with `transformers`' keys that
`load_ctc_checkpoint` (and so evaluate.py --ctc_path) reads back.

--synthetic N needs no files: the seeded tiny encoder and the N seeded waveforms of `evaluate.py --synthetic`, with the greedy output of
a seeded teacher head as the transcripts; the head that is fitted starts from zero, so a correct loss and backward drive the loss down.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import evaluate  # noqa: E402
from unitspeech_amd.audio import read_wav, to_16k  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402


def encoder_state_dict(sd, prefix_out: str):
    """A checkpoint's encoder keys under `prefix_out.` whether they came bare or under either class's prefix."""
    out = {}
    for k, v in sd.items():
        if k.startswith("lm_head."):
            continue
        for p in ("hubert.", "wav2vec2."):
            if k.startswith(p):
                k = k[len(p):]
                break
        out[prefix_out + "." + k] = v
    return out


def build_model(args, vocabulary, device):
    from unitspeech_amd.asr import HubertForCTC, Wav2Vec2ForCTC
    sd = torch.load(args.encoder_path, map_location="cpu")
    if not isinstance(sd, dict):
        raise SystemExit(f"{args.encoder_path}: expected a state dict")
    config = {}
    if args.config_path:
        with open(args.config_path, encoding="utf-8") as f:
            config = {k: v for k, v in json.load(f).items() if k not in ("vocab_size", "pad_token_id")}
    cls = Wav2Vec2ForCTC if any(k.startswith("wav2vec2.") for k in sd) else HubertForCTC
    model = cls.base(vocab_size=len(vocabulary), pad_token_id=vocabulary.blank_id, trainable=True, **config)
    weights = encoder_state_dict(sd, cls._prefix)
    head = model.lm_head.state_dict()
    if "lm_head.weight" in sd and tuple(sd["lm_head.weight"].shape) == tuple(head["weight"].shape):
        head = {"weight": sd["lm_head.weight"], "bias": sd.get("lm_head.bias", head["bias"])}
    weights.update({"lm_head." + k: v for k, v in head.items()})
    model.load_state_dict(weights)
    return model.to(device).eval()


def synthetic_task(n, seed, device):
    """-> (model with a zero trainable head, vocabulary, items, transcripts): the transcripts are the teacher head's greedy output."""
    from unitspeech_amd.asr import HubertForCTC
    teacher, vocabulary = evaluate.synthetic_model(device, seed)
    items = evaluate.synthetic_waves(n, seed)
    resamplers = {}
    wavs16 = [to_16k(w, r, device, resamplers) for _, w, r in items]
    transcripts, _ = evaluate.transcribe_all(teacher, vocabulary, wavs16, n)
    model = HubertForCTC(vocab_size=len(vocabulary), pad_token_id=vocabulary.blank_id, trainable=True, **evaluate.TINY)
    sd = {k: v for k, v in teacher.state_dict().items() if not k.startswith("lm_head.")}
    sd.update({"lm_head." + k: torch.zeros_like(v) for k, v in model.lm_head.state_dict().items()})
    model.load_state_dict(sd)
    return model.to(device).eval(), vocabulary, wavs16, transcripts


def encode_targets(texts, vocabulary, device):
    ids = [vocabulary.encode(t) for t in texts]
    L = max(1, max(len(i) for i in ids))
    tg = torch.full((len(ids), L), (vocabulary.blank_id + 1) % len(vocabulary), dtype=torch.int64)
    for b, i in enumerate(ids):
        tg[b, :len(i)] = torch.tensor(i, dtype=torch.int64)
    return tg.to(device), torch.tensor([len(i) for i in ids], dtype=torch.int64).to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--filelist", default=None, help="`wav|transcript` lines")
    ap.add_argument("--vocab_path", default=None, help="vocab.json: {token: id}")
    ap.add_argument("--encoder_path", default=None, help="state dict of the base-form encoder (or of a whole CTC model)")
    ap.add_argument("--config_path", default=None, help="the encoder's config.json, when it is not the base size")
    ap.add_argument("--blank", default="<pad>")
    ap.add_argument("--word_delimiter", default="|")
    ap.add_argument("--normalize", action="store_true", help="zero mean, unit variance per waveform")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=0, help="stop after this many optimizer steps (0: run the epochs out)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--optimizer", choices=("fused", "torch"), default="fused", help="FusedAdam of the library, or torch.optim.Adam")
    ap.add_argument("--out", default=None, help="where the fitted model's state dict goes")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded waveforms, a seeded tiny encoder, a teacher head's transcripts")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP recogniser has no CPU fallback")
    from unitspeech_amd.asr import CTCVocabulary, error_rates, normalize_text
    device = torch.device(args.device)
    if args.synthetic:
        model, vocabulary, wavs16, transcripts = synthetic_task(args.synthetic, args.seed, device)
    else:
        if not args.filelist or not args.vocab_path or not args.encoder_path:
            raise SystemExit("give --filelist, --vocab_path and --encoder_path, or --synthetic N")
        with open(args.filelist, encoding="utf-8") as f:
            entries = evaluate.parse_filelist(f.read())
        if not entries:
            raise SystemExit(f"{args.filelist}: no files")
        vocabulary = CTCVocabulary(args.vocab_path, args.blank, args.word_delimiter)
        model = build_model(args, vocabulary, device)
        resamplers = {}
        wavs16 = [to_16k(*read_wav(path), device, resamplers) for path, _, _ in entries]
        transcripts = [normalize_text(text, vocabulary) for _, text, _ in entries]
    for i, w in enumerate(wavs16):
        if w.shape[0] < evaluate.MIN_SAMPLES_16K:
            raise SystemExit(f"file {i}: {w.shape[0]} samples at 16 kHz are fewer than the receptive field ({evaluate.MIN_SAMPLES_16K})")
    if args.normalize:
        wavs16 = [(w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7) for w in wavs16]
    params = [model.lm_head.weight, model.lm_head.bias]
    if args.optimizer == "fused":
        from unitspeech_amd.optim import FusedAdam
        opt = FusedAdam(params, lr=args.lr)
    else:
        opt = torch.optim.Adam(params, lr=args.lr)
    batches = plan_batches([int(w.shape[0]) for w in wavs16], args.batch)
    history, steps = [], 0
    for epoch in range(args.epochs):
        total = torch.zeros((), device=device)
        done = 0
        for idx in batches:
            if args.steps and steps >= args.steps:
                break
            x, n = pad_batch([wavs16[i] for i in idx])
            tg, tl = encode_targets([transcripts[i] for i in idx], vocabulary, device)
            opt.zero_grad(set_to_none=True)
            loss = model.loss(x, n, tg, tl, reduction="mean", zero_infinity=True)
            loss.backward()
            opt.step()
            total += loss.detach()
            done += 1
            steps += 1
        if not done:
            break
        hyps, _ = evaluate.transcribe_all(model, vocabulary, wavs16, args.batch)
        scored = [(h, t) for h, t in zip(hyps, transcripts) if t.split()]
        cer = error_rates([h for h, _ in scored], [t for _, t in scored], device)["cer"] if scored else float("nan")
        history.append({"epoch": epoch, "loss": float(total) / done, "cer": cer, "steps": steps})
        print(json.dumps(history[-1]))
    if args.out:
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, args.out)
    return history


if __name__ == "__main__":
    main()
