#!/usr/bin/env python3
"""Text -> waveform for a whole list of utterances on the HIP library, in ragged batches: what inference.py does for one text, with the
utterances batched through every stage, the vocoder included.

    python synthesize_batch.py --textlist LIST --reference_root CHECKOUT --out DIR [--ID N] [--batch 8] [--max_padded_frames 16384]
    python synthesize_batch.py --synthetic 5 --batch 3 --diffusion_steps 2 --dump_mel --out DIR

LIST holds one `name|text` line per utterance.  The utterances are sorted by symbol count and cut into batches (`plan_batches`: at most
--batch items, and at most --max_padded_frames mel frames in the padded batch, estimated before the durations are known as items x
longest symbol count x --frames_per_symbol).  Each batch runs Encoder -> DurationPredictor -> `UnitSpeech.execute_text_to_speech(...,
return_lengths=True, mel_range=...)` -> `BigVGAN.forward(mel, lengths=y_lengths)`: the mel of a batch is cropped to its longest item and
a shorter item holds no silence past its own end, so the vocoder takes each item's frame count and gives it the samples it has when it is
vocoded alone.  Written to DIR: `<name>.wav` (float32, the vocoder's sampling rate, clamped to [-1, 1], `y_lengths[b] * hop` samples) and,
with --dump_mel, `<name>.mel.npy`, the item's [num_mels, y_lengths[b]] slice of the de-normalised mel.

--sv56 [--ndb N] brings each utterance to N dB active speech level (ITU-T P.56, default -26; the reference's sv56 step) on the device: the
batch goes from the vocoder's output and lengths through `unitspeech_amd.level.normalize_level(..., via_int16=True, out_int16=True)` in one
call, and `<name>.wav` is then int16.  --keep_raw with --sv56 also writes `<name>.raw.wav`, the int16 before the normalisation.

--synthetic N runs without checkpoints or a phonemiser, on the stand-ins of `inference.py --synthetic --hip_vocoder`: N seeded sentences
of seeded lengths, seeded decoder weights, the closed-form text encoder / duration predictor (`unitspeech_amd.frontend`) and a seeded
BigVGAN (the 22 kHz / 80-band base generator unless --vocoder_config names another).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.batching import pad_batch, plan_batches as _plan  # noqa: E402

WORDS = ("buna", "ziua", "the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "speech", "unit", "voice", "mel", "wave", "north",
         "wind", "and", "sun", "were", "disputing", "which", "was", "stronger")


def parse_textlist(text: str):
    """`name|text` lines -> [(name, text)] in file order (blank lines are skipped; a text that itself holds `|` stays whole)."""
    out, seen = [], set()
    for no, line in enumerate(text.splitlines(), start=1):
        line = line.strip()
        if not line:
            continue
        name, sep, body = line.partition("|")
        name, body = name.strip(), body.strip()
        if not sep or not name or not body or os.sep in name:
            raise ValueError(f"text list line {no}: expected `name|text`, got {line!r}")
        if name in seen:
            raise ValueError(f"text list line {no}: the name {name!r} appears twice")
        seen.add(name)
        out.append((name, body))
    return out


def plan_batches(symbols, max_batch: int, max_padded_frames: int, frames_per_symbol: int = 6):
    """Cut utterances of the given symbol counts into batches: -> a list of lists of indices into `symbols`.  Sorted by symbol count (ties in
    index order); a batch is closed when one more utterance would make it larger than `max_batch` items or its estimated padded size
    (items x its longest symbol count x `frames_per_symbol`) larger than `max_padded_frames`.  Every index appears exactly once; an
    utterance that alone is over the frame cap gets a batch of its own."""
    if frames_per_symbol < 1:
        raise ValueError("plan_batches: frames_per_symbol must be at least 1")
    return _plan([int(n) * frames_per_symbol if int(n) >= 1 else int(n) for n in symbols], max_batch, max_padded_frames)


def synthetic_texts(n: int, seed: int = 0):
    """-> [(name, text)]: n seeded sentences of 1 to 6 seeded words, so the symbol counts (and with them the frame counts) differ."""
    if n < 1:
        raise ValueError("--synthetic N: N must be at least 1")
    g = np.random.Generator(np.random.Philox(key=9000 + seed))
    out = []
    for i in range(n):
        k = int(g.integers(1, 7))
        out.append((f"synthetic_{i:04d}", " ".join(WORDS[int(j)] for j in g.integers(0, len(WORDS), size=k))))
    return out


def synthetic_vocoder(device, seed: int = 0, config=None):
    """The seeded BigVGAN of --synthetic on `device`, eval mode."""
    from unitspeech_amd.vocoder import BIGVGAN_BASE_22KHZ_80BAND, BigVGAN, synthetic_bigvgan_state_dict
    h = BIGVGAN_BASE_22KHZ_80BAND if config is None else config
    vocoder = BigVGAN(h)
    vocoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(h, seed).items()})
    return vocoder.to(device).eval()


def pad_ids(ids, device):
    """A list of id lists -> (phoneme [B, Lmax] int64 padded with 0, phoneme_lengths [B]) on `device`."""
    x, lens = pad_batch([torch.as_tensor(v, dtype=torch.long) for v in ids])
    return x.to(device), torch.tensor(lens, dtype=torch.long, device=device)


@torch.no_grad()
def synthesize(decoder, text_encoder, duration_predictor, vocoder, ids, spk_emb, mel_range, n_down, max_batch, max_padded_frames,
               frames_per_symbol=6, sv56_ndb=None, keep_raw=False, rate=22050, **tts_kw):
    """ids: one id list per utterance -> ([(wav [n * hop] on the host, clamped; mel [num_mels, n] on the host)] in the order given, the
    batches as `plan_batches` cut them).  With `sv56_ndb` the wav is the int16 of the level normalisation and a third entry follows:
    (level_db, gain, clipped, the un-normalised int16 wav or None)."""
    device = spk_emb.device
    batches = plan_batches([len(v) for v in ids], max_batch, max_padded_frames, frames_per_symbol)
    out = [None] * len(ids)
    for idx in batches:
        phoneme, phoneme_lengths = pad_ids([ids[i] for i in idx], device)
        spk = spk_emb.expand(len(idx), -1, -1).contiguous()
        _, mel, _, y_lengths = decoder.execute_text_to_speech(
            phoneme=phoneme, phoneme_lengths=phoneme_lengths, spk_emb=spk, text_encoder=text_encoder, duration_predictor=duration_predictor,
            num_downsamplings_in_unet=n_down, mel_range=mel_range, return_lengths=True, **tts_kw)
        frames = y_lengths.tolist()                                   # one read for the vocoder's launch and the crops below
        wav = vocoder.forward(mel, lengths=frames).clamp(-1, 1)
        if sv56_ndb is not None:
            from unitspeech_amd.level import normalize_level
            n = y_lengths * vocoder.hop                                  # stays on the device: nothing is read back before the gain is applied
            norm, info = normalize_level(wav, rate, sv56_ndb, lengths=n, via_int16=True, out_int16=True)
            raw = (wav * 32767).to(torch.int16).cpu() if keep_raw else None
            norm, level, gain, clipped = norm.cpu(), info.level_db.tolist(), info.gain.tolist(), info.clipped.tolist()
        wav = wav.cpu()
        mel = mel.cpu()
        for b, i in enumerate(idx):
            n = frames[b] * vocoder.hop
            if sv56_ndb is None:
                out[i] = (wav[b, 0, :n].clone(), mel[b, :, :frames[b]].clone())
            else:
                out[i] = (norm[b, 0, :n].clone(), mel[b, :, :frames[b]].clone(),
                          (level[b], gain[b], clipped[b], None if raw is None else raw[b, 0, :n].clone()))
    return out, batches


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--textlist", default=None, help="`name|text` lines")
    ap.add_argument("--out", required=True, help="directory for <name>.wav (and <name>.mel.npy)")
    ap.add_argument("--batch", type=int, default=8, help="most utterances in one batch")
    ap.add_argument("--max_padded_frames", type=int, default=16384, help="most mel frames in one padded batch, as estimated from the symbols")
    ap.add_argument("--frames_per_symbol", type=int, default=6, help="the estimate's frames per symbol")
    ap.add_argument("--dump_mel", action="store_true", help="also write <name>.mel.npy")
    ap.add_argument("--sv56", action="store_true", help="normalise each utterance's active speech level on the device; <name>.wav is int16")
    ap.add_argument("--ndb", type=float, default=-26.0, help="--sv56: the target level in dB relative to full scale")
    ap.add_argument("--keep_raw", action="store_true", help="--sv56: also write <name>.raw.wav, the int16 before the normalisation")
    ap.add_argument("--ID", type=int, default=-10, help="the speaker ID (a fine-tuned decoder of the reference checkout when >= 0)")
    ap.add_argument("--text_gradient_scale", type=float, default=1.0)
    ap.add_argument("--spk_gradient_scale", type=float, default=1.0)
    ap.add_argument("--length_scale", type=float, default=1.0)
    ap.add_argument("--diffusion_steps", type=int, default=50)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded sentences through seeded weights and the stand-in front end")
    ap.add_argument("--vocoder_config", default=None, help="--synthetic: generator config JSON (default: the 22 kHz / 80-band base BigVGAN)")
    ap.add_argument("--reference_root", default=None, help="checkout of the reference with its checkpoints (without --synthetic)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP decoder and vocoder have no CPU fallback")
    from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_state_dict
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    cfg = DecoderConfig()
    n_down = len(cfg.dim_mults) - 1
    if args.synthetic:
        from unitspeech_amd.frontend import SyntheticFrontEnd, text_to_ids
        items = synthetic_texts(args.synthetic, args.seed)
        decoder = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
        decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()})
        decoder = decoder.to(device).eval()
        fe = SyntheticFrontEnd(cfg.n_feats, device)
        text_encoder, duration_predictor = fe.text_encoder, fe.duration_predictor
        spk = np.random.Generator(np.random.Philox(key=args.ID & 0xffff)).standard_normal((1, 1, cfg.spk_emb_dim), dtype=np.float32)
        spk_emb = torch.from_numpy(spk / np.linalg.norm(spk)).to(device)
        mel_range = (torch.tensor(-11.5, device=device), torch.tensor(2.0, device=device))
        ids = [text_to_ids(text)[0][0].tolist() for _, text in items]
        config = None
        if args.vocoder_config:
            with open(args.vocoder_config) as f:
                config = json.load(f)
        vocoder = synthetic_vocoder(device, 0, config)
    else:
        if not args.textlist or not args.reference_root:
            raise SystemExit("give --textlist and --reference_root (reference checkout with its checkpoints), or --synthetic N")
        with open(args.textlist, encoding="utf-8") as f:
            items = parse_textlist(f.read())
        if not items:
            raise SystemExit(f"{args.textlist}: no utterances")
        root = args.reference_root
        sys.path.insert(0, root)
        from conf.hydra_config import MainConfig as rcfg                                   # noqa: E402
        from unitspeech.text import cleaned_text_to_sequence, phonemize, symbols           # noqa: E402
        from unitspeech.util import get_phonemizer, intersperse                            # noqa: E402
        from unitspeech_amd.checkpoint import build_decoder, load_decoder_checkpoint
        from unitspeech_amd.encoder import DurationPredictor, Encoder
        from unitspeech_amd.vocoder import get_vocoder
        vocoder = get_vocoder(config_path=os.path.join(root, rcfg.vocoder.config_path), checkpoint=os.path.join(root, rcfg.vocoder.ckpt_path),
                              device=device)
        ck = os.path.join(root, rcfg.decoder.checkpoint if args.ID < 0 else f"{rcfg.finetune.finetuned_decoders_path}/{args.ID}.pt")
        dd = load_decoder_checkpoint(ck)
        decoder = build_decoder(dd, device).eval()
        mel_range, spk_emb = (dd.mel_min.to(device), dd.mel_max.to(device)), dd.speaker_embedding(max(args.ID, 0)).to(device)
        e = rcfg.text_encoder
        text_encoder = Encoder(n_vocab=len(symbols) + 1, n_feats=cfg.n_feats, n_channels=e.n_channels, filter_channels=e.filter_channels,
                               n_heads=e.n_heads, n_layers=e.n_layers, kernel_size=e.kernel_size, p_dropout=e.p_dropout,
                               window_size=e.window_size).to(device)
        text_encoder.load_state_dict(torch.load(os.path.join(root, e.checkpoint), map_location="cpu")["model"])
        d = rcfg.duration_predictor
        duration_predictor = DurationPredictor(in_channels=d.in_channels, filter_channels=d.filter_channels, kernel_size=d.kernel_size,
                                               p_dropout=d.p_dropout, spk_emb_dim=d.spk_emb_dim).to(device)
        duration_predictor.load_state_dict(torch.load(os.path.join(root, d.checkpoint), map_location="cpu")["model"])
        text_encoder.eval(); duration_predictor.eval()
        phonemizer = get_phonemizer(rcfg.inference.language)
        ids = [intersperse(cleaned_text_to_sequence(phonemize(text, phonemizer)), len(symbols)) for _, text in items]
    results, batches = synthesize(decoder, text_encoder, duration_predictor, vocoder, ids, spk_emb.reshape(1, 1, -1), mel_range, n_down, args.batch,
                                  args.max_padded_frames, args.frames_per_symbol, sv56_ndb=args.ndb if args.sv56 else None,
                                  keep_raw=args.keep_raw, rate=int(vocoder.h.get("sampling_rate", 22050)), diffusion_steps=args.diffusion_steps,
                                  length_scale=args.length_scale, text_gradient_scale=args.text_gradient_scale,
                                  spk_gradient_scale=args.spk_gradient_scale)
    from scipy.io.wavfile import write
    os.makedirs(args.out, exist_ok=True)
    rate = int(vocoder.h.get("sampling_rate", 22050))
    for (name, _), res in zip(items, results):
        wav, mel = res[0], res[1]
        write(os.path.join(args.out, f"{name}.wav"), rate, wav.numpy())
        if args.dump_mel:
            np.save(os.path.join(args.out, f"{name}.mel.npy"), mel.numpy())
        if args.sv56:
            level, gain, clipped, raw = res[2]
            if raw is not None:
                write(os.path.join(args.out, f"{name}.raw.wav"), rate, raw.numpy())
            print(f"{name}: level {level:.2f} dB, gain {gain:.4f}, {clipped} clipped samples")
    frames = [int(res[1].shape[1]) for res in results]
    padded = sum(len(b) * max(frames[i] for i in b) for b in batches)
    print(f"{len(items)} utterances in {len(batches)} batches ({sum(frames)} mel frames, {padded} padded, "
          f"{sum(frames) * vocoder.hop / rate:.1f} s of audio) -> {args.out}")


if __name__ == "__main__":
    main()
