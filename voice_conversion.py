#!/usr/bin/env python3
"""Voice conversion on the HIP library: the reference's scripts/voice_conversion.py, device-resident from the source waveform to the
converted one, for one source or for a list of sources in ragged batches.

    python voice_conversion.py --source_path SRC.wav --contentvec_path CONTENTVEC.pt [--encoder_path ...] [--decoder_path ...]
                               [--config_path ...] [--generated_sample_path OUT.wav] [--diffusion_step 50]
    python voice_conversion.py --synthetic 3 --batch 2 --diffusion_step 4 --out DIR

Per batch: `Resample(rate, 22050)` when the source's rate differs -> mel_length = samples // hop_length -> `Resample(22050, 16000)` ->
`HubertModel` (ContentVec) at last_hidden_state -> `UnitSpeech.execute_voice_conversion(..., mel_range=(mel_min, mel_max),
return_lengths=True)` (ContentVec encoder, `us_vc_align`, reverse diffusion) -> `BigVGAN(mel, lengths)` -> one wav per source, clamped to
[-1, 1], `mel_length * hop` samples.  One line is printed per batch.

The flags are the reference's, plus: --contentvec_path, a local state dict in `transformers`' layout (what
`HubertModelWithFinalProj.from_pretrained(...).state_dict()` saves; `final_proj.*` is ignored) -- nothing is fetched by name;
--vocoder_config / --vocoder_path when the config's own vocoder paths do not resolve from the working directory; --seed; --batch K and
--out DIR for several sources (--source_path may be given more than once; the outputs are DIR/<source name>.wav).  The source is read
with scipy.io.wavfile (PCM or float wav; several channels are averaged) and resampled by the library's own `Resample`, not by librosa.

--sv56 [--ndb N] brings each converted waveform to N dB active speech level (ITU-T P.56, default -26; the reference's sv56 step): the batch
goes from the vocoder's output and lengths through `unitspeech_amd.level.normalize_level(..., via_int16=True, out_int16=True)` in one call
and the wavs are int16.  --keep_raw with --sv56 also writes `<name>.raw.wav`, the int16 before the normalisation.

--synthetic N needs no files: N seeded waveforms of different lengths (`unitspeech_amd.mel.synthetic_waveform`) in length-sorted batches
of K through seeded weights of every module (HuBERT-base, the voice-conversion.json encoder, the decoder, the base BigVGAN).
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
from unitspeech_amd.audio import read_wav  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402

VC_ENCODER = dict(n_channels=192, filter_channels=768, n_layers=6, kernel_size=3, p_dropout=0.1, n_heads=2, window_size=4,
                  n_contentvec=768)                     # unitspeech/checkpoints/voice-conversion.json "encoder"
SAMPLING_RATE, HOP = 22050, 256


def synthetic_sources(n: int, seed: int = 0):
    """-> [(name, waveform at 22050 Hz)]: n seeded waveforms of 0.6 to 1.5 s, all of different lengths."""
    if n < 1:
        raise ValueError("--synthetic N: N must be at least 1")
    from unitspeech_amd.mel import synthetic_waveform
    g = np.random.Generator(np.random.Philox(key=7000 + seed))
    out = []
    for i in range(n):
        samples = int(g.integers(int(0.6 * SAMPLING_RATE), int(1.5 * SAMPLING_RATE))) + i
        out.append((f"synthetic_{i:04d}", synthetic_waveform(samples, seed * 1000 + i, SAMPLING_RATE)))
    return out


class Pipeline:
    """The modules of one conversion run on one device, and `convert(waveforms, rate)` for one batch."""

    def __init__(self, contentvec, encoder, decoder, vocoder, spk_emb, mel_range, n_down, hop, sampling_rate, device):
        self.contentvec, self.encoder, self.decoder, self.vocoder = contentvec, encoder, decoder, vocoder
        self.spk_emb, self.mel_range, self.n_down, self.hop, self.sampling_rate, self.device = spk_emb, mel_range, n_down, hop, sampling_rate, device
        self._resamplers = {}

    def resampler(self, orig, new):
        from unitspeech_amd.resample import Resample
        key = (int(orig), int(new))
        if key not in self._resamplers:
            self._resamplers[key] = Resample(*key).to(self.device)
        return self._resamplers[key]

    @torch.no_grad()
    def convert(self, waves, rate, sv56_ndb=None, keep_raw=False, **vc_kw):
        """waves: float32 arrays sampled at `rate` -> ([waveform [mel_length * hop] on the host per source], a dict of the batch's counts).
        With `sv56_ndb` the waveforms are the int16 of the level normalisation and the dict also holds level_db, gain, clipped and, with
        `keep_raw`, raw: the int16 waveforms before it."""
        B = len(waves)
        wav, lens = pad_batch(waves)
        wav = wav.to(self.device)
        if rate != self.sampling_rate:
            r = self.resampler(rate, self.sampling_rate)
            wav, lens = r(wav, lens), [r.out_length(n) for n in lens]
        mel_lengths = [n // self.hop for n in lens]                                   # scripts/voice_conversion.py:65
        if min(mel_lengths) < 1:
            raise ValueError(f"a source shorter than one mel frame ({self.hop} samples at {self.sampling_rate} Hz)")
        r16 = self.resampler(self.sampling_rate, 16000)
        wav16, lens16 = r16(wav, lens), [r16.out_length(n) for n in lens]
        feats = self.contentvec(wav16, lens16)                                        # last_hidden_state [B, L, H]
        cv_lengths = [self.contentvec.frames(n) for n in lens16]
        spk = self.spk_emb.expand(B, -1, -1).contiguous()
        _, mel, _ = self.decoder.execute_voice_conversion(
            feats, torch.tensor(cv_lengths, dtype=torch.long, device=self.device), mel_lengths, spk, self.encoder, self.n_down,
            mel_range=self.mel_range, return_lengths=True, **vc_kw)
        audio = self.vocoder.forward(mel, lengths=mel_lengths).clamp(-1, 1)
        extra = {}
        if sv56_ndb is not None:
            from unitspeech_amd.level import normalize_level
            samples = [n * self.vocoder.hop for n in mel_lengths]
            norm, lv = normalize_level(audio, self.sampling_rate, sv56_ndb, lengths=samples, via_int16=True, out_int16=True)
            extra = dict(level_db=lv.level_db.tolist(), gain=lv.gain.tolist(), clipped=lv.clipped.tolist())
            if keep_raw:
                raw = (audio * 32767).to(torch.int16).cpu()
                extra["raw"] = [raw[b, 0, :samples[b]].clone() for b in range(B)]
            audio = norm
        audio = audio.cpu()
        out = [audio[b, 0, :mel_lengths[b] * self.vocoder.hop].clone() for b in range(B)]
        return out, dict(sources=B, contentvec_frames=cv_lengths, mel_frames=mel_lengths, samples=[int(o.numel()) for o in out], **extra)


def build_synthetic(device, seed):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hubert_torch import base_config, synthetic_hubert_state_dict
    from synthesize_batch import synthetic_vocoder
    from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_state_dict
    from unitspeech_amd.encoder import ContentVecEncoder, EncoderConfig, synthetic_encoder_state_dict
    from unitspeech_amd.hubert import HubertModel
    cfg = DecoderConfig()
    decoder = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
    decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()})
    contentvec = HubertModel.base()
    contentvec.load_state_dict(synthetic_hubert_state_dict(base_config(), seed))
    e = VC_ENCODER
    ecfg = EncoderConfig(150, cfg.n_feats, e["n_channels"], e["filter_channels"], e["n_heads"], e["n_layers"], e["kernel_size"], e["window_size"],
                         e["n_contentvec"])
    encoder = ContentVecEncoder(n_vocab=150, n_feats=cfg.n_feats, **e)
    encoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(ecfg, seed).items()})
    spk = np.random.Generator(np.random.Philox(key=8000 + seed)).standard_normal((1, 1, cfg.spk_emb_dim), dtype=np.float32)
    spk_emb = torch.from_numpy(spk / np.linalg.norm(spk)).to(device)
    mel_range = (torch.tensor(-11.5, device=device), torch.tensor(2.0, device=device))
    vocoder = synthetic_vocoder(device, 0)
    return Pipeline(contentvec.to(device).eval(), encoder.to(device).eval(), decoder.to(device).eval(), vocoder, spk_emb, mel_range,
                    len(cfg.dim_mults) - 1, HOP, SAMPLING_RATE, device)


def build_from_checkpoints(args, device):
    from unitspeech_amd import UnitSpeech
    from unitspeech_amd.encoder import ContentVecEncoder
    from unitspeech_amd.hubert import HubertModel
    from unitspeech_amd.vocoder import get_vocoder
    if not args.contentvec_path:
        raise SystemExit("--contentvec_path: a local state dict of the ContentVec model in transformers' layout is needed (nothing is fetched by name)")
    with open(args.config_path) as f:
        hps = json.load(f)
    data, dec = hps["data"], hps["decoder"]
    contentvec = HubertModel.base()
    sd = torch.load(args.contentvec_path, map_location="cpu")
    contentvec.load_state_dict(sd["model"] if "model" in sd and not torch.is_tensor(sd["model"]) else sd)
    encoder = ContentVecEncoder(n_vocab=150, n_feats=data["n_feats"], **hps["encoder"])
    encoder.load_state_dict(torch.load(args.encoder_path, map_location="cpu")["model"])
    decoder = UnitSpeech(n_feats=data["n_feats"], **dec)
    dd = torch.load(args.decoder_path, map_location="cpu")
    decoder.load_state_dict(dd["model"])
    vocoder = get_vocoder(args.vocoder_config or hps["train"]["vocoder_config_path"], args.vocoder_path or hps["train"]["vocoder_ckpt_path"], device)
    spk_emb = torch.as_tensor(dd["spk_emb"]).reshape(1, 1, -1).to(device)
    mel_range = (torch.as_tensor(dd["mel_min"]).to(device), torch.as_tensor(dd["mel_max"]).to(device))
    return Pipeline(contentvec.to(device).eval(), encoder.to(device).eval(), decoder.to(device).eval(), vocoder, spk_emb, mel_range,
                    len(dec["dim_mults"]) - 1, int(data["hop_length"]), int(data["sampling_rate"]), device)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--encoder_path", default="unitspeech/checkpoints/contentvec_encoder.pt", help="ContentVec encoder checkpoint")
    ap.add_argument("--decoder_path", default="unitspeech/outputs/finetuned_decoder.pt", help="fine-tuned decoder checkpoint")
    ap.add_argument("--config_path", default="unitspeech/checkpoints/voice-conversion.json", help="configuration of voice conversion")
    ap.add_argument("--generated_sample_path", default="unitspeech/outputs/output_vc.wav", help="where the converted audio of one source goes")
    ap.add_argument("--source_path", action="append", default=None, help="source audio (wav); more than one needs --out")
    ap.add_argument("--text_gradient_scale", type=float, default=1.0)
    ap.add_argument("--spk_gradient_scale", type=float, default=1.0)
    ap.add_argument("--diffusion_step", type=int, default=50)
    ap.add_argument("--contentvec_path", default=None, help="local transformers-layout state dict of the ContentVec model")
    ap.add_argument("--vocoder_config", default=None)
    ap.add_argument("--vocoder_path", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded sources through seeded weights; needs no files")
    ap.add_argument("--batch", type=int, default=8, metavar="K", help="most sources in one batch")
    ap.add_argument("--out", default=None, metavar="DIR", help="directory for <name>.wav (several sources, --synthetic)")
    ap.add_argument("--sv56", action="store_true", help="normalise each converted waveform's active speech level on the device; the wavs are int16")
    ap.add_argument("--ndb", type=float, default=-26.0, help="--sv56: the target level in dB relative to full scale")
    ap.add_argument("--keep_raw", action="store_true", help="--sv56: also write <name>.raw.wav, the int16 before the normalisation")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP library has no CPU fallback")
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    if args.synthetic:
        if not args.out:
            raise SystemExit("--synthetic needs --out DIR")
        items = [(name, w, SAMPLING_RATE) for name, w in synthetic_sources(args.synthetic, args.seed)]
        pipe = build_synthetic(device, args.seed)
    else:
        if not args.source_path:
            raise SystemExit("give --source_path (a wav file), or --synthetic N")
        if len(args.source_path) > 1 and not args.out:
            raise SystemExit("several --source_path need --out DIR")
        items = [(os.path.splitext(os.path.basename(p))[0],) + read_wav(p) for p in args.source_path]
        pipe = build_from_checkpoints(args, device)
    from scipy.io.wavfile import write
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    # one batch holds sources of one sampling rate, sorted by length
    for rate in sorted({r for _, _, r in items}):
        group = [i for i, it in enumerate(items) if it[2] == rate]
        for batch in plan_batches([len(items[i][1]) for i in group], args.batch):
            idx = [group[j] for j in batch]
            out, info = pipe.convert([items[i][1] for i in idx], rate, sv56_ndb=args.ndb if args.sv56 else None,
                                     keep_raw=args.sv56 and args.keep_raw, diffusion_steps=args.diffusion_step,
                                     text_gradient_scale=args.text_gradient_scale, spk_gradient_scale=args.spk_gradient_scale)
            for k, (i, wav) in enumerate(zip(idx, out)):
                path = os.path.join(args.out, items[i][0] + ".wav") if args.out else args.generated_sample_path
                if os.path.dirname(path):
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                write(path, pipe.sampling_rate, wav.numpy())
                if "raw" in info:
                    write(os.path.splitext(path)[0] + ".raw.wav", pipe.sampling_rate, info["raw"][k].numpy())
                if args.sv56:
                    print(f"{items[i][0]}: level {info['level_db'][k]:.2f} dB, gain {info['gain'][k]:.4f}, {info['clipped'][k]} clipped samples")
            print(f"batch of {info['sources']} sources: contentvec frames {info['contentvec_frames']}, mel frames {info['mel_frames']}, "
                  f"samples written {info['samples']}", flush=True)


if __name__ == "__main__":
    main()
