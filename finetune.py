#!/usr/bin/env python3
"""Speaker adaptation with the HIP decoder: the reference's `finetune.py` command line (:177-191) and inner loop (:131-165:
`decoder.fine_tune` -> `loss.backward()` -> `clip_grad_norm_(1)` -> `Adam(lr=2e-5).step()`), decoder swapped for
`unitspeech_amd.UnitSpeech`.

  default       the reference's pre-steps (speaker embedder, unit extractor, unit encoder, mel extraction; finetune.py:47-128)
                come from a checkout of the reference given with --reference_root and stay on the stock PyTorch path.
  --synthetic   seeded synthetic decoder weights and a synthetic (mel, units, durations, speaker embedding) tuple: runs the
                fine-tuning loop itself (BASELINE.json configs[3]) without any downloaded model.  --hip_mel takes the mel from a seeded
                waveform through the HIP mel front end instead of random numbers; --hip_hubert (with --hip_units) takes the dense features
                from the HIP HuBERT encoder (seeded base-size weights) on a seeded waveform, resampled 22050 -> 16000 with --hip_resample;
                --hip_wavlm takes spk_emb from the HIP WavLM-large (seeded) in front of the seeded HIP ECAPA-TDNN on that waveform.
  --features F  the OUTPUTS of the reference's pre-steps (finetune.py:86-128) from a `.pt` (torch.save of a dict) or `.npz` file, so the
                speaker embedder / unit extractor can run wherever their checkpoints live and the adaptation here:
                  mel        [1, 80, L]   normalised to [-1, 1] as finetune.py:104 leaves it (or raw with "mel_is_normalized": False); or
                             wav [T] or [1, T], the reference utterance at the decoder's sampling rate (`wav_sampling_rate`, when given,
                             must say so, unless --hip_resample is given: the waveform is then brought to 22050 Hz on the device,
                             unitspeech_amd.resample): the mel of :86-104 is then computed on the device (unitspeech_amd.mel) and
                             normalised with mel_min / mel_max
                  spk_emb    [1, 256] or [1, 1, 256]   (divided by its norm here, :110); or  spk_hidden_states [L, 1, T, C], the
                             speaker encoder's upstream hidden states (ecapa_tdnn.py:262-264) + --speaker_encoder_checkpoint (:106-110)
                             or  wav with --hip_wavlm + --speaker_encoder_path, the reference's whole embedder checkpoint: the waveform
                             is brought to 16 kHz on the device and WavLM and the ECAPA-TDNN both run on HIP (:113-117)
                  duration   [1, Lu]      frames per unit (process_unit, :114)
                  cond_x     [1, 80, Lu]  the unit encoder's output (:123); or  unit [1, Lu] int64 + --unit_encoder_checkpoint (:66-79)
                  dense      [T, D]       in place of unit / duration: the unit extractor's dense features (:112), quantised and brought to
                             the mel rate on the device (unitspeech_amd.units) with the centres of --kmeans_checkpoint (a scikit-learn
                             KMeans saved with joblib) or `centers` [K, D] in the file; needs --unit_encoder_checkpoint
                  wav                     also in place of dense / unit / duration, with --hubert_checkpoint (a HuBERT-base checkpoint in
                             transformers' or fairseq's layout; --hubert_layer, default 11) and --kmeans_checkpoint: the waveform is
                             brought to 16 kHz on the device (:113), the HIP HuBERT encoder (unitspeech_amd.hubert) gives the dense features
                             and the units come from them as above
                  mel_min, mel_max        scalars (else the decoder checkpoint's, :98-99)
Saves {"model", "spk_emb", "mel_min", "mel_max"} like finetune.py:167-173.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

from unitspeech_amd import DecoderConfig, FusedAdam, UnitSpeech, synthetic_state_dict
from unitspeech_amd.audio import load_tensor_file
from unitspeech_amd.checkpoint import build_decoder, infer_config, load_decoder_checkpoint, save_finetuned_checkpoint
from unitspeech_amd.util import fix_len_compatibility, generate_path, sequence_mask


SAMPLING_RATE = 22050
MEL_ARGS = (1024, 80, SAMPLING_RATE, 256, 1024, 0, 8000)          # finetune.py:86-96: n_fft, num_mels, sampling_rate, hop, win, fmin, fmax


def load_features(args, cfg, base, device):
    """--features: (mel, cond_x, duration, spk_emb, mel_min, mel_max) on `device` from the file the reference's pre-steps were saved to."""
    path = args.features
    d = {k: (torch.as_tensor(v) if not isinstance(v, torch.Tensor) else v) for k, v in load_tensor_file(path).items()}
    if "wav" in d and getattr(args, "hubert_checkpoint", None) and not any(k in d for k in ("dense", "unit", "cond_x")):
        # finetune.py:112-113: the unit extractor's dense model on the utterance at 16 kHz
        from unitspeech_amd.hubert import HubertFeatureReader, load_hubert_checkpoint
        from unitspeech_amd.resample import Resample
        rate = int(d["wav_sampling_rate"]) if "wav_sampling_rate" in d else SAMPLING_RATE
        wav16 = d["wav"].float().reshape(1, -1).to(device)
        if rate != 16000:
            wav16 = Resample(rate, 16000).to(device)(wav16)                     # :113, torchaudio.transforms.Resample(22050, 16000)
        hubert, normalize = load_hubert_checkpoint(args.hubert_checkpoint)
        d["dense"] = HubertFeatureReader(hubert, layer=args.hubert_layer, normalize=normalize).to(device)(wav16[0]).cpu()
    if "dense" in d and "unit" not in d and "cond_x" not in d:
        # finetune.py:112-114: KMeans.predict, unique_consecutive and process_unit(encoded, 16000, 256), here in one library call
        from unitspeech_amd.units import KMeansQuantizer
        if "centers" not in d and not args.kmeans_checkpoint:
            raise SystemExit(f"--features {path}: `dense` needs the k-means centres: --kmeans_checkpoint or `centers` in the file")
        quantizer = KMeansQuantizer.from_centers(d["centers"]) if "centers" in d else KMeansQuantizer(args.kmeans_checkpoint)
        dense = d["dense"].float().reshape(1, -1, d["dense"].shape[-1]).to(device)
        unit, duration, n = quantizer.encode(dense, None, 16000, 256)
        n = int(n[0])
        if int(quantizer.last_counters[0]):
            raise SystemExit(f"--features {path}: `dense` has rows with non-finite values")
        d["unit"], d["duration"] = unit[:, :n].cpu(), duration[:, :n].cpu()
    hip_spk = bool(args.speaker_encoder_checkpoint) and "spk_emb" not in d and "spk_hidden_states" in d
    hip_wavlm = getattr(args, "hip_wavlm", False) and bool(getattr(args, "speaker_encoder_path", None)) and "spk_emb" not in d and "wav" in d
    if getattr(args, "hip_wavlm", False) and not hip_wavlm and "spk_emb" not in d:
        raise SystemExit(f"--features {path}: --hip_wavlm needs `wav` in the file and --speaker_encoder_path (the whole embedder's checkpoint)")
    hip_mel = "mel" not in d and "wav" in d
    for k in ("mel", "spk_emb", "duration"):
        if k not in d and not (k == "spk_emb" and (hip_spk or hip_wavlm)) and not (k == "mel" and hip_mel):
            raise SystemExit(f"--features {path}: missing `{k}`" + (" (or `wav`)" if k == "mel" else ""))

    def scalar(name):
        if name in d:
            return d[name].float().reshape(())
        if base is not None and getattr(base, name, None) is not None:
            return getattr(base, name).float().reshape(())
        raise SystemExit(f"--features {path}: no `{name}` in the file and no decoder checkpoint to take it from (finetune.py:98-99)")
    mel_min, mel_max = scalar("mel_min"), scalar("mel_max")
    if hip_mel:
        # finetune.py:86-104: mel_spectrogram(wav, 1024, 80, 22050, 256, 1024, 0, 8000, center=False), then the normalisation
        from unitspeech_amd.mel import MelSpectrogram
        rate = int(d["wav_sampling_rate"]) if "wav_sampling_rate" in d else SAMPLING_RATE
        if rate != SAMPLING_RATE and not getattr(args, "hip_resample", False):
            raise SystemExit(f"--features {path}: `wav` is at {rate} Hz, the decoder's mel is defined at {SAMPLING_RATE} Hz; "
                             "resample it first, or pass --hip_resample to have the library do it on the device")
        wav = d["wav"].float()
        if wav.dim() not in (1, 2) or (wav.dim() == 2 and wav.shape[0] != 1):
            raise SystemExit(f"--features: wav must be [T] or [1, T], got {tuple(wav.shape)}")
        wav = wav.reshape(1, -1).to(device)
        if rate != SAMPLING_RATE:
            from unitspeech_amd.resample import Resample
            wav = Resample(rate, SAMPLING_RATE).to(device)(wav)                  # data.py:75, torchaudio.transforms.Resample(sr, 22050)
        mel = MelSpectrogram(*MEL_ARGS).to(device)(wav, mel_min=mel_min, mel_max=mel_max).cpu()
    else:
        mel = d["mel"].float()
    if mel.dim() == 2:
        mel = mel.unsqueeze(0)
    if mel.dim() != 3 or mel.shape[0] != 1 or mel.shape[1] != cfg.n_feats:
        raise SystemExit(f"--features: mel must be [1, {cfg.n_feats}, L], got {tuple(mel.shape)}")
    if not hip_mel and "mel_is_normalized" in d and not bool(d["mel_is_normalized"]):
        mel = (mel - mel_min) / (mel_max - mel_min) * 2 - 1                      # finetune.py:104
    if hip_wavlm:
        # finetune.py:113-117: the utterance at 16 kHz through the whole speaker embedder (WavLM, then the ECAPA-TDNN), over its norm
        from unitspeech_amd.resample import Resample
        from unitspeech_amd.speaker_encoder import load_speaker_embedder_checkpoint
        rate = int(d["wav_sampling_rate"]) if "wav_sampling_rate" in d else SAMPLING_RATE
        wav16 = d["wav"].float().reshape(1, -1).to(device)
        if rate != 16000:
            wav16 = Resample(rate, 16000).to(device)(wav16)
        spk = load_speaker_embedder_checkpoint(args.speaker_encoder_path, device).embed_wav(wav16).reshape(1, 1, -1)
        if spk.shape[-1] != cfg.spk_emb_dim:
            raise SystemExit(f"--speaker_encoder_path: the embedder gives {spk.shape[-1]} elements, the decoder takes {cfg.spk_emb_dim}")
    elif hip_spk:
        from unitspeech_amd.speaker_encoder import load_speaker_encoder_checkpoint
        hidden = d["spk_hidden_states"].float()
        spk_embedder = load_speaker_encoder_checkpoint(args.speaker_encoder_checkpoint, device, feat_dim=int(hidden.shape[-1]),
                                                       emb_dim=cfg.spk_emb_dim)                      # :48-49
        spk = spk_embedder.embed(hidden.to(device)).reshape(1, 1, -1)                              # :106-110, the norm included
    else:
        spk = d["spk_emb"].float().reshape(1, 1, -1)
        if spk.shape[-1] != cfg.spk_emb_dim:
            raise SystemExit(f"--features: spk_emb must have {cfg.spk_emb_dim} elements, got {spk.shape[-1]}")
        spk = spk / spk.norm()                                                   # :110
    duration = d["duration"].float().reshape(1, -1)
    if "cond_x" in d:
        cond_x = d["cond_x"].float()
        if cond_x.dim() == 2:
            cond_x = cond_x.unsqueeze(0)
    elif "unit" in d:
        if not args.unit_encoder_checkpoint:
            raise SystemExit("--features with `unit` needs --unit_encoder_checkpoint (or store the unit encoder's output as `cond_x`)")
        from unitspeech_amd.encoder import Encoder, EncoderConfig
        sd = torch.load(args.unit_encoder_checkpoint, map_location="cpu")
        sd = sd["model"] if "model" in sd else sd
        ec = EncoderConfig(n_vocab=int(sd["emb.weight"].shape[0]), n_feats=cfg.n_feats)
        unit_encoder = Encoder(ec.n_vocab, ec.n_feats, ec.n_channels, ec.filter_channels, ec.n_heads, ec.n_layers, ec.kernel_size, 0.1,
                               window_size=ec.window_size)
        unit_encoder.load_state_dict(sd)
        unit = d["unit"].long().reshape(1, -1).to(device)
        with torch.no_grad():
            cond_x, _, _ = unit_encoder.to(device).eval()(unit, torch.LongTensor([unit.shape[-1]]).to(device))        # :122-123
    else:
        raise SystemExit(f"--features {path}: give `cond_x` (the unit encoder's output) or `unit`")
    if cond_x.shape[0] != 1 or cond_x.shape[1] != cfg.n_feats or cond_x.shape[-1] != duration.shape[-1]:
        raise SystemExit(f"--features: cond_x {tuple(cond_x.shape)} and duration {tuple(duration.shape)} disagree")
    if int(duration.sum()) > mel.shape[-1] + duration.shape[-1]:
        raise SystemExit(f"--features: the durations cover {int(duration.sum())} frames, the mel has {mel.shape[-1]}")
    return mel.to(device), cond_x.float().to(device), duration.to(device), spk.to(device), mel_min, mel_max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference_sample", type=str, default="reference.wav", help="Sample used to adapt the model to the speaker.")
    ap.add_argument("--ID", type=int, default=-1, help="Unique value used to identify the finetuned decoder.")
    ap.add_argument("--n_iters", type=int, default=500, help="Number of fine-tuning iterations.")
    ap.add_argument("--learning_rate", type=float, default=2e-5, help="Learning rate of the optimizer during fine-tuning.")
    ap.add_argument("--torch_optimizer", action="store_true", help="clip_grad_norm_ + torch.optim.Adam instead of the HIP clip+Adam")
    ap.add_argument("--no_graph", action="store_true", help="launch every kernel of an iteration eagerly instead of replaying the captured HIP graph of the forward (unitspeech_amd.graph)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--features", type=str, default=None, help="file with the pre-step tensors of finetune.py:86-128 (see the module docstring)")
    ap.add_argument("--unit_encoder_checkpoint", type=str, default=None, help="--features with `unit` instead of `cond_x`: the unit encoder's "
                                                                              "checkpoint ({'model': state_dict}, finetune.py:77-78)")
    ap.add_argument("--kmeans_checkpoint", type=str, default=None, help="--features with `dense` instead of `unit` / `duration`: the unit "
                    "extractor's k-means model (scikit-learn KMeans saved with joblib); units and durations come from the HIP unit extraction")
    ap.add_argument("--hip_units", action="store_true", help="--synthetic --learned_frontend: the units and durations come from the HIP unit "
                    "extraction (k-means quantiser + process_unit) on synthetic dense features and centres instead of random units")
    ap.add_argument("--hip_hubert", action="store_true", help="--synthetic --learned_frontend --hip_units: the dense features come from the HIP "
                    "HuBERT encoder (seeded base-size weights) on a seeded waveform (at 22050 Hz and resampled on the device with --hip_resample)")
    ap.add_argument("--hubert_checkpoint", type=str, default=None, help="--features with `wav` instead of `dense` / `unit`: a HuBERT-base checkpoint "
                    "(transformers' state_dict or fairseq's {'model': ...}) for the HIP HuBERT encoder; needs --kmeans_checkpoint or `centers`")
    ap.add_argument("--hubert_layer", type=int, default=11, help="the encoder layer whose output is quantised (the reference's mHuBERT units: 11)")
    ap.add_argument("--speaker_encoder_checkpoint", type=str, default=None, help="--features with `spk_hidden_states` instead of `spk_emb`: the "
                    "speaker encoder's checkpoint ({'model': state_dict}, util.py:183-188); the embedding comes from the HIP ECAPA-TDNN")
    ap.add_argument("--hip_speaker_encoder", action="store_true", help="--synthetic: spk_emb from the HIP ECAPA-TDNN (seeded weights) on "
                    "synthetic upstream hidden states instead of a random vector")
    ap.add_argument("--hip_wavlm", action="store_true", help="--synthetic: spk_emb from the HIP WavLM-large (seeded weights drawn on the device) in "
                    "front of the seeded HIP ECAPA-TDNN, on a seeded waveform (at 22050 Hz and resampled on the device with --hip_resample); "
                    "--features with `wav`: spk_emb from the whole embedder of --speaker_encoder_path")
    ap.add_argument("--speaker_encoder_path", type=str, default=None, help="--features with `wav` and --hip_wavlm: the reference's speaker "
                    "embedder checkpoint ({'model': state_dict} with its feature_extract.* keys); WavLM and the ECAPA-TDNN both run on HIP")
    ap.add_argument("--wavlm_layers", type=int, default=24, help="--synthetic --hip_wavlm: encoder layers of the seeded WavLM (the trunk then "
                    "takes that many + 1 hidden states); for short test runs")
    ap.add_argument("--hip_mel", action="store_true", help="--synthetic: the mel comes from the HIP mel front end on a seeded waveform (normalised "
                    "with mel_min / mel_max) instead of random numbers")
    ap.add_argument("--hip_resample", action="store_true", help="--features with `wav` at another `wav_sampling_rate` than 22050: resample it "
                    "on the device (the HIP sinc resampler, torchaudio.transforms.Resample's arithmetic) before the mel")
    ap.add_argument("--learned_frontend", action="store_true", help="--synthetic: cond_x from the HIP unit encoder (seeded weights) on synthetic units")
    ap.add_argument("--reference_root", type=str, default=None)
    ap.add_argument("--out_dir", type=str, default="checkpoints/inference")
    ap.add_argument("--decoder_checkpoint", type=str, default=None,
                    help="pre-trained decoder checkpoint to start from (train_STEP1.py:297-304 layout); --synthetic uses seeded weights otherwise")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--report_memory", action="store_true", help="print the allocated device memory with every progress line and the f16x3 range status at the end")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the HIP decoder has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    import random
    random.seed(args.seed)
    cfg = DecoderConfig()
    n_down = len(cfg.dim_mults) - 1
    segment = fix_len_compatibility(2 * 22050 // 256, n_down)                 # out_size, finetune.py:40-44 (= 176)
    base = None
    if args.decoder_checkpoint:
        base = load_decoder_checkpoint(args.decoder_checkpoint)                  # finetune.py:61-63
        decoder = build_decoder(base)
        cfg = infer_config(base.model)
    else:
        decoder = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)

    if args.features:
        if base is None and args.synthetic:
            decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()})
        elif base is None:
            raise SystemExit("--features needs --decoder_checkpoint (or --synthetic for seeded decoder weights)")
        mel, cond_x, duration, spk_emb, mel_min, mel_max = load_features(args, cfg, base, device)
    elif args.synthetic:
        if base is None:
            decoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()})
        g = np.random.Generator(np.random.Philox(key=args.ID & 0xffff))
        L = 600
        Lu = L // 3
        mel = torch.from_numpy(g.standard_normal((1, cfg.n_feats, L), dtype=np.float32)).clamp(-1, 1).to(device)
        if args.hip_mel:
            # finetune.py:86-104: the mel of the reference utterance and its normalisation; here L frames of a seeded waveform
            from unitspeech_amd.mel import MelSpectrogram, synthetic_waveform
            wav = torch.from_numpy(synthetic_waveform(L * MEL_ARGS[3], args.ID & 0xffff, SAMPLING_RATE)).to(device)
            mel = MelSpectrogram(*MEL_ARGS).to(device)(wav, mel_min=-11.5, mel_max=2.0)
            print(f"hip mel: {wav.numel()} samples -> {mel.shape[-1]} frames in [{float(mel.min()):.3f}, {float(mel.max()):.3f}]")
        cond_x = (torch.from_numpy(g.standard_normal((1, cfg.n_feats, Lu), dtype=np.float32)) * 0.5).to(device)
        if args.learned_frontend:
            # finetune.py:66-78,122-123: cond_x is the (frozen, eval-mode) unit encoder's output for the utterance's unit sequence;
            # here the HIP Encoder at the reference's sizes (n_vocab = n_units = 1000) with seeded weights on synthetic units
            from unitspeech_amd.encoder import Encoder, EncoderConfig, synthetic_encoder_state_dict
            ec = EncoderConfig(n_vocab=1000, n_feats=cfg.n_feats)
            unit_encoder = Encoder(ec.n_vocab, ec.n_feats, ec.n_channels, ec.filter_channels, ec.n_heads, ec.n_layers, ec.kernel_size, 0.1,
                                   window_size=ec.window_size)
            unit_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(ec, 0).items()})
            unit = torch.from_numpy(g.integers(0, ec.n_vocab, size=(1, Lu)).astype(np.int64)).to(device)
            duration = torch.full((1, Lu), 3.0, device=device)
            if args.hip_hubert and not args.hip_units:
                raise SystemExit("--hip_hubert needs --hip_units (its features feed the unit quantiser)")
            if args.hip_units:
                # finetune.py:112-114: the units are the k-means labels of the unit extractor's dense features (50 Hz, 16 kHz audio) brought
                # to the mel rate by process_unit(encoded, 16000, 256); here seeded centres and features for the L mel frames
                from unitspeech_amd.units import KMeansQuantizer, synthetic_centers, synthetic_dense
                centers = synthetic_centers(ec.n_vocab, 768, args.ID & 0xffff)
                if args.hip_hubert:
                    # finetune.py:112-113: the dense features are the unit extractor's HuBERT on the utterance at 16 kHz; here seeded base-size
                    # weights on a seeded waveform of L * 256 // 320 frames
                    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
                    from hubert_torch import base_config, synthetic_hubert_state_dict
                    from unitspeech_amd.hubert import HubertFeatureReader, HubertModel
                    from unitspeech_amd.mel import synthetic_waveform
                    n16 = 400 + 320 * (L * 256 // 320 - 1)
                    if args.hip_resample:
                        from unitspeech_amd.resample import Resample
                        n22 = -(-n16 * 441 // 320)
                        wav16 = Resample(SAMPLING_RATE, 16000).to(device)(torch.from_numpy(synthetic_waveform(n22, args.ID & 0xffff, SAMPLING_RATE)).to(device))[:n16]
                    else:
                        wav16 = torch.from_numpy(synthetic_waveform(n16, args.ID & 0xffff, 16000)).to(device)
                    hubert = HubertModel.base()
                    hubert.load_state_dict(synthetic_hubert_state_dict(base_config(), args.ID & 0xffff))
                    dense = HubertFeatureReader(hubert, layer=args.hubert_layer).to(device)(wav16)
                    print(f"hip hubert: {wav16.numel()} samples at 16 kHz -> {dense.shape[0]} frames of {dense.shape[1]} (layer {args.hubert_layer})")
                else:
                    dense = torch.from_numpy(synthetic_dense(centers, L * 256 // 320, args.ID & 0xffff)).to(device)
                unit, duration, n = KMeansQuantizer.from_centers(centers).encode(dense.unsqueeze(0), None, 16000, 256)
                Lu = int(n[0])
                unit, duration = unit[:, :Lu], duration[:, :Lu]
                print(f"hip units: {dense.shape[0]} dense frames -> {Lu} units over {int(duration.sum())} mel frames")
            cond_x, _, _ = unit_encoder.to(device).eval()(unit, torch.LongTensor([Lu]).to(device))
        else:
            if args.hip_units:
                raise SystemExit("--hip_units needs --learned_frontend (the units feed the HIP unit encoder)")
            if args.hip_hubert:
                raise SystemExit("--hip_hubert needs --learned_frontend --hip_units (its features feed the unit quantiser)")
            duration = torch.full((1, Lu), 3.0, device=device)
        if args.hip_wavlm:
            # finetune.py:113-117: spk_emb is the embedder's output for the reference utterance at 16 kHz over its norm: WavLM-large, every
            # hidden state into the ECAPA-TDNN.  Here both at the reference's sizes with seeded weights on a seeded waveform.
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
            from wavlm_torch import large_config, synthetic_wavlm_state_dict
            from unitspeech_amd.mel import synthetic_waveform
            from unitspeech_amd.speaker_encoder import ECAPA_TDNN_SMALL, synthetic_ecapa_state_dict
            from unitspeech_amd.wavlm import WavLMModel
            if not 0 <= args.wavlm_layers <= 24:
                raise SystemExit("--wavlm_layers must be between 0 and 24")
            n16 = 400 + 320 * (L * 256 // 320 - 1)
            if args.hip_resample:
                from unitspeech_amd.resample import Resample
                n22 = -(-n16 * 441 // 320)
                wav16 = Resample(SAMPLING_RATE, 16000).to(device)(torch.from_numpy(synthetic_waveform(n22, args.ID & 0xffff, SAMPLING_RATE)).to(device))[:n16]
            else:
                wav16 = torch.from_numpy(synthetic_waveform(n16, args.ID & 0xffff, 16000)).to(device)
            wcfg = dict(large_config(), num_hidden_layers=args.wavlm_layers)
            wavlm = WavLMModel(**wcfg)
            wavlm.load_state_dict(synthetic_wavlm_state_dict(wcfg, args.ID & 0xffff, device=device), assign=True)      # drawn on the device: no 1.2 GB upload
            spk_embedder = ECAPA_TDNN_SMALL(feat_dim=1024, emb_dim=cfg.spk_emb_dim, feat_type="wavlm_large", feat_num=args.wavlm_layers + 1)
            spk_embedder.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(spk_embedder.config(), 0).items()})
            spk_embedder = spk_embedder.eval().attach_upstream(wavlm.eval(), normalize=True).to(device)
            spk_emb = spk_embedder.embed_wav(wav16.reshape(1, -1)).reshape(1, 1, -1)
            print(f"hip wavlm: {wav16.numel()} samples at 16 kHz -> {args.wavlm_layers + 1} hidden states of {wavlm.frames(wav16.numel())} x 1024 -> "
                  f"spk_emb {spk_emb.shape[-1]}")
        elif args.hip_speaker_encoder:
            # finetune.py:106-110: spk_emb is the ECAPA-TDNN's embedding of the reference utterance over its norm; here the HIP module
            # at the reference's sizes (WavLM-large: 25 hidden states of 1024) with seeded weights on 3 s of seeded hidden states
            from unitspeech_amd.speaker_encoder import synthetic_speaker_embedder, synthetic_hidden_states
            spk_embedder = synthetic_speaker_embedder(cfg.spk_emb_dim).to(device)
            hidden = torch.from_numpy(synthetic_hidden_states(25, 1, 149, 1024, args.ID & 0xffff)).to(device)
            spk_emb = spk_embedder.embed(hidden).reshape(1, 1, -1)
        else:
            spk = torch.from_numpy(g.standard_normal((1, 1, cfg.spk_emb_dim), dtype=np.float32)).to(device)
            spk_emb = spk / spk.norm()
        mel_min, mel_max = torch.tensor(-11.5), torch.tensor(2.0)
    elif args.hip_wavlm:
        raise SystemExit("--hip_wavlm needs --synthetic (or --features with `wav` and --speaker_encoder_path)")
    elif args.hip_mel:
        raise SystemExit("--hip_mel needs --synthetic (with --features, put `wav` in the file)")
    else:
        if not args.reference_root:
            raise SystemExit("give --features (the pre-step tensors), --reference_root (reference checkout with its checkpoints) or use --synthetic")
        raise SystemExit("running the pre-steps here needs the reference's WavLM/ECAPA speaker embedder, mHuBERT unit extractor and unit "
                         "encoder checkpoints (finetune.py:47-128), none of which are available offline; run the pre-steps with the "
                         "reference, save their tensors and pass the file with --features (the unit extractor itself runs here: `wav` with "
                         "--hubert_checkpoint and --kmeans_checkpoint)")
    decoder = decoder.to(device).train()
    # finetune.py:81 uses torch.optim.Adam; FusedAdam is the same update (clip + Adam) in three HIP launches
    opt = (torch.optim.Adam if args.torch_optimizer else FusedAdam)(decoder.parameters(), lr=args.learning_rate)
    mel_lengths = torch.LongTensor([mel.shape[-1]]).to(device)
    mel_mask = sequence_mask(mel_lengths, mel.shape[-1]).unsqueeze(1).to(mel.dtype)
    x_mask = torch.ones(1, 1, cond_x.shape[-1], device=device)
    attn = generate_path(duration, (x_mask.unsqueeze(-1) * mel_mask.unsqueeze(2)).squeeze(1))

    def probe():
        """--report_memory: the diffusion loss of the utterance's first segment at 8 FIXED (t, z) draws, outside the training run's random stream:
        the same probe before and after the adaptation says whether it made progress (single iterations' losses vary 5x with their t)."""
        cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(device)
        was_training = decoder.training
        decoder.eval()
        seg_mask = torch.ones(1, 1, segment, device=device)
        a0 = attn[:, :, :segment]
        cond_y = torch.matmul(a0.transpose(1, 2), cond_x.transpose(1, 2)).transpose(1, 2)          # unitspeech.py:484-486 for a crop at offset 0
        tot = 0.0
        with torch.no_grad():
            for k in range(8):
                torch.manual_seed(4321 + k)
                loss, _ = decoder.compute_loss(mel[:, :, :segment], seg_mask, cond_y, spk_emb=spk_emb)
                tot += float(loss)
        decoder.train(was_training)
        torch.set_rng_state(cpu_state)
        torch.cuda.set_rng_state(dev_state, device)
        return tot / 8

    if args.report_memory:
        print(f"probe loss before {probe():.5f}")
    graph = None
    if not args.no_graph:
        from unitspeech_amd.graph import FineTuneGraph
        graph = FineTuneGraph(decoder, spk_emb, mel.shape[0], segment, cfg.n_feats)    # forward + backward of an iteration as one HIP graph
    t0 = time.perf_counter()
    for it in range(args.n_iters):                                                           # finetune.py:131-165
        if graph is not None:
            loss = graph.step(cond_x, mel, mel_lengths, attn)
        else:
            loss = decoder.fine_tune(cond_x, mel, mel_mask, mel_lengths, mel.shape[-1], attn, spk_emb, segment, cfg.n_feats)
            opt.zero_grad(set_to_none=True)
            loss.backward()
        if args.torch_optimizer:
            torch.nn.utils.clip_grad_norm_(decoder.parameters(), 1)
            opt.step()
        else:
            opt.step(max_norm=1)
        if it % 50 == 0 or it == args.n_iters - 1:
            print(f"iter {it:4d}  diffusion loss {loss.item():.5f}")
            if args.report_memory:
                print(f"          allocated {torch.cuda.memory_allocated(device) >> 20} MiB")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.n_iters} iterations in {dt:.2f} s ({1e3 * dt / max(args.n_iters, 1):.1f} ms/iter)")
    if args.report_memory:
        print(f"range status {decoder.range_status()}")
        print(f"probe loss after {probe():.5f}")
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, f"{args.ID}.pt")
    save_finetuned_checkpoint(path, decoder, spk_emb, mel_min, mel_max, base=base)           # finetune.py:167-173
    print(f"saved {path}")


if __name__ == "__main__":
    main()
