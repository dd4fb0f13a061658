#!/usr/bin/env python3
"""Speaker embeddings of a whole dataset on the HIP library: the reference's preprocessing/process_spkr_embs.py and
process_uncond_spk.py in one pass, with the utterances embedded in ragged batches instead of one at a time.

    python extract_speaker_embeddings.py --filelist LIST --speaker_encoder_path EMBEDDER.pt --out DIR [--batch 32]
                                         [--max_padded_samples 5120000]
    python extract_speaker_embeddings.py --synthetic 12 --speakers 3 --batch 4 --out DIR

LIST holds one `path|text|speaker` line per utterance.  A path names what finetune.py --features reads: a `.pt` (torch.save of a dict)
or `.npz` file with `wav` ([T] or [1, T]) and, unless it is 22050 Hz, `wav_sampling_rate`.  Each utterance is resampled to 16 kHz
(`unitspeech_amd.resample.Resample`), the utterances are sorted by length and cut into batches (`plan_batches`), and each batch goes
through `ECAPA_TDNN.forward(wav, lengths)` of `load_speaker_embedder_checkpoint` (WavLM, then the ECAPA-TDNN trunk, both with per-item
lengths: an utterance's embedding has the bits it has when it is embedded alone, whatever it is batched with).

Written to DIR: `<speaker>.pt`, the mean embedding [1, emb_dim] of the speaker's utterances, unnormalised as in the reference, and
`spk_uncond.pt` [1, 1, emb_dim], the mean of those means (speakers in the order of their first line).  A speaker's mean is
`torch.stack(rows in file-list order).mean(0)` in fp32; the reference keeps a running mean `(m * n + e) / (n + 1)`, which differs from it
by rounding only.

--synthetic N runs without files or checkpoints: N seeded 22050 Hz waveforms of seeded ragged lengths over --speakers speakers, through a
seeded tiny WavLM (large form) and trunk.
"""
from __future__ import annotations

import argparse
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.audio import load_tensor_file, to_16k  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402

MIN_SAMPLES_16K = 400            # the receptive field of the wav2vec2-family feature extractor: one frame
SYNTHETIC_RATE = 22050
# the tiny upstream (WavLM, large form) and trunk of --synthetic
TINY_WAVLM = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
                  intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
                  num_buckets=32, max_bucket_distance=40, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
TINY_TRUNK = dict(feat_dim=40, channels=16, emb_dim=8, global_context_att=False, n_layers=3)


def parse_filelist(text: str):
    """`path|text|speaker` lines -> [(path, text, speaker)] in file order (unitspeech/util.py:49 `parse_filelist`; blank lines are
    skipped, and a text that itself holds `|` stays whole: the path is the first field and the speaker the last)."""
    out = []
    for no, line in enumerate(text.splitlines(), start=1):
        line = line.strip()
        if not line:
            continue
        parts = line.split("|")
        if len(parts) < 3 or not parts[0] or not parts[-1]:
            raise ValueError(f"file list line {no}: expected `path|text|speaker`, got {line!r}")
        out.append((parts[0], "|".join(parts[1:-1]), parts[-1]))
    return out


def speaker_means(rows, speakers):
    """rows[i]: the embedding [emb_dim] of utterance i, speakers[i] its speaker -> (OrderedDict speaker -> mean [1, emb_dim] over the
    speaker's rows in file order, speakers in the order of their first utterance; spk_uncond [1, 1, emb_dim], the mean of the means)."""
    by = OrderedDict()
    for r, s in zip(rows, speakers):
        by.setdefault(s, []).append(r.float())
    means = OrderedDict((s, torch.stack(v).mean(0).unsqueeze(0)) for s, v in by.items())
    uncond = torch.stack(list(means.values()), dim=0).mean(dim=0, keepdim=True)          # process_uncond_spk.py:37-40
    return means, uncond


def running_mean(rows):
    """The reference's update (process_spkr_embs.py:90-95) over the same rows, [1, emb_dim]."""
    m = None
    for n, e in enumerate(rows):
        e = e.float().unsqueeze(0)
        m = e if m is None else (m * n + e) / (n + 1)
    return m


def synthetic_dataset(n: int, speakers: int, seed: int = 0):
    """-> [(name, speaker, waveform [T] at SYNTHETIC_RATE)]: seeded lengths between 0.4 and 1.6 s, speakers dealt in blocks as the
    reference's lists have them."""
    from unitspeech_amd.mel import synthetic_waveform
    if n < 1 or speakers < 1 or speakers > n:
        raise ValueError("--synthetic N --speakers S: 1 <= S <= N")
    g = np.random.Generator(np.random.Philox(key=7000 + seed))
    lens = g.integers(int(0.4 * SYNTHETIC_RATE), int(1.6 * SYNTHETIC_RATE), size=n)
    return [(f"synthetic_{i:04d}", f"spk{i * speakers // n}", torch.from_numpy(synthetic_waveform(int(lens[i]), seed * 1000 + i, SYNTHETIC_RATE)))
            for i in range(n)]


def synthetic_embedder(device, seed: int = 0):
    """The seeded tiny WavLM (large form) with the seeded tiny trunk behind it, on `device`, eval mode."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from wavlm_torch import synthetic_wavlm_state_dict
    from unitspeech_amd.speaker_encoder import ECAPA_TDNN, synthetic_ecapa_state_dict
    from unitspeech_amd.wavlm import WavLMModel
    t = TINY_TRUNK
    trunk = ECAPA_TDNN(feat_dim=t["feat_dim"], channels=t["channels"], emb_dim=t["emb_dim"], global_context_att=t["global_context_att"],
                       feat_type="wavlm_large", feat_num=t["n_layers"])
    trunk.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(t, seed).items()})
    wavlm = WavLMModel(**TINY_WAVLM)
    wavlm.load_state_dict(synthetic_wavlm_state_dict(TINY_WAVLM, seed))
    return trunk.attach_upstream(wavlm, normalize=True).to(device).eval()


def load_utterance(path: str):
    """-> (waveform [T] fp32 on the host, sampling rate) from a `.pt` / `.npz` file with `wav` and optionally `wav_sampling_rate`."""
    d = load_tensor_file(path)
    if not isinstance(d, dict) or "wav" not in d:
        raise SystemExit(f"{path}: expected a dict with `wav` (and `wav_sampling_rate` unless it is {SYNTHETIC_RATE} Hz)")
    wav = torch.as_tensor(d["wav"]).float()
    if wav.dim() not in (1, 2) or (wav.dim() == 2 and wav.shape[0] != 1):
        raise SystemExit(f"{path}: wav must be [T] or [1, T], got {tuple(wav.shape)}")
    return wav.reshape(-1), int(d["wav_sampling_rate"]) if "wav_sampling_rate" in d else SYNTHETIC_RATE


@torch.no_grad()
def embed_all(embedder, wavs16, max_batch, max_padded_samples):
    """wavs16: 16 kHz waveforms [T_i] on the device -> their embeddings [emb_dim], on the host, in the order given."""
    lens = [int(w.shape[0]) for w in wavs16]
    rows = [None] * len(wavs16)
    batches = plan_batches(lens, max_batch, max_padded_samples)
    for idx in batches:
        x, n = pad_batch([wavs16[i] for i in idx])
        emb = embedder(x, n).cpu()
        for b, i in enumerate(idx):
            rows[i] = emb[b]
    return rows, batches


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--filelist", default=None, help="`path|text|speaker` lines")
    ap.add_argument("--speaker_encoder_path", default=None, help="the whole embedder's checkpoint ({'model': state_dict} with feature_extract.*)")
    ap.add_argument("--out", required=True, help="directory for <speaker>.pt and spk_uncond.pt")
    ap.add_argument("--batch", type=int, default=32, help="most utterances in one call")
    ap.add_argument("--max_padded_samples", type=int, default=32 * 160000, help="most 16 kHz samples in one padded batch (items x longest)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded waveforms through a seeded tiny embedder")
    ap.add_argument("--speakers", type=int, default=3, help="--synthetic: number of speakers")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP speaker embedder has no CPU fallback")
    device = torch.device(args.device)
    if args.synthetic:
        items = [(name, spk, wav, SYNTHETIC_RATE) for name, spk, wav in synthetic_dataset(args.synthetic, args.speakers, args.seed)]
        embedder = synthetic_embedder(device, args.seed)
    else:
        if not args.filelist or not args.speaker_encoder_path:
            raise SystemExit("give --filelist and --speaker_encoder_path, or --synthetic N")
        from unitspeech_amd.speaker_encoder import load_speaker_embedder_checkpoint
        with open(args.filelist, encoding="utf-8") as f:
            entries = parse_filelist(f.read())
        if not entries:
            raise SystemExit(f"{args.filelist}: no utterances")
        items = [(path, spk) + load_utterance(path) for path, _, spk in entries]
        embedder = load_speaker_embedder_checkpoint(args.speaker_encoder_path, device)
    resamplers, wavs16 = {}, []
    for name, _, wav, rate in items:
        w = to_16k(wav, rate, device, resamplers)
        if w.shape[0] < MIN_SAMPLES_16K:
            raise SystemExit(f"{name}: {w.shape[0]} samples at 16 kHz are fewer than the upstream's receptive field ({MIN_SAMPLES_16K})")
        wavs16.append(w)
    rows, batches = embed_all(embedder, wavs16, args.batch, args.max_padded_samples)
    means, uncond = speaker_means(rows, [spk for _, spk, _, _ in items])
    os.makedirs(args.out, exist_ok=True)
    for spk, m in means.items():
        torch.save(m, os.path.join(args.out, f"{spk}.pt"))
    torch.save(uncond, os.path.join(args.out, "spk_uncond.pt"))
    padded = sum(len(b) * max(int(wavs16[i].shape[0]) for i in b) for b in batches)
    print(f"{len(items)} utterances in {len(batches)} batches ({sum(int(w.shape[0]) for w in wavs16)} samples, {padded} padded), "
          f"{len(means)} speakers -> {args.out}")


if __name__ == "__main__":
    main()
