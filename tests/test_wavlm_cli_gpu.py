"""`finetune.py --hip_wavlm`: the synthetic adaptation run with the speaker embedding taken from the HIP WavLM-large (seeded weights, drawn on
the device) in front of the seeded HIP ECAPA-TDNN, on a seeded 22050 Hz waveform that the HIP resampler brings to 16 kHz."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_finetune_cli_with_the_hip_wavlm(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--hip_wavlm", "--hip_resample", "--n_iters", "3", "--ID", "5",
                        "--out_dir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hip wavlm: 153680 samples at 16 kHz -> 25 hidden states of 480 x 1024 -> spk_emb 256" in r.stdout
    losses = [float(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith("iter ")]
    assert len(losses) >= 1 and all(np.isfinite(losses))


def test_hip_wavlm_needs_a_source(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--hip_wavlm", "--n_iters", "1", "--out_dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--hip_wavlm needs" in r.stderr


def test_features_file_with_a_waveform_and_the_embedder_checkpoint(tmp_path):
    """`--features` holding `wav` with --hip_wavlm --speaker_encoder_path: spk_emb is the loaded embedder's embed_wav of the waveform at 16 kHz"""
    import argparse

    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import finetune
    from wavlm_torch import synthetic_wavlm_state_dict
    from unitspeech_amd import DecoderConfig
    from unitspeech_amd.mel import synthetic_waveform
    from unitspeech_amd.resample import Resample
    from unitspeech_amd.speaker_encoder import load_speaker_embedder_checkpoint, synthetic_ecapa_state_dict
    cfg, device = DecoderConfig(), torch.device("cuda", 0)
    wcfg = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
                intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
                num_buckets=320, max_bucket_distance=800, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
    ck = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(dict(feat_dim=40, channels=16, emb_dim=cfg.spk_emb_dim, global_context_att=False,
                                                                             n_layers=3), 4).items()}
    ck.update({"feature_extract.model." + k: v for k, v in synthetic_wavlm_state_dict(wcfg, 9, masked_spec_embed=False).items()})     # HF's names pass the mapping unchanged
    path = str(tmp_path / "embedder.pt")
    torch.save({"model": ck}, path)
    wav = torch.from_numpy(synthetic_waveform(256 * 90 + 40, 3))
    feats = {"wav": wav, "wav_sampling_rate": 22050, "cond_x": torch.zeros(1, 80, 30), "duration": torch.full((1, 30), 3.0),
             "mel_min": torch.tensor(-11.3), "mel_max": torch.tensor(1.9)}
    args = argparse.Namespace(kmeans_checkpoint=None, speaker_encoder_checkpoint=None, unit_encoder_checkpoint=None, hip_wavlm=True,
                              speaker_encoder_path=path, features=str(tmp_path / "features.pt"))
    torch.save(feats, args.features)
    _, _, _, spk, _, _ = finetune.load_features(args, cfg, None, device)
    wav16 = Resample(22050, 16000).to(device)(wav[None].to(device))
    want = load_speaker_embedder_checkpoint(path, device).embed_wav(wav16)
    assert tuple(spk.shape) == (1, 1, cfg.spk_emb_dim) and torch.equal(spk.reshape(1, -1), want) and abs(float(spk.norm()) - 1.0) < 1e-5
    # without the checkpoint the flag is refused with a message
    args.speaker_encoder_path = None
    with pytest.raises(SystemExit, match="--hip_wavlm needs"):
        finetune.load_features(args, cfg, None, device)
