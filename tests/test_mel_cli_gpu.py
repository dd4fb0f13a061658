"""finetune.py with the HIP mel front end (GPU): `--synthetic --hip_mel` end to end, and a `--features` file that carries the waveform."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_finetune_cli_with_the_hip_mel(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--hip_mel", "--n_iters", "3", "--ID", "5", "--out_dir",
                        str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hip mel: 153600 samples -> 600 frames" in r.stdout
    losses = [float(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith("iter ")]
    assert len(losses) == 2 and all(np.isfinite(losses))
    ck = torch.load(tmp_path / "5.pt", map_location="cpu")
    assert set(ck) == {"model", "spk_emb", "mel_min", "mel_max"} and all(torch.isfinite(v).all() for v in ck["model"].values())
    # without --synthetic the flag is refused with a message
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--hip_mel", "--out_dir", str(tmp_path)], capture_output=True, text=True,
                        timeout=300, cwd=ROOT)
    assert r2.returncode != 0 and "--hip_mel needs --synthetic" in r2.stderr and "Traceback" not in r2.stderr


def test_features_file_with_a_waveform_yields_the_modules_mel(tmp_path):
    import finetune
    from unitspeech_amd import DecoderConfig
    from unitspeech_amd.mel import MelSpectrogram, synthetic_waveform
    cfg, device = DecoderConfig(), torch.device("cuda", 0)
    wav = torch.from_numpy(synthetic_waveform(256 * 90 + 40, 3))
    mel_min, mel_max = torch.tensor(-11.3), torch.tensor(1.9)
    feats = {"wav": wav, "wav_sampling_rate": 22050, "cond_x": torch.zeros(1, 80, 30), "duration": torch.full((1, 30), 3.0),
             "spk_emb": torch.ones(1, 256), "mel_min": mel_min, "mel_max": mel_max}
    args = argparse.Namespace(kmeans_checkpoint=None, speaker_encoder_checkpoint=None, unit_encoder_checkpoint=None)
    want = MelSpectrogram(1024, 80, 22050, 256, 1024, 0, 8000).to(device)(wav.to(device), mel_min=mel_min, mel_max=mel_max)
    assert tuple(want.shape) == (1, 80, 90) and float(want.min()) >= -1.01 and float(want.max()) <= 1.01
    for name, w in (("flat", wav), ("row", wav[None])):
        args.features = str(tmp_path / f"{name}.pt")
        torch.save({**feats, "wav": w}, args.features)
        mel, cond_x, duration, spk, mn, mx = finetune.load_features(args, cfg, None, device)
        assert mel.device.type == "cuda" and torch.equal(mel, want) and float(mn) == float(mel_min) and float(mx) == float(mel_max)
    # a waveform at another rate is refused with a message: the library has no resampler
    args.features = str(tmp_path / "rate.pt")
    torch.save({**feats, "wav_sampling_rate": 16000}, args.features)
    with pytest.raises(SystemExit, match="16000 Hz"):
        finetune.load_features(args, cfg, None, device)
    # neither mel nor wav
    args.features = str(tmp_path / "none.pt")
    torch.save({k: v for k, v in feats.items() if k != "wav"}, args.features)
    with pytest.raises(SystemExit, match="missing `mel`"):
        finetune.load_features(args, cfg, None, device)
