"""BigVGAN vocoder on the HIP library (GPU): the reference goldens (large config included), both weight-norm forms, batch and run
determinism, edge lengths against the torch restatement, and the inference.py --hip_vocoder command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vocoder_torch import bigvgan_forward  # noqa: E402

from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BigVGAN, synthetic_bigvgan_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(cfg, seed, remove=False):
    m = BigVGAN(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(cfg, seed).items()})
    m = m.to(DEV).eval()
    if remove:
        m.remove_weight_norm()
    return m


@pytest.mark.parametrize("name", ["vocoder_tiny", "vocoder_base", "vocoder_large"])
def test_hip_vocoder_matches_the_reference_golden(golden, name):
    g = golden(name)
    cfg = json.loads(str(g["config"]))
    out = _model(cfg, int(g["seed"]))(torch.from_numpy(g["mel"]).to(DEV)).cpu().numpy()
    assert out.shape == g["wav64"].shape and np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - g["wav64"]).max())
    tol = max(1e-4, 10 * float(np.abs(g["wav32"] - g["wav64"]).max()))
    print(f"\n{name}: max|HIP - fp64 reference| = {err:.2e} (fp32 reference {np.abs(g['wav32'] - g['wav64']).max():.2e}, tolerance {tol:.1e})")
    assert err <= tol


def test_weight_norm_form_and_removed_form_give_bit_identical_output(golden):
    g = golden("vocoder_base")
    cfg = json.loads(str(g["config"]))
    mel = torch.from_numpy(g["mel"]).to(DEV)
    a = _model(cfg, 1)(mel)
    b = _model(cfg, 1, remove=True)(mel)
    assert torch.equal(a, b)


def test_batch_items_and_repeated_runs_are_bit_identical(golden):
    g = golden("vocoder_large")
    cfg = json.loads(str(g["config"]))
    m = _model(cfg, 2)
    gen = torch.Generator().manual_seed(5)
    mel = (torch.randn(3, 80, 29, generator=gen) * 2 - 5).to(DEV)
    batch = m(mel)
    assert torch.equal(batch, m(mel))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], m(mel[i:i + 1].contiguous()))


@pytest.mark.parametrize("cfg,T", [("tiny", 1), ("tiny", 37), ("tiny", 129), ("large", 1), ("large", 37)])
def test_edge_lengths_match_the_torch_restatement(golden, cfg, T):
    """T = 129 puts exactly one step of conv_pre and of the first up-sampler into a second 128-step tile of the convolution's loader."""
    c = json.loads(str(golden("vocoder_" + cfg)["config"])) if cfg == "tiny" else BIGVGAN_22KHZ_80BAND
    sd = {k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(c, 3).items()}
    gen = torch.Generator().manual_seed(T)
    mel = (torch.randn(2, c["num_mels"], T, generator=gen) * 2 - 5).to(DEV)
    out = _model(c, 3)(mel)
    with torch.no_grad():
        ref = bigvgan_forward(c, sd, mel.double())
    assert out.shape == ref.shape == (2, 1, T * int(np.prod(c["upsample_rates"])))
    err = float((out.double() - ref).abs().max())
    print(f"\n{cfg} T={T}: max|HIP - fp64 torch restatement| = {err:.2e}")
    assert err <= 1e-4


def test_inference_cli_hip_vocoder_writes_the_wav(tmp_path):
    from scipy.io import wavfile
    out = tmp_path / "sample.wav"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--synthetic", "--hip_vocoder", "--text", "buna ziua",
                        "--diffusion_steps", "4", "--generated_sample_path", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    mel = np.load(str(out)[:-4] + ".mel.npy")
    sr, wav = wavfile.read(str(out))
    assert sr == 22050 and wav.dtype == np.float32
    assert wav.shape == (256 * mel.shape[1],) and np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    want = _model(BIGVGAN_22KHZ_80BAND, 0)(torch.from_numpy(mel)[None].to(DEV)).cpu().numpy().reshape(-1)
    assert np.array_equal(wav, want)
