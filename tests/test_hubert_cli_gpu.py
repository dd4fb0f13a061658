"""`finetune.py --hip_hubert`: the synthetic adaptation run with the dense features taken from the HIP HuBERT encoder (seeded base-size weights)
on a seeded 22050 Hz waveform that the HIP resampler brings to 16 kHz, feeding the unit quantiser, process_unit and the unit encoder."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_finetune_cli_with_the_hip_hubert(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--learned_frontend", "--hip_units", "--hip_hubert",
                        "--hip_resample", "--n_iters", "3", "--ID", "5", "--out_dir", str(tmp_path)], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hip hubert: 153680 samples at 16 kHz -> 480 frames of 768 (layer 11)" in r.stdout
    assert "hip units: 480 dense frames -> " in r.stdout
    losses = [float(line.split()[-1]) for line in r.stdout.splitlines() if line.startswith("iter ")]
    assert len(losses) >= 1 and all(np.isfinite(losses))


def test_hip_hubert_needs_the_unit_leg(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--hip_hubert", "--n_iters", "1", "--out_dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--hip_hubert needs" in r.stderr
