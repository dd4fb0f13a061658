"""evaluate.py's MOS column on the GPU: every file's score is what `MOSPredictor` gives for that waveform alone, bit for bit, whatever
batch it was scored in; the corpus figure is their mean."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_evaluate_synthetic_mos_column(tmp_path):
    out = tmp_path / "result.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--batch", "4", "--mos", "--out", str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, encoding="utf-8") as f:
        result = json.load(f)
    corpus = json.loads(r.stdout.strip().splitlines()[-1])
    assert result["files"] == 6 and result["batches"] == 2 and all("MOS" in line for line in r.stdout.splitlines()[:6])
    import evaluate
    from unitspeech_amd.audio import to_16k
    device = torch.device("cuda:0")
    predictor = evaluate.synthetic_mos(device, 0)
    resamplers, solo = {}, {}
    for name, wav, rate in evaluate.synthetic_waves(6, 0):
        solo[name] = float(predictor(to_16k(wav, rate, device, resamplers)[None])[0])
    got = {rec["file"]: rec["mos"] for rec in result["per_file"]}
    assert got == solo                                     # the same floats: the same bits
    assert len(set(solo.values())) == 6 and all(np.isfinite(v) for v in solo.values())
    values = [rec["mos"] for rec in result["per_file"]]
    assert result["mos"] == float(np.mean(values)) and result["mos_min"] == min(values) and result["mos_max"] == max(values)
    assert corpus["mos"] == result["mos"] and corpus["mos_min"] == result["mos_min"] and corpus["mos_max"] == result["mos_max"]

