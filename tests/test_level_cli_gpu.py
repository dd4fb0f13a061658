"""The command lines of the level normalisation on the device: normalize_level.py on its seeded inputs and synthesize_batch.py --sv56
against the yardstick tools/level_numpy.py applied to the very samples the tools read or wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import level_numpy as L  # noqa: E402

pytestmark = pytest.mark.gpu


def decidable(x, rate, ndb, what):
    """The yardstick's output for int16 samples x, after asserting that rounding noise cannot change it."""
    lv = L.active_speech_level(x, rate)
    m = L.threshold_margin(L.envelope(L.to_full_scale(x), rate))
    assert m >= 1e-9, f"{what}: q comes within {m:.2e} of a threshold"
    f = L.gain_factor(lv.level_db, ndb)
    m = L.tie_margin(L.scaled_lsb(x, f))
    assert f == 1.0 or m >= 1e-6, f"{what}: a value lies {m:.2e} LSB from a rounding tie"
    return L.round_saturate(L.scaled_lsb(x, f))[0], lv, f


def test_normalize_level_tool(tmp_path):
    from scipy.io import wavfile
    import normalize_level as N
    out = tmp_path / "norm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "normalize_level.py"), "--synthetic", "4", "--batch", "3", "--out_dir", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    items = N.synthetic_items(4, 0)
    assert sorted(os.listdir(out)) == sorted(f"{n}.wav" for n, _, _ in items)
    assert len({len(x) for _, x, _ in items}) == 4
    for name, x, rate in items:
        want, lv, f = decidable(x, rate, -26.0, name)
        sr, got = wavfile.read(str(out / f"{name}.wav"))
        assert sr == rate and got.dtype == np.int16 and np.array_equal(got, want), name
        assert lv.level_db > -100.0 and f"{name}: level {lv.level_db:.2f} dB, gain {f:.4f}, " in r.stdout


def test_synthesize_batch_sv56(tmp_path):
    from scipy.io import wavfile
    import synthesize_batch as S
    base = [sys.executable, os.path.join(ROOT, "synthesize_batch.py"), "--synthetic", "3", "--batch", "2", "--diffusion_steps", "2"]
    plain, norm = tmp_path / "plain", tmp_path / "norm"
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    names = [n for n, _ in S.synthetic_texts(3, 0)]
    assert sorted(os.listdir(plain)) == sorted(f"{n}.wav" for n in names)                  # without the flags: today's files
    r = subprocess.run(base + ["--sv56", "--keep_raw", "--out", str(norm)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(norm)) == sorted([f"{n}.wav" for n in names] + [f"{n}.raw.wav" for n in names])
    for name in names:
        sr0, x = wavfile.read(str(plain / f"{name}.wav"))
        sr1, raw = wavfile.read(str(norm / f"{name}.raw.wav"))
        sr2, got = wavfile.read(str(norm / f"{name}.wav"))
        assert sr0 == sr1 == sr2 == 22050 and x.dtype == np.float32 and raw.dtype == got.dtype == np.int16
        assert np.array_equal(raw, (x * 32767).astype(np.int16)), name                      # the reference's route from the float waveform
        want, lv, f = decidable(raw, 22050, -26.0, name)
        print(f"{name}: level {lv.level_db} factor {f}")
        assert np.array_equal(got, want), name
        if lv.level_db == -100.0:
            assert np.array_equal(got, raw)
