"""The yardstick of the active speech level (tools/level_numpy.py: ITU-T P.56 method B in fp64 numpy) against the ITU loop as written and
against closed-form cases, and the wiring of the new calls.  No device work is launched here."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import level_numpy as L  # noqa: E402

from unitspeech_amd import _build, _lib  # noqa: E402

SYMBOLS = ["us_level_chunk", "us_level_workspace_bytes", "us_level_measure", "us_level_apply"]


@pytest.mark.parametrize("rate", [8000, 16000, 48000])
def test_vectorised_counts_equal_the_sequential_loop(rate):
    g, hang = L.constants(rate)
    assert hang == {8000: 1600, 16000: 3200, 48000: 9600}[rate] and g == math.exp(-1.0 / (rate * 0.03))
    x = L.burst_signal(3 * hang + 6 * 4096 + 17, rate, seed=rate // 1000)
    q = L.envelope(L.to_full_scale(x), rate)
    a = L.activity_counts(q, hang)
    assert np.array_equal(a, L.activity_counts_loop(q, hang))
    assert a[0] > 0 and np.all(np.diff(a) <= 0)                # the signal reaches thresholds, and they are nested


@pytest.mark.parametrize("amp", [0.5, 0.05])
def test_sine_level(amp):
    rate = 16000
    x = amp * np.sin(2 * np.pi * 440.0 * np.arange(3 * rate) / rate)
    lv = L.active_speech_level(x, rate)
    assert abs(lv.level_db - 20 * math.log10(amp / math.sqrt(2))) <= 0.05, lv.level_db
    assert lv.activity > 0.99, lv.activity
    assert abs(lv.peak - amp) < 1e-3 * amp


def test_silence_has_no_level():
    rate = 16000
    lv = L.active_speech_level(np.zeros(rate), rate)
    assert lv.level_db == -100.0 and lv.activity == 0.0 and not lv.counts.any()
    x = 1e-5 * np.sin(2 * np.pi * 300.0 * np.arange(rate) / rate)            # the envelope stays below 2^-15 = 3.05e-5
    assert L.envelope(x, rate).max() < 2.0 ** -15
    lv = L.active_speech_level(x, rate)
    assert lv.level_db == -100.0 and lv.activity == 0.0 and not lv.counts.any()
    assert L.gain_factor(lv.level_db, -26.0) == 1.0
    lv = L.active_speech_level(np.zeros(0), rate)
    assert lv.level_db == -100.0 and lv.activity == 0.0


def test_shift_law():
    rate = 16000
    x = L.to_full_scale(L.burst_signal(30000, rate, seed=3)) * 0.5
    a, b = L.active_speech_level(x, rate), L.active_speech_level(2.0 * x, rate)
    assert np.array_equal(b.counts[1:], a.counts[:-1])         # a_j(2x) = a_{j-1}(x): doubling is exact in floating point
    assert a.counts[0] > a.counts[3] > 0
    assert abs((b.level_db - a.level_db) - 20 * math.log10(2.0)) <= 1e-9
    assert abs(b.activity - a.activity) <= 1e-9


def test_rounding_and_quantisation_rules():
    out, clipped = L.round_saturate(np.array([0.5, -0.5, 1.5, -1.5, 2.4999, 32767.4, 32767.5, -32768.5, -32769.0, 1e9]))
    assert out.tolist() == [1, -1, 2, -2, 2, 32767, 32767, -32768, -32768, 32767] and clipped == 4
    q = L.quantize_reference(np.array([0.99999, -0.99999, 1.0, -1.0, 0.5, -0.00002, 0.00004], dtype=np.float32))
    assert q.tolist() == [32766, -32766, 32767, -32767, 16383, 0, 1]
    x = L.burst_signal(9000, 16000, seed=1)
    y = L.sv56(x, 16000, -26.0)
    assert y.dtype == np.int16 and y.shape == x.shape
    f = L.gain_factor(L.active_speech_level(x, 16000).level_db, -26.0)
    assert f != 1.0 and np.abs(y.astype(np.float64) - x.astype(np.float64) * f).max() <= 0.5


def test_wiring():
    from unitspeech_amd import level
    txt = open(os.path.join(ROOT, "include", "unitspeech_hip.h")).read()
    declared = set(re.findall(r"\b(us_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES, s
    assert "level.hip" in _build.SOURCES
    assert level.__all__ == ["active_speech_level", "normalize_level", "sv56"]
    for name in level.__all__:
        assert callable(getattr(level, name))
    assert level.SpeechLevel._fields == ("level_db", "activity", "rms_db", "peak", "counts")
    assert level.LevelInfo._fields == level.SpeechLevel._fields + ("gain", "clipped")


def test_normalize_level_tool_host_side(tmp_path):
    from scipy.io import wavfile
    import normalize_level as N
    items = N.synthetic_items(4, 0)
    assert [n for n, _, _ in items] == [f"synthetic_{i:04d}" for i in range(4)] and len({len(x) for _, x, _ in items}) == 4
    assert all(x.dtype == np.int16 and r == N.SYNTHETIC_RATE and np.abs(x).max() > 1000 for _, x, r in items)
    assert np.array_equal(items[2][1], N.synthetic_items(4, 0)[2][1]) and not np.array_equal(items[2][1][:500], N.synthetic_items(4, 1)[2][1][:500])
    assert N.plan_batches([5, 3, 9, 3], 3) == [[1, 3, 0], [2]]
    with pytest.raises(ValueError):
        N.plan_batches([1], 0)
    s = items[0][1][:1000]
    wavfile.write(str(tmp_path / "a.wav"), 16000, s)
    wavfile.write(str(tmp_path / "b.wav"), 8000, (s / 32768.0).astype(np.float32))
    wavfile.write(str(tmp_path / "c.wav"), 8000, np.stack([s, s], axis=1))
    x, r = N.read_samples(str(tmp_path / "a.wav"))
    assert r == 16000 and x.dtype == np.int16 and np.array_equal(x, s)                 # int16 goes in as it is
    x, r = N.read_samples(str(tmp_path / "b.wav"))
    assert r == 8000 and x.dtype == np.float32 and np.array_equal(x, (s / 32768.0).astype(np.float32))
    x, r = N.read_samples(str(tmp_path / "c.wav"))
    assert x.dtype == np.float32 and x.shape == (1000,) and np.allclose(x, s / 32768.0)


def test_the_scripts_take_the_flags():
    for script in ("inference.py", "synthesize_batch.py", "voice_conversion.py", "evaluate.py"):
        src = open(os.path.join(ROOT, script)).read()
        assert '"--sv56"' in src and '"--ndb"' in src and "normalize_level" in src, script
    for script in ("synthesize_batch.py", "voice_conversion.py"):
        assert '"--keep_raw"' in open(os.path.join(ROOT, script)).read(), script
