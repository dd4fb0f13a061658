"""The host side of the mel front end (no GPU): the numpy filter bank against an independent implementation, and the fp64 restatement of
the reference's `mel_spectrogram` (tools/mel_torch.py) that the GPU tests use as their yardstick."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mel_torch import mel_spectrogram_torch  # noqa: E402

from unitspeech_amd.mel import MelSpectrogram, mel_filterbank, mel_spectrogram, synthetic_waveform  # noqa: E402

REF = dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000)


def test_filterbank_matches_the_transformers_implementation():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    for sr, n_fft, n_mels, fmin, fmax in ((22050, 1024, 80, 0, 8000), (16000, 64, 8, 0, 4000), (24000, 2048, 100, 20, 12000)):
        want = audio_utils.mel_filter_bank(n_fft // 2 + 1, n_mels, fmin, fmax, sr, norm="slaney", mel_scale="slaney").T
        got = mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12


def test_filterbank_shape_and_live_bins_of_the_reference_configuration():
    fb = mel_filterbank(22050, 1024, 80, 0, 8000)
    assert fb.shape == (80, 513) and (fb >= 0).all()
    assert int(np.nonzero(fb.astype(np.float32).any(axis=0))[0].max()) == 371        # bin 371 is 7989 Hz, bin 372 is 8010 Hz > fmax
    assert (fb.sum(axis=1) > 0).all()                                                 # no empty band
    m = MelSpectrogram(**REF)
    assert tuple(m.mel_basis.shape) == (80, 513) and m.mel_basis.dtype == torch.float32 and tuple(m.window.shape) == (1024,)
    assert torch.equal(m.window, torch.hann_window(1024))


@pytest.mark.parametrize("T", [385, 1500, 256 * 64 + 100])
def test_restatement_frame_count(T):
    m = MelSpectrogram(**REF)
    y = torch.from_numpy(synthetic_waveform(T, 1))[None]
    for dtype in (torch.float64, torch.float32):
        out = mel_spectrogram_torch(y, m.mel_basis, m.window, 1024, 256, 1024, dtype=dtype)
        assert tuple(out.shape) == (1, 80, T // 256) and out.dtype == dtype and torch.isfinite(out).all()


def test_restatement_of_silence_is_the_clamp():
    """sqrt(1e-9) in every bin; the largest band sum of the filter bank times that is 1.55e-6, below the 1e-5 clamp."""
    m = MelSpectrogram(**REF)
    assert float(m.mel_basis.double().sum(dim=1).max()) * math.sqrt(1e-9) < 1e-5
    out = mel_spectrogram_torch(torch.zeros(2, 2000), m.mel_basis, m.window, 1024, 256, 1024)
    assert torch.equal(out, torch.full((2, 80, 7), math.log(1e-5), dtype=torch.float64))


def test_center_true_is_refused():
    with pytest.raises(NotImplementedError):
        mel_spectrogram(torch.zeros(1, 4096), 1024, 80, 22050, 256, 1024, 0, 8000, center=True)


def test_cpu_waveform_is_refused():
    with pytest.raises(RuntimeError, match="ROCm device"):
        MelSpectrogram(**REF)(torch.zeros(1, 4096))


def test_create_refusals_and_keys_through_the_c_abi():
    """us_mel_create touches no device: the configuration checks, the weight keys and the sizes can be read on any machine."""
    import ctypes as C
    from unitspeech_amd import _lib
    lib = _lib.load()

    def create(n_fft, hop, win, num_mels):
        h = C.c_void_p()
        c = _lib.us_mel_config(n_fft=n_fft, hop=hop, win=win, num_mels=num_mels)
        return lib.us_mel_create(C.byref(h), C.byref(c)), h
    for bad in ((1024, 300, 1024, 80), (1024, 256, 2048, 80), (8192, 256, 1024, 80), (1024, 1, 1024, 80), (1024, 256, 1024, 0), (1024, 0, 1024, 80)):
        rc, h = create(*bad)
        assert rc == -1 and not h, bad                               # US_EINVAL, no handle
    rc, h = create(1024, 256, 1024, 80)
    assert rc == 0 and h
    assert lib.us_mel_num_weights(h) == 2 and [lib.us_mel_weight_key(h, i) for i in range(3)] == [b"mel_basis", b"window", None]
    assert lib.us_mel_frames(h, 1500) == 5 and lib.us_mel_frames(h, 255) == 0
    # X [B][256][F + 3] and the magnitudes [B][513][F], padded to 64 floats each, plus the alignment slack
    assert lib.us_mel_workspace_bytes(h, 2, 1500) == (2 * 256 * 8 + 5184) * 4 + 256
    assert lib.us_mel_destroy(h) == 0
