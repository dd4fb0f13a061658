"""Mel-spectrogram front end on the HIP library: waveform -> (normalised) log-mel, the tensor every training and fine-tuning path of the
reference starts from.

Drop-in for the reference's `unitspeech/vocoder/meldataset.py:51-74` `mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size,
win_size, fmin, fmax, center=False)` with the normalisation of `finetune.py:104` folded in on request.  The filter bank is the Slaney-scale,
Slaney-normalised one `librosa.filters.mel` returns, computed here in numpy (librosa is not needed); the arithmetic is `csrc/mel.hip`.
There is no CPU fallback: waveforms must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._args import c_lengths, host_lengths
from ._handle import HandleModule


def _hz_to_mel(f):
    """Slaney's auditory-toolbox scale: linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> np.ndarray:
    """`librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=)` with its defaults (htk=False, norm="slaney") in fp64:
    [n_mels, n_fft // 2 + 1] triangles on the Slaney mel scale, each divided by half its width in Hz."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    bins = 1 + n_fft // 2
    fft_freqs = np.arange(bins, dtype=np.float64) * (float(sr) / n_fft)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin)), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


class MelSpectrogram(HandleModule):
    """`forward(wav [B, T] or [T], lengths=None, mel_min=None, mel_max=None, pad_value=0.0)` -> [B, num_mels, T // hop_size].

    `lengths` (host integers) are the samples of each item: an item's frames are computed from its own samples only (reflection at its
    own end), and the frames past its `length // hop_size` are `pad_value`.  With `mel_min` / `mel_max` (a scalar or one value per band)
    the output is `(m - mel_min) / (mel_max - mel_min) * 2 - 1`.  The buffers `mel_basis` and `window` are what the library computes with."""
    _abi, _what = "mel", "mel-spectrogram front end"
    _cache_sources = True

    def __init__(self, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000):
        super().__init__()
        self.n_fft, self.num_mels, self.sampling_rate = int(n_fft), int(num_mels), int(sampling_rate)
        self.hop_size, self.win_size, self.fmin, self.fmax = int(hop_size), int(win_size), fmin, fmax
        basis = mel_filterbank(sampling_rate, self.n_fft, self.num_mels, fmin, fmax)
        self.register_buffer("mel_basis", torch.from_numpy(basis).float())              # meldataset.py:59-60
        self.register_buffer("window", torch.hann_window(self.win_size))                # :61

    def _sources(self):
        return OrderedDict((k, ((getattr(self, k),), None)) for k in ("mel_basis", "window"))

    def _create(self, lib, device):
        c = _lib.us_mel_config()
        c.n_fft, c.hop, c.win, c.num_mels = self.n_fft, self.hop_size, self.win_size, self.num_mels
        _lib.check(lib.us_mel_create(C.byref(self._h), C.byref(c)), None, "us_mel_create")

    def _range(self, v, device, name):
        if not isinstance(v, torch.Tensor):
            v = torch.tensor(v, dtype=torch.float32)
        v = v.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        if v.numel() not in (1, self.num_mels):
            raise ValueError(f"MelSpectrogram: {name} must be a scalar or have {self.num_mels} values, got {v.numel()}")
        return v

    @torch.no_grad()
    def forward(self, wav, lengths=None, mel_min=None, mel_max=None, pad_value=0.0):
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        if wav.dim() != 2 or wav.shape[0] < 1:
            raise ValueError(f"MelSpectrogram: expected a waveform [B, T] or [T], got {tuple(wav.shape)}")
        if (mel_min is None) != (mel_max is None):
            raise ValueError("MelSpectrogram: give both mel_min and mel_max, or neither")
        device = wav.device
        lib, stream = self._sync(device)
        x = wav.detach().to(dtype=torch.float32).contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        lens = c_lengths(host_lengths(lengths, B, "MelSpectrogram"))
        n_norm, mn, mx = 0, None, None
        if mel_min is not None:
            mn, mx = self._range(mel_min, device, "mel_min"), self._range(mel_max, device, "mel_max")
            if mn.numel() != mx.numel():
                mn, mx = mn.expand(max(mn.numel(), mx.numel())).contiguous(), mx.expand(max(mn.numel(), mx.numel())).contiguous()
            n_norm = mn.numel()
        out = torch.empty(B, self.num_mels, T // self.hop_size, device=device)
        ws = self._workspace(lib, device, B, T)
        self._call(lib, device, "forward", self._h, x.data_ptr(), lens, B, T, None if mn is None else mn.data_ptr(),
                   None if mx is None else mx.data_ptr(), n_norm, float(pad_value), out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return out

    @torch.no_grad()
    def minmax(self, mel, frame_lengths=None):
        """Per-band (min, max), each [num_mels], over the valid frames of mel [B, num_mels, F] (`frame_lengths`: host integers, default
        F each): the inner loop of the reference's preprocessing/process_mel_normalization.py."""
        if mel.dim() != 3 or mel.shape[1] != self.num_mels or mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"MelSpectrogram.minmax: expected [B, {self.num_mels}, F], got {tuple(mel.shape)}")
        device = mel.device
        lib, stream = self._sync(device)
        x = mel.detach().to(dtype=torch.float32).contiguous()
        B, F = int(x.shape[0]), int(x.shape[2])
        lens = c_lengths(host_lengths(frame_lengths, B, "MelSpectrogram.minmax"))
        out = torch.empty(2, self.num_mels, device=device)
        self._call(lib, device, "minmax", self._h, x.data_ptr(), lens, B, F, out.data_ptr(), stream)
        return out[0], out[1]


_modules = {}


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """The reference's function (meldataset.py:51): y [B, T] in [-1, 1] on a ROCm device -> log-mel [B, num_mels, T // hop_size].  One
    module is kept per (configuration, device).  `center=True` is never used by the reference and is not built."""
    if center:
        raise NotImplementedError("mel_spectrogram: center=True is not built (the reference always passes center=False)")
    key = (int(n_fft), int(num_mels), int(sampling_rate), int(hop_size), int(win_size), float(fmin), None if fmax is None else float(fmax),
           str(y.device))
    m = _modules.get(key)
    if m is None:
        m = _modules[key] = MelSpectrogram(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax).to(y.device)
    return m(y)


def synthetic_waveform(n: int, seed: int = 0, sampling_rate: int = 22050) -> np.ndarray:
    """Seeded speech-like waveform [n] fp32 with peak 0.8: twelve harmonics of a gliding 120 Hz fundamental under a syllable-rate
    envelope, plus a noise floor of 1e-3 -- loud and quiet bands side by side, as in a recording."""
    g = np.random.Generator(np.random.Philox(key=3000 + seed))
    t = np.arange(n, dtype=np.float64) / sampling_rate
    phase = 2 * np.pi * np.cumsum(120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t)) / sampling_rate
    amps = g.random(12) / np.arange(1, 13)
    y = sum(a * np.sin(k * phase + 2 * np.pi * g.random()) for k, a in enumerate(amps, start=1))
    y = y * (0.5 + 0.5 * np.sin(2 * np.pi * 2.3 * t + 2 * np.pi * g.random()))
    y = 0.8 * y / np.abs(y).max() + 1e-3 * g.standard_normal(n)
    return np.ascontiguousarray(y, dtype=np.float32)
