"""Sinc resampler on the HIP library: `torchaudio.transforms.Resample` / `torchaudio.functional.resample`, the sample-rate conversion
the reference runs in front of the speaker encoder and the unit extractor (22050 -> 16000, finetune.py:113) and in its data loader (any rate
-> 22050, data.py:75).

The interpolation kernel is torchaudio's (`_get_sinc_resample_kernel`: a Hann- or Kaiser-windowed sinc per output phase), computed here
with torch in fp64 and rounded once to fp32 (torchaudio is not needed); the arithmetic is `csrc/resample.hip`.  There is no CPU fallback:
waveforms must live on a ROCm device.  The output has exactly ceil(new * T / orig) samples.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import torch

from . import _lib
from ._args import c_lengths, host_lengths
from ._handle import HandleModule

_KAISER_BETA = 14.769656459379492


def sinc_resample_kernel(orig_freq, new_freq, gcd, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """torchaudio's `_get_sinc_resample_kernel(..., dtype=None)`: (kernel fp32 [new', 1, orig' + 2 width], width) with orig' = orig_freq //
    gcd, new' = new_freq // gcd.  Row c is the windowed sinc `scale * sinc(pi t) * window(t)`, t = base * (k - width) / orig' - base * c /
    new' clamped to +-lowpass_filter_width, base = rolloff * min(orig', new'), scale = base / orig'; fp64 throughout, one rounding."""
    if not (int(orig_freq) == orig_freq and int(new_freq) == new_freq):
        raise ValueError("sinc_resample_kernel: frequencies must be of integer type (the kernel is periodic in their ratio)")
    if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
        raise ValueError(f"Invalid resampling method: {resampling_method}")
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    orig, new = int(orig_freq) // int(gcd), int(new_freq) // int(gcd)
    base = min(orig, new) * float(rolloff)
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    else:
        b = torch.tensor(_KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
        window = torch.i0(b * torch.sqrt(1 - (t / lowpass_filter_width) ** 2)) / torch.i0(b)
    t = t * math.pi
    kernel = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    return kernel.to(torch.float32), width


class Resample(HandleModule):
    """`forward(waveform [..., T], lengths=None)` -> [..., ceil(new' * T / orig')], torchaudio's constructor arguments.

    `lengths` (host integers, one per waveform of the flattened leading dimensions) are the samples of each item: an item's
    ceil(new' * length / orig') outputs are computed from its own samples only, and the rest of its row is 0.  The buffer `kernel`
    (torchaudio's name and shape) is what the library computes with."""
    _abi, _what = "resample", "resampler"
    _cache_sources = True

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None):
        super().__init__()
        self.orig_freq, self.new_freq = orig_freq, new_freq
        self.gcd = math.gcd(int(orig_freq), int(new_freq))
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta = resampling_method, lowpass_filter_width, rolloff, beta
        self.orig, self.new = int(orig_freq) // self.gcd, int(new_freq) // self.gcd
        if self.orig_freq != self.new_freq:
            kernel, self.width = sinc_resample_kernel(orig_freq, new_freq, self.gcd, lowpass_filter_width, rolloff, resampling_method, beta)
            self.register_buffer("kernel", kernel)

    def _sources(self):
        return OrderedDict((("kernel", ((self.kernel,), None)),))

    def _create(self, lib, device):
        c = _lib.us_resample_config(orig_freq=self.orig, new_freq=self.new, width=self.width)
        _lib.check(lib.us_resample_create(C.byref(self._h), C.byref(c)), None, "us_resample_create")

    def out_length(self, T: int) -> int:
        return (self.new * int(T) + self.orig - 1) // self.orig

    @torch.no_grad()
    def forward(self, waveform, lengths=None):
        if self.orig_freq == self.new_freq:
            return waveform
        if waveform.dim() < 1 or waveform.shape[-1] < 1 or waveform.numel() < 1:
            raise ValueError(f"Resample: expected a waveform [..., T], got {tuple(waveform.shape)}")
        device = waveform.device
        lib, stream = self._sync(device)
        shape = waveform.shape
        x = waveform.detach().to(dtype=torch.float32).reshape(-1, shape[-1]).contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        lens = c_lengths(host_lengths(lengths, B, "Resample"))
        out = torch.empty(B, self.out_length(T), device=device)
        ws = self._workspace(lib, device, B, T)
        self._call(lib, device, "forward", self._h, x.data_ptr(), lens, B, T, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return out.reshape(shape[:-1] + (out.shape[-1],))


_modules = {}


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """`torchaudio.functional.resample` on a ROCm device; one module is kept per (arguments, device)."""
    if orig_freq <= 0.0 or new_freq <= 0.0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if orig_freq == new_freq:
        return waveform
    key = (orig_freq, new_freq, int(lowpass_filter_width), float(rolloff), str(resampling_method), None if beta is None else float(beta),
           str(waveform.device))
    m = _modules.get(key)
    if m is None:
        m = _modules[key] = Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta).to(waveform.device)
    return m(waveform)
