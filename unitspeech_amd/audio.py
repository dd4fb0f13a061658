"""What the command-line tools do to a file before the library sees it: reading a wav (`read_wav`), bringing a waveform to 16 kHz on
the device (`to_16k`), opening a saved dictionary of tensors (`load_tensor_file`).  scipy is imported where it is needed."""
from __future__ import annotations

import numpy as np
import torch

__all__ = ["read_wav", "to_16k", "load_tensor_file"]


def read_wav(path, keep_int16: bool = False):
    """-> (mono samples, sampling rate) with scipy.io.wavfile: float32 in units of full scale, several channels averaged.  With
    `keep_int16` a single channel is taken off a [N, 1] file first and mono int16 stays int16."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    if keep_int16:
        if data.ndim == 2 and data.shape[1] == 1:
            data = data[:, 0]
        if data.dtype == np.int16 and data.ndim == 1:
            return np.ascontiguousarray(data), int(rate)
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    data = data.astype(np.float32)
    if data.ndim == 2:
        data = data.mean(axis=1)
    return np.ascontiguousarray(data), int(rate)


@torch.no_grad()
def to_16k(wav, rate, device, resamplers):
    """One waveform [T] at `rate` (an array or a tensor) -> fp32 [T'] at 16 kHz on `device` (preprocessing/utils.py:8-14); `resamplers`
    is the caller's dict, which keeps one `Resample` per rate."""
    from .resample import Resample
    wav = torch.as_tensor(wav).float().to(device)
    if rate == 16000:
        return wav
    if rate not in resamplers:
        resamplers[rate] = Resample(rate, 16000).to(device)
    return resamplers[rate](wav)


def load_tensor_file(path):
    """A `.npz` file as a dict of host tensors; anything else is what `torch.load` gives (the caller checks that it is a dict)."""
    if path.endswith(".npz"):
        with np.load(path) as f:
            return {k: torch.from_numpy(np.asarray(f[k])) for k in f.files}
    return torch.load(path, map_location="cpu")
