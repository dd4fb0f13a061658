"""Active speech level (ITU-T P.56 method B, the "speech voltmeter") and the gain normalisation the reference's `sv56.py` shells out to
the ITU `sv56demo` binary for, on the HIP library and on ragged batches (csrc/level.hip).

  active_speech_level   wav -> level_db, activity, rms_db, peak and the 15 activity counts per item, as device tensors
  normalize_level       wav -> the waveform brought to `ndb` dB below full scale (fp32, or int16 rounded and saturated), and what was measured
  sv56                  the reference's `sv56(x, sr, ndb)`: numpy int16 in, numpy int16 of the same length out

The envelope, the counts and the level run in fp64 on the device; measuring and applying are enqueued back to back with nothing read to
the host in between.  An item has the same bits alone and inside any batch.  An item without measurable speech (level -100) or with a
non-finite sample (level NaN) comes back unchanged.  Parity with the `sv56demo` binary is not claimed; the yardstick is
tools/level_numpy.py.  There is no CPU fallback: a tensor that is not on a GPU raises.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._args import call as _call, device_lengths

__all__ = ["active_speech_level", "normalize_level", "sv56"]

SpeechLevel = namedtuple("SpeechLevel", "level_db activity rms_db peak counts")
LevelInfo = namedtuple("LevelInfo", "level_db activity rms_db peak counts gain clipped")

MAX_B, MAX_T = 65535, 1 << 30


def chunk() -> int:
    """The number of samples of a chunk: an item is cut into chunks of this size from its own start."""
    return int(_lib.load().us_level_chunk())


def _rows(wav, what):
    """-> (x [B, T] contiguous fp32 or int16, the dtype code): a [T], [B, T] or [B, 1, T] tensor."""
    if not torch.is_tensor(wav):
        raise TypeError(f"{what}: wav must be a tensor")
    if not wav.is_cuda:
        raise RuntimeError(f"{what}: the tensor is on {wav.device}; the level runs on the GPU only (there is no CPU fallback)")
    x = wav.detach()
    if x.dim() == 1:
        x = x[None]
    elif x.dim() == 3 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError(f"{what}: wav must be a non-empty [T], [B, T] or [B, 1, T], got {tuple(wav.shape)}")
    if x.dtype == torch.int16:
        code = _lib.US_LEVEL_I16
    elif x.dtype.is_floating_point:
        x, code = x.to(torch.float32), _lib.US_LEVEL_F32
    else:
        raise TypeError(f"{what}: wav must be floating point (units of full scale) or int16, got {wav.dtype}")
    B, T = x.shape
    if B > MAX_B or T > MAX_T:
        raise ValueError(f"{what}: at most {MAX_B} items of {MAX_T} samples, got {B} x {T}")
    return x.contiguous(), code


def _sample_rate(sample_rate, what):
    sr = int(sample_rate)
    if sr != sample_rate or sr <= 0:
        raise ValueError(f"{what}: the sample rate must be a positive integer, got {sample_rate!r}")
    return sr


def _measure(x, code, quantize, lens, sr):
    """-> (stats [B, 8] fp64, counts [B, 15] int64, the workspace, its size)."""
    B, T = x.shape
    dev = x.device
    n = int(_lib.load().us_level_workspace_bytes(B, T))
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    stats = torch.empty(B, 8, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 15, dtype=torch.int64, device=dev)
    _call(dev, "us_level_measure", x, code, int(quantize), lens, B, T, sr, stats, counts, ws, n)
    return stats, counts, ws, n


def _level(stats, counts):
    return SpeechLevel(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], counts)


@torch.no_grad()
def active_speech_level(wav, sample_rate, lengths=None):
    """wav: [T], [B, T] or [B, 1, T] on the GPU, floating point in units of full scale or int16; lengths [B] (samples per item, None: all)
    -> SpeechLevel(level_db [B], activity [B], rms_db [B], peak [B] in fp64, counts [B, 15] int64), all on the device.  level_db is -100
    where there is no measurable speech and NaN for an item with a non-finite sample."""
    x, code = _rows(wav, "active_speech_level")
    lens = device_lengths(lengths, x.shape[0], x.device, "active_speech_level")
    stats, counts, _, _ = _measure(x, code, False, lens, _sample_rate(sample_rate, "active_speech_level"))
    return _level(stats, counts)


@torch.no_grad()
def normalize_level(wav, sample_rate, ndb: float = -26.0, lengths=None, via_int16: bool = False, out_int16: bool = False):
    """Bring each item's active speech level to `ndb` dB relative to full scale -> (out, LevelInfo).

    out has wav's shape: fp32 = x * factor (computed in fp64, rounded once, not clamped), or with `out_int16` int16 = x * factor * 32768
    rounded half away from zero and saturated, a saturated sample counting in `clipped`.  Samples at or past lengths[b] come out as 0.
    `via_int16` first takes a floating-point input the reference's way to int16, `(x * 32767).astype(int16)`, so that the result is what
    the reference's `write` + `sv56` gives; the level in LevelInfo is then that of the quantised samples.  LevelInfo carries the fields
    of SpeechLevel plus gain [B] fp64 (the factor; 1 for an item left unchanged) and clipped [B] int64."""
    x, code = _rows(wav, "normalize_level")
    B, T = x.shape
    dev = x.device
    lens = device_lengths(lengths, B, dev, "normalize_level")
    quantize = bool(via_int16) and code == _lib.US_LEVEL_F32
    stats, counts, ws, n = _measure(x, code, quantize, lens, _sample_rate(sample_rate, "normalize_level"))
    out = torch.empty(B, T, dtype=torch.int16 if out_int16 else torch.float32, device=dev)
    gain = torch.empty(B, dtype=torch.float64, device=dev)
    clipped = torch.empty(B, dtype=torch.int64, device=dev)
    _call(dev, "us_level_apply", x, code, int(quantize), lens, B, T, stats, float(ndb), out, _lib.US_LEVEL_I16 if out_int16 else _lib.US_LEVEL_F32,
          gain, clipped, ws, n)
    shape = tuple(wav.shape)
    return out.reshape(shape), LevelInfo(stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3], counts, gain, clipped)


def sv56(x, sr, ndb, device="cuda"):
    """The reference's `sv56(x, sr, ndb)` without the binary: x numpy int16 [n] -> numpy int16 [n]."""
    x = np.asarray(x)
    if x.dtype != np.int16 or x.ndim != 1:
        raise TypeError(f"sv56: x must be a one-dimensional int16 array, got {x.dtype} {x.shape}")
    if x.size == 0:
        return x.copy()
    out, _ = normalize_level(torch.from_numpy(np.ascontiguousarray(x)).to(device), sr, ndb, out_int16=True)
    return out.cpu().numpy()
