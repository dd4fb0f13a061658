"""fp64 NumPy statement of voice conversion's mel-rate alignment (scripts/voice_conversion.py:22-33 of the reference), the
yardstick of `us_vc_align`: `F.interpolate(cond_x, size=mel_length, mode='linear')` (align_corners=False), the zero pad to the
U-Net's length multiple and `y_mask`, per item from its own lengths.

The source coordinate of output frame t is max((t + 0.5) * Lx / Ly - 0.5, 0).  It is evaluated exactly, as the rational
num / (2 Ly) with num = max((2 t + 1) Lx - Ly, 0): i0 = num // (2 Ly), lambda = (num mod 2 Ly) / (2 Ly).  torch's own kernels
evaluate it in the tensor's dtype from a precomputed scale Lx / Ly, which at long lengths is off by far more than a rounding of
the blend (fp32: 6.7e-5 at 499 -> 860; fp64 F.interpolate: 1e-3 at 16000 -> 27562, where a coordinate lands on the other side
of an integer), so torch cannot be the yardstick; tests/test_vc.py pins this file to exact rational arithmetic and to the
reference's output at a short length.  The product (unitspeech_amd) never imports it.
"""
from __future__ import annotations

import numpy as np


def coordinates(Lx: int, Ly: int):
    """-> (i0 [Ly] int64, i1 [Ly] int64, lam [Ly] float64) of the Ly output frames over Lx source frames."""
    t = np.arange(Ly, dtype=np.int64)
    num = np.maximum((2 * t + 1) * Lx - Ly, 0)
    den = 2 * Ly
    i0 = np.minimum(num // den, Lx - 1)
    i1 = i0 + (i0 < Lx - 1)
    lam = (num - i0 * den).astype(np.float64) / float(den)
    return i0, i1, lam


def interpolate(x: np.ndarray, Ly: int) -> np.ndarray:
    """x [..., Lx] -> [..., Ly] in fp64: (1 - lam) x[i0] + lam x[i1]."""
    x = np.asarray(x, dtype=np.float64)
    i0, i1, lam = coordinates(x.shape[-1], Ly)
    return (1.0 - lam) * x[..., i0] + lam * x[..., i1]


def vc_align(cond_x: np.ndarray, x_lengths, y_lengths, Tp: int):
    """cond_x [B, F, L], per-item lengths -> (cond_y [B, F, Tp] fp64, y_mask [B, 1, Tp] fp64): item b interpolated from its own
    x_lengths[b] frames to its own y_lengths[b] frames, zeros and a zero mask on [y_lengths[b], Tp)."""
    cond_x = np.asarray(cond_x, dtype=np.float64)
    B, F, L = cond_x.shape
    cond_y = np.zeros((B, F, Tp))
    y_mask = np.zeros((B, 1, Tp))
    for b in range(B):
        lx, ly = int(x_lengths[b]), int(y_lengths[b])
        if not (1 <= lx <= L and 1 <= ly <= Tp):
            raise ValueError(f"vc_align: item {b}: lengths ({lx}, {ly}) outside [1, {L}] x [1, {Tp}]")
        cond_y[b, :, :ly] = interpolate(cond_x[b, :, :lx], ly)
        y_mask[b, 0, :ly] = 1.0
    return cond_y, y_mask
