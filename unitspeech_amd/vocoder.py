"""BigVGAN vocoder on the HIP library: mel [B, num_mels, T] -> waveform [B, 1, T * hop] (inference).  With `lengths` (valid frames per
item) the batch is ragged: nothing past an item's end reaches its samples, and each item has the bits it has when it runs alone.

Drop-in for the reference's `unitspeech/vocoder/models.py:117-191` `BigVGAN(h)`: the same constructor argument (an `AttrDict`
or a plain dict of the JSON config), the same module tree and therefore the same `state_dict` keys, shapes and order, in both
forms -- with weight norm (`weight_g` / `weight_v`, as the checkpoint's "generator" dict stores it) and after
`remove_weight_norm()`.  The torch modules below only hold
parameters; the arithmetic is `csrc/vocoder.hip`.  Weight norm is folded where the parameters live, by the same
`WeightNorm.compute_weight` that `remove_weight_norm()` uses, so both forms hand the library bit-identical weights.

There is no CPU fallback: tensors must live on a ROCm device.  resblock "2" (`AMPBlock2`) is not built and raises.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import math
import warnings
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
from torch import nn
from torch.nn.utils.weight_norm import WeightNorm

from . import _lib
from ._args import c_lengths, host_lengths
from ._handle import HandleModule

# configs of the 22 kHz / 80-band BigVGAN generators (hop 256): the large one and the base one
BIGVGAN_22KHZ_80BAND = {
    "resblock": "1", "upsample_rates": [4, 4, 2, 2, 2, 2], "upsample_kernel_sizes": [8, 8, 4, 4, 4, 4], "upsample_initial_channel": 1536,
    "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "activation": "snakebeta",
    "snake_logscale": True, "num_mels": 80, "n_fft": 1024, "hop_size": 256, "win_size": 1024, "sampling_rate": 22050, "fmin": 0,
    "fmax": 8000,
}
BIGVGAN_BASE_22KHZ_80BAND = dict(BIGVGAN_22KHZ_80BAND, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4],
                                 upsample_initial_channel=512)


class _H(dict):
    """Attribute access to a config dict (what the reference's `AttrDict` gives it)."""
    __getattr__ = dict.__getitem__


def _config(h) -> _H:
    if isinstance(h, str):
        with open(h) as f:
            h = json.load(f)
    return _H(h if isinstance(h, dict) else vars(h))


def kaiser_sinc_filter1d(cutoff: float, half_width: float, kernel_size: int) -> torch.Tensor:
    """Kaiser-windowed sinc low-pass [1, 1, kernel_size], normalised to unit sum (alias_free_torch/filter.py).  Used only to give a
    freshly built module its filter buffers; a loaded state_dict brings its own."""
    even = kernel_size % 2 == 0
    half = kernel_size // 2
    a = 2.285 * (half - 1) * math.pi * 4 * half_width + 7.95
    beta = 0.1102 * (a - 8.7) if a > 50.0 else (0.5842 * (a - 21) ** 0.4 + 0.07886 * (a - 21.0) if a >= 21.0 else 0.0)
    window = torch.kaiser_window(kernel_size, beta=beta, periodic=False)
    t = torch.arange(-half, half) + 0.5 if even else torch.arange(kernel_size) - half
    f = 2 * cutoff * window * torch.sinc(2 * cutoff * t)
    return (f / f.sum()).view(1, 1, kernel_size)


# ---- parameter containers (module tree of models.py / activations.py / alias_free_torch) -------------------------------------

def _wn(m: nn.Module) -> nn.Module:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # torch.nn.utils.weight_norm is deprecated; it is what the reference's keys come from
        return torch.nn.utils.weight_norm(m)


def _remove_wn(m: nn.Module) -> None:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.nn.utils.remove_weight_norm(m)


class _Snake(nn.Module):
    def __init__(self, c, logscale, beta):
        super().__init__()
        init = torch.zeros(c) if logscale else torch.ones(c)
        self.alpha = nn.Parameter(init.clone())
        if beta:
            self.beta = nn.Parameter(init.clone())


class _Filter(nn.Module):
    def __init__(self, cutoff, half_width):
        super().__init__()
        self.register_buffer("filter", kaiser_sinc_filter1d(cutoff, half_width, 12))


class _DownSample(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _Filter(0.25, 0.3)


class _Activation1d(nn.Module):
    def __init__(self, c, h):
        super().__init__()
        self.act = _Snake(c, bool(h.snake_logscale), h.activation == "snakebeta")
        self.upsample = _Filter(0.25, 0.3)
        self.downsample = _DownSample()


class _AMPBlock1(nn.Module):
    def __init__(self, h, c, k, d):
        super().__init__()
        pad = lambda dil: (k * dil - dil) // 2
        self.convs1 = nn.ModuleList([_wn(nn.Conv1d(c, c, k, 1, dilation=d[i], padding=pad(d[i]))) for i in range(3)])
        self.convs2 = nn.ModuleList([_wn(nn.Conv1d(c, c, k, 1, dilation=1, padding=pad(1))) for _ in range(3)])
        self.activations = nn.ModuleList([_Activation1d(c, h) for _ in range(6)])


def _check_config(h: _H) -> None:
    if str(h.resblock) != "1":
        raise NotImplementedError(f"BigVGAN resblock {h.resblock!r} (AMPBlock2) is not built: only resblock '1' (AMPBlock1)")
    if h.activation not in ("snake", "snakebeta"):
        raise NotImplementedError(f"activation {h.activation!r}: only 'snake' and 'snakebeta'")
    if len(h.upsample_rates) != len(h.upsample_kernel_sizes) or not 1 <= len(h.upsample_rates) <= 8:
        raise ValueError("upsample_rates and upsample_kernel_sizes must have the same length, 1 to 8")
    if not 1 <= len(h.resblock_kernel_sizes) <= 4 or len(h.resblock_dilation_sizes) != len(h.resblock_kernel_sizes) or \
            any(len(d) != 3 for d in h.resblock_dilation_sizes):
        raise ValueError("1 to 4 resblock kernel sizes, each with 3 dilations (AMPBlock1)")


class BigVGAN(HandleModule):
    """`BigVGAN(h)` of models.py:117; `forward(mel [B, num_mels, T]) -> [B, 1, T * prod(upsample_rates)]`."""
    _abi, _what = "vocoder", "vocoder"

    def __init__(self, h):
        super().__init__()
        h = _config(h)
        _check_config(h)
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        c0 = int(h.upsample_initial_channel)
        self.conv_pre = _wn(nn.Conv1d(h.num_mels, c0, 7, 1, padding=3))
        self.ups = nn.ModuleList([nn.ModuleList([_wn(nn.ConvTranspose1d(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u, padding=(k - u) // 2))])
                                  for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes))])
        self.resblocks = nn.ModuleList([_AMPBlock1(h, c0 // 2 ** (i + 1), k, d) for i in range(self.num_upsamples)
                                        for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes)])
        ch = c0 // 2 ** self.num_upsamples
        self.activation_post = _Activation1d(ch, h)
        self.conv_post = _wn(nn.Conv1d(ch, 1, 7, 1, padding=3))
        self.hop = int(np.prod(h.upsample_rates))

    def remove_weight_norm(self):
        """models.py:193-202: every convolution loses its weight norm (the folded weight becomes the parameter `weight`)."""
        print("Removing weight norm...")
        for l in self.ups:
            for m in l:
                _remove_wn(m)
        for blk in self.resblocks:
            for m in list(blk.convs1) + list(blk.convs2):
                _remove_wn(m)
        _remove_wn(self.conv_pre)
        _remove_wn(self.conv_post)

    # ---- engine ----------------------------------------------------------------------------------------------------------

    def _config_struct(self):
        h = self.h
        c = _lib.us_vocoder_config()
        c.num_mels, c.upsample_initial_channel, c.resblock = int(h.num_mels), int(h.upsample_initial_channel), int(h.resblock)
        c.n_up, c.n_kernels = self.num_upsamples, self.num_kernels
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            c.upsample_rates[i], c.upsample_kernel_sizes[i] = int(u), int(k)
        for j, (k, d) in enumerate(zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes)):
            c.resblock_kernel_sizes[j] = int(k)
            for l in range(3):
                c.resblock_dilation_sizes[j][l] = int(d[l])
        c.activation = _lib.US_VOCODER_SNAKEBETA if h.activation == "snakebeta" else _lib.US_VOCODER_SNAKE
        c.snake_logscale = int(bool(h.snake_logscale))
        return c

    def _create(self, lib, device):
        c = self._config_struct()
        _lib.check(lib.us_vocoder_create(C.byref(self._h), C.byref(c)), None, "us_vocoder_create")

    def _sources(self):
        """Folded conv weights (made anew while the weight norm is on), biases, Snake parameters, filters."""
        out = OrderedDict()
        for name, m in self.named_modules():
            if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                hook = next((hk for hk in m._forward_pre_hooks.values() if isinstance(hk, WeightNorm)), None)
                if hook is None:
                    out[name + ".weight"] = ((m.weight,), None)
                else:
                    out[name + ".weight"] = ((getattr(m, hook.name + "_g"), getattr(m, hook.name + "_v")),
                                             lambda m=m, hook=hook: hook.compute_weight(m))
                out[name + ".bias"] = ((m.bias,), None)
        for key, t in self.state_dict(keep_vars=True).items():
            if key.endswith((".alpha", ".beta", ".filter")):
                out[key] = ((t,), None)
        return out

    @torch.no_grad()
    def forward(self, x, lengths=None):
        """mel [B, num_mels, T] -> [B, 1, T * hop].  `lengths` (B frame counts in [1, T]: a list, a host tensor or a device tensor, which
        costs one synchronisation to read): the batch is ragged, item b is valid on its first lengths[b] frames and whatever lies past
        them (NaN included) is never read; `out[b, :, :lengths[b] * hop]` has the bits of `forward(x[b:b+1, :, :lengths[b]])` and the
        samples past it are zeros (`us_vocoder_forward_lengths`)."""
        if x.dim() != 3 or x.shape[1] != self.h.num_mels or x.shape[2] < 1:
            raise ValueError(f"BigVGAN: expected mel [B, {self.h.num_mels}, T], got {tuple(x.shape)}")
        b, _, t = x.shape
        lengths = host_lengths(lengths, b, "BigVGAN.forward", integers_only=True)
        device = x.device
        lib, stream = self._sync(device)
        mel = x.detach().to(dtype=torch.float32).contiguous()
        wav = torch.empty(b, 1, t * self.hop, device=device)
        ws = self._workspace(lib, device, b, t)
        if lengths is None:
            self._call(lib, device, "forward", self._h, mel.data_ptr(), wav.data_ptr(), b, t, ws.data_ptr(), ws.numel(), stream)
        else:
            self._call(lib, device, "forward_lengths", self._h, mel.data_ptr(), c_lengths(lengths), wav.data_ptr(), b, t, ws.data_ptr(),
                       ws.numel(), stream)
        return wav


    @torch.no_grad()
    def debug_layer(self, prefix, x, res=None, sum=None, div=0.0, out=None, lengths=None):
        """One layer alone through the launch `forward` uses (us_vocoder_debug_layer): a convolution (`conv_pre`, `ups.<i>.0`,
        `resblocks.<n>.convs1|convs2.<l>`; with its epilogue's `res`, `sum` and `div`), an Activation1d (`resblocks.<n>.activations.<a>`,
        `activation_post`) or `conv_post` (tanh included).  x [B, C, Tin] -> [B, Cout, Tout]; `out`, `res` and `sum` are contiguous fp32
        tensors of that shape on x's device and may share storage, as they do in the forward.  `lengths` (B input-step counts in [1, Tin],
        as `forward` takes them): the ragged launch (us_vocoder_debug_layer_lengths); a convolution or an Activation1d then leaves `out`
        as it was at and past an item's end (give `out` to define it there), and `conv_post` writes zeros there."""
        lengths = host_lengths(lengths, x.shape[0] if x.dim() == 3 else -1, "BigVGAN.debug_layer", integers_only=True)
        device = x.device
        lib, stream = self._sync(device)
        try:
            mod = self.get_submodule(prefix)
        except AttributeError:
            mod = None
        if isinstance(mod, nn.ConvTranspose1d):
            cin, cout, rate = mod.in_channels, mod.out_channels, mod.stride[0]
        elif isinstance(mod, nn.Conv1d):
            cin, cout, rate = mod.in_channels, mod.out_channels, 1
        elif isinstance(mod, _Activation1d):
            cin = cout = mod.act.alpha.shape[0]
            rate = 1
        else:
            cin, cout, rate = x.shape[1], 1, 1           # not a layer: the library names the refusal
        if x.dim() != 3 or x.shape[1] != cin or x.shape[2] < 1:
            raise ValueError(f"BigVGAN.debug_layer({prefix}): expected [B, {cin}, T], got {tuple(x.shape)}")
        b, _, t = x.shape
        shape = (b, cout, t * rate)
        x = x.detach().to(dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty(shape, device=device)
        for name, v in (("out", out), ("res", res), ("sum", sum)):
            if v is not None and (tuple(v.shape) != shape or v.dtype != torch.float32 or v.device != device or not v.is_contiguous()):
                raise ValueError(f"BigVGAN.debug_layer({prefix}): {name} must be a contiguous fp32 {shape} on {device}")
        ptr = lambda v: None if v is None else v.data_ptr()
        with torch.cuda.device(device):
            if lengths is None:
                rc = lib.us_vocoder_debug_layer(self._h, prefix.encode(), x.data_ptr(), ptr(res), ptr(sum), float(div), out.data_ptr(), b, t, stream)
            else:
                rc = lib.us_vocoder_debug_layer_lengths(self._h, prefix.encode(), x.data_ptr(), ptr(res), ptr(sum), float(div), out.data_ptr(), b, t,
                                                        c_lengths(lengths), stream)
        self._check(lib, rc, f"us_vocoder_debug_layer({prefix})" if lengths is None else f"us_vocoder_debug_layer_lengths({prefix})")
        return out


def get_vocoder(config_path, checkpoint, device):
    """unitspeech/util.py:174-181 on the HIP vocoder: config JSON, checkpoint["generator"], to(device), eval, remove_weight_norm."""
    with open(config_path) as f:
        h = json.load(f)
    vocoder = BigVGAN(h)
    vocoder.load_state_dict(torch.load(checkpoint, map_location=lambda storage, loc: storage)["generator"])
    _ = vocoder.to(device).eval()
    vocoder.remove_weight_norm()
    return vocoder


def _rng(seed: int, name: str) -> np.random.Generator:
    key = int.from_bytes(hashlib.sha256(f"bigvgan/{seed}/{name}".encode()).digest()[:8], "little")
    return np.random.Generator(np.random.Philox(key=key))


GAINS = {"conv_pre": 0.3, "ups": 1.0, "resblocks": 0.5, "conv_post": 0.3}     # |folded weight| per normalised slice, by layer


def synthetic_bigvgan_state_dict(h, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded weights in the weight-norm form (the checkpoint's "generator" layout), reference key order.  Conv directions v ~ N(0, 0.01)
    as init_weights draws them (xutils.py); magnitudes g = GAINS[layer] (1 + 0.1 z) per normalised slice (weight_norm would start at
    |v|, which makes the signal fade through six levels), so the waveform spans a good part of (-1, 1) without sitting in the tanh's
    saturation; biases N(0, 0.01); log-scale alpha / beta N(0, 0.1) (linear ones 1 + 0.1 z).  Filters: the kaiser-sinc buffers of a
    fresh module."""
    h = _config(h)
    shapes = BigVGAN(h).state_dict()
    out = OrderedDict()

    def z(name, shape):
        return _rng(seed, name).standard_normal(shape, dtype=np.float32)

    def direction(name, shape):
        return 0.01 * z(name, shape)

    for name, t in shapes.items():
        shape = tuple(t.shape)
        if name.endswith(".filter"):
            v = t.numpy()
        elif name.endswith((".alpha", ".beta")):
            v = 0.1 * z(name, shape) if h.snake_logscale else 1.0 + 0.1 * z(name, shape)
        elif name.endswith(".bias"):
            v = 0.01 * z(name, shape)
        elif name.endswith(".weight_v"):
            v = direction(name, shape)
        elif name.endswith(".weight_g"):
            vname = name[:-1] + "v"
            vv = direction(vname, tuple(shapes[vname].shape)).astype(np.float64)
            v = np.full(shape, GAINS.get(name.split(".")[0], 0.5)) * (1.0 + 0.1 * z(name, shape))
        else:
            raise KeyError(name)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def bigvgan_flops(h, T: int) -> float:
    """Algorithmic FLOPs (2 x multiply-adds) of one forward of T mel frames, batch 1: the dense convolutions (conv_pre, the
    transposed up-samplers counted per real product, the AMP convolutions, conv_post) plus the anti-aliased activations' two 12-tap
    filters (2 x 6 taps per up-sampled sample, 12 per output)."""
    h = _config(h)
    c, t = int(h.upsample_initial_channel), int(T)
    f = 2.0 * h.num_mels * c * 7 * t
    n_act = 0.0
    for u, k in zip(h.upsample_rates, h.upsample_kernel_sizes):
        f += 2.0 * c * (c // 2) * k * t
        c, t = c // 2, t * u
        for kr in h.resblock_kernel_sizes:
            f += 6 * 2.0 * c * c * kr * t
        n_act += 6 * len(h.resblock_kernel_sizes) * c * t
    n_act += c * t
    f += 2.0 * c * 7 * t
    return f + n_act * 2.0 * (2 * 6 + 12)
