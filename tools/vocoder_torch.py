"""Torch-only restatement of the BigVGAN forward (unitspeech/vocoder/models.py:169-191, :60-69; activations.py;
alias_free_torch/{act,resample,filter}.py), written from the reference as its specification.

It takes the generator's config dict and a state_dict in either form (weight_g / weight_v or folded weights) and runs on any
device in any float dtype.  It is the comparison leg of bench_vocoder.py (eager PyTorch on the same GPU) and the source of the
extra shapes of tests/test_vocoder_gpu.py; tests/test_vocoder.py pins it to the goldens of tools/make_goldens_vocoder.py.  The
product (unitspeech_amd) never imports it.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """g * v / |v|, the norm taken over every axis but the first (torch weight_norm with dim=0: per output channel of a Conv1d
    [out, in, k], per INPUT channel of a ConvTranspose1d [in, out, k])."""
    return v * (g / v.norm(dim=tuple(range(1, v.dim())), keepdim=True))


def weights(sd: Dict[str, torch.Tensor], prefix: str) -> torch.Tensor:
    if prefix + ".weight" in sd:
        return sd[prefix + ".weight"]
    return torch._weight_norm(sd[prefix + ".weight_v"], sd[prefix + ".weight_g"], 0)      # the op weight_norm's hook runs


def activation1d(x: torch.Tensor, sd, prefix: str, h) -> torch.Tensor:
    """Activation1d: UpSample1d(2, 12) -> Snake / SnakeBeta -> DownSample1d(2, 12)."""
    c = x.shape[1]
    fu = sd[prefix + ".upsample.filter"].to(x.dtype)
    fd = sd[prefix + ".downsample.lowpass.filter"].to(x.dtype)
    # up-sampling: replicate pad 5, transposed depthwise conv stride 2, times 2, crop 15 / 15
    y = F.pad(x, (5, 5), mode="replicate")
    y = 2 * F.conv_transpose1d(y, fu.expand(c, -1, -1), stride=2, groups=c)
    y = y[..., 15:-15]
    alpha = sd[prefix + ".act.alpha"].to(x.dtype).view(1, -1, 1)
    beta = sd[prefix + ".act.beta"].to(x.dtype).view(1, -1, 1) if h["activation"] == "snakebeta" else alpha
    if h["snake_logscale"]:
        alpha, beta = torch.exp(alpha), torch.exp(beta)
    y = y + (1.0 / (beta + 1e-9)) * torch.sin(y * alpha) ** 2
    # low-pass + down-sampling: replicate pad (5, 6), depthwise conv stride 2
    y = F.pad(y, (5, 6), mode="replicate")
    return F.conv1d(y, fd.expand(c, -1, -1), stride=2, groups=c)


def bigvgan_forward(h, sd: Dict[str, torch.Tensor], mel: torch.Tensor) -> torch.Tensor:
    """mel [B, num_mels, T] -> wav [B, 1, T * prod(upsample_rates)] in mel's dtype / device (sd tensors are cast to them)."""
    dt, dev = mel.dtype, mel.device
    sd = {k: v.to(device=dev, dtype=dt) for k, v in sd.items()}
    if str(h["resblock"]) != "1":
        raise NotImplementedError("AMPBlock2")
    nk = len(h["resblock_kernel_sizes"])
    x = F.conv1d(mel, weights(sd, "conv_pre"), sd["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(x, weights(sd, f"ups.{i}.0"), sd[f"ups.{i}.0.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (kr, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            xr = x
            for l in range(3):
                xt = activation1d(xr, sd, f"{p}.activations.{2 * l}", h)
                xt = F.conv1d(xt, weights(sd, f"{p}.convs1.{l}"), sd[f"{p}.convs1.{l}.bias"], dilation=dil[l], padding=dil[l] * (kr - 1) // 2)
                xt = activation1d(xt, sd, f"{p}.activations.{2 * l + 1}", h)
                xt = F.conv1d(xt, weights(sd, f"{p}.convs2.{l}"), sd[f"{p}.convs2.{l}.bias"], padding=(kr - 1) // 2)
                xr = xt + xr
            xs = xr if xs is None else xs + xr
        x = xs / nk
    x = activation1d(x, sd, "activation_post", h)
    x = F.conv1d(x, weights(sd, "conv_post"), sd["conv_post.bias"], padding=3)
    return torch.tanh(x)
