"""Torch-only, differentiable restatement of the DurationPredictor's training forward (unitspeech/duration_predictor.py:47-63),
written from the reference as its specification, with the dropout masks as explicit inputs.

`masks` maps a dropout site (the numbering of include/unitspeech_hip.h: 0 follows norm_1, 1 follows norm_2) to the scaled keep
mask (0 or 1 / (1 - p)) in the reference tensor's shape [B, filter_channels, L]; a missing site is the identity (eval mode).  It
runs on any device in any float dtype; tests/test_duration_train.py pins it to the reference goldens and it is the eager leg of
bench_tts_step.py.  The product (unitspeech_amd) never imports it.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F


def layer_norm(x, g, b, eps=1e-5):
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), g, b, eps).transpose(1, -1)


def conv(x, sd, p):
    w = sd[p + ".weight"]
    return F.conv1d(x, w, sd[p + ".bias"], padding=w.shape[2] // 2)


def duration_forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, x_mask: torch.Tensor, g: Optional[torch.Tensor] = None,
                     masks: Optional[Dict[int, torch.Tensor]] = None) -> torch.Tensor:
    """x [B, C, L], x_mask [B, 1, L], g [B, 1, S] or None -> logw [B, 1, L]; differentiable in every tensor of sd (not in x)."""
    masks = masks or {}
    drop = lambda t, site: t * masks[site].to(t.dtype) if site in masks else t
    x = x.detach()
    if g is not None:
        x = torch.cat([x, g.transpose(1, 2).repeat(1, 1, x.shape[-1])], dim=1)
    h = drop(layer_norm(torch.relu(conv(x * x_mask, sd, "conv_1")), sd["norm_1.gamma"], sd["norm_1.beta"]), 0)
    h = drop(layer_norm(torch.relu(conv(h * x_mask, sd, "conv_2")), sd["norm_2.gamma"], sd["norm_2.beta"]), 1)
    return conv(h * x_mask, sd, "proj") * x_mask


def duration_mse(logw: torch.Tensor, w: torch.Tensor, x_mask: torch.Tensor) -> torch.Tensor:
    """The reverse=False branch (:60-62)."""
    return torch.sum((logw - torch.log(w + 1e-6) * x_mask) ** 2) / torch.sum(x_mask)
