"""Torch-only, differentiable restatement of the Encoder's training forward (unitspeech/encoder.py:253-308 in train mode), written
from the reference as its specification, with the dropout masks as explicit inputs.

`masks` maps a dropout site (the numbering of include/unitspeech_hip.h: 0..2 the prenet's relu_drop, 3 + 4i / 4 + 4i / 5 + 4i /
6 + 4i the attention probabilities / the drop after attention / the FFN's drop / the drop after the FFN of layer i) to the
scaled keep mask (0 or 1 / (1 - p)) in the reference tensor's shape; a missing site is the identity (eval mode).  The relative
position terms are written in band form (score[i][j] += q_i . rel_k[j - i + W] for |j - i| <= W), which is what the reference's
pad-and-skew reaches.  It runs on any device in any float dtype; tests/test_encoder_train.py pins it to the reference goldens
and it is the eager leg of bench_unit_encoder.py.  The product (unitspeech_amd) never imports it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

PRENET_LAYERS = 3


def layer_norm(x, g, b, eps=1e-4):
    mean = torch.mean(x, 1, keepdim=True)
    var = torch.mean((x - mean) ** 2, 1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * g.view(1, -1, 1) + b.view(1, -1, 1)


def conv(x, sd, p):
    w = sd[p + ".weight"]
    return F.conv1d(x, w, sd[p + ".bias"], padding=w.shape[2] // 2)


def band(emb: torch.Tensor, L: int) -> torch.Tensor:
    """[1, 2W+1, D] -> E [L, L, D] with E[i, j] = emb[j - i + W] for |j - i| <= W, else 0."""
    e = emb[0]
    W = (e.shape[0] - 1) // 2
    i = torch.arange(L, device=e.device)
    off = i.view(1, L) - i.view(L, 1) + W
    ok = (off >= 0) & (off <= 2 * W)
    return e[off.clamp(0, 2 * W)] * ok.unsqueeze(-1).to(e.dtype)


def encoder_forward(sd: Dict[str, torch.Tensor], n_heads: int, ids: torch.Tensor, lengths: torch.Tensor,
                    masks: Optional[Dict[int, torch.Tensor]] = None, tape: Optional[Dict[str, torch.Tensor]] = None):
    """-> (mu_x [B, n_feats, L], x [B, C, L], x_mask [B, 1, L]); differentiable in every tensor of sd.

    `ids` [B, L] of an integer dtype are symbols for the Embedding front; a floating-point `ids` [B, L, n_contentvec] holds
    features for the Linear front (encoder.py:279-280, `emb.weight` [C, n_contentvec]).  Feature rows at or past an item's length
    count as zeros whatever they hold (the library does not read them).

    With `tape` (a dict), the intermediates a kernel-level test needs are stored in it under the names below, each with its
    gradient retained: after a backward, `tape[name].grad` is the operand the corresponding backward launch reads."""
    masks = masks or {}

    def keep(name, t):
        if tape is not None:
            if t.requires_grad:
                t.retain_grad()
            tape[name] = t
        return t
    drop = lambda t, site: t * masks[site].to(t.dtype) if site in masks else t
    emb = sd["emb.weight"]
    L = ids.shape[1]
    valid = torch.arange(L, device=ids.device).view(1, L) < lengths.view(-1, 1)
    if ids.is_floating_point():
        C = emb.shape[0]
        feats = torch.where(valid.unsqueeze(-1), ids.to(emb.dtype), torch.zeros((), dtype=emb.dtype, device=ids.device))
        x = keep("x0", (F.linear(feats, emb) * math.sqrt(C)).transpose(1, 2))
    else:
        C = emb.shape[1]
        x = keep("x0", (emb[ids] * math.sqrt(C)).transpose(1, 2))              # [B, C, L]
    x_mask = valid.unsqueeze(1).to(x.dtype)
    # prenet (ConvReluNorm)
    x_org, h = x, x
    for i in range(PRENET_LAYERS):
        h = keep(f"prenet.{i}.conv", conv(keep(f"prenet.{i}.in", h * x_mask), sd, f"prenet.conv_layers.{i}"))
        h = layer_norm(h, sd[f"prenet.norm_layers.{i}.gamma"], sd[f"prenet.norm_layers.{i}.beta"])
        h = drop(torch.relu(h), i)
    x = (x_org + conv(h, sd, "prenet.proj")) * x_mask
    # transformer blocks (EncoderModule)
    n_layers = sum(1 for k in sd if k.startswith("encoder.norm_layers_1.") and k.endswith(".gamma"))
    attn_mask = x_mask.unsqueeze(2) * x_mask.unsqueeze(-1)
    D = C // n_heads
    B = ids.shape[0]
    for i in range(n_layers):
        ap, site = f"encoder.attn_layers.{i}", 3 + 4 * i
        x = keep(f"layer.{i}.x", x * x_mask)
        q = keep(f"layer.{i}.q", conv(x, sd, ap + ".conv_q")).view(B, n_heads, D, L).transpose(2, 3)      # kept as [B, C, L]
        k = keep(f"layer.{i}.k", conv(x, sd, ap + ".conv_k")).view(B, n_heads, D, L).transpose(2, 3)
        v = keep(f"layer.{i}.v", conv(x, sd, ap + ".conv_v")).view(B, n_heads, D, L).transpose(2, 3)
        scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(D)
        rel = ap + ".emb_rel_k" in sd
        if rel:
            scores = scores + torch.einsum("bhid,ijd->bhij", q, band(sd[ap + ".emb_rel_k"], L)) / math.sqrt(D)
        scores = scores.masked_fill(attn_mask == 0, -1e4)
        p = drop(torch.softmax(scores, dim=-1), site)
        out = torch.matmul(p, v)
        if rel:
            out = out + torch.einsum("bhij,ijd->bhid", p, band(sd[ap + ".emb_rel_v"], L))
        y = conv(keep(f"layer.{i}.attn", out.transpose(2, 3).reshape(B, C, L)), sd, ap + ".conv_o")
        x = layer_norm(x + drop(y, site + 1), sd[f"encoder.norm_layers_1.{i}.gamma"], sd[f"encoder.norm_layers_1.{i}.beta"])
        fp = f"encoder.ffn_layers.{i}"
        y = drop(torch.relu(conv(x * x_mask, sd, fp + ".conv_1")), site + 2)
        y = conv(y * x_mask, sd, fp + ".conv_2") * x_mask
        x = layer_norm(x + drop(y, site + 3), sd[f"encoder.norm_layers_2.{i}.gamma"], sd[f"encoder.norm_layers_2.{i}.beta"])
    x = x * x_mask
    mu_x = conv(x, sd, "proj_m") * x_mask
    return mu_x, x, x_mask
