"""Torch-only restatement of the ECAPA-TDNN speaker encoder's eval-mode forward (unitspeech/speaker_encoder/ecapa_tdnn.py:248-287
and the modules it calls), from the upstream model's hidden states to the embedding, written from the reference as its
specification.

It takes a config dict (`feat_dim`, `channels`, `emb_dim`, `global_context_att`, `n_layers`), a state_dict in the reference's keys
(without `feature_extract.*`) and the hidden states, and runs on any device in fp32 or fp64.  It is the comparison leg of
bench_speaker_encoder.py (eager PyTorch on the same GPU) and the source of the extra shapes of tests/test_speaker_encoder_gpu.py;
tests/test_speaker_encoder.py pins it to the goldens of tools/make_goldens_speaker.py.  The product (unitspeech_amd) never imports it.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

DILATIONS = (2, 3, 4)          # layer2, layer3, layer4 (:225-227)
SCALE = 8                      # Res2 scale


def _bn(x, sd, p):
    """BatchNorm1d in eval mode: the running statistics, eps 1e-5."""
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _conv_relu_bn(x, sd, p, **kw):
    return _bn(F.relu(F.conv1d(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], **kw)), sd, p + ".bn")


def get_feat(sd, hidden_states):
    """:261-271.  [L, B, T, C] (or a list of L [B, T, C]) -> softmax-weighted sum, transpose, + 1e-6, InstanceNorm1d; a 3-d tensor is
    the already combined [B, C, T] (the fbank / mfcc form), which only gets the InstanceNorm1d."""
    if isinstance(hidden_states, (list, tuple)):
        hidden_states = torch.stack(list(hidden_states), dim=0)
    x = hidden_states
    if x.dim() == 4:
        w = F.softmax(sd["feature_weight"], dim=-1).view(-1, 1, 1, 1)
        x = (w * x).sum(dim=0)
        x = torch.transpose(x, 1, 2) + 1e-6
    # InstanceNorm1d without affine or running statistics: biased variance over T, eps 1e-5 (written out: F.instance_norm refuses T = 1)
    mean = x.mean(dim=2, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=2, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5)


def se_res2_block(x, sd, p, dilation):
    """SE_Res2Block.forward (:116-126) without a shortcut (in_channels == out_channels)."""
    y = _conv_relu_bn(x, sd, p + ".Conv1dReluBn1")
    width = y.shape[1] // SCALE
    spx = torch.split(y, width, 1)
    out, sp = [], None
    for i in range(SCALE - 1):                                             # :38-46
        sp = spx[i] if i == 0 else sp + spx[i]
        q = f"{p}.Res2Conv1dReluBn"
        sp = F.conv1d(sp, sd[f"{q}.convs.{i}.weight"], sd[f"{q}.convs.{i}.bias"], padding=dilation, dilation=dilation)
        sp = _bn(F.relu(sp), sd, f"{q}.bns.{i}")
        out.append(sp)
    out.append(spx[SCALE - 1])
    y = _conv_relu_bn(torch.cat(out, dim=1), sd, p + ".Conv1dReluBn2")
    s = y.mean(dim=2)                                                     # SE_Connect (:78-84)
    s = F.relu(F.linear(s, sd[p + ".SE_Connect.linear1.weight"], sd[p + ".SE_Connect.linear1.bias"]))
    s = torch.sigmoid(F.linear(s, sd[p + ".SE_Connect.linear2.weight"], sd[p + ".SE_Connect.linear2.bias"]))
    return y * s.unsqueeze(2) + x


def attentive_stats_pool(x, sd, p, global_context_att):
    """:145-161"""
    if global_context_att:
        mean = torch.mean(x, dim=-1, keepdim=True).expand_as(x)
        std = torch.sqrt(torch.var(x, dim=-1, keepdim=True) + 1e-10).expand_as(x)
        x_in = torch.cat((x, mean, std), dim=1)
    else:
        x_in = x
    alpha = torch.tanh(F.conv1d(x_in, sd[p + ".linear1.weight"], sd[p + ".linear1.bias"]))
    alpha = torch.softmax(F.conv1d(alpha, sd[p + ".linear2.weight"], sd[p + ".linear2.bias"]), dim=2)
    mean = torch.sum(alpha * x, dim=2)
    residuals = torch.sum(alpha * (x ** 2), dim=2) - mean ** 2
    return torch.cat([mean, torch.sqrt(residuals.clamp(min=1e-9))], dim=1)


def ecapa_forward(cfg, sd: Dict[str, torch.Tensor], hidden_states, dtype: Optional[torch.dtype] = None, stages: Optional[dict] = None):
    """hidden states -> [B, emb_dim] (`ECAPA_TDNN.forward`, :274-287).  The arithmetic runs in `dtype` (default: the hidden states')
    on the hidden states' device; `stages`, when given, receives the intermediates `feat`, `layer1`, `layer2`, `layer3`, `layer4`
    and `pooling`."""
    if isinstance(hidden_states, (list, tuple)):
        hidden_states = torch.stack(list(hidden_states), dim=0)
    dt = dtype or hidden_states.dtype
    dev = hidden_states.device
    if any(k.startswith(f"layer{i}.shortcut") for k in sd for i in (2, 3, 4)):
        raise NotImplementedError("SE_Res2Block shortcut")
    sd = {k: v.to(device=dev, dtype=dt) for k, v in sd.items() if v.is_floating_point()}
    x = get_feat(sd, hidden_states.to(dt))
    out1 = _conv_relu_bn(x, sd, "layer1", padding=2)
    out2 = se_res2_block(out1, sd, "layer2", DILATIONS[0])
    out3 = se_res2_block(out2, sd, "layer3", DILATIONS[1])
    out4 = se_res2_block(out3, sd, "layer4", DILATIONS[2])
    out = F.relu(F.conv1d(torch.cat([out2, out3, out4], dim=1), sd["conv.weight"], sd["conv.bias"]))
    pooled = attentive_stats_pool(out, sd, "pooling", bool(cfg["global_context_att"]))
    if stages is not None:
        stages.update(feat=x, layer1=out1, layer2=out2, layer3=out3, layer4=out4, pooling=pooled)
    return F.linear(_bn(pooled, sd, "bn"), sd["linear.weight"], sd["linear.bias"])
