"""A torch restatement of the HuBERT encoder forward (group-norm extractor, post-LN layers), written from the model's definition:
the fp64 yardstick of tests/test_hubert*.py and the eager leg of bench_hubert.py.  It needs torch only.

    hubert_forward_torch(sd, cfg, wav [B, T], lengths=None, dtype=torch.float64, normalize=False) -> list of n_layers + 1 tensors [B, F, H]

`sd` holds the weights under transformers.HubertModel's key names, `cfg` the configuration's fields as a dict (see `base_config`).
Entry n of the result is the encoder's state after n layers (HF's `hidden_states[n]`, fairseq's `output_layer = n`).

Per-item lengths (samples) have the library's semantics, which are NOT those of HF's attention_mask: item b's rows are what the model gives
for wav[b, :lengths[b]] alone.  The group norm's statistics run over the item's own steps, the positional convolution sees zeros past its
last frame, attention runs over its own frames, samples at or past the length are never used (they may be NaN), and rows past the item's
frames are 0.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def base_config():
    """HuBERT-base (facebook/hubert-base-ls960, mHuBERT, ContentVec)."""
    return dict(conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=768,
                num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, num_conv_pos_embeddings=128,
                num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)


def frames(cfg, n: int) -> int:
    """Frames of an n-sample item: floor((L - k) / s) + 1 per extractor layer (0 or less: shorter than the receptive field)."""
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def pos_conv_weight(sd, dtype=None):
    """The positional convolution's weight from its weight-norm parts: g * v / |v|, the norm over dims 0 and 1 (g is [1, 1, k])."""
    p = "encoder.pos_conv_embed.conv."
    if p + "parametrizations.weight.original0" in sd:
        g, v = sd[p + "parametrizations.weight.original0"], sd[p + "parametrizations.weight.original1"]
    else:
        g, v = sd[p + "weight_g"], sd[p + "weight_v"]
    if dtype is not None:
        g, v = g.to(dtype), v.to(dtype)
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _layer_norm(x, w, b, eps):          # over the last axis, biased variance, two-pass
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt(d.pow(2).mean(-1, keepdim=True) + eps) * w + b


@torch.no_grad()
def hubert_forward_torch(sd, cfg, wav, lengths=None, dtype=torch.float64, normalize=False, n_layers_out=None):
    dev = wav.device
    W = {k: v.to(device=dev, dtype=dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    B, T = wav.shape
    lens = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor([int(n) for n in lengths], dtype=torch.long)
    assert int(lens.max()) <= T and frames(cfg, int(lens.min())) >= 1, "an item is longer than the batch or shorter than the receptive field"
    lens = lens.to(dev)

    def mask_of(n, width):                   # [B, width] True on each item's first n[b] positions
        return torch.arange(width, device=dev)[None, :] < n[:, None]

    m = mask_of(lens, T)
    x = torch.where(m, wav.to(dtype), torch.zeros((), dtype=dtype, device=dev))
    if normalize:                            # F.layer_norm(x, x.shape) per item over its own samples
        n = lens.to(dtype)[:, None]
        mu = x.sum(1, keepdim=True) / n
        d = torch.where(m, x - mu, torch.zeros((), dtype=dtype, device=dev))
        x = d / torch.sqrt(d.pow(2).sum(1, keepdim=True) / n + 1e-5)
    x = x[:, None, :]
    n = lens
    for i, (k, s) in enumerate(zip(cfg["conv_kernel"], cfg["conv_stride"])):
        x = F.conv1d(x, W[f"feature_extractor.conv_layers.{i}.conv.weight"], stride=s)
        n = (n - k) // s + 1
        if i == 0:                           # GroupNorm(C, C): per channel over the item's valid steps
            mk = mask_of(n, x.shape[-1])[:, None, :]
            cnt = n.to(dtype)[:, None, None]
            mu = torch.where(mk, x, torch.zeros((), dtype=dtype, device=dev)).sum(-1, keepdim=True) / cnt
            d = torch.where(mk, x - mu, torch.zeros((), dtype=dtype, device=dev))
            x = d / torch.sqrt(d.pow(2).sum(-1, keepdim=True) / cnt + 1e-5)
            x = x * W["feature_extractor.conv_layers.0.layer_norm.weight"][None, :, None] + W["feature_extractor.conv_layers.0.layer_norm.bias"][None, :, None]
        x = _gelu(x)
    eps = float(cfg.get("layer_norm_eps", 1e-5))
    fm = mask_of(n, x.shape[-1])[:, :, None]                 # [B, F, 1]
    zero = torch.zeros((), dtype=dtype, device=dev)
    x = x.transpose(1, 2)
    x = _layer_norm(x, W["feature_projection.layer_norm.weight"], W["feature_projection.layer_norm.bias"], eps)
    x = x @ W["feature_projection.projection.weight"].t() + W["feature_projection.projection.bias"]
    x = torch.where(fm, x, zero)
    kp, g = int(cfg["num_conv_pos_embeddings"]), int(cfg["num_conv_pos_embedding_groups"])
    pos = F.conv1d(x.transpose(1, 2), pos_conv_weight(W), W["encoder.pos_conv_embed.conv.bias"], padding=kp // 2, groups=g)
    if kp % 2 == 0:
        pos = pos[:, :, :-1]
    x = x + _gelu(pos).transpose(1, 2)
    x = torch.where(fm, _layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps), zero)
    out = [x]
    H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    d = H // nh
    L = int(cfg["num_hidden_layers"]) if n_layers_out is None else int(n_layers_out)
    Fr = x.shape[1]
    for i in range(L):
        p = f"encoder.layers.{i}."
        q = (x @ W[p + "attention.q_proj.weight"].t() + W[p + "attention.q_proj.bias"]) * d ** -0.5
        k_ = x @ W[p + "attention.k_proj.weight"].t() + W[p + "attention.k_proj.bias"]
        v = x @ W[p + "attention.v_proj.weight"].t() + W[p + "attention.v_proj.bias"]
        q, k_, v = (t.view(B, Fr, nh, d).transpose(1, 2) for t in (q, k_, v))
        sc = q @ k_.transpose(-1, -2)
        sc = sc.masked_fill(~fm.view(B, 1, 1, Fr), float("-inf"))
        a = (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(B, Fr, H)
        a = a @ W[p + "attention.out_proj.weight"].t() + W[p + "attention.out_proj.bias"]
        x = _layer_norm(x + a, W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], eps)
        f = _gelu(x @ W[p + "feed_forward.intermediate_dense.weight"].t() + W[p + "feed_forward.intermediate_dense.bias"])
        f = f @ W[p + "feed_forward.output_dense.weight"].t() + W[p + "feed_forward.output_dense.bias"]
        x = torch.where(fm, _layer_norm(x + f, W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps), zero)
        out.append(x)
    return out


def synthetic_hubert_state_dict(cfg, seed=0, masked_spec_embed=True):
    """Seeded weights under HF's key names, initialised as HF's `_init_weights` does: N(0, 0.02) linears with zero biases, Kaiming-normal
    extractor convolutions, the positional convolution N(0, 2 sqrt(1 / (k * H))) with zero bias, unit LayerNorm / GroupNorm."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    H, I = int(cfg["hidden_size"]), int(cfg["intermediate_size"])
    if masked_spec_embed:
        sd["masked_spec_embed"] = torch.rand(H, generator=g)
    cin = 1
    for i, (c, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        sd[f"feature_extractor.conv_layers.{i}.conv.weight"] = torch.randn(c, cin, k, generator=g) * math.sqrt(2.0 / (cin * k))
        if i == 0:
            sd["feature_extractor.conv_layers.0.layer_norm.weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
            sd["feature_extractor.conv_layers.0.layer_norm.bias"] = 0.1 * torch.randn(c, generator=g)
        cin = c

    def ln(p, n):
        sd[p + ".weight"] = 1.0 + 0.1 * torch.randn(n, generator=g)
        sd[p + ".bias"] = 0.1 * torch.randn(n, generator=g)

    def lin(p, o, i_):
        sd[p + ".weight"] = 0.02 * torch.randn(o, i_, generator=g)
        sd[p + ".bias"] = 0.02 * torch.randn(o, generator=g)

    ln("feature_projection.layer_norm", cin)
    lin("feature_projection.projection", H, cin)
    kp, gr = int(cfg["num_conv_pos_embeddings"]), int(cfg["num_conv_pos_embedding_groups"])
    sd["encoder.pos_conv_embed.conv.bias"] = 0.02 * torch.randn(H, generator=g)
    v = torch.randn(H, H // gr, kp, generator=g) * 2.0 * math.sqrt(1.0 / (kp * H))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1.0 + 0.1 * torch.randn(1, 1, kp, generator=g))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = v
    ln("encoder.layer_norm", H)
    for i in range(int(cfg["num_hidden_layers"])):
        p = f"encoder.layers.{i}"
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            lin(f"{p}.attention.{n}", H, H)
        ln(p + ".layer_norm", H)
        lin(p + ".feed_forward.intermediate_dense", I, H)
        lin(p + ".feed_forward.output_dense", H, I)
        ln(p + ".final_layer_norm", H)
    return sd
