"""A torch restatement of the WavLM encoder forward, written from the model's definition: the fp64 yardstick of tests/test_wavlm*.py and the
eager leg of bench_wavlm.py.  It needs torch only.  Both published forms are covered: the layer-norm extractor with conv biases and the
pre-LN encoder (WavLM-large), and the group-norm extractor with post-LN layers (WavLM-base, base-plus).

    wavlm_forward_torch(sd, cfg, wav [B, T], lengths=None, dtype=torch.float64, normalize=False) -> list of n_layers + 1 tensors [B, F, H]

`sd` holds the weights under transformers.WavLMModel's key names, `cfg` the configuration's fields as a dict (see `large_config`).  Entry n
of the result is HF's `hidden_states[n]`: in the pre-LN form the un-normalised input of layer n for n < L and `encoder.layer_norm` of the
stream for n = L (with `n_layers_out = n < L` the list ends at the un-normalised entry n, as HF's does).

Per-item lengths (samples) have the library's semantics, those of tools/hubert_torch.py: item b's rows are what the model gives for
wav[b, :lengths[b]] alone, samples at or past the length are never used, and rows past the item's frames are 0.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from hubert_torch import _gelu, _layer_norm, frames, pos_conv_weight  # noqa: F401  (frames is re-exported)


def large_config():
    """WavLM-large (microsoft/wavlm-large; s3prl's wavlm_large)."""
    return dict(conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=1024,
                num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24, num_conv_pos_embeddings=128,
                num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True,
                num_buckets=320, max_bucket_distance=800)


def base_plus_config():
    """WavLM-base and base-plus (microsoft/wavlm-base-plus)."""
    return dict(large_config(), hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12,
                feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)


def _relative_positions_bucket(rel, num_buckets, max_distance):
    """T5-style bucket of rel = key - query (a long tensor): num_buckets / 2 per sign, exact below num_buckets / 4, logarithmic up to
    max_distance and clamped to the last bucket from there."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    rel = rel.abs()
    max_exact = nb // 2
    large = torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)
    large = (max_exact + large).to(torch.long).clamp(max=nb - 1)
    return out + torch.where(rel < max_exact, rel, large)


def first_saturated_distance(num_buckets, max_distance):
    """The smallest |delta| from which the bucket no longer changes."""
    last = num_buckets // 2 - 1
    d = torch.arange(0, 4 * max_distance + 4)
    return int(d[_relative_positions_bucket(-d, num_buckets, max_distance) == last][0])


@torch.no_grad()
def wavlm_forward_torch(sd, cfg, wav, lengths=None, dtype=torch.float64, normalize=False, n_layers_out=None):
    dev = wav.device
    W = {k: v.to(device=dev, dtype=dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    layer_form = cfg.get("feat_extract_norm", "layer") == "layer"
    pre_ln = bool(cfg.get("do_stable_layer_norm", layer_form))
    B, T = wav.shape
    lens = torch.full((B,), T, dtype=torch.long) if lengths is None else torch.as_tensor([int(n) for n in lengths], dtype=torch.long)
    assert int(lens.max()) <= T and frames(cfg, int(lens.min())) >= 1, "an item is longer than the batch or shorter than the receptive field"
    lens = lens.to(dev)
    zero = torch.zeros((), dtype=dtype, device=dev)

    def mask_of(n, width):                   # [B, width] True on each item's first n[b] positions
        return torch.arange(width, device=dev)[None, :] < n[:, None]

    m = mask_of(lens, T)
    x = torch.where(m, wav.to(dtype), zero)
    if normalize:                            # F.layer_norm(x, x.shape) per item over its own samples
        n = lens.to(dtype)[:, None]
        mu = x.sum(1, keepdim=True) / n
        d = torch.where(m, x - mu, zero)
        x = d / torch.sqrt(d.pow(2).sum(1, keepdim=True) / n + 1e-5)
    x = x[:, None, :]
    n = lens
    for i, (k, s) in enumerate(zip(cfg["conv_kernel"], cfg["conv_stride"])):
        p = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, W[p + "conv.weight"], W.get(p + "conv.bias") if cfg.get("conv_bias", layer_form) else None, stride=s)
        n = (n - k) // s + 1
        if layer_form:                       # LayerNorm over the channels of each step (eps 1e-5: nn.LayerNorm's default, not the config's)
            x = _layer_norm(x.transpose(1, 2), W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], 1e-5).transpose(1, 2)
        elif i == 0:                         # GroupNorm(C, C): per channel over the item's valid steps
            mk = mask_of(n, x.shape[-1])[:, None, :]
            cnt = n.to(dtype)[:, None, None]
            mu = torch.where(mk, x, zero).sum(-1, keepdim=True) / cnt
            d = torch.where(mk, x - mu, zero)
            x = d / torch.sqrt(d.pow(2).sum(-1, keepdim=True) / cnt + 1e-5)
            x = x * W[p + "layer_norm.weight"][None, :, None] + W[p + "layer_norm.bias"][None, :, None]
        x = _gelu(x)
    eps = float(cfg.get("layer_norm_eps", 1e-5))
    fm = mask_of(n, x.shape[-1])[:, :, None]                 # [B, F, 1]
    x = x.transpose(1, 2)
    x = _layer_norm(x, W["feature_projection.layer_norm.weight"], W["feature_projection.layer_norm.bias"], eps)
    x = x @ W["feature_projection.projection.weight"].t() + W["feature_projection.projection.bias"]
    x = torch.where(fm, x, zero)
    kp, g = int(cfg["num_conv_pos_embeddings"]), int(cfg["num_conv_pos_embedding_groups"])
    pos = F.conv1d(x.transpose(1, 2), pos_conv_weight(W), W["encoder.pos_conv_embed.conv.bias"], padding=kp // 2, groups=g)
    if kp % 2 == 0:
        pos = pos[:, :, :-1]
    x = torch.where(fm, x + _gelu(pos).transpose(1, 2), zero)
    if not pre_ln:
        x = torch.where(fm, _layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps), zero)
    out = [x]
    H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    d = H // nh
    Ltot = int(cfg["num_hidden_layers"])
    L = Ltot if n_layers_out is None else int(n_layers_out)
    Fr = x.shape[1]
    pos_ids = torch.arange(Fr)
    bucket = _relative_positions_bucket(pos_ids[None, :] - pos_ids[:, None], int(cfg["num_buckets"]), int(cfg["max_bucket_distance"]))
    bias = W["encoder.layers.0.attention.rel_attn_embed.weight"][bucket.to(dev)].permute(2, 0, 1)         # [heads, q, k]

    def attention(p, a):                     # a: the attention's input [B, F, H]
        ah = a.view(B, Fr, nh, d).transpose(1, 2)                                                          # [B, heads, F, d]
        pr = ah @ W[p + "attention.gru_rel_pos_linear.weight"].t() + W[p + "attention.gru_rel_pos_linear.bias"]
        ga, gb = torch.sigmoid(pr.view(B, nh, Fr, 2, 4).sum(-1)).unbind(-1)
        gate = ga * (gb * W[p + "attention.gru_rel_pos_const"].view(1, nh, 1) - 1.0) + 2.0              # [B, heads, F]
        q = (a @ W[p + "attention.q_proj.weight"].t() + W[p + "attention.q_proj.bias"]) * d ** -0.5
        k_ = a @ W[p + "attention.k_proj.weight"].t() + W[p + "attention.k_proj.bias"]
        v = a @ W[p + "attention.v_proj.weight"].t() + W[p + "attention.v_proj.bias"]
        q, k_, v = (t.view(B, Fr, nh, d).transpose(1, 2) for t in (q, k_, v))
        sc = q @ k_.transpose(-1, -2) + gate[..., None] * bias[None]
        sc = sc.masked_fill(~fm.view(B, 1, 1, Fr), float("-inf"))
        o = (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(B, Fr, H)
        return o @ W[p + "attention.out_proj.weight"].t() + W[p + "attention.out_proj.bias"]

    def ffn(p, a):
        f = _gelu(a @ W[p + "feed_forward.intermediate_dense.weight"].t() + W[p + "feed_forward.intermediate_dense.bias"])
        return f @ W[p + "feed_forward.output_dense.weight"].t() + W[p + "feed_forward.output_dense.bias"]

    for i in range(L):
        p = f"encoder.layers.{i}."
        if pre_ln:
            x = x + attention(p, _layer_norm(x, W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], eps))
            x = x + ffn(p, _layer_norm(x, W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps))
            x = torch.where(fm, x, zero)
            last = i + 1 == Ltot
            out.append(torch.where(fm, _layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps), zero) if last else x)
        else:
            x = _layer_norm(x + attention(p, x), W[p + "layer_norm.weight"], W[p + "layer_norm.bias"], eps)
            x = torch.where(fm, _layer_norm(x + ffn(p, x), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps), zero)
            out.append(x)
    if pre_ln and Ltot == 0:
        out[0] = torch.where(fm, _layer_norm(x, W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], eps), zero)
    return out


def synthetic_wavlm_state_dict(cfg, seed=0, masked_spec_embed=True, device="cpu"):
    """Seeded weights under HF's key names and in HF's order, at the scales of HF's `_init_weights`, with every bias, norm parameter,
    `gru_rel_pos_const` and `rel_attn_embed` moved off its initial value so that a wrong formula shows.  `device`: where they are drawn."""
    g = torch.Generator(device=device).manual_seed(int(seed))

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=device)

    sd = {}
    H, I, nh = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["num_attention_heads"])
    layer_form = cfg.get("feat_extract_norm", "layer") == "layer"
    if masked_spec_embed:
        sd["masked_spec_embed"] = torch.rand(H, generator=g, device=device)

    def ln(p, n):
        sd[p + ".weight"] = 1.0 + 0.1 * randn(n)
        sd[p + ".bias"] = 0.1 * randn(n)

    def lin(p, o, i_, std=0.02):
        sd[p + ".weight"] = std * randn(o, i_)
        sd[p + ".bias"] = 0.02 * randn(o)

    cin = 1
    for i, (c, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}."
        sd[p + "conv.weight"] = randn(c, cin, k) * math.sqrt(2.0 / (cin * k))
        if cfg.get("conv_bias", layer_form):
            sd[p + "conv.bias"] = 0.1 * randn(c)
        if layer_form or i == 0:
            ln(p + "layer_norm", c)
        cin = c
    ln("feature_projection.layer_norm", cin)
    lin("feature_projection.projection", H, cin)
    kp, gr = int(cfg["num_conv_pos_embeddings"]), int(cfg["num_conv_pos_embedding_groups"])
    sd["encoder.pos_conv_embed.conv.bias"] = 0.02 * randn(H)
    v = randn(H, H // gr, kp) * 2.0 * math.sqrt(1.0 / (kp * H))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1.0 + 0.1 * randn(1, 1, kp))
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = v
    ln("encoder.layer_norm", H)
    for i in range(int(cfg["num_hidden_layers"])):
        p = f"encoder.layers.{i}"
        sd[p + ".attention.gru_rel_pos_const"] = 1.0 + 0.3 * randn(1, nh, 1, 1)
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            lin(f"{p}.attention.{n}", H, H)
        lin(p + ".attention.gru_rel_pos_linear", 8, H // nh, std=0.3)
        if i == 0:
            sd[p + ".attention.rel_attn_embed.weight"] = 0.5 * randn(int(cfg["num_buckets"]), nh)
        ln(p + ".layer_norm", H)
        lin(p + ".feed_forward.intermediate_dense", I, H)
        lin(p + ".feed_forward.output_dense", H, I)
        ln(p + ".final_layer_norm", H)
    return sd
