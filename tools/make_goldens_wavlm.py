#!/usr/bin/env python3
"""Writes tests/golden/wavlm_{a,b}.npz from the installed `transformers.WavLMModel` in fp64 on the CPU: two tiny seeded models, four
waveforms each, every item run alone (B = 1, no attention_mask) with output_hidden_states=True.

    python tools/make_goldens_wavlm.py

A is the large form (layer-norm extractor with conv biases, pre-LN encoder), B the base form (group-norm extractor, post-LN layers, no conv
bias).  Both use num_buckets = 32 and max_bucket_distance = 40, whose buckets saturate at |delta| = 33: the last item has 71 frames, so
exact, logarithmic and clamped buckets of both signs occur.

Each file holds: `config` (json), `keys` and `shapes` (json: the state_dict's keys in HF's order and their shapes), the weights as `w:<key>`
(fp32, what the model was run with after rounding), and per item i `wav_i` (fp32), `normalize_i` (0 / 1: F.layer_norm(x, x.shape) was
applied in fp64 before the model) and `hs_i` [n_layers + 1][F][H] fp64.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], intermediate_size=72,
              num_hidden_layers=2, layer_norm_eps=1e-5, num_buckets=32, max_bucket_distance=40)
CONFIGS = {
    "a": dict(COMMON, hidden_size=40, num_attention_heads=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
              feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
    "b": dict(COMMON, hidden_size=48, num_attention_heads=3, num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=4,
              feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False),
}
# (samples, DC offset, normalize)
ITEMS = [(400, 0.0, 0), (720, 0.0, 0), (1999, 0.5, 0), (22800, 0.0, 1)]


def waveform(n, seed, dc):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    y = 0.3 * torch.sin(2 * np.pi * 220.0 * t) + 0.2 * torch.sin(2 * np.pi * 1370.0 * t + 1.0) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    return (y + dc).to(torch.float32)


def main():
    from transformers import WavLMConfig, WavLMModel
    for name, c in CONFIGS.items():
        seed = {"a": 21, "b": 22}[name]
        torch.manual_seed(seed)
        cfg = WavLMConfig(vocab_size=32, hidden_act="gelu", feat_extract_activation="gelu", hidden_dropout=0.0, attention_dropout=0.0,
                          activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0, **c)
        model = WavLMModel(cfg).eval()
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():                # HF starts biases at 0, norms at (1, 0) and the gate constant at 1: move them, so that each one is seen
            for k, p in model.named_parameters():
                if k.endswith(".bias") or "layer_norm" in k:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
                if k.endswith("original0"):
                    p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
                if k.endswith("gru_rel_pos_const"):
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
                if k.endswith("gru_rel_pos_linear.weight"):
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
                if k.endswith("rel_attn_embed.weight"):
                    p.copy_(0.5 * torch.randn(p.shape, generator=g))
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        m64 = model.double()
        out = {"config": json.dumps(c), "keys": json.dumps(list(sd.keys())), "shapes": json.dumps([list(v.shape) for v in sd.values()]),
               "n_items": np.int64(len(ITEMS))}
        for k, v in sd.items():
            out["w:" + k] = v.numpy().astype(np.float32)
        for i, (n, dc, norm) in enumerate(ITEMS):
            y = waveform(n, 1000 * seed + i, dc)
            x = y.double()[None]
            if norm:
                x = F.layer_norm(x, x.shape)
            with torch.no_grad():
                hs = m64(x, output_hidden_states=True).hidden_states
            out[f"wav_{i}"] = y.numpy()
            out[f"normalize_{i}"] = np.int64(norm)
            out[f"hs_{i}"] = torch.stack([h[0] for h in hs]).numpy()
            print(name, i, n, "frames", hs[0].shape[1], "max|hs|", float(np.abs(out[f"hs_{i}"]).max()))
        path = os.path.join(ROOT, "tests", "golden", f"wavlm_{name}.npz")
        np.savez(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
