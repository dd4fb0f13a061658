#!/usr/bin/env python3
"""Writes tests/golden/mos_{a,b}.npz in fp64 on the CPU: a tiny seeded `transformers.Wav2Vec2Model` as the upstream (make_goldens_ctc.py's
recipe: biases and norms moved off their initial values, eager attention, every item run alone) and a seeded MOS head on its hidden states,
stated with `torch.nn.Linear` modules as s3prl's downstream is (a: H = 40, 2 layers, P = 16; b: H = 48, 3 layers, P = 24).

    python tools/make_goldens_mos.py            # writes the files with SEEDS
    python tools/make_goldens_mos.py --search   # prints the first seed of each model that meets the requirements

Each file holds: `config` (json: the upstream's fields), `head` (json: hidden_size, n_states, projector_dim), `keys` (json: the upstream's
state_dict keys in HF's order), the upstream's weights as `w:<key>` and the head's as `h:<key>` (fp32, what the models were run with after
rounding), per item i `wav_i` (fp32), `hs_i` [L+1][F][H], `e_i`, `mu_i`, `alpha_i` [F] (fp64) and `scores` [items][4]: attention pooling,
attention pooling clipped, mean pooling, mean pooling clipped (the mean variants on the same weights without the pooling layer).

A seed is taken only when, for the 18-frame item, the largest alpha lies in [2 / F, 0.9] (attention neither uniform nor one-hot), the
softmaxed layer weights span at least a factor 3, every unclipped score has |score| < 1.5 (tanh off saturation), and the attention and mean
scores of some item differ by at least 0.05.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_goldens_ctc import COMMON, ITEMS, waveform  # noqa: E402

CONFIGS = {
    "a": (dict(COMMON, hidden_size=40, num_attention_heads=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4), 16),
    "b": (dict(COMMON, hidden_size=48, num_attention_heads=3, num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=4,
               num_hidden_layers=3), 24),
}
SEEDS = {"a": 3, "b": 1}            # from --search
VARIANTS = ("attention", "attention_clipped", "mean", "mean_clipped")


def conditions(alpha_long, s, scores):
    """The four requirements above -> (ok, a line that says which hold); scores [items][4] in VARIANTS' order."""
    F = len(alpha_long)
    top = float(np.max(alpha_long))
    c1 = 2.0 / F <= top <= 0.9
    c2 = float(s.max() / s.min()) >= 3.0
    c3 = bool((np.abs(scores[:, [0, 2]]) < 1.5).all())
    c4 = bool((np.abs(scores[:, 0] - scores[:, 2]) >= 0.05).any())
    return c1 and c2 and c3 and c4, f"max alpha {top:.3f} ({c1}), layer span {float(s.max() / s.min()):.2f} ({c2}), |score| < 1.5 ({c3}), att/mean gap ({c4})"


def make(name, seed):
    import transformers
    c, P = CONFIGS[name]
    torch.manual_seed(seed)
    cfg = transformers.Wav2Vec2Config(hidden_act="gelu", feat_extract_norm="group", feat_extract_activation="gelu", conv_bias=False,
                                      do_stable_layer_norm=False, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                                      feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, attn_implementation="eager", **c)
    model = transformers.Wav2Vec2Model(cfg).eval()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():                # HF starts biases at 0 and norms at (1, 0): move them, so that each one is seen
        for k, p in model.named_parameters():
            if k.endswith(".bias") or "layer_norm" in k:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if k.endswith("original0"):
                p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    m64 = model.double()
    H, n = c["hidden_size"], c["num_hidden_layers"] + 1
    # the head, as s3prl states it: Featurizer.weights, connector, mean_net_pooling.W, mean_net_linear
    weights = torch.randn(n, generator=g)
    connector, pool, linear = torch.nn.Linear(H, P), torch.nn.Linear(P, 1), torch.nn.Linear(P, 1)
    with torch.no_grad():
        connector.weight.copy_(torch.randn(P, H, generator=g) * H ** -0.5)
        connector.bias.copy_(0.1 * torch.randn(P, generator=g))
        pool.weight.copy_(torch.randn(1, P, generator=g) * 2.0 * P ** -0.5)
        pool.bias.copy_(0.1 * torch.randn(1, generator=g))
        linear.weight.copy_(torch.randn(1, P, generator=g) * P ** -0.5)
        linear.bias.copy_(0.1 * torch.randn(1, generator=g))
    head = {"featurizer.weights": weights, "connector.weight": connector.weight, "connector.bias": connector.bias,
            "model.mean_net_pooling.W.weight": pool.weight, "model.mean_net_pooling.W.bias": pool.bias,
            "model.mean_net_linear.weight": linear.weight, "model.mean_net_linear.bias": linear.bias}
    head = {k: v.detach().clone() for k, v in head.items()}
    connector, pool, linear = connector.double(), pool.double(), linear.double()
    out = {"config": json.dumps(c), "head": json.dumps(dict(hidden_size=H, n_states=n, projector_dim=P)), "keys": json.dumps(list(sd.keys())),
           "n_items": np.int64(len(ITEMS)), "variants": json.dumps(VARIANTS)}
    for k, v in sd.items():
        out["w:" + k] = v.numpy().astype(np.float32)
    for k, v in head.items():
        out["h:" + k] = v.numpy().astype(np.float32)
    s = torch.softmax(weights.double(), dim=-1)
    scores = np.zeros((len(ITEMS), 4))
    for i, nsamp in enumerate(ITEMS):
        y = waveform(nsamp, 1000 * seed + i)
        with torch.no_grad():
            hs = torch.stack(m64(y.double()[None], output_hidden_states=True).hidden_states, 0)[:, 0]       # [L+1][F][H]
            x = (s.view(-1, 1, 1) * hs).sum(0)
            z = connector(x)
            e = pool(z)[:, 0]
            alpha = torch.softmax(e, dim=0)
            att = linear((alpha[:, None] * z).sum(0))[0]
            mu = linear(z)[:, 0]
            mean = mu.mean()
        scores[i] = [float(att), float(2 * torch.tanh(att) + 3), float(mean), float(2 * torch.tanh(mean) + 3)]
        out[f"wav_{i}"] = y.numpy()
        out[f"hs_{i}"], out[f"e_{i}"], out[f"mu_{i}"], out[f"alpha_{i}"] = hs.numpy(), e.numpy(), mu.numpy(), alpha.numpy()
    out["scores"] = scores
    good, line = conditions(out[f"alpha_{len(ITEMS) - 1}"], s.numpy(), scores)
    return out, good, f"{name} seed {seed}: scores {np.round(scores[:, 0], 3).tolist()} / mean {np.round(scores[:, 2], 3).tolist()}; {line} -> {'ok' if good else 'no'}"


def main():
    if "--search" in sys.argv:
        for name in CONFIGS:
            for seed in range(1, 400):
                _, good, line = make(name, seed)
                if good:
                    print(line)
                    break
        return
    for name in CONFIGS:
        out, good, line = make(name, SEEDS[name])
        print(line)
        assert good, "SEEDS no longer meet the requirements: run --search"
        path = os.path.join(ROOT, "tests", "golden", f"mos_{name}.npz")
        np.savez(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
