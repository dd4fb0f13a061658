#!/usr/bin/env python3
"""Writes tests/golden/ctc_{a,b}.npz from the installed `transformers` in fp64 on the CPU: a tiny seeded `HubertForCTC` (a: H = 40, V = 12)
and `Wav2Vec2ForCTC` (b: H = 48, V = 33), four waveforms each, every item run alone (B = 1, no attention_mask).

    python tools/make_goldens_ctc.py            # writes the files with SEEDS
    python tools/make_goldens_ctc.py --search   # prints the first seed of each model that meets the requirements

Each file holds: `config` (json, with vocab_size and pad_token_id), `keys` (json: the state_dict's keys in HF's order), the weights as
`w:<key>` (fp32, what the model was run with after rounding), per item i `wav_i` (fp32), `hidden_i` [F][H], `logits_i` [F][V] (fp64) and
`ids_i` [F] (the argmax of the fp64 logits), and `min_margin`, the smallest gap between the two largest fp64 logits over all frames, with
`max_logit`.  `lm_head.weight` is drawn with unit scale so that the ids vary.  A seed is taken only when, over the four items, at least 4
distinct ids occur, one of them the blank, one frame repeats its predecessor, and min_margin >= 1e-3 * max |logit|: then a correct fp32
engine decodes the same ids on every frame (the UNITS_SEED practice of tests/test_hubert_gpu.py).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], intermediate_size=72,
              num_hidden_layers=2, layer_norm_eps=1e-5)
CONFIGS = {
    "a": ("HubertForCTC", dict(COMMON, hidden_size=40, num_attention_heads=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
                               vocab_size=12, pad_token_id=0)),
    "b": ("Wav2Vec2ForCTC", dict(COMMON, hidden_size=48, num_attention_heads=3, num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=4,
                                 vocab_size=33, pad_token_id=0)),
}
SEEDS = {"a": 1, "b": 9}            # from --search
ITEMS = [400, 720, 1999, 6001]       # samples: 1, 2, 5 and 18 frames


def waveform(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    y = 0.3 * torch.sin(2 * np.pi * 220.0 * t) * (0.5 + 0.5 * torch.sin(2 * np.pi * 7.0 * t)) + 0.2 * torch.sin(2 * np.pi * 1370.0 * t + 1.0)
    return (y + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).to(torch.float32)


def make(name, seed):
    import transformers
    cls_name, c = CONFIGS[name]
    cfg_cls = transformers.HubertConfig if cls_name == "HubertForCTC" else transformers.Wav2Vec2Config
    torch.manual_seed(seed)
    cfg = cfg_cls(hidden_act="gelu", feat_extract_norm="group", feat_extract_activation="gelu", conv_bias=False, do_stable_layer_norm=False,
                  hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0,
                  attn_implementation="eager", **c)
    model = getattr(transformers, cls_name)(cfg).eval()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():                # HF starts biases at 0 and norms at (1, 0): move them, so that each one is seen
        for k, p in model.named_parameters():
            if k == "lm_head.weight":
                p.copy_(torch.randn(p.shape, generator=g))
            elif k.endswith(".bias") or "layer_norm" in k:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if k.endswith("original0"):
                p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    m64 = model.double()
    out = {"config": json.dumps(c), "class": cls_name, "keys": json.dumps(list(sd.keys())), "n_items": np.int64(len(ITEMS))}
    for k, v in sd.items():
        out["w:" + k] = v.numpy().astype(np.float32)
    margin, biggest, all_ids, repeat = np.inf, 0.0, [], False
    for i, n in enumerate(ITEMS):
        y = waveform(n, 1000 * seed + i)
        with torch.no_grad():
            r = m64(y.double()[None], output_hidden_states=True)
        logits = r.logits[0].numpy()
        ids = logits.argmax(-1).astype(np.int64)
        top = np.sort(logits, axis=-1)
        margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
        biggest = max(biggest, float(np.abs(logits).max()))
        all_ids += ids.tolist()
        repeat = repeat or bool((ids[1:] == ids[:-1]).any())
        out[f"wav_{i}"] = y.numpy()
        out[f"hidden_{i}"] = r.hidden_states[-1][0].numpy()
        out[f"logits_{i}"] = logits
        out[f"ids_{i}"] = ids
    out["min_margin"], out["max_logit"] = np.float64(margin), np.float64(biggest)
    good = len(set(all_ids)) >= 4 and c["pad_token_id"] in all_ids and repeat and margin >= 1e-3 * biggest
    return out, good, f"{name} seed {seed}: ids {all_ids} min_margin {margin:.3e} max|logit| {biggest:.2f} -> {'ok' if good else 'no'}"


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
        path = os.path.join(ROOT, "tests", "golden", f"ctc_{name}.npz")
        np.savez(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
