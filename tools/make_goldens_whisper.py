#!/usr/bin/env python3
"""Writes tests/golden/whisper_{a,b,long,wide}.npz from the installed `transformers.WhisperForConditionalGeneration` in fp64 on the CPU: tiny
seeded models, three items each (`long`: two).

    python tools/make_goldens_whisper.py [name ...]          # no name: all of them

a: d_model 64, 2 heads (d_head 32), S 50, 24 target positions, V 96.  b: d_model 128, 2 heads (d_head 64, the real one), S 72 (a multiple
of neither 16 nor 64), 40 target positions (the self cache crosses 16 and 32), V 203 (odd, as the real 51,865 is).
long: the positions stretched and every pair a and b keep equal skewed.  S 1100 (above the 1024 threads of the cross attention, a multiple of
neither 64 nor 16), 136 target positions (a lane of the self attention takes a third key), 4 encoder heads against 1 decoder head (d_head 16
and 64), 1 encoder layer against 3 decoder layers, ffn 96 against 132 (K = 132: a multiple of 4 only), V 101.  Two items: three do not fit
under 1 MiB.  Its `enc` does not fit beside the weights either and goes to whisper_long_enc.npz at the rows `enc_rows`: 0 - 63, every
fifth row from 65 on, and every row from 992 on.
wide: K and the vocabulary stretched.  d_model 144 (the GEMM's wave 0 makes three trips over K, the others two; decoder d_head 36, a
multiple of 4 but not of 16; encoder d_head 48), 2 encoder layers against 1 decoder layer, ffn 200 against 1028 (16 x 64 + 4: a 17th trip
of wave 0 with one live quarter), S 70, 20 target positions, V 530 (two chunks of 512 logits).  Its weights alone take 0.6 MiB, so `enc` and
`logits` hold the first two items only (fp64 does not compress); `features`, `ids`, `tokens`, `lengths` and the rest hold all three.

A default-initialised tiny model emits one or two distinct tokens for ever, and a cache bug would not show.  So the weights are drawn anew:
token embeddings std 0.03, decoder positions std 0.7, matrices N(0, g^2 / fan_in) with g = 1.7, LayerNorm weights 1 +- 0.1, biases 0.1.  Seeds
are searched from SEED0 on, and a golden is written only when all three hold:
 1. the worst top-1 / top-2 margin over all steps and items is at least 1e-3 of the largest |logit|;
 2. some item has at least 8 distinct generated tokens and the three items' outputs differ;
 3. with `eos` chosen after a first pass, two items stop at different steps, at least 5 apart, and one never stops (`long`: one item
    never stops and the other stops at step 70 or later, so that both items fill the cache beyond 64 positions);
and, for the suppression test, some item's runner-up at the first generated position is 1e-3 of the largest |logit| above the third.

A file stays under 1 MiB because every tensor of two or more dimensions but the encoder's sinusoids lies on a grid: multiples, at most 127,
of the power of two `q:<key>` at or below a quarter of its standard deviation, stored as int8 in `w:<key>`; the models were run with exactly
those values (tools/whisper_torch.py: golden_state_dict).

Each file holds `config` (json, transformers' field names), `seed`, `keys` / `shapes` (json), the weights as `w:<key>` (fp32, or int8 with
`q:<key>`), `features` [3][n_mels][2 S] fp32, `enc` [3][S][d_model] fp64 (`long`: in its own file, with `enc_rows`), `ids`
[3][max_target_positions] (planted, the first one 1) and
`logits` [3][max_target_positions][V] fp64 (teacher forcing), `prompt` [3][4], `eos`, `tokens` [3][max_new] and `lengths` [3] (greedy, eos at
and after an item's end), `top_idx` / `top_val` [3][max_new][3] (the three largest logits of every step of the pass without eos) and `margin`
(the worst relative top-1 / top-2 margin).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    "a": dict(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
              decoder_ffn_dim=128, num_mel_bins=16, max_source_positions=50, max_target_positions=24, vocab_size=96),
    "b": dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=256,
              decoder_ffn_dim=256, num_mel_bins=24, max_source_positions=72, max_target_positions=40, vocab_size=203),
    "long": dict(d_model=64, encoder_attention_heads=4, decoder_attention_heads=1, encoder_layers=1, decoder_layers=3, encoder_ffn_dim=96,
                 decoder_ffn_dim=132, num_mel_bins=10, max_source_positions=1100, max_target_positions=136, vocab_size=101),
    "wide": dict(d_model=144, encoder_attention_heads=3, decoder_attention_heads=4, encoder_layers=2, decoder_layers=1, encoder_ffn_dim=200,
                 decoder_ffn_dim=1028, num_mel_bins=12, max_source_positions=70, max_target_positions=20, vocab_size=530),
}
SEED0 = {"a": 100, "b": 200, "long": 300, "wide": 400}
ITEMS = {"a": 3, "b": 3, "long": 2, "wide": 3}
P = 4
FLOAT_ITEMS = {"wide": 2}         # the items `enc` and `logits` hold, where all of them do not fit under 1 MiB
LONG_STOP = 70                    # `long`: the item that stops does so at this step or later


def enc_rows(S):
    """the rows of `enc` that whisper_long_enc.npz holds"""
    return np.asarray(sorted(set(range(64)) | set(range(65, S, 5)) | set(range(992, S))), dtype=np.int64)


def features(c, seed, items=3):
    """`items` smooth log-mel-like items in about [-1, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    n, T = c["num_mel_bins"], 2 * c["max_source_positions"]
    t = torch.arange(T, dtype=torch.float64)[None, None] / T
    f = torch.arange(n, dtype=torch.float64)[None, :, None] / n
    ph = torch.rand(items, 1, 1, generator=g, dtype=torch.float64)
    x = 0.6 * torch.sin(2 * np.pi * (3 * t + 2 * f + ph)) + 0.4 * torch.cos(2 * np.pi * (7 * t * (1 + ph) - f)) + 0.3 * torch.randn(items, n, T, generator=g, dtype=torch.float64)
    return x.float()


def reinit(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            r = lambda std=1.0: std * torch.randn(p.shape, generator=g)
            if k.endswith("embed_tokens.weight"):
                p.copy_(r(0.03))
            elif k == "model.decoder.embed_positions.weight":
                p.copy_(r(0.7))
            elif k == "model.encoder.embed_positions.weight":
                continue                                      # the sinusoids
            elif "layer_norm" in k:
                p.copy_((1.0 if k.endswith(".weight") else 0.0) + r(0.1))
            elif k.endswith(".bias"):
                p.copy_(r(0.1))
            elif p.dim() >= 2:
                p.copy_(r(1.7 / float(np.sqrt(p[0].numel()))))
            if p.dim() >= 2:                                  # onto the grid the file stores (see the module's text)
                q = grid(p)
                p.copy_(torch.round(p / q).clamp_(-127, 127) * q)


def grid(p):
    """the power of two at or below a quarter of the tensor's standard deviation"""
    return 2.0 ** int(np.floor(np.log2(float(p.std()) / 4)))


def seeded_model(c, seed):
    """transformers' model of configuration `c` with the weights of `reinit` at `seed` -> (the model in fp32, its state_dict without proj_out)"""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    torch.manual_seed(seed)
    cfg = WhisperConfig(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0,
                        activation_function="gelu", scale_embedding=False, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                        decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None, **c)
    model = WhisperForConditionalGeneration(cfg).eval()
    reinit(model, seed)
    return model, {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith("model.")}


def try_seed(name, c, seed):
    model, sd = seeded_model(c, seed)
    m64 = model.double()
    Tm, V = c["max_target_positions"], c["vocab_size"]
    max_new = Tm - P
    B = ITEMS[name]
    x = features(c, seed + 1, B)
    g = torch.Generator().manual_seed(seed + 2)
    ids = torch.randint(3, V, (B, Tm), generator=g)
    ids[:, 0] = 1
    with torch.no_grad():
        enc = m64.model.encoder(x.double()).last_hidden_state
        logits = m64(input_features=x.double(), decoder_input_ids=ids, use_cache=False).logits
        # the first pass, without an end: the whole prefix again at every step, no cache
        seq = ids[:, :P].clone()
        top_idx, top_val = [], []
        for _ in range(max_new):
            lg = m64(input_features=x.double(), decoder_input_ids=seq, use_cache=False).logits[:, -1]
            v, i = lg.topk(3, dim=-1)
            top_idx.append(i)
            top_val.append(v)
            seq = torch.cat([seq, i[:, :1]], dim=1)
    top_idx, top_val = torch.stack(top_idx, 1), torch.stack(top_val, 1)          # [B][max_new][3]
    gen = seq[:, P:]
    big = float(top_val.abs().max())
    margin = float((top_val[..., 0] - top_val[..., 1]).min()) / big
    distinct = [len(set(r.tolist())) for r in gen]
    if margin < 1e-3 or max(distinct) < 8 or len({tuple(r.tolist()) for r in gen}) < B:
        return None, f"margin {margin:.2e}, distinct {distinct}"
    if float((top_val[:, 0, 1] - top_val[:, 0, 2]).max()) / big < 1e-3:
        return None, "no runner-up margin at the first position"
    eos = None
    for e in range(3, V):
        first = [(r == e).nonzero()[0, 0].item() if (r == e).any() else None for r in gen]
        stops = sorted(f for f in first if f is not None)
        if (len(stops) == 1 and stops[0] >= LONG_STOP) if name == "long" else (len(stops) == 2 and stops[1] - stops[0] >= 5 and stops[0] >= 1):
            eos = e
            break
    if eos is None:
        return None, "no eos with two stops 5 apart and one item running on" if name != "long" else f"no eos with one stop at {LONG_STOP} or later"
    tokens = gen.clone()
    lengths = []
    for b in range(B):
        hit = (gen[b] == eos).nonzero()
        nb = int(hit[0, 0]) if len(hit) else max_new
        tokens[b, nb:] = eos
        lengths.append(nb)
    out = {"config": json.dumps(c), "seed": np.int64(seed), "keys": json.dumps(list(sd.keys())),
           "shapes": json.dumps([list(v.shape) for v in sd.values()]), "features": x.numpy(), "enc": enc.numpy(), "ids": ids.numpy(),
           "logits": logits.numpy(), "prompt": ids[:, :P].numpy(), "eos": np.int64(eos), "tokens": tokens.numpy(),
           "lengths": np.asarray(lengths, dtype=np.int64), "top_idx": top_idx.numpy(), "top_val": top_val.numpy(), "margin": np.float64(margin)}
    if name in FLOAT_ITEMS:
        out["enc"], out["logits"] = out["enc"][:FLOAT_ITEMS[name]], out["logits"][:FLOAT_ITEMS[name]]
    if name == "long":
        rows = enc_rows(c["max_source_positions"])
        out["enc_file"] = {"enc_rows": rows, "enc": out.pop("enc")[:, rows]}
    for k, v in sd.items():
        if v.dim() >= 2 and k != "model.encoder.embed_positions.weight":
            q = grid(v)
            out["w:" + k], out["q:" + k] = torch.round(v / q).to(torch.int8).numpy(), np.float32(q)
            assert torch.equal(torch.from_numpy(out["w:" + k]).float() * q, v), k
        else:
            out["w:" + k] = v.numpy().astype(np.float32)
    return out, f"margin {margin:.2e}, distinct {distinct}, eos {eos}, lengths {lengths}, max|logit| {big:.2f}"


def main():
    names = sys.argv[1:] or list(CONFIGS)
    if set(names) - set(CONFIGS):
        raise SystemExit(f"unknown configuration among {names}: the tool knows {list(CONFIGS)}")
    for name in names:
        c = CONFIGS[name]
        for seed in range(SEED0[name], SEED0[name] + 200):
            out, msg = try_seed(name, c, seed)
            print(name, seed, msg)
            if out is not None:
                break
        else:
            raise SystemExit(f"no seed met the conditions for configuration {name}")
        files = {f"whisper_{name}.npz": out}
        if "enc_file" in out:
            files[f"whisper_{name}_enc.npz"] = out.pop("enc_file")
        for file, arrays in files.items():
            path = os.path.join(ROOT, "tests", "golden", file)
            np.savez_compressed(path, **arrays)
            print(path, os.path.getsize(path), "bytes")
            assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
