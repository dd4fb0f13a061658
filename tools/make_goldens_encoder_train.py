#!/usr/bin/env python3
"""Golden gradients of the Encoder from the REFERENCE class (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_encoder_train.py

Instantiates `unitspeech.encoder.Encoder` of the reference (loader of tools/make_goldens.py) with the seeded weights of
`unitspeech_amd.encoder.synthetic_encoder_state_dict`, in eval mode (dropout off; autograd still runs), and differentiates
loss = sum(mu_x * g_mu) + sum(x * g_x) for seeded upstream gradients g_mu, g_x:
  encoder_train_tiny.npz  32 channels, 64 filter channels, 2 heads, 2 layers, W = 4, 50 symbols; B = 3, L = 23, lengths
                          (23, 14, 3): every gradient in fp32 and in fp64 (the fp64 run is the reference module in double)
  encoder_train_full.npz  conf/hydra_config.py sizes (192 / 768 / 6 layers / 2 heads / W = 4, 1000 units); B = 2, L = 60, lengths
                          (60, 41): mu_x, x, the fp64 norm of every gradient and the full fp64 gradients (stored as fp32) of proj_m.*
                          and of the last layer's emb_rel_k / emb_rel_v / conv_o
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_goldens import TINY as TINY_DEC, ReplayRandn, build, load_reference, save  # noqa: E402
from unitspeech_amd.encoder import EncoderConfig, synthetic_encoder_state_dict  # noqa: E402

TINY = EncoderConfig(n_vocab=50, n_feats=16, n_channels=32, filter_channels=64, n_heads=2, n_layers=2, kernel_size=3, window_size=4)
FULL = EncoderConfig(n_vocab=1000)


def run(cfg, B, L, lengths, key, dtype):
    import unitspeech.encoder as E
    enc = E.Encoder(cfg.n_vocab, cfg.n_feats, cfg.n_channels, cfg.filter_channels, cfg.n_heads, cfg.n_layers, cfg.kernel_size, 0.1,
                    window_size=cfg.window_size)
    sd = {k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(cfg, 0).items()}
    assert list(sd) == list(enc.state_dict()), "encoder state_dict key order mismatch"
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dtype).eval()
    g = np.random.Generator(np.random.Philox(key=key))
    ids = torch.from_numpy(g.integers(0, cfg.n_vocab, size=(B, L)).astype(np.int64))
    lens = torch.LongTensor(lengths)
    g_mu = torch.from_numpy(g.standard_normal((B, cfg.n_feats, L), dtype=np.float32))
    g_x = torch.from_numpy(g.standard_normal((B, cfg.n_channels, L), dtype=np.float32))
    mu_x, x, x_mask = enc(ids, lens)
    loss = (mu_x * g_mu.to(dtype)).sum() + (x * g_x.to(dtype)).sum()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in enc.named_parameters()}
    return dict(ids=ids, lengths=lens, g_mu=g_mu, g_x=g_x, mu_x=mu_x.detach(), x=x.detach(), x_mask=x_mask), grads


STEP2_E = EncoderConfig(n_vocab=50, n_feats=80, n_channels=32, filter_channels=64, n_heads=2, n_layers=2, kernel_size=3, window_size=4)


def step2_batch(B=3, units=(20, 15, 9), seed=73):
    """Seeded STEP2 batch: units, durations (1-4 frames per unit, 0 on padding), mel (y_lengths = sum of durations), speaker
    embeddings (unit norm).  Shared with tests/test_encoder_train_gpu.py and train_unit_encoder.py --synthetic."""
    g = np.random.Generator(np.random.Philox(key=seed))
    L = max(units)
    x = g.integers(0, STEP2_E.n_vocab, size=(B, L)).astype(np.int64)
    dur = g.integers(1, 5, size=(B, L)).astype(np.float32)
    for b, n in enumerate(units):
        dur[b, n:] = 0
    ylen = dur.sum(1).astype(np.int64)
    y = g.standard_normal((B, STEP2_E.n_feats, int(ylen.max())), dtype=np.float32)
    for b in range(B):
        y[b, :, ylen[b]:] = 0
    spk = g.standard_normal((B, TINY_DEC.spk_emb_dim), dtype=np.float32)
    spk /= np.linalg.norm(spk, axis=1, keepdims=True)
    return dict(x=x, x_lengths=np.array(units, dtype=np.int64), x_duration=dur, y=y, y_lengths=ylen, spk=spk)


def import_stubbed(name):
    """Import a reference script whose third-party imports (hydra, loggers, ...) are missing here: each missing module becomes a
    stub, as tools/make_goldens.py does for the reference package."""
    import importlib
    from unittest.mock import MagicMock
    tb = MagicMock()                       # torch.utils.tensorboard raises ImportError without the tensorboard package
    tb.__spec__ = importlib.machinery.ModuleSpec("torch.utils.tensorboard", None)
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    for _ in range(80):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            if e.name.startswith(("unitspeech", "conf", name)):
                raise
            m = MagicMock()
            m.__spec__ = importlib.machinery.ModuleSpec(e.name, None)
            m.__path__ = []
            sys.modules[e.name] = m
    raise RuntimeError("could not import " + name)


def step2(U):
    import random
    import types
    S2 = import_stubbed("train_STEP2")
    import unitspeech.encoder as E
    torch.manual_seed(5)
    random.seed(5)
    enc = E.Encoder(STEP2_E.n_vocab, STEP2_E.n_feats, STEP2_E.n_channels, STEP2_E.filter_channels, STEP2_E.n_heads, STEP2_E.n_layers,
                    STEP2_E.kernel_size, 0.1, window_size=STEP2_E.window_size)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(STEP2_E, 0).items()}, strict=True)
    enc.eval()
    dec = build(U, TINY_DEC, 0)
    dec.requires_grad_(False)
    d = step2_batch()
    B = d["x"].shape[0]
    batch = {"x": torch.from_numpy(d["x"]), "x_lengths": torch.from_numpy(d["x_lengths"]), "x_duration": torch.from_numpy(d["x_duration"]),
             "x_duration_lengths": torch.from_numpy(d["x_lengths"]), "y": torch.from_numpy(d["y"]),
             "y_lengths": torch.from_numpy(d["y_lengths"]), "spk_id": torch.arange(B)}
    spk_table = torch.nn.Embedding(B, TINY_DEC.spk_emb_dim)
    spk_table.weight.data.copy_(torch.from_numpy(d["spk"]))
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(n_feats=STEP2_E.n_feats))
    t = torch.tensor([0.21, 0.55, 0.87])
    z = torch.from_numpy(np.random.Generator(np.random.Philox(key=74)).standard_normal((B, 80, 32), dtype=np.float32))
    picks = []
    orig_choice, orig_rand, orig_cuda = random.choice, torch.rand, torch.Tensor.cuda
    random.choice = lambda r: (picks.append(orig_choice(r)), picks[-1])[1]
    torch.rand = lambda *a, **k: t.clone()
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with ReplayRandn([z]):
            prior, diff = S2.compute_train_step_loss(cfg, batch, spk_table, {i: i for i in range(B)}, enc, dec, 32)
    finally:
        random.choice, torch.rand, torch.Tensor.cuda = orig_choice, orig_rand, orig_cuda
    (prior + diff).backward()
    starts = [picks.pop(0) if n > 32 else 0 for n in d["y_lengths"]]
    arrs = dict(d, starts=np.array(starts, dtype=np.int64), t=t, z=z, prior_loss=prior.detach(), diff_loss=diff.detach())
    for k, p in enc.named_parameters():
        arrs["grad/" + k] = p.grad
    save("encoder_train_step2", **arrs)
    print(f"step2: prior {float(prior):.5f} diff {float(diff):.5f} starts {starts}")


def main():
    torch.set_num_threads(8)
    U = load_reference()
    step2(U)
    if "--step2-only" in sys.argv:
        return
    base, g32 = run(TINY, 3, 23, [23, 14, 3], 71, torch.float32)
    _, g64 = run(TINY, 3, 23, [23, 14, 3], 71, torch.float64)
    arrs = dict(base)
    for k in g32:
        arrs["g32/" + k] = g32[k]
        arrs["g64/" + k] = g64[k]
    save("encoder_train_tiny", **arrs)
    base, g64 = run(FULL, 2, 60, [60, 41], 72, torch.float64)
    arrs = {k: (v.float() if v.is_floating_point() else v) for k, v in base.items()}
    for k, v in g64.items():
        arrs["norm/" + k] = v.norm()
        last = f"encoder.attn_layers.{FULL.n_layers - 1}."
        if k.startswith(("proj_m.", last + "emb_rel", last + "conv_o.")):
            arrs["g64/" + k] = v.float()        # fp64 gradient rounded once to fp32 (file size)
    save("encoder_train_full", **arrs)


if __name__ == "__main__":
    main()
