#!/usr/bin/env python3
"""Golden vectors of the BigVGAN vocoder from the REFERENCE class (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_vocoder.py

Imports `unitspeech.vocoder.models.BigVGAN` of the reference checkout with the missing-module stubs of tools/make_goldens.py,
loads the seeded weights of `unitspeech_amd.vocoder.synthetic_bigvgan_state_dict` in weight-norm form (the checkpoint's
"generator" layout), runs the forward in fp32 and in fp64 and writes tests/golden/vocoder_<name>.npz with
  config            the generator config as JSON text (settings only)
  seed              weight seed (the weights are regenerated from it, so none is stored)
  mel               [B, num_mels, T] input
  wav32, wav64      the reference's output in fp32 and fp64 (their distance is the fp32 noise floor)
  keys_wn / shapes_wn            state_dict keys and shapes of the weight-norm form, in order
  keys_removed / shapes_removed  the same after the reference's remove_weight_norm()
Configs: tiny (32 channels, rates [4, 2, 2], Snake with linear alpha, B = 2), the base 22 kHz one (T = 24) and the large 22 kHz
one (T = 12).
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import OUT, load_reference, save  # noqa: E402
from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BIGVGAN_BASE_22KHZ_80BAND, synthetic_bigvgan_state_dict  # noqa: E402

TINY = {"resblock": "1", "upsample_rates": [4, 2, 2], "upsample_kernel_sizes": [8, 4, 4], "upsample_initial_channel": 32,
        "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]], "activation": "snake", "snake_logscale": False,
        "num_mels": 8}
CASES = [("tiny", TINY, 2, 16, 0), ("base", BIGVGAN_BASE_22KHZ_80BAND, 1, 24, 1), ("large", BIGVGAN_22KHZ_80BAND, 1, 12, 2)]


def reference_bigvgan():
    load_reference()                       # stubs every third-party module the reference checkout lacks here
    from unitspeech.vocoder.env import AttrDict
    from unitspeech.vocoder.models import BigVGAN
    return BigVGAN, AttrDict


def mel_input(cfg, B, T, seed):
    g = np.random.Generator(np.random.Philox(key=1000 + seed))
    return (g.standard_normal((B, cfg["num_mels"], T), dtype=np.float32) * 2.0 - 5.0).astype(np.float32)


def key_lists(sd):
    return np.array(list(sd)), np.array([",".join(str(s) for s in t.shape) for t in sd.values()])


def main():
    BigVGAN, AttrDict = reference_bigvgan()
    torch.manual_seed(0)
    for name, cfg, B, T, seed in CASES:
        model = BigVGAN(AttrDict(cfg))
        sd = {k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(cfg, seed).items()}
        assert list(sd) == list(model.state_dict()), "state_dict key order mismatch"
        model.load_state_dict(sd, strict=True)
        model.eval()
        keys_wn, shapes_wn = key_lists(model.state_dict())
        mel = mel_input(cfg, B, T, seed)
        with torch.no_grad():
            wav32 = model(torch.from_numpy(mel)).numpy()
            wav64 = model.double()(torch.from_numpy(mel).double()).numpy()
            with contextlib.redirect_stdout(io.StringIO()):
                model.remove_weight_norm()
        keys_removed, shapes_removed = key_lists(model.state_dict())
        save(f"vocoder_{name}", config=np.array(json.dumps(cfg)), seed=np.array(seed), mel=mel, wav32=wav32.astype(np.float32), wav64=wav64,
             keys_wn=keys_wn, shapes_wn=shapes_wn, keys_removed=keys_removed, shapes_removed=shapes_removed)
        print(f"vocoder_{name}: wav {wav32.shape}, std {wav64.std():.3f}, max|wav| {np.abs(wav64).max():.3f}, "
              f"fp32 vs fp64 max {np.abs(wav32 - wav64).max():.2e}")


if __name__ == "__main__":
    main()
