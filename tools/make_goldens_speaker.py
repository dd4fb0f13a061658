#!/usr/bin/env python3
"""Golden vectors of the ECAPA-TDNN speaker encoder from the REFERENCE class (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_speaker.py

Imports `unitspeech.speaker_encoder.ecapa_tdnn` of the reference checkout with the missing-module stubs of tools/make_goldens.py and
replaces its `UpstreamExpert` with a local stand-in that returns preset hidden states, so the reference's own `forward` runs
`get_feat` and the trunk end to end without the upstream model (constructing the class with `config_path=None` would call
torch.hub.load; this script never does).  Weights are `unitspeech_amd.speaker_encoder.synthetic_ecapa_state_dict`, hidden states
`synthetic_hidden_states`; both are regenerated from their seeds by the tests, so neither is stored at full size.  Writes
tests/golden/speaker_<name>.npz with
  config            feat_dim / channels / emb_dim / global_context_att / n_layers as JSON text
  seed, B, T        weight and hidden-state seed, batch and frames
  emb32, emb64      the reference's output in fp32 and fp64 (their distance is the fp32 noise floor)
  keys / shapes     state_dict keys and shapes without `feature_extract.*`, in order
  keys_fbank / shapes_fbank      the same for feat_type 'fbank' (no feature_weight), taken from the trunk's modules
  tiny cases only:  hidden [L, B, T, C] and the fp64 intermediates feat, layer1, layer2, layer3, layer4, pooling
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import load_reference, save  # noqa: E402
from unitspeech_amd.speaker_encoder import synthetic_ecapa_state_dict, synthetic_hidden_states  # noqa: E402

TINY = {"feat_dim": 16, "channels": 16, "emb_dim": 8, "global_context_att": False, "n_layers": 3}
FULL = {"feat_dim": 1024, "channels": 512, "emb_dim": 256, "global_context_att": False, "n_layers": 25}
CASES = [("tiny", TINY, 2, 23, 0, True), ("tiny_gca", dict(TINY, global_context_att=True), 2, 23, 1, True),
         ("full", FULL, 1, 149, 2, False), ("full_long", FULL, 2, 499, 3, False)]


class _Upstream(nn.Module):
    """Stand-in for the s3prl upstream: one dummy parameter, no transformer layers, and the preset hidden states as its output (zeros
    of the right count before any is set: the reference's constructor runs it once to count them, ecapa_tdnn.py:237-246)."""
    layers, feat_dim = 1, 1

    def __init__(self, *a, **kw):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))
        self.model = nn.Module()
        self.model.encoder = nn.Module()
        self.model.encoder.layers = []
        self.preset = None

    def forward(self, wavs):
        if self.preset is None:
            return {"hidden_states": [torch.zeros(1, 1, self.feat_dim)] * self.layers}
        return {"hidden_states": self.preset}


def reference_module(cfg):
    load_reference()
    from unitspeech.speaker_encoder import ecapa_tdnn as E
    E.UpstreamExpert = _Upstream
    _Upstream.layers, _Upstream.feat_dim = cfg["n_layers"], cfg["feat_dim"]
    return E.ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"],
                        global_context_att=cfg["global_context_att"], feat_type="wavlm_large", config_path="stub")


def key_lists(sd, drop=()):
    items = [(k, t) for k, t in sd.items() if not k.startswith("feature_extract.") and k not in drop]
    return np.array([k for k, _ in items]), np.array([",".join(str(s) for s in t.shape) for _, t in items])


def main():
    torch.manual_seed(0)
    for name, cfg, B, T, seed, store in CASES:
        model = reference_module(cfg)
        sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, seed).items()}
        keys, shapes = key_lists(model.state_dict())
        assert list(sd) == list(keys), "state_dict key order mismatch"
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("feature_extract.") for k in missing), (missing, unexpected)
        model.eval()
        hid = synthetic_hidden_states(cfg["n_layers"], B, T, cfg["feat_dim"], seed)
        wav = torch.zeros(B, 16)
        stages = {}
        hooks = [getattr(model, n).register_forward_hook(lambda m, i, o, n=n: stages.__setitem__(n, o.detach().numpy().copy()))
                 for n in ("instance_norm", "layer1", "layer2", "layer3", "layer4", "pooling")]
        with torch.no_grad():
            model.feature_extract.preset = [torch.from_numpy(hid[l]) for l in range(hid.shape[0])]
            emb32 = model(wav).numpy()
            model = model.double()
            model.feature_extract.preset = [torch.from_numpy(hid[l]).double() for l in range(hid.shape[0])]
            emb64 = model(wav.double()).numpy()
        for h in hooks:
            h.remove()
        keys_fbank, shapes_fbank = key_lists(model.state_dict(), drop=("feature_weight",))
        arrs = dict(config=np.array(json.dumps(cfg)), seed=np.array(seed), B=np.array(B), T=np.array(T), emb32=emb32.astype(np.float32),
                    emb64=emb64, keys=keys, shapes=shapes, keys_fbank=keys_fbank, shapes_fbank=shapes_fbank)
        if store:
            arrs.update(hidden=hid, feat=stages["instance_norm"], layer1=stages["layer1"], layer2=stages["layer2"],
                        layer3=stages["layer3"], layer4=stages["layer4"], pooling=stages["pooling"])
        save(f"speaker_{name}", **arrs)
        print(f"speaker_{name}: emb {emb64.shape}, max|emb| {np.abs(emb64).max():.3f}, fp32 vs fp64 max {np.abs(emb32 - emb64).max():.2e}, "
              f"{len(keys)} keys")


if __name__ == "__main__":
    main()
