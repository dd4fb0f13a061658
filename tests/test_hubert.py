"""The HuBERT encoder's host side (no GPU): what us_hubert_create accepts and refuses, the frame count, the key list against transformers',
the fp64 restatement (tools/hubert_torch.py) against the goldens written from transformers.HubertModel, and the checkpoint spellings."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hubert_torch import base_config, frames, hubert_forward_torch, pos_conv_weight, synthetic_hubert_state_dict  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.hubert import HubertFeatureReader, HubertModel, from_fairseq_state_dict  # noqa: E402

TINY = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
            intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)


def struct_of(cfg, **over):
    s = HubertModel(**cfg)._config_struct()
    for k, v in over.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(s, k)[i] = x
        else:
            setattr(s, k, v)
    return s


def create(s):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.us_hubert_create(C.byref(h), C.byref(s))
    return lib, h, rc


@pytest.fixture(scope="module")
def base_handle():
    lib, h, rc = create(struct_of(base_config()))
    assert rc == _lib.US_OK
    yield lib, h
    lib.us_hubert_destroy(h)


@pytest.mark.parametrize("cfg", [base_config(), TINY], ids=["base", "tiny"])
def test_create_accepts(cfg):
    lib, h, rc = create(struct_of(cfg))
    assert rc == _lib.US_OK and h
    assert lib.us_hubert_num_weights(h) > 0
    assert lib.us_hubert_destroy(h) == _lib.US_OK


@pytest.mark.parametrize("over", [
    dict(feat_extract_norm=_lib.US_HUBERT_NORM_LAYER),
    dict(do_stable_layer_norm=1),
    dict(n_heads=7),                          # 768 / 7
    dict(n_heads=6),                          # head dimension 128
    dict(hidden_size=72, n_heads=4),          # head dimension 18: not a multiple of 4
    dict(pos_conv_groups=10),                 # 768 / 10
    dict(n_conv=9),
], ids=["layer_norm_extractor", "stable_layer_norm", "heads_do_not_divide", "head_dim_128", "head_dim_18", "groups_do_not_divide", "9_conv_layers"])
def test_create_refuses(over):
    lib, h, rc = create(struct_of(base_config(), **over))
    assert rc == -1 and not h                 # US_EINVAL
    assert b"us_hubert_create" in lib.us_last_error(None)


def test_frames_closed_form(base_handle):
    lib, h = base_handle
    assert lib.us_hubert_frames(h, 399) < 0
    assert b"receptive field (400)" in lib.us_hubert_last_error(h)
    for n, want in ((400, 1), (719, 1), (720, 2), (16000, 49), (32000, 99)):
        assert lib.us_hubert_frames(h, n) == want == frames(base_config(), n), n


def test_workspace_bytes(base_handle):
    lib, h = base_handle
    assert lib.us_hubert_workspace_bytes(h, 0, 16000) == 0
    assert lib.us_hubert_workspace_bytes(h, 1, 399) == 0
    one, two = lib.us_hubert_workspace_bytes(h, 1, 16000), lib.us_hubert_workspace_bytes(h, 2, 16000)
    assert 0 < one < two


def test_forward_refuses_bad_arguments_before_any_launch(base_handle):
    lib, h = base_handle
    dummy = C.c_void_p(256)                   # never dereferenced: every check below comes first
    lens = (C.c_int64 * 2)(16000, 399)
    assert lib.us_hubert_forward(h, dummy, lens, 2, 16000, 0, 12, dummy, None, dummy, 1 << 40, None) == -1
    assert b"lengths[1] = 399" in lib.us_hubert_last_error(h) and b"receptive field" in lib.us_hubert_last_error(h)
    assert lib.us_hubert_forward(h, dummy, None, 1, 16000, 0, 13, dummy, None, dummy, 1 << 40, None) == -1
    assert lib.us_hubert_forward(h, dummy, None, 1, 399, 0, 12, dummy, None, dummy, 1 << 40, None) == -1
    assert lib.us_hubert_forward(h, dummy, None, 1, 16000, 0, 12, dummy, None, dummy, 1 << 40, None) == -4      # US_EWEIGHTS: nothing loaded


@pytest.mark.parametrize("name", ["a", "b"])
def test_keys_match_the_golden_and_transformers(golden, name):
    g = golden("hubert_" + name)
    cfg = json.loads(str(g["config"]))
    m = HubertModel(**cfg)
    keys = list(m.state_dict().keys())
    assert keys == json.loads(str(g["keys"]))
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == g["w:" + k].shape, k
    # the C handle takes the same keys, the weight-norm pair folded and masked_spec_embed left out
    lib, h, rc = create(m._config_struct())
    assert rc == _lib.US_OK
    ckeys = [lib.us_hubert_weight_key(h, i).decode() for i in range(lib.us_hubert_num_weights(h))]
    lib.us_hubert_destroy(h)
    assert set(ckeys) == set(m._sources().keys())
    p = "encoder.pos_conv_embed.conv."
    assert set(ckeys) == (set(keys) - {"masked_spec_embed", p + "parametrizations.weight.original0", p + "parametrizations.weight.original1"}) | {p + "weight"}
    transformers = pytest.importorskip("transformers")
    hf = transformers.HubertModel(transformers.HubertConfig(vocab_size=32, **cfg))
    assert set(keys) == set(hf.state_dict().keys())
    assert set(HubertModel.base().state_dict().keys()) == set(transformers.HubertModel(transformers.HubertConfig()).state_dict().keys())


def golden_state_dict(g):
    return {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_fp64_matches_transformers_goldens(golden, name):
    g = golden("hubert_" + name)
    cfg, sd = json.loads(str(g["config"])), golden_state_dict(g)
    dc = 0
    for i in range(int(g["n_items"])):
        wav, ref = torch.from_numpy(g[f"wav_{i}"]), g[f"hs_{i}"]
        dc += abs(float(wav.mean())) > 0.4
        hs = hubert_forward_torch(sd, cfg, wav[None], None, torch.float64, normalize=bool(g[f"normalize_{i}"]))
        assert len(hs) == ref.shape[0] == cfg["num_hidden_layers"] + 1 and ref.shape[1] == frames(cfg, len(wav))
        for n, x in enumerate(hs):
            assert np.abs(x[0].numpy() - ref[n]).max() <= 1e-10 * np.abs(ref[n]).max(), (i, n)
    assert dc == 1 and sum(int(g[f"normalize_{i}"]) for i in range(4)) == 1


def test_restatement_ragged_batch_equals_items_alone(golden):
    g = golden("hubert_a")
    cfg, sd = json.loads(str(g["config"])), golden_state_dict(g)
    order = (3, 0, 2, 1)
    wavs = [torch.from_numpy(g[f"wav_{i}"]) for i in order]
    batch = torch.full((4, max(len(w) for w in wavs)), float("nan"))
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = w
    for normalize in (False, True):
        got = hubert_forward_torch(sd, cfg, batch, [len(w) for w in wavs], torch.float64, normalize=normalize)
        for b, w in enumerate(wavs):
            alone = hubert_forward_torch(sd, cfg, w[None], None, torch.float64, normalize=normalize)
            f = alone[0].shape[1]
            for n in range(len(alone)):
                assert torch.isfinite(got[n]).all()
                assert (got[n][b, :f] - alone[n][0]).abs().max() <= 1e-12 * alone[n].abs().max()
                assert (got[n][b, f:] == 0).all()


def test_weight_g_spelling_and_final_proj():
    sd = synthetic_hubert_state_dict(TINY, 3)
    p = "encoder.pos_conv_embed.conv."
    old = {k: v for k, v in sd.items() if "parametrizations" not in k and k != "masked_spec_embed"}
    old[p + "weight_g"] = sd[p + "parametrizations.weight.original0"]
    old[p + "weight_v"] = sd[p + "parametrizations.weight.original1"]
    old["final_proj.weight"], old["final_proj.bias"] = torch.zeros(8, 40), torch.zeros(8)
    m = HubertModel(**TINY)
    m.load_state_dict(old)
    back = m.state_dict()
    for k, v in sd.items():
        if k != "masked_spec_embed":
            assert torch.equal(back[k], v), k
    # the folded weight the library is given is the restatement's
    folded = m._sources()[p + "weight"][1]()
    assert torch.allclose(folded, pos_conv_weight(sd), rtol=1e-6, atol=0)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in old.items() if k != p + "bias"})


def test_fairseq_mapping_round_trip():
    sd = synthetic_hubert_state_dict(TINY, 4)
    p = "encoder.pos_conv_embed.conv."
    fs = {"mask_emb": torch.zeros(40), "label_embs_concat": torch.zeros(504, 8), "final_proj.weight": torch.zeros(8, 40), "final_proj.bias": torch.zeros(8)}
    for k, v in sd.items():
        if k == "masked_spec_embed":
            continue
        k = k.replace(p + "parametrizations.weight.original0", "encoder.pos_conv.0.weight_g").replace(p + "parametrizations.weight.original1", "encoder.pos_conv.0.weight_v")
        k = k.replace(p + "bias", "encoder.pos_conv.0.bias")
        k = k.replace("feature_extractor.conv_layers.0.layer_norm.", "feature_extractor.conv_layers.0.2.")
        for i in range(7):
            k = k.replace(f"feature_extractor.conv_layers.{i}.conv.", f"feature_extractor.conv_layers.{i}.0.")
        k = k.replace("feature_projection.layer_norm.", "layer_norm.").replace("feature_projection.projection.", "post_extract_proj.")
        if k.startswith("encoder.layers."):
            k = k.replace(".attention.", ".self_attn.").replace(".feed_forward.intermediate_dense.", ".fc1.").replace(".feed_forward.output_dense.", ".fc2.")
            if ".final_layer_norm." not in k:
                k = k.replace(".layer_norm.", ".self_attn_layer_norm.")
        fs[k] = v
    assert "encoder.layers.1.self_attn_layer_norm.weight" in fs and "encoder.layers.0.fc1.bias" in fs and "layer_norm.weight" in fs
    mapped = from_fairseq_state_dict(fs)
    assert not any(k.startswith(("final_proj", "label_embs", "mask_emb")) for k in mapped)
    m = HubertModel(**TINY)
    m.load_state_dict(mapped)
    back = m.state_dict()
    for k, v in sd.items():
        if k != "masked_spec_embed":
            assert torch.equal(back[k], v), k


def test_no_cpu_fallback_and_no_training():
    m = HubertModel(**TINY).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 800))
    reader = HubertFeatureReader(m, layer=1)
    assert reader.code_hop_size == 320 and reader.expected_sample_rate == 16000
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reader(torch.zeros(800))
    for bad in (dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(num_attention_heads=3)):
        with pytest.raises(ValueError):
            HubertModel(**dict(TINY, **bad))
