"""The WavLM encoder's host side (no GPU): what us_wavlm_create accepts and refuses, the host bucket map, the key list against the goldens
and transformers', the fp64 restatement (tools/wavlm_torch.py) against the goldens written from transformers.WavLMModel, the fairseq key
mapping, and the speaker embedder's upstream attachment and checkpoint loader."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from wavlm_torch import (_relative_positions_bucket, base_plus_config, first_saturated_distance, frames, large_config,  # noqa: E402
                         synthetic_wavlm_state_dict, wavlm_forward_torch)

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.speaker_encoder import ECAPA_TDNN, load_speaker_embedder_checkpoint, synthetic_ecapa_state_dict  # noqa: E402
from unitspeech_amd.wavlm import WavLMModel, from_fairseq_wavlm_state_dict  # noqa: E402

COMMON = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
              intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
              num_buckets=32, max_bucket_distance=40)
TINY_LARGE = dict(COMMON, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
TINY_BASE = dict(COMMON, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)
POS = "encoder.pos_conv_embed.conv."


def struct_of(cfg, **over):
    s = WavLMModel(**cfg)._config_struct()
    for k, v in over.items():
        setattr(s, k, v)
    return s


def create(s):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.us_wavlm_create(C.byref(h), C.byref(s))
    return lib, h, rc


@pytest.mark.parametrize("cfg", [large_config(), base_plus_config(), TINY_LARGE, TINY_BASE], ids=["large", "base_plus", "tiny_large", "tiny_base"])
def test_create_accepts(cfg):
    lib, h, rc = create(struct_of(cfg))
    assert rc == _lib.US_OK and h
    assert lib.us_wavlm_num_weights(h) > 0
    assert lib.us_wavlm_frames(h, 400) == 1 and lib.us_wavlm_frames(h, 32000) == 99 == frames(cfg, 32000)
    assert lib.us_wavlm_frames(h, 399) < 0 and b"receptive field (400)" in lib.us_wavlm_last_error(h)
    assert lib.us_wavlm_workspace_bytes(h, 0, 16000) == 0 and lib.us_wavlm_workspace_bytes(h, 1, 399) == 0
    assert 0 < lib.us_wavlm_workspace_bytes(h, 1, 16000) < lib.us_wavlm_workspace_bytes(h, 2, 16000)
    assert lib.us_wavlm_destroy(h) == _lib.US_OK


@pytest.mark.parametrize("over", [
    dict(feat_extract_norm=_lib.US_HUBERT_NORM_GROUP),                          # group, stable, bias
    dict(do_stable_layer_norm=0),                                               # layer, post-LN, bias
    dict(conv_bias=0),                                                          # layer, stable, no bias
    dict(feat_extract_norm=_lib.US_HUBERT_NORM_GROUP, do_stable_layer_norm=0),  # group, post-LN, bias
    dict(feat_extract_norm=_lib.US_HUBERT_NORM_GROUP, conv_bias=0),             # group, stable, no bias
    dict(do_stable_layer_norm=0, conv_bias=0),                                  # layer, post-LN, no bias
    dict(n_heads=7),                                                            # 1024 / 7
    dict(n_heads=8),                                                            # head dimension 128
    dict(num_buckets=321),
    dict(num_buckets=2),
    dict(max_bucket_distance=80),                                               # not above num_buckets / 4
], ids=["group_stable_bias", "layer_post_bias", "layer_stable_nobias", "group_post_bias", "group_stable_nobias", "layer_post_nobias",
        "heads_do_not_divide", "head_dim_128", "odd_num_buckets", "two_buckets", "max_distance_too_small"])
def test_create_refuses(over):
    lib, h, rc = create(struct_of(large_config(), **over))
    assert rc == -1 and not h                 # US_EINVAL
    assert b"us_wavlm_create" in lib.us_last_error(None)


def test_hubert_create_still_refuses_the_wavlm_forms():
    from unitspeech_amd.hubert import HubertModel
    lib = _lib.load()
    for over in (dict(feat_extract_norm=_lib.US_HUBERT_NORM_LAYER), dict(do_stable_layer_norm=1)):
        s = HubertModel.base()._config_struct()
        for k, v in over.items():
            setattr(s, k, v)
        h = C.c_void_p()
        assert lib.us_hubert_create(C.byref(h), C.byref(s)) == -1 and not h


@pytest.mark.parametrize("buckets,distance,saturated", [(320, 800, 778), (32, 40, 33)])
def test_position_bucket_host_map(buckets, distance, saturated):
    lib, h, rc = create(struct_of(dict(TINY_LARGE, num_buckets=buckets, max_bucket_distance=distance)))
    assert rc == _lib.US_OK
    delta = torch.arange(-2000, 2001)
    got = torch.tensor([lib.us_wavlm_position_bucket(h, int(d)) for d in delta])
    lib.us_wavlm_destroy(h)
    want = _relative_positions_bucket(delta, buckets, distance)
    assert torch.equal(got, want)
    assert first_saturated_distance(buckets, distance) == saturated
    last_neg, last_pos = buckets // 2 - 1, buckets - 1
    assert int(got[2000 - saturated]) == last_neg and int(got[2000 - saturated + 1]) != last_neg
    assert int(got[2000 + saturated]) == last_pos and int(got[2000 + saturated - 1]) != last_pos
    assert (got[:2000 - saturated + 1] == last_neg).all() and (got[2000 + saturated:] == last_pos).all()
    try:
        from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    except ImportError:
        return
    att = WavLMAttention(embed_dim=8, num_heads=2, num_buckets=buckets, max_distance=distance)
    assert torch.equal(got, att._relative_positions_bucket(delta))


def test_forward_refuses_bad_arguments_before_any_launch():
    lib, h, rc = create(struct_of(large_config()))
    assert rc == _lib.US_OK
    dummy = C.c_void_p(256)                   # never dereferenced: every check below comes first
    lens = (C.c_int64 * 2)(16000, 399)
    fh = 49 * 1024
    assert lib.us_wavlm_forward(h, dummy, lens, 2, 16000, 0, 24, dummy, None, 0, 0, dummy, 1 << 40, None) == -1
    assert b"lengths[1] = 399" in lib.us_wavlm_last_error(h) and b"receptive field" in lib.us_wavlm_last_error(h)
    assert lib.us_wavlm_forward(h, dummy, None, 1, 16000, 0, 25, dummy, None, 0, 0, dummy, 1 << 40, None) == -1
    assert b"n_layers_out" in lib.us_wavlm_last_error(h)
    assert lib.us_wavlm_forward(h, dummy, None, 1, 399, 0, 24, dummy, None, 0, 0, dummy, 1 << 40, None) == -1
    # overlapping hidden states: two items one layer apart in the items-outer layout
    assert lib.us_wavlm_forward(h, dummy, None, 2, 16000, 0, 24, dummy, dummy, fh, fh, dummy, 1 << 40, None) == -1
    assert b"strides" in lib.us_wavlm_last_error(h)
    for item, layer in ((25 * fh, fh), (fh, 2 * fh)):                 # both layouts pass the stride check and stop at the missing weights
        assert lib.us_wavlm_forward(h, dummy, None, 2, 16000, 0, 24, dummy, dummy, item, layer, dummy, 1 << 40, None) == -4      # US_EWEIGHTS
    lib.us_wavlm_destroy(h)


@pytest.mark.parametrize("name", ["a", "b"])
def test_keys_shapes_and_order_match_the_golden(golden, name):
    g = golden("wavlm_" + name)
    cfg = json.loads(str(g["config"]))
    m = WavLMModel(**cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == json.loads(str(g["keys"]))
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["shapes"]))
    # the C handle takes the same keys in the same order, the weight-norm pair folded and masked_spec_embed left out
    lib, h, rc = create(m._config_struct())
    assert rc == _lib.US_OK
    ckeys = [lib.us_wavlm_weight_key(h, i).decode() for i in range(lib.us_wavlm_num_weights(h))]
    lib.us_wavlm_destroy(h)
    assert set(ckeys) == set(m._sources().keys())
    want = [k for k in sd if k != "masked_spec_embed" and "parametrizations" not in k]
    want.insert(want.index(POS + "bias") + 1, POS + "weight")
    assert ckeys == want
    transformers = pytest.importorskip("transformers")
    hf = transformers.WavLMModel(transformers.WavLMConfig(vocab_size=32, **cfg))
    assert list(sd.keys()) == list(hf.state_dict().keys())


def test_large_and_base_plus_shapes():
    m = WavLMModel.large()
    sd = m.state_dict()
    assert m.config["num_hidden_layers"] == 24 and len([k for k in sd if k.endswith("attention.q_proj.weight")]) == 24
    assert tuple(sd["encoder.layers.23.attention.q_proj.weight"].shape) == (1024, 1024)
    assert tuple(sd["encoder.layers.23.feed_forward.intermediate_dense.weight"].shape) == (4096, 1024)
    assert tuple(sd["encoder.layers.0.attention.rel_attn_embed.weight"].shape) == (320, 16)
    assert tuple(sd["encoder.layers.5.attention.gru_rel_pos_linear.weight"].shape) == (8, 64)
    assert tuple(sd["encoder.layers.5.attention.gru_rel_pos_const"].shape) == (1, 16, 1, 1)
    assert tuple(sd["feature_extractor.conv_layers.6.conv.bias"].shape) == (512,) and "feature_extractor.conv_layers.6.layer_norm.weight" in sd
    assert "encoder.layers.1.attention.rel_attn_embed.weight" not in sd
    b = WavLMModel.base_plus().state_dict()
    assert tuple(b["encoder.layers.11.attention.q_proj.weight"].shape) == (768, 768) and "feature_extractor.conv_layers.0.conv.bias" not in b
    assert "feature_extractor.conv_layers.1.layer_norm.weight" not in b


def golden_state_dict(g):
    return {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_fp64_matches_transformers_goldens(golden, name):
    g = golden("wavlm_" + name)
    cfg, sd = json.loads(str(g["config"])), golden_state_dict(g)
    for i in range(int(g["n_items"])):
        wav, ref = torch.from_numpy(g[f"wav_{i}"]), g[f"hs_{i}"]
        hs = wavlm_forward_torch(sd, cfg, wav[None], None, torch.float64, normalize=bool(g[f"normalize_{i}"]))
        assert len(hs) == ref.shape[0] == cfg["num_hidden_layers"] + 1 and ref.shape[1] == frames(cfg, len(wav))
        for n, x in enumerate(hs):
            assert np.abs(x[0].numpy() - ref[n]).max() <= 1e-10 * np.abs(ref[n]).max(), (i, n)
    assert g["hs_3"].shape[1] == 71 > first_saturated_distance(cfg["num_buckets"], cfg["max_bucket_distance"]) and int(g["normalize_3"]) == 1


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_ragged_batch_and_output_layer(golden, name):
    g = golden("wavlm_" + name)
    cfg, sd = json.loads(str(g["config"])), golden_state_dict(g)
    wavs = [torch.from_numpy(g[f"wav_{i}"]) for i in (2, 0, 1)]
    batch = torch.full((3, max(len(w) for w in wavs)), float("nan"))
    for b, w in enumerate(wavs):
        batch[b, :len(w)] = w
    got = wavlm_forward_torch(sd, cfg, batch, [len(w) for w in wavs], torch.float64, normalize=True)
    for b, w in enumerate(wavs):
        alone = wavlm_forward_torch(sd, cfg, w[None], None, torch.float64, normalize=True)
        f = alone[0].shape[1]
        for n in range(len(alone)):
            assert torch.isfinite(got[n]).all()
            assert (got[n][b, :f] - alone[n][0]).abs().max() <= 1e-12 * alone[n].abs().max()
            assert (got[n][b, f:] == 0).all()
    # hidden state n < L of a shorter run is the full run's (un-normalised in the pre-LN form); state L is normalised there
    full = wavlm_forward_torch(sd, cfg, wavs[0][None], None, torch.float64)
    one = wavlm_forward_torch(sd, cfg, wavs[0][None], None, torch.float64, n_layers_out=1)
    assert len(one) == 2 and torch.equal(one[0], full[0]) and torch.equal(one[1], full[1])


@pytest.mark.parametrize("cfg", [TINY_LARGE, TINY_BASE], ids=["large_form", "base_form"])
def test_synthetic_state_dict_has_the_models_keys_off_their_initial_values(cfg):
    sd = synthetic_wavlm_state_dict(cfg, 3)
    ref = WavLMModel(**cfg).state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
        if k.endswith(".bias") or "layer_norm" in k or k.endswith("gru_rel_pos_const") or k.endswith("rel_attn_embed.weight"):
            assert not torch.equal(v, ref[k]), k


def to_fairseq(sd, ln_spelling):
    fs = {"mask_emb": torch.zeros(40), "label_embs_concat": torch.zeros(504, 8), "final_proj.weight": torch.zeros(8, 40), "final_proj.bias": torch.zeros(8)}
    for k, v in sd.items():
        if k == "masked_spec_embed":
            continue
        k = k.replace(POS + "parametrizations.weight.original0", "encoder.pos_conv.0.weight_g").replace(POS + "parametrizations.weight.original1", "encoder.pos_conv.0.weight_v")
        k = k.replace(POS + "bias", "encoder.pos_conv.0.bias")
        for i in range(7):
            k = k.replace(f"feature_extractor.conv_layers.{i}.layer_norm.", f"feature_extractor.conv_layers.{i}.{ln_spelling}.")
            k = k.replace(f"feature_extractor.conv_layers.{i}.conv.", f"feature_extractor.conv_layers.{i}.0.")
        k = k.replace("feature_projection.layer_norm.", "layer_norm.").replace("feature_projection.projection.", "post_extract_proj.")
        if k.startswith("encoder.layers."):
            k = k.replace(".attention.gru_rel_pos_linear.", ".self_attn.grep_linear.").replace(".attention.gru_rel_pos_const", ".self_attn.grep_a")
            k = k.replace(".attention.rel_attn_embed.", ".self_attn.relative_attention_bias.")
            k = k.replace(".attention.", ".self_attn.").replace(".feed_forward.intermediate_dense.", ".fc1.").replace(".feed_forward.output_dense.", ".fc2.")
            if ".final_layer_norm." not in k:
                k = k.replace(".layer_norm.", ".self_attn_layer_norm.")
        fs[k] = v
    return fs


@pytest.mark.parametrize("ln_spelling", ["2", "2.1"])
@pytest.mark.parametrize("cfg", [TINY_LARGE, TINY_BASE], ids=["large_form", "base_form"])
def test_fairseq_mapping_round_trip(cfg, ln_spelling):
    sd = synthetic_wavlm_state_dict(cfg, 4)
    fs = to_fairseq(sd, ln_spelling)
    assert "encoder.layers.1.self_attn.grep_a" in fs and "encoder.layers.0.self_attn.relative_attention_bias.weight" in fs
    assert "encoder.layers.1.self_attn.grep_linear.bias" in fs and f"feature_extractor.conv_layers.0.{ln_spelling}.weight" in fs
    assert ("feature_extractor.conv_layers.3.0.bias" in fs) == cfg["conv_bias"]
    mapped = from_fairseq_wavlm_state_dict(fs)
    assert not any(k.startswith(("final_proj", "label_embs", "mask_emb")) for k in mapped)
    m = WavLMModel(**cfg)
    m.load_state_dict(mapped)
    back = m.state_dict()
    for k, v in sd.items():
        if k != "masked_spec_embed":
            assert torch.equal(back[k], v), k


def test_no_cpu_fallback_and_constructor_refusals():
    m = WavLMModel(**TINY_LARGE).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 800))
    for bad in (dict(feat_extract_norm="group"), dict(do_stable_layer_norm=False), dict(conv_bias=False), dict(num_attention_heads=3)):
        with pytest.raises(ValueError):
            WavLMModel(**dict(TINY_LARGE, **bad))


SPK = dict(feat_dim=40, channels=16, emb_dim=8, global_context_att=False, n_layers=3)


def tiny_trunk():
    m = ECAPA_TDNN(feat_dim=40, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(SPK, 1).items()})
    return m.eval()


def test_upstream_attachment_leaves_the_trunk_as_it_is():
    m = tiny_trunk()
    with pytest.raises(NotImplementedError, match=r"(?s)upstream.*forward_features"):
        m(torch.zeros(1, 16000))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="hidden states"):
        m.attach_upstream(WavLMModel(**dict(TINY_LARGE, num_hidden_layers=3)))
    w = WavLMModel(**TINY_LARGE)
    assert m.attach_upstream(w) is m and m.upstream is w and not w.training
    after = m.state_dict()
    assert list(after.keys()) == list(before.keys()) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any("upstream" in n for n, _ in m.named_modules()) and len(list(m.parameters())) == len([k for k in before if "running" not in k and "num_batches" not in k])
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # the upstream is reached: it refuses the CPU tensor itself
        m(torch.zeros(1, 16000))
    with pytest.raises(ValueError, match="one utterance"):
        m.embed_wav(torch.zeros(2, 16000))


@pytest.mark.parametrize("cfg", [TINY_LARGE, TINY_BASE], ids=["large_form", "base_form"])
def test_load_speaker_embedder_checkpoint(tmp_path, cfg):
    trunk = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(SPK, 2).items()}
    up = synthetic_wavlm_state_dict(cfg, 6)
    ck = dict(trunk)
    ck.update({"feature_extract.model." + k: v for k, v in to_fairseq(up, "2.1").items()})
    path = os.path.join(tmp_path, "embedder.pt")
    torch.save({"model": ck}, path)
    m = load_speaker_embedder_checkpoint(path, max_bucket_distance=40)
    w = m.upstream
    assert w is not None and not m.training and not w.training
    assert {k: w.config[k] for k in cfg} == cfg                        # every size, and the form, inferred from the shapes
    assert m._upstream_normalize == (cfg["feat_extract_norm"] == "layer")
    assert (m.feat_dim, m.channels[0], m.emb_dim, m.feat_num) == (40, 16, 8, 3)
    for k, v in up.items():
        if k != "masked_spec_embed":
            assert torch.equal(w.state_dict()[k], v), k
    assert list(m.state_dict().keys()) == list(trunk.keys()) and all(torch.equal(m.state_dict()[k], v) for k, v in trunk.items())
    # a file without the upstream is pointed to the trunk's own loader
    bare = os.path.join(tmp_path, "trunk.pt")
    torch.save({"model": trunk}, bare)
    with pytest.raises(ValueError, match="load_speaker_encoder_checkpoint"):
        load_speaker_embedder_checkpoint(bare)
