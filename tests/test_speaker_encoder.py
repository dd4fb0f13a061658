"""ECAPA-TDNN speaker encoder, CPU side: the torch restatement (tools/speaker_encoder_torch.py) against the reference goldens and their
intermediates, the module's state_dict against the reference's key lists for both feat_type families, the checkpoint loader, and the
C ABI's key list and refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.speaker_encoder import (ECAPA_TDNN, ECAPA_TDNN_SMALL, load_speaker_encoder_checkpoint, synthetic_ecapa_state_dict,  # noqa: E402
                                            synthetic_hidden_states)

CASES = ["speaker_tiny", "speaker_tiny_gca", "speaker_full", "speaker_full_long"]
STAGES = ["feat", "layer1", "layer2", "layer3", "layer4", "pooling"]


def _inputs(g):
    cfg, seed = json.loads(str(g["config"])), int(g["seed"])
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, seed).items()}
    hid = synthetic_hidden_states(cfg["n_layers"], int(g["B"]), int(g["T"]), cfg["feat_dim"], seed)
    return cfg, sd, torch.from_numpy(hid)


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_golden(golden, name):
    """fp64 against the reference's fp64: the same operations in another grouping, so rounding at 1e-16 relative through ~15 layers of
    O(1..100) activations: 1e-10 is the bar.  fp32: within ten times the reference's own fp32 - fp64 distance."""
    g = golden(name)
    cfg, sd, hid = _inputs(g)
    if "hidden" in g:
        assert np.array_equal(hid.numpy(), g["hidden"])
    stages = {}
    with torch.no_grad():
        e64 = ecapa_forward(cfg, sd, hid, dtype=torch.float64, stages=stages).numpy()
        e32 = ecapa_forward(cfg, sd, hid).numpy()
    assert e64.shape == g["emb64"].shape == (int(g["B"]), cfg["emb_dim"])
    floor = float(np.abs(g["emb32"] - g["emb64"]).max())
    d64, d32 = float(np.abs(e64 - g["emb64"]).max()), float(np.abs(e32.astype(np.float64) - g["emb64"]).max())
    print(f"\n{name}: restatement fp64 {d64:.2e}, fp32 {d32:.2e}; reference fp32 floor {floor:.2e}")
    assert d64 <= 1e-10
    assert d32 <= 10 * floor
    assert 0.05 < np.abs(g["emb64"]).max() < 5.0
    for s in STAGES:
        if s in g:
            assert np.abs(stages[s].numpy() - g[s]).max() <= 1e-10, s


def _keys(sd):
    return [str(k) for k in sd], [",".join(str(s) for s in t.shape) for t in sd.values()]


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_shapes_and_order_match_the_reference(golden, name):
    g = golden(name)
    cfg = json.loads(str(g["config"]))
    kw = dict(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"], global_context_att=cfg["global_context_att"])
    m = ECAPA_TDNN(feat_type="wavlm_large", feat_num=cfg["n_layers"], config_path="unused", **kw)
    keys, shapes = _keys(m.state_dict())
    assert keys == list(g["keys"]) and shapes == list(g["shapes"])
    assert len(keys) == 222 and keys[0] == "feature_weight" and sum(k.endswith("num_batches_tracked") for k in keys) == 29
    assert list(synthetic_ecapa_state_dict(cfg, 0)) == keys
    for feat_type in ("fbank", "mfcc"):
        keys, shapes = _keys(ECAPA_TDNN(feat_type=feat_type, **kw).state_dict())
        assert keys == list(g["keys_fbank"]) and shapes == list(g["shapes_fbank"]) and len(keys) == 221


def test_small_constructor_and_upstream_layer_counts():
    m = ECAPA_TDNN_SMALL(feat_dim=1024, emb_dim=256, feat_type="wavlm_large")
    assert m.feature_weight.shape == (25,) and m.layer1.conv.weight.shape == (512, 1024, 5) and m.linear.weight.shape == (256, 3072)
    assert ECAPA_TDNN_SMALL(feat_dim=768, feat_type="hubert_base").feature_weight.shape == (13,)
    with pytest.raises(ValueError, match="feat_num"):
        ECAPA_TDNN(feat_type="some_upstream")
    with pytest.raises(ValueError, match="multiple of 8"):
        ECAPA_TDNN(channels=12)


def test_forward_needs_the_upstream_and_a_device():
    m = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)
    with pytest.raises(NotImplementedError, match="forward_features") as e:
        m(torch.zeros(1, 16000))
    assert "upstream" in str(e.value)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.forward_features(torch.zeros(3, 1, 5, 16))
    with pytest.raises(ValueError, match="hidden states"):
        m.forward_features(torch.zeros(4, 1, 5, 16))
    with pytest.raises(ValueError, match="combined"):
        ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8).forward_features(torch.zeros(3, 1, 5, 16))
    with pytest.raises(ValueError, match="one utterance"):
        m.embed(torch.zeros(3, 2, 5, 16))


def test_checkpoint_loader_drops_the_upstream_and_is_strict(tmp_path):
    cfg = {"feat_dim": 1024, "channels": 512, "emb_dim": 256, "global_context_att": False, "n_layers": 25}
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, 4).items()}
    full = dict(sd)
    full["feature_extract.model.encoder.layers.0.self_attn.k_proj.weight"] = torch.zeros(4, 4)
    full["feature_extract.model.mask_emb"] = torch.zeros(4)
    torch.save({"model": full}, tmp_path / "embedder.pt")
    m = load_speaker_encoder_checkpoint(str(tmp_path / "embedder.pt"))
    assert not m.training and list(m.state_dict()) == list(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    short = {k: v for k, v in full.items() if k != "layer3.SE_Connect.linear2.bias"}
    torch.save({"model": short}, tmp_path / "short.pt")
    with pytest.raises(RuntimeError, match="layer3.SE_Connect.linear2.bias"):
        load_speaker_encoder_checkpoint(str(tmp_path / "short.pt"))
    extra = dict(full)
    extra["layer2.shortcut.weight"] = torch.zeros(512, 512, 1)
    torch.save({"model": extra}, tmp_path / "shortcut.pt")
    with pytest.raises(RuntimeError, match="shortcut"):
        load_speaker_encoder_checkpoint(str(tmp_path / "shortcut.pt"))


def test_library_key_list_and_refusals():
    """The C ABI's own checks (no device work is launched): the key list is the module's floating-point state_dict, and sizes the
    kernels do not cover are refused at create."""
    lib = _lib.load()
    for gca in (False, True):
        m = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, global_context_att=gca, feat_type="wavlm_large", feat_num=3)
        h = C.c_void_p()
        c = m._config_struct()
        assert lib.us_speaker_create(C.byref(h), C.byref(c)) == 0
        n = lib.us_speaker_num_weights(h)
        keys = [lib.us_speaker_weight_key(h, i).decode() for i in range(n)]
        assert keys == list(m._sources()) and n == 222 - 29
        assert lib.us_speaker_workspace_bytes(h, 2, 23) > 4 * 2 * 23 * (16 + 7 * 16 + 2 * 1536 + 128)
        lib.us_speaker_destroy(h)
    h = C.c_void_p()
    for field, value in (("channels", 12), ("channels", 1024), ("feat_dim", 0), ("n_layers", 65), ("global_context_att", 2)):
        bad = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8)._config_struct()
        setattr(bad, field, value)
        assert lib.us_speaker_create(C.byref(h), C.byref(bad)) == -1, field
    assert b"multiple of 8" in lib.us_speaker_last_error(None) or b"bad" in lib.us_speaker_last_error(None)
    assert C.sizeof(_lib.us_speaker_config) == 5 * 4


def test_debug_conv_refuses_bad_arguments_before_any_device_work():
    """us_speaker_debug_conv: null and non-positive arguments, an unknown activation, convolution or BatchNorm, a BatchNorm with fewer
    channels than the convolution, batch strides shorter than the tensors, sizes past the kernel's limits, and (last) weights that were
    never loaded."""
    lib = _lib.load()
    h = C.c_void_p()
    c = ECAPA_TDNN(feat_dim=13, channels=40, emb_dim=7, global_context_att=True, feat_type="wavlm_large", feat_num=2)._config_struct()
    assert lib.us_speaker_create(C.byref(h), C.byref(c)) == 0
    p = 4096                     # never dereferenced: every call below is refused on the host
    EINVAL, ENOKEY, EWEIGHTS = -1, -2, -4
    call = lib.us_speaker_debug_conv
    T = 9
    ok = dict(h=h, prefix=b"layer1.conv", bn=b"layer1.bn", act=1, x=p, in_bs=13 * T, out=p, out_bs=40 * T, bias2=None, B=2, T=T)

    def run(**kw):
        a = dict(ok, **kw)
        return call(a["h"], a["prefix"], a["bn"], a["act"], a["x"], a["in_bs"], a["out"], a["out_bs"], a["bias2"], a["B"], a["T"], None)

    for kw in (dict(h=None), dict(prefix=None), dict(x=None), dict(out=None), dict(B=0), dict(T=0), dict(T=-3), dict(act=3), dict(act=-1)):
        assert run(**kw) == EINVAL, kw
    for bad in (b"", b"layer1", b"layer1.conv.weight", b"layer2.Res2Conv1dReluBn.convs.0", b"layer5.Conv1dReluBn1.conv", b"linear"):
        assert run(prefix=bad) == ENOKEY, bad
    for bad in (b"layer1", b"layer2.Res2Conv1dReluBn.bns.0", b"bn.weight"):
        assert run(bn=bad) == ENOKEY, bad
        assert bad in lib.us_speaker_last_error(h)
    assert run(prefix=b"conv", bn=b"layer1.bn", in_bs=120 * T, out_bs=1536 * T) == EINVAL          # 40 BatchNorm channels for 1536
    assert b"fewer channels" in lib.us_speaker_last_error(h)
    assert run(in_bs=13 * T - 1) == EINVAL and run(out_bs=40 * T - 1) == EINVAL
    assert b"stride" in lib.us_speaker_last_error(h)
    assert run(prefix=b"pooling.linear1", bn=None, in_bs=1536 * T - 1, out_bs=128 * T) == EINVAL   # Cin is 1536 of the weight's 4608
    assert run(B=65536) == EINVAL
    big = 1 << 26
    assert run(T=big, in_bs=13 * big, out_bs=40 * big) == EINVAL                                  # 40 * 2^26 >= 2^31
    # everything in order: the next check is the weights
    assert run() == EWEIGHTS and run(bn=None, act=0) == EWEIGHTS and run(bn=b"") == EWEIGHTS
    assert run(in_bs=100 * T, out_bs=120 * T) == EWEIGHTS                                         # channel slices of wider tensors
    assert run(prefix=b"pooling.linear1", bn=b"bn", act=2, in_bs=1536 * T, out_bs=128 * T, bias2=p) == EWEIGHTS
    lib.us_speaker_destroy(h)
