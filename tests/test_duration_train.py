"""Training side of the DurationPredictor, CPU checks: the torch restatement (tools/duration_torch.py) against the reference goldens
of tools/make_goldens_tts_train.py, the host-side surface of the new C entry points (no device work is launched) and the speaker swap."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import duration_torch as DT  # noqa: E402
from unitspeech_amd import _lib
from unitspeech_amd.encoder import DurationPredictor, DurationPredictorConfig, synthetic_duration_predictor_state_dict

TINY = DurationPredictorConfig(in_channels=16, filter_channels=24, kernel_size=3, spk_emb_dim=12)
FULL = DurationPredictorConfig()
NEW = ("us_duration_predictor_train_workspace_bytes", "us_duration_predictor_forward_train", "us_duration_predictor_backward",
       "us_duration_predictor_dropout_mask", "us_duration_predictor_tape_release", "us_duration_predictor_mse_loss")


def full_golden(golden):
    """duration_train_full and the convolution-weight gradients kept in files of their own (a committed file stays below 1 MiB)."""
    g = dict(golden("duration_train_full"))
    g["g64/conv_1.weight"] = np.concatenate([golden("duration_train_full_p1")["g64/conv_1.weight"],
                                             golden("duration_train_full_p2")["g64/conv_1.weight"]])
    g["g64/conv_2.weight"] = golden("duration_train_full_p3")["g64/conv_2.weight"]
    return g


def restatement(cfg, g, dtype):
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in synthetic_duration_predictor_state_dict(cfg, 0).items()}
    T = lambda k: torch.from_numpy(g[k]).to(dtype)
    logw = DT.duration_forward(sd, T("x"), T("x_mask"), T("g"))
    loss = DT.duration_mse(logw, T("w"), T("x_mask"))
    loss.backward()
    return logw.detach(), loss.detach(), {k: v.grad for k, v in sd.items()}


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def test_restatement_matches_the_reference_tiny_golden_in_fp64(golden):
    g = golden("duration_train_tiny")
    logw, loss, grads = restatement(TINY, g, torch.float64)
    np.testing.assert_allclose(logw.numpy(), g["logw64"], atol=1e-12)
    assert abs(float(loss) - float(g["loss64"])) <= 1e-9 * abs(float(g["loss64"]))
    assert len(grads) == 10
    for k, v in grads.items():
        assert rel(v, g["g64/" + k]) <= 1e-9, k


def test_restatement_matches_the_reference_full_golden(golden):
    g = full_golden(golden)
    logw, loss, grads = restatement(FULL, g, torch.float64)
    np.testing.assert_allclose(logw.numpy(), g["logw"], atol=2e-6)
    assert abs(float(loss) - float(g["loss"])) <= 1e-9 * abs(float(g["loss"]))
    assert len(grads) == 10
    for k, v in grads.items():
        assert abs(float(v.norm()) - float(g["norm/" + k])) <= 1e-9 * float(g["norm/" + k]), k
        assert rel(v, g["g64/" + k]) <= 1e-6, k        # the golden is fp64 rounded once to fp32 (6e-8)


def test_restatement_dropout_masks_are_applied_at_both_sites():
    sd = {k: torch.from_numpy(v).double() for k, v in synthetic_duration_predictor_state_dict(TINY, 0).items()}
    x, m, g = torch.randn(2, 16, 9).double(), torch.ones(2, 1, 9).double(), torch.randn(2, 1, 12).double()
    base = DT.duration_forward(sd, x, m, g)
    for site in (0, 1):
        assert torch.equal(DT.duration_forward(sd, x, m, g, {site: torch.ones(2, 24, 9)}), base)
        keep = (torch.rand(2, 24, 9) > 0.5).double() * 2
        assert not torch.allclose(DT.duration_forward(sd, x, m, g, {site: keep}), base)


def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "unitspeech_hip.h")).read()
    for s in NEW:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert s + "(" in header, s


def test_c_abi_refuses_bad_arguments_without_device_work():
    lib = _lib.load()
    assert lib.us_duration_predictor_train_workspace_bytes(None, 1, 1) == 0
    assert lib.us_duration_predictor_forward_train(None, None, None, None, None, 1, 1, 0.1, 0, None, 0, None) == -1
    assert lib.us_duration_predictor_backward(None, None, 1, 1, None, None, 0, None, 0, None) == -1
    assert lib.us_duration_predictor_dropout_mask(None, 0, 0, 1, 1, 0.1, None, None) == -1
    assert lib.us_duration_predictor_tape_release(None, None) == -1
    assert lib.us_duration_predictor_mse_loss(None, None, None, None, None, 1, 1, None) == -1
    h, e = C.c_void_p(), C.c_void_p()
    c = _lib.us_duration_config(TINY.in_channels, TINY.filter_channels, TINY.kernel_size, TINY.spk_emb_dim)
    assert lib.us_duration_predictor_create(C.byref(h), C.byref(c)) == 0
    ec = _lib.us_encoder_config(20, 8, 16, 32, 2, 2, 3, 4)
    assert lib.us_encoder_create(C.byref(e), C.byref(ec)) == 0
    try:
        small = lib.us_duration_predictor_train_workspace_bytes(h, 1, 8)
        assert 0 < small < lib.us_duration_predictor_train_workspace_bytes(h, 2, 8) < lib.us_duration_predictor_train_workspace_bytes(h, 2, 16)
        assert lib.us_duration_predictor_train_workspace_bytes(h, 0, 8) == 0
        assert lib.us_duration_predictor_train_workspace_bytes(e, 1, 8) == 0          # an Encoder handle
        # weights are not loaded: refused with the Encoder's code before anything is launched
        assert lib.us_duration_predictor_forward_train(h, None, None, None, None, 1, 8, 0.1, 0, None, 0, None) == -4
        assert lib.us_duration_predictor_backward(h, None, 1, 8, None, None, 0, None, 0, None) == -4
        assert lib.us_duration_predictor_forward_train(e, None, None, None, None, 1, 8, 0.1, 0, None, 0, None) == -1
        assert lib.us_duration_predictor_dropout_mask(h, 0, 2, 1, 8, 0.1, None, None) == -1
        assert lib.us_duration_predictor_tape_release(h, None) == 0
        assert lib.us_duration_predictor_tape_release(e, None) == -1
        assert lib.us_encoder_tape_release(h, None) == -1                               # unchanged: Encoder handles only
        # the sentences themselves, whole
        err = lambda hh: lib.us_frontend_last_error(hh).decode()
        p = 4096                                   # a non-null address that must never be read
        fwd = lambda hh, B=1, L=8: lib.us_duration_predictor_forward_train(hh, None, None, None, None, B, L, 0.1, 0, None, 0, None)
        bwd = lambda hh, B=1, L=8: lib.us_duration_predictor_backward(hh, None, B, L, None, None, 0, None, 0, None)
        msk = lambda hh, site=0, pd=0.1, out=p: lib.us_duration_predictor_dropout_mask(hh, 0, site, 1, 8, pd, out, None)
        assert fwd(h) == -4 and err(h) == "us_duration_predictor_forward_train: weight 'conv_1.weight' has not been loaded"
        assert bwd(h) == -4 and err(h) == "us_duration_predictor_backward: weight 'conv_1.weight' has not been loaded"
        for B, L in ((0, 8), (1, 0), (65536, 8), (1, 65536)):
            assert fwd(h, B, L) == -1 and err(h) == "us_duration_predictor_forward_train: bad B or L"
            assert bwd(h, B, L) == -1 and err(h) == "us_duration_predictor_backward: bad B or L"
        for site in (2, -1):
            assert msk(h, site=site) == -1 and err(h) == "us_duration_predictor_dropout_mask: no such site"
        for pd in (1.0, float("nan")):
            assert msk(h, pd=pd) == -1 and err(h) == "us_duration_predictor_dropout_mask: p_dropout must be below 1"
        assert msk(h, out=None) == -1 and err(h) == "us_duration_predictor_dropout_mask: bad argument"
        for hh in (e, None):                       # an Encoder handle, and none at all (the sentence is then the library's last error)
            assert fwd(hh) == -1 and err(hh) == "us_duration_predictor_forward_train: not a duration-predictor handle"
            assert bwd(hh) == -1 and err(hh) == "us_duration_predictor_backward: not a duration-predictor handle"
            assert lib.us_duration_predictor_tape_release(hh, None) == -1
            assert err(hh) == "us_duration_predictor_tape_release: not a duration-predictor handle"
            assert msk(hh) == -1 and err(hh) == "us_duration_predictor_dropout_mask: bad argument"
            assert lib.us_duration_predictor_forward(hh, None, None, None, None, 1, 8, None, 0, None) == -1
            assert err(hh) == "us_duration_predictor_forward: not a duration-predictor handle"
            assert lib.us_duration_predictor_train_workspace_bytes(hh, 1, 8) == 0
        assert lib.us_encoder_tape_release(h, None) == -1 and err(h) == "us_encoder_tape_release: not an encoder handle"
        # workspace sizes in bytes, as the library gave them before the layout took its offsets from handle.h's WsTake
        for (B, L), want in {(1, 8): 135680, (3, 19): 165376, (4, 60): 273664}.items():
            assert lib.us_duration_predictor_train_workspace_bytes(h, B, L) == want, (B, L)
    finally:
        lib.us_frontend_destroy(h)
        lib.us_frontend_destroy(e)


def test_trainable_is_keyword_only_and_train_mode_needs_it():
    with pytest.raises(TypeError):
        DurationPredictor(16, 24, 3, 0.1, 12, True)
    assert DurationPredictor(16, 24, 3, 0.1, spk_emb_dim=12, trainable=True).trainable
    dp = DurationPredictor(16, 24, 3, 0.1, spk_emb_dim=12).train()
    assert dp.trainable is False
    with pytest.raises(RuntimeError, match="inference-only"):
        dp._sync(torch.device("cuda"))
    with pytest.raises(NotImplementedError):
        dp.eval()(torch.zeros(1, 16, 4), torch.ones(1, 1, 4), w=torch.ones(1, 1, 4), g=torch.zeros(1, 1, 12))


def test_speaker_swap_picks_the_reference_items_and_leaves_its_input_untouched():
    from unitspeech_amd.tts_train import random_replace_tensor
    for B, seed in ((8, 3), (32, 11), (3, 0)):
        spk = torch.randn(B, 1, 6)
        keep = spk.clone()
        uncond = torch.full((1, 6), 7.0)
        torch.manual_seed(seed)
        out = random_replace_tensor(spk, uncond)
        torch.manual_seed(seed)
        idx = torch.randperm(B)[:int(B * 0.25)]            # util.random_replace_tensor, :224-231
        want = keep.clone()
        for i in idx:
            want[i] = uncond
        assert torch.equal(out, want) and torch.equal(spk, keep)
        assert int((out == 7.0).all(-1).sum()) == int(B * 0.25)
