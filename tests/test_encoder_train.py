"""Training side of the Encoder, CPU checks: the torch restatement (tools/encoder_torch.py) against the reference goldens of
tools/make_goldens_encoder_train.py, and the host-side surface of the new C entry points (no device work is launched)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import encoder_torch as ET  # noqa: E402
from unitspeech_amd import _lib
from unitspeech_amd.encoder import Encoder, EncoderConfig, encoder_state_shapes, synthetic_encoder_state_dict

TINY = EncoderConfig(n_vocab=50, n_feats=16, n_channels=32, filter_channels=64, n_heads=2, n_layers=2, kernel_size=3, window_size=4)
FULL = EncoderConfig(n_vocab=1000)


def sd_of(cfg, dtype, requires_grad=True):
    return {k: torch.from_numpy(v).to(dtype).requires_grad_(requires_grad) for k, v in synthetic_encoder_state_dict(cfg, 0).items()}


def restatement_grads(cfg, g, dtype):
    sd = sd_of(cfg, dtype)
    ids, lens = torch.from_numpy(g["ids"]), torch.from_numpy(g["lengths"])
    mu_x, x, x_mask = ET.encoder_forward(sd, cfg.n_heads, ids, lens)
    loss = (mu_x * torch.from_numpy(g["g_mu"]).to(dtype)).sum() + (x * torch.from_numpy(g["g_x"]).to(dtype)).sum()
    loss.backward()
    return mu_x.detach(), x.detach(), x_mask, {k: v.grad for k, v in sd.items()}


def rel(a, b, floor=1e-12):
    """|a - b| / |b|; `floor` bounds the denominator for keys whose true gradient is zero (the key bias: softmax is invariant to
    a score shift along a row), where only round-off remains."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(floor))


def test_restatement_matches_the_reference_tiny_golden_in_fp64_and_fp32(golden):
    g = golden("encoder_train_tiny")
    mu_x, x, x_mask, grads = restatement_grads(TINY, g, torch.float64)
    np.testing.assert_allclose(mu_x.numpy(), g["mu_x"], atol=1e-5)        # golden forward outputs are the fp32 run
    np.testing.assert_allclose(x.numpy(), g["x"], atol=1e-5)
    np.testing.assert_array_equal(x_mask.numpy(), g["x_mask"])
    assert list(grads) == list(encoder_state_shapes(TINY))
    for k, v in grads.items():
        assert rel(v, g["g64/" + k], 1e-3) <= 1e-10, k
    _, _, _, grads32 = restatement_grads(TINY, g, torch.float32)
    for k, v in grads32.items():
        if np.linalg.norm(g["g64/" + k]) < 1e-10:         # analytically zero (key bias): only fp32 round-off on both sides
            assert float(v.norm()) < 1e-4 and np.linalg.norm(g["g32/" + k]) < 1e-4, k
            continue
        spread = rel(g["g32/" + k], g["g64/" + k], 1e-3)    # the reference's own fp32-vs-fp64 distance for this key
        assert spread <= 1e-5, k
        assert rel(v, g["g64/" + k], 1e-3) <= max(10 * spread, 1e-6), k


def test_restatement_matches_the_reference_full_golden(golden):
    g = golden("encoder_train_full")
    mu_x, x, _, grads = restatement_grads(FULL, g, torch.float64)
    np.testing.assert_allclose(mu_x.numpy(), g["mu_x"], atol=2e-5)
    np.testing.assert_allclose(x.numpy(), g["x"], atol=2e-5)
    for k, v in grads.items():
        assert abs(float(v.norm()) - float(g["norm/" + k])) <= 1e-9 * max(float(g["norm/" + k]), 1e-3), k
        if "g64/" + k in g:
            assert rel(v, g["g64/" + k]) <= 1e-6, k


def test_restatement_dropout_masks_are_applied_at_every_site():
    """A mask at each site changes the outputs; the identity mask does not (the site numbering of the header)."""
    cfg = TINY
    sd = sd_of(cfg, torch.float64, requires_grad=False)
    ids, lens = torch.randint(0, cfg.n_vocab, (2, 9)), torch.LongTensor([9, 6])
    base = ET.encoder_forward(sd, cfg.n_heads, ids, lens)[0]
    shapes = {0: (2, 32, 9), 1: (2, 32, 9), 2: (2, 32, 9)}
    for i in range(cfg.n_layers):
        s = 3 + 4 * i
        shapes.update({s: (2, 2, 9, 9), s + 1: (2, 32, 9), s + 2: (2, 64, 9), s + 3: (2, 32, 9)})
    for site, shape in shapes.items():
        one = ET.encoder_forward(sd, cfg.n_heads, ids, lens, {site: torch.ones(shape)})[0]
        assert torch.equal(one, base), site
        m = (torch.rand(shape) > 0.5).double() * 2
        assert not torch.allclose(ET.encoder_forward(sd, cfg.n_heads, ids, lens, {site: m})[0], base), site


def test_c_abi_new_entry_points_refuse_bad_arguments_without_device_work():
    lib = _lib.load()
    for s in ("us_encoder_train_workspace_bytes", "us_encoder_forward_train", "us_encoder_backward", "us_encoder_dropout_mask",
              "us_encoder_tape_release", "us_prior_loss", "us_finetune_segment_backward"):
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.us_encoder_train_workspace_bytes(None, 1, 1) == 0
    assert lib.us_encoder_forward_train(None, None, None, None, None, None, 1, 1, 0.1, 0, None, 0, None) == -1
    assert lib.us_encoder_backward(None, None, None, 1, 1, None, None, 0, None, 0, None) == -1
    assert lib.us_encoder_dropout_mask(None, 0, 0, 1, 1, 0.1, None, None) == -1
    assert lib.us_encoder_tape_release(None, None) == -1
    assert lib.us_prior_loss(None, None, None, None, None, 1, 1, 1, None) == -1
    assert lib.us_finetune_segment_backward(None, None, None, None, None, 1, 1, 1, 1, 1, None) == -1
    h = C.c_void_p()
    c = _lib.us_encoder_config(TINY.n_vocab, TINY.n_feats, TINY.n_channels, TINY.filter_channels, TINY.n_heads, TINY.n_layers,
                               TINY.kernel_size, TINY.window_size)
    assert lib.us_encoder_create(C.byref(h), C.byref(c)) == 0
    try:
        small = lib.us_encoder_train_workspace_bytes(h, 1, 8)
        assert 0 < small < lib.us_encoder_train_workspace_bytes(h, 2, 8) < lib.us_encoder_train_workspace_bytes(h, 2, 16)
        assert lib.us_encoder_train_workspace_bytes(h, 0, 8) == 0
        # weights are not loaded: refused before anything is launched
        assert lib.us_encoder_forward_train(h, None, None, None, None, None, 1, 8, 0.1, 0, None, 0, None) == -4
        assert lib.us_encoder_dropout_mask(h, 0, 3 + 4 * TINY.n_layers, 1, 8, 0.1, None, None) == -1
        assert lib.us_encoder_tape_release(h, None) == 0
    finally:
        lib.us_frontend_destroy(h)


def test_train_mode_needs_trainable_and_says_so():
    enc = Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, window_size=4).train()
    assert enc.trainable is False
    with pytest.raises(RuntimeError, match="inference-only.*trainable=True"):
        enc._sync(torch.device("cuda"))
    with pytest.raises(TypeError):
        Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, None, 4, True)          # trainable is keyword-only
    assert Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, window_size=4, trainable=True).trainable
