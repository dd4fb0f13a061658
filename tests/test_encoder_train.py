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
        # the sentences themselves, whole
        err = lambda hh: lib.us_frontend_last_error(hh).decode()
        p = 4096                                   # a non-null address that must never be read
        fwd = lambda hh, B=1, L=8: lib.us_encoder_forward_train(hh, None, None, None, None, None, B, L, 0.1, 0, None, 0, None)
        bwd = lambda hh, B=1, L=8: lib.us_encoder_backward(hh, None, None, B, L, None, None, 0, None, 0, None)
        msk = lambda hh, site=0, pd=0.1, out=p: lib.us_encoder_dropout_mask(hh, 0, site, 1, 8, pd, out, None)
        assert fwd(h) == -4 and err(h) == "us_encoder_forward_train: weight 'emb.weight' has not been loaded"
        assert bwd(h) == -4 and err(h) == "us_encoder_backward: weight 'emb.weight' has not been loaded"
        assert fwd(h, L=9000) == -4 and err(h) == "us_encoder_forward_train: weight 'emb.weight' has not been loaded"   # before the LDS bound
        for B, L in ((0, 8), (1, 0), (65536, 8), (1, 65536)):
            assert fwd(h, B, L) == -1 and err(h) == "us_encoder_forward_train: bad B or L"
            assert bwd(h, B, L) == -1 and err(h) == "us_encoder_backward: bad B or L"
        assert msk(h, site=3 + 4 * TINY.n_layers) == -1 and err(h) == "us_encoder_dropout_mask: no such site"
        assert msk(h, site=-1) == -1 and err(h) == "us_encoder_dropout_mask: no such site"
        assert msk(h, pd=1.0) == -1 and err(h) == "us_encoder_dropout_mask: p_dropout must be below 1"
        assert msk(h, pd=float("nan")) == -1 and err(h) == "us_encoder_dropout_mask: p_dropout must be below 1"
        assert msk(h, out=None) == -1 and err(h) == "us_encoder_dropout_mask: bad argument"
        # a DurationPredictor handle, and none at all (the sentence is then the library's last error)
        d = C.c_void_p()
        dc = _lib.us_duration_config(16, 24, 3, 12)
        assert lib.us_duration_predictor_create(C.byref(d), C.byref(dc)) == 0
        try:
            for hh in (d, None):
                assert fwd(hh) == -1 and err(hh) == "us_encoder_forward_train: not an encoder handle"
                assert bwd(hh) == -1 and err(hh) == "us_encoder_backward: not an encoder handle"
                assert lib.us_encoder_tape_release(hh, None) == -1 and err(hh) == "us_encoder_tape_release: not an encoder handle"
                assert msk(hh) == -1 and err(hh) == "us_encoder_dropout_mask: bad argument"
                assert lib.us_encoder_forward(hh, None, None, None, None, None, 1, 8, None, 0, None) == -1
                assert err(hh) == "us_encoder_forward: not an encoder handle"
                assert lib.us_encoder_train_workspace_bytes(hh, 1, 8) == 0 and lib.us_encoder_debug_workspace_bytes(hh, 1, 8) == 0
        finally:
            lib.us_frontend_destroy(d)
        # workspace sizes in bytes, as the library gave them before the layouts took their offsets from handle.h's WsTake
        sizes = {(1, 8): (322304, 70144), (3, 19): (603648, 87552), (4, 60): (1848832, 136448)}
        for (B, L), want in sizes.items():
            assert (lib.us_encoder_train_workspace_bytes(h, B, L), lib.us_encoder_debug_workspace_bytes(h, B, L)) == want, (B, L)
    finally:
        lib.us_frontend_destroy(h)


ODD = EncoderConfig(n_vocab=30, n_feats=17, n_channels=40, filter_channels=72, n_heads=2, n_layers=2, kernel_size=5, window_size=4)


def test_c_abi_debug_entry_points_refuse_bad_arguments_without_device_work():
    """us_encoder_debug_*: a null handle or operand, an unknown mode / flag / dropout site, an operand the mode does not take
    (US_EINVAL) and an unknown key or layer (US_ENOKEY) are all refused before the weights are even looked at (US_EWEIGHTS: none
    is loaded here), so no launch can have happened."""
    lib = _lib.load()
    for s in ("us_encoder_debug_workspace_bytes", "us_encoder_debug_conv", "us_encoder_debug_ln_bwd", "us_encoder_debug_attention",
              "us_encoder_debug_embed_grad"):
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    conv, ln, att, emb = lib.us_encoder_debug_conv, lib.us_encoder_debug_ln_bwd, lib.us_encoder_debug_attention, lib.us_encoder_debug_embed_grad
    p = 4096                                   # a non-null address that must never be read
    assert lib.us_encoder_debug_workspace_bytes(None, 1, 1) == 0
    assert conv(None, b"proj_m", 0, p, None, None, None, None, 1.0, 0, -1, 0.0, 0, p, None, None, 1, 1, p, 1 << 30, None) == -1
    assert ln(None, b"prenet.norm_layers.0", p, p, None, 1.0, p, p, p, 1, 1, p, 1 << 30, None) == -1
    assert att(None, 0, p, p, p, p, 0.0, 0, p, p, None, None, None, None, None, None, None, 1, 1, p, 1 << 30, None) == -1
    assert emb(None, p, p, p, 1, 1, None) == -1
    h = C.c_void_p()
    c = _lib.us_encoder_config(ODD.n_vocab, ODD.n_feats, ODD.n_channels, ODD.filter_channels, ODD.n_heads, ODD.n_layers, ODD.kernel_size,
                               ODD.window_size)
    assert lib.us_encoder_create(C.byref(h), C.byref(c)) == 0
    d = lib.us_frontend_destroy
    try:
        small = lib.us_encoder_debug_workspace_bytes(h, 1, 8)
        assert 0 < small < lib.us_encoder_debug_workspace_bytes(h, 2, 8) < lib.us_encoder_debug_workspace_bytes(h, 64, 400)
        assert lib.us_encoder_debug_workspace_bytes(h, 0, 8) == 0
        fwd = lambda key, mode=0, x=p, dout=None, mask=None, add=None, gate=None, flags=0, site=-1, pd=0.0, out=p, dw=None, db=None, B=1, L=8: \
            conv(h, key, mode, x, dout, mask, add, gate, 1.0, flags, site, pd, 0, out, dw, db, B, L, p, 1 << 30, None)
        assert fwd(None) == -1 and fwd(b"proj_m", mode=3) == -1 and fwd(b"proj_m", flags=8) == -1
        assert fwd(b"proj_m", x=None) == -1 and fwd(b"proj_m", out=None) == -1 and fwd(b"proj_m", dout=p) == -1
        assert fwd(b"proj_m", flags=1) == -1                                   # a mask flag without a mask
        assert fwd(b"proj_m", site=3 + 4 * ODD.n_layers, pd=0.1) == -1 and fwd(b"proj_m", site=0, pd=1.0) == -1
        assert fwd(b"proj_m", mode=1, dout=p, out=None, dw=p) == -1            # wgrad without db
        assert fwd(b"proj_m", mode=1, dout=p, out=None, dw=p, db=p, add=p) == -1
        assert fwd(b"proj_m", mode=2, x=None, dout=p, site=0, pd=0.1) == -1     # only the forward drops
        assert fwd(b"proj_m", mode=2, x=p, dout=p) == -1
        assert fwd(b"proj_m", B=0) == -1 and fwd(b"proj_m", L=70000) == -1
        assert fwd(b"proj_n") == -2 and fwd(b"emb") == -2 and fwd(b"prenet.norm_layers.0") == -2
        assert fwd(b"proj_m") == -4 and fwd(b"proj_m", mode=1, dout=p, out=None, dw=p, db=p) == -4          # only the weights are missing
        assert fwd(b"encoder.ffn_layers.1.conv_2", mode=2, x=None, dout=p, gate=p, add=p, mask=p, flags=4) == -4
        lnc = lambda key, x=p, dy=p, dx=p, dg=p, db=p: ln(h, key, x, dy, None, 1.0, dx, dg, db, 1, 8, p, 1 << 30, None)
        assert lnc(None) == -1 and lnc(b"prenet.norm_layers.0", x=None) == -1 and lnc(b"prenet.norm_layers.0", db=None) == -1
        assert lnc(b"prenet.norm_layers.3") == -2 and lnc(b"proj_m") == -2
        assert lnc(b"encoder.norm_layers_2.1") == -4
        ac = lambda layer=0, q=p, P=p, pd=0.0, dO=None, DS=None, rest=None, gk=None: \
            att(h, layer, q, p, p, p, pd, 0, p, P, dO, DS, rest, rest, rest, gk, gk, 1, 8, p, 1 << 30, None)
        assert ac(q=None) == -1 and ac(P=None) == -1 and ac(pd=1.0) == -1 and ac(pd=-0.5) == -1
        assert ac(DS=p) == -1 and ac(dO=p) == -1 and ac(dO=p, DS=p, rest=p) == -1       # a half-given backward
        assert ac(layer=ODD.n_layers) == -2 and ac(layer=-1) == -2
        assert ac() == -4 and ac(dO=p, DS=p, rest=p, gk=p) == -4
        assert emb(h, None, p, p, 1, 8, None) == -1 and emb(h, p, p, None, 1, 8, None) == -1 and emb(h, p, p, p, 1, 0, None) == -1
        assert emb(h, p, p, p, 1, 8, None) == -4
        # the sentences themselves, whole
        err = lambda hh: lib.us_frontend_last_error(hh).decode()
        lnb = lambda B=1, L=8: ln(h, b"prenet.norm_layers.0", p, p, None, 1.0, p, p, p, B, L, p, 1 << 30, None)
        acb = lambda B=1, L=8: att(h, 0, p, p, p, p, 0.0, 0, p, p, None, None, None, None, None, None, None, B, L, p, 1 << 30, None)
        calls = {"us_encoder_debug_conv": lambda B=1, L=8: fwd(b"proj_m", B=B, L=L), "us_encoder_debug_ln_bwd": lnb,
                 "us_encoder_debug_attention": acb, "us_encoder_debug_embed_grad": lambda B=1, L=8: emb(h, p, p, p, B, L, None)}
        for name, call in calls.items():
            for B, L in ((0, 8), (1, 0), (65536, 8), (1, 65536), (65535, 33)):          # the last: B * L * 1024 passes 2^31
                assert call(B, L) == -1 and err(h) == name + ": bad B or L", (name, B, L)
            assert call(1, 9000) == -1 and err(h) == name + ": more than ~8000 symbols per utterance"     # before the weights
            assert call() == -4 and err(h) == name + ": weight 'emb.weight' has not been loaded"
        assert fwd(b"proj_m", mode=1, dout=p, out=None, dw=p, db=p) == -4
        small_ws = conv(h, b"proj_m", 0, p, None, None, None, None, 1.0, 0, -1, 0.0, 0, p, None, None, 1, 8, p, 16, None)
        assert small_ws == -4                      # the workspace is looked at after the weights
        dp = C.c_void_p()
        dc = _lib.us_duration_config(16, 24, 3, 12)
        assert lib.us_duration_predictor_create(C.byref(dp), C.byref(dc)) == 0
        try:
            for hh in (dp, None):
                wrong = {"us_encoder_debug_conv": lambda: conv(hh, b"proj_m", 0, p, None, None, None, None, 1.0, 0, -1, 0.0, 0, p, None, None, 1, 8, p, 1 << 30, None),
                         "us_encoder_debug_ln_bwd": lambda: ln(hh, b"prenet.norm_layers.0", p, p, None, 1.0, p, p, p, 1, 8, p, 1 << 30, None),
                         "us_encoder_debug_attention": lambda: att(hh, 0, p, p, p, p, 0.0, 0, p, p, None, None, None, None, None, None, None, 1, 8, p, 1 << 30, None),
                         "us_encoder_debug_embed_grad": lambda: emb(hh, p, p, p, 1, 8, None)}
                for name, call in wrong.items():
                    assert call() == -1 and err(hh) == name + ": not an encoder handle", name
        finally:
            d(dp)
    finally:
        d(h)


def test_the_odd_configuration_constructs_and_ends_reductions_inside_a_slice():
    """The configuration tests/test_encoder_train_kernels_gpu.py adds to TINY and FULL: K * Cin is no multiple of the GEMM's
    16-wide reduction slice for the prenet and the FFN convolutions, N and Cin are no multiples of the 64-wide tile, D = 20."""
    sd = synthetic_encoder_state_dict(ODD, 0)
    assert list(sd) == list(encoder_state_shapes(ODD))
    Encoder(ODD.n_vocab, ODD.n_feats, ODD.n_channels, ODD.filter_channels, ODD.n_heads, ODD.n_layers, ODD.kernel_size, 0.1,
            window_size=ODD.window_size, trainable=True).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    for key in ("prenet.conv_layers.0", "encoder.ffn_layers.0.conv_1", "encoder.ffn_layers.0.conv_2", "proj_m"):
        cout, cin, k = sd[key + ".weight"].shape
        assert (k * cin) % 16 != 0 and cin % 64 != 0 and cout % 64 != 0, key
    assert ODD.n_channels // ODD.n_heads == 20
    ids, lens = torch.randint(0, ODD.n_vocab, (2, 7)), torch.LongTensor([7, 3])
    mu_x, _, _ = ET.encoder_forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, ODD.n_heads, ids, lens)
    assert mu_x.shape == (2, 17, 7) and bool(torch.isfinite(mu_x).all())


def wgrad_split_geometry(rows):
    """(splits, rows_per_split) of gemm_conv_wgrad (csrc/encoder_train.hip: wgrad_splits, and the round-up to the 16-row slice)."""
    s = min(max(rows // 512, 1), 32)
    return s, (-(-rows // s) + 15) // 16 * 16


def test_no_row_count_leaves_the_weight_gradient_an_empty_last_split():
    """splits * rows_per_split never passes rows by a whole split for rows <= 20,000 (below the cap of 32 it would take
    512 < 16 (splits - 1), above it rows <= 15,872 < 32 * 512), so an EMPTY last split does not occur and the GPU tests cannot
    run one; the shapes they do run (a short last split at 1030 rows, the cap at 16,500) are checked here too."""
    for rows in range(1, 20001):
        s, per = wgrad_split_geometry(rows)
        assert (s - 1) * per < rows, rows
    assert wgrad_split_geometry(1030) == (2, 528) and wgrad_split_geometry(12800) == (25, 512) and wgrad_split_geometry(16500) == (32, 528)
    assert wgrad_split_geometry(1024) == (2, 512) and wgrad_split_geometry(65) == (1, 80)


def test_train_mode_needs_trainable_and_says_so():
    enc = Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, window_size=4).train()
    assert enc.trainable is False
    with pytest.raises(RuntimeError, match="inference-only.*trainable=True"):
        enc._sync(torch.device("cuda"))
    with pytest.raises(TypeError):
        Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, None, 4, True)          # trainable is keyword-only
    assert Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, window_size=4, trainable=True).trainable
