"""Voice conversion, host side (no device work): the ContentVec encoder's state_dict layout and C-ABI key table, the fp64 NumPy
statement of the mel-rate alignment (tools/vc_numpy.py) against exact rational arithmetic and against the reference's own
`voice_conversion()` output (tests/golden/vc_tiny.npz), and the torch restatement's Linear front (tools/encoder_torch.py) against
the reference class in fp64 (tests/golden/vc_encoder_tiny.npz).  Goldens: tools/make_goldens_vc.py.
"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import encoder_torch as ET  # noqa: E402
import vc_numpy as VN  # noqa: E402
from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.encoder import ContentVecEncoder, Encoder, EncoderConfig, encoder_state_shapes, synthetic_encoder_state_dict  # noqa: E402

TINY_E = EncoderConfig(n_vocab=20, n_feats=8, n_channels=16, filter_channels=32, n_heads=2, n_layers=2, kernel_size=3, window_size=4,
                       n_contentvec=12)
FULL_E = EncoderConfig(n_vocab=150, n_feats=80, n_channels=192, filter_channels=768, n_heads=2, n_layers=6, kernel_size=3, window_size=4,
                       n_contentvec=768)


def make(cfg, **kw):
    return ContentVecEncoder(cfg.n_vocab, cfg.n_feats, cfg.n_channels, cfg.filter_channels, cfg.n_heads, cfg.n_layers, cfg.kernel_size, 0.1,
                             n_contentvec=cfg.n_contentvec, window_size=cfg.window_size, **kw)


def test_state_dict_is_the_reference_modules(golden):
    """Keys and shapes in order as the reference's Encoder(n_contentvec=768) registered them (stored by the goldens' generator), so the
    reference's contentvec_encoder.pt loads strictly; the synthetic dict does."""
    g = golden("vc_encoder_full")
    want = [(str(k), tuple(int(n) for n in str(s).split(","))) for k, s in zip(g["keys"], g["shapes"])]
    enc = make(FULL_E)
    assert [(k, tuple(v.shape)) for k, v in enc.state_dict().items()] == want
    assert want[0] == ("emb.weight", (192, 768))
    assert list(encoder_state_shapes(FULL_E).items()) == want
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(FULL_E, 0).items()}, strict=True)
    # the default argument list is the reference's with n_contentvec = 768
    assert ContentVecEncoder(150, 80, 192, 768, 2, 6, 3, 0.1, window_size=4).cfg == FULL_E


def test_synthetic_draws_of_the_id_encoder_are_unchanged():
    """`emb.weight` of the id encoder keeps its draw (scaled by n_channels ** -0.5 from its second axis); the Linear front scales by
    n_channels ** -0.5 too, from its first."""
    cfg = EncoderConfig(n_vocab=20, n_feats=8, n_channels=16, filter_channels=32, n_heads=2, n_layers=2)
    sd = synthetic_encoder_state_dict(cfg, 0)
    assert sd["emb.weight"].shape == (20, 16)
    lin = synthetic_encoder_state_dict(TINY_E, 0)
    assert lin["emb.weight"].shape == (16, 12)
    assert abs(float(lin["emb.weight"].std()) - 16 ** -0.5) < 0.05
    for k in sd:
        if k != "emb.weight":
            assert np.array_equal(sd[k], lin[k]), k


def test_encoder_with_n_contentvec_still_refuses_and_names_the_class():
    with pytest.raises(NotImplementedError, match="ContentVecEncoder"):
        Encoder(20, 8, 16, 32, 2, 2, 3, 0.1, n_contentvec=4)
    with pytest.raises(ValueError):
        ContentVecEncoder(20, 8, 16, 32, 2, 2, 3, 0.1, n_contentvec=1025)
    enc = make(TINY_E).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 4, 12), torch.LongTensor([4]))
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 4, 11), torch.LongTensor([4]))


def test_c_abi_contentvec_handle_key_table_and_refusals():
    """Handle creation does no GPU work.  The key table is the reference's with the Linear-layout emb.weight; n_contentvec outside
    1..1024 is refused; each kind of handle refuses the other kind's entry points before anything is read."""
    lib = _lib.load()
    c = _lib.us_encoder_config(-7, 8, 16, 32, 2, 2, 3, 4)                # n_vocab is ignored
    h = C.c_void_p()
    for bad in (0, -1, 1025):
        assert lib.us_encoder_create_contentvec(C.byref(h), C.byref(c), bad) == -1
    assert lib.us_encoder_create_contentvec(C.byref(h), C.byref(c), 12) == 0
    keys = [lib.us_frontend_weight_key(h, i).decode() for i in range(lib.us_frontend_num_weights(h))]
    assert keys == list(encoder_state_shapes(TINY_E))
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.us_encoder_forward(h, p, p, p, p, p, 1, 1, None, 0, None) == -1
    assert b"ContentVec handle" in lib.us_frontend_last_error(h)
    assert lib.us_encoder_forward_train(h, p, p, p, p, p, 1, 1, 0.0, 0, None, 0, None) == -1
    assert lib.us_encoder_backward(h, p, p, 1, 1, None, None, 0, None, 0, None) == -1
    assert lib.us_frontend_destroy(h) == 0
    ids = C.c_void_p()
    c = _lib.us_encoder_config(20, 8, 16, 32, 2, 2, 3, 4)
    assert lib.us_encoder_create(C.byref(ids), C.byref(c)) == 0
    assert lib.us_encoder_forward_features(ids, p, p, p, p, p, 1, 1, None, 0, None) == -1
    assert b"not a ContentVec handle" in lib.us_frontend_last_error(ids)
    assert lib.us_encoder_forward_features_train(ids, p, p, p, p, p, 1, 1, 0.0, 0, None, 0, None) == -1
    assert lib.us_encoder_backward_features(ids, p, p, p, 1, 1, None, None, 0, None, 0, None) == -1
    assert lib.us_frontend_destroy(ids) == 0


# ---- the alignment's yardstick --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lx,ly", [(1, 5), (9, 15), (12, 7), (13, 13), (37, 64), (499, 860)])
def test_vc_numpy_equals_the_exact_rational_result(lx, ly):
    x = np.random.Generator(np.random.Philox(key=lx * 10007 + ly)).standard_normal(lx).astype(np.float32)
    got = VN.interpolate(x, ly)
    xf = [Fraction(float(v)) for v in x]
    for t in range(ly):
        num, den = max((2 * t + 1) * lx - ly, 0), 2 * ly
        i0 = min(num // den, lx - 1)
        i1 = i0 + (1 if i0 < lx - 1 else 0)
        lam = Fraction(num - i0 * den, den)
        assert lam == max(Fraction(2 * t + 1, 2) * Fraction(lx, ly) - Fraction(1, 2), 0) - i0      # the coordinate, exactly
        want = (1 - lam) * xf[i0] + lam * xf[i1]
        # fp64 rounds lam, 1 - lam, two products and a sum
        assert abs(Fraction(float(got[t])) - want) <= 4 * 2.0 ** -53 * float(np.abs(x).max()), (t, float(got[t]), float(want))
    if lx == ly:
        assert np.array_equal(got, x.astype(np.float64))


def test_vc_numpy_reproduces_the_reference_function(golden):
    """cond_y and y_mask of the reference's voice_conversion() at 9 -> 15 (padded to 16) from its own fp32 encoder output.

    Bound: torch evaluates the coordinate in fp32 as scale * (t + 0.5) - 0.5 with scale = fl(Lx / Ly): the rounding of scale, of the
    product and of the difference are each at most 2^-24 Lx, so lambda is off by at most 3 Lx 2^-24 (+ 2^-24 for 1 - lambda), which
    moves the blend by at most twice that times max|x|; the fp32 blend itself (two products and a sum) adds 3 2^-24 max|x|.  With
    Lx = 9: (2 (3 * 9 + 1) + 3) 2^-24 = 59 * 2^-24 = 3.5e-6 of max|x|."""
    g = golden("vc_tiny")
    lx, ly, tp = int(g["lengths"][0]), int(g["mel_length"]), int(g["tp"])
    cond_y, y_mask = VN.vc_align(g["cond_x"], [lx], [ly], tp)
    assert cond_y.shape == g["cond_y"].shape and np.array_equal(y_mask, g["y_mask"].astype(np.float64))
    bound = (2 * (3 * lx + 1) + 3) * 2.0 ** -24 * float(np.abs(g["cond_x"]).max())
    err = float(np.abs(cond_y - g["cond_y"]).max())
    print(f"vc_numpy vs reference at {lx} -> {ly}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.all(cond_y[:, :, ly:] == 0) and np.all(g["cond_y"][:, :, ly:] == 0)


def test_vc_numpy_is_per_item_and_validates_lengths():
    x = np.random.Generator(np.random.Philox(key=5)).standard_normal((3, 4, 12))
    cond_y, y_mask = VN.vc_align(x, [12, 7, 3], [21, 12, 5], 24)
    for b, (lx, ly) in enumerate(((12, 21), (7, 12), (3, 5))):
        one, m = VN.vc_align(x[b:b + 1, :, :lx], [lx], [ly], 24)
        assert np.array_equal(cond_y[b], one[0]) and np.array_equal(y_mask[b], m[0])
        assert np.all(cond_y[b, :, ly:] == 0) and y_mask[b, 0].sum() == ly
    for xl, yl in (([0, 7, 3], [21, 12, 5]), ([13, 7, 3], [21, 12, 5]), ([12, 7, 3], [25, 12, 5]), ([12, 7, 3], [21, 0, 5])):
        with pytest.raises(ValueError):
            VN.vc_align(x, xl, yl, 24)


# ---- the torch restatement's Linear front -----------------------------------------------------------------------------------

def test_restatement_with_the_linear_front_matches_the_reference_in_fp64(golden):
    g = golden("vc_encoder_tiny")
    sd = {k: torch.from_numpy(v).double() for k, v in synthetic_encoder_state_dict(TINY_E, 0).items()}
    feats, lens = torch.from_numpy(g["feats"]).double(), torch.from_numpy(g["lengths"])
    mu_x, x, x_mask = ET.encoder_forward(sd, TINY_E.n_heads, feats, lens)
    assert torch.equal(x_mask.float(), torch.from_numpy(g["x_mask"]).float())
    assert float((mu_x - torch.from_numpy(g["mu_x"])).abs().max()) <= 1e-12
    assert float((x - torch.from_numpy(g["x"])).abs().max()) <= 1e-12
    # rows past an item's length do not count, whatever they hold
    dirty = feats.clone()
    for b, n in enumerate(lens.tolist()):
        dirty[b, n:] = float("nan")
    mu2, x2, _ = ET.encoder_forward(sd, TINY_E.n_heads, dirty, lens)
    assert torch.equal(mu2, mu_x) and torch.equal(x2, x)


def test_restatement_gradients_match_the_reference_in_fp64(golden):
    g = golden("vc_encoder_train_tiny")
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in synthetic_encoder_state_dict(TINY_E, 0).items()}
    mu_x, x, _ = ET.encoder_forward(sd, TINY_E.n_heads, torch.from_numpy(g["feats"]).double(), torch.from_numpy(g["lengths"]))
    ((mu_x * torch.from_numpy(g["g_mu"]).double()).sum() + (x * torch.from_numpy(g["g_x"]).double()).sum()).backward()
    scale = max(float(np.linalg.norm(g["g64/" + k])) for k in sd)
    for k, v in sd.items():
        ref = torch.from_numpy(g["g64/" + k])
        assert float((v.grad - ref).norm()) <= 1e-10 * scale, k
