"""BigVGAN vocoder, CPU side: the torch restatement (tools/vocoder_torch.py) against the reference goldens, the module's state_dict
against the reference's key lists in both weight-norm forms, the weight-norm fold, and the configurations that must be refused."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vocoder_torch import bigvgan_forward, fold_weight_norm  # noqa: E402

from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BigVGAN, bigvgan_flops, synthetic_bigvgan_state_dict  # noqa: E402

CASES = ["vocoder_tiny", "vocoder_base", "vocoder_large"]


def _sd(g):
    return {k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(json.loads(str(g["config"])), int(g["seed"])).items()}


@pytest.mark.parametrize("name", CASES)
def test_torch_restatement_matches_the_reference_golden(golden, name):
    g = golden(name)
    cfg, sd = json.loads(str(g["config"])), _sd(g)
    mel = torch.from_numpy(g["mel"])
    with torch.no_grad():
        y32 = bigvgan_forward(cfg, sd, mel).numpy()
        y64 = bigvgan_forward(cfg, sd, mel.double()).numpy()
    assert y32.shape == g["wav32"].shape == g["wav64"].shape
    assert np.abs(y64 - g["wav64"]).max() <= 1e-6
    assert np.abs(y32 - g["wav32"]).max() <= 1e-6
    assert 0.05 < g["wav64"].std() and np.abs(g["wav64"]).max() < 0.95        # neither silent nor saturated


def _keys(sd):
    return [str(k) for k in sd], [",".join(str(s) for s in t.shape) for t in sd.values()]


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_shapes_match_the_reference_in_both_forms(golden, name, capsys):
    g = golden(name)
    m = BigVGAN(json.loads(str(g["config"])))
    keys, shapes = _keys(m.state_dict())
    assert keys == list(g["keys_wn"]) and shapes == list(g["shapes_wn"])
    assert list(_sd(g)) == keys
    m.remove_weight_norm()
    keys, shapes = _keys(m.state_dict())
    assert keys == list(g["keys_removed"]) and shapes == list(g["shapes_removed"])
    assert not any(k.endswith(("weight_g", "weight_v")) for k in keys)


def test_weight_norm_fold_matches_g_v_over_norm_on_both_conv_types():
    torch.manual_seed(0)
    m = BigVGAN(dict(BIGVGAN_22KHZ_80BAND, upsample_initial_channel=16, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4],
                     resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]]))
    for prefix, mod in (("conv_pre", m.conv_pre), ("ups.0.0", m.ups[0][0]), ("resblocks.1.convs1.2", m.resblocks[1].convs1[2])):
        with torch.no_grad():
            mod.weight_g.mul_(torch.rand_like(mod.weight_g) + 0.5)
        g, v = mod.weight_g.detach().double().numpy(), mod.weight_v.detach().double().numpy()
        # Conv1d [out, in, k]: one norm per output channel; ConvTranspose1d [in, out, k] (weight_norm dim=0): one per INPUT channel
        want = np.stack([g[i].reshape(()) * v[i] / np.sqrt((v[i] ** 2).sum()) for i in range(v.shape[0])])
        got = fold_weight_norm(mod.weight_g.detach().double(), mod.weight_v.detach().double()).numpy()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        src = dict(m._sources())[prefix + ".weight"]
        np.testing.assert_allclose(src[1]().detach().double().numpy(), want, rtol=1e-6, atol=1e-9)
    assert m.ups[0][0].weight_g.shape == (16, 1, 1) and m.ups[0][0].weight_v.shape == (16, 8, 4)


def test_unsupported_configurations_raise():
    with pytest.raises(NotImplementedError, match="AMPBlock2"):
        BigVGAN(dict(BIGVGAN_22KHZ_80BAND, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]]))
    with pytest.raises(NotImplementedError):
        BigVGAN(dict(BIGVGAN_22KHZ_80BAND, activation="relu"))
    with pytest.raises(ValueError):
        BigVGAN(dict(BIGVGAN_22KHZ_80BAND, upsample_kernel_sizes=[8, 8]))
    m = BigVGAN(dict(BIGVGAN_22KHZ_80BAND, upsample_initial_channel=16, upsample_rates=[2], upsample_kernel_sizes=[4],
                     resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]]))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(torch.zeros(1, 80, 4))


def test_library_refuses_shapes_it_does_not_implement():
    """The C ABI's own checks (no device work): AMPBlock2, kernels that are not a multiple of the rate, even resblock kernels."""
    import ctypes as C

    from unitspeech_amd import _lib
    lib = _lib.load()
    m = BigVGAN(BIGVGAN_22KHZ_80BAND)
    good = m._config_struct()
    h = C.c_void_p()
    assert lib.us_vocoder_create(C.byref(h), C.byref(good)) == 0
    assert lib.us_vocoder_num_weights(h) == len([k for k in m._sources()])
    assert {lib.us_vocoder_weight_key(h, i).decode() for i in range(lib.us_vocoder_num_weights(h))} == set(m._sources())
    lib.us_vocoder_destroy(h)
    for field, value in (("resblock", 2), ("activation", 7)):
        bad = m._config_struct()
        setattr(bad, field, value)
        assert lib.us_vocoder_create(C.byref(h), C.byref(bad)) == -1
    bad = m._config_struct()
    bad.upsample_kernel_sizes[0] = 6                 # rate 4: not a multiple
    assert lib.us_vocoder_create(C.byref(h), C.byref(bad)) == -1
    assert b"multiple" in lib.us_vocoder_last_error(None)
    bad = m._config_struct()
    bad.resblock_kernel_sizes[1] = 4
    assert lib.us_vocoder_create(C.byref(h), C.byref(bad)) == -1


def test_debug_layer_refuses_bad_arguments_before_any_device_work():
    """us_vocoder_debug_layer: null and non-positive arguments, an unknown prefix, an epilogue operand on a layer that has no epilogue,
    sizes past the forward's limits, and (last, so everything above is checked first) weights that were never loaded."""
    import ctypes as C

    from unitspeech_amd import _lib
    lib = _lib.load()
    m = BigVGAN(dict(BIGVGAN_22KHZ_80BAND, upsample_initial_channel=16, upsample_rates=[3, 2], upsample_kernel_sizes=[9, 4],
                     resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]]))
    h = C.c_void_p()
    c = m._config_struct()
    assert lib.us_vocoder_create(C.byref(h), C.byref(c)) == 0
    p = 4096                     # never dereferenced: every call below is refused on the host
    EINVAL, ENOKEY, EWEIGHTS = -1, -2, -4
    call = lib.us_vocoder_debug_layer
    assert call(None, b"conv_pre", p, None, None, 0.0, p, 1, 4, None) == EINVAL
    assert call(h, None, p, None, None, 0.0, p, 1, 4, None) == EINVAL
    assert call(h, b"conv_pre", None, None, None, 0.0, p, 1, 4, None) == EINVAL
    assert call(h, b"conv_pre", p, None, None, 0.0, None, 1, 4, None) == EINVAL
    assert call(h, b"conv_pre", p, None, None, 0.0, p, 0, 4, None) == EINVAL
    assert call(h, b"conv_pre", p, None, None, 0.0, p, 1, 0, None) == EINVAL
    assert call(h, b"conv_pre", p, None, None, -1.0, p, 1, 4, None) == EINVAL
    assert call(h, b"conv_pre", p, None, None, float("nan"), p, 1, 4, None) == EINVAL
    for bad in (b"", b"conv_pre.weight", b"ups.2.0", b"ups.0", b"resblocks.2.convs1.0", b"resblocks.0.convs1.3", b"resblocks.0.activations.6"):
        assert call(h, bad, p, None, None, 0.0, p, 1, 4, None) == ENOKEY, bad
        assert bad in lib.us_vocoder_last_error(h)
    for layer in (b"resblocks.1.activations.5", b"activation_post", b"conv_post"):
        assert call(h, layer, p, p, None, 0.0, p, 1, 4, None) == EINVAL, layer
        assert call(h, layer, p, None, p, 0.0, p, 1, 4, None) == EINVAL, layer
        assert call(h, layer, p, None, None, 2.0, p, 1, 4, None) == EINVAL, layer
        assert b"epilogue" in lib.us_vocoder_last_error(h)
    assert call(h, b"conv_pre", p, None, None, 0.0, p, 4096, 4, None) == EINVAL           # B * channels past a grid dimension
    assert call(h, b"ups.0.0", p, None, None, 0.0, p, 1, 1 << 27, None) == EINVAL         # Cout * Tin * rate = 8 * 3 * 2^27 >= 2^31
    assert call(h, b"ups.0.0", p, None, None, 0.0, p, 1, 1 << 26, None) == EWEIGHTS       # within the limits: next check
    for layer in (b"conv_pre", b"ups.1.0", b"resblocks.1.convs2.2", b"resblocks.0.activations.0", b"activation_post", b"conv_post"):
        assert call(h, layer, p, None, None, 0.0, p, 1, 4, None) == EWEIGHTS, layer
    assert call(h, b"resblocks.0.convs2.2", p, p, p, 1.0, p, 1, 4, None) == EWEIGHTS      # a convolution takes the epilogue operands
    lib.us_vocoder_destroy(h)


def test_flops_per_frame_of_the_two_22khz_generators():
    from unitspeech_amd.vocoder import BIGVGAN_BASE_22KHZ_80BAND
    assert 1.80e9 < bigvgan_flops(BIGVGAN_22KHZ_80BAND, 1024) / 1024 < 1.86e9           # torch.utils.flop_counter: 1.83 G
    assert 0.62e9 < bigvgan_flops(BIGVGAN_BASE_22KHZ_80BAND, 1024) / 1024 < 0.66e9      # 0.64 G
