"""The weight table the vocoder and speaker handles share with the front end (csrc/handle.h), through the raw C ABI: the same refusals
test_frontend.py checks on a front-end handle, on the smallest configuration each `create` accepts."""
import ctypes as C

import pytest
import torch

from unitspeech_amd import _lib

pytestmark = pytest.mark.gpu
B, T = 1, 4


def _vocoder(lib, h):
    c = _lib.us_vocoder_config()
    c.num_mels, c.upsample_initial_channel, c.resblock, c.n_up, c.n_kernels = 4, 4, 1, 1, 1
    c.upsample_rates[0], c.upsample_kernel_sizes[0], c.resblock_kernel_sizes[0] = 2, 4, 3
    for l, d in enumerate((1, 3, 5)):
        c.resblock_dilation_sizes[0][l] = d
    c.activation, c.snake_logscale = _lib.US_VOCODER_SNAKE, 0
    assert lib.us_vocoder_create(C.byref(h), C.byref(c)) == 0
    mel, wav = torch.zeros(B, 4, T, device="cuda"), torch.zeros(B, 1, 2 * T, device="cuda")
    return "conv_pre.weight", (4, 4, 7), lambda: lib.us_vocoder_forward(h, mel.data_ptr(), wav.data_ptr(), B, T, None, 0, None)


def _speaker(lib, h):
    c = _lib.us_speaker_config(feat_dim=8, channels=8, emb_dim=4, n_layers=0, global_context_att=0)
    assert lib.us_speaker_create(C.byref(h), C.byref(c)) == 0
    x, emb = torch.zeros(B, 8, T, device="cuda"), torch.zeros(B, 4, device="cuda")
    return "layer1.conv.weight", (8, 8, 5), lambda: lib.us_speaker_forward(h, x.data_ptr(), 0, B, T, emb.data_ptr(), 0, None, 0, None)


@pytest.mark.parametrize("name,make", [("vocoder", _vocoder), ("speaker", _speaker)])
def test_c_abi_reports_unknown_keys_wrong_shapes_and_missing_weights(name, make):
    lib = _lib.load()
    load, last_error, destroy = (getattr(lib, f"us_{name}_{f}") for f in ("load_weight", "last_error", "destroy"))
    h = C.c_void_p()
    key, shape, forward = make(lib, h)
    w = torch.zeros(*shape, device="cuda")
    shp = (C.c_int64 * 3)(*shape)
    assert load(h, b"conv_9.weight", w.data_ptr(), shp, 3, None) == -2                                           # ENOKEY
    assert b"unknown key" in last_error(h)
    bad = (C.c_int64 * 3)(shape[0], shape[1] - 1, shape[2])
    assert load(h, key.encode(), w.data_ptr(), bad, 3, None) == -3                                               # ESHAPE
    if name == "speaker":
        assert load(h, b"layer2.shortcut.weight", w.data_ptr(), shp, 3, None) == -2
        assert b"shortcuts" in last_error(h)
    assert load(h, key.encode(), w.data_ptr(), shp, 3, None) == 0
    assert forward() == -4                                                                                       # EWEIGHTS
    assert b"has not been loaded" in last_error(h)
    torch.cuda.synchronize()
    assert destroy(h) == 0
