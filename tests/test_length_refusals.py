"""The refusal of an out-of-range item length and the workspace sizes of the modules that take per-item lengths (no GPU): every entry point
is called with pointers that are never dereferenced, one length too short and one too long, and the whole last-error string is compared with
the wording the library had before the refusals were folded into one helper.  The workspace sizes are pinned the same way, at one and at 33
items (a second group of 32)."""
import ctypes as C

import pytest

from unitspeech_amd import _lib
from unitspeech_amd.hubert import HubertModel
from unitspeech_amd.speaker_encoder import ECAPA_TDNN
from unitspeech_amd.vocoder import BigVGAN
from unitspeech_amd.wavlm import WavLMModel

EINVAL = -1
P = 4096                              # stands for every device pointer: never dereferenced
VOCODER = {"resblock": "1", "upsample_rates": [4, 2, 2], "upsample_kernel_sizes": [8, 4, 4], "upsample_initial_channel": 32,
           "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]], "activation": "snake", "snake_logscale": False,
           "num_mels": 8}
HUBERT = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
              intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)
WAVLM = dict(HUBERT, num_buckets=32, max_bucket_distance=40, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)


def _configs():
    return {
        "vocoder": BigVGAN(VOCODER)._config_struct(),
        "speaker": ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)._config_struct(),
        "mel": _lib.us_mel_config(n_fft=1024, hop=256, win=1024, num_mels=80),
        "resample": _lib.us_resample_config(orig_freq=441, new_freq=320, width=6),
        "hubert": HubertModel(**HUBERT)._config_struct(),
        "wavlm": WavLMModel(**WAVLM)._config_struct(),
    }


@pytest.fixture(scope="module")
def handles():
    lib = _lib.load()
    hs = {}
    for name, cfg in _configs().items():
        hs[name] = C.c_void_p()
        assert getattr(lib, f"us_{name}_create")(C.byref(hs[name]), C.byref(cfg)) == _lib.US_OK, name
    yield lib, hs
    for name, h in hs.items():
        getattr(lib, f"us_{name}_destroy")(h)


def _call(lib, hs, entry, lengths):
    """rc and the module's last error of `entry` on a batch of three items with these lengths"""
    arr = (C.c_int64 * 3)(*lengths)
    h = hs[entry.split("_")[1]]
    rc = {
        "us_vocoder_forward_lengths": lambda: lib.us_vocoder_forward_lengths(h, P, arr, P, 3, 9, P, 1 << 30, None),
        "us_vocoder_debug_layer_lengths": lambda: lib.us_vocoder_debug_layer_lengths(h, b"conv_pre", P, None, None, 0.0, P, 3, 9, arr, None),
        "us_speaker_forward_lengths": lambda: lib.us_speaker_forward_lengths(h, P, 3, 3, 9, arr, P, 0, P, 1 << 30, None),
        "us_mel_forward": lambda: lib.us_mel_forward(h, P, arr, 3, 4000, None, None, 0, 0.0, P, P, 1 << 30, None),
        "us_mel_minmax": lambda: lib.us_mel_minmax(h, P, arr, 3, 20, P, None),
        "us_resample_forward": lambda: lib.us_resample_forward(h, P, arr, 3, 4000, P, P, 1 << 30, None),
        "us_hubert_forward": lambda: lib.us_hubert_forward(h, P, arr, 3, 4000, 0, 2, P, None, P, 1 << 40, None),
        "us_wavlm_forward": lambda: lib.us_wavlm_forward(h, P, arr, 3, 4000, 0, 2, P, None, 0, 0, P, 1 << 40, None),
    }[entry]()
    return rc, getattr(lib, f"us_{entry.split('_')[1]}_last_error")(h).decode()


# entry point -> (lengths with item 1 too short, the refusal, lengths with item 2 too long, the refusal)
REFUSALS = {
    "us_vocoder_forward_lengths": (
        [9, 0, 4], "us_vocoder_forward_lengths: lengths[1] = 0 must be at least 1 and at most Tmax = 9",
        [9, 4, 10], "us_vocoder_forward_lengths: lengths[2] = 10 must be at least 1 and at most Tmax = 9"),
    "us_vocoder_debug_layer_lengths": (
        [9, 0, 4], "us_vocoder_debug_layer_lengths: lengths[1] = 0 must be at least 1 and at most Tin_max = 9",
        [9, 4, 10], "us_vocoder_debug_layer_lengths: lengths[2] = 10 must be at least 1 and at most Tin_max = 9"),
    "us_speaker_forward_lengths": (
        [9, 0, 4], "us_speaker_forward_lengths: lengths[1] = 0 must be at least 1 and at most Tmax = 9",
        [9, 4, 10], "us_speaker_forward_lengths: lengths[2] = 10 must be at least 1 and at most Tmax = 9"),
    "us_mel_forward": (
        [4000, 384, 4000], "us_mel_forward: lengths[1] = 384 is outside (384, 4000]",
        [4000, 385, 4001], "us_mel_forward: lengths[2] = 4001 is outside (384, 4000]"),
    "us_mel_minmax": (
        [20, -1, 0], "us_mel_minmax: lengths[1] = -1 is outside (-1, 20]",
        [20, 0, 21], "us_mel_minmax: lengths[2] = 21 is outside (-1, 20]"),
    "us_resample_forward": (
        [4000, 0, 1], "us_resample_forward: lengths[1] = 0 is outside [1, 4000]",
        [4000, 1, 4001], "us_resample_forward: lengths[2] = 4001 is outside [1, 4000]"),
    "us_hubert_forward": (
        [4000, 399, 400], "us_hubert_forward: lengths[1] = 399 must be at least the receptive field (400 samples) and at most Tmax",
        [4000, 400, 4001], "us_hubert_forward: lengths[2] = 4001 must be at least the receptive field (400 samples) and at most Tmax"),
    "us_wavlm_forward": (
        [4000, 399, 400], "us_wavlm_forward: lengths[1] = 399 must be at least the receptive field (400 samples) and at most Tmax",
        [4000, 400, 4001], "us_wavlm_forward: lengths[2] = 4001 must be at least the receptive field (400 samples) and at most Tmax"),
}


@pytest.mark.parametrize("entry", list(REFUSALS))
def test_a_length_out_of_range_is_refused_in_the_same_words(handles, entry):
    lib, hs = handles
    short, short_msg, long_, long_msg = REFUSALS[entry]
    assert _call(lib, hs, entry, short) == (EINVAL, short_msg)
    assert _call(lib, hs, entry, long_) == (EINVAL, long_msg)
    # both at once: the first item out of range is the one named
    both = [short[0], short[1], long_[2]]
    assert _call(lib, hs, entry, both) == (EINVAL, short_msg)


# module -> (T or Tmax, bytes at B = 1, bytes at B = 33)
WORKSPACES = {
    "vocoder": (9, 11776, 380416),
    "speaker": (9, 158976, 5192960),
    "mel": (4000, 49664, 1624320),
    "resample": (4000, 19712, 640768),
    "hubert": (4000, 137472, 4481536),
    "wavlm": (4000, 176128, 5752064),
}


@pytest.mark.parametrize("module", list(WORKSPACES))
def test_workspace_sizes_are_what_they_were(handles, module):
    lib, hs = handles
    T, one, many = WORKSPACES[module]
    fn = getattr(lib, f"us_{module}_workspace_bytes")
    assert (fn(hs[module], 1, T), fn(hs[module], 33, T)) == (one, many)
