"""Ragged vocoder batches, the parts that need no GPU: the two new entry points' declarations, exports, prototypes and host-side refusals,
`BigVGAN.forward(x, lengths)`'s own checks, the text-list parser and batch planner of synthesize_batch.py, and the keyword
`execute_text_to_speech` grew."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from synthesize_batch import parse_textlist, plan_batches, synthetic_texts  # noqa: E402

from unitspeech_amd import UnitSpeech, _lib  # noqa: E402
from unitspeech_amd.vocoder import BigVGAN  # noqa: E402

TINY = {"resblock": "1", "upsample_rates": [4, 2, 2], "upsample_kernel_sizes": [8, 4, 4], "upsample_initial_channel": 32,
        "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]], "activation": "snake", "snake_logscale": False,
        "num_mels": 8}


def _args(header, name):
    m = re.search(rf"int {name}\(([^;]*)\);", header)
    assert m, f"{name} is not declared in include/unitspeech_hip.h"
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_prototypes_are_declared_registered_and_exported():
    with open(os.path.join(ROOT, "include", "unitspeech_hip.h")) as f:
        header = f.read()
    fwd = _args(header, "us_vocoder_forward_lengths")
    assert fwd == ["us_vocoder_handle h", "const float* mel", "const int64_t* lengths", "float* wav", "int B", "int Tmax", "void* workspace",
                   "size_t workspace_bytes", "us_stream stream"]
    dbg = _args(header, "us_vocoder_debug_layer_lengths")
    assert dbg == ["us_vocoder_handle h", "const char* prefix", "const float* in", "const float* res", "const float* sum", "float div",
                   "float* out", "int B", "int Tin_max", "const int64_t* lengths", "us_stream stream"]
    for name, args, at in (("us_vocoder_forward_lengths", fwd, 2), ("us_vocoder_debug_layer_lengths", dbg, 9)):
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(args) and argtypes[at] == C.POINTER(C.c_int64)
        assert hasattr(_lib.load(), name)
    # the uniform calls keep their signatures
    assert len(_lib.SIGNATURES["us_vocoder_forward"][1]) == 8 and len(_lib.SIGNATURES["us_vocoder_debug_layer"][1]) == 10
    assert len(_args(header, "us_vocoder_forward")) == 8 and len(_args(header, "us_vocoder_debug_layer")) == 10


def test_lengths_are_refused_on_the_host_before_any_device_work():
    """Null, too short and too long lengths are US_EINVAL with the item named; lengths in range pass on to the next check, the weights
    (never loaded here), so nothing was launched on the way."""
    lib = _lib.load()
    h = C.c_void_p()
    c = BigVGAN(TINY)._config_struct()
    assert lib.us_vocoder_create(C.byref(h), C.byref(c)) == 0
    p, T = 4096, 9                   # never dereferenced
    EINVAL, EWEIGHTS = -1, -4

    def run(lengths, B=3, Tmax=T):
        arr = None if lengths is None else (C.c_int64 * len(lengths))(*lengths)
        return lib.us_vocoder_forward_lengths(h, p, arr, p, B, Tmax, p, 1 << 30, None)

    def layer(lengths, B=3, Tmax=T, prefix=b"conv_pre"):
        arr = None if lengths is None else (C.c_int64 * len(lengths))(*lengths)
        return lib.us_vocoder_debug_layer_lengths(h, prefix, p, None, None, 0.0, p, B, Tmax, arr, None)

    for call, name in ((run, b"us_vocoder_forward_lengths"), (layer, b"us_vocoder_debug_layer_lengths")):
        assert call(None) == EINVAL and b"lengths is null" in lib.us_vocoder_last_error(h)
        assert call([9, 0, 4]) == EINVAL and name + b": lengths[1] = 0" in lib.us_vocoder_last_error(h)
        assert call([9, 4, 10]) == EINVAL and b"lengths[2] = 10" in lib.us_vocoder_last_error(h)
        assert call([-1, 4, 4]) == EINVAL and b"lengths[0] = -1" in lib.us_vocoder_last_error(h)
        assert call([9, 4, 1], B=0) == EINVAL and call([9, 4, 1], Tmax=0) == EINVAL
        assert call([9, 4, 1]) == EWEIGHTS
    assert layer([9, 4, 1], prefix=b"no.such.layer") == -2 and b"unknown layer" in lib.us_vocoder_last_error(h)
    # the item has its own grid dimension: a batch the uniform call refuses for its size reaches the next check
    B = 65535 // 32 + 1
    assert lib.us_vocoder_forward(h, p, p, B, T, p, 1 << 40, None) == EINVAL and run([T] * B, B=B) == EWEIGHTS
    lib.us_vocoder_destroy(h)


def test_the_module_checks_the_lengths_before_the_device():
    sig = inspect.signature(BigVGAN.forward)
    assert list(sig.parameters) == ["self", "x", "lengths"] and sig.parameters["lengths"].default is None
    assert inspect.signature(BigVGAN.debug_layer).parameters["lengths"].default is None
    m, x = BigVGAN(TINY), torch.zeros(3, 8, 5)
    with pytest.raises(ValueError, match=r"2 lengths for 3 items \(item 2 has none\)"):
        m(x, lengths=[5, 5])
    with pytest.raises(ValueError, match="4 lengths for 3 items"):
        m(x, lengths=torch.tensor([5, 5, 5, 5]))
    with pytest.raises(ValueError, match="integers"):
        m(x, lengths=torch.tensor([5.0, 5.0, 5.0]))
    with pytest.raises(ValueError, match="integers"):
        m(x, lengths=np.array([5.0, 5.0, 5.0]))
    with pytest.raises(ValueError, match="item 1"):
        m(x, lengths=[5, 2.5, 5])
    with pytest.raises(ValueError, match="item 0"):
        m(x, lengths=[True, 1, 1])
    with pytest.raises(ValueError, match="2 lengths for 3 items"):
        m.debug_layer("conv_pre", x, lengths=[5, 5])
    with pytest.raises(RuntimeError, match="ROCm device"):              # lengths in order: the next refusal is the device's
        m(x, lengths=np.array([5, 4, 1], dtype=np.int32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(x)


def _check_plan(symbols, max_batch, max_frames, per_symbol):
    batches = plan_batches(symbols, max_batch, max_frames, per_symbol)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(len(symbols))), "every utterance exactly once"
    for b in batches:
        assert 1 <= len(b) <= max_batch
        longest = max(symbols[i] for i in b)
        assert len(b) * longest * per_symbol <= max_frames or len(b) == 1, (b, longest)
    for prev, nxt in zip(batches, batches[1:]):                     # sorted by symbol count
        assert max(symbols[i] for i in prev) <= min(symbols[i] for i in nxt)
    return batches


def test_plan_batches_covers_every_utterance_within_both_bounds():
    g = np.random.Generator(np.random.Philox(key=12))
    for n, max_batch, max_frames, per_symbol in ((1, 4, 1000, 6), (7, 1, 10 ** 9, 6), (64, 8, 10 ** 9, 6), (64, 32, 4000, 6), (100, 5, 900, 3),
                                                 (33, 32, 16384, 8)):
        symbols = [int(v) for v in g.integers(3, 200, size=n)]
        batches = _check_plan(symbols, max_batch, max_frames, per_symbol)
        if max_frames >= 10 ** 9:
            assert len(batches) == -(-n // max_batch)                # only the item bound cuts: full batches, then the rest
    assert plan_batches([], 4, 100) == []
    # an utterance over the frame cap stays, alone; equal counts keep file order
    batches = _check_plan([10, 900, 12, 11, 500], 4, 200, 6)
    assert [1] in batches and [4] in batches and batches[0] == [0, 3] and batches[1] == [2]
    assert _check_plan([20] * 5, 2, 10 ** 6, 6) == [[0, 1], [2, 3], [4]]
    with pytest.raises(ValueError):
        plan_batches([5], 0, 100)
    with pytest.raises(ValueError):
        plan_batches([5], 1, 100, 0)
    with pytest.raises(ValueError, match="utterance 1"):
        plan_batches([5, 0], 2, 100)


def test_text_lists_and_synthetic_sentences():
    text = "one|hello there\n\n  two | with | a bar  \n"
    assert parse_textlist(text) == [("one", "hello there"), ("two", "with | a bar")]
    with pytest.raises(ValueError, match="line 2"):
        parse_textlist("a|x\nno bar here\n")
    with pytest.raises(ValueError, match="line 2"):
        parse_textlist("a|x\na|y\n")
    with pytest.raises(ValueError, match="line 1"):
        parse_textlist("a/b|x\n")
    items = synthetic_texts(5, 0)
    assert items == synthetic_texts(5, 0) and len({n for n, _ in items}) == 5 and all(t for _, t in items)
    # --synthetic 5 --batch 3: some batch holds utterances of different symbol counts, so the vocoder's batch is ragged
    symbols = [2 * len(t) + 1 for _, t in items]
    assert any(len({symbols[i] for i in b}) > 1 for b in plan_batches(symbols, 3, 16384))


def test_execute_text_to_speech_has_the_keyword_only_return_lengths():
    p = inspect.signature(UnitSpeech.execute_text_to_speech).parameters["return_lengths"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
