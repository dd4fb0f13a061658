"""What the command-line tools share: `unitspeech_amd.batching` (plan_batches, pad_batch), `unitspeech_amd.audio.read_wav`, and
`_args.call`, the one way into a plain library function.  Only the last test touches a device."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unitspeech_amd import _args, _lib  # noqa: E402
from unitspeech_amd.audio import read_wav  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402


def test_plan_batches_uncapped_is_the_capped_plan_with_a_cap_nothing_reaches():
    g = np.random.Generator(np.random.Philox(key=21))
    for n, max_batch in ((1, 4), (7, 1), (64, 8), (33, 32), (100, 5)):
        lengths = [int(v) for v in g.integers(1, 160000, size=n)]
        assert plan_batches(lengths, max_batch) == plan_batches(lengths, max_batch, 10 ** 15)
    assert plan_batches([5, 3, 9, 3], 3) == [[1, 3, 0], [2]]
    assert plan_batches([], 2) == []


def test_plan_batches_uncapped_accepts_a_zero_length_and_the_cap_refuses_it():
    assert plan_batches([4, 0, 2], 2) == [[1, 2], [0]]
    with pytest.raises(ValueError, match="utterance 1"):
        plan_batches([4, 0, 2], 2, 100)
    for bad in ((0, None), (2, 0)):
        with pytest.raises(ValueError):
            plan_batches([4], *bad)


def test_pad_batch_keeps_the_dtype_and_zero_fills():
    g = np.random.Generator(np.random.Philox(key=22))
    arrays = [g.integers(-3000, 3000, size=n).astype(np.int16) for n in (5, 0, 9, 1)]
    tensors = [torch.from_numpy(g.standard_normal(n, dtype=np.float32)) for n in (3, 8, 2)]
    for items, dtype in ((arrays, torch.int16), (tensors, torch.float32)):
        x, n = pad_batch(items)
        assert n == [len(v) for v in items] and x.dtype == dtype and x.device.type == "cpu" and tuple(x.shape) == (len(items), max(n))
        for b, v in enumerate(items):
            assert torch.equal(x[b, :n[b]], torch.as_tensor(v)) and not x[b, n[b]:].any()


def test_read_wav_both_ways(tmp_path):
    from scipy.io import wavfile
    g = np.random.Generator(np.random.Philox(key=23))
    s = g.integers(-30000, 30000, size=600).astype(np.int16)
    t = g.integers(-30000, 30000, size=600).astype(np.int16)
    as_f32 = s.astype(np.float32) / 32768.0
    i32 = g.integers(-2 ** 31, 2 ** 31, size=600).astype(np.int32)
    u8 = g.integers(0, 256, size=600).astype(np.uint8)
    f32 = g.uniform(-1, 1, size=600).astype(np.float32)
    stereo = np.stack([s, t], axis=1)
    # name -> (what is written, what comes back without keep_int16, what comes back with it)
    cases = {"mono": (s, as_f32, s), "column": (s[:, None], as_f32, s),
             "stereo": (stereo, (stereo.astype(np.float32) / 32768.0).mean(axis=1), None),
             "int32": (i32, i32.astype(np.float32) / float(2 ** 31), None),
             "uint8": (u8, (u8.astype(np.float32) - 128.0) / 128.0, None), "float32": (f32, f32, None)}
    for name, (data, plain, kept) in cases.items():
        path = str(tmp_path / f"{name}.wav")
        wavfile.write(path, 8000, data)
        for keep, want in ((False, plain), (True, plain if kept is None else kept)):
            x, rate = read_wav(path, keep_int16=keep)
            assert rate == 8000 and type(rate) is int, name
            assert x.dtype == want.dtype and x.shape == (600,) and x.flags["C_CONTIGUOUS"] and np.array_equal(x, want), (name, keep)


class _StubLibrary:
    def __init__(self, rc):
        self.rc, self.seen = rc, None

    def us_stub(self, *args):
        self.seen = args
        return self.rc

    def us_last_error(self, handle):
        assert handle is None
        return b"us_stub: no"


def _stubbed(monkeypatch, rc):
    lib, devices = _StubLibrary(rc), []

    @contextlib.contextmanager
    def device(dev):
        devices.append(dev)
        yield

    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(_args, "stream", lambda: "the stream")
    return lib, devices


def test_call_converts_the_arguments_and_appends_the_stream(monkeypatch):
    lib, devices = _stubbed(monkeypatch, 0)
    a, b = torch.arange(4, dtype=torch.float32), torch.arange(6, dtype=torch.int64)[2:]
    assert _args.call("dev", "us_stub", a, None, 3, 0.5, b) is None
    assert lib.seen == (a.data_ptr(), None, 3, 0.5, b.data_ptr(), "the stream")
    assert devices == ["dev"]


def test_call_raises_under_the_symbols_name(monkeypatch):
    _stubbed(monkeypatch, -1)
    with pytest.raises(RuntimeError) as e:
        _args.call("dev", "us_stub", None)
    assert str(e.value) == "libunitspeech_hip: us_stub failed with EINVAL: us_stub: no"
    assert str(e.value).startswith("libunitspeech_hip: us_stub failed with")


def test_f32_detaches_unless_told_not_to():
    x = torch.ones(3, dtype=torch.float64, requires_grad=True)
    assert _args.f32(None, "cpu") is None
    y = _args.f32(x, "cpu")
    assert y.dtype == torch.float32 and y.is_contiguous() and not y.requires_grad
    assert _args.f32(x, "cpu", detach=False).requires_grad


@pytest.mark.gpu
def test_a_plain_entry_points_refusal_reaches_the_caller_through_call():
    dev = torch.device("cuda", 0)
    centers = torch.zeros(4, 8, device=dev)
    packed = torch.empty(4096, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError) as e:
        _args.call(dev, "us_units_pack_centers", centers, 0, 8, packed, packed.numel())        # K = 0: refused before any launch
    assert str(e.value).startswith("libunitspeech_hip: us_units_pack_centers failed with EINVAL: us_units_pack_centers: ")
    assert "K = 0, D = 8" in str(e.value)
