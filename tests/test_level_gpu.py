"""unitspeech_amd.level (csrc/level.hip) on the device against the fp64 numpy yardstick tools/level_numpy.py: exact activity counts, the
level to fp64 libm noise, exact int16 output, bitwise independence of the batch an item lies in.

Every input is first pushed through the yardstick and must be decidable: no q[k] within a relative 1e-9 of a threshold (re-association
moves q by about 1e-13) and no value within 1e-6 LSB of a rounding tie.  An input that is not decidable fails the test and is to be
changed; nothing is skipped."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import level_numpy as L  # noqa: E402

pytestmark = pytest.mark.gpu

Q_MARGIN, TIE_MARGIN = 1e-9, 1e-6


def chunk():
    from unitspeech_amd import level
    return level.chunk()


def placed_bursts(n, bursts, seed):
    """int16 [n]: uniform noise of amplitude amp on [start, end) for each (start, end, amp), zeros elsewhere."""
    g = np.random.Generator(np.random.Philox(key=5100 + seed))
    x = np.zeros(n, dtype=np.float64)
    for start, end, amp in bursts:
        x[start:min(end, n)] = amp * g.uniform(-1.0, 1.0, size=max(0, min(end, n) - start))
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rate, int16 signal): built around the chunk size C so that burst ends, gaps and hangovers fall on the seams."""
    C = chunk()
    if name == "seams16k":       # I = 3200: burst ends inside the last I samples of a chunk, short and long gaps over the seams at C, 2C, 3C
        b = [(0, C - 10, 0.2), (C + 500, 2 * C - 1000, 0.01), (2 * C + 3000, 3 * C - 1, 0.4), (3 * C + 5, 3 * C + 17, 0.003)]
        return 16000, placed_bursts(3 * C + 17, b, 1)
    if name == "hang48k":        # I = 9600 > 2 C: the hangover of the burst ending in chunk 0 runs through chunks 1 and 2 into chunk 3
        assert L.constants(48000)[1] > 2 * C
        b = [(0, C // 3, 0.9), (4 * C - 50, 4 * C + 700, 0.05), (4 * C + 1500, 5 * C + 33, 0.002)]
        return 48000, placed_bursts(5 * C + 33, b, 2)
    if name == "bursts8k":
        return 8000, L.burst_signal(2 * C + 100, 8000, seed=4)
    if name == "bursts16k":
        return 16000, L.burst_signal(3 * C + 17, 16000, seed=7)
    if name == "peaky":          # quiet noise with a few full-scale spikes: normalising to -3 dB saturates both ways
        x = placed_bursts(2 * C + 40, [(0, 2 * C + 40, 0.02)], 3).astype(np.int32)
        x[[300, 5000, 2 * C + 7]] = 30000
        x[[900, C + 1, 2 * C - 3]] = -30000
        return 16000, x.astype(np.int16)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def yardstick(name, n=None):
    """The yardstick's measurement of the first n samples of a case, decidability asserted."""
    rate, x = case(name)
    x = x if n is None else x[:n]
    m = L.threshold_margin(L.envelope(L.to_full_scale(x), rate))
    assert m >= Q_MARGIN, f"{name}[:{n}]: q comes within {m:.2e} of a threshold; change the input"
    return L.active_speech_level(x, rate)


def decidable_rounding(x, factor, what):
    m = L.tie_margin(L.scaled_lsb(x, factor))
    assert m >= TIE_MARGIN, f"{what}: a value lies {m:.2e} LSB from a rounding tie; change the input"


def bits(t):
    return t.detach().cpu().reshape(-1).view(torch.int64) if t.dtype == torch.float64 else t.detach().cpu()


def check_level(got, want, b=0):
    assert np.array_equal(got.counts[b].cpu().numpy(), want.counts), (got.counts[b].tolist(), want.counts.tolist())
    for f in ("level_db", "rms_db", "activity"):
        g, w = float(getattr(got, f)[b]), float(getattr(want, f))
        print(f"{f}: device {g!r} yardstick {w!r}")
        assert abs(g - w) <= 1e-9, (f, g, w)
    assert float(got.peak[b]) == want.peak


@pytest.mark.parametrize("which", ["1", "C-1", "C", "C+1", "3C+17"])
def test_counts_exact_at_the_seams(which):
    from unitspeech_amd import level
    C = chunk()
    n = {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "3C+17": 3 * C + 17}[which]
    rate, x = case("seams16k")
    want = yardstick("seams16k", n)
    got = level.active_speech_level(torch.from_numpy(x[:n].copy()).cuda(), rate)
    check_level(got, want)
    if n >= C:
        assert want.counts[0] > 0 and want.level_db > -100.0


@pytest.mark.parametrize("name", ["hang48k", "bursts8k", "bursts16k"])
def test_counts_exact_other_rates(name):
    from unitspeech_amd import level
    rate, x = case(name)
    want = yardstick(name)
    assert want.level_db > -100.0 and want.counts[0] > want.counts[5] > 0
    check_level(level.active_speech_level(torch.from_numpy(x).cuda(), rate), want)
    xf = torch.from_numpy(L.to_full_scale(x).astype(np.float32)).cuda()        # s / 32768 is exact in fp32: the float entry sees the same samples
    check_level(level.active_speech_level(xf, rate), want)


def test_hangover_spans_more_than_two_chunks():
    C = chunk()
    rate, x = case("hang48k")
    hang = L.constants(rate)[1]
    want = yardstick("hang48k")
    # threshold 12 (2^-3) is reached by the first burst alone, in chunk 0; its hangover runs through all of chunks 1 and 2 into chunk 3
    above = np.nonzero(L.envelope(L.to_full_scale(x), rate) >= 2.0 ** -3)[0]
    assert above.size and above.max() < C and 3 * C < above.max() + hang < len(x)
    assert want.counts[12] == above.max() - above.min() + 1 + hang


def test_shift_law_on_the_device():
    from unitspeech_amd import level
    rate, x = case("bursts16k")
    yardstick("bursts16k")
    h = (L.to_full_scale(x) * 0.5).astype(np.float32)                           # exact in fp32, and so is 2 h
    assert L.threshold_margin(L.envelope(h.astype(np.float64), rate)) >= Q_MARGIN
    a = level.active_speech_level(torch.from_numpy(h).cuda(), rate)
    b = level.active_speech_level(torch.from_numpy(2 * h).cuda(), rate)
    ca, cb = a.counts[0].cpu().numpy(), b.counts[0].cpu().numpy()
    assert np.array_equal(cb[1:], ca[:-1]) and ca[0] > ca[3] > 0
    assert abs(float(b.level_db[0]) - float(a.level_db[0]) - 20 * math.log10(2.0)) <= 1e-9
    assert abs(float(b.activity[0]) - float(a.activity[0])) <= 1e-9


@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("out_int16", [True, False])
def test_ragged_batch_has_the_bits_of_each_item_alone(pad, out_int16):
    from unitspeech_amd import level
    C = chunk()
    rate, x = case("seams16k")
    _, y = case("bursts16k")
    T = 3 * C + 17 + pad                                           # 3 C + 24 is a multiple of 8: the rows take the 16-byte path
    lens = [3 * C + 17, 0, C + 1, 777, 2 * C - 5]
    batch = np.full((5, T), 12345, dtype=np.int16)                 # whatever lies past an item's length is never read
    batch[0, :lens[0]] = x
    batch[2, :lens[2]] = y[:lens[2]]
    batch[3, :lens[3]] = 0
    batch[4, :lens[4]] = y[100:100 + lens[4]]
    dev = torch.from_numpy(batch).cuda()
    out, info = level.normalize_level(dev, rate, -26.0, lengths=lens, out_int16=out_int16)
    out2, info2 = level.normalize_level(dev, rate, -26.0, lengths=torch.tensor(lens), out_int16=out_int16)
    assert torch.equal(out, out2)
    for f in info._fields:
        assert torch.equal(bits(getattr(info, f)), bits(getattr(info2, f))), f
    assert out.shape == dev.shape and out.dtype == (torch.int16 if out_int16 else torch.float32)
    for b, n in enumerate(lens):
        assert not out[b, n:].any(), b
        if n == 0:
            assert float(info.level_db[b]) == -100.0 and float(info.activity[b]) == 0.0 and float(info.gain[b]) == 1.0
            assert not info.counts[b].any() and int(info.clipped[b]) == 0
            continue
        alone, ia = level.normalize_level(torch.from_numpy(batch[b, :n].copy()).cuda(), rate, -26.0, out_int16=out_int16)
        assert torch.equal(out[b, :n], alone), b
        for f in info._fields:
            assert torch.equal(bits(getattr(info, f)[b]), bits(getattr(ia, f)[0])), (b, f)
    assert float(info.level_db[3]) == -100.0 and float(info.gain[3]) == 1.0 and float(info.level_db[0]) > -100.0


@pytest.mark.parametrize("name", ["seams16k", "hang48k", "bursts8k"])
def test_sv56_drop_in(name):
    from unitspeech_amd import level
    rate, x = case(name)
    want = yardstick(name)
    decidable_rounding(x, L.gain_factor(want.level_db, -26.0), name)
    got = level.sv56(x, rate, -26.0)
    assert got.dtype == np.int16 and np.array_equal(got, L.sv56(x, rate, -26.0))


def test_sv56_saturates_and_counts_clipped_samples():
    from unitspeech_amd import level
    rate, x = case("peaky")
    want = yardstick("peaky")
    f = L.gain_factor(want.level_db, -3.0)
    decidable_rounding(x, f, "peaky")
    ref, clipped = L.round_saturate(L.scaled_lsb(x, f))
    assert clipped >= 6 and ref.max() == 32767 and ref.min() == -32768
    out, info = level.normalize_level(torch.from_numpy(x).cuda(), rate, -3.0, out_int16=True)
    assert np.array_equal(out.cpu().numpy(), ref) and int(info.clipped[0]) == clipped
    assert abs(float(info.gain[0]) - f) <= 1e-9 * f
    assert np.array_equal(level.sv56(x, rate, -3.0), ref)


def float_signal(n, rate, seed):
    return np.clip(L.burst_signal(n, rate, seed, amplitudes=(0.4, 0.001, 0.1, 0.02), int16=False) * np.float32(3.0), -1.0, 1.0).astype(np.float32)


def test_via_int16_takes_the_reference_route():
    from unitspeech_amd import level
    C, rate = chunk(), 22050
    x = float_signal(2 * C + 24, rate, 11)
    s = L.quantize_reference(x)
    assert np.array_equal(s, (x * 32767).astype(np.int16)) and np.abs(x).max() == 1.0
    want = L.active_speech_level(s, rate)
    assert L.threshold_margin(L.envelope(L.to_full_scale(s), rate)) >= Q_MARGIN and want.level_db > -100.0
    decidable_rounding(s, L.gain_factor(want.level_db, -26.0), "via_int16")
    for shape in ((-1,), (1, 1, -1)):
        out, info = level.normalize_level(torch.from_numpy(x).cuda().reshape(shape), rate, -26.0, via_int16=True, out_int16=True)
        assert out.shape == torch.from_numpy(x).reshape(shape).shape and out.dtype == torch.int16
        assert np.array_equal(out.cpu().numpy().reshape(-1), L.sv56(s, rate, -26.0))
        check_level(info, want)


@pytest.mark.parametrize("n_extra", [0, 5])
def test_float_path_within_one_ulp(n_extra):
    from unitspeech_amd import level
    C, rate = chunk(), 22050
    x = float_signal(C + 8 + n_extra, rate, 12)
    want = L.active_speech_level(x, rate)
    assert L.threshold_margin(L.envelope(x.astype(np.float64), rate)) >= Q_MARGIN and want.level_db > -100.0
    f = L.gain_factor(want.level_db, -26.0)
    ref = (x.astype(np.float64) * f).astype(np.float32)
    out, info = level.normalize_level(torch.from_numpy(x).cuda(), rate, -26.0)
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))
    check_level(info, want)
    assert abs(float(info.gain[0]) - f) <= 1e-9 * f and int(info.clipped[0]) == 0


def test_degenerate_items_come_back_unchanged():
    from unitspeech_amd import level
    C, rate = chunk(), 16000
    z = torch.zeros(C + 3, dtype=torch.int16).cuda()
    out, info = level.normalize_level(z, rate, -26.0, out_int16=True)
    assert float(info.level_db[0]) == -100.0 and float(info.gain[0]) == 1.0 and torch.equal(out, z)
    _, x = case("bursts16k")
    quiet = torch.from_numpy((L.to_full_scale(x[:C + 3]) * 2.0 ** -16).astype(np.float32)).cuda()     # the envelope never reaches 2^-15
    out, info = level.normalize_level(quiet, rate, -26.0)
    assert float(info.level_db[0]) == -100.0 and float(info.activity[0]) == 0.0 and torch.equal(out, quiet)
    f = torch.from_numpy(L.to_full_scale(x[:2 * C]).astype(np.float32)).cuda().repeat(2, 1)
    f[1, C + 9] = float("nan")
    out, info = level.normalize_level(f, rate, -26.0)
    assert math.isnan(float(info.level_db[1])) and float(info.gain[1]) == 1.0
    assert torch.equal(out[1].view(torch.int32), f[1].view(torch.int32))                                # unchanged, the NaN included
    assert float(info.level_db[0]) > -100.0 and float(info.gain[0]) != 1.0                              # its neighbour is not affected
    alone, _ = level.normalize_level(f[0].clone(), rate, -26.0)
    assert torch.equal(out[0], alone)
    f[1, C + 9] = float("inf")
    assert math.isnan(float(level.active_speech_level(f, rate).level_db[1]))


def raw_call(wav, lens, T, rate, out, ndb=-26.0, in_code=None, out_code=None, B=None):
    """The two C calls on torch buffers -> (rc of measure, rc of apply)."""
    from unitspeech_amd import _lib
    lib = _lib.load()
    B = len(lens) if B is None else B
    in_code = (_lib.US_LEVEL_I16 if wav.dtype == torch.int16 else _lib.US_LEVEL_F32) if in_code is None else in_code
    out_code = (_lib.US_LEVEL_I16 if out.dtype == torch.int16 else _lib.US_LEVEL_F32) if out_code is None else out_code
    n = int(lib.us_level_workspace_bytes(min(B, 65535), T)) or 4096
    ws = torch.empty(n, dtype=torch.uint8, device=wav.device)
    stats = torch.zeros(max(len(lens), 1), 8, dtype=torch.float64, device=wav.device)
    counts = torch.zeros(max(len(lens), 1), 15, dtype=torch.int64, device=wav.device)
    ln = torch.tensor(lens, dtype=torch.int64, device=wav.device)
    s = torch.cuda.current_stream().cuda_stream
    r1 = lib.us_level_measure(wav.data_ptr(), in_code, 0, ln.data_ptr(), B, T, rate, stats.data_ptr(), counts.data_ptr(), ws.data_ptr(), n, s)
    r2 = lib.us_level_apply(wav.data_ptr(), in_code, 0, ln.data_ptr(), B, T, stats.data_ptr(), ndb, out.data_ptr(), out_code, None, None,
                            ws.data_ptr(), n, s)
    torch.cuda.synchronize()
    return r1, r2, stats


@pytest.mark.parametrize("T_extra", [3, 8])
def test_nothing_is_written_past_the_rows(T_extra):
    C = chunk()
    rate, x = case("bursts16k")
    T, lens, pad = C + T_extra, [C + 1, 40], 64
    wav = torch.zeros(2, T, dtype=torch.int16)
    wav[0, :lens[0]] = torch.from_numpy(x[:lens[0]].copy())
    wav[1] = torch.from_numpy(x[C:C + T].copy())
    for dtype, poison in ((torch.int16, 0x5a5a), (torch.float32, 777.0)):
        buf = torch.full((2 * T + pad,), poison, dtype=dtype).cuda()
        r1, r2, stats = raw_call(wav.cuda(), lens, T, rate, buf)
        assert (r1, r2) == (0, 0)
        out = buf[:2 * T].view(2, T).cpu()
        assert bool((buf[2 * T:] == poison).all())
        for b, n in enumerate(lens):
            assert not out[b, n:].any()
        assert out[0, :lens[0]].any()
        f = L.gain_factor(L.active_speech_level(wav[0, :lens[0]].numpy(), rate).level_db, -26.0)
        if dtype == torch.int16:
            assert np.array_equal(out[0, :lens[0]].numpy(), L.round_saturate(L.scaled_lsb(wav[0, :lens[0]].numpy(), f))[0])


def test_refusals():
    from unitspeech_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    wav = torch.zeros(1, 64, dtype=torch.int16).cuda()
    out = torch.zeros(1, 64, dtype=torch.int16).cuda()
    assert raw_call(wav, [64], 64, 16000, out)[:2] == (0, 0)
    assert raw_call(wav, [64], 64, 0, out)[0] == EINVAL
    assert raw_call(wav, [64], 64, -16000, out)[0] == EINVAL
    assert raw_call(wav, [64], 64, 16000, out, B=65536)[:2] == (EINVAL, EINVAL)
    assert raw_call(wav, [64], 64, 16000, out, in_code=7)[:2] == (EINVAL, EINVAL)
    assert raw_call(wav, [64], 64, 16000, out, out_code=2)[1] == EINVAL
    assert raw_call(wav, [64], (1 << 30) + 1, 16000, out)[:2] == (EINVAL, EINVAL)
    assert lib.us_level_workspace_bytes(65536, 64) == 0 and lib.us_level_workspace_bytes(1, (1 << 30) + 1) == 0
    assert lib.us_level_workspace_bytes(0, 64) == 0 and lib.us_level_workspace_bytes(1, 0) == 0
    assert lib.us_level_workspace_bytes(65535, 64) > 0 and lib.us_level_workspace_bytes(1, 1 << 30) > 0
    from unitspeech_amd import level
    with pytest.raises(RuntimeError):
        level.active_speech_level(torch.zeros(100), 16000)                     # not on the GPU: there is no CPU fallback
    with pytest.raises(ValueError):
        level.active_speech_level(wav, 0)
