"""The HIP mel front end (csrc/mel.hip) on the GPU against the fp64 restatement of the reference's `mel_spectrogram`
(tools/mel_torch.py: the same fp32 filter bank and window upcast, so only the arithmetic differs).

Accuracy bar: E32 = max |fp32 CPU restatement - fp64| over a waveform's log-mel is the reference's own fp32 error; the library must be
within max(8 E32, 8 ulp(11.5) = 7.6e-6) of fp64.  The factor 8 covers an n_fft-term fp32 dot product against an FFT's ten butterfly stages
(sqrt(1024 / 10) ~ 10 in the worst case)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mel_torch import mel_spectrogram_torch, normalize  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.mel import MelSpectrogram, mel_spectrogram  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {
    # the reference's; lengths: one frame at the minimum legal length, not a multiple of hop (5 frames), 64 frames (both 32-frame sub-tiles
    # of one wave, none of the next), 129 frames (across the boundary of the 128-frame workgroup tile)
    "ref": (dict(n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0, fmax=8000),
            (385, 1500, 256 * 64 + 100, 256 * 129 + 17)),
    # another tap count (4 -> 4 with hop 16; 33 bins, 16 live) and a window shorter than n_fft; the same four kinds of length
    "small": (dict(n_fft=64, num_mels=8, sampling_rate=16000, hop_size=16, win_size=48, fmin=0, fmax=4000),
              (25, 100, 16 * 64 + 5, 16 * 129 + 3)),
}
KINDS = ("noise", "sine", "gap", "walk")
FLOOR = 8 * 2.0 ** -20                  # 8 ulp of 11.5 (|log 1e-5|): 7.6e-6


def waveform(kind, T, sr, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    t = np.arange(T) / sr
    if kind == "noise":                 # white noise at 0.3
        y = 0.3 * g.standard_normal(T)
    elif kind == "sine":                # quiet bands beside a loud one
        y = 0.9 * np.sin(2 * np.pi * 440.0 * t) + 1e-4 * g.standard_normal(T)
    elif kind == "gap":                 # noise between two stretches of exact zeros
        y = 0.3 * g.standard_normal(T)
        y[:T // 3] = 0.0
        y[T - T // 3:] = 0.0
    else:                               # amplitude-modulated integrated noise
        y = np.cumsum(g.standard_normal(T))
        y = 0.9 * y / np.abs(y).max() * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t))
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request):
    cfg, lengths = CONFIGS[request.param]
    m = MelSpectrogram(**cfg).cuda()
    return request.param, cfg, lengths, m


def restate(m, cfg, y, dtype):
    return mel_spectrogram_torch(y.cpu(), m.mel_basis.cpu(), m.window.cpu(), cfg["n_fft"], cfg["hop_size"], cfg["win_size"], dtype=dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_against_fp64(setup, kind):
    name, cfg, lengths, m = setup
    for T in lengths:
        y = waveform(kind, T, cfg["sampling_rate"], 100 + T)[None]
        r64 = restate(m, cfg, y, torch.float64)
        e32 = float((restate(m, cfg, y, torch.float32).double() - r64).abs().max())
        got = m(y.cuda())
        assert tuple(got.shape) == (1, cfg["num_mels"], T // cfg["hop_size"]) and got.dtype == torch.float32
        err = float((got.cpu().double() - r64).abs().max())
        bound = max(8 * e32, FLOOR)
        print(f"\nmel[{name}] {kind} T={T}: |hip - fp64| {err:.3e}, E32 {e32:.3e}, ratio {err / max(e32, 1e-30):.2f}, bound {bound:.3e}")
        assert math.isfinite(err) and err <= bound


def test_silence_is_the_clamp(setup):
    name, cfg, lengths, m = setup
    got = m(torch.zeros(2, lengths[1], device="cuda"))
    err = float((got.double() - math.log(1e-5)).abs().max())
    print(f"\nmel[{name}] silence: |hip - log(1e-5)| {err:.3e}")
    assert err <= FLOOR


def test_batch_items_equal_the_items_alone(setup):
    """Three lengths in one buffer, the tail of each row NaN: valid frames bit-identical to the item run alone (at its own Tmax), frames
    past an item's count equal pad_value, everything finite."""
    name, cfg, lengths, m = setup
    lens = [lengths[0], lengths[1], lengths[3]]
    hop, Tmax = cfg["hop_size"], max(lens)
    wav = torch.full((3, Tmax), float("nan"))
    for b, n in enumerate(lens):
        wav[b, :n] = waveform(KINDS[b], n, cfg["sampling_rate"], 7 + b)
    wav = wav.cuda()
    pad = -7.25
    got = m(wav, lengths=lens, pad_value=pad)
    assert tuple(got.shape) == (3, cfg["num_mels"], Tmax // hop) and torch.isfinite(got).all()
    for b, n in enumerate(lens):
        alone = m(wav[b, :n].clone())
        assert alone.shape[-1] == n // hop
        assert torch.equal(got[b, :, :n // hop], alone[0]), (b, n)
        assert (got[b, :, n // hop:] == pad).all()
    # lengths as a tensor, and the same call again: the same bits
    again = m(wav, lengths=torch.tensor(lens), pad_value=pad)
    assert torch.equal(again, got)


def test_normalisation_is_the_torch_expression_on_the_raw_output(setup):
    name, cfg, lengths, m = setup
    y = waveform("walk", lengths[2], cfg["sampling_rate"], 3)[None].cuda()
    raw = m(y)
    g = torch.Generator().manual_seed(5)
    per_min = (-11.5 + torch.rand(cfg["num_mels"], generator=g)).cuda()
    per_max = (1.0 + 2 * torch.rand(cfg["num_mels"], generator=g)).cuda()
    for mn, mx in ((torch.tensor(-11.5129, device="cuda"), torch.tensor(2.0737, device="cuda")), (per_min, per_max)):
        got = m(y, mel_min=mn, mel_max=mx)
        want = normalize(raw, mn.reshape(1, -1, 1), mx.reshape(1, -1, 1))          # finetune.py:104 evaluated by torch on the device
        assert torch.equal(got, want)
    assert torch.equal(m(y, mel_min=-11.5, mel_max=2.0), normalize(raw, torch.tensor(-11.5, device="cuda"), torch.tensor(2.0, device="cuda")))


def test_minmax_over_valid_frames(setup):
    name, cfg, lengths, m = setup
    lens = [lengths[3], lengths[1], lengths[2]]
    hop, Tmax = cfg["hop_size"], max(lens)
    wav = torch.zeros(3, Tmax)
    for b, n in enumerate(lens):
        wav[b, :n] = waveform(KINDS[b + 1], n, cfg["sampling_rate"], 11 + b)
    raw = m(wav.cuda(), lengths=lens, pad_value=1e9)
    frames = [n // hop for n in lens]
    lo, hi = m.minmax(raw, frames)
    valid = torch.cat([raw[b, :, :f] for b, f in enumerate(frames)], dim=1)
    assert torch.equal(lo, valid.amin(dim=1)) and torch.equal(hi, valid.amax(dim=1))
    lo_all, hi_all = m.minmax(raw[:, :, :frames[1]])
    assert torch.equal(lo_all, raw[:, :, :frames[1]].amin(dim=(0, 2))) and torch.equal(hi_all, raw[:, :, :frames[1]].amax(dim=(0, 2)))


def test_drop_in_function_equals_the_module(setup):
    name, cfg, lengths, m = setup
    y = torch.stack([waveform("noise", lengths[1], cfg["sampling_rate"], 1), waveform("sine", lengths[1], cfg["sampling_rate"], 2)]).cuda()
    got = mel_spectrogram(y, cfg["n_fft"], cfg["num_mels"], cfg["sampling_rate"], cfg["hop_size"], cfg["win_size"], cfg["fmin"], cfg["fmax"],
                          center=False)
    assert torch.equal(got, m(y))
    assert torch.equal(mel_spectrogram(y, cfg["n_fft"], cfg["num_mels"], cfg["sampling_rate"], cfg["hop_size"], cfg["win_size"], cfg["fmin"],
                                       cfg["fmax"]), got)


def test_more_items_than_one_launch_takes():
    """The lengths travel as kernel arguments, 64 items per launch: item 64 and on go through a second launch."""
    cfg, lengths = CONFIGS["small"]
    m = MelSpectrogram(**cfg).cuda()
    B, T = 67, 200
    wav = torch.stack([waveform("noise", T, cfg["sampling_rate"], 40 + b) for b in range(B)]).cuda()
    lens = [T - (b % 5) * 17 for b in range(B)]
    got = m(wav, lengths=lens, pad_value=0.5)
    for b in (0, 63, 64, 66):
        f = lens[b] // cfg["hop_size"]
        assert torch.equal(got[b, :, :f], m(wav[b, :lens[b]].clone())[0]) and (got[b, :, f:] == 0.5).all()
    lo, hi = m.minmax(got, [n // cfg["hop_size"] for n in lens])
    valid = torch.cat([got[b, :, :lens[b] // cfg["hop_size"]] for b in range(B)], dim=1)
    assert torch.equal(lo, valid.amin(dim=1)) and torch.equal(hi, valid.amax(dim=1))


def test_refusals():
    ref = CONFIGS["ref"][0]
    y = torch.zeros(1, 4096, device="cuda")
    with pytest.raises(RuntimeError, match="EINVAL"):                 # hop does not divide n_fft
        MelSpectrogram(**{**ref, "hop_size": 300})(y)
    with pytest.raises(RuntimeError, match="EINVAL"):
        MelSpectrogram(**{**ref, "win_size": 2048})(y)
    with pytest.raises(RuntimeError, match="EINVAL"):
        MelSpectrogram(**{**ref, "n_fft": 8192, "win_size": 1024})(torch.zeros(1, 16384, device="cuda"))
    with pytest.raises(RuntimeError, match="EINVAL"):                 # n_fft - hop odd
        MelSpectrogram(**{**ref, "hop_size": 1})(y)
    m = MelSpectrogram(**ref).cuda()
    with pytest.raises(RuntimeError, match="EINVAL"):                 # the reflection needs more than (n_fft - hop) / 2 = 384 samples
        m(y, lengths=[384])
    with pytest.raises(RuntimeError, match="EINVAL"):
        m(y[:, :384])
    with pytest.raises(RuntimeError, match="EINVAL"):
        m(y, lengths=[4097])
    assert tuple(m(y, lengths=[385]).shape) == (1, 80, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):            # a waveform that is not on a GPU
        m(torch.zeros(1, 4096))
    if torch.cuda.device_count() > 1:                                 # the handle lives on cuda:0; a call with cuda:1 current is refused
        lib = _lib.load()
        out = torch.empty(1, 80, 16, device="cuda:0")
        ws = torch.empty(lib.us_mel_workspace_bytes(m._h, 1, 4096), dtype=torch.uint8, device="cuda:0")
        with torch.cuda.device(1):
            rc = lib.us_mel_forward(m._h, y.data_ptr(), None, 1, 4096, None, None, 0, 0.0, out.data_ptr(), ws.data_ptr(), ws.numel(), None)
        assert rc == -1 and b"current device" in lib.us_mel_last_error(m._h)
    lib = _lib.load()
    assert lib.us_mel_frames(m._h, 4097) == 16 and lib.us_mel_num_weights(m._h) == 2
    assert [lib.us_mel_weight_key(m._h, i) for i in range(2)] == [b"mel_basis", b"window"]
