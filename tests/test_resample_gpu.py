"""The HIP resampler (csrc/resample.hip) on the GPU against the fp64 restatement of torchaudio's strided convolution
(tools/resample_torch.py: the same fp32 kernel upcast, so only the arithmetic differs).

Five configurations: new' = 320 (whole 64-row tiles), 441 (a last tile with 57 live rows), 2 and 1 (one nearly empty tile); K = 459, 334 and
629 (a partial second tap, not a multiple of 16) and 23 and 41 with Cin = 3 (8 and 14 taps, the last partial).  Lengths per configuration:
1 and orig' - 1 (one frame), 64 orig' (an exact multiple: torchaudio's spare frame is not needed; 64 frames are both 32-frame sub-tiles of one
wave and none of the next), 64 orig' + 1 (one sample over) and 129 orig' + 5 (130 frames, across the 128-frame workgroup tile).

Accuracy bar: E32 = max |fp32 CPU restatement - fp64| is torchaudio's own fp32 error and B_i = sum_k |kernel| |y| the magnitude an output is
summed from; the library must be within max(4 E32, 8 * 2^-24 * max_i B_i) of fp64.  A numpy fp32 emulation that adds the K products strictly
in order gave 0.70-1.83 E32 over the four hann configurations and the four inputs (E32 0.5-2.0e-7, the floor 3.4-7.8e-7; E32 is exactly 0 for
DC at one sample, hence the floor); the factor 4 leaves about 2x for the MFMA's pair-wise inner addition.
Ratios measured on an MI355X: not measured yet (DESIGN.md section 13 has the CPU emulation of the kernels' summation order)."""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resample_torch import resample_torch  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.resample import Resample, resample  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (orig_freq, new_freq, keyword arguments)
CONFIGS = {
    "22k_16k": (22050, 16000, {}),
    "16k_22k": (16000, 22050, {}),
    "24k_16k": (24000, 16000, {}),
    "48k_16k": (48000, 16000, {}),
    "kaiser": (22050, 16000, dict(resampling_method="sinc_interp_kaiser", lowpass_filter_width=64, rolloff=0.9475937167399596)),
}
KINDS = ("noise", "sine", "dc", "walk")


def lengths_of(orig):
    return (1, max(orig - 1, 1), 64 * orig, 64 * orig + 1, 129 * orig + 5)


def waveform(kind, T, sr, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    t = np.arange(T) / sr
    if kind == "noise":                 # white noise at 0.3
        y = 0.3 * g.standard_normal(T)
    elif kind == "sine":                # a smooth signal with a noise floor
        y = 0.9 * np.sin(2 * np.pi * 440.0 * t) + 1e-4 * g.standard_normal(T)
    elif kind == "dc":
        y = np.full(T, 0.75)
    else:                               # amplitude-modulated integrated noise
        y = np.cumsum(g.standard_normal(T))
        y = 0.9 * y / max(np.abs(y).max(), 1e-30) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t))
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request):
    of, nf, kw = CONFIGS[request.param]
    m = Resample(of, nf, **kw).cuda()
    return request.param, of, m


_refs = {}


def reference(name, m, of, kind, L):
    """(waveform, fp64 restatement, E32, max_i B_i), computed once per case"""
    key = (name, kind, L)
    if key not in _refs:
        y = waveform(kind, L, of, 100 + L)
        k = m.kernel.cpu()
        r64 = resample_torch(y, k, m.width, m.orig, m.new, torch.float64)
        e32 = float((resample_torch(y, k, m.width, m.orig, m.new, torch.float32).double() - r64).abs().max())
        mag = float(resample_torch(y.abs(), k.abs(), m.width, m.orig, m.new, torch.float64).max())
        _refs[key] = (y, r64, e32, mag)
    return _refs[key]


@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_against_fp64(setup, kind):
    name, of, m = setup
    for L in lengths_of(m.orig):
        y, r64, e32, mag = reference(name, m, of, kind, L)
        got = m(y.cuda())
        assert tuple(got.shape) == (-(-m.new * L // m.orig),) and got.dtype == torch.float32
        err = float((got.cpu().double() - r64).abs().max())
        bound = max(4 * e32, 8 * 2.0 ** -24 * mag)
        print(f"\nresample[{name}] {kind} L={L}: |hip - fp64| {err:.3e}, E32 {e32:.3e}, ratio {err / max(e32, 1e-30):.2f}, bound {bound:.3e}")
        assert math.isfinite(err) and err <= bound


def test_batch_items_equal_the_items_alone(setup):
    """Three lengths in one buffer, the tail of each row NaN: an item's outputs bit-identical to the item run alone (at its own Tmax), the
    rest of its row exactly 0, everything finite."""
    name, of, m = setup
    ls = lengths_of(m.orig)
    lens = [ls[1], ls[3], ls[4]]
    Tmax = max(lens)
    wav = torch.full((3, Tmax), float("nan"))
    for b, n in enumerate(lens):
        wav[b, :n] = waveform(KINDS[b], n, of, 7 + b)
    wav = wav.cuda()
    got = m(wav, lengths=lens)
    assert tuple(got.shape) == (3, m.out_length(Tmax)) and torch.isfinite(got).all()
    for b, n in enumerate(lens):
        alone = m(wav[b, :n].clone())
        t = -(-m.new * n // m.orig)
        assert tuple(alone.shape) == (t,)
        assert torch.equal(got[b, :t], alone), (b, n)
        assert (got[b, t:] == 0).all()
    # lengths as a tensor, and the same call again: the same bits
    again = m(wav, lengths=torch.tensor(lens))
    assert torch.equal(again, got)


def test_more_items_than_one_launch_takes():
    """The lengths travel as kernel arguments, 64 items per launch: item 64 and on go through a second launch."""
    of, nf, kw = CONFIGS["24k_16k"]
    m = Resample(of, nf, **kw).cuda()
    B, T = 67, 200
    wav = torch.stack([waveform("noise", T, of, 40 + b) for b in range(B)])
    lens = [T - (b % 5) * 17 for b in range(B)]
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    wav = wav.cuda()
    got = m(wav, lengths=lens)
    assert torch.isfinite(got).all()
    for b in (0, 63, 64, 66):
        t = m.out_length(lens[b])
        assert torch.equal(got[b, :t], m(wav[b, :lens[b]].clone())) and (got[b, t:] == 0).all()


def test_reach_of_one_sample(setup):
    """One NaN at sample m: output q new' + c is NaN exactly when q orig' - width <= m < q orig' - width + K, and every other output has the
    bits of the clean input's.  This sees a Kdim of taps * orig', a dropped last tap or a shifted frame; the edge taps are about 1e-33, so
    no finite bound can."""
    name, of, m = setup
    L = lengths_of(m.orig)[3]
    y = waveform("noise", L, of, 3)
    clean = m(y.cuda())
    q = torch.arange(clean.shape[-1], device="cuda") // m.new
    for s in sorted({min(max(v, 0), L - 1) for v in (0, m.orig - m.width - 1, m.orig - m.width, L - 1)}):
        bad = y.clone()
        bad[s] = float("nan")
        got = m(bad.cuda())
        hit = (q * m.orig - m.width <= s) & (s < q * m.orig + m.orig + m.width)
        assert torch.equal(torch.isnan(got), hit), (name, s)
        assert torch.equal(got[~hit], clean[~hit]), (name, s)


def test_nothing_is_written_past_the_end(setup):
    """Through the C ABI with `out` 256 floats longer than B * out_length and pre-filled: the tail keeps the sentinel."""
    name, of, m = setup
    lib = _lib.load()
    ls = lengths_of(m.orig)
    for L in (ls[3], 1):
        B = 2
        wav = torch.stack([waveform("noise", L, of, 1), waveform("walk", L, of, 2)]).cuda()
        m(wav[:1])                                                   # creates the handle and loads the kernel
        n = m.out_length(L)
        assert lib.us_resample_out_length(m._h, L) == n
        out = torch.full((B * n + 256,), -123.5, device="cuda")
        ws = torch.empty(lib.us_resample_workspace_bytes(m._h, B, L), dtype=torch.uint8, device="cuda")
        lens = (C.c_int64 * B)(L, max(L - 1, 1))
        rc = lib.us_resample_forward(m._h, wav.data_ptr(), lens, B, L, out.data_ptr(), ws.data_ptr(), ws.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0, lib.us_resample_last_error(m._h)
        assert (out[B * n:] == -123.5).all() and torch.isfinite(out).all() and (out[:B * n] != -123.5).all()
        assert torch.equal(out[:n], m(wav[0]))


def test_interface(setup):
    name, of, m = setup
    _, nf, kw = CONFIGS[name]
    T = 5 * m.orig + 3
    y = torch.stack([waveform(KINDS[i % 4], T, of, 20 + i) for i in range(6)]).reshape(2, 3, T).cuda()
    got = m(y)
    assert tuple(got.shape) == (2, 3, m.out_length(T))
    for i in range(2):
        for j in range(3):
            assert torch.equal(got[i, j], m(y[i, j]))
    fkw = dict(kw)
    assert torch.equal(resample(y, of, nf, **fkw), got)
    # the kernel is an ordinary buffer: a state_dict round trip restores it, on either side of .cuda()
    twin = Resample(of, nf, **kw)
    twin.kernel.zero_()
    twin.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    twin = twin.cuda()
    assert list(m.state_dict()) == ["kernel"] and torch.equal(twin(y), got)
    twin.kernel.zero_()
    assert (twin(y) == 0).all()
    twin.load_state_dict(m.state_dict())
    assert torch.equal(twin(y), got)


def test_refusals():
    lib = _lib.load()
    m = Resample(22050, 16000).cuda()
    y = torch.zeros(1, 4096, device="cuda")
    assert tuple(m(y).shape) == (1, 2973)
    for lens in ([0], [4097]):
        with pytest.raises(RuntimeError, match=r"EINVAL.*lengths\[0\]"):
            m(y, lengths=lens)
    with pytest.raises(ValueError, match="lengths"):
        m(y, lengths=[4096, 4096])
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match="EINVAL.*gcd"):                       # the C ABI takes the reduced rates only
        bad = Resample(22050, 16000)
        bad.orig, bad.new = 882, 640
        bad(y)
    out = torch.empty(1, 2973, device="cuda")
    n = lib.us_resample_workspace_bytes(m._h, 1, 4096)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")

    def forward(h, Tmax, ws_bytes):
        return lib.us_resample_forward(h, y.data_ptr(), None, 1, Tmax, out.data_ptr(), ws.data_ptr(), ws_bytes, None)
    for Tmax in (0, -5, 2 ** 30 + 1):
        assert forward(m._h, Tmax, n) == -1 and b"Tmax" in lib.us_resample_last_error(m._h)
    assert forward(m._h, 4096, n - 1) == -5 and b"workspace too small" in lib.us_resample_last_error(m._h)
    assert forward(m._h, 4096, n) == 0
    h = C.c_void_p()                                                             # a handle whose kernel was never loaded
    c = _lib.us_resample_config(orig_freq=441, new_freq=320, width=9)
    assert lib.us_resample_create(C.byref(h), C.byref(c)) == 0
    assert forward(h, 4096, n) == -4 and b"'kernel' has not been loaded" in lib.us_resample_last_error(h)
    shape = (C.c_int64 * 3)(320, 1, 458)
    assert lib.us_resample_load_weight(h, b"kernel", m.kernel.data_ptr(), shape, 3, None) == -3           # US_ESHAPE
    assert lib.us_resample_load_weight(h, b"window", m.kernel.data_ptr(), shape, 3, None) == -2           # US_ENOKEY
    assert lib.us_resample_destroy(h) == 0
    if torch.cuda.device_count() > 1:                                            # the handle lives on cuda:0; a call with cuda:1 current is refused
        with torch.cuda.device(1):
            rc = forward(m._h, 4096, n)
        assert rc == -1 and b"current device" in lib.us_resample_last_error(m._h)
    torch.cuda.synchronize()


def test_features_file_at_another_rate_is_resampled_first(tmp_path):
    import finetune
    from unitspeech_amd import DecoderConfig
    from unitspeech_amd.mel import MelSpectrogram, synthetic_waveform
    cfg, device = DecoderConfig(), torch.device("cuda", 0)
    wav = torch.from_numpy(synthetic_waveform(16000, 3, 16000))
    mel_min, mel_max = torch.tensor(-11.3), torch.tensor(1.9)
    feats = {"wav": wav, "wav_sampling_rate": 16000, "cond_x": torch.zeros(1, 80, 30), "duration": torch.full((1, 30), 2.0),
             "spk_emb": torch.ones(1, 256), "mel_min": mel_min, "mel_max": mel_max}
    path = str(tmp_path / "rate.pt")
    torch.save(feats, path)
    args = argparse.Namespace(features=path, kmeans_checkpoint=None, speaker_encoder_checkpoint=None, unit_encoder_checkpoint=None, hip_resample=True)
    at_22k = Resample(16000, 22050).to(device)(wav.to(device))
    assert tuple(at_22k.shape) == (22050,)
    want = MelSpectrogram(1024, 80, 22050, 256, 1024, 0, 8000).to(device)(at_22k, mel_min=mel_min, mel_max=mel_max)
    mel, cond_x, duration, spk, mn, mx = finetune.load_features(args, cfg, None, device)
    assert mel.device.type == "cuda" and tuple(mel.shape) == (1, 80, 86) and torch.equal(mel, want)
    # without the flag (a Namespace that does not know it) the refusal stands and names it
    del args.hip_resample
    with pytest.raises(SystemExit, match="16000 Hz") as e:
        finetune.load_features(args, cfg, None, device)
    assert "--hip_resample" in str(e.value)
