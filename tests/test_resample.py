"""The host side of the resampler (no GPU): torchaudio's sinc kernel as `unitspeech_amd.resample.sinc_resample_kernel` builds it, and the
restatement of torchaudio's strided convolution (tools/resample_torch.py) that the GPU tests use as their yardstick, against an independent
direct evaluation of the interpolation sum, against analytic sines, and for its length and its reach."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from resample_torch import resample_torch  # noqa: E402

from unitspeech_amd.resample import Resample, resample, sinc_resample_kernel  # noqa: E402

# name: (orig_freq, new_freq, keyword arguments, orig', new', width, K)
CONFIGS = {
    "22k_16k": (22050, 16000, {}, 441, 320, 9, 459),
    "16k_22k": (16000, 22050, {}, 320, 441, 7, 334),
    "24k_16k": (24000, 16000, {}, 3, 2, 10, 23),
    "48k_16k": (48000, 16000, {}, 3, 1, 19, 41),
    "kaiser": (22050, 16000, dict(resampling_method="sinc_interp_kaiser", lowpass_filter_width=64, rolloff=0.9475937167399596), 441, 320, 94, 629),
}


def make(name):
    of, nf, kw, orig, new, width, K = CONFIGS[name]
    kernel, w = sinc_resample_kernel(of, nf, math.gcd(of, nf), **kw)
    return kernel, w, orig, new


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_shape_width_and_dc_gain(name):
    of, nf, kw, orig, new, width, K = CONFIGS[name]
    kernel, w = sinc_resample_kernel(of, nf, math.gcd(of, nf), **kw)
    assert w == width and tuple(kernel.shape) == (new, 1, K) and kernel.dtype == torch.float32
    assert K == orig + 2 * width
    if nf < of:                                  # every phase passes DC with unit gain
        gain = kernel.double().sum(dim=2).reshape(-1)
        assert float((gain - 1).abs().max()) <= 2e-3, float((gain - 1).abs().max())
    m = Resample(of, nf, **kw)
    assert torch.equal(m.kernel, kernel) and m.width == width and (m.orig, m.new) == (orig, new)


def test_unknown_method_is_refused():
    for method in ("sinc_interp_blackman", "linear"):
        with pytest.raises(ValueError, match="Invalid resampling method"):
            sinc_resample_kernel(22050, 16000, 50, resampling_method=method)
    with pytest.raises(ValueError, match="Invalid resampling method"):
        Resample(22050, 16000, resampling_method="nearest")
    with pytest.raises(ValueError):
        sinc_resample_kernel(22050, 16000, 50, lowpass_filter_width=0)


def direct(y, orig, new, width, lpfw=6, rolloff=0.99):
    """out[i] = sum_m y[m] g(base (m / orig - i / new)) over the kernel's support q orig - width <= m < q orig + orig + width (i = q new + c),
    g the Hann-windowed sinc, one output and one sample at a time in numpy fp64."""
    L = len(y)
    base = min(orig, new) * rolloff
    n_out = -(-new * L // orig)
    out = np.zeros(n_out)
    for i in range(n_out):
        q = i // new
        acc = 0.0
        for m in range(max(q * orig - width, 0), min(q * orig + orig + width, L)):
            t = base * (m / orig - i / new)
            t = min(max(t, -lpfw), lpfw)
            s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            acc += y[m] * s * math.cos(t * math.pi / lpfw / 2) ** 2 * (base / orig)
        out[i] = acc
    return out


@pytest.mark.parametrize("name,L", [("22k_16k", 1000), ("24k_16k", 100)])
def test_restatement_against_a_direct_evaluation(name, L):
    """The only difference is the fp32 rounding of the kernel (relative 2^-24 per entry, sum |kernel| |y| of a few units at most)."""
    kernel, width, orig, new = make(name)
    y = 0.3 * np.random.Generator(np.random.Philox(key=5)).standard_normal(L)
    got = resample_torch(torch.from_numpy(y), kernel, width, orig, new, torch.float64).numpy()
    want = direct(y, orig, new, width)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"\nresample[{name}] L={L}: |restatement fp64 - direct| {err:.3e}")
    assert err <= 2e-7


@pytest.mark.parametrize("rates", [(22050, 16000), (16000, 22050), (48000, 16000)])
@pytest.mark.parametrize("freq", [440.0, 3000.0])
def test_restatement_reproduces_a_sine(rates, freq):
    """A reversed kernel, a frame shifted by one sample or a phase taken for its neighbour shows here: 0.3 samples of delay at 3000 Hz and
    16 kHz is an error of 0.9 * 2 pi * 3000 * 0.3 / 16000 = 0.3."""
    of, nf = rates
    g = math.gcd(of, nf)
    kernel, width = sinc_resample_kernel(of, nf, g)
    L = of // 2
    y = 0.9 * torch.sin(2 * math.pi * freq * torch.arange(L, dtype=torch.float64) / of)
    for dtype in (torch.float64, torch.float32):
        got = resample_torch(y, kernel, width, of // g, nf // g, dtype).double()
        want = 0.9 * torch.sin(2 * math.pi * freq * torch.arange(got.shape[-1], dtype=torch.float64) / nf)
        edge = nf // 100
        err = float((got - want)[edge:-edge].abs().max())
        print(f"\nresample {of}->{nf} sine {freq:.0f} Hz {dtype}: |restatement - analytic| {err:.3e}")
        assert err <= 2e-3


@pytest.mark.parametrize("name", list(CONFIGS))
def test_restatement_length(name):
    kernel, width, orig, new = make(name)
    for L in sorted({1, max(orig - 1, 1), orig, orig + 1, 33 * orig + 7}):
        y = torch.ones(2, L)
        for dtype in (torch.float64, torch.float32):
            out = resample_torch(y, kernel, width, orig, new, dtype)
            assert tuple(out.shape) == (2, -(-new * L // orig)) and out.dtype == dtype and torch.isfinite(out).all()
    assert tuple(resample_torch(torch.ones(2, 3, 50), kernel, width, orig, new).shape) == (2, 3, -(-new * 50 // orig))


def nan_reach(m, L, orig, new, width):
    """Outputs that sample m of an L-sample item reaches: q new + c with q orig - width <= m < q orig - width + K."""
    n_out = -(-new * L // orig)
    q = torch.arange(n_out) // new
    return (q * orig - width <= m) & (m < q * orig + orig + width)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_restatement_reach_of_one_sample(name):
    kernel, width, orig, new = make(name)
    L = 5 * orig + 3
    y = 0.3 * torch.from_numpy(np.random.Generator(np.random.Philox(key=9)).standard_normal(L)).float()
    clean = resample_torch(y, kernel, width, orig, new, torch.float32)
    for m in sorted({min(max(v, 0), L - 1) for v in (0, orig - width - 1, orig - width, L - 1)}):
        bad = y.clone()
        bad[m] = float("nan")
        got = resample_torch(bad, kernel, width, orig, new, torch.float32)
        hit = nan_reach(m, L, orig, new, width)
        assert torch.equal(torch.isnan(got), hit), (name, m)
        assert torch.equal(got[~hit], clean[~hit]), (name, m)


def test_create_refusals_and_sizes_through_the_c_abi():
    """us_resample_create touches no device: the configuration checks, the weight key and the sizes can be read on any machine."""
    import ctypes as C
    from unitspeech_amd import _lib
    lib = _lib.load()

    def create(orig, new, width):
        h = C.c_void_p()
        c = _lib.us_resample_config(orig_freq=orig, new_freq=new, width=width)
        return lib.us_resample_create(C.byref(h), C.byref(c)), h
    for bad, word in (((0, 320, 9), b"positive"), ((441, -1, 9), b"positive"), ((22050, 16000, 9), b"4096"), ((4097, 4096, 9), b"4096"),
                      ((882, 640, 9), b"gcd"), ((3, 3, 9), b"gcd"), ((441, 320, -1), b"width")):
        rc, h = create(*bad)
        assert rc == -1 and not h, bad                               # US_EINVAL, no handle
        assert word in lib.us_last_error(None), (bad, lib.us_last_error(None))
    rc, h = create(441, 320, 9)
    assert rc == 0 and h
    assert lib.us_resample_num_weights(h) == 1 and [lib.us_resample_weight_key(h, i) for i in range(2)] == [b"kernel", None]
    for T, want in ((1, 1), (440, 320), (441, 320), (442, 321), (22050, 16000), (2 ** 30, (320 * 2 ** 30 + 440) // 441), (0, 0)):
        assert lib.us_resample_out_length(h, T) == want, T
    # X [B][441][frames + 1]: 16000 outputs are 50 frames of 320, K = 459 is two taps; padded to 64 floats, plus the alignment slack
    assert lib.us_resample_workspace_bytes(h, 2, 22050) == ((2 * 441 * 51 + 63) // 64 * 64) * 4 + 256
    assert lib.us_resample_workspace_bytes(h, 0, 22050) == 0
    assert lib.us_resample_destroy(h) == 0
    rc, h = create(1, 4096, 0)                                       # the largest ratio: 2^42 outputs for 2^30 samples
    assert rc == 0 and lib.us_resample_out_length(h, 2 ** 30) == 2 ** 42 and lib.us_resample_destroy(h) == 0


def test_cpu_waveform_is_refused():
    with pytest.raises(RuntimeError, match="ROCm device"):
        Resample(22050, 16000)(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match="ROCm device"):
        resample(torch.zeros(4096), 22050, 16000)


def test_equal_rates_pass_the_input_through():
    y = torch.randn(2, 100)
    m = Resample(16000, 16000)
    assert m(y) is y and not m._h and "kernel" not in m.state_dict()
    assert Resample()(y) is y
    assert resample(y, 22050, 22050) is y
