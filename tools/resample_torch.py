"""torchaudio's `_apply_sinc_resample_kernel` restated with plain torch ops and a `dtype` argument: the yardstick of the HIP resampler and
the eager leg of bench_resample.py.  Written from the formula

  out[q * new + c] = sum_{k < orig + 2 width} kernel[c][0][k] * y[q * orig + k - width],   y = 0 outside [0, T),

for q * new + c < ceil(new * T / orig), with orig and new the two rates divided by their gcd.

  dtype=torch.float64   the yardstick: the same fp32 kernel, upcast, so only the arithmetic differs
  dtype=torch.float32   torchaudio's own fp32 path (on the CPU, or on a GPU for bench_resample.py)

The length is the exact integer ceil(new * T / orig); torchaudio evaluates the same expression through a tensor of the default dtype.
"""
import torch


def resample_torch(y, kernel, width, orig, new, dtype=torch.float64):
    """y [..., T]; kernel [new, 1, orig + 2 * width] as `unitspeech_amd.resample.sinc_resample_kernel` returns it (fp32) ->
    [..., ceil(new * T / orig)] in `dtype`."""
    shape = y.shape
    y = y.to(dtype).reshape(-1, shape[-1])
    T = int(shape[-1])
    y = torch.nn.functional.pad(y, (width, width + orig))                            # one spare frame: T // orig + 1 frames in all
    out = torch.nn.functional.conv1d(y[:, None], kernel.to(device=y.device, dtype=dtype), stride=orig)      # [N, new, frames]
    out = out.transpose(1, 2).reshape(y.shape[0], -1)                                # sample q * new + c
    target = (new * T + orig - 1) // orig
    return out[..., :target].reshape(shape[:-1] + (target,))
