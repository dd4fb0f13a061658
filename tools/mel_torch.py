"""The reference's `mel_spectrogram` (unitspeech/vocoder/meldataset.py:63-72, center=False) restated with plain torch ops and a `dtype`
argument: the yardstick of the HIP mel front end.  The reference module itself imports librosa for the filter bank; its arithmetic is
`torch.stft` plus one matrix product, which is all that is here.

  dtype=torch.float64   the yardstick: the same fp32 filter bank and window, upcast, so only the arithmetic differs
  dtype=torch.float32   the reference's own fp32 path (on the CPU, or on a GPU for bench_mel.py)
"""
import torch


def mel_spectrogram_torch(y, mel_basis, window, n_fft, hop_size, win_size, dtype=torch.float64, center=False):
    """y [B, T]; mel_basis [num_mels, n_fft // 2 + 1] and window [win_size] as the reference builds them (fp32) -> log-mel [B, num_mels,
    T // hop_size] in `dtype`."""
    y = y.to(dtype)
    pad = int((n_fft - hop_size) / 2)
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)                         # :63-64
    spec = torch.stft(y, n_fft, hop_length=hop_size, win_length=win_size, window=window.to(device=y.device, dtype=dtype), center=center,
                      pad_mode='reflect', normalized=False, onesided=True, return_complex=True)                # :66-67
    spec = torch.sqrt(torch.real(spec * spec.conj() + 1e-9))                                                   # :69
    spec = torch.matmul(mel_basis.to(device=y.device, dtype=dtype), spec)                                      # :71
    return torch.log(torch.clamp(spec, min=1e-5))                                                              # :72 -> :30, C = 1


def normalize(mel, mel_min, mel_max):
    return (mel - mel_min) / (mel_max - mel_min) * 2 - 1                                                       # finetune.py:104
