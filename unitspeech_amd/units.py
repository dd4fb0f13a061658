"""From the dense upstream features to the unit sequence, on the device (csrc/units.hip).

Drop-ins with the reference's names and signatures for the three host steps of finetune.py:112-128:

  KMeansQuantizer   textless/data/kmeans_quantizer.py: scikit-learn `KMeans.predict`  -> `us_units_quantize`
  SpeechEncoder     textless/data/speech_encoder.py: dense model + quantizer + `unique_consecutive`  -> `us_units_dedup`
  process_unit      unitspeech/util.py:69-102: 50 Hz units to mel-rate (unit, duration)  -> `us_units_process`

The dense model (mHuBERT through fairseq) stays the caller's torch module.  All results are integers and exact: the units are the fp64
argmin of the squared distance over the fp32 inputs (first index on ties), whatever the fp32 GEMM rounds.  There is no CPU fallback:
a tensor that is not on a GPU raises.
"""
from __future__ import annotations

import warnings
from typing import Optional

import torch

from . import _lib

__all__ = ["KMeansQuantizer", "SpeechEncoder", "process_unit", "process_units_batch", "dedup_units"]

MAX_K, MAX_D, MAX_SPAN = 2048, 1024, 64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the tensor is on {t.device}; the unit extraction runs on the GPU only (there is no CPU fallback)")


def _i64(t, dev):
    return torch.as_tensor(t).detach().to(device=dev, dtype=torch.int64).contiguous()


def _workspace(lib, dev, B, Tmax, K, D, Lout):
    n = int(lib.us_units_workspace_bytes(B, Tmax, K, D, Lout))
    if n == 0:
        raise ValueError(f"unit extraction: unsupported sizes B = {B}, T = {Tmax}, K = {K}, D = {D}, output frames = {Lout}")
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def _check_rates(sampling_rate, hop_length):
    sampling_rate, hop_length = int(sampling_rate), int(hop_length)
    if sampling_rate < 50 or hop_length < 1:
        raise ValueError(f"process_unit: sampling_rate {sampling_rate} must be at least 50 and hop_length {hop_length} at least 1")
    spf = sampling_rate // 50
    if (hop_length + spf - 2) // spf + 1 > MAX_SPAN:
        raise ValueError(f"process_unit: with sampling_rate {sampling_rate} and hop_length {hop_length} an output frame spans more than "
                         f"{MAX_SPAN} frames of the 50 Hz stream")
    return sampling_rate, hop_length, spf


def synthetic_centers(K: int, D: int, seed: int):
    """Seeded stand-in for a k-means codebook: [K, D] fp32 numpy, unit-variance entries."""
    import numpy as np
    g = np.random.Generator(np.random.Philox(key=[seed, 0x6b6d]))
    return g.standard_normal((K, D), dtype=np.float32)


def synthetic_dense(centers, T: int, seed: int, noise: float = 0.5, mean_run: float = 3.0):
    """Seeded stand-in for upstream features: a sticky unit stream (geometric run lengths of mean `mean_run`) whose frames are their
    centre plus Gaussian noise, so the rows look like real features and not like an isotropic cloud.  -> [T, D] fp32 numpy."""
    import numpy as np
    g = np.random.Generator(np.random.Philox(key=[seed, 0x6465]))
    K, D = centers.shape
    runs = g.geometric(1.0 / mean_run, size=T)
    ids = np.repeat(g.integers(0, K, size=T), runs)[:T]
    return (centers[ids] + noise * g.standard_normal((T, D), dtype=np.float32)).astype(np.float32)


class KMeansQuantizer(torch.nn.Module):
    """`KMeansQuantizer(checkpoint_path)` reads the joblib file of a scikit-learn KMeans and keeps its `cluster_centers_`;
    `from_centers(tensor [K, D])` takes them directly.  K <= 2048, D a multiple of 4 up to 1024."""

    def __init__(self, checkpoint_path=None, *, centers=None):
        super().__init__()
        if centers is None:
            if checkpoint_path is None:
                raise ValueError("KMeansQuantizer: give checkpoint_path or use KMeansQuantizer.from_centers(tensor)")
            centers = torch.from_numpy(self.load_kmeans_model(checkpoint_path).cluster_centers_)
        centers = torch.as_tensor(centers).detach().to(torch.float32).contiguous()
        if centers.dim() != 2:
            raise ValueError(f"KMeansQuantizer: centres must be [K, D], got {tuple(centers.shape)}")
        K, D = centers.shape
        if not 1 <= K <= MAX_K:
            raise ValueError(f"KMeansQuantizer: K = {K} centres; the library takes 1 to {MAX_K}")
        if D % 4 or not 4 <= D <= MAX_D:
            raise ValueError(f"KMeansQuantizer: D = {D}; the library takes a multiple of 4 up to {MAX_D}")
        if not bool(torch.isfinite(centers).all()):
            raise ValueError("KMeansQuantizer: the centres must be finite")
        self.register_buffer("centers", centers)
        self.register_buffer("_float_tensor", torch.tensor([0], dtype=torch.float))
        self._packed = None
        self.last_counters = None          # device int32 [2] of the last call: rows with a non-finite feature, rows decided in fp64

    @classmethod
    def from_centers(cls, centers) -> "KMeansQuantizer":
        return cls(centers=centers)

    @staticmethod
    def load_kmeans_model(checkpoint_path: str):
        import joblib
        with open(checkpoint_path, "rb") as fd, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return joblib.load(fd)

    @property
    def vocab_size(self) -> int:
        return int(self.centers.shape[0])

    @property
    def device(self):
        return self._float_tensor.device

    def _apply(self, fn, *a, **kw):
        self._packed = None
        return super()._apply(fn, *a, **kw)

    def packed(self, dev):
        """The centres in the library's operand form on `dev` (packed once per device placement)."""
        if self._packed is None or self._packed.device != dev:
            lib = _lib.load()
            K, D = self.centers.shape
            c = self.centers.to(dev)
            n = int(lib.us_units_packed_bytes(K, D))
            buf = torch.empty(n, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                rc = lib.us_units_pack_centers(c.data_ptr(), K, D, buf.data_ptr(), n, _stream())
            _lib.check(rc, None, "us_units_pack_centers")
            self._packed = buf
        return self._packed

    def _dense(self, dense, lengths):
        _need_gpu(dense, "KMeansQuantizer")
        K, D = self.centers.shape
        if dense.dim() != 3 or dense.shape[-1] != D:
            raise ValueError(f"KMeansQuantizer: features must be [B, T, {D}], got {tuple(dense.shape)}")
        dev = dense.device
        x = dense.detach().to(torch.float32).contiguous()
        B, T = x.shape[:2]
        lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else _i64(lengths, dev)
        if lens.shape != (B,):
            raise ValueError(f"KMeansQuantizer: lengths {tuple(lens.shape)} must hold {B} values")
        return x, lens, B, T, K, D, dev

    @torch.no_grad()
    def quantize(self, dense, lengths=None):
        """dense [B, Tmax, D], lengths [B] -> units [B, Tmax] int64 (-1 at t >= lengths[b] and on rows with a non-finite feature).
        Nothing is read back; `last_counters` holds the two device counters."""
        x, lens, B, T, K, D, dev = self._dense(dense, lengths)
        units = torch.empty(B, T, dtype=torch.int64, device=dev)
        if B * T == 0:
            return units
        lib = _lib.load()
        ws, n = _workspace(lib, dev, B, T, K, D, 0)
        self.last_counters = torch.empty(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.us_units_quantize(x.data_ptr(), lens.data_ptr(), self.packed(dev).data_ptr(), B, T, K, D, units.data_ptr(),
                                       self.last_counters.data_ptr(), ws.data_ptr(), n, _stream())
        _lib.check(rc, None, "us_units_quantize")
        return units

    def forward(self, x):
        """x [T, D] -> units [T] int64 on x's device (`KMeans.predict`)."""
        if x.dim() != 2:
            raise ValueError(f"KMeansQuantizer: features must be [T, D], got {tuple(x.shape)}")
        return self.quantize(x.unsqueeze(0))[0]

    @torch.no_grad()
    def encode(self, dense, lengths=None, sampling_rate: int = 16000, hop_length: int = 256):
        """dense [B, Tmax, D], lengths [B] -> (unit [B, Lu] int64, duration [B, Lu] fp32, unit_lengths [B] int64) at the mel rate:
        quantize and `process_unit` in one library call, with no host synchronisation.  Lu is the largest possible frame count;
        entries beyond unit_lengths[b] are 0."""
        sampling_rate, hop_length, spf = _check_rates(sampling_rate, hop_length)
        x, lens, B, T, K, D, dev = self._dense(dense, lengths)
        Lout = max(1, T * spf // hop_length)
        lib = _lib.load()
        ws, n = _workspace(lib, dev, B, T, K, D, Lout)
        unit = torch.empty(B, Lout, dtype=torch.int64, device=dev)
        dur = torch.empty(B, Lout, dtype=torch.int64, device=dev)
        dur_f = torch.empty(B, Lout, dtype=torch.float32, device=dev)
        n_out = torch.empty(B, dtype=torch.int64, device=dev)
        self.last_counters = torch.empty(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.us_units_encode(x.data_ptr(), lens.data_ptr(), self.packed(dev).data_ptr(), B, T, K, D, sampling_rate, hop_length,
                                     unit.data_ptr(), dur.data_ptr(), dur_f.data_ptr(), n_out.data_ptr(), Lout,
                                     self.last_counters.data_ptr(), ws.data_ptr(), n, _stream())
        _lib.check(rc, None, "us_units_encode")
        return unit, dur_f, n_out


@torch.no_grad()
def dedup_units(units, lengths=None):
    """units [B, Tmax] int64 with lengths [B] -> (units, durations [B, Tmax] int64, zero padded, n [B] int64): per item
    `torch.unique_consecutive(return_counts=True)`, without a host synchronisation."""
    _need_gpu(units, "dedup_units")
    dev = units.device
    u = _i64(units, dev)
    B, T = u.shape
    lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else _i64(lengths, dev)
    out_u = torch.zeros(B, T, dtype=torch.int64, device=dev)
    out_d = torch.zeros(B, T, dtype=torch.int64, device=dev)
    n_out = torch.zeros(B, dtype=torch.int64, device=dev)
    if B * T == 0:
        return out_u, out_d, n_out
    lib = _lib.load()
    ws, n = _workspace(lib, dev, B, T, 0, 0, 0)
    with torch.cuda.device(dev):
        rc = lib.us_units_dedup(u.data_ptr(), lens.data_ptr(), B, T, out_u.data_ptr(), out_d.data_ptr(), n_out.data_ptr(), ws.data_ptr(), n,
                                _stream())
    _lib.check(rc, None, "us_units_dedup")
    return out_u, out_d, n_out


@torch.no_grad()
def process_units_batch(units, durations, n_in, sampling_rate, hop_length, max_frames: Optional[int] = None):
    """`process_unit` for a padded batch, without a host synchronisation.  units [B, Lin] int64, durations [B, Lin] (None: all ones),
    n_in [B] valid entries per item (None: Lin).  max_frames bounds sum(durations) of every item; it sizes the outputs and is
    needed when durations are given (Lin otherwise).  Returns (unit [B, Lu] int64, duration [B, Lu] int64, duration as fp32,
    unit_lengths [B] int64); entries beyond unit_lengths[b] are 0, and unit_lengths[b] is -1 for an item with more than max_frames."""
    sampling_rate, hop_length, spf = _check_rates(sampling_rate, hop_length)
    _need_gpu(units, "process_units_batch")
    dev = units.device
    u = _i64(units, dev)
    B, Lin = u.shape
    if durations is not None and max_frames is None:
        raise ValueError("process_units_batch: max_frames (a bound on the sum of an item's durations) is needed with durations")
    fmax = Lin if max_frames is None else int(max_frames)
    d = None if durations is None else _i64(durations, dev)
    if d is not None and d.shape != u.shape:
        raise ValueError(f"process_units_batch: units {tuple(u.shape)} and durations {tuple(d.shape)} disagree")
    lens = torch.full((B,), Lin, dtype=torch.int64, device=dev) if n_in is None else _i64(n_in, dev)
    Lout = max(1, fmax * spf // hop_length)
    unit = torch.zeros(B, Lout, dtype=torch.int64, device=dev)
    dur = torch.zeros(B, Lout, dtype=torch.int64, device=dev)
    dur_f = torch.zeros(B, Lout, dtype=torch.float32, device=dev)
    n_out = torch.zeros(B, dtype=torch.int64, device=dev)
    if B * Lin == 0:
        return unit, dur, dur_f, n_out
    lib = _lib.load()
    ws, n = _workspace(lib, dev, B, Lin, 0, 0, Lout)
    with torch.cuda.device(dev):
        rc = lib.us_units_process(u.data_ptr(), d.data_ptr() if d is not None else None, lens.data_ptr(), B, Lin, sampling_rate, hop_length,
                                  unit.data_ptr(), dur.data_ptr(), dur_f.data_ptr(), n_out.data_ptr(), Lout, ws.data_ptr(), n, _stream())
    _lib.check(rc, None, "us_units_process")
    return unit, dur, dur_f, n_out


@torch.no_grad()
def process_unit(encoded, sampling_rate, hop_length):
    """Drop-in for `unitspeech.util.process_unit`: encoded {"units", "durations"} (1-D, on the GPU) -> (unit, duration) LongTensors of
    exact length on the same device.  One count is read back, the only synchronisation when `encoded` carries the SpeechEncoder's
    "dense" [T, D] (its T bounds the output); without it the sum of the durations is read first.  An input shorter than one hop gives
    two empty tensors (the reference raises an IndexError there)."""
    units, durations = encoded["units"], encoded["durations"]
    _need_gpu(units, "process_unit")
    if units.dim() != 1 or durations.shape != units.shape:
        raise ValueError(f"process_unit: units {tuple(units.shape)} and durations {tuple(durations.shape)} must be 1-D and agree")
    dense = encoded.get("dense") if hasattr(encoded, "get") else None
    fmax = int(dense.shape[0]) if isinstance(dense, torch.Tensor) and dense.dim() == 2 else int(durations.sum())
    unit, dur, _, n_out = process_units_batch(units.unsqueeze(0), durations.unsqueeze(0), None, sampling_rate, hop_length, max_frames=max(fmax, 1))
    n = int(n_out[0])
    if n < 0:
        raise RuntimeError(f"process_unit: the durations cover more than the {fmax} frames of `dense`")
    return unit[0, :n], dur[0, :n]


class SpeechEncoder(torch.nn.Module):
    """Drop-in for textless' SpeechEncoder with the quantisation and the run-length encoding on the device.  `dense_model` is the
    caller's torch module (waveform -> [T, D]); `quantizer_model` a `KMeansQuantizer` of this module."""

    def __init__(self, dense_model, quantizer_model, deduplicate: bool, add_bos_eos: bool = False, need_f0: bool = False,
                 f0_normalizer=None, f0_quantizer=None):
        super().__init__()
        if need_f0 or f0_normalizer is not None or f0_quantizer is not None:
            raise NotImplementedError("SpeechEncoder: the F0 stream is not part of this library (UnitSpeech does not use it): pass "
                                      "need_f0=False and no f0_normalizer / f0_quantizer")
        if not isinstance(quantizer_model, KMeansQuantizer):
            raise TypeError("SpeechEncoder: quantizer_model must be a unitspeech_amd.units.KMeansQuantizer")
        self.dense_model = dense_model
        self.quantizer_model = quantizer_model
        self.deduplicate = deduplicate
        self.add_bos_eos = add_bos_eos
        self.need_f0 = False
        self.unit_vocab_size = self.quantizer_model.vocab_size
        self.register_buffer("bos", torch.tensor([self.unit_vocab_size], dtype=torch.int))
        self.register_buffer("eos", torch.tensor([self.unit_vocab_size + 1], dtype=torch.int))
        self.register_buffer("_float_tensor", torch.tensor([0], dtype=torch.float))

    @classmethod
    def by_name(cls, *args, **kwargs):
        raise NotImplementedError("SpeechEncoder.by_name downloads pre-trained models by name, which this library does not do: build the "
                                  "dense model yourself and pass SpeechEncoder(dense_model, KMeansQuantizer(checkpoint_path), deduplicate, "
                                  "need_f0=False)")

    @property
    def device(self):
        return self._float_tensor.device

    @property
    def vocab_size(self) -> int:
        return self.quantizer_model.vocab_size

    @property
    def code_hop_size(self) -> int:
        return self.dense_model.code_hop_size

    @property
    def expected_sample_rate(self) -> int:
        return self.dense_model.expected_sample_rate

    @torch.no_grad()
    def encode_dense(self, dense, lengths=None):
        """dense [B, Tmax, D], lengths [B] -> {"units", "durations" [B, Tmax] int64, "lengths" [B] int64, "dense"}: the quantised
        (and, with deduplicate, run-length encoded, zero padded) streams of a batch, without a host synchronisation."""
        units = self.quantizer_model.quantize(dense, lengths)
        B, T = units.shape
        lens = torch.full((B,), T, dtype=torch.int64, device=units.device) if lengths is None else _i64(lengths, units.device)
        if self.deduplicate:
            units, durations, n = dedup_units(units, lens)
        else:
            valid = torch.arange(T, device=units.device).unsqueeze(0) < lens.unsqueeze(1)
            units, durations, n = torch.where(valid, units, torch.zeros_like(units)), valid.to(torch.int64), lens.clamp(0, T)
        return {"units": units, "durations": durations, "lengths": n, "dense": dense}

    @torch.no_grad()
    def forward(self, waveform, speaker=None):
        if waveform.ndim > 1:
            waveform = waveform.mean(0)
        dense = self.dense_model(waveform)
        units = self.quantizer_model(dense)
        if self.deduplicate:
            u, d, n = dedup_units(units.unsqueeze(0))
            n = int(n[0])                                   # the one read-back: the reference's outputs have the exact length
            units, durations = u[0, :n], d[0, :n]
        else:
            durations = torch.ones_like(units)
        if self.add_bos_eos:
            units = torch.cat([self.bos.to(units.device), units, self.eos.to(units.device)])
            z = torch.zeros_like(durations[0:1])
            durations = torch.cat([z, durations, z])
            z = torch.zeros_like(dense[0:1, :])
            dense = torch.cat([z, dense, z])
        return {"units": units.to(self.device), "durations": durations.to(self.device), "dense": dense}
