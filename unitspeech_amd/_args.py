"""Batch arguments on their way into the HIP library: per-item lengths as host integers (`host_lengths`, `c_lengths`) or as a device
int64 tensor (`device_lengths`), the small conversions every wrapper around a plain library function needs (`f32`, `i64`), and the call
of such a function itself (`call`)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


def stream():
    """The current stream of the current device as a `hipStream_t` argument (a pointer whether or not the function declares its types)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(dev, name, *args):
    """The plain (handle-free) library function `name` with `dev` current: a tensor goes in as its `data_ptr()`, None as a null
    pointer, everything else as it is, and the current stream of `dev` is appended.  A refusal is raised under the symbol's name."""
    tensor = torch.Tensor
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(*[a.data_ptr() if isinstance(a, tensor) else a for a in args], stream())
    if rc != _lib.US_OK:
        _lib.check(rc, what=name)


def f32(t, dev, detach=True):
    """-> `t` as a contiguous fp32 tensor on `dev` (None stays None); `detach=False` keeps it in the autograd graph."""
    if t is None:
        return None
    return (t.detach() if detach else t).to(device=dev, dtype=torch.float32).contiguous()


def i64(t, dev):
    return torch.as_tensor(t).detach().to(device=dev, dtype=torch.int64).contiguous()


def need_gpu(t, what, noun):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the tensor is on {t.device}; {noun} runs on the GPU only (there is no CPU fallback)")


def host_lengths(lengths, B, what, integers_only=False):
    """-> the B per-item lengths as Python ints, or None for None (the library checks their range and names the item).  `lengths` is a
    list, a numpy array or a tensor of any shape with B elements; a device tensor is read back here: one synchronisation.  Values go
    through `int()` unless `integers_only`, which refuses a dtype or an element that is not an integer."""
    if lengths is None:
        return None
    if isinstance(lengths, (torch.Tensor, np.ndarray)):
        if integers_only:
            if isinstance(lengths, torch.Tensor):
                integer = not (lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool)
            else:
                integer = lengths.dtype.kind in "iu"
            if not integer:
                raise ValueError(f"{what}: lengths must be integers, got dtype {lengths.dtype}")
        lengths = lengths.reshape(-1).tolist()
    if integers_only:
        for i, n in enumerate(lengths):
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
                raise ValueError(f"{what}: lengths must be integers, item {i} has {n!r}")
    v = [int(n) for n in lengths]
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} lengths for {B} items" + (f" (item {len(v)} has none)" if len(v) < B else ""))
    return v


def c_lengths(v):
    """Host lengths as the library's `const int64_t*` (None stays None: no lengths)."""
    return None if v is None else (C.c_int64 * len(v))(*v)


def device_lengths(lengths, B, dev, what):
    """-> lengths as a contiguous int64 [B] on `dev`, or None for None."""
    if lengths is None:
        return None
    lens = i64(lengths, dev)
    if lens.shape != (B,):
        raise ValueError(f"{what}: lengths {tuple(lens.shape)} must hold {B} values")
    return lens
