"""`HandleModule`: a torch module whose arithmetic lives behind one opaque handle of the HIP library that takes its weights by
state_dict key (csrc/handle.h: us_frontend, us_vocoder, us_speaker, us_mel, us_resample, us_hubert, us_wavlm, us_whisper).  It owns the handle, pushes the weights whose storage or version
changed since the last call, keeps the caller-owned workspace, and makes the library calls of a forward (`_call`: the handle's device
current, the return code checked under the symbol's name).  Per-item lengths reach those calls through `_args`."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch

from . import _lib


class HandleModule(torch.nn.Module):
    _abi = ""                  # "frontend" / "vocoder" / "speaker" / "mel" / "resample" / "hubert" / "wavlm" / "whisper": us_{_abi}_load_weight, _last_error, _destroy, _workspace_bytes
    _what = ""                 # how the module calls itself when it refuses a device
    _cache_sources = False     # True: _sources() is walked once, and again after .to() / .float() (for a module whose parameters
                               # are never registered anew; state_dict() of a few hundred entries is not free next to a short forward)

    def __init__(self):
        super().__init__()
        self._h = C.c_void_p()
        self._device = None
        self._tags = {}
        self._src = None
        self._ws = None

    def _create(self, lib, device):
        """Create the handle into self._h (called with `device` current)."""
        raise NotImplementedError

    def _sources(self):
        """C-ABI key -> (tensors its value is made from, function making it, or None when the value is the one tensor itself).
        Default: every floating-point entry of the state_dict."""
        return OrderedDict((k, ((t,), None)) for k, t in self.state_dict(keep_vars=True).items() if t.is_floating_point())

    def _precondition(self):
        """Raise when the module must not run as it stands (checked before the library is touched)."""

    def _fn(self, lib, name):
        return getattr(lib, f"us_{self._abi}_{name}")

    def _apply(self, fn, *args, **kwargs):
        self._src = None                   # .to() / .float() replace the buffers: a cached source list is rebuilt
        return super()._apply(fn, *args, **kwargs)

    def _sync(self, device: torch.device, **precondition):
        if device.type != "cuda":
            raise RuntimeError(f"the HIP {self._what} needs tensors on a ROCm device (no CPU fallback); got " + str(device))
        self._precondition(**precondition)
        lib = _lib.load()
        if not self._h or self._device != device:
            self._close()
            with torch.cuda.device(device):
                self._create(lib, device)
            self._device, self._tags = device, {}
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        src = self._src
        if src is None:            # split once: the steady state is the tag comparison, and a module of ~200 keys is host-bound
            items = self._sources().items()
            src = ([(k, parts[0]) for k, (parts, make) in items if make is None],
                   [(k, parts, make) for k, (parts, make) in items if make is not None])
            if self._cache_sources:
                self._src = src
        tags = self._tags

        def push(key, t, tag, own):
            # the library copies on the stream: a buffer that is not the storage of a tensor the module keeps must outlive the copy
            kept = own and t.dtype == torch.float32 and t.device == device and t.is_contiguous()
            buf = t.detach() if kept else t.detach().to(device=device, dtype=torch.float32).contiguous()
            shape = (C.c_int64 * buf.dim())(*buf.shape)
            rc = self._fn(lib, "load_weight")(self._h, key.encode(), buf.data_ptr(), shape, buf.dim(), stream)
            self._check(lib, rc, f"us_{self._abi}_load_weight({key})")
            if not kept:
                torch.cuda.current_stream(device).synchronize()
            tags[key] = tag

        # the handle allocates its weight store on the CURRENT device and refuses calls made under another one (handle.h: on_device)
        with torch.no_grad(), torch.cuda.device(device):
            for key, t in src[0]:
                tag = (t.data_ptr(), t._version, t.device)
                if tags.get(key) != tag:
                    push(key, t, tag, True)
            for key, parts, make in src[1]:
                tag = tuple((p.data_ptr(), p._version, p.device) for p in parts)
                if tags.get(key) != tag:
                    push(key, make(), tag, False)
        return lib, stream

    def _workspace(self, lib, device, *dims):
        """Caller-owned activation scratch of one forward call, grown and never shrunk (torch's caching allocator: no hipMalloc /
        hipFree in the call)."""
        n = int(self._fn(lib, "workspace_bytes")(self._h, *dims))
        ws = self._ws
        if ws is None or ws.numel() < n or ws.device != device:
            self._ws = None
            self._ws = ws = torch.empty(n, dtype=torch.uint8, device=device)
        return ws

    def _call(self, lib, device, name, *args):
        """us_{_abi}_{name}(*args) with `device` current; a refusal is raised under the symbol's full name."""
        with torch.cuda.device(device):
            rc = self._fn(lib, name)(*args)
        self._check(lib, rc, f"us_{self._abi}_{name}")

    def _check(self, lib, rc, what):
        if rc != _lib.US_OK:
            msg = self._fn(lib, "last_error")(self._h)
            raise RuntimeError(f"libunitspeech_hip: {what} failed with {_lib.ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")

    def _close(self):
        if getattr(self, "_h", None):
            self._fn(_lib.load(), "destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass
