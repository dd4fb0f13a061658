"""`Encoder` and `DurationPredictor` of the conditioning producer on the HIP library.

Drop-in for `unitspeech/encoder.py:253-308` (`Encoder`: text encoder and unit encoder are two instances) and
`unitspeech/duration_predictor.py:24-63` (`DurationPredictor`): same constructor arguments, same `state_dict` keys in
the same order (the sub-modules below are parameter containers, exactly as in `unitspeech_amd.unitspeech`), same call
signatures and return values -- `Encoder(x, x_lengths) -> (mu_x, x, x_mask)`, `DurationPredictor(x, x_mask, w=None,
g=spk_emb, reverse=True) -> logw` -- so `UnitSpeech.execute_text_to_speech(phoneme, lengths, spk_emb, text_encoder,
duration_predictor, ...)` takes them where it takes the reference's modules.

In eval mode the reference's Dropouts are the identity.  `Encoder(..., trainable=True)` in train mode runs the training forward
of csrc/encoder_train.hip (every Dropout of the reference) through a `torch.autograd.Function` whose backward produces the
gradient of every parameter; `DurationPredictor(..., trainable=True)` does the same through csrc/duration_train.hip, including its
training branch (`reverse=False`: the MSE against log durations, :60-61).  Without `trainable=True` train mode is refused.  There is
no CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import weakref
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import call as _call, f32 as _f32
from ._handle import HandleModule

PRENET_LAYERS, PRENET_KERNEL = 3, 5            # unitspeech/encoder.py:283-284


@dataclass(frozen=True)
class EncoderConfig:
    """`Encoder.__init__` arguments; defaults are conf/hydra_config.py:85-105 (n_vocab: 149 symbols + 1 / 1000 units)."""
    n_vocab: int = 150
    n_feats: int = 80
    n_channels: int = 192
    filter_channels: int = 768
    n_heads: int = 2
    n_layers: int = 6
    kernel_size: int = 3
    window_size: Optional[int] = 4
    n_contentvec: int = 0          # > 0: emb is Linear(n_contentvec -> n_channels, bias=False) (checkpoints/voice-conversion.json: 768)


@dataclass(frozen=True)
class DurationPredictorConfig:
    """`DurationPredictor.__init__` arguments; defaults are conf/hydra_config.py:112-116."""
    in_channels: int = 192
    filter_channels: int = 256
    kernel_size: int = 3
    spk_emb_dim: int = 256


def encoder_state_shapes(cfg: EncoderConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """state_dict keys and shapes in the reference module's registration order (unitspeech/encoder.py:270-291)."""
    c, d = cfg.n_channels, cfg.n_channels // cfg.n_heads
    sh: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    sh["emb.weight"] = (c, cfg.n_contentvec) if cfg.n_contentvec else (cfg.n_vocab, c)      # Linear [out, in] / Embedding
    for i in range(PRENET_LAYERS):
        sh[f"prenet.conv_layers.{i}.weight"] = (c, c, PRENET_KERNEL)
        sh[f"prenet.conv_layers.{i}.bias"] = (c,)
    for i in range(PRENET_LAYERS):
        sh[f"prenet.norm_layers.{i}.gamma"] = (c,)
        sh[f"prenet.norm_layers.{i}.beta"] = (c,)
    sh["prenet.proj.weight"] = (c, c, 1)
    sh["prenet.proj.bias"] = (c,)
    for i in range(cfg.n_layers):
        p = f"encoder.attn_layers.{i}"
        if cfg.window_size:
            sh[p + ".emb_rel_k"] = (1, 2 * cfg.window_size + 1, d)
            sh[p + ".emb_rel_v"] = (1, 2 * cfg.window_size + 1, d)
        for n in "qkvo":
            sh[f"{p}.conv_{n}.weight"] = (c, c, 1)
            sh[f"{p}.conv_{n}.bias"] = (c,)
    for i in range(cfg.n_layers):
        sh[f"encoder.norm_layers_1.{i}.gamma"] = (c,)
        sh[f"encoder.norm_layers_1.{i}.beta"] = (c,)
    for i in range(cfg.n_layers):
        p = f"encoder.ffn_layers.{i}"
        sh[p + ".conv_1.weight"] = (cfg.filter_channels, c, cfg.kernel_size)
        sh[p + ".conv_1.bias"] = (cfg.filter_channels,)
        sh[p + ".conv_2.weight"] = (c, cfg.filter_channels, cfg.kernel_size)
        sh[p + ".conv_2.bias"] = (c,)
    for i in range(cfg.n_layers):
        sh[f"encoder.norm_layers_2.{i}.gamma"] = (c,)
        sh[f"encoder.norm_layers_2.{i}.beta"] = (c,)
    sh["proj_m.weight"] = (cfg.n_feats, c, 1)
    sh["proj_m.bias"] = (cfg.n_feats,)
    return sh


def duration_predictor_state_shapes(cfg: DurationPredictorConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    f, cin = cfg.filter_channels, cfg.in_channels + cfg.spk_emb_dim
    return OrderedDict([("conv_1.weight", (f, cin, cfg.kernel_size)), ("conv_1.bias", (f,)), ("norm_1.gamma", (f,)), ("norm_1.beta", (f,)),
                        ("conv_2.weight", (f, f, cfg.kernel_size)), ("conv_2.bias", (f,)), ("norm_2.gamma", (f,)), ("norm_2.beta", (f,)),
                        ("proj.weight", (1, f, 1)), ("proj.bias", (1,))])


def _synthetic(shapes, seed: int, tag: str, linear_front: bool = False) -> Dict[str, np.ndarray]:
    """Seeded weights from (seed, tensor name) with NumPy's Philox stream, like params.synthetic_state_dict: every tensor is
    non-trivial (the reference initialises `prenet.proj` to zero, which would hide the whole prenet from a parity test)."""
    out = OrderedDict()
    for name, shape in shapes.items():
        key = int.from_bytes(hashlib.sha256(f"{tag}/{seed}/{name}".encode()).digest()[:8], "little")
        g = np.random.Generator(np.random.Philox(key=key))
        z = g.standard_normal(shape, dtype=np.float32)
        if name.endswith("gamma"):
            v = 1.0 + 0.1 * z
        elif name.endswith(("beta", "bias")):
            v = 0.1 * z
        elif name == "emb.weight":
            v = z * (shape[0] if linear_front else shape[1]) ** -0.5      # n_channels ** -0.5 for either front, encoder.py:283
        elif "emb_rel" in name:
            v = z * shape[2] ** -0.5                       # :88-92
        else:                                             # Conv1d [out, in, k]
            v = z * (shape[1] * shape[2]) ** -0.5
        out[name] = v.astype(np.float32)
    return out


def synthetic_encoder_state_dict(cfg: EncoderConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    return _synthetic(encoder_state_shapes(cfg), seed, "encoder", bool(cfg.n_contentvec))


def synthetic_duration_predictor_state_dict(cfg: DurationPredictorConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    return _synthetic(duration_predictor_state_shapes(cfg), seed, "duration_predictor")


# ---- parameter containers (state_dict layout only; the arithmetic lives in csrc/frontend.hip) ----------------------------

class _Conv1dParams(torch.nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(cout, cin, k).normal_(0, (cin * k) ** -0.5))
        self.bias = torch.nn.Parameter(torch.zeros(cout))


class _NormParams(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.gamma = torch.nn.Parameter(torch.ones(c))
        self.beta = torch.nn.Parameter(torch.zeros(c))


class _EmbParams(torch.nn.Module):
    def __init__(self, n, c):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(n, c).normal_(0, c ** -0.5))


class _Prenet(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv_layers = torch.nn.ModuleList([_Conv1dParams(c, c, PRENET_KERNEL) for _ in range(PRENET_LAYERS)])
        self.norm_layers = torch.nn.ModuleList([_NormParams(c) for _ in range(PRENET_LAYERS)])
        self.proj = _Conv1dParams(c, c, 1)
        with torch.no_grad():
            self.proj.weight.zero_()           # encoder.py:54-55


class _AttnParams(torch.nn.Module):
    def __init__(self, c, n_heads, window):
        super().__init__()
        d = c // n_heads
        if window:
            self.emb_rel_k = torch.nn.Parameter(torch.randn(1, 2 * window + 1, d) * d ** -0.5)
            self.emb_rel_v = torch.nn.Parameter(torch.randn(1, 2 * window + 1, d) * d ** -0.5)
        self.conv_q = _Conv1dParams(c, c, 1)
        self.conv_k = _Conv1dParams(c, c, 1)
        self.conv_v = _Conv1dParams(c, c, 1)
        self.conv_o = _Conv1dParams(c, c, 1)


class _FfnParams(torch.nn.Module):
    def __init__(self, c, f, k):
        super().__init__()
        self.conv_1 = _Conv1dParams(c, f, k)
        self.conv_2 = _Conv1dParams(f, c, k)


class _Transformer(torch.nn.Module):
    def __init__(self, c, f, n_heads, n_layers, k, window):
        super().__init__()
        self.attn_layers = torch.nn.ModuleList([_AttnParams(c, n_heads, window) for _ in range(n_layers)])
        self.norm_layers_1 = torch.nn.ModuleList([_NormParams(c) for _ in range(n_layers)])
        self.ffn_layers = torch.nn.ModuleList([_FfnParams(c, f, k) for _ in range(n_layers)])
        self.norm_layers_2 = torch.nn.ModuleList([_NormParams(c) for _ in range(n_layers)])


class _FrontEndModule(HandleModule):
    """Owns one `us_frontend_handle`."""
    _abi, _what = "frontend", "front end"

    def _precondition(self, training_ok: bool = False):
        if self.training and not training_ok:
            hint = " or construct it with trainable=True to train it"
            raise RuntimeError(f"{type(self).__name__} is inference-only (the reference's Dropout layers are not built): call .eval()"
                               + hint)


class Encoder(_FrontEndModule):
    """`unitspeech/encoder.py:253` `Encoder(n_vocab, n_feats, n_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout,
    n_contentvec=0, window_size=None)`."""
    _train_abi = "encoder"                     # us_{_train_abi}_forward_train, _backward, _train_workspace_bytes, _tape_release

    def __init__(self, n_vocab, n_feats, n_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout=0.0, n_contentvec=0,
                 window_size=None, *, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        if n_contentvec:
            raise NotImplementedError("Encoder(n_contentvec > 0) (a Linear front instead of the Embedding, encoder.py:281) is a class of "
                                      "its own here: use ContentVecEncoder")
        self.cfg = EncoderConfig(int(n_vocab), int(n_feats), int(n_channels), int(filter_channels), int(n_heads), int(n_layers),
                                 int(kernel_size), int(window_size) if window_size else None)
        self.p_dropout = p_dropout
        self.emb = _EmbParams(n_vocab, n_channels)
        self.prenet = _Prenet(n_channels)
        self.encoder = _Transformer(n_channels, filter_channels, n_heads, n_layers, kernel_size, window_size)
        self.proj_m = _Conv1dParams(n_channels, n_feats, 1)

    def _create(self, lib, device):
        c = _lib.us_encoder_config(self.cfg.n_vocab, self.cfg.n_feats, self.cfg.n_channels, self.cfg.filter_channels, self.cfg.n_heads,
                                   self.cfg.n_layers, self.cfg.kernel_size, self.cfg.window_size or 0)
        _lib.check(lib.us_encoder_create(C.byref(self._h), C.byref(c)), None, "us_encoder_create")

    def forward(self, x, x_lengths):
        """x [B, L] symbol ids, x_lengths [B] -> (mu_x [B, n_feats, L], x [B, n_channels, L], x_mask [B, 1, L]).

        With trainable=True in train mode: the training forward (dropout p = 0.5 in the prenet, p_dropout elsewhere, seeded from
        torch's default generator), differentiable with respect to every parameter that requires grad."""
        if x.dim() != 2 or x_lengths.dim() != 1 or x_lengths.shape[0] != x.shape[0]:
            raise ValueError(f"Encoder: expected ids [B, L] and lengths [B], got {tuple(x.shape)} and {tuple(x_lengths.shape)}")
        if self.training and self.trainable:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            params = list(self.state_dict(keep_vars=True).values())
            return _EncoderTrain.apply(self, x, x_lengths, seed, float(self.p_dropout), *params)
        return self._forward_eval(x, x_lengths)

    def _operands(self, x, x_lengths):
        """What either forward hands to the library: [ids, lengths] as contiguous int64 on x's device, and the (mu_x, x, x_mask) it fills."""
        (b, l), dev = x.shape, x.device
        ins = [x.to(torch.int64).contiguous(), x_lengths.to(device=dev, dtype=torch.int64).contiguous()]
        return ins, (torch.empty(b, self.cfg.n_feats, l, device=dev), torch.empty(b, self.cfg.n_channels, l, device=dev),
                     torch.empty(b, 1, l, device=dev))

    @torch.no_grad()
    def _forward_eval(self, x, x_lengths):
        lib, stream = self._sync(x.device)
        ins, outs = self._operands(x, x_lengths)
        ws = self._workspace(lib, x.device, *x.shape)
        with torch.cuda.device(x.device):
            rc = lib.us_encoder_forward(self._h, *_ptrs(ins + list(outs)), *x.shape, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, "us_encoder_forward")
        return outs


    # ---- one launch group alone (the us_encoder_debug_* test hooks), for tests/test_encoder_train_kernels_gpu.py ---------------
    # Tensors are contiguous fp32 on the module's device, channel-last [B, L, C] as the kernels see them; mask is [B, L].

    def _debug(self, ref, b, l):
        lib, stream = self._sync(ref.device, training_ok=True)
        n = int(lib.us_encoder_debug_workspace_bytes(self._h, b, l))
        ws = self._dbg_ws = getattr(self, "_dbg_ws", None)
        if ws is None or ws.numel() < n or ws.device != ref.device:
            self._dbg_ws = None
            ws = self._dbg_ws = torch.empty(n, dtype=torch.uint8, device=ref.device)
        return lib, stream, ws

    @staticmethod
    def _ptr(t, shape, name):
        if t is None:
            return None
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or t.device.type != "cuda":
            raise ValueError(f"Encoder debug hook: {name} must be a contiguous fp32 {tuple(shape)} on the device, got {tuple(t.shape)} {t.dtype}")
        return t.data_ptr()

    @torch.no_grad()
    def debug_conv(self, key, mode, x=None, dout=None, mask=None, add=None, gate=None, gate_scale=1.0, mask_in=False, relu=False,
                   mask_out=False, drop_site=-1, p_dropout=0.0, seed=0):
        """The convolution `key` alone (us_encoder_debug_conv).  mode "fwd": x [B, L, Cin] -> out [B, L, Cout]; "wgrad": x, dout
        [B, L, Cout] -> (dw [Cout, Cin, K], db [Cout]); "dgrad": dout -> din [B, L, Cin] (with add, gate / gate_scale, mask_out)."""
        cout, cin, k = encoder_state_shapes(self.cfg)[key + ".weight"] if key + ".weight" in encoder_state_shapes(self.cfg) else (0, 0, 0)
        ref = x if x is not None else dout
        b, l = ref.shape[:2]
        lib, stream, ws = self._debug(ref, b, l)
        dev = ref.device
        m = {"fwd": _lib.US_ENCODER_CONV_FWD, "wgrad": _lib.US_ENCODER_CONV_WGRAD, "dgrad": _lib.US_ENCODER_CONV_DGRAD}[mode]
        flags = (_lib.US_ENCODER_CONV_MASK_IN if mask_in else 0) | (_lib.US_ENCODER_CONV_RELU if relu else 0) | \
            (_lib.US_ENCODER_CONV_MASK_OUT if mask_out else 0)
        out = dw = db = None
        if mode == "wgrad":
            dw, db = torch.empty(cout, cin, k, device=dev), torch.empty(cout, device=dev)
        else:
            out = torch.empty(b, l, cout if mode == "fwd" else cin, device=dev)
        P = self._ptr
        with torch.cuda.device(dev):
            rc = lib.us_encoder_debug_conv(self._h, key.encode(), m, P(x, (b, l, cin), "x"), P(dout, (b, l, cout), "dout"), P(mask, (b, l), "mask"),
                                           P(add, (b, l, cout if mode == "fwd" else cin), "add"), P(gate, (b, l, cin), "gate"), float(gate_scale),
                                           flags, int(drop_site), float(p_dropout), int(seed), P(out, out.shape, "out") if out is not None else None,
                                           P(dw, (cout, cin, k), "dw"), P(db, (cout,), "db"), b, l, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, f"us_encoder_debug_conv({key}, {mode})")
        return (dw, db) if mode == "wgrad" else out

    @torch.no_grad()
    def debug_ln_bwd(self, key, x, dy, gate=None, gate_scale=1.0):
        """Backward of the LayerNorm `key` alone (us_encoder_debug_ln_bwd): x, dy [B, L, C] -> (dx, dgamma, dbeta)."""
        b, l, c = x.shape
        lib, stream, ws = self._debug(x, b, l)
        dx, dg, db = torch.empty_like(x), torch.empty(c, device=x.device), torch.empty(c, device=x.device)
        P, sh = self._ptr, (b, l, self.cfg.n_channels)
        with torch.cuda.device(x.device):
            rc = lib.us_encoder_debug_ln_bwd(self._h, key.encode(), P(x, sh, "x"), P(dy, sh, "dy"), P(gate, sh, "gate"), float(gate_scale),
                                             dx.data_ptr(), dg.data_ptr(), db.data_ptr(), b, l, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, f"us_encoder_debug_ln_bwd({key})")
        return dx, dg, db

    @torch.no_grad()
    def debug_attention(self, layer, q, k, v, mask, p_dropout=0.0, seed=0, dO=None):
        """The attention of transformer layer `layer` alone, training form (us_encoder_debug_attention): q, k, v [B, L, C] ->
        {"out", "P"}, and with dO also {"DS", "dq", "dk", "dv", "emb_rel_k", "emb_rel_v"} (the last two only with a window)."""
        b, l, c = q.shape
        lib, stream, ws = self._debug(q, b, l)
        dev, h, d, w = q.device, self.cfg.n_heads, self.cfg.n_channels // self.cfg.n_heads, self.cfg.window_size or 0
        r = {"out": torch.empty(b, l, c, device=dev), "P": torch.empty(b, h, l, l, device=dev)}
        if dO is not None:
            r.update(DS=torch.empty(b, h, l, l, device=dev), dq=torch.empty(b, l, c, device=dev), dk=torch.empty(b, l, c, device=dev),
                     dv=torch.empty(b, l, c, device=dev))
            if w:
                r.update(emb_rel_k=torch.empty(1, 2 * w + 1, d, device=dev), emb_rel_v=torch.empty(1, 2 * w + 1, d, device=dev))
        P, sh = self._ptr, (b, l, self.cfg.n_channels)
        opt = lambda n: r[n].data_ptr() if n in r else None
        with torch.cuda.device(dev):
            rc = lib.us_encoder_debug_attention(self._h, int(layer), P(q, sh, "q"), P(k, sh, "k"), P(v, sh, "v"), P(mask, (b, l), "mask"),
                                                float(p_dropout), int(seed), r["out"].data_ptr(), r["P"].data_ptr(), P(dO, sh, "dO"), opt("DS"),
                                                opt("dq"), opt("dk"), opt("dv"), opt("emb_rel_k"), opt("emb_rel_v"), b, l, ws.data_ptr(),
                                                ws.numel(), stream)
        self._check(lib, rc, f"us_encoder_debug_attention({layer})")
        return r

    @torch.no_grad()
    def debug_embed_grad(self, ids, dx0):
        """emb.weight's gradient alone (us_encoder_debug_embed_grad): ids [B, L] int64, dx0 [B, L, C] -> [n_vocab, C]."""
        b, l = ids.shape
        lib, stream = self._sync(dx0.device, training_ok=True)
        if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device != dx0.device:
            raise ValueError("Encoder.debug_embed_grad: ids must be contiguous int64 on the device")
        grad = torch.empty(self.cfg.n_vocab, self.cfg.n_channels, device=dx0.device)
        with torch.cuda.device(dx0.device):
            rc = lib.us_encoder_debug_embed_grad(self._h, ids.data_ptr(), self._ptr(dx0, (b, l, self.cfg.n_channels), "dx0"), grad.data_ptr(),
                                                 b, l, stream)
        self._check(lib, rc, "us_encoder_debug_embed_grad")
        return grad


class _LinearParams(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(cout, cin).normal_(0, cout ** -0.5))      # encoder.py:280,283


class ContentVecEncoder(_FrontEndModule):
    """`unitspeech/encoder.py:253` `Encoder(..., n_contentvec=768, ...)`: the Encoder whose front is `Linear(n_contentvec ->
    n_channels, bias=False)` (:279-280), as `scripts/voice_conversion.py` builds it from checkpoints/voice-conversion.json.  Same
    argument list and `state_dict` as the reference (`contentvec_encoder.pt`'s ["model"] loads strictly); `n_vocab` is accepted and
    unused.  `forward(feats [B, L, n_contentvec], lengths [B]) -> (mu_x, x, x_mask)`.  Rows of `feats` at or past an item's length
    are never read.  `trainable=True`: as `Encoder`, differentiable with respect to every parameter (not to `feats`)."""
    _train_abi = "encoder"
    _train_forward, _train_backward = "us_encoder_forward_features_train", "us_encoder_backward_features"

    def __init__(self, n_vocab, n_feats, n_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout=0.0, n_contentvec=768,
                 window_size=None, *, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        if not 1 <= int(n_contentvec) <= 1024:
            raise ValueError(f"ContentVecEncoder: n_contentvec must be in 1..1024, got {n_contentvec}")
        self.cfg = EncoderConfig(int(n_vocab), int(n_feats), int(n_channels), int(filter_channels), int(n_heads), int(n_layers),
                                 int(kernel_size), int(window_size) if window_size else None, int(n_contentvec))
        self.p_dropout = p_dropout
        self.emb = _LinearParams(n_contentvec, n_channels)
        self.prenet = _Prenet(n_channels)
        self.encoder = _Transformer(n_channels, filter_channels, n_heads, n_layers, kernel_size, window_size)
        self.proj_m = _Conv1dParams(n_channels, n_feats, 1)

    def _create(self, lib, device):
        c = _lib.us_encoder_config(1, self.cfg.n_feats, self.cfg.n_channels, self.cfg.filter_channels, self.cfg.n_heads, self.cfg.n_layers,
                                   self.cfg.kernel_size, self.cfg.window_size or 0)
        _lib.check(lib.us_encoder_create_contentvec(C.byref(self._h), C.byref(c), self.cfg.n_contentvec), None,
                   "us_encoder_create_contentvec")

    def forward(self, feats, lengths):
        """feats [B, L, n_contentvec], lengths [B] -> (mu_x [B, n_feats, L], x [B, n_channels, L], x_mask [B, 1, L])."""
        if feats.dim() != 3 or feats.shape[2] != self.cfg.n_contentvec or lengths.dim() != 1 or lengths.shape[0] != feats.shape[0]:
            raise ValueError(f"ContentVecEncoder: expected features [B, L, {self.cfg.n_contentvec}] and lengths [B], got "
                             f"{tuple(feats.shape)} and {tuple(lengths.shape)}")
        if self.training and self.trainable:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            params = list(self.state_dict(keep_vars=True).values())
            return _ContentVecEncoderTrain.apply(self, feats, lengths, seed, float(self.p_dropout), *params)
        return self._forward_eval(feats, lengths)

    def _operands(self, feats, lengths):
        (b, l, _), dev = feats.shape, feats.device
        ins = [_f32(feats, dev), lengths.to(device=dev, dtype=torch.int64).contiguous()]
        return ins, (torch.empty(b, self.cfg.n_feats, l, device=dev), torch.empty(b, self.cfg.n_channels, l, device=dev),
                     torch.empty(b, 1, l, device=dev))

    @torch.no_grad()
    def _forward_eval(self, feats, lengths):
        lib, stream = self._sync(feats.device)
        ins, outs = self._operands(feats, lengths)
        b, l = feats.shape[:2]
        ws = self._workspace(lib, feats.device, b, l)
        with torch.cuda.device(feats.device):
            rc = lib.us_encoder_forward_features(self._h, *_ptrs(ins + list(outs)), b, l, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, "us_encoder_forward_features")
        return outs


def _ptrs(tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


# ---- the autograd bridge of the two trainable modules ----------------------------------------------------------------------
# Each training forward owns its workspace, which is the tape: ctx keeps it until backward.  The two C ABIs end alike:
# us_{abi}_forward_train(h, operands..., B, L, p, seed, ws, bytes, stream), us_{abi}_backward(h, upstream..., B, L, keys, grads, n, ws,
# bytes, stream).

def _release_tape(mod_ref, ptr):
    mod = mod_ref()
    if mod is not None and getattr(mod, "_h", None):
        getattr(_lib.load(), f"us_{mod._train_abi}_tape_release")(mod._h, ptr)


def _tape_forward(ctx, mod, operands, b, l, p, seed, params):
    """Run mod's training forward on `operands` (tensors on the device, or None) into a workspace of its own, kept in ctx as the tape."""
    device = operands[0].device
    lib, stream = mod._sync(device, training_ok=True)
    abi = mod._train_abi
    ws = torch.empty(int(getattr(lib, f"us_{abi}_train_workspace_bytes")(mod._h, b, l)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        name = getattr(mod, "_train_forward", f"us_{abi}_forward_train")
        rc = getattr(lib, name)(mod._h, *_ptrs(operands), b, l, p, seed, ws.data_ptr(), ws.numel(), stream)
    mod._check(lib, rc, name)
    ctx.mod, ctx.ws, ctx.shape = mod, ws, (b, l)
    ctx.versions = [(t.data_ptr(), t._version) for t in params]
    # the handle forgets this tape when the workspace tensor goes (its memory may then hold anything)
    weakref.finalize(ws, _release_tape, weakref.ref(mod), ws.data_ptr())


def _tape_backward(ctx, upstream, n_inputs):
    """mod's backward from the tape in ctx for the `upstream` gradients (None: zero); what autograd's backward returns: None for
    the n_inputs inputs in front of the parameters, then the gradient of every parameter that requires one."""
    mod, ws, (b, l) = ctx.mod, ctx.ws, ctx.shape
    sd = mod.state_dict(keep_vars=True)
    if [(t.data_ptr(), t._version) for t in sd.values()] != ctx.versions:
        raise RuntimeError(f"{type(mod).__name__} backward: a parameter was modified in place after the training forward (the tape holds "
                           "activations of the old weights); run the forward again")
    device = ws.device
    lib, stream = mod._sync(device, training_ok=True)
    grads = [torch.empty(t.shape, device=device) if n else None for t, n in zip(sd.values(), ctx.needs_input_grad[n_inputs:])]
    sel = [(k, g) for k, g in zip(sd, grads) if g is not None]
    keys = (C.c_char_p * max(len(sel), 1))(*[k.encode() for k, _ in sel])
    ptrs = (C.c_void_p * max(len(sel), 1))(*[g.data_ptr() for _, g in sel])
    upstream = [_f32(t, device) for t in upstream]
    with torch.cuda.device(device):
        name = getattr(mod, "_train_backward", f"us_{mod._train_abi}_backward")
        rc = getattr(lib, name)(mod._h, *_ptrs(upstream), b, l, keys, ptrs, len(sel), ws.data_ptr(), ws.numel(), stream)
    mod._check(lib, rc, name)
    return (None,) * n_inputs + tuple(grads)


class _EncoderTrain(torch.autograd.Function):
    """us_encoder_forward_train / us_encoder_backward.  p < 0 runs without any dropout (the reference in eval mode, differentiated)."""

    @staticmethod
    def forward(ctx, enc, x, x_lengths, seed, p, *params):
        ins, outs = enc._operands(x, x_lengths)
        _tape_forward(ctx, enc, ins + list(outs), *x.shape, p, seed, params)
        ctx.mark_non_differentiable(outs[2])
        return outs

    @staticmethod
    def backward(ctx, g_mu, g_x, _g_mask):
        return _tape_backward(ctx, (g_mu, g_x), 5)


class _ContentVecEncoderTrain(torch.autograd.Function):
    """us_encoder_forward_features_train / us_encoder_backward_features.  The backward is handed the features again (the tape does
    not copy them); no gradient is returned for them."""

    @staticmethod
    def forward(ctx, enc, feats, lengths, seed, p, *params):
        ins, outs = enc._operands(feats, lengths)
        _tape_forward(ctx, enc, ins + list(outs), *feats.shape[:2], p, seed, params)
        ctx.feats = ins[0]
        ctx.mark_non_differentiable(outs[2])
        return outs

    @staticmethod
    def backward(ctx, g_mu, g_x, _g_mask):
        return _tape_backward(ctx, (ctx.feats, g_mu, g_x), 5)


class DurationPredictor(_FrontEndModule):
    """`unitspeech/duration_predictor.py:24` `DurationPredictor(in_channels, filter_channels, kernel_size, p_dropout, spk_emb_dim=0)`.

    Without `trainable=True` it is inference only (eval mode, `reverse=True`).  With it, a call made in train mode (both Dropouts at
    p_dropout, seeded from torch's default generator) or in eval mode with grad enabled (no dropout) is differentiable with respect to
    every parameter that requires grad: `reverse=True` returns logw, `reverse=False` the loss of :60-62 against `w`.  No gradient leaves
    through `x` (the reference detaches it) or through `g` (a `g` that requires grad is refused rather than silently given None).
    In eval mode under `torch.no_grad()` the inference path runs, so its bits are the non-trainable module's."""

    _train_abi = "duration_predictor"

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout=0.0, spk_emb_dim=0, *, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.cfg = DurationPredictorConfig(int(in_channels), int(filter_channels), int(kernel_size), int(spk_emb_dim))
        self.p_dropout = p_dropout
        cin = in_channels + spk_emb_dim
        self.conv_1 = _Conv1dParams(cin, filter_channels, kernel_size)
        self.norm_1 = _NormParams(filter_channels)
        self.conv_2 = _Conv1dParams(filter_channels, filter_channels, kernel_size)
        self.norm_2 = _NormParams(filter_channels)
        self.proj = _Conv1dParams(filter_channels, 1, 1)

    def _create(self, lib, device):
        c = _lib.us_duration_config(self.cfg.in_channels, self.cfg.filter_channels, self.cfg.kernel_size, self.cfg.spk_emb_dim)
        _lib.check(lib.us_duration_predictor_create(C.byref(self._h), C.byref(c)), None, "us_duration_predictor_create")

    def forward(self, x, x_mask, w=None, g=None, reverse=False):
        """x [B, in_channels, L], x_mask [B, 1, L], g [B, 1, spk_emb_dim] -> logw [B, 1, L] (reverse=True), or with w [B, 1, L] the
        scalar loss sum((logw - log(w + 1e-6) x_mask)^2) / sum(x_mask) (reverse=False, trainable=True only)."""
        if not reverse and not self.trainable:
            raise NotImplementedError("DurationPredictor(reverse=False) (the training loss, duration_predictor.py:60-61) needs "
                                      "trainable=True")
        if x.dim() != 3 or x.shape[1] != self.cfg.in_channels or x_mask.shape != (x.shape[0], 1, x.shape[2]):
            raise ValueError(f"DurationPredictor: expected x [B, {self.cfg.in_channels}, L] and x_mask [B, 1, L], got {tuple(x.shape)} "
                             f"and {tuple(x_mask.shape)}")
        if (g is None) != (self.cfg.spk_emb_dim == 0) or (g is not None and tuple(g.shape) != (x.shape[0], 1, self.cfg.spk_emb_dim)):
            raise ValueError(f"DurationPredictor: g must be [B, 1, {self.cfg.spk_emb_dim}] (None iff spk_emb_dim == 0)")
        if not reverse and (w is None or w.numel() != x_mask.numel()):
            raise ValueError("DurationPredictor(reverse=False): w [B, 1, L] (the target durations) is required")
        if self.trainable and (self.training or torch.is_grad_enabled()):
            if g is not None and g.requires_grad:
                raise RuntimeError("DurationPredictor: g requires grad, but this module returns no gradient for g (conv_1's data gradient "
                                   "is not built); pass g.detach()")
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.training else 0
            params = list(self.state_dict(keep_vars=True).values())
            logw = _DurationTrain.apply(self, x, x_mask, g, seed, float(self.p_dropout) if self.training else -1.0, *params)
        else:
            logw = self._forward_eval(x, x_mask, g)
        return logw if reverse else _DurationMseFn.apply(logw, w, x_mask)

    def _operands(self, x, x_mask, g):
        """What either forward hands to the library: [x, x_mask, g] as contiguous fp32 on x's device (g None without a speaker
        embedding), and the logw [B, 1, L] it fills."""
        return [_f32(t, x.device) for t in (x, x_mask, g)], torch.empty(x.shape[0], 1, x.shape[2], device=x.device)

    @torch.no_grad()
    def _forward_eval(self, x, x_mask, g):
        lib, stream = self._sync(x.device)
        ins, logw = self._operands(x, x_mask, g)
        ws = self._workspace(lib, x.device, x.shape[0], x.shape[2])
        with torch.cuda.device(x.device):
            rc = lib.us_duration_predictor_forward(self._h, *_ptrs(ins + [logw]), x.shape[0], x.shape[2], ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, "us_duration_predictor_forward")
        return logw


class _DurationTrain(torch.autograd.Function):
    """us_duration_predictor_forward_train / us_duration_predictor_backward.  p < 0 runs without dropout (the reference in eval
    mode, differentiated)."""

    @staticmethod
    def forward(ctx, dp, x, x_mask, g, seed, p, *params):
        ins, logw = dp._operands(x, x_mask, g)
        _tape_forward(ctx, dp, ins + [logw], x.shape[0], x.shape[2], p, seed, params)
        return logw

    @staticmethod
    def backward(ctx, g_logw):
        return _tape_backward(ctx, (g_logw,), 6)


class _DurationMseFn(torch.autograd.Function):
    """us_duration_predictor_mse_loss: duration_predictor.py:60-62, differentiable in logw."""

    @staticmethod
    def forward(ctx, logw, w, x_mask):
        device = logw.device
        lw, ww, m = _f32(logw, device), _f32(w, device), _f32(x_mask, device)
        loss = torch.empty((), device=device)
        d_logw = torch.empty_like(lw)
        _call(device, "us_duration_predictor_mse_loss", lw, ww, m, loss, d_logw, lw.shape[0], lw.shape[-1])
        ctx.save_for_backward(d_logw)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_logw,) = ctx.saved_tensors
        return d_logw * g, None, None
