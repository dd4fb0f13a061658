"""ECAPA-TDNN speaker encoder on the HIP library: the upstream model's hidden states -> speaker embedding [B, emb_dim] (inference).

Drop-in for the reference's `unitspeech/speaker_encoder/ecapa_tdnn.py:164-298` `ECAPA_TDNN` / `ECAPA_TDNN_SMALL` from the hidden
states on: the same constructor arguments, the same module tree and therefore the same `state_dict` keys, shapes and order with
every `feature_extract.*` key removed (the fbank / mfcc extraction is not part of this library; a WavLM upstream is `wavlm.WavLMModel`,
put in front with `attach_upstream`, after which `forward(wav)` is the reference's).
The torch modules below only hold parameters; the arithmetic is `csrc/speaker.hip`.

`forward_features(hidden_states)` is the entry point: `[L, B, T, C]`, a list of L `[B, T, C]`, or an already combined `[B, C, T]`.
With `lengths` (valid frames per item) the batch is ragged: nothing past an item's end reaches its embedding, and each row has the
bits the item gives when it runs alone (`us_speaker_forward_lengths`).
There is no CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
from torch import nn

from . import _lib
from ._args import c_lengths, host_lengths
from ._handle import HandleModule

# number of hidden states the s3prl upstreams return (the CNN output plus one per transformer layer): the length of `feature_weight`
UPSTREAM_LAYERS = {"wavlm_large": 25, "hubert_large_ll60k": 25, "wav2vec2_xlsr": 25, "wav2vec2_large_ll60k": 25,
                   "wavlm_base_plus": 13, "wavlm_base": 13, "hubert_base": 13, "wav2vec2_base_960": 13}
OUT_CHANNELS = 1536            # ecapa_tdnn.py:222
BOTTLENECK = 128               # se_bottleneck_dim and attention_channels (:225-232)
SCALE = 8
STAGES = {"feat": 0, "layer1": 1, "blocks": 2, "pooling": 3}
ACTS = {None: _lib.US_SPEAKER_ACT_NONE, "none": _lib.US_SPEAKER_ACT_NONE, "relu": _lib.US_SPEAKER_ACT_RELU, "tanh": _lib.US_SPEAKER_ACT_TANH}


class _Conv1dReluBn(nn.Module):
    def __init__(self, cin, cout, k=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k)
        self.bn = nn.BatchNorm1d(cout)


class _Res2Conv1dReluBn(nn.Module):
    def __init__(self, channels):
        super().__init__()
        w = channels // SCALE
        self.convs = nn.ModuleList([nn.Conv1d(w, w, 3) for _ in range(SCALE - 1)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(w) for _ in range(SCALE - 1)])


class _SEConnect(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.linear1 = nn.Linear(channels, BOTTLENECK)
        self.linear2 = nn.Linear(BOTTLENECK, channels)


class _SERes2Block(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.Conv1dReluBn1 = _Conv1dReluBn(channels, channels)
        self.Res2Conv1dReluBn = _Res2Conv1dReluBn(channels)
        self.Conv1dReluBn2 = _Conv1dReluBn(channels, channels)
        self.SE_Connect = _SEConnect(channels)


class _AttentiveStatsPool(nn.Module):
    def __init__(self, in_dim, global_context_att):
        super().__init__()
        self.linear1 = nn.Conv1d(in_dim * 3 if global_context_att else in_dim, BOTTLENECK, 1)
        self.linear2 = nn.Conv1d(BOTTLENECK, in_dim, 1)


class ECAPA_TDNN(HandleModule):
    """`ECAPA_TDNN(...)` of ecapa_tdnn.py:164.  `feat_num` (not a reference argument) gives the number of hidden states for an upstream
    `feat_type` this module does not know (the reference asks the upstream itself, :237-246)."""
    _abi, _what = "speaker", "speaker encoder"
    # weights: every floating-point entry of the state_dict (`num_batches_tracked` plays no part in eval mode), ~200 keys against a
    # forward of a millisecond or two, and no parameter is ever registered anew
    _cache_sources = True

    def __init__(self, feat_dim=80, channels=512, emb_dim=192, global_context_att=False, feat_type='fbank', sr=16000,
                 feature_selection="hidden_states", update_extract=False, config_path=None, feat_num=None):
        super().__init__()
        if channels <= 0 or channels % SCALE != 0:
            raise ValueError(f"channels must be a positive multiple of {SCALE}, got {channels}")
        self.feat_type, self.feature_selection, self.update_extract, self.sr = feat_type, feature_selection, False, sr
        self.feat_dim, self.emb_dim, self.global_context_att = int(feat_dim), int(emb_dim), bool(global_context_att)
        if feat_type in ("fbank", "mfcc"):
            self.feat_num = 0
        else:
            if feat_num is None and feat_type not in UPSTREAM_LAYERS:
                raise ValueError(f"feat_type {feat_type!r}: give feat_num, the number of hidden states the upstream returns")
            self.feat_num = int(feat_num if feat_num is not None else UPSTREAM_LAYERS[feat_type])
            self.feature_weight = nn.Parameter(torch.zeros(self.feat_num))
        self.instance_norm = nn.InstanceNorm1d(feat_dim)
        self.channels = [channels] * 4 + [OUT_CHANNELS]
        self.layer1 = _Conv1dReluBn(feat_dim, channels, 5)
        self.layer2 = _SERes2Block(channels)
        self.layer3 = _SERes2Block(channels)
        self.layer4 = _SERes2Block(channels)
        self.conv = nn.Conv1d(channels * 3, OUT_CHANNELS, 1)
        self.pooling = _AttentiveStatsPool(OUT_CHANNELS, self.global_context_att)
        self.bn = nn.BatchNorm1d(OUT_CHANNELS * 2)
        self.linear = nn.Linear(OUT_CHANNELS * 2, emb_dim)

    def config(self) -> dict:
        return {"feat_dim": self.feat_dim, "channels": self.channels[0], "emb_dim": self.emb_dim,
                "global_context_att": self.global_context_att, "n_layers": self.feat_num}

    def load_state_dict(self, state_dict, strict=True, **kw):
        if any(".shortcut." in k for k in state_dict):
            raise RuntimeError("ECAPA_TDNN: the state_dict has SE_Res2Block `shortcut` keys (in_channels != out_channels), which this "
                               "module does not build: every block of the reference's configuration keeps its channel count")
        return super().load_state_dict(state_dict, strict=strict, **kw)

    # ---- engine ----------------------------------------------------------------------------------------------------------

    def _config_struct(self):
        c = _lib.us_speaker_config()
        c.feat_dim, c.channels, c.emb_dim, c.n_layers = self.feat_dim, self.channels[0], self.emb_dim, self.feat_num
        c.global_context_att = int(self.global_context_att)
        return c

    def _create(self, lib, device):
        c = self._config_struct()
        _lib.check(lib.us_speaker_create(C.byref(self._h), C.byref(c)), None, "us_speaker_create")

    def _input(self, hidden_states):
        """-> (contiguous fp32 tensor, L, B, T) with L = 0 for the combined [B, C, T] form."""
        if isinstance(hidden_states, (list, tuple)):
            hidden_states = torch.stack(list(hidden_states), dim=0)
        x = hidden_states
        if x.dim() == 4:
            if self.feat_num == 0:
                raise ValueError(f"ECAPA_TDNN(feat_type={self.feat_type!r}) has no feature_weight: give the combined [B, {self.feat_dim}, T]")
            if x.shape[0] != self.feat_num or x.shape[3] != self.feat_dim or x.shape[1] < 1 or x.shape[2] < 1:
                raise ValueError(f"ECAPA_TDNN: expected hidden states [{self.feat_num}, B, T, {self.feat_dim}], got {tuple(x.shape)}")
            L, B, T = x.shape[0], x.shape[1], x.shape[2]
        elif x.dim() == 3:
            if x.shape[1] != self.feat_dim or x.shape[0] < 1 or x.shape[2] < 1:
                raise ValueError(f"ECAPA_TDNN: expected combined features [B, {self.feat_dim}, T], got {tuple(x.shape)}")
            L, B, T = 0, x.shape[0], x.shape[2]
        else:
            raise ValueError(f"ECAPA_TDNN: expected [L, B, T, C] or [B, C, T], got {tuple(x.shape)}")
        return x.detach().to(dtype=torch.float32).contiguous(), int(L), int(B), int(T)

    @torch.no_grad()
    def _run(self, hidden_states, normalize: bool, lengths=None, what="forward_features"):
        x, L, B, T = self._input(hidden_states)
        lengths = host_lengths(lengths, B, "ECAPA_TDNN." + what)
        device = x.device
        lib, stream = self._sync(device)
        out = torch.empty(B, self.emb_dim, device=device)
        ws = self._workspace(lib, device, B, T)
        if lengths is None:
            self._call(lib, device, "forward", self._h, x.data_ptr(), L, B, T, out.data_ptr(), int(normalize), ws.data_ptr(), ws.numel(), stream)
        else:
            self._call(lib, device, "forward_lengths", self._h, x.data_ptr(), L, B, T, c_lengths(lengths), out.data_ptr(), int(normalize),
                       ws.data_ptr(), ws.numel(), stream)
        self._last = (B, T)
        return out

    def forward_features(self, hidden_states, lengths=None):
        """`ECAPA_TDNN.forward` (:274-287) from `get_feat`'s input on: -> [B, emb_dim].  `lengths` (B values in [1, T], a list or a tensor):
        item b is valid on its first lengths[b] frames of the padded T, whatever lies past them (NaN included) is never used, and row b
        has the bits of `forward_features` on that item alone."""
        return self._run(hidden_states, False, lengths)

    def embed(self, hidden_states, lengths=None):
        """finetune.py:106-110: the embedding of one utterance divided by its norm, [1, emb_dim].  With `lengths`: a ragged batch, each row
        divided by its own norm, [B, emb_dim]."""
        if lengths is None and self._input(hidden_states)[2] != 1:
            raise ValueError("ECAPA_TDNN.embed: one utterance at a time (the norm is taken over the whole output): item 1 is one too many; "
                             "give `lengths` for a batch, which divides each row by its own norm")
        return self._run(hidden_states, True, lengths, "embed")

    @torch.no_grad()
    def debug_conv(self, prefix, x, bn_prefix=None, act=None, bias2=None, out=None):
        """One dense convolution alone through the launch `forward_features` uses (us_speaker_debug_conv): `layer1.conv`,
        `layer<l>.Conv1dReluBn<1|2>.conv`, `conv`, `pooling.linear1` (the first 1536 input channels of its weight) or `pooling.linear2`;
        -> bn(act(conv(x) + bias + bias2)).  x [B, Cin, T] and `out` [B, Cout, T] are fp32 with time contiguous and channels T apart, and
        may be channel slices of wider tensors (their batch strides are passed on); bias2 [B, Cout]."""
        device = x.device
        lib, stream = self._sync(device)
        mod = self.get_submodule(prefix)
        cin = OUT_CHANNELS if prefix == "pooling.linear1" else mod.in_channels
        cout = mod.out_channels
        if x.dim() != 3 or x.shape[1] != cin or x.shape[2] < 1:
            raise ValueError(f"ECAPA_TDNN.debug_conv({prefix}): expected [B, {cin}, T], got {tuple(x.shape)}")
        b, _, t = x.shape
        if out is None:
            out = torch.empty(b, cout, t, device=device)
        for name, v, c in (("x", x, cin), ("out", out, cout)):
            if tuple(v.shape) != (b, c, t) or v.dtype != torch.float32 or v.device != device or (t > 1 and v.stride(2) != 1) or \
                    (c > 1 and v.stride(1) != t) or (b > 1 and v.stride(0) < c * t):
                raise ValueError(f"ECAPA_TDNN.debug_conv({prefix}): {name} must be fp32 [{b}, {c}, {t}] on {device}, time contiguous, channels "
                                 f"{t} apart")
        if bias2 is not None:
            bias2 = bias2.detach().to(device=device, dtype=torch.float32).contiguous()
            if tuple(bias2.shape) != (b, cout):
                raise ValueError(f"ECAPA_TDNN.debug_conv({prefix}): bias2 must be [{b}, {cout}]")
        bs = lambda v, c: int(v.stride(0)) if b > 1 else c * t
        with torch.cuda.device(device):
            rc = lib.us_speaker_debug_conv(self._h, prefix.encode(), bn_prefix.encode() if bn_prefix else None, ACTS[act], x.data_ptr(),
                                           bs(x, cin), out.data_ptr(), bs(out, cout), None if bias2 is None else bias2.data_ptr(), b, t, stream)
        self._check(lib, rc, f"us_speaker_debug_conv({prefix})")
        return out

    # ---- the upstream in front (get_feat, :248-272) ------------------------------------------------------------------------------

    def attach_upstream(self, wavlm, normalize=True):
        """Put a `wavlm.WavLMModel` in front: `forward(wav [B, T])` then runs it and the trunk on all its hidden states, which the
        library writes as [L + 1, B, F, H] (`get_feat` + `forward`, :248-287).  `normalize`: s3prl's wavlm_large applies
        `F.layer_norm(wav, wav.shape)` to each waveform first.  The upstream is not a submodule: its parameters stay out of
        `state_dict()`, as `feature_extract.*` does in this module's checkpoints; `.to()` and `.cuda()` move it along."""
        n = wavlm.config["num_hidden_layers"] + 1
        if n != self.feat_num or wavlm.config["hidden_size"] != self.feat_dim:
            raise ValueError(f"ECAPA_TDNN.attach_upstream: the upstream gives {n} hidden states of width {wavlm.config['hidden_size']}, the trunk "
                             f"takes {self.feat_num} of width {self.feat_dim}")
        object.__setattr__(self, "_upstream", wavlm.eval())
        self._upstream_normalize = bool(normalize)
        return self

    @property
    def upstream(self):
        return self.__dict__.get("_upstream")

    def _apply(self, fn, *args, **kwargs):
        if self.upstream is not None:
            self.upstream._apply(fn, *args, **kwargs)
        return super()._apply(fn, *args, **kwargs)

    def _hidden_states(self, wav, lengths=None):
        _, hs = self.upstream(wav, lengths, output_hidden_states=True, normalize=self._upstream_normalize, layers_first=True)
        return hs

    def _frames(self, wav, lengths):
        """samples per item -> the upstream's frames per item (None stays None)"""
        v = host_lengths(lengths, wav.shape[0], "ECAPA_TDNN.forward")
        return None if v is None else [self.upstream.frames(n) for n in v]

    def forward(self, x, lengths=None):
        """`ECAPA_TDNN.forward(wav)` (:248-287): wav [B, T] at 16 kHz -> [B, emb_dim].  `lengths` are samples per item: the upstream runs
        ragged and the trunk runs over `upstream.frames(lengths[b])` frames of item b, so row b is what the item gives alone.  (Before the
        trunk took lengths, this call ran it over all frames of the padded batch, and the padded frames entered the statistics of the
        shorter items; no caller relied on those numbers.)"""
        if self.upstream is None:
            raise NotImplementedError("ECAPA_TDNN.forward(wav) needs the upstream feature extractor (WavLM / HuBERT through s3prl, or fbank / mfcc), "
                                      "which is outside this library: run the upstream and call forward_features(hidden_states)")
        return self._run(self._hidden_states(x, lengths), False, self._frames(x, lengths), "forward")

    def embed_wav(self, wav, lengths=None):
        """finetune.py:113-117: the embedding of one 16 kHz utterance [1, T] divided by its norm, [1, emb_dim].  With `lengths` (samples per
        item): a padded batch [B, T], each row divided by its own norm."""
        if self.upstream is None:
            raise NotImplementedError("ECAPA_TDNN.embed_wav needs an upstream: attach_upstream(WavLMModel), or run the upstream and call "
                                      "embed(hidden_states)")
        if wav.dim() != 2 or (lengths is None and wav.shape[0] != 1):
            raise ValueError("ECAPA_TDNN.embed_wav: one utterance [1, T] at a time (the norm is taken over the whole output), or a padded "
                             "batch [B, T] with `lengths`")
        return self._run(self._hidden_states(wav, lengths), True, self._frames(wav, lengths), "embed_wav")

    @torch.no_grad()
    def stage(self, name: str) -> torch.Tensor:
        """An intermediate of the last forward_features call (a copy): `feat` [B, C, T] after get_feat, `layer1` [B, channels, T],
        `blocks` [B, 3 channels, T] (layer2, layer3, layer4 along the channels) and `pooling` [B, 3072] before `bn`.  After a call with
        `lengths`, T is the padded length and only the first lengths[b] frames of item b are defined (`feat` is 0 past them, the others hold
        whatever the workspace held)."""
        lib = _lib.load()
        B, T = self._last
        ptr, shape = C.c_void_p(), (C.c_int64 * 3)()
        rc = lib.us_speaker_stage(self._h, STAGES[name], B, T, self._ws.data_ptr(), self._ws.numel(), C.byref(ptr), shape)
        self._check(lib, rc, f"us_speaker_stage({name})")
        off, n = ptr.value - self._ws.data_ptr(), shape[0] * shape[1] * shape[2]
        torch.cuda.current_stream(self._ws.device).synchronize()
        out = self._ws[off:off + 4 * n].view(torch.float32).view(*[s for s in shape]).clone()
        return out.squeeze(-1) if name == "pooling" else out


def ECAPA_TDNN_SMALL(feat_dim, emb_dim=256, feat_type='fbank', sr=16000, feature_selection="hidden_states", update_extract=False,
                     config_path=None, feat_num=None):
    return ECAPA_TDNN(feat_dim=feat_dim, channels=512, emb_dim=emb_dim, feat_type=feat_type, sr=sr, feature_selection=feature_selection,
                      update_extract=update_extract, config_path=config_path, feat_num=feat_num)


def load_speaker_encoder_checkpoint(path, device=None, feat_dim=1024, emb_dim=256, feat_type="wavlm_large"):
    """unitspeech/util.py:183-188 `get_speaker_embedder` on the HIP module: ECAPA_TDNN_SMALL(1024, 256, "wavlm_large"), the
    checkpoint's {"model": state_dict} without its `feature_extract.*` keys loaded strictly, eval mode."""
    state_dict = torch.load(path, map_location=lambda storage, loc: storage)
    model = ECAPA_TDNN_SMALL(feat_dim=feat_dim, emb_dim=emb_dim, feat_type=feat_type, config_path=None)
    sd = OrderedDict((k, v) for k, v in state_dict["model"].items() if not k.startswith("feature_extract."))
    model.load_state_dict(sd, strict=True)
    model = model.eval()
    return model.to(device) if device is not None else model


def load_speaker_embedder_checkpoint(path, device=None, feat_type="wavlm_large", **wavlm_config):
    """The reference's whole speaker embedder from its {"model": state_dict} file: the trunk from the keys outside `feature_extract.*`, as
    `load_speaker_encoder_checkpoint` loads it (sizes from the tensor shapes), and a `WavLMModel` from the `feature_extract.model.*`
    keys through `from_fairseq_wavlm_state_dict`, its sizes read from the shapes too (`wavlm.wavlm_config_from_state_dict`; keywords
    override), attached with s3prl's waveform normalisation when the extractor is the layer-norm form.  Eval mode."""
    from .wavlm import WavLMModel, from_fairseq_wavlm_state_dict, wavlm_config_from_state_dict
    sd = torch.load(path, map_location=lambda storage, loc: storage)["model"]
    pre = "feature_extract.model."
    up = OrderedDict((k[len(pre):], v) for k, v in sd.items() if k.startswith(pre))
    if not up:
        raise ValueError(f"{path} holds no `feature_extract.*` keys, so there is no upstream to load: use load_speaker_encoder_checkpoint "
                         "and forward_features(hidden_states)")
    up = from_fairseq_wavlm_state_dict(up)
    cfg = wavlm_config_from_state_dict(up, **wavlm_config)
    wavlm = WavLMModel(**cfg)
    wavlm.load_state_dict(up)
    trunk = OrderedDict((k, v) for k, v in sd.items() if not k.startswith("feature_extract."))
    model = ECAPA_TDNN(feat_dim=int(trunk["layer1.conv.weight"].shape[1]), channels=int(trunk["layer1.conv.weight"].shape[0]),
                       emb_dim=int(trunk["linear.weight"].shape[0]), feat_type=feat_type, feat_num=int(trunk["feature_weight"].shape[0]),
                       global_context_att=int(trunk["pooling.linear1.weight"].shape[1]) == 3 * OUT_CHANNELS)
    model.load_state_dict(trunk, strict=True)
    model = model.eval().attach_upstream(wavlm, normalize=cfg["feat_extract_norm"] == "layer")
    return model.to(device) if device is not None else model


def _rng(seed: int, name: str) -> np.random.Generator:
    key = int.from_bytes(hashlib.sha256(f"ecapa/{seed}/{name}".encode()).digest()[:8], "little")
    return np.random.Generator(np.random.Philox(key=key))


def _module(cfg) -> ECAPA_TDNN:
    n = int(cfg.get("n_layers", 0))
    return ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"],
                      global_context_att=bool(cfg["global_context_att"]), feat_type="upstream" if n else "fbank", feat_num=n or None)


def synthetic_ecapa_state_dict(cfg, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded weights in the reference's key order for a config dict (`feat_dim`, `channels`, `emb_dim`, `global_context_att`,
    `n_layers`).  Convolution and linear weights N(0, 2 / fan_in) (activations keep their scale through the ReLUs), biases 0.05 N(0, 1),
    `linear.weight` a hundredth of that,
    BatchNorm weights and running variances uniform in [0.5, 1.5), BatchNorm biases and running means 0.1 N(0, 1), `feature_weight`
    N(0, 1), `num_batches_tracked` 1000: nothing is left at a value that would hide a wrong formula."""
    out = OrderedDict()
    for name, t in _module(cfg).state_dict().items():
        shape, g = tuple(t.shape), _rng(seed, name)
        leaf = name.rsplit(".", 1)[-1]
        is_bn = ".bn." in name or ".bns." in name or name.startswith("bn.")
        if leaf == "num_batches_tracked":
            out[name] = np.array(1000, dtype=np.int64)
            continue
        if name == "feature_weight":
            v = g.standard_normal(shape, dtype=np.float32)
        elif leaf == "running_var" or (is_bn and leaf == "weight"):
            v = 0.5 + g.random(shape, dtype=np.float32)
        elif leaf == "running_mean" or (is_bn and leaf == "bias"):
            v = 0.1 * g.standard_normal(shape, dtype=np.float32)
        elif leaf == "weight":
            gain = 0.01 if name == "linear.weight" else 1.0         # the residual stream grows block by block; a trained embedding is O(1)
            v = g.standard_normal(shape, dtype=np.float32) * np.float32(gain * np.sqrt(2.0 / np.prod(shape[1:])))
        elif leaf == "bias":
            v = 0.05 * g.standard_normal(shape, dtype=np.float32)
        else:
            raise KeyError(name)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def synthetic_speaker_embedder(emb_dim: int = 256, seed: int = 0) -> ECAPA_TDNN:
    """ECAPA_TDNN_SMALL(1024, emb_dim, "wavlm_large") -- what util.get_speaker_embedder builds -- with seeded weights, eval mode."""
    m = ECAPA_TDNN_SMALL(feat_dim=1024, emb_dim=emb_dim, feat_type="wavlm_large")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(m.config(), seed).items()})
    return m.eval()


def synthetic_hidden_states(L: int, B: int, T: int, C_: int, seed: int = 0) -> np.ndarray:
    """Seeded hidden states [L, B, T, C]: N(0, 1) drawn layer by layer, layer l scaled by (1 + 0.2 l) so the layer weights matter."""
    g = np.random.Generator(np.random.Philox(key=2000 + seed))
    x = np.empty((L, B, T, C_), dtype=np.float32)
    for l in range(L):
        x[l] = g.standard_normal((B, T, C_), dtype=np.float32) * np.float32(1.0 + 0.2 * l)
    return x
