"""WavLM encoder on the HIP library: the upstream of the speaker embedder (the reference's `ECAPA_TDNN_SMALL(feat_type="wavlm_large")`,
s3prl's `wavlm_large`): 16 kHz waveform -> every hidden state [B, F, H], one frame per 320 samples.

`WavLMModel` keeps its parameters under exactly the `state_dict` keys of `transformers.WavLMModel` for the same configuration, in that
order, so an HF checkpoint loads as it is; `from_fairseq_wavlm_state_dict` renames a fairseq / s3prl WavLM checkpoint's keys.  Both
published forms are built: the layer-norm extractor with conv biases and the pre-LN encoder (large), and the group-norm extractor with
post-LN layers (base, base-plus).  The arithmetic is `csrc/hubert.hip`; there is no CPU fallback and no training.
"""
from __future__ import annotations

import ctypes as C
import re
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._handle import HandleModule
from .hubert import _FAIRSEQ, _POS, _set

_LARGE = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), hidden_size=1024, num_attention_heads=16,
              intermediate_size=4096, num_hidden_layers=24, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
              feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, num_buckets=320, max_bucket_distance=800)
_BASE_PLUS = dict(_LARGE, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, feat_extract_norm="group",
                  do_stable_layer_norm=False, conv_bias=False)


class WavLMModel(HandleModule):
    """`forward(wav [B, T], lengths=None, output_layer=None, output_hidden_states=False, normalize=False, layers_first=False)` -> [B, F, H].

    The constructor takes the fields of transformers' `WavLMConfig` by keyword (others, such as the dropouts, are accepted and unused in
    eval mode); `WavLMModel.large()` and `.base_plus()` are the published sizes.  `lengths` are samples per item with `HubertModel`'s
    semantics: an item's rows are what the model gives for its own samples alone, rows past its frames are 0.  `output_layer` n gives HF's
    `hidden_states[n]` (in the pre-LN form the un-normalised input of layer n for n < L).  With `output_hidden_states` the result is
    `(out, hidden_states)`, [B, n + 1, F, H], or [n + 1, B, F, H] with `layers_first` (what `ECAPA_TDNN.forward_features` takes), written
    in that order by the library.  `normalize`: `F.layer_norm(wav, wav.shape)` per item over its own samples first (s3prl's wavlm_large)."""
    _abi, _what = "wavlm", "WavLM encoder"
    _cache_sources = True

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=_LARGE["conv_dim"],
                 conv_stride=_LARGE["conv_stride"], conv_kernel=_LARGE["conv_kernel"], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                 layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, num_buckets=320,
                 max_bucket_distance=800, hidden_act="gelu", feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0, **unused):
        super().__init__()
        large = feat_extract_norm == "layer" and bool(do_stable_layer_norm) and bool(conv_bias)
        base = feat_extract_norm == "group" and not do_stable_layer_norm and not conv_bias
        if not (large or base):
            raise ValueError("WavLMModel: (feat_extract_norm, do_stable_layer_norm, conv_bias) must be ('layer', True, True), WavLM-large's "
                             "form, or ('group', False, False), WavLM-base's")
        if hidden_act != "gelu" or feat_extract_activation != "gelu":
            raise ValueError("WavLMModel: GELU activations are what is built")
        if not (len(conv_dim) == len(conv_kernel) == len(conv_stride)) or not 1 <= len(conv_dim) <= _lib.US_HUBERT_MAX_CONV:
            raise ValueError(f"WavLMModel: conv_dim, conv_kernel and conv_stride need the same length, at most {_lib.US_HUBERT_MAX_CONV}")
        self.config = dict(conv_dim=[int(v) for v in conv_dim], conv_kernel=[int(v) for v in conv_kernel], conv_stride=[int(v) for v in conv_stride],
                           hidden_size=int(hidden_size), num_attention_heads=int(num_attention_heads), intermediate_size=int(intermediate_size),
                           num_hidden_layers=int(num_hidden_layers), num_conv_pos_embeddings=int(num_conv_pos_embeddings),
                           num_conv_pos_embedding_groups=int(num_conv_pos_embedding_groups), layer_norm_eps=float(layer_norm_eps),
                           feat_extract_norm=str(feat_extract_norm), do_stable_layer_norm=bool(do_stable_layer_norm), conv_bias=bool(conv_bias),
                           num_buckets=int(num_buckets), max_bucket_distance=int(max_bucket_distance))
        c = self.config
        H, I, nh = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"]
        if H % nh or H % c["num_conv_pos_embedding_groups"]:
            raise ValueError("WavLMModel: hidden_size must be divisible by the heads and by the positional convolution's groups")

        def affine(p, n):
            _set(self, p + ".weight", torch.ones(n))
            _set(self, p + ".bias", torch.zeros(n))

        def linear(p, o, i):
            _set(self, p + ".weight", torch.zeros(o, i))
            _set(self, p + ".bias", torch.zeros(o))

        if mask_time_prob > 0.0 or mask_feature_prob > 0.0:             # HF registers it under this condition; unused in eval
            _set(self, "masked_spec_embed", torch.zeros(H))
        cin = 1
        for i, (ch, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
            p = f"feature_extractor.conv_layers.{i}."
            _set(self, p + "conv.weight", torch.zeros(ch, cin, k))
            if large:
                _set(self, p + "conv.bias", torch.zeros(ch))
            if large or i == 0:
                affine(p + "layer_norm", ch)
            cin = ch
        affine("feature_projection.layer_norm", cin)
        linear("feature_projection.projection", H, cin)
        kp, g = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        _set(self, _POS + "bias", torch.zeros(H))
        _set(self, _POS + "parametrizations.weight.original0", torch.ones(1, 1, kp))
        _set(self, _POS + "parametrizations.weight.original1", torch.ones(H, H // g, kp))
        affine("encoder.layer_norm", H)
        for i in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            _set(self, p + "attention.gru_rel_pos_const", torch.ones(1, nh, 1, 1))
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                linear(p + "attention." + n, H, H)
            linear(p + "attention.gru_rel_pos_linear", 8, H // nh)
            if i == 0:
                _set(self, p + "attention.rel_attn_embed.weight", torch.zeros(c["num_buckets"], nh))
            affine(p + "layer_norm", H)
            linear(p + "feed_forward.intermediate_dense", I, H)
            linear(p + "feed_forward.output_dense", H, I)
            affine(p + "final_layer_norm", H)

    @classmethod
    def large(cls, **overrides):
        """WavLM-large: microsoft/wavlm-large, s3prl's wavlm_large."""
        return cls(**dict(_LARGE, **overrides))

    @classmethod
    def base_plus(cls, **overrides):
        """WavLM-base and base-plus: microsoft/wavlm-base-plus."""
        return cls(**dict(_BASE_PLUS, **overrides))

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------

    def load_state_dict(self, state_dict, strict=True, **kw):
        """HF's keys; also the older `...conv.weight_g` / `weight_v` spelling of the positional convolution; a checkpoint without
        `masked_spec_embed` keeps the module's."""
        sd = OrderedDict()
        for k, v in state_dict.items():
            if k == _POS + "weight_g":
                k = _POS + "parametrizations.weight.original0"
            elif k == _POS + "weight_v":
                k = _POS + "parametrizations.weight.original1"
            sd[k] = v
        if hasattr(self, "masked_spec_embed"):
            sd.setdefault("masked_spec_embed", self.masked_spec_embed.detach())
        else:
            sd.pop("masked_spec_embed", None)
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- engine ----------------------------------------------------------------------------------------------------------------

    def _config_struct(self):
        c = self.config
        s = _lib.us_wavlm_config()
        s.n_conv = len(c["conv_dim"])
        for i in range(s.n_conv):
            s.conv_dim[i], s.conv_kernel[i], s.conv_stride[i] = c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i]
        s.hidden_size, s.n_heads, s.intermediate_size, s.n_layers = (c["hidden_size"], c["num_attention_heads"], c["intermediate_size"],
                                                                     c["num_hidden_layers"])
        s.pos_conv_kernel, s.pos_conv_groups = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        s.feat_extract_norm = _lib.US_HUBERT_NORM_LAYER if c["feat_extract_norm"] == "layer" else _lib.US_HUBERT_NORM_GROUP
        s.do_stable_layer_norm, s.layer_norm_eps, s.conv_bias = int(c["do_stable_layer_norm"]), c["layer_norm_eps"], int(c["conv_bias"])
        s.num_buckets, s.max_bucket_distance = c["num_buckets"], c["max_bucket_distance"]
        return s

    def _create(self, lib, device):
        s = self._config_struct()
        _lib.check(lib.us_wavlm_create(C.byref(self._h), C.byref(s)), None, "us_wavlm_create")

    def _sources(self):
        """Every parameter under its own key, except masked_spec_embed (unused in eval) and the positional convolution's weight-norm pair,
        which goes in folded: weight = g * v / |v|, the norm over dims 0 and 1 (torch's `_weight_norm(v, g, dim=2)`)."""
        out = OrderedDict()
        sd = self.state_dict(keep_vars=True)
        for k, t in sd.items():
            if k == "masked_spec_embed" or k.startswith(_POS + "parametrizations."):
                continue
            out[k] = ((t,), None)
        g, v = sd[_POS + "parametrizations.weight.original0"], sd[_POS + "parametrizations.weight.original1"]
        out[_POS + "weight"] = ((g, v), lambda: torch._weight_norm(v.detach().float(), g.detach().float(), 2))
        return out

    def _precondition(self):
        if self.training:
            raise RuntimeError("WavLMModel is inference-only (dropout, time masking and the backward pass are not built): call .eval()")

    def frames(self, n: int) -> int:
        """Frames of an n-sample item (0: shorter than the receptive field)."""
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            n = (n - k) // s + 1 if n >= k else 0
        return n

    @torch.no_grad()
    def forward(self, wav, lengths=None, output_layer=None, output_hidden_states=False, normalize=False, layers_first=False):
        if wav.dim() != 2 or wav.shape[0] < 1:
            raise ValueError(f"WavLMModel: expected a waveform [B, T], got {tuple(wav.shape)}")
        device = wav.device
        lib, stream = self._sync(device)
        x = wav.detach().to(dtype=torch.float32).contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        L = self.config["num_hidden_layers"]
        n = L if output_layer is None else int(output_layer)
        lens = None
        if lengths is not None:
            v = [int(i) for i in (lengths.reshape(-1).tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
            if len(v) != B:
                raise ValueError(f"WavLMModel: {len(v)} lengths for {B} waveforms")
            lens = (C.c_int64 * B)(*v)
        F, H = self.frames(T), self.config["hidden_size"]
        if F < 1:                                # the library's own refusal, with its message
            self._check(lib, min(int(lib.us_wavlm_frames(self._h, T)), -1), "us_wavlm_frames")
        out = torch.empty(B, F, H, device=device)
        hs, n1 = None, max(n, 0) + 1
        if output_hidden_states:
            hs = torch.empty((n1, B, F, H) if layers_first else (B, n1, F, H), device=device)
        item, layer = (F * H, B * F * H) if layers_first else (n1 * F * H, F * H)
        ws = self._workspace(lib, device, B, T)
        with torch.cuda.device(device):
            rc = lib.us_wavlm_forward(self._h, x.data_ptr(), lens, B, T, int(bool(normalize)), n, out.data_ptr(),
                                      hs.data_ptr() if hs is not None else None, item, layer, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, "us_wavlm_forward")
        return (out, hs) if output_hidden_states else out


_FAIRSEQ_WAVLM = [
    (r"\.self_attn\.grep_linear\.", ".attention.gru_rel_pos_linear."),
    (r"\.self_attn\.grep_a$", ".attention.gru_rel_pos_const"),
    (r"\.self_attn\.relative_attention_bias\.", ".attention.rel_attn_embed."),
    (r"^feature_extractor\.conv_layers\.(\d+)\.2\.1\.", r"feature_extractor.conv_layers.\1.layer_norm."),
    (r"^feature_extractor\.conv_layers\.(\d+)\.2\.", r"feature_extractor.conv_layers.\1.layer_norm."),
] + _FAIRSEQ


def from_fairseq_wavlm_state_dict(sd):
    """A fairseq / s3prl WavLM checkpoint's `model` dictionary under `WavLMModel`'s (transformers') key names: the HuBERT renames, the
    gated relative position bias's (`grep_linear`, `grep_a`, `relative_attention_bias`), the extractor's conv bias, and its LayerNorm
    under either `conv_layers.N.2.{weight,bias}` or `conv_layers.N.2.1.{weight,bias}` (fairseq wraps it between two transposes).
    `mask_emb`, `label_embs_concat` and `final_proj.*` are dropped.  fairseq and s3prl are not available where this library is developed:
    the mapping is tested on a hand-made dictionary of the right names and shapes only."""
    out = OrderedDict()
    for k, v in sd.items():
        if k in ("mask_emb", "label_embs_concat") or k.startswith("final_proj."):
            continue
        for pat, rep in _FAIRSEQ_WAVLM:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out


def wavlm_config_from_state_dict(sd, **overrides):
    """`WavLMModel`'s constructor arguments read from the shapes of a state_dict under HF's names.  The extractor's strides are not in
    the shapes and are the published ones for seven layers; the norm form is inferred from the presence of a LayerNorm in extractor
    layer 1, and pre-LN goes with it, as in every published WavLM.  Keywords override."""
    n_conv = 1 + max(int(m.group(1)) for m in (re.match(r"feature_extractor\.conv_layers\.(\d+)\.conv\.weight$", k) for k in sd) if m)
    n_layers = 1 + max(int(m.group(1)) for m in (re.match(r"encoder\.layers\.(\d+)\.", k) for k in sd) if m)
    conv = [sd[f"feature_extractor.conv_layers.{i}.conv.weight"] for i in range(n_conv)]
    layer_form = "feature_extractor.conv_layers.1.layer_norm.weight" in sd
    H = int(sd["feature_projection.projection.weight"].shape[0])
    d = int(sd["encoder.layers.0.attention.gru_rel_pos_linear.weight"].shape[1])
    v = sd.get(_POS + "parametrizations.weight.original1", sd.get(_POS + "weight_v"))
    emb = sd["encoder.layers.0.attention.rel_attn_embed.weight"]
    cfg = dict(conv_dim=[int(w.shape[0]) for w in conv], conv_kernel=[int(w.shape[2]) for w in conv],
               conv_stride=list(_LARGE["conv_stride"]) if n_conv == 7 else [1] * n_conv, hidden_size=H, num_attention_heads=H // d,
               intermediate_size=int(sd["encoder.layers.0.feed_forward.intermediate_dense.weight"].shape[0]), num_hidden_layers=n_layers,
               num_conv_pos_embeddings=int(v.shape[2]), num_conv_pos_embedding_groups=H // int(v.shape[1]), feat_extract_norm="layer" if layer_form else "group",
               do_stable_layer_norm=layer_form, conv_bias="feature_extractor.conv_layers.0.conv.bias" in sd, num_buckets=int(emb.shape[0]),
               max_bucket_distance=800)
    cfg.update(overrides)
    return cfg
