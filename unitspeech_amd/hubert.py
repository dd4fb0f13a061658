"""HuBERT encoder on the HIP library: the dense model in front of the unit quantiser (the reference's textless
`HubertFeatureReader`, fairseq's `extract_features(output_layer=L)`) and its ContentVec extractor (`transformers.HubertModel`,
scripts/voice_conversion.py:46-68): 16 kHz waveform -> [B, F, H] features, one frame per 320 samples.

`HubertModel` keeps its parameters under exactly the `state_dict` keys of `transformers.HubertModel` for the same configuration (group-norm
extractor, post-LN layers), so an HF checkpoint loads as it is; `from_fairseq_state_dict` renames a fairseq HuBERT checkpoint's keys.  The
arithmetic is `csrc/hubert.hip`; there is no CPU fallback and no training.
"""
from __future__ import annotations

import ctypes as C
import re
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._handle import HandleModule

_BASE = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), hidden_size=768, num_attention_heads=12,
             intermediate_size=3072, num_hidden_layers=12, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)
_POS = "encoder.pos_conv_embed.conv."


def _set(root, key, tensor):
    """Register `tensor` as a parameter under the dotted `key`, making plain container modules on the way."""
    *path, leaf = key.split(".")
    m = root
    for p in path:
        if p not in m._modules:
            m.add_module(p, torch.nn.Module())
        m = m._modules[p]
    m.register_parameter(leaf, torch.nn.Parameter(tensor, requires_grad=False))


class HubertModel(HandleModule):
    """`forward(wav [B, T], lengths=None, output_layer=None, output_hidden_states=False)` -> [B, F, H] on wav's device.

    The constructor takes the fields of transformers' `HubertConfig` by keyword (others, such as the dropouts, are accepted and unused in
    eval mode); `HubertModel.base()` is HuBERT-base.  `lengths` are samples per item: an item's rows are what the model gives for its own
    samples alone (not HF's attention_mask behaviour), rows past its frames are 0.  `output_layer` n stops after n layers (HF's
    `hidden_states[n]`, fairseq's `output_layer`); with `output_hidden_states` the result is `(out, hidden_states [B, n + 1, F, H])`."""
    _abi, _what = "hubert", "HuBERT encoder"
    _cache_sources = True

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=_BASE["conv_dim"],
                 conv_stride=_BASE["conv_stride"], conv_kernel=_BASE["conv_kernel"], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                 layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, feat_proj_layer_norm=True,
                 hidden_act="gelu", feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0, **unused):
        super().__init__()
        if feat_extract_norm != "group":
            raise ValueError("HubertModel: only the group-norm feature extractor (feat_extract_norm='group') is built")
        if do_stable_layer_norm:
            raise ValueError("HubertModel: the pre-LN encoder (do_stable_layer_norm=True) is not built")
        if conv_bias or not feat_proj_layer_norm or hidden_act != "gelu" or feat_extract_activation != "gelu":
            raise ValueError("HubertModel: conv_bias=False, feat_proj_layer_norm=True and GELU activations are what is built")
        if not (len(conv_dim) == len(conv_kernel) == len(conv_stride)) or not 1 <= len(conv_dim) <= _lib.US_HUBERT_MAX_CONV:
            raise ValueError(f"HubertModel: conv_dim, conv_kernel and conv_stride need the same length, at most {_lib.US_HUBERT_MAX_CONV}")
        self.config = dict(conv_dim=[int(v) for v in conv_dim], conv_kernel=[int(v) for v in conv_kernel], conv_stride=[int(v) for v in conv_stride],
                           hidden_size=int(hidden_size), num_attention_heads=int(num_attention_heads), intermediate_size=int(intermediate_size),
                           num_hidden_layers=int(num_hidden_layers), num_conv_pos_embeddings=int(num_conv_pos_embeddings),
                           num_conv_pos_embedding_groups=int(num_conv_pos_embedding_groups), layer_norm_eps=float(layer_norm_eps))
        c = self.config
        H, I = c["hidden_size"], c["intermediate_size"]
        if H % c["num_attention_heads"] or H % c["num_conv_pos_embedding_groups"]:
            raise ValueError("HubertModel: hidden_size must be divisible by the heads and by the positional convolution's groups")

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
            _set(self, f"feature_extractor.conv_layers.{i}.conv.weight", torch.zeros(ch, cin, k))
            if i == 0:
                affine("feature_extractor.conv_layers.0.layer_norm", ch)
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
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                linear(p + "attention." + n, H, H)
            affine(p + "layer_norm", H)
            linear(p + "feed_forward.intermediate_dense", I, H)
            linear(p + "feed_forward.output_dense", H, I)
            affine(p + "final_layer_norm", H)

    @classmethod
    def base(cls, **overrides):
        """HuBERT-base: facebook/hubert-base-ls960, mHuBERT, ContentVec."""
        return cls(**dict(_BASE, **overrides))

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------

    def load_state_dict(self, state_dict, strict=True, **kw):
        """HF's keys; also the older `...conv.weight_g` / `weight_v` spelling of the positional convolution (how content-vec-best is stored);
        `final_proj.*` (HubertModelWithFinalProj) is ignored, and a checkpoint without `masked_spec_embed` keeps the module's."""
        sd = OrderedDict()
        for k, v in state_dict.items():
            if k.startswith("final_proj."):
                continue
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
        s = _lib.us_hubert_config()
        s.n_conv = len(c["conv_dim"])
        for i in range(s.n_conv):
            s.conv_dim[i], s.conv_kernel[i], s.conv_stride[i] = c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i]
        s.hidden_size, s.n_heads, s.intermediate_size, s.n_layers = (c["hidden_size"], c["num_attention_heads"], c["intermediate_size"],
                                                                     c["num_hidden_layers"])
        s.pos_conv_kernel, s.pos_conv_groups = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        s.feat_extract_norm, s.do_stable_layer_norm, s.layer_norm_eps = _lib.US_HUBERT_NORM_GROUP, 0, c["layer_norm_eps"]
        return s

    def _create(self, lib, device):
        s = self._config_struct()
        _lib.check(lib.us_hubert_create(C.byref(self._h), C.byref(s)), None, "us_hubert_create")

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
            raise RuntimeError("HubertModel is inference-only (dropout, time masking and the backward pass are not built): call .eval()")

    def frames(self, n: int) -> int:
        """Frames of an n-sample item (0: shorter than the receptive field)."""
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            n = (n - k) // s + 1 if n >= k else 0
        return n

    @torch.no_grad()
    def forward(self, wav, lengths=None, output_layer=None, output_hidden_states=False, normalize=False):
        if wav.dim() != 2 or wav.shape[0] < 1:
            raise ValueError(f"HubertModel: expected a waveform [B, T], got {tuple(wav.shape)}")
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
                raise ValueError(f"HubertModel: {len(v)} lengths for {B} waveforms")
            lens = (C.c_int64 * B)(*v)
        F, H = self.frames(T), self.config["hidden_size"]
        if F < 1:                                # the library's own refusal, with its message
            self._check(lib, min(int(lib.us_hubert_frames(self._h, T)), -1), "us_hubert_frames")
        out = torch.empty(B, F, H, device=device)
        hs = torch.empty(B, max(n, 0) + 1, F, H, device=device) if output_hidden_states else None
        ws = self._workspace(lib, device, B, T)
        with torch.cuda.device(device):
            rc = lib.us_hubert_forward(self._h, x.data_ptr(), lens, B, T, int(bool(normalize)), n, out.data_ptr(),
                                       hs.data_ptr() if hs is not None else None, ws.data_ptr(), ws.numel(), stream)
        self._check(lib, rc, "us_hubert_forward")
        return (out, hs) if output_hidden_states else out


class HubertFeatureReader(torch.nn.Module):
    """Drop-in for textless' `HubertFeatureReader` around a `HubertModel`: `forward(x [T])` -> [T', D] features of layer `layer`, chunked at
    `max_chunk` samples as the reference does (hubert_feature_reader.py:66-76).  The result stays on the device, so `units.SpeechEncoder`
    quantises it without a host round trip.  `normalize` is the fairseq task's flag (`F.layer_norm(x, x.shape)` over the whole input)."""

    def __init__(self, model: HubertModel, layer=6, max_chunk=100 * 16_000, normalize=False):
        super().__init__()
        self.model = model.eval()
        self.layer = int(layer)
        self.max_chunk = int(max_chunk)
        self.should_normalize = bool(normalize)
        self.register_buffer("_float_tensor", torch.tensor([0], dtype=torch.float))

    @property
    def device(self):
        return self._float_tensor.device

    @property
    def code_hop_size(self) -> int:
        return 320

    @property
    def expected_sample_rate(self) -> int:
        return 16_000

    def forward(self, x):
        return self.get_features(x)

    @torch.no_grad()
    def get_features(self, x):
        x = x.to(self.device).reshape(1, -1)
        single = x.shape[1] <= self.max_chunk
        if self.should_normalize and not single:           # over the whole input, before it is cut: the chunks share one mean and variance
            x = torch.nn.functional.layer_norm(x, x.shape)
        feat = [self.model(x[:, s:s + self.max_chunk], output_layer=self.layer, normalize=self.should_normalize and single)
                for s in range(0, x.shape[1], self.max_chunk)]
        return feat[0][0] if single else torch.cat(feat, 1)[0]


_FAIRSEQ = [
    (r"^feature_extractor\.conv_layers\.(\d+)\.0\.", r"feature_extractor.conv_layers.\1.conv."),
    (r"^feature_extractor\.conv_layers\.0\.2\.", "feature_extractor.conv_layers.0.layer_norm."),
    (r"^layer_norm\.", "feature_projection.layer_norm."),
    (r"^post_extract_proj\.", "feature_projection.projection."),
    (r"^encoder\.pos_conv\.0\.", "encoder.pos_conv_embed.conv."),
    (r"\.self_attn_layer_norm\.", ".layer_norm."),
    (r"\.self_attn\.", ".attention."),
    (r"\.fc1\.", ".feed_forward.intermediate_dense."),
    (r"\.fc2\.", ".feed_forward.output_dense."),
]


def from_fairseq_state_dict(sd):
    """A fairseq HuBERT checkpoint's `model` dictionary under `HubertModel`'s (transformers') key names.  `mask_emb`, `label_embs_concat`
    and `final_proj.*` (masking and the pre-training heads, unused in eval) are dropped.  fairseq is not available where this library is
    developed: the mapping is tested on a hand-made dictionary of the right names and shapes only."""
    out = OrderedDict()
    for k, v in sd.items():
        if k in ("mask_emb", "label_embs_concat") or k.startswith("final_proj."):
            continue
        for pat, rep in _FAIRSEQ:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out


def load_hubert_checkpoint(path, **config):
    """(`HubertModel` in eval mode, the reader's normalize flag) from a checkpoint file: a `transformers` state_dict (as `torch.save`d; a
    `hubert.` prefix is dropped), or fairseq's `{"model": ..., "cfg": ...}` (its task's `normalize` is the flag).  The configuration is
    HuBERT-base unless fields are given."""
    ck = torch.load(path, map_location="cpu")
    normalize = False
    if isinstance(ck, dict) and "model" in ck and isinstance(ck["model"], dict):
        cfg = ck.get("cfg") or {}
        task = cfg.get("task") if isinstance(cfg, dict) else getattr(cfg, "task", None)
        normalize = bool((task.get("normalize", False) if isinstance(task, dict) else getattr(task, "normalize", False)) if task is not None else False)
        sd = from_fairseq_state_dict(ck["model"])
    else:
        sd = OrderedDict((k[len("hubert."):] if k.startswith("hubert.") else k, v) for k, v in ck.items())
    model = HubertModel.base(**config)
    model.load_state_dict(sd)
    return model.eval(), normalize
