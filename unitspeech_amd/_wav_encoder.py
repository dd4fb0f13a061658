"""What `hubert.HubertModel` and `wavlm.WavLMModel` share: one wav2vec2-family encoder over `csrc/hubert.hip`, 16 kHz waveform -> [B, F, H].

`_WaveformEncoder` is driven by the model's configuration, as `hubert_keys` in `csrc/hubert.hip` is: the parameters it registers (and so
the `state_dict` keys, shapes and order of `transformers`), the library's config struct, the weights it hands over and the forward up to
the library call.  A subclass brings its constructor, the forms it refuses, the fields of its own config struct and the layout of the
hidden states it returns.
"""
from __future__ import annotations

import ctypes as C
import re
from collections import OrderedDict

import torch

from . import _lib
from ._args import c_lengths, host_lengths
from ._handle import HandleModule

POS = "encoder.pos_conv_embed.conv."
_FIELDS = dict(conv_dim=lambda v: [int(i) for i in v], conv_kernel=lambda v: [int(i) for i in v], conv_stride=lambda v: [int(i) for i in v],
               hidden_size=int, num_attention_heads=int, intermediate_size=int, num_hidden_layers=int, num_conv_pos_embeddings=int,
               num_conv_pos_embedding_groups=int, layer_norm_eps=float, feat_extract_norm=str, do_stable_layer_norm=bool, conv_bias=bool,
               num_buckets=int, max_bucket_distance=int)


def _set(root, key, tensor):
    """Register `tensor` as a parameter under the dotted `key`, making plain container modules on the way."""
    *path, leaf = key.split(".")
    m = root
    for p in path:
        if p not in m._modules:
            m.add_module(p, torch.nn.Module())
        m = m._modules[p]
    m.register_parameter(leaf, torch.nn.Parameter(tensor, requires_grad=False))


def _register(root, c, masked_spec_embed):
    """The parameters of configuration `c` under transformers' keys and in its order (`hubert_keys` in csrc/hubert.hip walks the same
    way): a conv bias with `conv_bias`, a LayerNorm in every extractor layer of the layer-norm form and in layer 0 only otherwise, the
    gated relative position bias when the configuration has buckets."""
    H, I, nh = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"]
    layer_form, rel_pos = c.get("feat_extract_norm") == "layer", "num_buckets" in c

    def affine(p, n):
        _set(root, p + ".weight", torch.ones(n))
        _set(root, p + ".bias", torch.zeros(n))

    def linear(p, o, i):
        _set(root, p + ".weight", torch.zeros(o, i))
        _set(root, p + ".bias", torch.zeros(o))

    if masked_spec_embed:                                               # unused in eval
        _set(root, "masked_spec_embed", torch.zeros(H))
    cin = 1
    for i, (ch, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}."
        _set(root, p + "conv.weight", torch.zeros(ch, cin, k))
        if c.get("conv_bias"):
            _set(root, p + "conv.bias", torch.zeros(ch))
        if layer_form or i == 0:
            affine(p + "layer_norm", ch)
        cin = ch
    affine("feature_projection.layer_norm", cin)
    linear("feature_projection.projection", H, cin)
    kp, g = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    _set(root, POS + "bias", torch.zeros(H))
    _set(root, POS + "parametrizations.weight.original0", torch.ones(1, 1, kp))
    _set(root, POS + "parametrizations.weight.original1", torch.ones(H, H // g, kp))
    affine("encoder.layer_norm", H)
    for i in range(c["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        if rel_pos:
            _set(root, p + "attention.gru_rel_pos_const", torch.ones(1, nh, 1, 1))
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            linear(p + "attention." + n, H, H)
        if rel_pos:
            linear(p + "attention.gru_rel_pos_linear", 8, H // nh)
            if i == 0:
                _set(root, p + "attention.rel_attn_embed.weight", torch.zeros(c["num_buckets"], nh))
        affine(p + "layer_norm", H)
        linear(p + "feed_forward.intermediate_dense", I, H)
        linear(p + "feed_forward.output_dense", H, I)
        affine(p + "final_layer_norm", H)


class _WaveformEncoder(HandleModule):
    """`__init__(config, masked_spec_embed)`: `config` holds transformers' fields by name and becomes `self.config`, each value in its own
    type; `masked_spec_embed`: register that parameter (HF does when a masking probability is positive)."""
    _cache_sources = True
    _ignored_prefixes = ()     # state_dict keys `load_state_dict` leaves out

    def __init__(self, config, masked_spec_embed):
        super().__init__()
        name = type(self).__name__
        n_conv = len(config["conv_dim"])
        if not (n_conv == len(config["conv_kernel"]) == len(config["conv_stride"])) or not 1 <= n_conv <= _lib.US_HUBERT_MAX_CONV:
            raise ValueError(f"{name}: conv_dim, conv_kernel and conv_stride need the same length, at most {_lib.US_HUBERT_MAX_CONV}")
        self.config = c = {k: _FIELDS[k](v) for k, v in config.items()}
        if c["hidden_size"] % c["num_attention_heads"] or c["hidden_size"] % c["num_conv_pos_embedding_groups"]:
            raise ValueError(f"{name}: hidden_size must be divisible by the heads and by the positional convolution's groups")
        _register(self, c, masked_spec_embed)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------

    def load_state_dict(self, state_dict, strict=True, **kw):
        """HF's keys; also the older `...conv.weight_g` / `weight_v` spelling of the positional convolution (how content-vec-best is
        stored); keys under `_ignored_prefixes` are left out, and a checkpoint without `masked_spec_embed` keeps the module's."""
        old = {POS + "weight_g": POS + "parametrizations.weight.original0", POS + "weight_v": POS + "parametrizations.weight.original1"}
        sd = OrderedDict((old.get(k, k), v) for k, v in state_dict.items() if not k.startswith(self._ignored_prefixes))
        if hasattr(self, "masked_spec_embed"):
            sd.setdefault("masked_spec_embed", self.masked_spec_embed.detach())
        else:
            sd.pop("masked_spec_embed", None)
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- engine ----------------------------------------------------------------------------------------------------------------

    def _config_struct(self):
        """The library's config struct of this model (`us_{_abi}_config`) with the fields of `us_hubert_config` filled in."""
        c = self.config
        s = getattr(_lib, f"us_{self._abi}_config")()
        s.n_conv = len(c["conv_dim"])
        for i in range(s.n_conv):
            s.conv_dim[i], s.conv_kernel[i], s.conv_stride[i] = c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i]
        s.hidden_size, s.n_heads, s.intermediate_size, s.n_layers = (c["hidden_size"], c["num_attention_heads"], c["intermediate_size"],
                                                                     c["num_hidden_layers"])
        s.pos_conv_kernel, s.pos_conv_groups = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        s.feat_extract_norm = _lib.US_HUBERT_NORM_LAYER if c.get("feat_extract_norm") == "layer" else _lib.US_HUBERT_NORM_GROUP
        s.do_stable_layer_norm, s.layer_norm_eps = int(c.get("do_stable_layer_norm", False)), c["layer_norm_eps"]
        return s

    def _create(self, lib, device):
        s = self._config_struct()
        _lib.check(self._fn(lib, "create")(C.byref(self._h), C.byref(s)), None, f"us_{self._abi}_create")

    def _sources(self):
        """Every parameter under its own key, except masked_spec_embed (unused in eval) and the positional convolution's weight-norm pair,
        which goes in folded: weight = g * v / |v|, the norm over dims 0 and 1 (torch's `_weight_norm(v, g, dim=2)`)."""
        out = OrderedDict()
        sd = self.state_dict(keep_vars=True)
        for k, t in sd.items():
            if k == "masked_spec_embed" or k.startswith(POS + "parametrizations."):
                continue
            out[k] = ((t,), None)
        g, v = sd[POS + "parametrizations.weight.original0"], sd[POS + "parametrizations.weight.original1"]
        out[POS + "weight"] = ((g, v), lambda: torch._weight_norm(v.detach().float(), g.detach().float(), 2))
        return out

    def _precondition(self):
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only (dropout, time masking and the backward pass are not built): call .eval()")

    def frames(self, n: int) -> int:
        """Frames of an n-sample item (0: shorter than the receptive field)."""
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            n = (n - k) // s + 1 if n >= k else 0
        return n

    def _hidden_layout(self, B, n1, F, H):
        """-> (the shape of the hidden states of a batch, the arguments of `us_{_abi}_forward` that describe it)."""
        raise NotImplementedError

    @torch.no_grad()
    def _encode(self, wav, lengths, output_layer, output_hidden_states, normalize, **layout):
        """The forward of both models; `layout` goes to `_hidden_layout`."""
        name = type(self).__name__
        if wav.dim() != 2 or wav.shape[0] < 1:
            raise ValueError(f"{name}: expected a waveform [B, T], got {tuple(wav.shape)}")
        device = wav.device
        lib, stream = self._sync(device)
        x = wav.detach().to(dtype=torch.float32).contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        n = self.config["num_hidden_layers"] if output_layer is None else int(output_layer)
        lens = c_lengths(host_lengths(lengths, B, name))
        F, H = self.frames(T), self.config["hidden_size"]
        if F < 1:                                # the library's own refusal, with its message
            self._check(lib, min(int(self._fn(lib, "frames")(self._h, T)), -1), f"us_{self._abi}_frames")
        out = torch.empty(B, F, H, device=device)
        shape, extra = self._hidden_layout(B, max(n, 0) + 1, F, H, **layout)
        hs = torch.empty(shape, device=device) if output_hidden_states else None
        ws = self._workspace(lib, device, B, T)
        self._call(lib, device, "forward", self._h, x.data_ptr(), lens, B, T, int(bool(normalize)), n, out.data_ptr(),
                   hs.data_ptr() if hs is not None else None, *extra, ws.data_ptr(), ws.numel(), stream)
        return (out, hs) if output_hidden_states else out


def rename_fairseq(sd, table):
    """A fairseq checkpoint's `model` dictionary with every (pattern, replacement) of `table` applied to its keys in turn.  `mask_emb`,
    `label_embs_concat` and `final_proj.*` (masking and the pre-training heads, unused in eval) are dropped."""
    out = OrderedDict()
    for k, v in sd.items():
        if k in ("mask_emb", "label_embs_concat") or k.startswith("final_proj."):
            continue
        for pat, rep in table:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out
