"""WavLM encoder on the HIP library: the upstream of the speaker embedder (the reference's `ECAPA_TDNN_SMALL(feat_type="wavlm_large")`,
s3prl's `wavlm_large`): 16 kHz waveform -> every hidden state [B, F, H], one frame per 320 samples.

`WavLMModel` keeps its parameters under exactly the `state_dict` keys of `transformers.WavLMModel` for the same configuration, in that
order, so an HF checkpoint loads as it is; `from_fairseq_wavlm_state_dict` renames a fairseq / s3prl WavLM checkpoint's keys.  Both
published forms are built: the layer-norm extractor with conv biases and the pre-LN encoder (large), and the group-norm extractor with
post-LN layers (base, base-plus).  The arithmetic is `csrc/hubert.hip`; there is no CPU fallback and no training.
"""
from __future__ import annotations

import re

from ._wav_encoder import POS, _WaveformEncoder, rename_fairseq
from .hubert import from_fairseq_state_dict

_LARGE = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), hidden_size=1024, num_attention_heads=16,
              intermediate_size=4096, num_hidden_layers=24, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
              feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, num_buckets=320, max_bucket_distance=800)
_BASE_PLUS = dict(_LARGE, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12, feat_extract_norm="group",
                  do_stable_layer_norm=False, conv_bias=False)


class WavLMModel(_WaveformEncoder):
    """`forward(wav [B, T], lengths=None, output_layer=None, output_hidden_states=False, normalize=False, layers_first=False)` -> [B, F, H].

    The constructor takes the fields of transformers' `WavLMConfig` by keyword (others, such as the dropouts, are accepted and unused in
    eval mode); `WavLMModel.large()` and `.base_plus()` are the published sizes.  `lengths` are samples per item with `HubertModel`'s
    semantics: an item's rows are what the model gives for its own samples alone, rows past its frames are 0.  `output_layer` n gives HF's
    `hidden_states[n]` (in the pre-LN form the un-normalised input of layer n for n < L).  With `output_hidden_states` the result is
    `(out, hidden_states)`, [B, n + 1, F, H], or [n + 1, B, F, H] with `layers_first` (what `ECAPA_TDNN.forward_features` takes), written
    in that order by the library.  `normalize`: `F.layer_norm(wav, wav.shape)` per item over its own samples first (s3prl's wavlm_large)."""
    _abi, _what = "wavlm", "WavLM encoder"

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=_LARGE["conv_dim"],
                 conv_stride=_LARGE["conv_stride"], conv_kernel=_LARGE["conv_kernel"], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                 layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, num_buckets=320,
                 max_bucket_distance=800, hidden_act="gelu", feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0, **unused):
        large = feat_extract_norm == "layer" and bool(do_stable_layer_norm) and bool(conv_bias)
        base = feat_extract_norm == "group" and not do_stable_layer_norm and not conv_bias
        if not (large or base):
            raise ValueError("WavLMModel: (feat_extract_norm, do_stable_layer_norm, conv_bias) must be ('layer', True, True), WavLM-large's "
                             "form, or ('group', False, False), WavLM-base's")
        if hidden_act != "gelu" or feat_extract_activation != "gelu":
            raise ValueError("WavLMModel: GELU activations are what is built")
        super().__init__(dict(conv_dim=conv_dim, conv_kernel=conv_kernel, conv_stride=conv_stride, hidden_size=hidden_size,
                              num_attention_heads=num_attention_heads, intermediate_size=intermediate_size, num_hidden_layers=num_hidden_layers,
                              num_conv_pos_embeddings=num_conv_pos_embeddings, num_conv_pos_embedding_groups=num_conv_pos_embedding_groups,
                              layer_norm_eps=layer_norm_eps, feat_extract_norm=feat_extract_norm, do_stable_layer_norm=do_stable_layer_norm,
                              conv_bias=conv_bias, num_buckets=num_buckets, max_bucket_distance=max_bucket_distance),
                         masked_spec_embed=mask_time_prob > 0.0 or mask_feature_prob > 0.0)         # HF registers it under this condition

    @classmethod
    def large(cls, **overrides):
        """WavLM-large: microsoft/wavlm-large, s3prl's wavlm_large."""
        return cls(**dict(_LARGE, **overrides))

    @classmethod
    def base_plus(cls, **overrides):
        """WavLM-base and base-plus: microsoft/wavlm-base-plus."""
        return cls(**dict(_BASE_PLUS, **overrides))

    def _config_struct(self):
        c = self.config
        s = super()._config_struct()
        s.conv_bias, s.num_buckets, s.max_bucket_distance = int(c["conv_bias"]), c["num_buckets"], c["max_bucket_distance"]
        return s

    def _hidden_layout(self, B, n1, F, H, layers_first=False):
        """us_wavlm_forward takes the strides of an item and of a layer in the hidden states."""
        return ((n1, B, F, H), (F * H, B * F * H)) if layers_first else ((B, n1, F, H), (n1 * F * H, F * H))

    def forward(self, wav, lengths=None, output_layer=None, output_hidden_states=False, normalize=False, layers_first=False):
        return self._encode(wav, lengths, output_layer, output_hidden_states, normalize, layers_first=layers_first)


_FAIRSEQ_WAVLM = [
    (r"\.self_attn\.grep_linear\.", ".attention.gru_rel_pos_linear."),
    (r"\.self_attn\.grep_a$", ".attention.gru_rel_pos_const"),
    (r"\.self_attn\.relative_attention_bias\.", ".attention.rel_attn_embed."),
    (r"^feature_extractor\.conv_layers\.(\d+)\.2\.1\.", r"feature_extractor.conv_layers.\1.layer_norm."),
    (r"^feature_extractor\.conv_layers\.(\d+)\.2\.", r"feature_extractor.conv_layers.\1.layer_norm."),
]


def from_fairseq_wavlm_state_dict(sd):
    """A fairseq / s3prl WavLM checkpoint's `model` dictionary under `WavLMModel`'s (transformers') key names: the HuBERT renames, the
    gated relative position bias's (`grep_linear`, `grep_a`, `relative_attention_bias`), the extractor's conv bias, and its LayerNorm
    under either `conv_layers.N.2.{weight,bias}` or `conv_layers.N.2.1.{weight,bias}` (fairseq wraps it between two transposes).
    `mask_emb`, `label_embs_concat` and `final_proj.*` are dropped.  fairseq and s3prl are not available where this library is developed:
    the mapping is tested on a hand-made dictionary of the right names and shapes only."""
    return from_fairseq_state_dict(rename_fairseq(sd, _FAIRSEQ_WAVLM))


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
    v = sd.get(POS + "parametrizations.weight.original1", sd.get(POS + "weight_v"))
    emb = sd["encoder.layers.0.attention.rel_attn_embed.weight"]
    cfg = dict(conv_dim=[int(w.shape[0]) for w in conv], conv_kernel=[int(w.shape[2]) for w in conv],
               conv_stride=list(_LARGE["conv_stride"]) if n_conv == 7 else [1] * n_conv, hidden_size=H, num_attention_heads=H // d,
               intermediate_size=int(sd["encoder.layers.0.feed_forward.intermediate_dense.weight"].shape[0]), num_hidden_layers=n_layers,
               num_conv_pos_embeddings=int(v.shape[2]), num_conv_pos_embedding_groups=H // int(v.shape[1]), feat_extract_norm="layer" if layer_form else "group",
               do_stable_layer_norm=layer_form, conv_bias="feature_extractor.conv_layers.0.conv.bias" in sd, num_buckets=int(emb.shape[0]),
               max_bucket_distance=800)
    cfg.update(overrides)
    return cfg
