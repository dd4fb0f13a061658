"""HuBERT encoder on the HIP library: the dense model in front of the unit quantiser (the reference's textless
`HubertFeatureReader`, fairseq's `extract_features(output_layer=L)`) and its ContentVec extractor (`transformers.HubertModel`,
scripts/voice_conversion.py:46-68): 16 kHz waveform -> [B, F, H] features, one frame per 320 samples.

`HubertModel` keeps its parameters under exactly the `state_dict` keys of `transformers.HubertModel` for the same configuration (group-norm
extractor, post-LN layers), so an HF checkpoint loads as it is; `from_fairseq_state_dict` renames a fairseq HuBERT checkpoint's keys.  The
arithmetic is `csrc/hubert.hip`; there is no CPU fallback and no training.
"""
from __future__ import annotations

import re
from collections import OrderedDict

import torch

from ._wav_encoder import _WaveformEncoder, rename_fairseq

_BASE = dict(conv_dim=(512,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), hidden_size=768, num_attention_heads=12,
             intermediate_size=3072, num_hidden_layers=12, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5)


class HubertModel(_WaveformEncoder):
    """`forward(wav [B, T], lengths=None, output_layer=None, output_hidden_states=False)` -> [B, F, H] on wav's device.

    The constructor takes the fields of transformers' `HubertConfig` by keyword (others, such as the dropouts, are accepted and unused in
    eval mode); `HubertModel.base()` is HuBERT-base.  `lengths` are samples per item: an item's rows are what the model gives for its own
    samples alone (not HF's attention_mask behaviour), rows past its frames are 0.  `output_layer` n stops after n layers (HF's
    `hidden_states[n]`, fairseq's `output_layer`); with `output_hidden_states` the result is `(out, hidden_states [B, n + 1, F, H])`."""
    _abi, _what = "hubert", "HuBERT encoder"
    _ignored_prefixes = ("final_proj.",)           # HubertModelWithFinalProj's head

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=_BASE["conv_dim"],
                 conv_stride=_BASE["conv_stride"], conv_kernel=_BASE["conv_kernel"], num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                 layer_norm_eps=1e-5, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, feat_proj_layer_norm=True,
                 hidden_act="gelu", feat_extract_activation="gelu", mask_time_prob=0.05, mask_feature_prob=0.0, **unused):
        if feat_extract_norm != "group":
            raise ValueError("HubertModel: only the group-norm feature extractor (feat_extract_norm='group') is built")
        if do_stable_layer_norm:
            raise ValueError("HubertModel: the pre-LN encoder (do_stable_layer_norm=True) is not built")
        if conv_bias or not feat_proj_layer_norm or hidden_act != "gelu" or feat_extract_activation != "gelu":
            raise ValueError("HubertModel: conv_bias=False, feat_proj_layer_norm=True and GELU activations are what is built")
        super().__init__(dict(conv_dim=conv_dim, conv_kernel=conv_kernel, conv_stride=conv_stride, hidden_size=hidden_size,
                              num_attention_heads=num_attention_heads, intermediate_size=intermediate_size, num_hidden_layers=num_hidden_layers,
                              num_conv_pos_embeddings=num_conv_pos_embeddings, num_conv_pos_embedding_groups=num_conv_pos_embedding_groups,
                              layer_norm_eps=layer_norm_eps),
                         masked_spec_embed=mask_time_prob > 0.0 or mask_feature_prob > 0.0)         # HF registers it under this condition

    @classmethod
    def base(cls, **overrides):
        """HuBERT-base: facebook/hubert-base-ls960, mHuBERT, ContentVec."""
        return cls(**dict(_BASE, **overrides))

    def _hidden_layout(self, B, n1, F, H):
        return (B, n1, F, H), ()                 # us_hubert_forward: item-major, no strides

    def forward(self, wav, lengths=None, output_layer=None, output_hidden_states=False, normalize=False):
        return self._encode(wav, lengths, output_layer, output_hidden_states, normalize)


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
    return rename_fairseq(sd, _FAIRSEQ)


_W2V2_DROPPED = ("quantizer.", "project_q.")
_W2V2_KNOWN = re.compile(r"^(feature_extractor\.conv_layers\.\d+\.conv\.weight"
                         r"|feature_extractor\.conv_layers\.0\.layer_norm\.(weight|bias)"
                         r"|feature_projection\.(layer_norm|projection)\.(weight|bias)"
                         r"|encoder\.pos_conv_embed\.conv\.(bias|weight_g|weight_v)"
                         r"|encoder\.layer_norm\.(weight|bias)"
                         r"|encoder\.layers\.\d+\.(attention\.(k|v|q|out)_proj|layer_norm|final_layer_norm|feed_forward\.(intermediate|output)_dense)"
                         r"\.(weight|bias))$")


def from_fairseq_wav2vec2_state_dict(sd):
    """A fairseq wav2vec 2.0 checkpoint's `model` dictionary (`wav2vec_small.pt`) under `HubertModel`'s key names: `from_fairseq_state_dict`'s
    table.  Dropped, as unused in eval: `mask_emb`, `label_embs_concat` and `final_proj.*` (as there), and the pre-training's quantiser,
    `quantizer.*` (`vars`, `weight_proj.*`) and `project_q.*`.  Any other key that is not one of the base form's is a ValueError naming it.
    Tested on a hand-made dictionary of the right names only, as `from_fairseq_state_dict` is."""
    out = rename_fairseq(OrderedDict((k, v) for k, v in sd.items() if not k.startswith(_W2V2_DROPPED)), _FAIRSEQ)
    unknown = [k for k in out if not _W2V2_KNOWN.match(k)]
    if unknown:
        raise ValueError(f"from_fairseq_wav2vec2_state_dict: unknown keys {unknown[:4]}{' ...' if len(unknown) > 4 else ''}")
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
