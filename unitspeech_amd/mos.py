"""A predicted mean opinion score on the HIP library (csrc/mos.hip): s3prl's `mos_wav2vec2` (upstream/mos_prediction), the third figure of
the reference's evaluation next to the error rates (`asr.py`, `whisper.py`) and the speaker similarity (`speaker_encoder.py`).

  MOSHead              the learned layer mix (s3prl's Featurizer) and the downstream head on any encoder's hidden states
  MOSPredictor         16 kHz waveform -> score: `HubertModel` in the wav2vec2-base form with every hidden state, then the head
  load_mos_checkpoint  an s3prl checkpoint file and the upstream's weights -> `MOSPredictor`

The head's parameters keep s3prl's names: `featurizer.weights`, `connector.{weight,bias}`, `model.mean_net_pooling.W.{weight,bias}`,
`model.mean_net_linear.{weight,bias}`.  The judge-bias branch, segment-wise scoring, the Featurizer's `normalize` and training are not
built.  There is no CPU fallback: a tensor that is not on a GPU raises.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from ._args import call as _call, device_lengths, f32 as _f32, host_lengths, need_gpu as _need_gpu
from ._wav_encoder import _set as _param
from .hubert import HubertModel, from_fairseq_wav2vec2_state_dict

__all__ = ["MOSHead", "MOSPredictor", "load_mos_checkpoint"]

MAX_STATES, MAX_H, MAX_P = 32, 1024, 4096
_ATT, _MEAN = "model.mean_net_pooling.W.", "model.mean_net_linear."
_IGNORED = ("model.bias_net_", "model.judge_")              # the judge-bias branch: unused when no judge id is given


class MOSHead(torch.nn.Module):
    """`forward(hidden_states, frame_lengths=None, layout="blhd", return_frames=False)` -> scores [B] (with `return_frames`:
    `(scores, mu [B, F], alpha [B, F])`, the per-frame scores and the pooling weights, 0 past an item's frames).

    hidden_states: [B, n_states, F, H] (`layout="blhd"`, what `HubertModel(..., output_hidden_states=True)` returns) or [n_states, B, F, H]
    (`"lbhd"`, `WavLMModel`'s), fp32 on the device, read in place.  frame_lengths [B]: frames per item (None: all F); an item's score is
    what the item gives alone, bit for bit; an item of 0 frames gets NaN.  n_states in [1, 32], hidden_size a multiple of 4 up to 1024,
    projector_dim in [1, 4096]."""

    def __init__(self, hidden_size: int, n_states: int, projector_dim: int, attention_pooling: bool = True, clipping: bool = False):
        super().__init__()
        H, n, P = int(hidden_size), int(n_states), int(projector_dim)
        if H % 4 or not 4 <= H <= MAX_H:
            raise ValueError(f"MOSHead: hidden_size = {H}; the library takes a multiple of 4 up to {MAX_H}")
        if not 1 <= n <= MAX_STATES:
            raise ValueError(f"MOSHead: n_states = {n}; the library takes 1 to {MAX_STATES}")
        if not 1 <= P <= MAX_P:
            raise ValueError(f"MOSHead: projector_dim = {P}; the library takes 1 to {MAX_P}")
        self.hidden_size, self.n_states, self.projector_dim = H, n, P
        self.attention_pooling, self.clipping = bool(attention_pooling), bool(clipping)
        _param(self, "featurizer.weights", torch.zeros(n))
        _param(self, "connector.weight", torch.zeros(P, H))
        _param(self, "connector.bias", torch.zeros(P))
        _param(self, _MEAN + "weight", torch.zeros(1, P))
        _param(self, _MEAN + "bias", torch.zeros(1))
        if self.attention_pooling:
            _param(self, _ATT + "weight", torch.zeros(1, P))
            _param(self, _ATT + "bias", torch.zeros(1))
        self._packed, self._tag = None, None

    def load_state_dict(self, state_dict, strict=True, **kw):
        """s3prl's keys; the judge-bias branch (`model.bias_net_*`, `model.judge_*`) is left out.  Any other unknown key is refused."""
        sd = OrderedDict((k, v) for k, v in state_dict.items() if not k.startswith(_IGNORED))
        return super().load_state_dict(sd, strict=strict, **kw)

    def packed(self, dev):
        """The head in the library's folded form on `dev`, packed again when a parameter's storage or version changed."""
        ps = list(self.parameters())
        tag = tuple((p.data_ptr(), p._version, p.device) for p in ps) + (dev,)
        if self._packed is None or self._tag != tag:
            sd = {k: _f32(v, dev) for k, v in self.state_dict(keep_vars=True).items()}
            n, H, P = self.n_states, self.hidden_size, self.projector_dim
            nbytes = int(_lib.load().us_mos_packed_bytes(n, H, P))
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _call(dev, "us_mos_pack_head", sd["featurizer.weights"], sd["connector.weight"], sd["connector.bias"], sd.get(_ATT + "weight"),
                  sd.get(_ATT + "bias"), sd[_MEAN + "weight"], sd[_MEAN + "bias"], n, H, P, buf, nbytes)
            self._packed, self._tag = buf, tag
        return self._packed

    @torch.no_grad()
    def folded(self, dev):
        """-> (s [n_states], v_e [H], v_m [H], k [2] = k_e, k_m) as the pack holds them, on `dev`."""
        n, H = self.n_states, self.hidden_size
        s, ve, vm, k = (torch.empty(m, device=dev) for m in (n, H, H, 2))
        _call(dev, "us_mos_unpack_head", self.packed(dev), n, H, s, ve, vm, k)
        return s, ve, vm, k

    @torch.no_grad()
    def forward(self, hidden_states, frame_lengths=None, layout: str = "blhd", return_frames: bool = False):
        _need_gpu(hidden_states, "MOSHead", "the MOS predictor")
        if layout not in ("blhd", "lbhd"):
            raise ValueError(f"MOSHead: layout = {layout!r}; expected 'blhd' or 'lbhd'")
        n, H = self.n_states, self.hidden_size
        want = "[B, %d, F, %d]" % (n, H) if layout == "blhd" else "[%d, B, F, %d]" % (n, H)
        hs = hidden_states
        if hs.dim() != 4 or hs.shape[-1] != H or hs.shape[1 if layout == "blhd" else 0] != n or hs.numel() == 0:
            raise ValueError(f"MOSHead: hidden_states must be a non-empty {want}, got {tuple(hs.shape)}")
        dev = hs.device
        hs = hs.detach().to(torch.float32).contiguous()
        B, F = (hs.shape[0], hs.shape[2]) if layout == "blhd" else (hs.shape[1], hs.shape[2])
        item, state = (n * F * H, F * H) if layout == "blhd" else (F * H, B * F * H)
        lens = device_lengths(frame_lengths, B, dev, "MOSHead")
        scores = torch.empty(B, device=dev)
        mu = torch.empty(B, F, device=dev) if return_frames else None
        alpha = torch.empty(B, F, device=dev) if return_frames else None
        nbytes = int(_lib.load().us_mos_workspace_bytes(B, F))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _call(dev, "us_mos_score", hs, item, state, lens, self.packed(dev), B, F, n, H, int(self.clipping), scores, mu, alpha, ws, nbytes)
        return (scores, mu, alpha) if return_frames else scores


class MOSPredictor(torch.nn.Module):
    """`forward(wav16 [B, T], lengths=None)` -> scores [B]: the upstream with every hidden state, frames per item from `upstream.frames`,
    then the head, with nothing read back in between.  `lengths` are samples per item (host values); an item's score is what the item gives
    alone.  `score_frames` also returns mu and alpha [B, F], one entry per 20 ms frame."""

    def __init__(self, upstream: HubertModel, head: MOSHead):
        super().__init__()
        if head.hidden_size != upstream.config["hidden_size"] or head.n_states != upstream.config["num_hidden_layers"] + 1:
            raise ValueError(f"MOSPredictor: the head takes {head.n_states} states of width {head.hidden_size}, the upstream gives "
                             f"{upstream.config['num_hidden_layers'] + 1} of width {upstream.config['hidden_size']}")
        self.upstream, self.head = upstream, head

    def _run(self, wav, lengths, return_frames):
        v = host_lengths(lengths, wav.shape[0], "MOSPredictor")
        frames = None if v is None else torch.tensor([self.upstream.frames(n) for n in v], dtype=torch.int64).to(wav.device, non_blocking=True)
        _, hs = self.upstream(wav, v, output_hidden_states=True)
        return self.head(hs, frames, "blhd", return_frames)

    @torch.no_grad()
    def forward(self, wav16, lengths=None):
        return self._run(wav16, lengths, False)

    @torch.no_grad()
    def score_frames(self, wav16, lengths=None):
        """-> (scores [B], mu [B, F], alpha [B, F])."""
        return self._run(wav16, lengths, True)


def _field(holder, name):
    """`name` out of a dict, an object with attributes, or (s3prl's Config) a nested dict: the first place that has it, else None."""
    if holder is None:
        return None
    if isinstance(holder, dict):
        if name in holder:
            return holder[name]
        for v in holder.values():
            if isinstance(v, dict):
                r = _field(v, name)
                if r is not None:
                    return r
        return None
    return getattr(holder, name, None)


def load_mos_checkpoint(path, upstream_path=None, featurizer_key: str = "Featurizer", downstream_key: str = "Downstream", args_key: str = "Args",
                        config_key: str = "Config", projector_dim=None, clipping=None, attention_pooling=None, **config):
    """An s3prl MOS checkpoint (`checkpoint[featurizer_key]` with `weights`, `checkpoint[downstream_key]` with the connector and the
    head, `checkpoint[args_key]` / `[config_key]`, an object or a dict, for `projector_dim`, `clipping` and `attention_pooling`) ->
    `MOSPredictor` in eval mode.  The four top-level names are keyword arguments because they are written from memory of s3prl.

    A value given by keyword wins; one not found in the file is read off the tensors: `projector_dim` from `connector.weight`,
    `attention_pooling` from the presence of `model.mean_net_pooling.*`.  `clipping` cannot be read off a shape: when the file does not hold
    it, it must be given (ValueError).  A checkpoint whose Featurizer asks for `normalize` (or holds a `layer_norm`) is refused.

    `upstream_path`: a `torch.save`d `transformers.Wav2Vec2Model` state dict (a `wav2vec2.` prefix is dropped), or fairseq's
    `wav2vec_small.pt` (`{"model": ...}`, through `from_fairseq_wav2vec2_state_dict`).  Further keywords are `HubertModel`'s fields
    (default: the base size)."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or featurizer_key not in ck or downstream_key not in ck:
        raise ValueError(f"{path}: expected `{featurizer_key}` and `{downstream_key}` at the top level")
    feat, down = ck[featurizer_key], ck[downstream_key]
    holders = [ck.get(args_key), ck.get(config_key)]

    def found(name):
        for h in holders:
            r = _field(h, name)
            if r is not None:
                return r
        return None

    if found("normalize") or any("layer_norm" in k or k.startswith("norm") for k in feat):
        raise ValueError(f"{path}: the Featurizer's per-layer layer_norm (normalize=True) is not built")
    extra = [k for k in feat if k != "weights"]
    if "weights" not in feat or extra:
        raise ValueError(f"{path}: the Featurizer must hold `weights` alone, got {list(feat)[:4]}")
    if "connector.weight" not in down:
        raise ValueError(f"{path}: `{downstream_key}` holds no connector.weight")
    if projector_dim is None:
        projector_dim = found("projector_dim")
    if projector_dim is None:
        projector_dim = int(down["connector.weight"].shape[0])
    has_att = any(k.startswith("model.mean_net_pooling.") for k in down)
    if attention_pooling is None:
        attention_pooling = found("attention_pooling")
    if attention_pooling is None:
        attention_pooling = has_att
    if clipping is None:
        clipping = found("clipping")
    if clipping is None:
        raise ValueError(f"{path}: `clipping` is neither in `{args_key}` nor in `{config_key}` and cannot be read off a shape: give clipping=")
    n_states, H = int(feat["weights"].shape[0]), int(down["connector.weight"].shape[1])
    head = MOSHead(H, n_states, int(projector_dim), bool(attention_pooling), bool(clipping))
    sd = OrderedDict(down)
    sd["featurizer.weights"] = feat["weights"]
    head.load_state_dict(sd)
    upstream = HubertModel.base(**config)
    if upstream_path is not None:
        up = torch.load(upstream_path, map_location="cpu", weights_only=False)
        if isinstance(up, dict) and isinstance(up.get("model"), dict):
            up = from_fairseq_wav2vec2_state_dict(up["model"])
        else:
            up = OrderedDict((k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k, v) for k, v in up.items())
        upstream.load_state_dict(up)
    return MOSPredictor(upstream, head).eval()
