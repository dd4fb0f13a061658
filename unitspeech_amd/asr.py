"""A CTC recogniser on the HIP library and the scoring that goes with it: 16 kHz waveform -> token ids -> text -> CER / WER
(csrc/ctc.hip), the counterpart of the reference's `evaluation/` (which transcribes the synthesised speech and scores it by error rate).

  CTCHead                         `lm_head` of a CTC model on any [B, F, H] device features: logits, log_probs, greedy decoding
  HubertForCTC / Wav2Vec2ForCTC   `transformers`' classes of the same names for the base form (group-norm extractor, post-LN layers, no
                                  adapter), with exactly their `state_dict` keys, around the library's `HubertModel`
  CTCVocabulary, normalize_text   HF's `vocab.json`; ids -> text, text -> ids, and the reference text brought to the vocabulary
  edit_distance, error_rates      Levenshtein distance per pair on the device; corpus and per-utterance CER / WER
  ctc_loss, forced_align          fitting the head on frozen features (csrc/ctc_train.hip): the CTC loss, differentiable in the logits, and
                                  the best alignment of a transcript to the frames; `CTCHead(..., trainable=True)` is the head that trains

The recogniser's contract is HF's: ids are the argmax of the fp32 logits (the lower index on ties).  Nothing is read back to the host
between the encoder, the head and the collapse.  There is no CPU fallback: a tensor that is not on a GPU raises.
"""
from __future__ import annotations

import json
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._args import call as _call, device_lengths, f32 as _f32, host_lengths, i64 as _i64, need_gpu as _need_gpu
from .hubert import _BASE, HubertModel

__all__ = ["CTCHead", "HubertForCTC", "Wav2Vec2ForCTC", "load_ctc_checkpoint", "CTCVocabulary", "normalize_text", "edit_distance",
           "error_rates", "ctc_loss", "forced_align"]

MAX_V, MAX_H, MAX_TOKENS = 2048, 1024, 4096
MAX_TARGET = 1024                 # tokens per target of ctc_loss / forced_align


@torch.no_grad()
def ctc_collapse(ids, lengths=None, blank: int = 0, first_frame: bool = False):
    """ids [B, Tmax] int64 with lengths [B] (frames; None: all) -> (tokens [B, Tmax], n [B]) and, when asked, first_frame [B, Tmax]:
    equal neighbours merged, then `blank` dropped; zero beyond n[b]."""
    _need_gpu(ids, "ctc_collapse", "the recogniser")
    dev = ids.device
    u = _i64(ids, dev)
    if u.dim() != 2 or u.numel() == 0:
        raise ValueError(f"ctc_collapse: ids must be a non-empty [B, Tmax], got {tuple(u.shape)}")
    B, T = u.shape
    lens = device_lengths(lengths, B, dev, "ctc_collapse")
    tokens = torch.empty(B, T, dtype=torch.int64, device=dev)
    ff = torch.empty(B, T, dtype=torch.int64, device=dev) if first_frame else None
    n = torch.empty(B, dtype=torch.int64, device=dev)
    _call(dev, "us_ctc_collapse", u, lens, B, T, int(blank), tokens, ff, n)
    return (tokens, n, ff) if first_frame else (tokens, n)


class CTCHead(torch.nn.Module):
    """`lm_head`: `weight` [V, H] and `bias` [V].  V in [2, 2048], H a multiple of 4 up to 1024.

    `forward(features [B, F, H], frame_lengths=None)` -> logits [B, F, V] (`log_probs=True`: `(logits, log_probs)`); rows at or beyond
    frame_lengths[b] are 0.  `decode(...)` -> `(tokens [B, F], n [B])`, greedy.

    `trainable=True` (the `Encoder(..., trainable=True)` convention): the two parameters require grad, and `forward` with gradients
    enabled records `us_ctc_head_backward` as the logits' backward; the features get a gradient only when they require one."""

    def __init__(self, hidden_size: int, vocab_size: int, trainable: bool = False):
        super().__init__()
        H, V = int(hidden_size), int(vocab_size)
        if not 2 <= V <= MAX_V:
            raise ValueError(f"CTCHead: vocab_size = {V}; the library takes 2 to {MAX_V}")
        if H % 4 or not 4 <= H <= MAX_H:
            raise ValueError(f"CTCHead: hidden_size = {H}; the library takes a multiple of 4 up to {MAX_H}")
        self.trainable = bool(trainable)
        self.weight = torch.nn.Parameter(torch.zeros(V, H), requires_grad=self.trainable)
        self.bias = torch.nn.Parameter(torch.zeros(V), requires_grad=self.trainable)
        self._packed, self._tag = None, None

    def packed(self, dev):
        """The head in the library's operand form on `dev`, packed again when a parameter's storage or version changed."""
        tag = tuple((p.data_ptr(), p._version, p.device) for p in (self.weight, self.bias)) + (dev,)
        if self._packed is None or self._tag != tag:
            V, H = self.weight.shape
            n = int(_lib.load().us_ctc_packed_bytes(V, H))
            buf = torch.empty(n, dtype=torch.uint8, device=dev)
            # w and b are read on the stream their memory would be reused on
            _call(dev, "us_ctc_pack_head", _f32(self.weight, dev), _f32(self.bias, dev), V, H, buf, n)
            self._packed, self._tag = buf, tag
        return self._packed

    @torch.no_grad()
    def _run(self, features, frame_lengths, log_probs, ids):
        _need_gpu(features, "CTCHead", "the recogniser")
        V, H = self.weight.shape
        if features.dim() != 3 or features.shape[-1] != H or features.numel() == 0:
            raise ValueError(f"CTCHead: features must be a non-empty [B, F, {H}], got {tuple(features.shape)}")
        dev = features.device
        x = features.detach().to(torch.float32).contiguous()
        B, F = x.shape[:2]
        lens = device_lengths(frame_lengths, B, dev, "CTCHead")
        logits = torch.empty(B, F, V, device=dev)
        lp = torch.empty(B, F, V, device=dev) if log_probs else None
        out_ids = torch.empty(B, F, dtype=torch.int64, device=dev) if ids else None
        _call(dev, "us_ctc_logits", x, lens, self.packed(dev), B, F, V, H, logits, lp, out_ids)
        return logits, lp, out_ids, lens

    def forward(self, features, frame_lengths=None, log_probs: bool = False):
        if self.trainable and torch.is_grad_enabled() and (self.weight.requires_grad or self.bias.requires_grad or features.requires_grad):
            logits, lp = _HeadFn.apply(self, features, frame_lengths, log_probs, self.weight, self.bias)   # lp carries no gradient
        else:
            logits, lp, _, _ = self._run(features, frame_lengths, log_probs, False)
        return (logits, lp) if log_probs else logits

    def argmax(self, features, frame_lengths=None):
        """-> (logits, ids [B, F] int64): ids == logits.argmax(-1) inside the lengths, -1 beyond."""
        logits, _, ids, _ = self._run(features, frame_lengths, False, True)
        return logits, ids

    def decode(self, features, frame_lengths=None, blank: int = 0, first_frame: bool = False, log_probs: bool = False):
        """-> (tokens [B, F] int64, n [B] int64), then first_frame [B, F] and log_probs [B, F, V] when asked for, in that order."""
        _, lp, ids, lens = self._run(features, frame_lengths, log_probs, True)
        out = ctc_collapse(ids, lens, blank, first_frame)
        return out + (lp,) if log_probs else out


class _HeadFn(torch.autograd.Function):
    """logits = us_ctc_logits(features) with us_ctc_head_backward as its backward (dW, db, and dX when the features require grad)."""

    @staticmethod
    def forward(ctx, head, features, frame_lengths, log_probs, weight, bias):
        logits, lp, _, lens = head._run(features, frame_lengths, log_probs, False)
        ctx.save_for_backward(features, weight)
        ctx.lens = lens
        if lp is not None:
            ctx.mark_non_differentiable(lp)
        return logits, lp

    @staticmethod
    def backward(ctx, g, _):
        features, weight = ctx.saved_tensors
        dev = g.device
        B, F, V = g.shape
        H = weight.shape[1]
        g = g.detach().to(torch.float32).contiguous()
        x = features.detach().to(torch.float32).contiguous()
        w = _f32(weight, dev)
        dw, db = torch.empty(V, H, device=dev), torch.empty(V, device=dev)
        dx = torch.empty(B, F, H, device=dev) if ctx.needs_input_grad[1] else None
        n = int(_lib.load().us_ctc_head_backward_workspace_bytes(B, F, V, H))
        ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        _call(dev, "us_ctc_head_backward", g, x, ctx.lens, w, B, F, V, H, dw, db, dx, ws, n)
        return (None, None if dx is None else dx.to(features.dtype), None, None, dw.to(weight.dtype) if ctx.needs_input_grad[4] else None,
                db if ctx.needs_input_grad[5] else None)


def _sequences(what, x, targets, frame_lengths, target_lengths):
    """The checked device arguments of a loss / alignment call: x [B, T, V] fp32, targets [B, Lmax] int64 and the two length vectors."""
    _need_gpu(x, what, "the recogniser")
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty [B, T, V], got {tuple(x.shape)}")
    dev = x.device
    B = x.shape[0]
    tg = _i64(targets, dev)
    if tg.dim() != 2 or tg.shape[0] != B:
        raise ValueError(f"{what}: targets {tuple(tg.shape)} must be [{B}, Lmax]")
    if target_lengths is None:
        raise ValueError(f"{what}: target_lengths is needed")
    return (x.detach().to(torch.float32).contiguous(), tg, device_lengths(frame_lengths, B, dev, what),
            device_lengths(target_lengths, B, dev, what))


def _ctc_loss_call(x, tg, fl, tl, blank, zero_infinity, stage=_lib.US_CTC_WHOLE, grad_out=None, ws=None, with_grad=False):
    """One us_ctc_loss call -> (loss, grad_logits or None, workspace).  US_CTC_FORWARD leaves alpha in the workspace it returns;
    US_CTC_BACKWARD takes that workspace and `grad_out` and runs the backward sweep alone; US_CTC_WHOLE with `with_grad` does both at once."""
    dev = x.device
    B, T, V = x.shape
    Lmax = int(tg.shape[1])
    with_grad = bool(with_grad) or stage == _lib.US_CTC_BACKWARD
    n = int(_lib.load().us_ctc_loss_workspace_bytes(B, T, Lmax, int(with_grad or stage == _lib.US_CTC_FORWARD)))
    if ws is None:
        ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    loss = torch.empty(B, device=dev)
    grad = torch.empty(B, T, V, device=dev) if with_grad else None
    _call(dev, "us_ctc_loss", x, fl, tg if Lmax else None, tl, grad_out, B, T, V, Lmax, int(blank), int(bool(zero_infinity)), stage, loss, grad,
          ws, n)
    return loss, grad, ws


class _CTCLossFn(torch.autograd.Function):
    """The per-item losses.  The forward keeps alpha in the call's workspace; the backward runs the backward sweep alone on it, with the
    incoming per-item gradient as `grad_out`, so the scaled gradient is written by the kernel itself."""

    @staticmethod
    def forward(ctx, logits, tg, fl, tl, blank, zero_infinity):
        x = logits.detach().to(torch.float32).contiguous()
        loss, _, ws = _ctc_loss_call(x, tg, fl, tl, blank, zero_infinity, _lib.US_CTC_FORWARD)
        ctx.save_for_backward(x)
        ctx.args = (tg, fl, tl, blank, zero_infinity, ws)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        (x,) = ctx.saved_tensors
        tg, fl, tl, blank, zero_infinity, ws = ctx.args
        go = go.detach().to(torch.float32).contiguous()
        _, grad, _ = _ctc_loss_call(x, tg, fl, tl, blank, zero_infinity, _lib.US_CTC_BACKWARD, go, ws)
        return grad.to(ctx.dtype), None, None, None, None, None


def ctc_loss(logits, targets, frame_lengths, target_lengths, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False):
    """The CTC loss of logits [B, T, V] (batch-first; the log-softmax is taken inside) against targets [B, Lmax] int64, with frame_lengths
    [B] (None: all T) and target_lengths [B]; at most 1024 tokens per target.  Differentiable in `logits`.

    `reduction`: "none" -> [B]; "sum"; "mean" as torch has it: each item divided by its target length (clamped to 1), then the average.
    An infeasible item has loss +inf (0 with `zero_infinity`) and a ZERO gradient, where torch writes NaN gradients unless
    `zero_infinity` is set.  An item has the same loss and gradient bits alone and in any batch."""
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"ctc_loss: reduction = {reduction!r}; expected 'none', 'sum' or 'mean'")
    _, tg, fl, tl = _sequences("ctc_loss", logits, targets, frame_lengths, target_lengths)
    if torch.is_grad_enabled() and logits.requires_grad:
        loss = _CTCLossFn.apply(logits, tg, fl, tl, int(blank), bool(zero_infinity))
    else:
        loss = _ctc_loss_call(logits.detach().to(torch.float32).contiguous(), tg, fl, tl, blank, zero_infinity)[0]
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    return (loss / tl.clamp(min=1).to(loss.dtype)).mean()


@torch.no_grad()
def forced_align(scores, targets, frame_lengths, target_lengths, blank: int = 0):
    """The best alignment of targets [B, Lmax] to the frames of scores [B, T, V] (log-probabilities, or any additive score) ->
    (path [B, T] int64: the entry emitted at each frame, blank included, -1 beyond the item's frames; score [B]: the path's summed score;
    start [B, Lmax], frames [B, Lmax] int64: the first frame of each target token and the number of frames on it).

    Ties: staying in a state wins over advancing by one, that over skipping a blank; the last label wins over the final blank as the end.
    An infeasible item has score -inf, a path of -1 and frames 0."""
    x, tg, fl, tl = _sequences("forced_align", scores, targets, frame_lengths, target_lengths)
    dev = x.device
    B, T, V = x.shape
    Lmax = int(tg.shape[1])
    n = int(_lib.load().us_ctc_align_workspace_bytes(B, T, Lmax))
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    path = torch.empty(B, T, dtype=torch.int64, device=dev)
    score = torch.empty(B, device=dev)
    start = torch.empty(B, Lmax, dtype=torch.int64, device=dev)
    frames = torch.empty(B, Lmax, dtype=torch.int64, device=dev)
    _call(dev, "us_ctc_forced_align", x, fl, tg if Lmax else None, tl, B, T, V, Lmax, int(blank), path, score, start if Lmax else None,
          frames if Lmax else None, ws, n)
    return path, score, start, frames


class _EncoderForCTC(torch.nn.Module):
    _prefix = ""

    def __init__(self, vocab_size: int = 32, pad_token_id: int = 0, add_adapter: bool = False, trainable: bool = False, **config):
        super().__init__()
        if add_adapter:
            raise ValueError(f"{type(self).__name__}: the adapter (add_adapter=True) is not built")
        encoder = HubertModel(**config)
        if not 0 <= int(pad_token_id) < int(vocab_size):
            raise ValueError(f"{type(self).__name__}: pad_token_id {pad_token_id} is not in the vocabulary of {vocab_size}")
        self.add_module(self._prefix, encoder)
        self.lm_head = CTCHead(encoder.config["hidden_size"], vocab_size, trainable=trainable)
        self.vocab_size, self.pad_token_id = int(vocab_size), int(pad_token_id)

    @classmethod
    def base(cls, **overrides):
        """The base size (facebook/hubert-base-ls960, wav2vec2-base)."""
        return cls(**dict(_BASE, **overrides))

    @property
    def encoder(self) -> HubertModel:
        return self._modules[self._prefix]

    def load_state_dict(self, state_dict, strict=True, **kw):
        """transformers' keys; the encoder's part goes through `HubertModel.load_state_dict` (which also takes the older spelling of
        the positional convolution's weight norm)."""
        p = self._prefix + "."
        enc = OrderedDict((k[len(p):], v) for k, v in state_dict.items() if k.startswith(p))
        head = OrderedDict((k[len("lm_head."):], v) for k, v in state_dict.items() if k.startswith("lm_head."))
        rest = [k for k in state_dict if not k.startswith(p) and not k.startswith("lm_head.")]
        if strict and rest:
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: unexpected keys {rest[:4]}{' ...' if len(rest) > 4 else ''}")
        self.encoder.load_state_dict(enc, strict=strict, **kw)
        return self.lm_head.load_state_dict(head, strict=strict, **kw)

    def _frames(self, wav, lengths):
        v = host_lengths(lengths, wav.shape[0], type(self).__name__)
        if v is None:
            return None, None
        return v, torch.tensor([self.encoder.frames(n) for n in v], dtype=torch.int64).to(wav.device, non_blocking=True)

    @torch.no_grad()
    def forward(self, wav, lengths=None, normalize: bool = False):
        """wav [B, T] at 16 kHz on the device, lengths [B] in samples (host values) -> logits [B, F, V]; rows past an item's frames are 0."""
        v, frames = self._frames(wav, lengths)
        return self.lm_head(self.encoder(wav, v, normalize=normalize), frames)

    @torch.no_grad()
    def transcribe_ids(self, wav, lengths=None, normalize: bool = False, first_frame: bool = False):
        """-> (tokens [B, F] int64, n [B] int64) on the device (and first_frame [B, F], in frames of 20 ms, when asked): encoder, head and
        greedy collapse with `pad_token_id` as the blank, with no read back in between."""
        v, frames = self._frames(wav, lengths)
        return self.lm_head.decode(self.encoder(wav, v, normalize=normalize), frames, self.pad_token_id, first_frame)

    def loss(self, wav, lengths, targets, target_lengths, normalize: bool = False, reduction: str = "mean", zero_infinity: bool = False):
        """The CTC loss of the transcripts targets [B, Lmax] int64 (target_lengths [B]) with `pad_token_id` as the blank.  The encoder is
        frozen (it runs without gradients); a head built with `trainable=True` gets its gradients from `.backward()`."""
        v, frames = self._frames(wav, lengths)
        with torch.no_grad():
            features = self.encoder(wav, v, normalize=normalize)
        return ctc_loss(self.lm_head(features, frames), targets, frames, target_lengths, self.pad_token_id, reduction, zero_infinity)

    @torch.no_grad()
    def align(self, wav, lengths, targets, target_lengths, normalize: bool = False):
        """-> `forced_align`'s (path, score, start, frames) of the transcripts on the head's log-probabilities, in frames of 20 ms."""
        v, frames = self._frames(wav, lengths)
        _, lp = self.lm_head(self.encoder(wav, v, normalize=normalize), frames, log_probs=True)
        return forced_align(lp, targets, frames, target_lengths, self.pad_token_id)


class HubertForCTC(_EncoderForCTC):
    """`transformers.HubertForCTC` for the base form: keys `hubert.*`, `lm_head.weight`, `lm_head.bias`.  The constructor takes the config's
    fields by keyword, with `vocab_size` and `pad_token_id` (the blank); what `HubertModel` refuses, and `add_adapter=True`, is refused."""
    _prefix = "hubert"


class Wav2Vec2ForCTC(_EncoderForCTC):
    """`transformers.Wav2Vec2ForCTC` for the base form (wav2vec2-base and its fine-tunings): keys `wav2vec2.*`, `lm_head.*`.  For this form
    the two classes compute the same function of the same weights."""
    _prefix = "wav2vec2"


def load_ctc_checkpoint(path, **config):
    """A `torch.save`d `transformers` state dict -> `HubertForCTC` or `Wav2Vec2ForCTC` in eval mode, by the keys' prefix.  The
    configuration is the base one unless fields are given; `vocab_size` is read from `lm_head.weight`."""
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict) or "lm_head.weight" not in sd:
        raise ValueError(f"{path}: expected a state dict with `lm_head.weight`")
    if any(k.startswith("hubert.") for k in sd):
        cls = HubertForCTC
    elif any(k.startswith("wav2vec2.") for k in sd):
        cls = Wav2Vec2ForCTC
    else:
        raise ValueError(f"{path}: the keys start with neither `hubert.` nor `wav2vec2.`")
    config.setdefault("vocab_size", int(sd["lm_head.weight"].shape[0]))
    model = cls.base(**config)
    model.load_state_dict(sd)
    return model.eval()


# ---- text ------------------------------------------------------------------------------------------------------------------------

_CEDILLA = {"ş": "ș", "ţ": "ț", "Ş": "Ș", "Ţ": "Ț"}       # ş ţ Ş Ţ -> ș ț Ș Ț


class CTCVocabulary:
    """HF's `vocab.json` ({token: id}, a dict or a path).  `blank` is the CTC blank's token and `word_delimiter` the token that stands for
    a space.  Tokens of more than one character (`<unk>`, `<s>`, ...) are special: `decode` drops them."""

    def __init__(self, token_to_id, blank: str = "<pad>", word_delimiter: str = "|"):
        if not isinstance(token_to_id, dict):
            with open(token_to_id, encoding="utf-8") as f:
                token_to_id = json.load(f)
        self.token_to_id = {str(k): int(v) for k, v in token_to_id.items()}
        if len(set(self.token_to_id.values())) != len(self.token_to_id):
            raise ValueError("CTCVocabulary: two tokens share an id")
        if blank not in self.token_to_id:
            raise ValueError(f"CTCVocabulary: the blank {blank!r} is not in the vocabulary")
        self.id_to_token = {v: k for k, v in self.token_to_id.items()}
        self.blank, self.word_delimiter = blank, word_delimiter
        self.blank_id = self.token_to_id[blank]
        self.characters = {t for t in self.token_to_id if len(t) == 1 and t != word_delimiter}

    def __len__(self):
        return len(self.token_to_id)

    def decode(self, tokens, n=None):
        """tokens [B, L] (tensor, array or lists) with n [B] valid entries (None: all) -> list[str], words separated by one space."""
        rows = tokens.tolist() if hasattr(tokens, "tolist") else [list(r) for r in tokens]
        counts = [len(r) for r in rows] if n is None else (n.tolist() if hasattr(n, "tolist") else list(n))
        out = []
        for r, c in zip(rows, counts):
            toks = [self.id_to_token[int(i)] for i in r[:int(c)]]
            s = "".join(" " if t == self.word_delimiter else t for t in toks if len(t) == 1)
            out.append(" ".join(s.split()))
        return out

    def encode(self, text: str):
        """text -> ids, a space as the word delimiter; a character the vocabulary lacks is a ValueError (see `normalize_text`)."""
        ids = []
        for ch in text:
            t = self.word_delimiter if ch == " " else ch
            if t not in self.token_to_id or (ch != " " and ch not in self.characters):
                raise ValueError(f"CTCVocabulary.encode: {ch!r} is not in the vocabulary")
            ids.append(self.token_to_id[t])
        return ids


def normalize_text(s: str, vocabulary: CTCVocabulary) -> str:
    """A reference transcript as the recogniser could have written it: the vocabulary's letter case (when its letters are all of one
    case), Romanian cedilla forms folded to comma-below (ş -> ș, ţ -> ț and their capitals), characters the vocabulary lacks dropped,
    whitespace collapsed."""
    letters = [c for c in vocabulary.characters if c.isalpha()]
    if letters and all(c == c.upper() for c in letters):
        s = s.upper()
    elif letters and all(c == c.lower() for c in letters):
        s = s.lower()
    s = "".join(_CEDILLA.get(c, c) for c in s)
    s = "".join(c if c in vocabulary.characters else (" " if c.isspace() else "") for c in s)
    return " ".join(s.split())


# ---- scoring ---------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def edit_distance(hyp, ref, n_hyp, n_ref):
    """hyp [P, Lh], ref [P, Lr] int64 with n_hyp, n_ref [P] valid tokens, on the device -> the Levenshtein distance (unit costs) of each
    pair, [P] int64 on the device, exact.  At most 4096 tokens per sequence.  Substitution / deletion / insertion counts are not given:
    they depend on which optimal alignment is taken."""
    _need_gpu(hyp, "edit_distance", "the recogniser")
    dev = hyp.device
    a, b = _i64(hyp, dev), _i64(ref, dev)
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"edit_distance: hyp and ref must be [P, Lh] and [P, Lr], got {tuple(a.shape)} and {tuple(b.shape)}")
    P = int(a.shape[0])
    na, nb = device_lengths(n_hyp, P, dev, "edit_distance"), device_lengths(n_ref, P, dev, "edit_distance")
    if na is None or nb is None:
        raise ValueError("edit_distance: n_hyp and n_ref are needed")
    dist = torch.empty(P, dtype=torch.int64, device=dev)
    _call(dev, "us_edit_distance", a, na, int(a.shape[1]), b, nb, int(b.shape[1]), P, dist)
    return dist


def _padded(seqs, dev):
    L = max(1, max(len(s) for s in seqs))
    x = np.zeros((len(seqs), L), dtype=np.int64)
    for i, s in enumerate(seqs):
        x[i, :len(s)] = s
    return torch.from_numpy(x).to(dev), torch.tensor([len(s) for s in seqs], dtype=torch.int64).to(dev)


def error_rates(hyps, refs, device="cuda"):
    """Corpus and per-utterance character and word error rates of hypotheses against references (lists of str, already normalised).

    Characters (spaces included) and words (`str.split`, numbered through one dictionary over both lists) are mapped to ids on the host;
    each level is one `edit_distance` call.  The corpus rates are sum of distances / sum of reference lengths.  -> {"cer", "wer",
    "per_utterance": [{"cer", "wer", "char_distance", "chars", "word_distance", "words"}]}; an utterance with an empty reference has nan
    rates; ValueError when the references hold no character or no word at all."""
    if len(hyps) != len(refs):
        raise ValueError(f"error_rates: {len(hyps)} hypotheses for {len(refs)} references")
    if not len(refs) or not sum(len(r) for r in refs) or not sum(len(r.split()) for r in refs):
        raise ValueError("error_rates: the references are empty")
    dev = torch.device(device)
    words = {}
    levels = []
    for split in (lambda s: [ord(c) for c in s], lambda s: [words.setdefault(w, len(words)) for w in s.split()]):
        h, r = [split(s) for s in hyps], [split(s) for s in refs]
        (ht, hn), (rt, rn) = _padded(h, dev), _padded(r, dev)
        levels.append((edit_distance(ht, rt, hn, rn), [len(s) for s in r]))
    (cd, nc), (wd, nw) = [(d.tolist(), n) for d, n in levels]            # the one read back, after both calls are enqueued
    per = [{"cer": cd[i] / nc[i] if nc[i] else math.nan, "wer": wd[i] / nw[i] if nw[i] else math.nan, "char_distance": cd[i], "chars": nc[i],
            "word_distance": wd[i], "words": nw[i]} for i in range(len(refs))]
    return {"cer": sum(cd) / sum(nc), "wer": sum(wd) / sum(nw), "per_utterance": per}
