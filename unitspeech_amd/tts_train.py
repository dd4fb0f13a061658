"""The alignment side of the text-to-speech training step (`train_STEP1.py`'s `compute_train_step_loss`, :336-349) in library
launches.

`mas_log_prior` is the Gaussian log-prior between the encoder's mu_x and the mel (:336-342, masked as `maximum_path` masks it),
`maximum_path` a drop-in for the external `monotonic_align.maximum_path` (:343) that runs on the device and never copies the
[B, Tx, Ty] table to the host, `align` both in one call with the durations MAS implies, and `duration_loss` the MSE of the log
durations (:348-349, `util.duration_loss` after `log(1e-8 + sum(attn))`), differentiable in logw.

`compute_train_step_loss` assembles the whole iteration (:319-387) from those, the trainable `Encoder` and `DurationPredictor`, the
crop and prior loss of `unit_encoder_train` and the decoder's `compute_loss`; `random_replace_tensor` is the speaker swap of
:325-326.
"""
from __future__ import annotations

import torch

from typing import Optional, Sequence

from . import _lib
from ._args import call as _call, f32 as _f32, i64 as _i64
from .unit_encoder_train import align_segment, prior_loss

__all__ = ["mas_log_prior", "maximum_path", "maximum_path_lengths", "align", "duration_loss", "random_replace_tensor",
           "compute_train_step_loss"]


@torch.no_grad()
def mas_log_prior(mu_x, y, x_mask, y_mask):
    """mu_x [B, F, Tx], y [B, F, Ty], x_mask [B, 1, Tx], y_mask [B, 1, Ty] -> log_prior [B, Tx, Ty] fp32:
    (-0.5 sum_f y^2 + sum_f mu_x y - 0.5 sum_f mu_x^2 - 0.5 F log 2 pi) x_mask y_mask."""
    dev = mu_x.device
    B, F, Tx = mu_x.shape
    Ty = y.shape[-1]
    if y.shape[:2] != (B, F) or tuple(x_mask.shape) != (B, 1, Tx) or tuple(y_mask.shape) != (B, 1, Ty):
        raise ValueError(f"mas_log_prior: mu_x {tuple(mu_x.shape)}, y {tuple(y.shape)}, x_mask {tuple(x_mask.shape)}, "
                         f"y_mask {tuple(y_mask.shape)} do not agree")
    mu, yy, xm, ym = _f32(mu_x, dev), _f32(y, dev), _f32(x_mask, dev), _f32(y_mask, dev)
    out = torch.empty(B, Tx, Ty, device=dev)
    _call(dev, "us_mas_log_prior", mu, yy, xm, ym, out, B, F, Tx, Ty)
    return out


@torch.no_grad()
def maximum_path_lengths(log_prior, x_lengths, y_lengths):
    """log_prior [B, Tx, Ty] with per-item lengths -> (attn [B, Tx, Ty] fp32 0/1, durations [B, Tx] fp32).  With int64 device
    lengths nothing crosses to or from the host; host lengths are copied to the device first (a synchronous upload)."""
    dev = log_prior.device
    B, Tx, Ty = log_prior.shape
    lp, xl, yl = _f32(log_prior, dev), _i64(x_lengths, dev), _i64(y_lengths, dev)
    if xl.shape != (B,) or yl.shape != (B,):
        raise ValueError(f"maximum_path: lengths {tuple(xl.shape)} / {tuple(yl.shape)} must hold {B} values")
    attn = torch.empty(B, Tx, Ty, device=dev)
    dur = torch.empty(B, Tx, device=dev)
    n = int(_lib.load().us_maximum_path_workspace_bytes(B, Tx, Ty))
    ws = torch.empty(n, dtype=torch.uint8, device=dev) if n else None        # 0 while every item's table fits in LDS
    _call(dev, "us_maximum_path", lp, xl, yl, attn, dur, B, Tx, Ty, ws, n)
    return attn, dur


@torch.no_grad()
def maximum_path(value, mask):
    """Drop-in for `monotonic_align.maximum_path(value, mask)` (train_STEP1.py:343): value, mask [B, Tx, Ty] -> path [B, Tx, Ty]
    0/1 in value's dtype.  tx / ty are read off the mask's first column / row, as the reference does; the cells the algorithm
    reads all lie inside the mask, so value is not multiplied by it here."""
    if value.dim() != 3 or mask.shape != value.shape:
        raise ValueError(f"maximum_path: value {tuple(value.shape)} and mask {tuple(mask.shape)} must both be [B, Tx, Ty]")
    tx = mask.sum(1)[:, 0].to(torch.int64)
    ty = mask.sum(2)[:, 0].to(torch.int64)
    attn, _ = maximum_path_lengths(value, tx, ty)
    return attn.to(value.dtype)


@torch.no_grad()
def align(mu_x, y, x_mask, y_mask, x_lengths, y_lengths):
    """train_STEP1.py:336-345 -> (attn [B, Tx, Ty], durations [B, Tx]): the MAS alignment of the mel to mu_x and its row sums."""
    return maximum_path_lengths(mas_log_prior(mu_x, y, x_mask, y_mask), x_lengths, y_lengths)


class _DurationLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logw, durations, x_mask, x_lengths):
        dev = logw.device
        B, Tx = durations.shape
        if logw.numel() != B * Tx or x_mask.numel() != B * Tx:
            raise ValueError(f"duration_loss: logw {tuple(logw.shape)}, x_mask {tuple(x_mask.shape)} and durations [B, Tx] = "
                             f"{(B, Tx)} do not agree")
        if logw.dtype != torch.float32:
            raise TypeError(f"duration_loss: logw must be fp32 (the loss and its gradient are computed in fp32), got {logw.dtype}")
        lw, d, m, xl = _f32(logw, dev), _f32(durations, dev), _f32(x_mask, dev), _i64(x_lengths, dev)
        loss = torch.empty((), device=dev)
        d_logw = torch.empty_like(lw)
        _call(dev, "us_duration_loss", lw, d, m, xl, loss, d_logw, B, Tx)
        ctx.save_for_backward(d_logw)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_logw,) = ctx.saved_tensors
        return d_logw * g, None, None, None


def duration_loss(logw, durations, x_mask, x_lengths):
    """train_STEP1.py:348-349: sum((logw - log(1e-8 + durations) x_mask)^2) / sum(x_lengths) with logw, x_mask [B, 1, Tx] and
    durations [B, Tx] (the row sums of MAS's attn); differentiable in logw, which must be fp32."""
    return _DurationLossFn.apply(logw, durations, x_mask, x_lengths)


def random_replace_tensor(spk_embs, replacement_emb, replace_percentage: float = 0.25):
    """`util.random_replace_tensor` (train_STEP1.py:325-326): int(replace_percentage * B) items, the first of `torch.randperm(B)` on
    the default CPU generator, are replaced by `replacement_emb`.  Works on a copy: the caller's tensor is left as it was."""
    out = spk_embs.clone()
    n = int(spk_embs.size(0) * replace_percentage)
    idx = torch.randperm(spk_embs.size(0))[:n]
    if n:
        out[idx.to(out.device)] = replacement_emb.detach().to(out).reshape((1,) + tuple(out.shape[1:]))
    return out


def compute_train_step_loss(text_encoder, duration_predictor, decoder, x, x_lengths, y, y_lengths, spk_emb, out_size, *,
                            spk_uncond: Optional[torch.Tensor] = None, starts: Optional[Sequence[int]] = None,
                            t: Optional[torch.Tensor] = None, aux: Optional[dict] = None):
    """`compute_train_step_loss` (train_STEP1.py:319-387) -> (dur_loss, prior_loss, diff_loss).  x [B, Tx] symbol ids, y [B, n_feats,
    Ty], spk_emb [B, 1, spk_emb_dim]; `spk_uncond` enables the speaker swap, `starts` fixes the crop offsets (else `random.choice`, as
    the reference), `t` the diffusion times (else `compute_loss` draws them).  Gradients reach the encoder through mu_x (prior and
    diffusion loss), the predictor through logw only (its input is detached), and every decoder parameter.  The [B, Tx, Ty] table
    stays on the device.  A dict given as `aux` receives attn, durations, y_mask and mu_y."""
    if spk_uncond is not None:
        spk_emb = random_replace_tensor(spk_emb, spk_uncond)
    mu_x, h, x_mask = text_encoder(x, x_lengths)
    logw = duration_predictor(h.detach(), x_mask, w=None, g=spk_emb, reverse=True)
    Ty = y.shape[-1]
    y_mask = (torch.arange(Ty, device=y.device).unsqueeze(0) < y_lengths.to(y.device).unsqueeze(1)).unsqueeze(1).to(x_mask.dtype)
    attn, durations = align(mu_x, y, x_mask, y_mask, x_lengths, y_lengths)
    dur_loss = duration_loss(logw, durations, x_mask, x_lengths)
    y_seg, seg_mask, mu_y = align_segment(mu_x, y, y_lengths, attn, out_size, starts)
    if t is None:
        diff_loss, _ = decoder.compute_loss(y_seg, seg_mask, mu_y, spk_emb=spk_emb)
    else:
        diff_loss, _ = decoder.loss_t(y_seg, seg_mask, mu_y, t, spk_emb)
    if aux is not None:
        aux.update(attn=attn, durations=durations, y_mask=seg_mask, mu_y=mu_y)
    return dur_loss, prior_loss(y_seg, mu_y, seg_mask), diff_loss
