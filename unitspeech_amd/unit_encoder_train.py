"""The unit-encoder step of `train_STEP2.py` (`compute_train_step_loss`, :238-305) in library launches.

A trainable HIP `Encoder` produces cond_x; `us_tts_align` turns the given unit durations into the hard alignment
(`generate_path`, :263); `us_finetune_segment` crops y and the aligned cond_x to one random window per item (:266-297; the
window offset comes from Python's `random.choice` exactly as in the reference); the frozen HIP decoder gives the diffusion loss
(:299) and `us_prior_loss` the prior loss (:302-303).  Both losses are differentiable back to the encoder's parameters:
`us_prior_loss`'s gradient and the decoder's d/d cond meet at mu_y, `us_finetune_segment_backward` carries them to cond_x,
`us_encoder_backward` to the weights.
"""
from __future__ import annotations

import random
from typing import Optional, Sequence

import torch

from ._args import call as _call, f32 as _f32

__all__ = ["prior_loss", "align_segment", "duration_path", "compute_train_step_loss"]


class _PriorLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, mu_y, y_mask):
        dev = mu_y.device
        B, F, T = mu_y.shape
        yy, mu, m = _f32(y, dev), _f32(mu_y, dev), _f32(y_mask, dev)
        loss = torch.empty((), device=dev)
        d_mu = torch.empty_like(mu)
        _call(dev, "us_prior_loss", yy, mu, m, loss, d_mu, B, F, T)
        ctx.save_for_backward(d_mu)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_mu,) = ctx.saved_tensors
        return None, d_mu * g, None


def prior_loss(y, mu_y, y_mask):
    """train_STEP2.py:302-303: sum(0.5 ((y - mu_y)^2 + log 2 pi) y_mask) / (sum(y_mask) n_feats); differentiable in mu_y."""
    return _PriorLossFn.apply(y, mu_y, y_mask)


class _SegmentAlignFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cond_x, y, attn, meta, segment_size):
        dev = cond_x.device
        B, F, Lu = cond_x.shape
        Ly = y.shape[-1]
        cx, yy, at = _f32(cond_x, dev), _f32(y, dev), _f32(attn, dev)
        y_cut = torch.empty(B, F, segment_size, device=dev)
        mu_y = torch.empty_like(y_cut)
        seg_mask = torch.empty(B, 1, segment_size, device=dev)
        _call(dev, "us_finetune_segment", cx, yy, at, meta[0], meta[1], y_cut, mu_y, seg_mask, B, F, Lu, Ly, segment_size)
        ctx.save_for_backward(at, meta)
        ctx.dims = (B, F, Lu, Ly, segment_size)
        ctx.mark_non_differentiable(y_cut, seg_mask)
        return y_cut, mu_y, seg_mask

    @staticmethod
    def backward(ctx, _g_y, g_mu, _g_mask):
        at, meta = ctx.saved_tensors
        B, F, Lu, Ly, S = ctx.dims
        if g_mu is None:
            return (None,) * 5
        g = _f32(g_mu, at.device)
        d_cx = torch.empty(B, F, Lu, device=at.device)
        _call(at.device, "us_finetune_segment_backward", g, at, meta[0], meta[1], d_cx, B, F, Lu, Ly, S)
        return d_cx, None, None, None, None


def duration_path(durations, x_mask, y_lengths, T):
    """`generate_path(duration, x_mask * y_mask)` (train_STEP2.py:261-263) through `us_tts_align`: attn [B, L, T] (0/1)."""
    dev = x_mask.device
    B, L = durations.shape
    w = _f32(durations, dev)
    xm = _f32(x_mask, dev).reshape(B, L)
    yl = y_lengths.to(device=dev, dtype=torch.int64).contiguous()
    dummy_x = torch.zeros(B, 1, L, device=dev)
    dummy_y = torch.empty(B, 1, T, device=dev)
    attn = torch.empty(B, L, T, device=dev)
    _call(dev, "us_tts_align", dummy_x, w, xm, yl, dummy_y, attn, None, B, 1, L, T)
    return attn


def align_segment(cond_x, y, y_lengths, attn, out_size, starts: Optional[Sequence[int]] = None):
    """train_STEP2.py:266-297: one window of out_size frames per item (offset `random.choice(range(0, y_length - out_size))`, 0 for
    shorter items; `starts` overrides it), no crop when out_size >= the longest y.  Returns (y, y_mask [B,1,S], mu_y) with mu_y =
    attn_cut^T cond_x differentiable in cond_x."""
    dev = cond_x.device
    B, Ly = y.shape[0], y.shape[-1]
    lens = [int(v) for v in y_lengths.cpu().tolist()]
    if len(lens) != B or any(n <= 0 or n > Ly for n in lens):
        raise ValueError(f"align_segment: y_lengths {lens} must hold {B} values in [1, {Ly}]")
    if out_size is None or out_size >= Ly:
        S, st = Ly, [0] * B
    else:
        S = int(out_size)
        st = list(starts) if starts is not None else [random.choice(range(0, n - S)) if n > S else 0 for n in lens]
    counts = [min(n, S) for n in lens]
    meta = torch.tensor([st, counts], dtype=torch.int64).to(dev)
    y_cut, mu_y, seg_mask = _SegmentAlignFn.apply(cond_x, y, attn, meta, S)
    return y_cut, seg_mask, mu_y


def compute_train_step_loss(unit_encoder, decoder, x_unit, x_unit_lengths, durations, y, y_lengths, spk_emb, out_size,
                            starts: Optional[Sequence[int]] = None, t: Optional[torch.Tensor] = None):
    """`compute_train_step_loss` (train_STEP2.py:238-305) -> (prior_loss, diff_loss).  durations [B, L_units] (frames per unit,
    0 on padding), y [B, n_feats, T], spk_emb [B, 1, spk_emb_dim]; `t` fixes the diffusion times (else `compute_loss` draws them)."""
    cond_x, _, x_mask = unit_encoder(x_unit, x_unit_lengths)
    attn = duration_path(durations, x_mask, y_lengths, y.shape[-1])
    y_seg, y_mask, mu_y = align_segment(cond_x, y, y_lengths, attn, out_size, starts)
    if t is None:
        diff_loss, _ = decoder.compute_loss(y_seg, y_mask, mu_y, spk_emb=spk_emb)
    else:
        diff_loss, _ = decoder.loss_t(y_seg, y_mask, mu_y, t, spk_emb)
    return prior_loss(y_seg, mu_y, y_mask), diff_loss
