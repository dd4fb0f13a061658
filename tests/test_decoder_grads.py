"""What the element-wise bar of tests/test_decoder_grads_gpu.py sees and the older bars do not (CPU only; the counterpart of
tests/test_wino_torch.py for the training backward).

The fp64 oracle gradients of one case of the table (T = 128, lengths [128, 121]) get three defects planted by arithmetic: the affected
parameter gradient is recomputed from the layer's saved input and the gradient w.r.t. its output in plain torch (checked against autograd
first), minus or plus the planted piece.  For each the old measures are printed -- the per-tensor relative L2 (bar 1e-4,
test_pretraining_batch_loss_and_every_gradient_vs_oracle_autograd) and the same over the odd-strided sample of that test's fp64 golden --
then the new one, max |planted - fp64| against max(10 x max |fp32 oracle - fp64|, 1e-5 x max |fp64|)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import grad_parity as GP      # noqa: E402

CASE = "T128_128_121"
CONV1 = "estimator.final_block.block.0.weight"             # 128 -> 128, 3x3, level 0
CONV2 = "estimator.downs.0.1.block2.block.0.weight"        # 128 -> 128, 3x3, level 0
GAMMA = "estimator.final_block.block.1.weight"             # the GroupNorm behind CONV1
OLD_BAR = 1e-4


@pytest.fixture(scope="module")
def ref():
    sd_np, inputs = GP.case_weights(CASE), GP.case_inputs(CASE)
    l64, r64, cap = GP.oracle_grads(sd_np, inputs, torch.float64, capture=(CONV1, CONV2, GAMMA))
    l32, r32 = GP.oracle_grads(sd_np, inputs, torch.float32)
    return inputs, r64, r32, GP.floors_of(r32, r64), cap


def measures(tag, name, planted, r64, floors):
    rel, samp = GP.rel_l2(planted, r64[name]), GP.sample_rel_l2(planted, r64[name])
    err, bar = float((planted - r64[name]).abs().max()), GP.bar_of(name, r64[name], floors[name])
    print(f"\n{tag}\n    {name}: relative L2 {rel:.2e}, over the golden's sample {samp:.2e} (old bar {OLD_BAR:.0e}: "
          f"{'passes' if max(rel, samp) <= OLD_BAR else 'fails'}) | max err {err:.2e}, bar {bar:.2e}: missed {err / bar:.1f}x")
    return rel, samp, err, bar


def pixel_range_end(shape, B, which):
    """The last pixel (row, column) of the which-th pixel range of an item, as wgrad_chunk cuts a 3x3 convolution's pixels."""
    Co, Ci, H, W = shape
    chunk = GP.wgrad_chunk(H * W, Co, Ci, 9, B)
    m = min((which + 1) * chunk, H * W) - 1
    return divmod(m, W)


def test_the_bar_and_the_order_cover_every_tensor(ref):
    """The fp32 oracle is within the bar of the fp64 oracle with 10x to spare, by construction; all 231 tensors are judged, none is zero;
    the fp64 oracle's grad_x0 / grad_cond are exactly 0 in masked columns."""
    inputs, r64, r32, floors, _ = ref
    assert len(r64) == 231 and len([n for n in r64 if n.startswith("estimator.")]) == 228
    assert GP.backward_order(r64.keys())[0] == "estimator.final_conv.weight"
    assert all(float(g.abs().max()) > 0 for g in r64.values())
    rows, misses = GP.judge(r32, r64, floors, tag="fp32 oracle")
    assert not misses and len(rows) == 231
    assert max(err / bar for _, err, _, bar in rows) <= 0.1 + 1e-12
    assert sum(1 for n in r64 if GP.is_gain(n)) == 8
    pad = (inputs[1] == 0).expand_as(r64["grad_x0"])
    assert bool(pad.any()) and float(r64["grad_x0"][pad].abs().max()) == 0.0 and float(r64["grad_cond"][pad].abs().max()) == 0.0


def test_a_tile_that_drops_the_last_pixel_of_its_range(ref):
    """One 64 x 64 tile (output channels 0..63, input channels 0..63, tap (-1, -1)) of a 3x3 weight gradient lacks the last pixel of item
    1's second pixel range: what a weight-gradient workgroup with `<` for `<=` at the end of its range leaves behind."""
    _, r64, _, floors, cap = ref
    x, gy = cap[CONV1]
    B, _, H, W = gy.shape
    xp = F.pad(x, (1, 1, 1, 1))
    tile = torch.einsum("bohw,bihw->oi", gy[:, :64], xp[:, :64, 0:H, 0:W])
    assert float((tile - r64[CONV1][:64, :64, 0, 0]).abs().max()) <= 1e-12 * float(r64[CONV1].abs().max())     # the recomputation is autograd's
    y, c = pixel_range_end((128, 128, H, W), B, 1)
    planted = r64[CONV1].clone()
    planted[:64, :64, 0, 0] = tile - gy[1, :64, y, c][:, None] * xp[1, :64, y, c][None, :]
    rel, samp, err, bar = measures(f"tile (0..63, 0..63, tap (-1,-1)) without pixel ({y}, {c}) of item 1", CONV1, planted, r64, floors)
    assert err > bar
    assert max(rel, samp) <= OLD_BAR          # ... and the old bars let it through


def test_one_tap_of_one_row_read_from_the_neighbouring_pixel(ref):
    """Output channel 5, tap (0, +1) of a 3x3 weight gradient: at one pixel (the last of item 1's first range) the activation comes from
    one column further right -- a coordinate carried one step too far at the end of a range."""
    _, r64, _, floors, cap = ref
    x, gy = cap[CONV2]
    B, _, H, W = gy.shape
    xq = F.pad(x, (1, 2, 1, 1))
    co, ky, kx = 5, 1, 2
    row = torch.einsum("bhw,bihw->i", gy[:, co], xq[:, :, ky:ky + H, kx:kx + W])
    assert float((row - r64[CONV2][co, :, ky, kx]).abs().max()) <= 1e-12 * float(r64[CONV2].abs().max())
    y, c = pixel_range_end((128, 128, H, W), B, 0)
    planted = r64[CONV2].clone()
    planted[co, :, ky, kx] = row + gy[1, co, y, c] * (xq[1, :, y + ky, c + kx + 1] - xq[1, :, y + ky, c + kx])
    rel, samp, err, bar = measures(f"row {co}, tap (0,+1): pixel ({y}, {c}) of item 1 reads column {c + 2}", CONV2, planted, r64, floors)
    assert err > bar
    assert max(rel, samp) <= OLD_BAR


def test_one_item_missing_from_one_channel_of_a_groupnorm_gamma_gradient(ref):
    """Channel 127 of a GroupNorm weight gradient without item 1's contribution (a per-item partial sum that is never added).  This one the
    old per-tensor bar sees as well (one element of 128 off by its own size): printed, not asserted."""
    _, r64, _, floors, cap = ref
    y, g = cap[GAMMA]
    B, C = y.shape[:2]
    yg = y.reshape(B, GP.O.GROUPS, -1)
    xhat = ((yg - yg.mean(-1, keepdim=True)) / torch.sqrt(yg.var(-1, unbiased=False, keepdim=True) + 1e-5)).reshape(y.shape)
    per_item = (g * xhat).sum((2, 3))
    assert float((per_item.sum(0) - r64[GAMMA]).abs().max()) <= 1e-12 * float(r64[GAMMA].abs().max())
    planted = per_item.sum(0)
    planted[C - 1] -= per_item[1, C - 1]
    rel, samp, err, bar = measures(f"channel {C - 1} without item 1", GAMMA, planted, r64, floors)
    assert err > bar


def test_the_case_table_reaches_both_values_of_every_weight_gradient_branch():
    """launch_wgrad's kernel switch (level width >= 16 or not), the writer (overwrite / add without atomics / zero fill + atomics) and the
    pixel cut (per item / one range across the items), restated in tools/grad_parity.py: each value at full width in some case."""
    seen = set()
    for cid, T, lengths, _ in GP.CASES.values():
        seen |= {(k, w) for (_, k, w) in GP.wgrad_table(T, len(lengths))}
    assert {k for k, _ in seen} == {"T", "F"}
    assert {w for _, w in seen} == {"ow", "rmw", "at", "v-rmw", "v-at"}
    for w in ("ow", "at", "v-at"):
        assert ("T", w) in seen and ("F", w) in seen
    # T = 176, the only width of the older tests: the carried-coordinate kernel alone
    assert {k for (_, k, _) in GP.wgrad_table(176, 1)} | {k for (_, k, _) in GP.wgrad_table(176, 8)} == {"T"}
    assert GP.wgrad_chunk(220, 1024, 1024, 9, 1) == 224 and GP.wgrad_chunk(14080, 128, 128, 9, 1) == 640      # train_host.inc's own examples
