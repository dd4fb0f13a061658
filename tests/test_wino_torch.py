"""tools/wino_torch.py, the CPU restatement of the Winograd forms that tests/test_decoder_blocks_gpu.py takes its fp32 floors from.

1. Identity: in fp64 with nothing rounded, each form IS the convolution (1e-12 of max |ref|), at image sizes with a single almost empty
   tile column, partial last tiles along both axes and a long row, Cin != Cout.
2. The element-wise bar of the GPU tests, max |got - fp64| <= max(10 x max |fp32 restatement at 22 bits - fp64|, 1e-5 max |fp64|), sees three
   local defects of the kind tiled kernels have, each planted in the fp64 restatement of one 512 x 20 x 34 `Block`; every one misses the bar
   by more than a factor of 10.  The relative L1 that the older decoder tests judge by (bar 2e-6) is printed beside it.
3. Floors: per form, max |fp32 restatement at 22 bits - fp64| against max |fp32 conv2d - fp64| on the same inputs (DESIGN.md quotes them)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wino_torch as WT      # noqa: E402

FORMS = (22, 44, 24)
OLD_BAR = 2e-6


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("H,W", [(10, 1), (10, 5), (20, 34), (40, 4)])
def test_each_form_is_the_convolution_in_fp64(form, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 12, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(20, 12, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(20, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, b, padding=1)
    got = WT.conv3x3_wino(x, w, b, form, torch.float64, None)
    assert got.shape == ref.shape
    e = float((got - ref).abs().max() / ref.abs().max())
    print(f"\nform {form} {H}x{W}: max |restatement - conv2d| / max |ref| = {e:.2e}")
    assert e <= 1e-12


def test_split22_is_the_two_plane_value():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -12, 3.14159274, -1234.56787, 1e-3 / 32, 6e-8], dtype=torch.float32)
    v = WT.split22(x)
    hi = x.half().float()
    assert torch.equal(v, hi + ((x - hi) * 2048).half().float() / 2048)
    assert float(((v - x).abs() / x.abs())[:4].max()) <= 2.0 ** -21        # 22 bits where hi is a normal fp16 number


# ---- 2. planted defects ---------------------------------------------------------------------------------------------------------------
C, H, W, B, FORM, P = 512, 20, 34, 2, 44, "blk"


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(7)
    sd = {f"{P}.block.0.weight": torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5, f"{P}.block.0.bias": (torch.rand(C, generator=g) * 2 - 1) / (9 * C) ** 0.5,
          f"{P}.block.1.weight": 1 + 0.1 * torch.randn(C, generator=g), f"{P}.block.1.bias": 0.1 * torch.randn(C, generator=g)}
    x = torch.randn(B, C, H, W, generator=g)
    mask = torch.ones(B, 1, 1, W)
    mask[1, :, :, W - 2:] = 0              # item 1 padded by 8 frames: 2 columns at level 2
    ref = WT.block_wino(sd, P, x, mask, None, torch.float64)
    floor = float((WT.block_wino(sd, P, x, mask, FORM, torch.float32, 22).double() - ref).abs().max())
    bar = max(10 * floor, 1e-5 * float(ref.abs().max()))
    return sd, x, mask, ref, floor, bar


def mutated(sd, x, mask, which):
    """The fp64 restatement of the Block with one defect planted."""
    xm = x.double() * mask.double()
    tiles = WT.wino_tiles(xm, FORM).clone()
    mh, mw = WT.TILE[FORM]
    tw = tiles.shape[3]
    if which == "tap":
        # tile (1, last): its top row, the first column outside the image.  A linear address one past a row's end is the next row's first pixel
        ty, q = 1, W - mw * (tw - 1) + 1
        assert mw * (tw - 1) - 1 + q == W and float(tiles[:, :, ty, tw - 1, 0, q].abs().max()) == 0.0
        tiles[0, 8:12, ty, tw - 1, 0, q] = xm[0, 8:12, mh * ty - 1 + 1, 0]          # one channel quad of item 0: what one thread of the transform loads
    y_full = WT.wino_from_tiles(tiles, sd[f"{P}.block.0.weight"], sd[f"{P}.block.0.bias"], FORM, torch.float64, None)
    y = y_full[:, :, :H, :W].clone()
    if which == "bias":
        o = int((sd[f"{P}.block.0.bias"].abs() - 0.005).abs().argmin())           # a bias of typical size, 0.005 (the largest is 0.0147)
        y[:, o, H - 1, :] -= sd[f"{P}.block.0.bias"][o].double()
    out = WT.block_tail(sd, P, y, mask)
    if which == "gn":
        # group 3 of item 1: mean and variance over the whole tile grid, the two columns outside the image included
        cg = C // WT.GROUPS
        ch = slice(3 * cg, 4 * cg)
        assert y_full.shape[-1] == W + 2
        m, v = y_full[1, ch].mean(), y_full[1, ch].var(unbiased=False)
        n = (y[1, ch] - m) / torch.sqrt(v + 1e-5)
        n = n * sd[f"{P}.block.1.weight"][ch].double()[:, None, None] + sd[f"{P}.block.1.bias"][ch].double()[:, None, None]
        out[1, ch] = WT.mish(n) * mask[1].double()
    return out


def test_the_restatement_itself_meets_the_bar(case):
    sd, x, mask, ref, floor, bar = case
    e = float((mutated(sd, x, mask, None) - ref).abs().max())
    print(f"\nno defect: max |fp64 restatement - fp64 oracle| {e:.2e}; floor {floor:.2e}, bar {bar:.2e}")
    assert e <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("which", ["tap", "bias", "gn"])
def test_the_elementwise_bar_sees_a_planted_defect(case, which):
    sd, x, mask, ref, floor, bar = case
    d = (mutated(sd, x, mask, which) - ref).abs()
    e, l1 = float(d.max()), float(d.mean() / ref.abs().mean())
    at = [int(v) for v in torch.unravel_index(d.argmax(), d.shape)]
    print(f"\ndefect '{which}': max |err| {e:.2e} at (item, channel, row, column) {at} = {e / bar:.0f} x the element-wise bar {bar:.2e} (floor {floor:.2e}); "
          f"relative L1 {l1:.2e} = {l1 / OLD_BAR:.2f} x the old bar {OLD_BAR:.0e}: {'ALSO above' if l1 > OLD_BAR else 'BELOW'} it")
    assert e >= 10 * bar


# ---- 3. floors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_floors_of_the_forms(form):
    (wm, wa), (dm, da), (rm, ra) = WT.floors(form)
    print(f"\nform {form} at 512 x 20 x 34: max |fp32 restatement at 22 bits - fp64| {wm:.3e}, max |fp32 conv2d - fp64| {dm:.3e}, ratio {wm / dm:.2f} "
          f"(means {wa:.3e} / {da:.3e}, ratio {wa / da:.2f}); max |fp64| {rm:.2f}")
    # a restatement that were not the convolution would be off by O(max |ref|); rounding alone stays far below 1e-4 of it
    assert 0 < wm <= 1e-4 * rm and 0 < dm <= wm * 4
