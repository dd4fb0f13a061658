#!/usr/bin/env python3
"""CPU restatement, in plain torch, of the Winograd forms the decoder's stride-1 3x3 convolutions run in (csrc/wino.hip, csrc/wino4.hip):
F(2x2,3x3) on the points {0, +-1, inf} (form 22), F(4x4,3x3) on {0, +-5/8, +-3/2, inf} (form 44) and F(2x4,3x3), F(2,3) down the rows and
F(4,3) along them (form 24).  TEST INFRASTRUCTURE ONLY: the forms change the rounding of a convolution, so the fair fp32 floor of a kernel
that runs one is this restatement in fp32, not `F.conv2d` in fp32.

    V = B^T d B          in `dtype`, along W first and then along H, as the kernels do
    U = G g G^T          in fp64, rounded once
    M[f] = V[f] U[f]     one product-sum over the input channels per frequency f = (i, j), in `dtype`
    Y = A^T M A + bias   in `dtype`

Tile grid ceil(H / MH) x ceil(W / MW); taps outside the image read zeros, outputs outside it are dropped.  The matrices come from
`gen_wino4_coef.cook_toom_exact`, which tests/test_host_logic.py pins to csrc/wino4_coef.h.

operand_bits = 22 rounds V and U to the two-plane operand hi + lo 2^-11 of the f16x3 GEMM (`f16x3_emulation.split16`); None rounds nothing.
With 22 bits the 4-wide forms scale their INPUT by 2^-5 and Y by 2^5, as wino4.hip does to keep V inside the fp16 range: a power of two,
so nothing changes but the values whose scaled `hi` is an fp16 subnormal (below about 2e-3 of activation), and those the model must follow.

    python tools/wino_torch.py        # the element-wise and mean floors of the three forms at 512 x 20 x 34"""
import os
import sys
from collections import OrderedDict
from typing import Mapping, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f16x3_emulation import split16          # noqa: E402
from gen_wino4_coef import cook_toom_exact   # noqa: E402

Tensor = torch.Tensor
GROUPS = 8
POINTS = {2: (0, 1, -1), 4: (0, "5/8", "-5/8", "3/2", "-3/2")}
TILE = {22: (2, 2), 44: (4, 4), 24: (2, 4)}      # form -> (MH, MW)


def matrices(m: int):
    """(A^T [m x n], G [n x 3], B^T [n x n]) of F(m, 3) as fp64 tensors, n = m + 2."""
    from fractions import Fraction as Fr
    AT, G, BT = cook_toom_exact([Fr(p) for p in POINTS[m]], m)
    t = lambda X: torch.tensor([[float(v) for v in row] for row in X], dtype=torch.float64)
    return t(AT), t(G), t(BT)


def split22(x: Tensor) -> Tensor:
    """x as the value hi + lo 2^-11 its two fp16 planes carry (hi = fp16(x), lo = fp16((x - hi) 2^11)), in x's dtype."""
    hi, lo = split16(x.detach().numpy())
    return (torch.from_numpy(hi).double() + torch.from_numpy(lo).double() / 2048.0).to(x.dtype)


def wino_tiles(x: Tensor, form: int) -> Tensor:
    """The (MH + 2) x (MW + 2) input tiles of x [B, C, H, W], zeros outside the image: [B, C, th, tw, MH + 2, MW + 2]."""
    mh, mw = TILE[form]
    H, W = x.shape[-2:]
    th, tw = -(-H // mh), -(-W // mw)
    xp = F.pad(x, (1, tw * mw + 1 - W, 1, th * mh + 1 - H))
    return xp.unfold(2, mh + 2, mh).unfold(3, mw + 2, mw)


_PACKS: "OrderedDict" = OrderedDict()      # the last few U = G g G^T: a test walks one convolution through many image sizes


def _packed_weights(w: Tensor, form: int, dtype: torch.dtype, operand_bits: Optional[int]) -> Tensor:
    """U = G g G^T in fp64, rounded once (to the two-plane value, or to `dtype`): [NH * NW, Cin, Cout]."""
    key = (tuple(w.shape), w.dtype, form, dtype, operand_bits, float(w.double().sum()), float(w.double().abs().sum()))      # (by content)
    if key in _PACKS:
        _PACKS.move_to_end(key)
        return _PACKS[key]
    mh, mw = TILE[form]
    Gh, Gw = matrices(mh)[1], matrices(mw)[1]
    U = torch.matmul(Gh, torch.matmul(w.double(), Gw.T))          # [Cout, Cin, nh, nw]
    U = split22(U.float().contiguous()).to(dtype) if operand_bits else U.to(dtype)
    U = U.permute(2, 3, 1, 0).reshape(-1, w.shape[1], w.shape[0]).contiguous()
    _PACKS[key] = U
    while len(_PACKS) > 8:
        _PACKS.popitem(last=False)
    return U


def wino_from_tiles(tiles: Tensor, w: Tensor, bias: Optional[Tensor], form: int, dtype: torch.dtype = torch.float64,
                    operand_bits: Optional[int] = None, in_scale: Optional[float] = None) -> Tensor:
    """The convolution from its input tiles: the whole tile grid's outputs [B, Cout, th * MH, tw * MW], those outside the image included."""
    assert operand_bits in (None, 22)
    mh, mw = TILE[form]
    (ATh, _, BTh), (ATw, _, BTw) = matrices(mh), matrices(mw)
    if in_scale is None:
        in_scale = 2.0 ** -5 if operand_bits and form != 22 else 1.0
    B, C, th, tw, nh, nw = tiles.shape
    d = tiles.to(dtype) * in_scale
    V = torch.matmul(BTh.to(dtype), torch.matmul(d, BTw.to(dtype).T))                # [B, C, th, tw, nh, nw]
    if operand_bits:
        V = split22(V.float().contiguous()).to(dtype)
    Uf = _packed_weights(w, form, dtype, operand_bits)                              # [nh * nw, C, Cout]
    Vf = V.permute(4, 5, 0, 2, 3, 1).reshape(nh * nw, B * th * tw, C)
    M = torch.bmm(Vf, Uf).reshape(nh, nw, B, th, tw, -1).permute(2, 5, 3, 4, 0, 1)   # [B, Cout, th, tw, nh, nw]
    Y = torch.matmul(ATh.to(dtype), torch.matmul(M, ATw.to(dtype).T))               # [B, Cout, th, tw, mh, mw]
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, th * mh, tw * mw)
    if in_scale != 1.0:
        Y = Y * (1.0 / in_scale)
    return Y if bias is None else Y + bias.to(dtype)[None, :, None, None]


def conv3x3_wino(x: Tensor, w: Tensor, bias: Optional[Tensor], form: Optional[int], dtype: torch.dtype = torch.float64,
                 operand_bits: Optional[int] = None) -> Tensor:
    """conv2d(x, w, bias, padding=1) in the Winograd form 22, 44 or 24; form None: the direct convolution in `dtype`."""
    if form is None:
        return F.conv2d(x.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), padding=1)
    H, W = x.shape[-2:]
    return wino_from_tiles(wino_tiles(x, form), w, bias, form, dtype, operand_bits)[:, :, :H, :W]


def mish(x: Tensor) -> Tensor:
    return x * torch.tanh(F.softplus(x))


def block_tail(sd: Mapping[str, Tensor], p: str, y: Tensor, mask: Tensor) -> Tensor:
    """What `Block` does with its convolution's output: mish(GroupNorm8(y)) * mask."""
    dt = y.dtype
    return mish(F.group_norm(y, GROUPS, sd[f"{p}.block.1.weight"].to(dt), sd[f"{p}.block.1.bias"].to(dt), eps=1e-5)) * mask.to(dt)


def block_wino(sd: Mapping[str, Tensor], p: str, x: Tensor, mask: Tensor, form: Optional[int], dtype: torch.dtype = torch.float64,
               operand_bits: Optional[int] = None) -> Tensor:
    """`oracle.decoder_oracle.block` with the convolution in the given form."""
    y = conv3x3_wino(x.to(dtype) * mask.to(dtype), sd[f"{p}.block.0.weight"], sd[f"{p}.block.0.bias"], form, dtype, operand_bits)
    return block_tail(sd, p, y, mask)


def resnet_block_wino(sd: Mapping[str, Tensor], p: str, x: Tensor, mask: Tensor, temb: Tensor, form1: Optional[int], form2: Optional[int],
                      dtype: torch.dtype = torch.float64, operand_bits: Optional[int] = None) -> Tensor:
    """`oracle.decoder_oracle.resnet_block` with block1's convolution in form1 and block2's in form2 (res_conv is a 1x1: no form)."""
    x, mask, temb = x.to(dtype), mask.to(dtype), temb.to(dtype)
    h = block_wino(sd, f"{p}.block1", x, mask, form1, dtype, operand_bits)
    h = h + F.linear(mish(temb), sd[f"{p}.mlp.1.weight"].to(dtype), sd[f"{p}.mlp.1.bias"].to(dtype))[:, :, None, None]
    h = block_wino(sd, f"{p}.block2", h, mask, form2, dtype, operand_bits)
    if f"{p}.res_conv.weight" in sd:
        return h + F.conv2d(x * mask, sd[f"{p}.res_conv.weight"].to(dtype), sd[f"{p}.res_conv.bias"].to(dtype))
    return h + x * mask


def floors(form: int, C: int = 512, Co: int = 512, H: int = 20, W: int = 34, B: int = 2, seed: int = 0):
    """(max, mean) |fp32 restatement at 22 bits - fp64| and (max, mean) |fp32 conv2d - fp64| on the same inputs, and max / mean |fp64|."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ew = (conv3x3_wino(x, w, b, form, torch.float32, 22).double() - ref).abs()
    ed = (F.conv2d(x, w, b, padding=1).double() - ref).abs()
    return (float(ew.max()), float(ew.mean())), (float(ed.max()), float(ed.mean())), (float(ref.abs().max()), float(ref.abs().mean()))


if __name__ == "__main__":
    for form in (22, 44, 24):
        (wm, wa), (dm, da), (rm, ra) = floors(form)
        print(f"form {form}: max |fp32 restatement at 22 bits - fp64| {wm:.3e} (mean {wa:.3e}); max |fp32 conv2d - fp64| {dm:.3e} (mean {da:.3e}); "
              f"ratio max {wm / dm:.2f}, mean {wa / da:.2f}; max |fp64| {rm:.2f}, mean {ra:.3f}")
