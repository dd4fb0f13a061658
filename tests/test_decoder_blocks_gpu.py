"""The decoder's inference forward, block by block through `us_debug_block`, judged ELEMENT BY ELEMENT against the fp64 oracle.

Every older forward test of this code (test_hip_parity*.py, test_wino*_gpu.py, test_split_store_gpu.py) judges a mean absolute error
against 2e-6; a mean over 10^5..10^6 outputs does not see one wrong tap at a tile corner, a partial last tile column that reads its
neighbour, or one GroupNorm group that counts a column outside the image (tests/test_wino_torch.py plants such defects and shows it).

Bar (the rule of tests/test_sampler_gpu.py `bar2` and tests/test_hubert_gpu.py `check`):

    max |library - fp64| <= max(10 x max |fp32 reference - fp64|, 1e-5 x max |fp64|)

The fp32 reference of a convolution that runs a Winograd form is that form's restatement in fp32 with 22-bit operands
(tools/wino_torch.py); of a direct convolution, and of everything on the exact-fp32 handle, the oracle in fp32.  Same inputs.
Every case prints err, floor, bar and the (item, channel, row, column) of its worst element; a test collects its misses and asserts once.

Full-size weights (`synthetic_state_dict(DecoderConfig(), 0)`), one handle per form set for the whole module:

    handle    US_WINO4        3x3 convolutions with Cin >= 256 at level 1 / 2 / 3        (Cin < 256 at levels >= 1: F(2x2), f16x3 operands)
    default   "0,44,44,24"    F(4x4) / F(4x4) / F(2x4)
    swap      "0,24,24,44"    F(2x4) / F(2x4) / F(4x4)
    f22       "0,0,0,0"       F(2x2) everywhere
    exact     (exact fp32)    F(2x2) with fp32 operands
    g1, g1x   default and exact, every Rezero gain 1 (the attention cases: at the synthetic 0.01 the branch is below the rounding of x + branch)
    nofuse    "0,44,0,24" and US_WINO_FUSE_GN=0: block1's GroupNorm as a pass of its own, one ResnetBlock per form
    level 0, and every convolution with Cout <= dim (the last up level, ups.2.*): the direct f16x3 implicit GEMM on all handles but exact.

T in {8, 24, 32, 40, 136}: widths 1, 3, 4, 5, 17 at level 3 (H = 10: 2.5 tiles of F(4x4)), 2, 6, 8, 10, 34 at level 2, 4, 12, 16, 20, 68 at
level 1 -- a single almost empty tile column, one under / exactly on / one over a tile, a long row with a partial end.  B = 2 with item 1
padded by 8 frames (T = 8: by 4); B = 5 once per kind, so that the row count of a GEMM is no multiple of 64."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import decoder_oracle as O
from unitspeech_amd import DecoderConfig, UnitSpeech, _lib, synthetic_state_dict

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wino_torch as WT      # noqa: E402

pytestmark = pytest.mark.gpu

FULL = DecoderConfig()
DEV = "cuda:0"
DIM, NF = FULL.dim, FULL.n_feats
TD = FULL.dim + FULL.spk_emb_dim
WIDTHS = [8, 24, 32, 40, 136]
SENTINEL = -1.2345e30
TAIL = 4096
FORMSETS = {"default": "0,44,44,24", "swap": "0,24,24,44", "f22": "0,0,0,0", "nofuse": "0,44,0,24"}


def make_model(sd_np, cfg=FULL):
    m = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    return m.to(DEV).eval()


class Handle:
    def __init__(self, name, eng, forms, exact, model):
        self.name, self.eng, self.forms, self.exact, self.model = name, eng, forms, exact, model
        self.ws = {}

    def form(self, level, cin, cout):
        """The form the library runs a stride-1 3x3 convolution of a ResnetBlock in (decoder.hip: want_wino, kWino4MinK); None = direct."""
        if level < 1 or cout <= DIM or self.exact:
            return None          # (the exact handle runs F(2x2) with fp32 operands: its floor is the fp32 oracle's)
        return self.forms[level] if self.forms[level] in (44, 24) and cin >= 256 else 22


@pytest.fixture(scope="module")
def sd_np():
    return synthetic_state_dict(FULL, 0)


@pytest.fixture(scope="module")
def sds(sd_np):
    return O.to_torch(sd_np), O.to_torch(sd_np, torch.float64)


def rezero_one(sd):
    return {k: (v * 0 + 1 if k.endswith(".fn.g") else v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def sds_g1(sds):
    return rezero_one(sds[0]), rezero_one(sds[1])


@pytest.fixture(scope="module")
def handles(sd_np):
    """One engine per form set, weights packed once.  US_WINO4 / US_WINO_FUSE_GN are read when the handle is created."""
    out, keep = {}, []
    dev = torch.device(DEV)
    for name, spec in FORMSETS.items():
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("US_WINO4", spec)
            if name == "nofuse":
                mp.setenv("US_WINO_FUSE_GN", "0")
            model = make_model(sd_np)
            out[name] = Handle(name, model._sync(dev), [int(v) for v in spec.split(",")], False, model)
            keep.append(model)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("US_WINO4", raising=False)
        out["exact"] = Handle("exact", keep[0]._sync(dev, exact=True), [0, 0, 0, 0], True, keep[0])
        # the attention cases: every Rezero gain 1 instead of the synthetic weights' 0.01, under which out = x + 0.01 fn(x) is x's own rounding
        g1 = make_model(rezero_one(sd_np))
        out["g1"] = Handle("g1", g1._sync(dev), [0, 44, 44, 24], False, g1)
        out["g1x"] = Handle("g1x", g1._sync(dev, exact=True), [0, 0, 0, 0], True, g1)
    assert out["exact"].eng.exact and not out["default"].eng.exact and out["g1x"].eng.exact
    yield out
    torch.cuda.synchronize()


MAIN = ("default", "swap", "f22", "exact")


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def call(h, kind, prefix, level, x_dev, mask_bt, temb, out_shape):
    """us_debug_block into a sentinel-filled buffer with TAIL sentinel floats behind it; returns the output [.., C] on the host after checking
    that every element was written and none behind the end was."""
    eng, lib = h.eng, h.eng.lib
    B, T = mask_bt.shape
    n = int(np.prod(out_shape))
    buf = torch.full((n + TAIL,), SENTINEL, device=DEV)
    key = (B, T)
    if key not in h.ws:
        h.ws[key] = torch.empty(int(lib.us_workspace_bytes(eng.handle, B, T)), dtype=torch.uint8, device=DEV)
    ws = h.ws[key]
    m = mask_bt.contiguous().to(DEV)
    te = temb.contiguous().to(DEV) if temb is not None else None
    rc = lib.us_debug_block(eng.handle, kind, prefix.encode(), level, C.c_void_p(x_dev.data_ptr()), C.c_void_p(m.data_ptr()),
                            C.c_void_p(te.data_ptr()) if te is not None else None, C.c_void_p(buf.data_ptr()), B, T, C.c_void_p(ws.data_ptr()),
                            ws.numel(), None)
    _lib.check(rc, eng.handle, "us_debug_block")
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[n:] == SENTINEL).all()), f"{h.name} {prefix}: wrote behind the output's end"
    left = int((buf[:n] == SENTINEL).sum())
    assert left == 0, f"{h.name} {prefix}: {left} output elements never written"
    return buf[:n].reshape(out_shape)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(y):
    return y.permute(0, 3, 1, 2)


def judge(misses, tag, got, r64, r32, zero_mask=None):
    """Prints err / floor / bar / place of the worst element; appends to `misses` what is over the bar.  zero_mask [B,1,1,W]: the level's
    frame mask."""
    d = (got.double() - r64).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    err, floor, top = float(d.max()), float((r32.double() - r64).abs().max()), float(r64.abs().max())
    bar = max(10 * floor, 1e-5 * top)
    at = tuple(int(v) for v in torch.unravel_index(d.argmax(), d.shape))
    print(f"{tag}: err {err:.3e} floor {floor:.3e} bar {bar:.3e} ({err / bar:.2f} of it) at (item, channel, row, column) {at}, max |fp64| {top:.2f}")
    if not err <= bar:
        misses.append(f"{tag}: err {err:.3e} > bar {bar:.3e} (floor {floor:.3e}) at {at}")
    if zero_mask is not None:
        # wherever the module masks -- the reference is exactly 0 in a padded column -- so must the library be (a ResnetBlock with a res_conv
        # does not: its padded columns hold res_conv's bias)
        z = ((1 - zero_mask) > 0).expand_as(r64) & (r64 == 0)
        leak = float(got[z].abs().max()) if bool(z.any()) else 0.0
        if leak != 0.0:
            misses.append(f"{tag}: masked columns hold {leak:.3e}, not 0")


def masks(B, T, level, ones=False):
    """(full-resolution [B, T], the level's [B, 1, 1, W]); item 1 padded by 8 frames (T = 8: by 4), B = 5: items 1 and 3 padded, item 4 by 16"""
    full = torch.ones(B, T)
    if not ones:
        pad = 8 if T > 8 else 4
        for b in range(1, B, 2):
            full[b, T - pad:] = 0
        if B > 4 and T > 16:
            full[4, T - 16:] = 0
    return full, full[:, ::(1 << level)].reshape(B, 1, 1, -1).clone()


def rand(key, *shape):
    g = np.random.Generator(np.random.Philox(key=key))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32))


def geom(level, T):
    return NF >> level, T >> level


# ---- ResnetBlock and Block --------------------------------------------------------------------------------------------------------------
# (prefix, the module's level, Cin, Cout)
RES = [("estimator.downs.0.1", 0, 128, 128), ("estimator.downs.1.0", 1, 128, 256), ("estimator.downs.1.1", 1, 256, 256),
       ("estimator.downs.2.0", 2, 256, 512), ("estimator.downs.2.1", 2, 512, 512), ("estimator.downs.3.0", 3, 512, 1024),
       ("estimator.downs.3.1", 3, 1024, 1024), ("estimator.mid_block1", 3, 1024, 1024), ("estimator.ups.0.0", 3, 2048, 512),
       ("estimator.ups.2.0", 1, 512, 128), ("estimator.ups.2.1", 1, 128, 128)]


@functools.lru_cache(maxsize=4)
def res_inputs(prefix, level, cin, T, B):
    H, W = geom(level, T)
    key = 1000 * level + T + 7 * B + len(prefix)
    return rand(key, B, cin, H, W), rand(key + 1, B, TD)


def resnet_refs(sds, prefix, level, x, mk, temb, combos):
    """fp64 oracle, and per (form1, form2) the fp32 reference"""
    sd32, sd64 = sds
    r64 = O.resnet_block(sd64, prefix, x.double(), mk.double(), temb.double())
    r32 = {}
    for f1, f2 in combos:
        if f1 is None and f2 is None:
            r32[(f1, f2)] = O.resnet_block(sd32, prefix, x, mk, temb)
        else:
            r32[(f1, f2)] = WT.resnet_block_wino(sd32, prefix, x, mk, temb, f1, f2, torch.float32, 22)
    return r64, r32


def run_resnet(misses, handles, names, sds, prefix, level, cin, cout, T, B, ones):
    H, W = geom(level, T)
    x, temb = res_inputs(prefix, level, cin, T, B)
    full, mk = masks(B, T, level, ones)
    xm = x * mk
    combo = {n: (handles[n].form(level, cin, cout), handles[n].form(level, cout, cout)) for n in names}
    r64, r32 = resnet_refs(sds, prefix, level, x, mk, temb, set(combo.values()))
    xd = nhwc(xm)
    outs = {}
    for n in names:
        got = nchw(call(handles[n], _lib.US_DEBUG_RESNET, prefix, level, xd, full, temb, (B, H, W, cout)))
        judge(misses, f"resnet {prefix} {n} forms {combo[n]} T={T} B={B} {'ones' if ones else 'mask'} {H}x{W}", got, r64, r32[combo[n]], mk)
        outs[n] = got
    return outs


@pytest.mark.parametrize("T", WIDTHS)
@pytest.mark.parametrize("prefix,level,cin,cout", RES)
def test_resnet_block_and_block(handles, sds, prefix, level, cin, cout, T):
    """The ResnetBlock with the real mask and with an all-ones mask (the padded columns show), and its block1 as a `Block` on its own."""
    misses = []
    print()
    for ones in (False, True):
        run_resnet(misses, handles, MAIN, sds, prefix, level, cin, cout, T, 2, ones)
    # Block = block1 of the ResnetBlock, all-ones mask
    sd32, sd64 = sds
    H, W = geom(level, T)
    x, _ = res_inputs(prefix, level, cin, T, 2)
    full, mk = masks(2, T, level, True)
    r64 = O.block(sd64, f"{prefix}.block1", x.double(), mk.double())
    xd = nhwc(x)
    r32 = {}
    for n in MAIN:
        f = handles[n].form(level, cin, cout)
        if f not in r32:
            r32[f] = O.block(sd32, f"{prefix}.block1", x, mk) if f is None else WT.block_wino(sd32, f"{prefix}.block1", x, mk, f, torch.float32, 22)
        got = nchw(call(handles[n], _lib.US_DEBUG_BLOCK, prefix, level, xd, full, None, (2, H, W, cout)))
        judge(misses, f"block  {prefix} {n} form {f} T={T} ones {H}x{W}", got, r64, r32[f])
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("prefix,level,cin,cout", [RES[2], RES[4], RES[7]])      # level 1: F(4x4); level 2: F(2x2); level 3: F(2x4)
def test_resnet_block_with_the_groupnorm_as_its_own_pass(handles, sds, prefix, level, cin, cout):
    misses = []
    print()
    run_resnet(misses, handles, ("nofuse",), sds, prefix, level, cin, cout, 136, 2, False)
    run_resnet(misses, handles, ("nofuse",), sds, prefix, level, cin, cout, 40, 2, False)
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("prefix,level,cin,cout", [RES[0], RES[2], RES[4], RES[7], RES[9]])
def test_resnet_block_batch_of_five_and_batch_independence(handles, sds, prefix, level, cin, cout):
    """B = 5 (a GEMM's row count is no multiple of 64), and item 0's bits do not depend on what it is batched with."""
    misses = []
    print()
    T = 40
    o5 = run_resnet(misses, handles, MAIN, sds, prefix, level, cin, cout, T, 5, False)
    H, W = geom(level, T)
    x, temb = res_inputs(prefix, level, cin, T, 5)
    for B in (1, 2):
        full, mk = masks(B, T, level)
        xd = nhwc(x[:B] * mk)
        for n in MAIN:
            got = nchw(call(handles[n], _lib.US_DEBUG_RESNET, prefix, level, xd, full, temb[:B], (B, H, W, cout)))
            if not torch.equal(got[0], o5[n][0]):
                misses.append(f"{prefix} {n}: item 0 of B = {B} differs from item 0 of B = 5 by {float((got[0] - o5[n][0]).abs().max()):.3e}")
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("prefix,level,cin,cout", [RES[0], RES[4], RES[7]])
def test_resnet_block_nan_in_item_0_leaves_item_1_alone(handles, prefix, level, cin, cout):
    misses = []
    T = 40
    H, W = geom(level, T)
    x, temb = res_inputs(prefix, level, cin, T, 2)
    full, mk = masks(2, T, level)
    xm = x * mk
    bad = xm.clone()
    bad[0, 5, H // 2, W // 2] = float("nan")
    for n in MAIN:
        a = nchw(call(handles[n], _lib.US_DEBUG_RESNET, prefix, level, nhwc(xm), full, temb, (2, H, W, cout)))
        b = nchw(call(handles[n], _lib.US_DEBUG_RESNET, prefix, level, nhwc(bad), full, temb, (2, H, W, cout)))
        if not torch.isnan(b[0]).any():
            misses.append(f"{prefix} {n}: the NaN did not reach item 0's output")
        if not torch.equal(a[1], b[1]):
            misses.append(f"{prefix} {n}: a NaN in item 0 changed item 1")
    assert not misses, "\n".join(misses)


# ---- attention --------------------------------------------------------------------------------------------------------------------------
# (prefix, level, C)
ATT = [("estimator.downs.0.2", 0, 128), ("estimator.downs.1.2", 1, 256), ("estimator.downs.2.2", 2, 512), ("estimator.downs.3.2", 3, 1024),
       ("estimator.mid_attn", 3, 1024), ("estimator.ups.0.2", 3, 512), ("estimator.ups.1.2", 2, 256), ("estimator.ups.2.2", 1, 128)]
ATT_NAMES = ("default", "exact")        # the attention and the resamplers do not depend on the Winograd forms
ATT_G1 = ("g1", "g1x")                  # the same two engines with every Rezero gain 1


def k_logits(sd64, prefix, x):
    b, c, h, w = x.shape
    qkv = F.conv2d(x.double(), sd64[f"{prefix}.fn.fn.to_qkv.weight"]).reshape(b, 3, O.HEADS * O.DIM_HEAD, h * w)
    return qkv[:, 1]


def run_attention(misses, handles, sds, prefix, level, c, T, B, x=None, tag=""):
    sd32, sd64 = sds
    H, W = geom(level, T)
    if x is None:
        x = rand(5000 + 10 * level + T + B, B, c, H, W)
    full, mk = masks(B, T, level)
    r64 = O.linear_attention(sd64, prefix, x.double()) * mk.double()      # the library stores an attention's output masked
    r32 = O.linear_attention(sd32, prefix, x) * mk
    outs = {}
    for n in ATT_G1:
        got = nchw(call(handles[n], _lib.US_DEBUG_ATTENTION, prefix, level, nhwc(x), full, None, (B, H, W, c)))
        judge(misses, f"attention {prefix} {n} T={T} B={B} n={H * W}{tag}", got, r64, r32, mk)
        outs[n] = got
    return outs


@pytest.mark.parametrize("prefix,level,c", ATT)
def test_attention(handles, sds_g1, prefix, level, c):
    """Every width; at level 0 also T = 104 (n = 8320: 65 chunks of 128 rows, two merge ranges).  T = 8 at level 3 is n = 10, one partial chunk;
    T = 32 at level 1 is n = 640, five chunks exactly.  B = 5 once; item 0's bits do not depend on the batch; a NaN in item 0 stays there."""
    sds = sds_g1
    misses = []
    print()
    for T in WIDTHS + ([104] if level == 0 else []):
        run_attention(misses, handles, sds, prefix, level, c, T, 2)
    T = 40
    o5 = run_attention(misses, handles, sds, prefix, level, c, T, 5)
    H, W = geom(level, T)
    x = rand(5000 + 10 * level + T + 5, 5, c, H, W)
    for n in ATT_G1:
        for B in (1, 2):
            full, _ = masks(B, T, level)
            got = nchw(call(handles[n], _lib.US_DEBUG_ATTENTION, prefix, level, nhwc(x[:B]), full, None, (B, H, W, c)))
            if not torch.equal(got[0], o5[n][0]):
                misses.append(f"{prefix} {n}: item 0 of B = {B} differs from item 0 of B = 5")
        full, _ = masks(2, T, level)
        bad = x[:2].clone()
        bad[0, 3, H // 2, W // 2] = float("nan")
        a = nchw(call(handles[n], _lib.US_DEBUG_ATTENTION, prefix, level, nhwc(x[:2]), full, None, (2, H, W, c)))
        b = nchw(call(handles[n], _lib.US_DEBUG_ATTENTION, prefix, level, nhwc(bad), full, None, (2, H, W, c)))
        if not torch.equal(a[1], b[1]) or not torch.isnan(b[0]).any():
            misses.append(f"{prefix} {n}: a NaN in item 0 changed item 1, or did not show in item 0")
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("prefix,level,c,T", [("estimator.downs.1.2", 1, 256, 32), ("estimator.downs.0.2", 0, 128, 104)])
def test_attention_with_large_k_logits_in_one_chunk(handles, sds_g1, prefix, level, c, T):
    """The online-softmax merge: 64 positions inside one 128-row chunk are scaled until the k logits there pass 40 (e^40 = 2.4e17 times the
    weight of a logit of 0); everywhere else they stay below 40.  Checked on the fp64 reference."""
    sds = sds_g1
    sd64 = sds[1]
    H, W = geom(level, T)
    n = H * W
    x = rand(6000 + level, 2, c, H, W)
    chunk = 2
    lo = 128 * chunk
    base = k_logits(sd64, prefix, x)
    flat = x.reshape(2, c, n).clone()
    flat[0, :, lo:lo + 64] *= 45.0 / float(base[0, :, lo:lo + 64].max())
    x = flat.reshape(2, c, H, W)
    k = k_logits(sd64, prefix, x)
    inside = float(k[0, :, lo:lo + 64].max())
    k[0, :, lo:lo + 64] = -1e30
    assert inside > 40 and float(k.max()) < 40, (inside, float(k.max()))
    misses = []
    print()
    run_attention(misses, handles, sds, prefix, level, c, T, 2, x, f" (k logits up to {inside:.1f} in chunk {chunk} of item 0)")
    assert not misses, "\n".join(misses)


# ---- Downsample and Upsample ------------------------------------------------------------------------------------------------------------
DOWN = [("estimator.downs.0.3", 0, 128), ("estimator.downs.1.3", 1, 256), ("estimator.downs.2.3", 2, 512)]
UP = [("estimator.ups.0.3", 3, 512), ("estimator.ups.1.3", 2, 256), ("estimator.ups.2.3", 1, 128)]


def resample_ref(sd, kind, prefix, x, mk):
    w, b = sd[f"{prefix}.conv.weight"], sd[f"{prefix}.conv.bias"]
    if kind == _lib.US_DEBUG_DOWN:
        return F.conv2d(x * mk, w, b, stride=2, padding=1)
    return F.conv_transpose2d(x * mk, w, b, stride=2, padding=1)


@pytest.mark.parametrize("kind,prefix,level,c", [(_lib.US_DEBUG_DOWN,) + d for d in DOWN] + [(_lib.US_DEBUG_UP,) + u for u in UP])
def test_downsample_and_upsample(handles, sds, kind, prefix, level, c):
    sd32, sd64 = sds
    down = kind == _lib.US_DEBUG_DOWN
    lo = level + 1 if down else level - 1       # the output's level: the library stores the result under that level's mask
    misses = []
    print()

    def run(names, T, B, x=None):
        H, W = geom(level, T)
        Ho, Wo = geom(lo, T)
        if x is None:
            x = rand(7000 + 10 * level + T + B, B, c, H, W)
        full, mk = masks(B, T, level)
        _, mko = masks(B, T, lo)
        xm = x * mk
        r64 = resample_ref(sd64, kind, prefix, x.double(), mk.double()) * mko.double()
        r32 = resample_ref(sd32, kind, prefix, x, mk) * mko
        outs = {}
        for n in names:
            got = nchw(call(handles[n], kind, prefix, level, nhwc(xm), full, None, (B, Ho, Wo, c)))
            judge(misses, f"{'down' if down else 'up'} {prefix} {n} T={T} B={B} {H}x{W}->{Ho}x{Wo}", got, r64, r32, mko)
            outs[n] = got
        return outs, x

    for T in WIDTHS:
        run(ATT_NAMES, T, 2)
    T = 40
    o5, x = run(ATT_NAMES, T, 5)
    H, W = geom(level, T)
    Ho, Wo = geom(lo, T)
    for n in ATT_NAMES:
        for B in (1, 2):
            full, mk = masks(B, T, level)
            got = nchw(call(handles[n], kind, prefix, level, nhwc(x[:B] * mk), full, None, (B, Ho, Wo, c)))
            if not torch.equal(got[0], o5[n][0]):
                misses.append(f"{prefix} {n}: item 0 of B = {B} differs from item 0 of B = 5")
        # no GroupNorm here: one NaN pixel reaches exactly the outputs it reaches in the reference (all-ones mask)
        ones, _ = masks(2, T, level, True)
        bad = x[:2].clone()
        bad[1, 2, H // 2, W - 1] = float("nan")
        ref = resample_ref(sd32, kind, prefix, bad, torch.ones(2, 1, 1, W))
        got = nchw(call(handles[n], kind, prefix, level, nhwc(bad), ones, None, (2, Ho, Wo, c)))
        if not torch.equal(torch.isnan(got), torch.isnan(ref)):
            misses.append(f"{prefix} {n}: a NaN pixel reaches {int(torch.isnan(got).sum())} outputs, in the reference {int(torch.isnan(ref).sum())}")
    assert not misses, "\n".join(misses)


# ---- the first ResnetBlock and the final Block + projection ------------------------------------------------------------------------------
def first_ref(sd, mu, x, m, temb):
    return O.resnet_block(sd, "estimator.downs.0.0", torch.stack([mu, x], 1), m, temb)


def final_ref(sd, x, m):
    h = O.block(sd, "estimator.final_block", x, m)
    return (F.conv2d(h * m, sd["estimator.final_conv.weight"], sd["estimator.final_conv.bias"]) * m).squeeze(1)


def test_first_resnet_block(handles, sds):
    """US_DEBUG_FIRST: launch_first_conv (the 2-channel 3x3 and res_conv), block2 and the GroupNorm pass that re-evaluates res_conv."""
    sd32, sd64 = sds
    misses = []
    print()
    P = "estimator.downs.0.0"

    def run(T, B, ones=False, mux=None):
        mu, x, temb = (rand(8000 + T + B, B, NF, T), rand(8001 + T + B, B, NF, T), rand(8002 + T + B, B, TD)) if mux is None else mux
        full, mk = masks(B, T, 0, ones)
        # (the walk stores this block's result masked: its readers take `x * mask`; the module itself leaves res_conv's bias in padded columns)
        r64 = first_ref(sd64, mu.double(), x.double(), mk.double(), temb.double()) * mk.double()
        r32 = first_ref(sd32, mu, x, mk, temb) * mk
        outs = {}
        for n in ATT_NAMES:
            got = nchw(call(handles[n], _lib.US_DEBUG_FIRST, P, 0, torch.stack([mu, x]).contiguous().to(DEV), full, temb, (B, NF, T, DIM)))
            judge(misses, f"first {n} T={T} B={B} {'ones' if ones else 'mask'}", got, r64, r32, mk)
            outs[n] = got
        return outs, (mu, x, temb)

    for T in WIDTHS:
        run(T, 2)
    run(136, 2, True)
    o5, (mu, x, temb) = run(40, 5)
    for n in ATT_NAMES:
        for B in (1, 2):
            full, _ = masks(B, 40, 0)
            got = nchw(call(handles[n], _lib.US_DEBUG_FIRST, P, 0, torch.stack([mu[:B], x[:B]]).contiguous().to(DEV), full, temb[:B], (B, NF, 40, DIM)))
            if not torch.equal(got[0], o5[n][0]):
                misses.append(f"first {n}: item 0 of B = {B} differs from item 0 of B = 5")
        full, _ = masks(2, 40, 0)
        bad = x[:2].clone()
        bad[0, 40, 20] = float("nan")
        a = nchw(call(handles[n], _lib.US_DEBUG_FIRST, P, 0, torch.stack([mu[:2], x[:2]]).contiguous().to(DEV), full, temb[:2], (2, NF, 40, DIM)))
        b = nchw(call(handles[n], _lib.US_DEBUG_FIRST, P, 0, torch.stack([mu[:2], bad]).contiguous().to(DEV), full, temb[:2], (2, NF, 40, DIM)))
        if not torch.equal(a[1], b[1]) or not torch.isnan(b[0]).any():
            misses.append(f"first {n}: a NaN in item 0 changed item 1, or did not show in item 0")
    assert not misses, "\n".join(misses)


def test_final_block_and_projection(handles, sds):
    """US_DEBUG_FINAL on both handles and in both forms of launch_final_conv: GroupNorm + Mish inside the projection (level 0, what inference
    runs) and the projection over the stored activation (level 1, what a training forward runs)."""
    sd32, sd64 = sds
    misses = []
    print()

    def run(T, B, form, ones=False):
        x = rand(9000 + T + B, B, DIM, NF, T)
        full, mk = masks(B, T, 0, ones)
        r64 = final_ref(sd64, x.double(), mk.double())
        r32 = final_ref(sd32, x, mk)
        outs = {}
        for n in ATT_NAMES:
            got = call(handles[n], _lib.US_DEBUG_FINAL, "", form, nhwc(x * mk), full, None, (B, NF, T))
            judge(misses, f"final {n} form {form} T={T} B={B} {'ones' if ones else 'mask'}", got[:, None], r64[:, None], r32[:, None], mk)
            outs[n] = got
        return outs, x

    for form in (0, 1):
        for T in WIDTHS:
            run(T, 2, form)
        run(136, 2, form, True)
        o5, x = run(40, 5, form)
        for n in ATT_NAMES:
            for B in (1, 2):
                full, mk = masks(B, 40, 0)
                got = call(handles[n], _lib.US_DEBUG_FINAL, "", form, nhwc(x[:B] * mk), full, None, (B, NF, 40))
                if not torch.equal(got[0], o5[n][0]):
                    misses.append(f"final {n} form {form}: item 0 of B = {B} differs from item 0 of B = 5")
            full, mk = masks(2, 40, 0)
            bad = (x[:2] * mk).clone()
            bad[0, 3, 40, 20] = float("nan")
            a = call(handles[n], _lib.US_DEBUG_FINAL, "", form, nhwc(x[:2] * mk), full, None, (2, NF, 40))
            b = call(handles[n], _lib.US_DEBUG_FINAL, "", form, nhwc(bad), full, None, (2, NF, 40))
            if not torch.equal(a[1], b[1]) or not torch.isnan(b[0]).any():
                misses.append(f"final {n} form {form}: a NaN in item 0 changed item 1, or did not show in item 0")
    assert not misses, "\n".join(misses)


# ---- whole evaluations: the pre-split two-plane hand-offs of the walk (hid_split, up_split, fin_split, the r1-to-r2 copy) ------------------
@pytest.mark.parametrize("T", [8, 40, 136])
@pytest.mark.parametrize("mults", [(1,), (1, 2), (1, 2, 4, 8)])
def test_whole_evaluation_elementwise(handles, sd_np, mults, T):
    """`us_debug_block` always passes fp32 tensors; the walk hands some convolutions two-plane fp16 operands.  Those are judged in place: whole
    evaluations of a one-level, a two-level (every split plan of the walk engaged) and the full network, T in {8, 40, 136}, with a padded and
    a fully padded item, on the default and the exact handle, under the same bar against `estimator_forward` in fp64 and fp32."""
    from unitspeech_amd import synthetic_inputs
    if mults == FULL.dim_mults:
        cfg, np_sd, model = FULL, sd_np, handles["default"].model
    else:
        cfg = DecoderConfig(dim_mults=mults)
        np_sd = synthetic_state_dict(cfg, 0)
        model = make_model(np_sd, cfg)
    sd32, sd64 = O.to_torch(np_sd), O.to_torch(np_sd, torch.float64)
    misses = []
    print()
    q = 1 << (len(mults) - 1)
    for T in (T,):
        lens = [T, max(T - 8, 4), 0]
        inp = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_inputs(cfg, 3, T, seed=50 + T, lengths=lens).items()}
        t = torch.tensor([0.9, 0.4, 0.07])
        r64 = O.estimator_forward(sd64, inp["z"].double(), inp["mask"].double(), inp["cond"].double(), t.double(), inp["spk_emb"].double())
        r32 = O.estimator_forward(sd32, inp["z"], inp["mask"], inp["cond"], t, inp["spk_emb"])
        for exact in (False, True):
            model.exact = exact
            try:
                with torch.no_grad():
                    out = model.estimator(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), t.to(DEV), inp["spk_emb"].to(DEV)).cpu()
            finally:
                model.exact = False
            judge(misses, f"evaluation dim_mults {mults} {'exact' if exact else 'default'} T={T} (T % {q} == {T % q})", out[:, None], r64[:, None],
                  r32[:, None], inp["mask"][:, :, None, :])
    assert not misses, "\n".join(misses)
