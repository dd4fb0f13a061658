"""Element-wise judgement of the decoder's training gradients.  TEST INFRASTRUCTURE ONLY (tests/test_decoder_grads.py,
tests/test_decoder_grads_gpu.py, tests/test_hip_parity_r3.py; nothing in unitspeech_amd/ imports it).

* the case table (T, per-item lengths, weight set) and the seeded inputs of a case (`crops`, `ReplayRandn`);
* the oracle's `loss_t` under torch autograd on the CPU in a given dtype: all 228 estimator gradients plus grad_x0 / grad_cond / grad_spk_emb;
* the bar, per tensor: max |got - fp64| <= max(10 x max |fp32 oracle - fp64|, 1e-5 x max |fp64|)  (the rule of tests/test_decoder_blocks_gpu.py);
  for the eight one-element Rezero gains the larger of that and 1e-4 of the gain's own magnitude;
* the order in which train_backward_body (csrc/train_host.inc) produces the tensors, so that the first one off its bar names the culprit;
* the old measures (per-tensor relative L2, the odd-strided sample of the 8 x 176 golden) for tests that show what they miss;
* a host-side restatement of wgrad_chunk / launch_wgrad_single_writer / launch_wgrad: which weight-gradient variant a convolution runs at a
  (T, B), and whether it overwrites or accumulates.  `python tools/grad_parity.py` prints the table of DESIGN.md section 26.
"""
from __future__ import annotations

import functools
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import decoder_oracle as O                          # noqa: E402
from unitspeech_amd.params import DecoderConfig, param_shapes   # noqa: E402

FULL = DecoderConfig()
INPUT_GRADS = ("grad_x0", "grad_cond", "grad_spk_emb")

# (id, T, lengths, gain-one weights?)  -- what each reaches: DESIGN.md section 26
CASES = OrderedDict((c[0], c) for c in [
    ("T8_8", 8, [8], False),
    ("T8_8_5", 8, [8, 5], False),
    ("T8_8_0", 8, [8, 0], False),
    ("T16_16_9", 16, [16, 9], False),
    ("T24_24_17_1", 24, [24, 17, 1], False),
    ("T40_33", 40, [33], False),
    ("T128_128_121", 128, [128, 121], False),
    ("T136_129", 136, [129], False),
    ("T8_8_5_g1", 8, [8, 5], True),
    ("T24_24_17_1_g1", 24, [24, 17, 1], True),
])
SMALL = ("T8_8", "T8_8_5", "T8_8_0", "T16_16_9", "T24_24_17_1", "T40_33", "T8_8_5_g1", "T24_24_17_1_g1")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def crops(B, T, key, lengths=None):
    """Seeded training inputs (x0, mask, cond, spk, t, z); lengths default to T - 8 (b mod 3)."""
    g = np.random.Generator(np.random.Philox(key=key))
    x0 = torch.from_numpy(g.standard_normal((B, FULL.n_feats, T), dtype=np.float32)).clamp(-1, 1)
    cond = torch.from_numpy(g.standard_normal((B, FULL.n_feats, T), dtype=np.float32) * 0.5)
    if lengths is None:
        lengths = [T - 8 * (b % 3) for b in range(B)]
    mask = torch.zeros(B, 1, T)
    for b, n in enumerate(lengths):
        mask[b, 0, :n] = 1.0
    spk = torch.from_numpy(g.standard_normal((B, 1, FULL.spk_emb_dim), dtype=np.float32))
    spk = spk / spk.norm(dim=-1, keepdim=True)
    t = torch.from_numpy(g.uniform(0.05, 0.95, size=(B,)).astype(np.float32))
    z = torch.from_numpy(g.standard_normal((B, FULL.n_feats, T), dtype=np.float32))
    return x0, mask, cond, spk, t, z


class ReplayRandn:
    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def __enter__(self):
        self.orig = torch.randn
        torch.randn = self
        return self

    def __exit__(self, *a):
        torch.randn = self.orig

    def __call__(self, *shape, **kw):
        d = self.draws[self.i]
        self.i += 1
        return d.to(device=kw.get("device", d.device), dtype=kw.get("dtype", d.dtype))


def case_inputs(case):
    _, T, lengths, _ = CASES[case]
    return crops(len(lengths), T, key=2600 + list(CASES).index(case), lengths=lengths)


@functools.lru_cache(maxsize=2)
def weights(gain_one=False):
    """Full-size synthetic weights; gain_one: every Rezero gain 1 and to_qkv unscaled, so that the attention branch's data gradient stands
    above the rounding of the skip path (at the shipped 0.01 an error in it never reaches an upstream tensor)."""
    from unitspeech_amd.params import synthetic_state_dict
    return synthetic_state_dict(FULL, 0, rezero_g=1.0, qkv_scale=1.0) if gain_one else synthetic_state_dict(FULL, 0)


def case_weights(case):
    return weights(CASES[case][3])


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
class _Capture:
    """While active, records (input, gradient w.r.t. the output) of the F.conv2d / F.group_norm calls whose weight is one of `targets`
    ({name: tensor}) into self.got[name] = [input, grad_output]."""

    def __init__(self, targets):
        self.targets, self.got = targets, {}

    def _wrap(self, fn, weight_pos):
        def call(*a, **kw):
            y = fn(*a, **kw)
            for name, w in self.targets.items():
                if len(a) > weight_pos and a[weight_pos] is w:
                    rec = self.got[name] = [a[0].detach(), None]
                    y.register_hook(lambda g, rec=rec: rec.__setitem__(1, g.detach()))
            return y
        return call

    def __enter__(self):
        self.orig = (O.F.conv2d, O.F.group_norm)
        O.F.conv2d, O.F.group_norm = self._wrap(self.orig[0], 1), self._wrap(self.orig[1], 2)
        return self

    def __exit__(self, *a):
        O.F.conv2d, O.F.group_norm = self.orig


def oracle_grads(sd_np, inputs, dtype, capture=()):
    """(loss, {name: gradient}) of the oracle's loss_t under autograd on the CPU in `dtype`: the 228 estimator tensors and the three input
    gradients, as float64.  capture: names of convolution / GroupNorm weights; then a third result {name: [the layer's input, the gradient
    w.r.t. its output]} (for tests that recompute one parameter gradient by hand)."""
    x0, mask, cond, spk, t, z = (v.to(dtype) for v in inputs)
    x0, cond, spk = (v.clone().requires_grad_(True) for v in (x0, cond, spk))
    sd = {k: v.clone().requires_grad_(True) for k, v in O.to_torch(sd_np, dtype).items()}
    with _Capture({n: sd[n] for n in capture}) as cap:
        loss, _ = O.loss_t(sd, x0, mask, cond, t, spk, z, FULL.n_feats, FULL.beta_min, FULL.beta_max, FULL.pe_scale)
        loss.backward()
    out = {k: v.grad.detach().double() for k, v in sd.items() if v.grad is not None and k.startswith("estimator.")}
    out.update(grad_x0=x0.grad.double(), grad_cond=cond.grad.double(), grad_spk_emb=spk.grad.double())
    return (float(loss.detach()), out, cap.got) if capture else (float(loss.detach()), out)


# ---- backward execution order -----------------------------------------------------------------------------------------------------------
def backward_order(names=None):
    """The 231 tensor names in the order train_backward_body finishes them: final projection, final Block, ups.2 .. ups.0 (Upsample,
    attention, second and first ResnetBlock), mid_block2, mid_attn, mid_block1, downs.3 .. downs.0, the first convolution's data gradients,
    then -- at the very end of the pass -- the time projections of every ResnetBlock (same block order), grad_spk_emb and the time MLP."""
    L = len(FULL.dim_mults)
    conv = lambda p: [p + ".weight", p + ".bias"]
    blk = lambda p: [p + ".block.1.weight", p + ".block.1.bias"] + conv(p + ".block.0")
    att = lambda p: [p + ".fn.fn.to_out.bias", p + ".fn.g", p + ".fn.fn.to_out.weight", p + ".fn.fn.to_qkv.weight"]
    shapes = param_shapes(FULL)
    res_prefixes = []

    def res(p):
        res_prefixes.append(p)
        return blk(p + ".block2") + blk(p + ".block1") + (conv(p + ".res_conv") if p + ".res_conv.weight" in shapes else [])

    out = conv("estimator.final_conv") + blk("estimator.final_block")
    for u in range(L - 2, -1, -1):
        p = f"estimator.ups.{u}"
        out += conv(p + ".3.conv") + att(p + ".2") + res(p + ".1") + res(p + ".0")
    out += res("estimator.mid_block2") + att("estimator.mid_attn") + res("estimator.mid_block1")
    for lv in range(L - 1, -1, -1):
        p = f"estimator.downs.{lv}"
        out += (conv(p + ".3.conv") if p + ".3.conv.weight" in shapes else []) + att(p + ".2") + res(p + ".1") + res(p + ".0")
    out += ["grad_x0", "grad_cond"]
    for p in res_prefixes:
        out += conv(p + ".mlp.1")
    out += ["grad_spk_emb"] + conv("estimator.mlp.2") + conv("estimator.mlp.0")
    want = {k for k in shapes if k.startswith("estimator.")} | set(INPUT_GRADS)
    assert len(out) == len(set(out)) and set(out) == want, sorted(want ^ set(out))[:8]
    if names is not None:
        assert set(names) == want, sorted(want ^ set(names))[:8]
    return out


# ---- the bar ----------------------------------------------------------------------------------------------------------------------------
def is_gain(name):
    return name.endswith(".fn.g")


def floors_of(ref32, ref64):
    """{name: max |fp32 oracle - fp64|}: all of the fp32 oracle that the bar needs."""
    return {n: float((ref32[n] - ref64[n]).abs().max()) for n in ref64}


def bar_of(name, r64, floor):
    """max(10 x max |fp32 oracle - fp64|, 1e-5 x max |fp64|); a Rezero gain: the larger of that and 1e-4 of its magnitude."""
    top = float(r64.abs().max())
    bar = max(10 * floor, 1e-5 * top)
    if is_gain(name):
        bar = max(bar, 1e-4 * top)
    return bar


def judge(got, ref64, floors, tag=""):
    """Every tensor of ref64, whole, element by element.  Returns (rows, misses): rows = (name, err, floor, bar) in backward order, misses =
    the lines of the tensors off their bar (or not finite), in backward order.  Prints the worst tensor and the gains."""
    order = backward_order(ref64.keys())
    assert set(got) >= set(order), sorted(set(order) - set(got))[:8]
    rows, misses = [], []
    for n in order:
        g, r64 = got[n].double().cpu(), ref64[n]
        assert g.shape == r64.shape, (n, tuple(g.shape), tuple(r64.shape))
        d = (g - r64).abs()
        err = float(d.max()) if bool(torch.isfinite(g).all()) else float("inf")
        floor = floors[n]
        bar = bar_of(n, r64, floor)
        rows.append((n, err, floor, bar))
        if not err <= bar:
            at = tuple(int(v) for v in torch.unravel_index(torch.nan_to_num(d, nan=float("inf")).argmax(), d.shape))
            misses.append(f"{n}: err {err:.3e} > bar {bar:.3e} (floor {floor:.3e}, max |fp64| {float(r64.abs().max()):.3e}) at {at}")
    w = max(rows, key=lambda r: r[1] / r[3])
    print(f"{tag}: worst tensor {w[0]}: err {w[1]:.3e}, fp32 oracle's {w[2]:.3e} (ratio {w[1] / max(w[2], 1e-300):.2f}), bar {w[3]:.3e}: {w[1] / w[3]:.3f} of it")
    gains = [r for r in rows if is_gain(r[0])]
    wg = max(gains, key=lambda r: r[1] / r[3])
    print(f"{tag}: worst Rezero gain {wg[0]}: err {wg[1]:.3e} = {wg[1] / float(ref64[wg[0]].abs().max()):.2e} of itself, fp32 oracle's {wg[2]:.3e}, "
          f"bar {wg[3]:.3e}: {wg[1] / wg[3]:.3f} of it")
    return rows, misses


# ---- the old measures -------------------------------------------------------------------------------------------------------------------
def rel_l2(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-300))


def sample_rel_l2(got, ref):
    """The measure of the 8 x 176 fp64 golden (test_pretraining_batch_loss_and_every_gradient_vs_oracle_autograd): tensors of <= 1,024
    elements whole, larger ones at the odd stride (numel // 4096 + 1) | 1."""
    g, r = got.double().reshape(-1), ref.reshape(-1)
    if r.numel() > 1024:
        s = (r.numel() // 4096 + 1) | 1
        g, r = g[::s], r[::s]
    return float((g - r).norm() / (r.norm() + 1e-300))


# ---- which weight-gradient variant runs (csrc/train_host.inc wgrad_chunk, csrc/train.hip launch_wgrad*) -----------------------------------
def wgrad_chunk(Ms, cout, cin, ntaps, B):
    target = 768 if B == 1 else 1536
    tt = ((cout + 63) // 64) * ((cin + 63) // 64) * ntaps * B
    nch = max(1, (target + tt - 1) // tt)
    chunk = max(64, (Ms + nch - 1) // nch)
    return (chunk + 7) // 8 * 8


def wgrad_variant(Hs, Ws, cout, cin, ntaps, taps_total, B, per_item=False):
    """(kernel, writer) of one launch_wgrad call on the default handle.  kernel: 'T' = wgrad_f16_kernel<true> (carried coordinates, Ws >= 16),
    'F' = <false>.  writer: 'ow' = one writer, overwrites garbage; 'rmw' = one writer, adds to the zero-filled scratch without atomics;
    'at' = zero fill + atomics.  A 'v' in front: one pixel range cut across all items (vchunk).  per_item: the attention's M1 = G^T q
    (gw_bstride != 0: one result per item, never vchunk)."""
    Ms = Hs * Ws
    chunk = wgrad_chunk(Ms, cout, cin, ntaps, B)
    kernel = "T" if Ws >= 16 else "F"
    single_writer = chunk >= Ms and (B == 1 or per_item)
    if not per_item and ntaps == taps_total and single_writer:
        return kernel, "ow"
    if B > 1 and not per_item:
        others = (cout // 128) * (cin // 128) * ntaps
        nch = max(1, (1536 + others - 1) // others)
        vc = max(chunk, (B * Ms + nch - 1) // nch)
        vc = (vc + 15) // 16 * 16
        return kernel, "v-rmw" if (B * Ms + vc - 1) // vc == 1 else "v-at"
    return kernel, "rmw" if chunk >= Ms else "at"


def wgrad_layers():
    """(name, level of the pixel grid the launch walks, Cout, Cin, taps per launch, taps in all, per-item) of every launch_wgrad call of
    the full-size backward; the 2-channel first block and the final projection have kernels of their own."""
    shapes, L = param_shapes(FULL), len(FULL.dim_mults)
    out = []
    for k, s in shapes.items():
        if not k.startswith("estimator.") or len(s) != 4 or s[0] % 128 or s[1] % 128:
            continue
        p = k.split(".")
        if p[1] == "downs":
            lv = int(p[2])
        elif p[1] == "ups":
            lv = L - 1 - int(p[2])
        elif p[1].startswith("mid"):
            lv = L - 1
        else:
            lv = 0
        if k.endswith(".3.conv.weight") and s[2] == 3:
            out.append((k, lv + 1, s[0], s[1], 9, 9, False))            # Downsample: walks its output grid
        elif k.endswith(".3.conv.weight"):
            out.append((k, lv, s[1], s[0], 4, 16, False))               # Upsample: four phase launches of four taps over its input grid
        elif k.endswith("to_out.weight"):
            out.append((k + " (M1)", lv, s[0], s[1], 1, 1, True))
        else:
            out.append((k, lv, s[0], s[1], s[2] * s[3], s[2] * s[3], False))
    return out


def wgrad_table(T, B):
    """{(level, kernel, writer): [layer names]} at one (T, B)."""
    out = {}
    for name, lv, co, ci, nt, tot, per_item in wgrad_layers():
        k, w = wgrad_variant(FULL.n_feats >> lv, T >> lv, co, ci, nt, tot, B, per_item)
        out.setdefault((lv, k, w), []).append(name)
    return out


if __name__ == "__main__":
    seen = {}
    for cid, T, lengths, g1 in CASES.values():
        if g1:
            continue
        tab = wgrad_table(T, len(lengths))
        print(f"T = {T}, B = {len(lengths)}  (widths {' / '.join(str(T >> l) for l in range(4))})")
        for lv in range(4):
            cells = [f"{k} {w} x{len(v)}" for (l, k, w), v in sorted(tab.items()) if l == lv]
            print(f"   level {lv}: " + ", ".join(cells))
        for (lv, k, w) in tab:
            seen.setdefault((k, w), []).append(cid)
    print("variants reached:", {k: sorted(set(v))[:3] for k, v in sorted(seen.items())})
