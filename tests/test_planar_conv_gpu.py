"""The planar Conv1d core (csrc/conv1d_planar.h) one layer at a time, on the GPU: every convolution, Activation1d and conv_post of three
BigVGAN configurations and the dense convolutions of four ECAPA-TDNN configurations, each run alone through us_vocoder_debug_layer /
us_speaker_debug_conv (the launches the forwards use) and compared with torch.nn.functional in fp64 on the same inputs; the
convolution epilogue's order and aliasing bit for bit; every output written exactly once and nothing outside it; and the two whole
models at those configurations.

The configurations sit where the model-level goldens do not: up-sampling rates 1, 3, 5 and 16, kernels of 1, 3 and 4 times the rate,
resblock kernels up to 31, dilations up to 64, 1 and 4 kernels per level, channel counts that put a few live channels into a second
64-channel tile, reductions (taps * Cin) that are no multiple of the 16-row K slice, Res2 widths 5 / 9 / 17 / 33 (padded to 16 / 16 /
32 / 48).

Bar of a layer test: err <= max(10 * floor, 1e-6 * max|ref|), floor = max|fp32 torch on the CPU - fp64| for the same layer and
inputs (ten times the fp32 floor is the convention of the model-level tests; the second term guards a floor that happens to be
near zero on a tiny reduction).  A wrong tap, phase or pad is off by a weight times an input, orders of magnitude above it.
Measured values: DESIGN.md, "planar Conv1d layer tests"."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402
from vocoder_torch import activation1d, bigvgan_forward  # noqa: E402

from unitspeech_amd.speaker_encoder import ECAPA_TDNN, synthetic_ecapa_state_dict, synthetic_hidden_states  # noqa: E402
from unitspeech_amd.vocoder import BigVGAN, synthetic_bigvgan_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 17
SENTINEL = 12345.0


def _vcfg(num_mels, c0, rates, kernels, rk, rd, activation, logscale):
    return {"resblock": "1", "num_mels": num_mels, "upsample_initial_channel": c0, "upsample_rates": rates, "upsample_kernel_sizes": kernels,
            "resblock_kernel_sizes": rk, "resblock_dilation_sizes": rd, "activation": activation, "snake_logscale": logscale}


VOC = {
    # k = 3u with odd u, u = 1, k = u; channels 24 -> 12 -> 6 -> 3; Kdim 35, 72, 36, ... (none a multiple of 16)
    "V1": _vcfg(5, 24, [3, 1, 2], [9, 3, 2], [5, 31], [[1, 2, 64], [1, 7, 9]], "snake", True),
    # 16 phases; Cout = 68 (four live channels in a second 64-channel tile); Kdim = 7 * 80; one kernel per level (div = 1)
    "V2": _vcfg(80, 136, [16], [32], [3], [[1, 3, 5]], "snakebeta", True),
    # k = 3u and k = 4u; four kernels per level
    "V3": _vcfg(8, 16, [5, 2], [15, 8], [3, 5, 7, 9], [[1, 3, 5]] * 4, "snakebeta", False),
}
SPK = {
    "S1": {"feat_dim": 13, "channels": 40, "emb_dim": 7, "global_context_att": True, "n_layers": 2},
    "S2": {"feat_dim": 80, "channels": 72, "emb_dim": 192, "global_context_att": False, "n_layers": 0},
    "S3": {"feat_dim": 24, "channels": 136, "emb_dim": 16, "global_context_att": True, "n_layers": 1},
    "S4": {"feat_dim": 16, "channels": 264, "emb_dim": 8, "global_context_att": False, "n_layers": 3},
}


def _seed(*parts):
    """A stable seed from strings and integers (hash() of a str changes from run to run)."""
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 2147483629
        s = (s * 131 + 7) % 2147483629
    return s


def _rand(shape, *key):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(_seed(*key)))


def _verdict(label, got, ref64, ref32, bad):
    """Prints err, floor and bar of one case and records a miss."""
    got = got.double().cpu()
    assert got.shape == ref64.shape, label
    err = float((got - ref64).abs().max())
    floor = float((ref32.double() - ref64).abs().max())
    bar = max(10 * floor, 1e-6 * float(ref64.abs().max()))
    ok = bool(torch.isfinite(got).all()) and err <= bar
    print(f"{label}: err {err:.2e} floor {floor:.2e} bar {bar:.2e}{'' if ok else '  <-- MISS'}")
    if not ok:
        bad.append(f"{label} err {err:.2e} > bar {bar:.2e}")
    return err, floor, bar


def _worse(worst, r):
    """Of two (err, floor, bar), the one nearer its bar (a bar of 0 is an exact case: only err > 0 is near it)."""
    ratio = lambda t: t[0] / t[2] if t[2] > 0 else (float("inf") if t[0] > 0 else 0.0)
    return r if worst is None or ratio(r) > ratio(worst) else worst


def _poisoned(x):
    """x with one NaN: batch item 0, channel 0, last step."""
    y = x.clone()
    y[0, 0, -1] = float("nan")
    return y


def _poison_verdict(label, got_poisoned, got_clean, ref_poisoned, bad):
    """The K slice's rows past taps * Cin (up to the next multiple of 16) carry zero weights and must read nothing: a loader that fetched
    the input for them would multiply the NaN by zero and spread it to steps no tap of the convolution covers.  So the NaN must reach
    exactly the outputs it reaches in the reference, and the other batch item must keep its bits."""
    a, b = torch.isnan(got_poisoned).cpu(), torch.isnan(ref_poisoned)
    ok = torch.equal(a, b) and torch.equal(got_poisoned[1], got_clean[1])
    print(f"{label}: NaN input sample reaches {int(a.sum())} outputs, reference {int(b.sum())}{'' if ok else '  <-- MISS'}")
    if not ok:
        bad.append(f"{label}: a NaN input sample reaches {int(a.sum())} outputs, {int(b.sum())} in the reference")


# ---- vocoder ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _voc_items(key):
    """(config, folded fp32 state_dict on the CPU, module on the GPU): the weight norm is removed on the CPU first, so the library and
    the reference read the very same fp32 weights."""
    cfg = VOC[key] if isinstance(key, str) else _vcfg(*key)
    m = BigVGAN(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(cfg, SEED).items()})
    m.remove_weight_norm()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return cfg, sd, m.to(DEV).eval()


def _voc_convs(m):
    return [(n, mod) for n, mod in m.named_modules() if isinstance(mod, (nn.Conv1d, nn.ConvTranspose1d)) and n != "conv_post"]


def _conv_ref(mod, sd, prefix, x, dt):
    w, b = sd[prefix + ".weight"].to(dt), sd[prefix + ".bias"].to(dt)
    k, d = mod.kernel_size[0], mod.dilation[0]
    if isinstance(mod, nn.ConvTranspose1d):
        u = mod.stride[0]
        return F.conv_transpose1d(x.to(dt), w, b, stride=u, padding=(k - u) // 2)
    return F.conv1d(x.to(dt), w, b, dilation=d, padding=d * (k - 1) // 2)


@pytest.mark.parametrize("Tin", [1, 2, 127, 128, 129, 300])
@pytest.mark.parametrize("name", ["V1", "V2", "V3"])
def test_a_every_vocoder_convolution_alone_matches_fp64(name, Tin):
    """128 is the tile's step count (kVcBN); 127 and 129 leave or add one step around its edge; 1 and 2 are shorter than dil * (k - 1) / 2
    of most layers, so every tap but the centre reads the zero halo.  A layer whose taps * Cin is no multiple of 16 also runs with one
    NaN in its input (_poison_verdict)."""
    cfg, sd, m = _voc_items(name)
    bad, worst = [], None
    print()
    with torch.no_grad():
        for prefix, mod in _voc_convs(m):
            x = _rand((2, mod.in_channels, Tin), name, prefix, Tin)
            got = m.debug_layer(prefix, x.to(DEV))
            kind = f"u={mod.stride[0]} k={mod.kernel_size[0]}" if isinstance(mod, nn.ConvTranspose1d) else f"k={mod.kernel_size[0]} d={mod.dilation[0]}"
            r = _verdict(f"(a) {name} {prefix} [{mod.in_channels}->{mod.out_channels} {kind}] Tin={Tin}", got, _conv_ref(mod, sd, prefix, x, torch.float64),
                         _conv_ref(mod, sd, prefix, x, torch.float32), bad)
            worst = _worse(worst, r)
            taps = mod.kernel_size[0] // mod.stride[0]
            if (taps * mod.in_channels) % 16 != 0:
                xp = _poisoned(x)
                _poison_verdict(f"(a) {name} {prefix} Kdim={taps * mod.in_channels} Tin={Tin}", m.debug_layer(prefix, xp.to(DEV)), got,
                                _conv_ref(mod, sd, prefix, xp, torch.float64), bad)
    print(f"(a) {name} Tin={Tin} worst err/bar: err {worst[0]:.2e} floor {worst[1]:.2e} bar {worst[2]:.2e}")
    assert not bad, f"{len(bad)} layers miss; first: {bad[0]}"


@pytest.mark.parametrize("Tin", [1, 131])
def test_b_epilogue_order_and_aliasing_are_bit_exact(Tin):
    """out = ((conv + bias) + res), then sum + that, then / div (vc_conv_kernel's stated order): bit-equal to fp32 torch on the plain
    output c.  With `out` the same buffer as `res` (the forward at l = 1) or as `sum` (at j > 0) the bits are the same."""
    cfg, sd, m = _voc_items("V3")
    prefix = "resblocks.1.convs2.2"           # level 0: 8 channels, k = 5
    ch = m.get_submodule(prefix).out_channels
    x = _rand((2, ch, Tin), "b", "x", Tin).to(DEV)
    res, acc = _rand((2, ch, Tin), "b", "res", Tin).to(DEV), _rand((2, ch, Tin), "b", "sum", Tin).to(DEV)
    c = m.debug_layer(prefix, x)
    assert torch.isfinite(c).all() and float(c.abs().max()) > 0.01
    want_r = c + res
    want_rs = acc + want_r
    want_rsd = want_rs / 4.0
    assert torch.equal(m.debug_layer(prefix, x, res=res), want_r)
    assert torch.equal(m.debug_layer(prefix, x, res=res, sum=acc), want_rs)
    assert torch.equal(m.debug_layer(prefix, x, res=res, sum=acc, div=4.0), want_rsd)
    assert torch.equal(m.debug_layer(prefix, x, sum=acc), acc + c)
    buf = res.clone()
    assert torch.equal(m.debug_layer(prefix, x, res=buf, out=buf), want_r)
    buf = res.clone()
    assert torch.equal(m.debug_layer(prefix, x, res=buf, sum=acc, div=4.0, out=buf), want_rsd)
    buf = acc.clone()
    assert torch.equal(m.debug_layer(prefix, x, res=res, sum=buf, out=buf), want_rs)
    buf = acc.clone()
    assert torch.equal(m.debug_layer(prefix, x, res=res, sum=buf, div=4.0, out=buf), want_rsd)


def _guarded(shape, guard=4096):
    """A NaN-filled tensor of `shape` inside a larger buffer of SENTINEL."""
    n = int(np.prod(shape))
    buf = torch.full((guard + n + guard,), SENTINEL, device=DEV)
    out = buf[guard:guard + n].view(shape)
    out.fill_(float("nan"))
    return buf, out, guard, n


@pytest.mark.parametrize("Tin", [1, 129])
@pytest.mark.parametrize("name,prefix", [("V2", "ups.0.0"), ("V1", "ups.0.0")])
def test_c_transposed_layers_write_every_sample_once_and_nothing_else(name, prefix, Tin):
    """u = 16 and u = 3: the u phases together cover [0, Tin * u) and stop there."""
    cfg, sd, m = _voc_items(name)
    mod = m.get_submodule(prefix)
    u = mod.stride[0]
    x = _rand((2, mod.in_channels, Tin), "c", name, Tin)
    buf, out, guard, n = _guarded((2, mod.out_channels, Tin * u))
    m.debug_layer(prefix, x.to(DEV), out=out)
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), "wrote outside the output"
    assert not bool(torch.isnan(out).any()), f"{int(torch.isnan(out).sum())} of {n} outputs never written"
    assert torch.equal(out, m.debug_layer(prefix, x.to(DEV)))
    bad = []
    print()
    _verdict(f"(c) {name} {prefix} u={u} Tin={Tin}", out, _conv_ref(mod, sd, prefix, x, torch.float64), _conv_ref(mod, sd, prefix, x, torch.float32), bad)
    assert not bad, bad[0]


@functools.lru_cache(maxsize=None)
def _act_items(C_, activation, logscale):
    # one up-sampler with u = k = 1 that halves 2 C channels: the level and activation_post both have C channels
    return _voc_items((4, 2 * C_, (1,), (1,), (3,), ((1, 3, 5),), activation, logscale))


@pytest.mark.parametrize("logscale", [True, False])
@pytest.mark.parametrize("activation", ["snake", "snakebeta"])
@pytest.mark.parametrize("C_", [1, 3])
def test_d_activation1d_alone_matches_fp64(C_, activation, logscale):
    """256 outputs per workgroup (kActN) and replicate pads of 5 and 6: T < 7 clamps on both sides at once, 255 / 256 / 257 sit around
    the tile edge, 513 puts one sample into a third tile."""
    cfg, sd, m = _act_items(C_, activation, logscale)
    bad, worst = [], None
    print()
    with torch.no_grad():
        for prefix in ("resblocks.0.activations.3", "activation_post"):
            for T in (1, 2, 3, 5, 6, 7, 255, 256, 257, 513):
                x = _rand((2, C_, T), "d", C_, activation, logscale, prefix, T)
                got = m.debug_layer(prefix, x.to(DEV))
                r = _verdict(f"(d) {activation} logscale={int(logscale)} C={C_} {prefix} T={T}", got, activation1d(x.double(), sd, prefix, cfg),
                             activation1d(x, sd, prefix, cfg), bad)
                worst = _worse(worst, r)
    print(f"(d) {activation} logscale={int(logscale)} C={C_} worst err/bar: err {worst[0]:.2e} floor {worst[1]:.2e} bar {worst[2]:.2e}")
    assert not bad, f"{len(bad)} cases miss; first: {bad[0]}"


@pytest.mark.parametrize("name", ["V1", "V2"])
def test_e_conv_post_alone_matches_fp64(name):
    """C = 3 and C = 68; 256 samples per workgroup."""
    cfg, sd, m = _voc_items(name)
    C_ = m.conv_post.in_channels
    assert C_ == {"V1": 3, "V2": 68}[name]
    bad = []
    print()

    def ref(x, dt):
        return torch.tanh(F.conv1d(x.to(dt), sd["conv_post.weight"].to(dt), sd["conv_post.bias"].to(dt), padding=3))

    for T in (1, 255, 256, 257):
        x = _rand((2, C_, T), "e", name, T)
        buf, out, guard, n = _guarded((2, 1, T))
        m.debug_layer("conv_post", x.to(DEV), out=out)
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())
        _verdict(f"(e) {name} conv_post C={C_} T={T}", out, ref(x, torch.float64), ref(x, torch.float32), bad)
    assert not bad, bad[0]


@pytest.mark.parametrize("T", [1, 2, 43])
@pytest.mark.parametrize("name", ["V1", "V2", "V3"])
def test_h_whole_vocoder_matches_fp64_and_batch_items_are_bit_identical(name, T):
    cfg = VOC[name]
    sdn = {k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(cfg, SEED).items()}
    m = BigVGAN(cfg)
    m.load_state_dict(sdn)
    m = m.to(DEV).eval()
    mel = _rand((2, cfg["num_mels"], T), "h", name, T) * 2 - 5
    out = m(mel.to(DEV))
    with torch.no_grad():
        ref64 = bigvgan_forward(cfg, sdn, mel.double())
        ref32 = bigvgan_forward(cfg, sdn, mel)
    assert out.shape == ref64.shape == (2, 1, T * int(np.prod(cfg["upsample_rates"]))) and torch.isfinite(out).all()
    err, floor = float((out.double().cpu() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
    bar = max(1e-4, 10 * floor)
    print(f"\n(h) {name} T={T}: err {err:.2e} floor {floor:.2e} bar {bar:.2e} (max|ref| {float(ref64.abs().max()):.3f})")
    assert err <= bar
    for i in range(2):
        assert torch.equal(out[i:i + 1], m(mel[i:i + 1].contiguous().to(DEV))), i


# ---- speaker encoder ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _spk_items(name):
    cfg = SPK[name]
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, SEED).items()}
    n = cfg["n_layers"]
    m = ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"], global_context_att=cfg["global_context_att"],
                   feat_type="upstream" if n else "fbank", feat_num=n or None)
    m.load_state_dict(sd)
    return cfg, sd, m.to(DEV).eval()


SPK_LAYERS = {              # label -> (conv prefix, a BatchNorm the forward folds with at least Cout channels)
    "layer1.conv": ("layer1.conv", "layer1.bn"),
    "1x1": ("layer3.Conv1dReluBn2.conv", "layer3.Conv1dReluBn2.bn"),
    "conv": ("conv", "bn"),
    "pooling.linear1": ("pooling.linear1", "bn"),
    "pooling.linear2": ("pooling.linear2", "bn"),
}
ACT = {"none": lambda v: v, "relu": torch.relu, "tanh": torch.tanh}


def _spk_ref(sd, prefix, bn, act, x, bias2, dt):
    w, b = sd[prefix + ".weight"].to(dt), sd[prefix + ".bias"].to(dt)
    cin, cout, k = x.shape[1], w.shape[0], w.shape[2]
    y = F.conv1d(x.to(dt), w[:, :cin], b, padding=k // 2)
    if bias2 is not None:
        y = y + bias2.to(dt)[:, :, None]
    y = ACT[act](y)
    if bn:
        scale = sd[bn + ".weight"].to(dt) / torch.sqrt(sd[bn + ".running_var"].to(dt) + 1e-5)
        shift = sd[bn + ".bias"].to(dt) - sd[bn + ".running_mean"].to(dt) * scale
        y = y * scale[:cout].view(1, -1, 1) + shift[:cout].view(1, -1, 1)
    return y


@pytest.mark.parametrize("layer", list(SPK_LAYERS))
@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_f_speaker_convolutions_alone_match_fp64(name, layer):
    """layer1.conv has k = 5 and Kdim 65 / 400 / 120 / 80; 64 steps per workgroup (kSpBN).  pooling.linear1 of a global-context model
    reads 1536 of its weight's 4608 input channels and takes the per-(b, co) bias.  A layer whose taps * Cin is no multiple of 16 also
    runs with one NaN in its input (_poison_verdict)."""
    cfg, sd, m = _spk_items(name)
    prefix, bn = SPK_LAYERS[layer]
    mod = m.get_submodule(prefix)
    cin = 1536 if prefix == "pooling.linear1" else mod.in_channels
    if prefix == "layer1.conv":
        assert mod.kernel_size[0] == 5 and 5 * cin == {"S1": 65, "S2": 400, "S3": 120, "S4": 80}[name]
    use_b2 = prefix == "pooling.linear1" and cfg["global_context_att"]
    if prefix == "pooling.linear1":
        assert mod.in_channels == (4608 if cfg["global_context_att"] else 1536)
    bad, worst = [], None
    print()
    with torch.no_grad():
        for T in (1, 63, 64, 65, 129):
            x = _rand((2, cin, T), "f", name, layer, T)
            b2 = 0.5 * _rand((2, mod.out_channels), "f", "bias2", name, T) if use_b2 else None
            xd, b2d = x.to(DEV), None if b2 is None else b2.to(DEV)
            for act in ("none", "relu", "tanh"):
                for use_bn in (None, bn):
                    got = m.debug_conv(prefix, xd, bn_prefix=use_bn, act=act, bias2=b2d)
                    r = _verdict(f"(f) {name} {prefix} [{cin}->{mod.out_channels} k={mod.kernel_size[0]}] act={act} bn={use_bn} "
                                 f"bias2={int(use_b2)} T={T}", got, _spk_ref(sd, prefix, use_bn, act, x, b2, torch.float64),
                                 _spk_ref(sd, prefix, use_bn, act, x, b2, torch.float32), bad)
                    worst = _worse(worst, r)
            if (mod.kernel_size[0] * cin) % 16 != 0:
                xp = _poisoned(x)
                _poison_verdict(f"(f) {name} {prefix} Kdim={mod.kernel_size[0] * cin} T={T}", m.debug_conv(prefix, xp.to(DEV), bias2=b2d),
                                m.debug_conv(prefix, xd, bias2=b2d), _spk_ref(sd, prefix, None, "none", xp, b2, torch.float64), bad)
    print(f"(f) {name} {layer} worst err/bar: err {worst[0]:.2e} floor {worst[1]:.2e} bar {worst[2]:.2e}")
    assert not bad, f"{len(bad)} cases miss; first: {bad[0]}"


@pytest.mark.parametrize("T", [1, 65])
def test_c_speaker_convolution_into_a_channel_slice_keeps_the_rest(T):
    """in and out as the middle third of [B][3 C][T] tensors (how the blocks write the [out2, out3, out4] concatenation): the other
    channels and the bands around the tensor keep the sentinel, every output is written, and the bits are those of a dense run."""
    cfg, sd, m = _spk_items("S2")
    prefix, bn, ch = "layer2.Conv1dReluBn1.conv", "layer2.Conv1dReluBn1.bn", 72
    x = _rand((2, ch, T), "c", "spk", T).to(DEV)
    dense = m.debug_conv(prefix, x, bn_prefix=bn, act="relu")
    wide_in = torch.full((2, 3 * ch, T), SENTINEL, device=DEV)
    wide_in[:, ch:2 * ch] = x
    buf, wide, guard, n = _guarded((2, 3 * ch, T))
    wide.fill_(SENTINEL)
    out = wide[:, ch:2 * ch]
    out.fill_(float("nan"))
    m.debug_conv(prefix, wide_in[:, ch:2 * ch], bn_prefix=bn, act="relu", out=out)
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), "wrote outside the tensor"
    assert bool((wide[:, :ch] == SENTINEL).all()) and bool((wide[:, 2 * ch:] == SENTINEL).all()), "wrote outside the channel slice"
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, dense)
    bad = []
    print()
    _verdict(f"(c) S2 {prefix} slice T={T}", out, _spk_ref(sd, prefix, bn, "relu", x.cpu(), None, torch.float64),
             _spk_ref(sd, prefix, bn, "relu", x.cpu(), None, torch.float32), bad)
    assert not bad, bad[0]


@pytest.mark.parametrize("T", [1, 73, 87, 101, 130])
@pytest.mark.parametrize("name", ["S1", "S2", "S3", "S4"])
def test_g_whole_speaker_encoder_stage_by_stage(name, T):
    """Res2 widths 5 / 9 / 17 / 33 against padded widths 16 / 16 / 32 / 48.  The Res2 kernel's window leaves TT = 128 - 14 dil = 100, 86,
    72 output steps for the three blocks: T = 101, 87, 73 each put exactly one step into a second window of one block.  Bar per stage:
    2e-5 + 1e-5 max|ref| (test_speaker_encoder_gpu.py).  With the global context and T = 1 the reference's unbiased variance of one
    sample is NaN and so is everything after it: the library must be NaN in the same places."""
    cfg, sd, m = _spk_items(name)
    assert (m._config_struct().channels // 8, -(-cfg["channels"] // 8 // 16) * 16) == {"S1": (5, 16), "S2": (9, 16), "S3": (17, 32), "S4": (33, 48)}[name]
    L, Fd = cfg["n_layers"], cfg["feat_dim"]
    hid = torch.from_numpy(synthetic_hidden_states(L, 2, T, Fd, 300 + T)) if L else _rand((2, Fd, T), "g", name, T)
    emb = m.forward_features(hid.to(DEV)).cpu()
    stages = {}
    with torch.no_grad():
        ref = ecapa_forward(cfg, sd, hid, dtype=torch.float64, stages=stages)
    blocks = m.stage("blocks").cpu()
    ch = cfg["channels"]
    got = {"feat": m.stage("feat").cpu(), "layer1": m.stage("layer1").cpu(), "layer2": blocks[:, :ch], "layer3": blocks[:, ch:2 * ch],
           "layer4": blocks[:, 2 * ch:], "pooling": m.stage("pooling").cpu(), "embedding": emb}
    stages["embedding"] = ref
    bad = []
    print()
    for s, v in got.items():
        r = stages[s]
        assert v.shape == r.shape, s
        nan = torch.isnan(r)
        assert (T == 1 and cfg["global_context_att"] and s in ("pooling", "embedding")) or not bool(nan.any()), s
        same_nan = torch.equal(torch.isnan(v), nan)
        fin = ~nan
        mx = float(r[fin].abs().max()) if bool(fin.any()) else 0.0
        err = float((v.double()[fin] - r[fin]).abs().max()) if bool(fin.any()) else 0.0
        tol = max(2e-5, 1e-5 * mx) if s == "embedding" else 2e-5 + 1e-5 * mx
        ok = same_nan and bool(torch.isfinite(v[fin]).all()) and err <= tol
        print(f"(g) {name} T={T} {s}: err {err:.2e} (max|ref| {mx:.2f}, NaN {int(nan.sum())}) bar {tol:.1e}{'' if ok else '  <-- MISS'}")
        if not ok:
            bad.append(s)
    assert not bad, f"first wrong stage: {bad[0]}"
