"""`us_reverse_diffusion` where the rest of the suite never takes it: guidance scales that are neither 0 nor 1 and differ from each
other (at (1, 1) the mode-3 combine of `sampler_update_kernel` is symmetric in the two unconditional branches and in the two scales,
and a multiplication by 1.0 is exact, so an exchanged, a dropped or a doubled scale gives the right bits there), loops longer than one
block of precomputed time projections (`kTimeBlock` = 64 steps: the refill, the short tail block and the offset arithmetic past
step 63), the largest block the default micro-batch forms (64 steps x 8 utterances x 3 branches = 1,536 rows), full-size weights from
seeds 1 and 2, and the two Python wrappers that hand the scales on.

Goldens: tests/golden/sampler_*.npz, the reference's own `UnitSpeech.forward` in fp32 and fp64 (tools/make_goldens_sampler.py).  The
reference's fp32-vs-fp64 mean-L1 is <= 2e-4 in every stored case but N = 130 (2.75e-4 at any seed: its fp32 and fp64 runs read
schedule tables that differ by a 130-term fp32 cumprod; the library reads the fp32 ones and measures 1.0e-4 / 2.7e-4
against the two columns).  tests/test_sampler.py pins the CPU oracle to the goldens and shows that a wrong scale lands more than
100 loop bars away.

Bar 1 (loops): mel-L1 <= 1e-3 against the reference in fp32 and in fp64 (the project's loop bar), library-vs-fp64 mean-L1 <= 10 x the
reference's own fp32-vs-fp64 mean-L1 (the rule of tests/test_hubert_gpu.py), masked frames exactly 0.
Bar 2 (one and two steps, elementwise): max|library - fp64| <= max(10 x max|oracle fp32 - fp64|, 1e-5 max|fp64|)."""
import numpy as np
import pytest
import torch

from oracle import decoder_oracle as O
from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_inputs, synthetic_state_dict
from unitspeech_amd.encoder import (ContentVecEncoder, DurationPredictor, DurationPredictorConfig, Encoder, EncoderConfig,
                                    synthetic_duration_predictor_state_dict, synthetic_encoder_state_dict)

pytestmark = pytest.mark.gpu

TINY = DecoderConfig(dim=16)
FULL = DecoderConfig()
DEV = "cuda:0"
LOOP_BAR = 1e-3
SCALE_PAIRS = [(1.7, 0.4), (0.4, 1.7), (2.5, 0.0), (0.0, 0.3)]
BLOCK_SEED = 41          # input seed of the largest-block test: oracle fp32-vs-fp64 mean-L1 of item 0 <= 2e-4 (asserted there)


def make_model(cfg, seed=0):
    m = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, seed).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny():
    sd = synthetic_state_dict(TINY, 0)
    return make_model(TINY), O.to_torch(sd), O.to_torch(sd, torch.float64)


def G(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def l1(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().mean().item()


def maxabs(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def inputs(cfg, g, n, B, T):
    """The generator's inputs, rebuilt from the stored seed and checked against the stored checksums."""
    inp = G(synthetic_inputs(cfg, B, T, seed=int(g["seed"]), n_steps=n, lengths=[int(v) for v in g["lengths"]]))
    for name, key in (("z", "z_abs_sum"), ("noise", f"noise_abs_sum_N{n}" if f"noise_abs_sum_N{n}" in g else "noise_abs_sum")):
        ref = float(g[key])
        assert abs(inp[name].double().abs().sum().item() - ref) <= 1e-9 * ref, name
    return inp


def hip(model, inp, n, wt, ws, **kw):
    if "rng" not in kw:
        kw["noise"] = inp["noise"].to(DEV)
    return model(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), n, wt, ws, **kw)


def oracle(sd, inp, n, wt, ws):
    dt = next(iter(sd.values())).dtype
    return O.reverse_diffusion(sd, inp["z"].to(dt), inp["mask"].to(dt), inp["cond"].to(dt), inp["spk_emb"].to(dt), n, wt, ws,
                               noise=inp["noise"].to(dt))


def bar1(tag, out, ref32, ref64, mask):
    e32, e64, gap = l1(out, ref32), l1(out, ref64), l1(ref32, ref64)
    print(f"\n{tag}: library vs reference fp32 {e32:.3e}, vs fp64 {e64:.3e}; reference fp32 vs fp64 {gap:.3e}; "
          f"mean|out| {ref64.abs().mean().item():.1f}")
    assert torch.isfinite(out).all()
    assert (out.cpu() * (1 - mask)).abs().max().item() == 0.0, "masked frames must be exactly zero"
    assert e32 <= LOOP_BAR and e64 <= LOOP_BAR
    assert e64 <= 10 * gap


def bar2(tag, out, o32, o64):
    e, gap, top = maxabs(out, o64), maxabs(o32, o64), o64.abs().max().item()
    print(f"\n{tag}: max|library - fp64| {e:.3e}; oracle max|fp32 - fp64| {gap:.3e}; max|fp64| {top:.2f}")
    assert e <= max(10 * gap, 1e-5 * top), tag


# ---- 1. unequal scales, ten steps, against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_unequal_scales_vs_reference_golden(golden, tiny, k):
    model = tiny[0]
    g = G(golden("sampler_tiny_scales"))
    wt, ws = float(g["w_text"][k]), float(g["w_spk"][k])
    assert (wt, ws) == SCALE_PAIRS[k]
    n = int(g["n_steps"])
    inp = inputs(TINY, g, n, 2, 16)
    bar1(f"tiny N={n} w=({wt}, {ws})", hip(model, inp, n, wt, ws), g["out"][k], g["out_fp64"][k], inp["mask"])


# ---- 2. the combine formula itself: one step (no noise term) and two (noise term), element by element ---------------------------
@pytest.fixture(scope="module")
def short_inputs():
    return {n: G(synthetic_inputs(TINY, 2, 8, seed=31, n_steps=n, lengths=[8, 5])) for n in (1, 2)}


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("wt,ws", SCALE_PAIRS + [(1e-3, 1e-3)])
def test_scales_in_one_and_two_steps_elementwise_vs_oracle(tiny, short_inputs, n, wt, ws):
    model, sd32, sd64 = tiny
    inp = short_inputs[n]
    out = hip(model, inp, n, wt, ws)
    assert (out.cpu() * (1 - inp["mask"])).abs().max().item() == 0.0
    bar2(f"N={n} w=({wt}, {ws})", out, oracle(sd32, inp, n, wt, ws), oracle(sd64, inp, n, wt, ws))


# ---- 3. a scale at or below zero is a branch not taken (unitspeech.py:300-330) --------------------------------------------------
@pytest.mark.parametrize("neg,zero", [((-0.5, 0.3), (0.0, 0.3)), ((1.7, -2.0), (1.7, 0.0))])
def test_nonpositive_scale_switches_its_branch_off(tiny, short_inputs, neg, zero):
    model, sd32, sd64 = tiny
    inp = short_inputs[2]
    a, b = hip(model, inp, 2, *neg), hip(model, inp, 2, *zero)
    assert torch.equal(a, b)
    bar2(f"N=2 w={neg}", a, oracle(sd32, inp, 2, *neg), oracle(sd64, inp, 2, *neg))
    bar2(f"N=2 w={zero}", b, oracle(sd32, inp, 2, *zero), oracle(sd64, inp, 2, *zero))


# ---- 4. past one block of time projections -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 130])
def test_loops_past_one_time_block_vs_reference_golden(golden, tiny, n):
    """N = 64: exactly one block; 65: a block and a tail of one step; 130: two refills and a tail of two.  At N = 65 the micro-batch
    is varied too: 2 makes the last micro-batch (one item) smaller than the planned one while a refill happens, and every item keeps
    its bits (the promise test_config2_batch64_... asserts at N = 2)."""
    model = tiny[0]
    g = G(golden("sampler_tiny_steps"))
    wt, ws = float(g["w_text"]), float(g["w_spk"])
    inp = inputs(TINY, g, n, 3, 16)
    assert model.micro_batch == 0
    out = hip(model, inp, n, wt, ws)
    bar1(f"tiny N={n} w=({wt}, {ws})", out, g[f"out_N{n}"], g[f"out_fp64_N{n}"], inp["mask"])
    if n == 65:
        try:
            for mb in (1, 2):
                model.micro_batch = mb
                other = hip(model, inp, n, wt, ws)
                for b in range(3):
                    assert torch.equal(other[b], out[b]), (mb, b)
        finally:
            model.micro_batch = 0


# ---- 5. the largest block of the default micro-batch: 64 steps x 8 utterances x 3 branches --------------------------------------
def test_largest_time_block_of_the_default_micro_batch(tiny):
    model, sd32, sd64 = tiny
    B, T, N, wt, ws = 8, 8, 64, 1.3, 0.7
    inp = G(synthetic_inputs(TINY, B, T, seed=BLOCK_SEED, n_steps=N, lengths=[T - b % 3 for b in range(B)]))
    assert model.micro_batch == 0                                       # library default: 8 utterances, 24 rows per step
    out = hip(model, inp, N, wt, ws, rng="philox", seed=23)
    assert torch.isfinite(out).all()
    for b in (0, 7):
        one = {k: v[b:b + 1] for k, v in inp.items() if k != "noise"}
        assert torch.equal(hip(model, one, N, wt, ws, rng="philox", seed=23, utt_offset=b), out[b:b + 1]), b
    # the same block with the noise given, so that the oracle can follow item 0
    given = hip(model, inp, N, wt, ws)
    item0 = {k: (v[:, :1] if k == "noise" else v[:1]) for k, v in inp.items()}
    assert torch.equal(hip(model, item0, N, wt, ws), given[:1])
    o32, o64 = oracle(sd32, item0, N, wt, ws), oracle(sd64, item0, N, wt, ws)
    assert l1(o32, o64) <= 2e-4, "pick another BLOCK_SEED: the oracle's own fp32-vs-fp64 distance leaves the bar no room"   # 9.3e-5
    bar1(f"tiny B=8 N={N} item 0", given[:1], o32, o64, item0["mask"])


# ---- 6. other weight draws at full size ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_full_size_loop_with_other_weight_draws_vs_reference_golden(golden, seed):
    g = G(golden("sampler_full_seeds"))
    assert seed in g["weight_seeds"].tolist()
    n, wt, ws = int(g["n_steps"]), float(g["w_text"]), float(g["w_spk"])
    inp = inputs(FULL, g, n, 1, 64)
    out = hip(make_model(FULL, seed), inp, n, wt, ws)
    bar1(f"full N={n} w=({wt}, {ws}) weight seed {seed}", out, g[f"out_s{seed}"], g[f"out_fp64_s{seed}"], inp["mask"])


# ---- 7. the wrappers hand the scales on in order -------------------------------------------------------------------------------
class fixed_randn_like:
    """torch.randn_like replaced by a given draw: the wrappers' z (the reference's randn_like)."""

    def __init__(self, z):
        self.z = z

    def __enter__(self):
        self.orig = torch.randn_like
        torch.randn_like = lambda t, *a, **k: self.z.clone()

    def __exit__(self, *a):
        torch.randn_like = self.orig


def philox_draws(key, n_steps, F, tp):
    gz = np.random.Generator(np.random.Philox(key=key))
    z = torch.from_numpy(gz.standard_normal((1, F, tp), dtype=np.float32)).to(DEV)
    noise = torch.from_numpy(np.stack([gz.standard_normal((1, F, tp), dtype=np.float32) for _ in range(n_steps)])).to(DEV)
    return z, noise


def direct_call_on(model, cond_y, tp, z, spk, n_steps, wt, ws, noise):
    """`model(z, y_mask, cond_y, spk, N, wt, ws)` on the conditioning a wrapper returned (cropped to the item's frames; the wrappers
    leave zeros from there to the U-Net length `tp`, and y_mask is the item's sequence mask)."""
    frames = cond_y.shape[-1]
    cond = torch.zeros(1, cond_y.shape[1], tp, device=DEV)
    cond[:, :, :frames] = cond_y
    y_mask = (torch.arange(tp, device=DEV) < frames).float().view(1, 1, tp)
    return model(z, y_mask, cond, spk, n_steps, wt, ws, noise=noise)[:, :, :frames]


def test_execute_text_to_speech_passes_the_scales_in_order(golden, tiny):
    model = tiny[0]
    g = golden("tts_modules_tiny")
    ecfg = EncoderConfig(n_vocab=20, n_feats=TINY.n_feats, n_channels=16, filter_channels=32, n_heads=2, n_layers=2, kernel_size=3,
                         window_size=4)
    dcfg = DurationPredictorConfig(in_channels=16, filter_channels=24, kernel_size=3, spk_emb_dim=TINY.spk_emb_dim)
    enc = Encoder(ecfg.n_vocab, ecfg.n_feats, ecfg.n_channels, ecfg.filter_channels, ecfg.n_heads, ecfg.n_layers, ecfg.kernel_size, 0.1,
                  window_size=ecfg.window_size)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(ecfg, 1).items()}, strict=True)
    dp = DurationPredictor(dcfg.in_channels, dcfg.filter_channels, dcfg.kernel_size, 0.1, spk_emb_dim=dcfg.spk_emb_dim)
    dp.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_duration_predictor_state_dict(dcfg, 1).items()}, strict=True)
    enc, dp = enc.to(DEV).eval(), dp.to(DEV).eval()
    ids, lens, spk = (torch.from_numpy(g[k]).to(DEV) for k in ("ids", "lengths", "spk_emb"))
    n_steps, tp = int(g["n_steps"]), int(g["tp"])
    z, noise = philox_draws(int(g["noise_key"]), n_steps, TINY.n_feats, tp)
    with fixed_randn_like(z):
        cond_y, dec, _ = model.execute_text_to_speech(ids, lens, spk, enc, dp, len(TINY.dim_mults) - 1, diffusion_steps=n_steps,
                                                      length_scale=1.0, text_gradient_scale=1.7, spk_gradient_scale=0.4, noise=noise)
    assert cond_y.shape[-1] == int(g["frames"])
    assert torch.equal(dec, direct_call_on(model, cond_y, tp, z, spk, n_steps, 1.7, 0.4, noise))
    assert not torch.equal(dec, direct_call_on(model, cond_y, tp, z, spk, n_steps, 0.4, 1.7, noise))


def test_execute_voice_conversion_passes_the_scales_in_order(golden, tiny):
    model = tiny[0]
    g = golden("vc_tiny")
    cfg = EncoderConfig(n_vocab=20, n_feats=TINY.n_feats, n_channels=16, filter_channels=32, n_heads=2, n_layers=2, kernel_size=3,
                        window_size=4, n_contentvec=12)
    enc = ContentVecEncoder(cfg.n_vocab, cfg.n_feats, cfg.n_channels, cfg.filter_channels, cfg.n_heads, cfg.n_layers, cfg.kernel_size, 0.1,
                            n_contentvec=cfg.n_contentvec, window_size=cfg.window_size)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(cfg, 1).items()}, strict=True)
    enc = enc.to(DEV).eval()
    feats, lens, spk = (torch.from_numpy(g[k]).to(DEV) for k in ("feats", "lengths", "spk_emb"))
    n_steps, tp, mel_length = int(g["n_steps"]), int(g["tp"]), int(g["mel_length"])
    z, noise = philox_draws(int(g["noise_key"]), n_steps, TINY.n_feats, tp)
    with fixed_randn_like(z):
        cond_y, dec = model.execute_voice_conversion(feats, lens, [mel_length], spk, enc, len(TINY.dim_mults) - 1, diffusion_steps=n_steps,
                                                     text_gradient_scale=1.7, spk_gradient_scale=0.4, noise=noise)
    assert cond_y.shape[-1] == mel_length
    assert torch.equal(dec, direct_call_on(model, cond_y, tp, z, spk, n_steps, 1.7, 0.4, noise))
    assert not torch.equal(dec, direct_call_on(model, cond_y, tp, z, spk, n_steps, 0.4, 1.7, noise))
