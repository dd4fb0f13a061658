"""The CPU oracle's `reverse_diffusion` against the sampler goldens of tools/make_goldens_sampler.py: guidance scales that are neither
0 nor 1 and differ from each other, loops longer than one block of precomputed time projections (64 steps), and full-size weights
drawn from seeds 1 and 2.  These pins entitle the oracle to judge the HIP sampler in tests/test_sampler_gpu.py, and the
discrimination test shows that the goldens tell an exchanged, a dropped and a doubled scale from the right one by a wide margin.

Every case runs whole, the two full-size ones included (about ten seconds each on eight CPU threads)."""
import numpy as np
import pytest
import torch

from oracle import decoder_oracle as O
from unitspeech_amd.params import DecoderConfig, synthetic_inputs, synthetic_state_dict

TINY = DecoderConfig(dim=16)
FULL = DecoderConfig()
# the bounds tests/test_oracle_golden.py holds the oracle's loops to: 1e-4 at the tiny width, the 1e-3 loop bar at full size
TINY_BOUND = 1e-4
FULL_BOUND = 1e-3
LOOP_BAR = 1e-3


def T(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def l1(a, b):
    return (a.double() - b.double()).abs().mean().item()


def inputs(cfg, g, n, B, T_):
    """The generator's inputs, rebuilt from the stored seed and checked against the stored checksums."""
    inp = T(synthetic_inputs(cfg, B, T_, seed=int(g["seed"]), n_steps=n, lengths=[int(v) for v in g["lengths"]]))
    for name, key in (("z", "z_abs_sum"), ("noise", f"noise_abs_sum_N{n}" if f"noise_abs_sum_N{n}" in g else "noise_abs_sum")):
        ref = float(g[key])
        assert abs(inp[name].double().abs().sum().item() - ref) <= 1e-9 * ref, name
    return inp


def run(sd, inp, n, wt, ws):
    return O.reverse_diffusion(sd, inp["z"], inp["mask"], inp["cond"], inp["spk_emb"], n, wt, ws, noise=inp["noise"])


@pytest.fixture(scope="module")
def sd_tiny():
    return O.to_torch(synthetic_state_dict(TINY, 0))


@pytest.fixture(scope="module")
def scales(golden):
    g = T(golden("sampler_tiny_scales"))
    return g, inputs(TINY, g, int(g["n_steps"]), 2, 16)


@pytest.mark.parametrize("k", range(4))
def test_oracle_reproduces_the_unequal_scale_goldens(scales, sd_tiny, k):
    g, inp = scales
    wt, ws = float(g["w_text"][k]), float(g["w_spk"][k])
    assert wt != ws and (wt, ws) != (1.0, 1.0)
    out = run(sd_tiny, inp, int(g["n_steps"]), wt, ws)
    e, gap = l1(out, g["out"][k]), l1(g["out"][k], g["out_fp64"][k])
    print(f"\nw=({wt}, {ws}): oracle vs reference fp32 {e:.3e}; reference fp32 vs fp64 {gap:.3e}")
    assert e <= TINY_BOUND
    assert (out * (1 - inp["mask"])).abs().max().item() == 0.0


@pytest.mark.parametrize("n", [64, 65, 130])
def test_oracle_reproduces_the_long_loop_goldens(golden, sd_tiny, n):
    g = T(golden("sampler_tiny_steps"))
    assert n in g["n_steps"].tolist()
    inp = inputs(TINY, g, n, 3, 16)
    out = run(sd_tiny, inp, n, float(g["w_text"]), float(g["w_spk"]))
    e, gap = l1(out, g[f"out_N{n}"]), l1(g[f"out_N{n}"], g[f"out_fp64_N{n}"])
    print(f"\nN={n}: oracle vs reference fp32 {e:.3e}; reference fp32 vs fp64 {gap:.3e}")
    assert e <= TINY_BOUND


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_reproduces_the_other_weight_draws(golden, seed):
    g = T(golden("sampler_full_seeds"))
    assert seed in g["weight_seeds"].tolist()
    n = int(g["n_steps"])
    inp = inputs(FULL, g, n, 1, 64)
    out = run(O.to_torch(synthetic_state_dict(FULL, seed)), inp, n, float(g["w_text"]), float(g["w_spk"]))
    e, gap = l1(out, g[f"out_s{seed}"]), l1(g[f"out_s{seed}"], g[f"out_fp64_s{seed}"])
    print(f"\nweight seed {seed}: oracle vs reference fp32 {e:.3e}; reference fp32 vs fp64 {gap:.3e}")
    assert e <= FULL_BOUND


def wrong_scales(wt, ws):
    """What a sampler with a defect in its scale handling would run instead of (wt, ws): the two exchanged, and each positive one
    replaced by 1.0 (a scale that is dropped looks like 1.0 wherever the suite only ever passed 1.0) alone and together."""
    alts = {(ws, wt), (1.0 if wt > 0 else wt, ws), (wt, 1.0 if ws > 0 else ws), (1.0 if wt > 0 else wt, 1.0 if ws > 0 else ws)}
    return sorted(a for a in alts if a != (wt, ws))


def test_goldens_tell_a_wrong_scale_from_the_right_one(scales, sd_tiny):
    """Every wrong pair lands farther than 100 loop bars from the golden: no test at the 1e-3 bar can pass with one of them."""
    g, inp = scales
    n = int(g["n_steps"])
    for k in range(4):
        wt, ws = float(g["w_text"][k]), float(g["w_spk"][k])
        alts = wrong_scales(wt, ws)
        assert len(alts) >= 2
        for a in alts:
            d = l1(run(sd_tiny, inp, n, *a), g["out"][k])
            print(f"\ngolden w=({wt}, {ws}) vs oracle at w={a}: mean-L1 {d:.3f}")
            assert d > 100 * LOOP_BAR, (wt, ws, a, d)


def test_a_scale_at_or_below_zero_switches_its_branch_off(scales, sd_tiny):
    """`classifier_free_guidance` tests `> 0.0` (unitspeech/unitspeech.py:300-330): a negative scale is a branch not taken."""
    g, inp = scales
    n = int(g["n_steps"])
    assert torch.equal(run(sd_tiny, inp, n, -0.5, 0.3), run(sd_tiny, inp, n, 0.0, 0.3))
    assert l1(run(sd_tiny, inp, n, 0.0, 0.3), g["out"][3]) <= TINY_BOUND
