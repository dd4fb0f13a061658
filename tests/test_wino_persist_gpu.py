"""The persistent kernel of the long-K Winograd-domain GEMMs (csrc/conv_igemm.hip: wino_persist_kernel; K >= 512 of the 4-wide forms, a bounded
grid of workgroups that carry the three-buffer pipeline from one tile into the next).  It sums every output element in the general kernel's order,
so switching it (US_WINO_PERSIST, read when the handle is created) must not change one bit: ResnetBlocks with the switch on against off -- with
the default grid, with 7 workgroups (many items each) and with more workgroups than items (empty ones) --, batch independence with it on, and
the full-size evaluation against the reference golden.  (wino_conv() routes K = 1024 and K = 512 except the F(2x4) form's 512 -> 512; that one and
the K = 2048 launch of the cases below stay on the general kernel, DESIGN 4.0e, and must of course not move either.)"""
import os

import numpy as np
import pytest
import torch

from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_inputs, synthetic_state_dict
from test_wino4_gpu import debug_block

pytestmark = pytest.mark.gpu

FULL = DecoderConfig()
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def G(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


@pytest.fixture(scope="module")
def sd_np():
    return synthetic_state_dict(FULL, 0)


def build(sd_np, monkeypatch, forms, persist, wgs=None):
    monkeypatch.setenv("US_WINO4", forms)
    monkeypatch.setenv("US_WINO_PERSIST", str(persist))
    if wgs is None:
        monkeypatch.delenv("US_WINO_PERSIST_WGS", raising=False)
    else:
        monkeypatch.setenv("US_WINO_PERSIST_WGS", str(wgs))
    m = UnitSpeech(FULL.n_feats, FULL.dim, list(FULL.dim_mults), FULL.beta_min, FULL.beta_max, FULL.pe_scale, FULL.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    m = m.to(DEV).eval()
    m._sync(torch.device(DEV))          # the handle is created here, under this environment
    return m


# (forms, level, ResnetBlock, channels in / out, T): with B = 2 the GEMM of a frequency has 2 * tiles rows, never a multiple of the row tile
CASES = [
    ("0,0,44,0", 2, "estimator.downs.2.1", 512, 512, 72),       # 512 -> 512, K = 512, F(4x4): 36 frequencies x 50 rows, 288 items
    ("0,0,0,24", 3, "estimator.mid_block1", 1024, 1024, 72),    # mid1, 1024 -> 1024, F(2x4): 24 frequencies x 30 rows, 384 items for 256 workgroups
    ("0,0,0,24", 3, "estimator.ups.0.0", 2048, 512, 72),        # 2048 -> 512, then 512 -> 512 in the F(2x4) form: neither is routed
    ("0,0,0,44", 3, "estimator.mid_block1", 1024, 1024, 72),    # K = 1024 in the F(4x4) form at level 3: 36 frequencies x 18 rows, 576 items
]
MANY_WGS = 4096        # more workgroups than any case has items


@pytest.mark.parametrize("forms,level,prefix,cin,cout,T", CASES)
def test_resnet_block_is_bit_identical_with_the_switch_on_and_off(sd_np, monkeypatch, forms, level, prefix, cin, cout, T):
    B, H, W = 2, FULL.n_feats >> level, T >> level
    g = np.random.Generator(np.random.Philox(key=3000 + level))
    x = torch.from_numpy(g.standard_normal((B, cin, H, W), dtype=np.float32))
    temb = torch.from_numpy(g.standard_normal((B, FULL.dim + FULL.spk_emb_dim), dtype=np.float32))
    mask_full = torch.ones(B, 1, T)
    mask_full[1, :, T - 24:] = 0
    mask = mask_full[:, :, ::(1 << level)].reshape(B, 1, 1, W)
    ones = torch.ones(B, 1, T)
    got = {}
    for arm, (persist, wgs) in {"off": (0, None), "on": (1, None), "on, 7 workgroups": (1, 7), "on, empty workgroups": (1, MANY_WGS)}.items():
        model = build(sd_np, monkeypatch, forms, persist, wgs)
        got[arm] = (debug_block(model, 1, prefix, level, x * mask, mask_full, temb, cout),      # the whole ResnetBlock
                    debug_block(model, 0, prefix, level, x, ones, None, cout))                   # block1 alone, padded columns shown
        del model
    for arm in ("on", "on, 7 workgroups", "on, empty workgroups"):
        for on, off in zip(got[arm], got["off"]):
            assert torch.isfinite(on).all() and float(on.abs().mean()) > 1e-3, arm
            assert torch.equal(on, off), arm


def test_batch_independence_with_the_switch_on(sd_np, monkeypatch):
    """The items a workgroup walks follow the batch; the order in which an output element is summed does not."""
    model = build(sd_np, monkeypatch, "0,44,44,24", 1)
    T = 136
    inp = G(synthetic_inputs(FULL, 3, T, seed=31, lengths=[T, T - 16, 8]))
    t = torch.tensor([0.9, 0.4, 0.07])
    with torch.no_grad():
        out = model.estimator(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), t.to(DEV), inp["spk_emb"].to(DEV))
        one = model.estimator(inp["z"][1:2].to(DEV), inp["mask"][1:2].to(DEV), inp["cond"][1:2].to(DEV), t[1:2].to(DEV), inp["spk_emb"][1:2].to(DEV))
    assert torch.isfinite(out).all() and torch.equal(out[1:2], one)


def test_full_size_evaluation_vs_reference_golden_on_and_off(sd_np, monkeypatch):
    g = G(np.load(os.path.join(GOLD, "estimator_full.npz")))
    outs = {}
    for persist in (1, 0):
        model = build(sd_np, monkeypatch, "0,44,44,24", persist)
        with torch.no_grad():
            outs[persist] = model.estimator(g["x"].to(DEV), g["mask"].to(DEV), g["mu"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV)).cpu()
        del model
    for persist in (1, 0):
        e32 = float((outs[persist].double() - g["out"].double()).abs().mean())
        e64 = float((outs[persist].double() - g["out_fp64"].double()).abs().mean())
        print(f"\nUS_WINO_PERSIST={persist}: evaluation L1 vs reference fp32 {e32:.2e} / fp64 {e64:.2e}")
        assert e32 <= 2e-6 and e64 <= 2e-6
    assert torch.equal(outs[1], outs[0])
