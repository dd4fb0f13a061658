"""The streaming kernel of the short-K Winograd-domain GEMMs (csrc/conv_igemm.hip: wino_stream_kernel; K = 256 of the 4-wide forms, the
weights of a workgroup's 256 columns in registers, only V streamed through LDS).  It sums every output element in the general kernel's order, so
switching it (US_WINO_STREAM, read when the handle is created) must not change one bit: ResnetBlocks whose launches reach every branch of the
kernel with the switch on against off, batch independence with it on, and the full-size evaluation against the reference golden."""
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


def build(sd_np, monkeypatch, forms, stream):
    monkeypatch.setenv("US_WINO4", forms)
    monkeypatch.setenv("US_WINO_STREAM", str(stream))
    m = UnitSpeech(FULL.n_feats, FULL.dim, list(FULL.dim_mults), FULL.beta_min, FULL.beta_max, FULL.pe_scale, FULL.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    m = m.to(DEV).eval()
    m._sync(torch.device(DEV))          # the handle is created here, under this environment
    return m


# (forms, level, ResnetBlock, channels in / out, T): with B = 2 the GEMM of a frequency has 2 * tiles rows
CASES = [
    ("0,44,0,0", 1, "estimator.downs.1.1", 256, 256, 136),    # 256 -> 256; 2 x 170 tiles = 340 rows: a partial last row tile, row groups of 1 and 2 tiles
    ("0,44,0,0", 1, "estimator.downs.1.0", 128, 256, 72),     # block2 256 -> 256 at 2 x 90 rows (block1's K = 128 has no 4-wide form and is not routed)
    ("0,0,44,0", 2, "estimator.downs.2.0", 256, 512, 72),     # 256 -> 512: two column groups, 50 rows (block2's K = 512 stays on the general kernel)
    ("0,0,24,0", 2, "estimator.downs.2.0", 256, 512, 72),     # F(2x4): 24 frequencies
]


@pytest.mark.parametrize("forms,level,prefix,cin,cout,T", CASES)
def test_resnet_block_is_bit_identical_with_the_switch_on_and_off(sd_np, monkeypatch, forms, level, prefix, cin, cout, T):
    B, H, W = 2, FULL.n_feats >> level, T >> level
    g = np.random.Generator(np.random.Philox(key=2000 + level))
    x = torch.from_numpy(g.standard_normal((B, cin, H, W), dtype=np.float32))
    temb = torch.from_numpy(g.standard_normal((B, FULL.dim + FULL.spk_emb_dim), dtype=np.float32))
    mask_full = torch.ones(B, 1, T)
    mask_full[1, :, T - 24:] = 0
    mask = mask_full[:, :, ::(1 << level)].reshape(B, 1, 1, W)
    ones = torch.ones(B, 1, T)
    got = {}
    for stream in (1, 0):
        model = build(sd_np, monkeypatch, forms, stream)
        got[stream] = (debug_block(model, 1, prefix, level, x * mask, mask_full, temb, cout),      # the whole ResnetBlock
                       debug_block(model, 0, prefix, level, x, ones, None, cout))                   # block1 alone, padded columns shown
        del model
    for on, off in zip(got[1], got[0]):
        assert torch.isfinite(on).all() and float(on.abs().mean()) > 1e-3
        assert torch.equal(on, off)


def test_batch_independence_with_the_switch_on(sd_np, monkeypatch):
    """The row-group count of the streaming kernel follows the batch; the order in which an output element is summed does not."""
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
    for stream in (1, 0):
        model = build(sd_np, monkeypatch, "0,44,44,24", stream)
        with torch.no_grad():
            outs[stream] = model.estimator(g["x"].to(DEV), g["mask"].to(DEV), g["mu"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV)).cpu()
        del model
    e32 = float((outs[1].double() - g["out"].double()).abs().mean())
    e64 = float((outs[1].double() - g["out_fp64"].double()).abs().mean())
    print(f"\nUS_WINO_STREAM=1: evaluation L1 vs reference fp32 {e32:.2e} / fp64 {e64:.2e}")
    assert e32 <= 2e-6 and e64 <= 2e-6
    assert torch.equal(outs[1], outs[0])
