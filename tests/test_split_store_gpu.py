"""The 16-byte stores of the two-plane fp16 tensors (csrc/pack_f16.h: store_split_pair16).  The memory passes that produce the form -- the
Winograd input transforms (wino4.hip, wino.hip) and gn_apply's out_split / out2 (ops.hip) -- let a lane pair exchange one quad and write two
whole 16-byte pieces where each lane wrote its own two 8-byte ones.  Values and addresses are the same, so the switch (US_SPLIT_STORE16, read
when the handle is created) must not change one bit: ResnetBlocks that reach every converted producer with the switch on against off, one whole
evaluation on against off and batch-independent with it on, and the full-size evaluation against the reference golden.  (The convolution
epilogue's out_split keeps its 8-byte stores; the whole evaluation runs those launches next to the converted ones.)"""
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


def build(sd_np, monkeypatch, forms, store16):
    if forms is None:
        monkeypatch.delenv("US_WINO4", raising=False)
    else:
        monkeypatch.setenv("US_WINO4", forms)
    monkeypatch.setenv("US_SPLIT_STORE16", str(store16))
    m = UnitSpeech(FULL.n_feats, FULL.dim, list(FULL.dim_mults), FULL.beta_min, FULL.beta_max, FULL.pe_scale, FULL.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    m = m.to(DEV).eval()
    m._sync(torch.device(DEV))          # the handle is created here, under this environment
    return m


# (forms, level, ResnetBlock, channels in / out, T).  T = 136 gives W = 68 / 34 / 17 at levels 1 - 3: odd and partial tile counts
CASES = [
    ("0,44,0,0", 1, "estimator.downs.1.1", 256, 256, 136),    # W44, K = 256
    ("0,44,0,0", 1, "estimator.downs.1.0", 128, 256, 136),    # 128 -> 256: the F(2x2) wino_input_kernel (block1) and the W44 GN form (block2)
    ("0,0,0,24", 3, "estimator.downs.3.1", 1024, 1024, 136),  # W24, C = 1024
    (None, 0, "estimator.downs.0.1", 128, 128, 72),           # level 0: gn_apply out_split feeding the pre-split direct convolution, out2 copy
    (None, 1, "estimator.ups.2.0", 512, 128, 136),            # narrow up level, 512 -> 128 with res_conv: gn_apply out2, plus the residual from scratch
]


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
    for store16 in (1, 0):
        model = build(sd_np, monkeypatch, forms, store16)
        got[store16] = (debug_block(model, 1, prefix, level, x * mask, mask_full, temb, cout),      # the whole ResnetBlock
                        debug_block(model, 0, prefix, level, x, ones, None, cout))                   # block1 alone, padded columns shown
        del model
    for on, off in zip(got[1], got[0]):
        assert torch.isfinite(on).all() and float(on.abs().mean()) > 1e-3
        assert torch.equal(on, off)


def test_whole_evaluation_on_against_off_and_batch_independent(sd_np, monkeypatch):
    """One evaluation of the score network: every converted producer at every level, feeding the convolutions that read the planes, next to the
    epilogue's own out_split tensors (attention outputs, Upsample outputs, the final Block's input)."""
    T = 136
    inp = G(synthetic_inputs(FULL, 3, T, seed=41, lengths=[T, T - 16, 8]))
    t = torch.tensor([0.9, 0.4, 0.07])
    outs = {}
    for store16 in (1, 0):
        model = build(sd_np, monkeypatch, "0,44,44,24", store16)
        with torch.no_grad():
            outs[store16] = model.estimator(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), t.to(DEV), inp["spk_emb"].to(DEV)).cpu()
            if store16:
                one = model.estimator(inp["z"][1:2].to(DEV), inp["mask"][1:2].to(DEV), inp["cond"][1:2].to(DEV), t[1:2].to(DEV),
                                      inp["spk_emb"][1:2].to(DEV)).cpu()
        del model
    assert torch.isfinite(outs[1]).all() and float(outs[1].abs().mean()) > 1e-3
    assert torch.equal(outs[1], outs[0])
    assert torch.equal(outs[1][1:2], one)


def test_full_size_evaluation_vs_reference_golden_on_and_off(sd_np, monkeypatch):
    g = G(np.load(os.path.join(GOLD, "estimator_full.npz")))
    outs = {}
    for store16 in (1, 0):
        model = build(sd_np, monkeypatch, "0,44,44,24", store16)
        with torch.no_grad():
            outs[store16] = model.estimator(g["x"].to(DEV), g["mask"].to(DEV), g["mu"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV)).cpu()
        del model
    e32 = float((outs[1].double() - g["out"].double()).abs().mean())
    e64 = float((outs[1].double() - g["out_fp64"].double()).abs().mean())
    print(f"\nUS_SPLIT_STORE16=1: evaluation L1 vs reference fp32 {e32:.2e} / fp64 {e64:.2e}")
    assert e32 <= 2e-6 and e64 <= 2e-6
    assert torch.equal(outs[1], outs[0])
