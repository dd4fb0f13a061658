"""Ragged batches through the HIP BigVGAN (us_vocoder_forward_lengths) on the GPU: every item of a padded batch against the same item run
alone (bit for bit) and against the fp64 torch restatement, NaN past every item's end and in the reused workspace, permutations, two
launch groups, single layers, both weight-norm forms, refusals, and synthesize_batch.py.

The tiny model is the `vocoder_tiny` golden's configuration (rates [4, 2, 2]: hop 16; 32 initial channels; resblock kernels 3 / 7,
dilations 1 / 3 / 5).  Lengths 40 / 33 / 17 / 16 / 8 / 1 frames: 8 frames are exactly one 128-step convolution tile at the last level, 16
exactly one 256-output activation tile there and 17 one frame more, 33 frames are 132 steps at the first level (just over one
convolution tile), and every tile of the 1-frame item's rows past the first lies beyond its end while item 0's are live.

Accuracy bar against fp64: 1e-4, the bar of tests/test_vocoder_gpu.py::test_edge_lengths_match_the_torch_restatement for these models."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vocoder_torch import bigvgan_forward  # noqa: E402

from unitspeech_amd.vocoder import BIGVGAN_22KHZ_80BAND, BigVGAN, synthetic_bigvgan_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [40, 33, 17, 16, 8, 1]
NAN = float("nan")


def _sd(cfg, seed):
    return {k: torch.from_numpy(v) for k, v in synthetic_bigvgan_state_dict(cfg, seed).items()}


def _model(cfg, seed, remove=False, sd=None):
    m = BigVGAN(cfg)
    m.load_state_dict(_sd(cfg, seed) if sd is None else sd)
    m = m.to(DEV).eval()
    if remove:
        m.remove_weight_norm()
    return m


def _mel(B, C, T, seed):
    return torch.randn(B, C, T, generator=torch.Generator().manual_seed(seed)) * 2 - 5


def _padded(mel, lens, Tmax=None, fill=NAN):
    """The batch with `fill` past every item's end (and up to Tmax)."""
    B, C, T = mel.shape
    out = torch.full((B, C, Tmax or T), fill, dtype=mel.dtype, device=mel.device)
    for b, n in enumerate(lens):
        out[b, :, :n] = mel[b, :, :n]
    return out


def _alone(m, mel, lens):
    return [m(mel[b:b + 1, :, :n].contiguous()) for b, n in enumerate(lens)]


def _assert_items(out, alone, lens, hop):
    for b, n in enumerate(lens):
        assert torch.equal(out[b:b + 1, :, :n * hop], alone[b]), (b, n)
        assert (out[b, :, n * hop:] == 0).all(), (b, n)


class Case:
    """The tiny model, its padded batch, and the results every test compares with: computed once, never written to."""

    def __init__(self):
        with np.load(os.path.join(ROOT, "tests", "golden", "vocoder_tiny.npz")) as f:
            self.cfg = json.loads(str(f["config"]))
        assert self.cfg["upsample_rates"] == [4, 2, 2] and self.cfg["upsample_initial_channel"] == 32
        self.seed, self.lens = 3, LENGTHS
        self.m = _model(self.cfg, self.seed)
        self.hop = self.m.hop
        self.clean = _mel(len(self.lens), self.cfg["num_mels"], max(self.lens), 11).to(DEV)
        self.mel = _padded(self.clean, self.lens)
        self.alone = _alone(self.m, self.clean, self.lens)
        self.ragged = self.m(self.mel, lengths=self.lens)


@pytest.fixture(scope="module")
def case():
    return Case()


def test_each_item_has_the_bits_it_has_alone(case):
    assert case.hop == 16 and tuple(case.ragged.shape) == (6, 1, 40 * 16) and torch.isfinite(case.ragged).all()
    _assert_items(case.ragged, case.alone, case.lens, case.hop)


def test_nothing_past_an_items_end_is_used(case):
    m, lens = case.m, case.lens
    m(_padded(case.clean, lens, 48, 0.0))                          # the workspace of the largest call below, then NaN all over it
    m._ws.view(torch.float32).fill_(NAN)
    a = m(case.mel, lengths=lens)
    m._ws.view(torch.float32).fill_(NAN)
    b = m(_padded(case.clean, lens, 48, float("inf")), lengths=torch.tensor(lens))
    assert tuple(b.shape) == (6, 1, 48 * 16)
    for out in (a, b):
        assert torch.isfinite(out).all()
        _assert_items(out, case.alone, lens, case.hop)
    assert torch.equal(a, case.ragged) and torch.equal(b[:, :, :40 * 16], case.ragged)


def _fp64_check(cfg, sd, mel, lens, out, what):
    hop, bad = int(np.prod(cfg["upsample_rates"])), []
    for b, n in enumerate(lens):
        with torch.no_grad():
            ref = bigvgan_forward(cfg, sd, mel[b:b + 1, :, :n].cpu().double())
        err = float((out[b:b + 1, :, :n * hop].cpu().double() - ref).abs().max())
        print(f"\n{what} item {b} ({n} frames): max|HIP - fp64 restatement of the item alone| = {err:.2e} (bar 1.0e-04)")
        if not err <= 1e-4:
            bad.append((b, n, err))
    assert not bad, bad


def test_each_item_matches_the_fp64_restatement_of_the_item_alone(case):
    _fp64_check(case.cfg, _sd(case.cfg, case.seed), case.clean, case.lens, case.ragged, "tiny")
    cfg, lens = BIGVGAN_22KHZ_80BAND, [37, 20, 5]
    sd = _sd(cfg, 3)                                                  # drawn once for the module and the restatement
    m = _model(cfg, 3, sd=sd)
    clean = _mel(3, 80, 37, 37).to(DEV)
    out = m(_padded(clean, lens), lengths=lens)
    assert tuple(out.shape) == (3, 1, 37 * 256) and torch.isfinite(out).all()
    _assert_items(out, _alone(m, clean, lens), lens, 256)
    _fp64_check(cfg, sd, clean, lens, out, "large")


def test_permutations_full_lengths_and_two_launch_groups(case):
    m, lens = case.m, case.lens
    perm = [3, 0, 5, 1, 4, 2]
    got = m(case.mel[perm].contiguous(), lengths=[lens[i] for i in perm])
    assert torch.equal(got, case.ragged[perm])
    assert torch.equal(m(case.clean, lengths=[40] * 6), m(case.clean))
    # more than one launch group of 32 items
    cyc = [1, 8, 9, 16, 17, 24]
    wide_lens = [cyc[i % 6] for i in range(35)]
    clean = _mel(35, case.cfg["num_mels"], 24, 35).to(DEV)
    out = m(_padded(clean, wide_lens), lengths=wide_lens)
    assert tuple(out.shape) == (35, 1, 24 * 16) and torch.isfinite(out).all()
    _assert_items(out, _alone(m, clean, wide_lens), wide_lens, case.hop)


def _layer(m, prefix, cin, lens, rate=1, seed=0, zeros_past_end=False, **epilogue):
    """`prefix` through the ragged launch, NaN past every end in every input, against the uniform launch on each item alone."""
    B, T = len(lens), max(lens)
    x = _padded(_mel(B, cin, T, 100 + seed).to(DEV) + 5, lens)
    cout = m.debug_layer(prefix, x[:1, :, :1].contiguous()).shape[1]
    extra = {k: _padded(_mel(B, cout, T * rate, 200 + seed + i).to(DEV) + 5, [n * rate for n in lens]) for i, k in enumerate(("res", "sum"))
             if epilogue.get(k)}
    div = epilogue.get("div", 0.0)
    out = torch.full((B, cout, T * rate), 7.0, device=DEV)
    got = m.debug_layer(prefix, x, div=div, out=out, lengths=lens, **extra)
    assert got is out
    for b, n in enumerate(lens):
        one = {k: v[b:b + 1, :, :n * rate].contiguous() for k, v in extra.items()}
        want = m.debug_layer(prefix, x[b:b + 1, :, :n].contiguous(), div=div, **one)
        assert torch.isfinite(want).all()
        assert torch.equal(got[b:b + 1, :, :n * rate], want), (prefix, b, n)
        assert (got[b, :, n * rate:] == (0.0 if zeros_past_end else 7.0)).all(), (prefix, b, n)


def test_ragged_layers_alone(case):
    m, cfg = case.m, case.cfg
    conv_lens = [130, 129, 128, 127, 1]
    _layer(m, "conv_pre", cfg["num_mels"], conv_lens, seed=1)
    assert cfg["resblock_kernel_sizes"][1] == 7 and cfg["resblock_dilation_sizes"][1][2] == 5
    _layer(m, "resblocks.1.convs1.2", 16, conv_lens, seed=2)                       # k = 7, d = 5: reach 15
    _layer(m, "resblocks.1.convs2.2", 16, conv_lens, seed=3, res=True, sum=True, div=2.0)
    _layer(m, "ups.0.0", 32, conv_lens, rate=4, seed=4)
    act_lens = [513, 257, 256, 255, 6, 5, 1]
    _layer(m, "resblocks.0.activations.0", 16, act_lens, seed=5)
    _layer(m, "activation_post", 4, act_lens, seed=6)
    _layer(m, "conv_post", 4, [300, 4, 3, 1], seed=7, zeros_past_end=True)


def test_both_weight_norm_forms(case):
    got = _model(case.cfg, case.seed, remove=True)(case.mel, lengths=case.lens)
    assert torch.equal(got, case.ragged)


def test_refusals_name_the_item(case):
    m, mel, lens = case.m, case.mel, case.lens
    with pytest.raises(RuntimeError, match=r"lengths\[2\] = 0"):
        m(mel, lengths=lens[:2] + [0] + lens[3:])
    with pytest.raises(RuntimeError, match=r"lengths\[4\] = 41"):
        m(mel, lengths=lens[:4] + [41] + lens[5:])
    with pytest.raises(RuntimeError, match=r"lengths\[1\] = 131"):
        m.debug_layer("conv_pre", torch.zeros(2, case.cfg["num_mels"], 130, device=DEV), lengths=[130, 131])
    with pytest.raises(ValueError, match=r"5 lengths for 6 items \(item 5 has none\)"):
        m(mel, lengths=lens[:-1])
    with pytest.raises(ValueError, match="7 lengths for 6 items"):
        m(mel, lengths=lens + [1])
    with pytest.raises(ValueError, match="integers"):
        m(mel, lengths=torch.tensor(lens, dtype=torch.float32))
    with pytest.raises(ValueError, match="item 3"):
        m(mel, lengths=lens[:3] + [16.0] + lens[4:])
    assert torch.equal(m(mel, lengths=lens), case.ragged)            # a refused call enqueued nothing and leaves the module as it was


def test_synthesize_batch_tool(tmp_path):
    from scipy.io import wavfile
    import synthesize_batch as S
    out = tmp_path / "tmp"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "synthesize_batch.py"), "--synthetic", "5", "--batch", "3", "--diffusion_steps", "2",
                        "--dump_mel", "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "5 utterances in 2 batches" in r.stdout
    items = S.synthetic_texts(5, 0)
    assert sorted(os.listdir(out)) == sorted([f"{n}.wav" for n, _ in items] + [f"{n}.mel.npy" for n, _ in items])
    vocoder = S.synthetic_vocoder(torch.device(DEV), 0)
    frames = []
    for name, _ in items:
        mel = np.load(out / f"{name}.mel.npy")
        sr, wav = wavfile.read(str(out / f"{name}.wav"))
        assert sr == 22050 and wav.dtype == np.float32 and mel.shape[0] == 80 and mel.dtype == np.float32
        assert wav.shape == (256 * mel.shape[1],) and np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
        want = vocoder(torch.from_numpy(mel)[None].to(DEV)).clamp(-1, 1).cpu().numpy().reshape(-1)
        assert np.array_equal(wav, want), name
        frames.append(mel.shape[1])
    batches = S.plan_batches([len(text) * 2 + 1 for _, text in items], 3, 16384)
    assert any(len({frames[i] for i in b}) > 1 for b in batches), (batches, frames)
