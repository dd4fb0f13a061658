"""ECAPA-TDNN speaker encoder on the HIP library (GPU): the reference goldens, per-stage parity on the tiny ones, run and batch
determinism, edge lengths against the fp64 torch restatement, the normalised form, and the two finetune.py command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402

from unitspeech_amd.speaker_encoder import (ECAPA_TDNN, synthetic_ecapa_state_dict, synthetic_hidden_states,  # noqa: E402
                                            synthetic_speaker_embedder)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL = {"feat_dim": 1024, "channels": 512, "emb_dim": 256, "global_context_att": False, "n_layers": 25}


def _model(cfg, seed):
    m = ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"], global_context_att=cfg["global_context_att"],
                   feat_type="wavlm_large", feat_num=cfg["n_layers"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, seed).items()})
    return m.to(DEV).eval()


def _golden_inputs(g):
    cfg, seed = json.loads(str(g["config"])), int(g["seed"])
    return cfg, seed, torch.from_numpy(synthetic_hidden_states(cfg["n_layers"], int(g["B"]), int(g["T"]), cfg["feat_dim"], seed))


@pytest.mark.parametrize("name", ["speaker_tiny", "speaker_tiny_gca", "speaker_full", "speaker_full_long"])
def test_hip_speaker_encoder_matches_the_reference_golden(golden, name):
    """Measured on MI355X (max|HIP - emb64| / bar): see DESIGN.md, "ECAPA-TDNN speaker encoder"."""
    g = golden(name)
    cfg, seed, hid = _golden_inputs(g)
    out = _model(cfg, seed).forward_features(hid.to(DEV)).cpu().numpy()
    assert out.shape == g["emb64"].shape and np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - g["emb64"]).max())
    floor = float(np.abs(g["emb32"] - g["emb64"]).max())
    tol = max(2e-5, 10 * floor)
    print(f"\n{name}: max|HIP - fp64 reference| = {err:.2e} (fp32 reference {floor:.2e}, tolerance {tol:.1e})")
    assert err <= tol


@pytest.mark.parametrize("name", ["speaker_tiny", "speaker_tiny_gca"])
def test_every_stage_matches_the_reference_intermediates(golden, name):
    """A wrong stage names itself.  Bar per stage: 1e-5 of the stage's largest magnitude (fp32 rounding, 6e-8, through at most ~15
    chained layers of sums of up to 48 products; a wrong tap, pad or scale is off by 1e-2 or more) plus the goldens' absolute 2e-5."""
    g = golden(name)
    cfg, seed, hid = _golden_inputs(g)
    m = _model(cfg, seed)
    assert np.array_equal(hid.numpy(), g["hidden"])
    m.forward_features(hid.to(DEV))
    blocks = m.stage("blocks").cpu().numpy()
    ch = cfg["channels"]
    got = {"feat": m.stage("feat").cpu().numpy(), "layer1": m.stage("layer1").cpu().numpy(), "layer2": blocks[:, :ch], "layer3": blocks[:, ch:2 * ch],
           "layer4": blocks[:, 2 * ch:], "pooling": m.stage("pooling").cpu().numpy()}
    bad = []
    for s, v in got.items():
        assert v.shape == g[s].shape, s
        err, tol = float(np.abs(v.astype(np.float64) - g[s]).max()), 2e-5 + 1e-5 * float(np.abs(g[s]).max())
        print(f"\n{name} {s}: max|HIP - fp64 reference| = {err:.2e} (max|ref| {np.abs(g[s]).max():.2f}, tolerance {tol:.1e})")
        if not err <= tol:
            bad.append(s)
    assert not bad, f"first wrong stage: {bad[0]}"


def test_repeated_runs_and_batch_items_are_bit_identical():
    m = _model(FULL, 5)
    hid = torch.from_numpy(synthetic_hidden_states(25, 3, 211, 1024, 7)).to(DEV)
    batch = m.forward_features(hid)
    assert torch.equal(batch, m.forward_features(hid))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], m.forward_features(hid[:, i:i + 1].contiguous())), i
    tiny = {"feat_dim": 16, "channels": 16, "emb_dim": 8, "global_context_att": True, "n_layers": 3}
    m = _model(tiny, 6)
    hid = torch.from_numpy(synthetic_hidden_states(3, 4, 77, 16, 8)).to(DEV)
    batch = m.forward_features(hid)
    assert torch.equal(batch, m.forward_features(hid))
    for i in range(4):
        assert torch.equal(batch[i:i + 1], m.forward_features(hid[:, i:i + 1].contiguous())), i


@pytest.mark.parametrize("size,T", [("tiny", T) for T in (1, 2, 9, 57, 65, 1499)] + [("full", T) for T in (1, 2, 9, 57, 1499)])
def test_edge_lengths_match_the_torch_restatement(golden, size, T):
    """T = 1, 2, 9 are shorter than the dilated receptive fields (every halo path); 65 puts exactly one step into a second 64-step tile of
    the convolution's loader; 1499 is a 30 s clip.  Bar: the goldens' absolute
    2e-5, or 1e-5 of the largest embedding entry where that is larger (the fp32 floor of the reference itself is 2e-6 at |emb| ~ 1)."""
    cfg = json.loads(str(golden("speaker_tiny")["config"])) if size == "tiny" else FULL
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, 3).items()}
    hid = torch.from_numpy(synthetic_hidden_states(cfg["n_layers"], 2, T, cfg["feat_dim"], 100 + T)).to(DEV)
    out = _model(cfg, 3).forward_features(hid)
    with torch.no_grad():
        ref = ecapa_forward(cfg, sd, hid, dtype=torch.float64)
    assert out.shape == ref.shape == (2, cfg["emb_dim"]) and torch.isfinite(out).all()
    err, tol = float((out.double() - ref).abs().max()), max(2e-5, 1e-5 * float(ref.abs().max()))
    print(f"\n{size} T={T}: max|HIP - fp64 torch restatement| = {err:.2e} (max|ref| {float(ref.abs().max()):.3f}, tolerance {tol:.1e})")
    assert err <= tol


def test_combined_input_and_list_input():
    """[B, C, T] (L = 0: only the InstanceNorm1d) for a module without feature_weight, and a list of L tensors for one with it."""
    cfg = {"feat_dim": 16, "channels": 16, "emb_dim": 8, "global_context_att": False, "n_layers": 0}
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, 9).items()}
    m = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, feat_type="fbank")
    m.load_state_dict(sd)
    x = torch.randn(2, 16, 41, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = m.to(DEV).eval().forward_features(x)
    with torch.no_grad():
        ref = ecapa_forward(cfg, sd, x, dtype=torch.float64)
    assert float((out.double() - ref).abs().max()) <= 2e-5
    cfg3 = dict(cfg, n_layers=3)
    m3 = _model(cfg3, 9)
    hid = torch.from_numpy(synthetic_hidden_states(3, 2, 41, 16, 2)).to(DEV)
    assert torch.equal(m3.forward_features(hid), m3.forward_features([hid[0], hid[1], hid[2]]))


def test_normalised_output_is_raw_over_its_norm():
    m = _model(FULL, 2)
    hid = torch.from_numpy(synthetic_hidden_states(25, 1, 149, 1024, 2)).to(DEV)
    raw, unit = m.forward_features(hid), m.embed(hid)
    want = raw / raw.norm()
    rel = float(((unit - want).abs() / want.abs().clamp_min(1e-30)).max())
    print(f"\nnormalize=1 against raw / raw.norm(): max relative difference {rel:.2e}, |unit| = {float(unit.norm()):.8f}")
    assert unit.shape == (1, 256) and rel <= 2e-7
    with pytest.raises(ValueError, match="one utterance"):
        m.embed(torch.cat([hid, hid], dim=1))


def test_finetune_cli_takes_the_speaker_embedding_from_the_hip_module(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--hip_speaker_encoder", "--n_iters", "2", "--ID", "7",
                        "--out_dir", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    ck = torch.load(tmp_path / "7.pt", map_location="cpu")
    hid = torch.from_numpy(synthetic_hidden_states(25, 1, 149, 1024, 7)).to(DEV)
    want = synthetic_speaker_embedder(256).to(DEV).embed(hid).cpu()
    assert ck["spk_emb"].shape == (1, 1, 256) and torch.equal(ck["spk_emb"].reshape(1, 256), want)
    assert abs(float(want.norm()) - 1.0) <= 1e-6


def test_finetune_cli_features_file_with_hidden_states(tmp_path):
    g = np.random.Generator(np.random.Philox(key=5))
    mel = torch.from_numpy(g.standard_normal((1, 80, 600), dtype=np.float32)).clamp(-1, 1)
    cond_x = torch.from_numpy(g.standard_normal((1, 80, 200), dtype=np.float32)) * 0.5
    hid = torch.from_numpy(synthetic_hidden_states(25, 1, 99, 1024, 11))
    feats = {"mel": mel, "cond_x": cond_x, "duration": torch.full((1, 200), 3.0), "spk_hidden_states": hid, "mel_min": torch.tensor(-11.5),
             "mel_max": torch.tensor(2.0)}
    torch.save(feats, tmp_path / "features.pt")
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(FULL, 12).items()}
    sd["feature_extract.model.mask_emb"] = torch.zeros(1024)
    torch.save({"model": sd}, tmp_path / "embedder.pt")
    base = [sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--features", str(tmp_path / "features.pt"), "--n_iters", "2", "--ID", "8",
            "--out_dir", str(tmp_path)]
    r = subprocess.run(base + ["--speaker_encoder_checkpoint", str(tmp_path / "embedder.pt")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    ck = torch.load(tmp_path / "8.pt", map_location="cpu")
    want = _model(FULL, 12).embed(hid.to(DEV)).cpu()
    assert torch.equal(ck["spk_emb"].reshape(1, 256), want)
    # without the flag the file fails as it always has: spk_emb is missing
    r2 = subprocess.run(base, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode != 0 and "missing `spk_emb`" in r2.stderr and "Traceback" not in r2.stderr
