"""One whole STEP1 iteration on the GPU (unitspeech_amd.tts_train.compute_train_step_loss) against the reference's
train_STEP1.compute_train_step_loss (tests/golden/tts_step1_tiny.npz, tools/make_goldens_tts_train.py), gradient routing, and the
train_tts.py / bench_tts_step.py command lines."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_state_dict
from unitspeech_amd.encoder import (DurationPredictor, DurationPredictorConfig, Encoder, EncoderConfig, _EncoderTrain,
                                    synthetic_duration_predictor_state_dict, synthetic_encoder_state_dict)
from unitspeech_amd.tts_train import compute_train_step_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EC = EncoderConfig(n_vocab=50, n_feats=80, n_channels=32, filter_channels=64, n_heads=2, n_layers=2, kernel_size=3, window_size=4)
DC = DecoderConfig(dim=16, dim_mults=(1, 2), spk_emb_dim=16)
PC = DurationPredictorConfig(in_channels=32, filter_channels=24, kernel_size=3, spk_emb_dim=16)


def modules():
    enc = Encoder(EC.n_vocab, EC.n_feats, EC.n_channels, EC.filter_channels, EC.n_heads, EC.n_layers, EC.kernel_size, 0.1,
                  window_size=EC.window_size, trainable=True)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(EC, 0).items()}, strict=True)
    dp = DurationPredictor(PC.in_channels, PC.filter_channels, PC.kernel_size, 0.1, spk_emb_dim=PC.spk_emb_dim, trainable=True)
    dp.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_duration_predictor_state_dict(PC, 0).items()}, strict=True)
    dec = UnitSpeech(DC.n_feats, DC.dim, list(DC.dim_mults), DC.beta_min, DC.beta_max, DC.pe_scale, DC.spk_emb_dim)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(DC, 0).items()}, strict=True)
    enc, dp, dec = enc.cuda().train(), dp.cuda().eval(), dec.cuda().eval()
    params = list(enc.state_dict(keep_vars=True).values())
    text_encoder = lambda x, l: _EncoderTrain.apply(enc, x, l, 0, -1.0, *params)       # the reference ran in eval mode
    return enc, text_encoder, dp, dec


def run(g, out_size, aux=None, with_z=True):
    T = lambda k: torch.from_numpy(g[k]).cuda()
    enc, text_encoder, dp, dec = modules()
    orig, z = torch.randn, T("z")
    if with_z:
        torch.randn = lambda *a, **k: z.clone()
    try:
        losses = compute_train_step_loss(text_encoder, dp, dec, T("x"), T("x_lengths"), T("y"), T("y_lengths"), T("spk").unsqueeze(1),
                                         out_size, starts=[int(v) for v in g["starts"]], t=T("t"), aux=aux)
    finally:
        torch.randn = orig
    return enc, dp, dec, losses


def test_one_step1_iteration_matches_the_reference(golden):
    g = golden("tts_step1_tiny")
    aux = {}
    enc, dp, dec, (dur, prior, diff) = run(g, 32, aux)
    assert np.array_equal(aux["attn"].cpu().numpy(), g["attn"])                                           # the alignment is EQUAL, not close
    (dur + prior + diff).backward()
    print(f"dur {float(dur):.6f}/{float(g['dur_loss']):.6f} prior {float(prior):.6f}/{float(g['prior_loss']):.6f} "
          f"diff {float(diff):.6f}/{float(g['diff_loss']):.6f}")
    assert abs(float(dur) - float(g["dur_loss"])) <= 1e-5 * abs(float(g["dur_loss"]))
    assert abs(float(prior) - float(g["prior_loss"])) <= 1e-5 * abs(float(g["prior_loss"]))
    assert abs(float(diff) - float(g["diff_loss"])) <= 1e-4 * abs(float(g["diff_loss"]))
    seen = 0
    for tag, m in (("enc", enc), ("dp", dp), ("dec", dec)):
        names = [k for k, _ in m.named_parameters()]
        scale = max(float(np.linalg.norm(g[f"grad/{tag}/{k}"])) for k in names if f"grad/{tag}/{k}" in g)
        for k, p in m.named_parameters():
            if f"grad/{tag}/{k}" not in g:               # the reference left it None (the decoder's text_uncon is not read by the loss)
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (tag, k)
                continue
            ref = torch.from_numpy(g[f"grad/{tag}/{k}"]).double()
            assert p.grad is not None, (tag, k)
            e = float((p.grad.double().cpu() - ref).norm()) / max(float(ref.norm()), 1e-3 * scale)
            assert e <= 1e-3, (tag, k, e)
            seen += 1
    assert seen == sum(1 for k in g if k.startswith("grad/"))                        # no key left out


def test_gradient_routing_and_the_uncropped_step(golden):
    g = golden("tts_step1_tiny")
    enc, dp, dec, (dur, prior, diff) = run(g, 32)
    (prior + diff).backward()
    assert all(p.grad is None for p in dp.parameters())                              # the predictor learns from logw only
    assert all(p.grad is not None for p in enc.parameters())
    enc, dp, dec, (dur, prior, diff) = run(g, 32)
    dur.backward()
    assert all(p.grad is None for p in enc.parameters())                             # the detach
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in dp.parameters())
    aux = {}
    enc, dp, dec, losses = run(g, None, aux, with_z=False)
    Ty = g["y"].shape[-1]
    assert aux["mu_y"].shape == (3, 80, Ty) and aux["y_mask"].shape == (3, 1, Ty) and aux["attn"].shape[-1] == Ty
    assert np.array_equal(aux["attn"].cpu().numpy(), g["attn"])
    assert np.array_equal(aux["y_mask"].sum((1, 2)).cpu().numpy().astype(np.int64), g["y_lengths"])
    assert all(math.isfinite(float(v)) for v in losses)


def test_train_tts_script_runs_and_the_losses_fall(tmp_path):
    from unitspeech_amd.checkpoint import load_decoder_checkpoint
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_tts.py"), "--synthetic", "--n_iters", "20", "--batch_size", "4",
                        "--log_dir", str(tmp_path)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    num = r"([-\d.eE+naif]+)"
    losses = [tuple(float(v) for v in m) for m in re.findall(rf"dur_loss {num} prior_loss {num} diff_loss {num}", r.stdout)]
    assert len(losses) == 20
    assert all(math.isfinite(v) for l in losses for v in l)
    assert losses[-1][0] < losses[0][0] and losses[-1][1] < losses[0][1]
    assert len(re.findall(r"grad_norm text_encoder [\d.]+ duration_predictor [\d.]+ decoder [\d.]+", r.stdout)) == 20
    ck = load_decoder_checkpoint(os.path.join(str(tmp_path), "pretrained_decoder.pt"))
    assert ck.iteration == 20 and isinstance(ck.spk_emb, dict)
    dc = DecoderConfig()
    ec = EncoderConfig(n_feats=dc.n_feats)
    pc = DurationPredictorConfig(in_channels=ec.n_channels, spk_emb_dim=dc.spk_emb_dim)
    esd = torch.load(os.path.join(str(tmp_path), "text_encoder.pt"), map_location="cpu")["model"]
    psd = torch.load(os.path.join(str(tmp_path), "duration_predictor.pt"), map_location="cpu")["model"]
    gen = torch.Generator().manual_seed(0)
    ids, lens = torch.randint(0, ec.n_vocab, (2, 30), generator=gen).cuda(), torch.LongTensor([30, 17]).cuda()
    spk = torch.randn(2, 1, pc.spk_emb_dim, generator=gen).cuda()
    outs = []
    for trainable in (False, True):
        kw = dict(trainable=True) if trainable else {}
        enc = Encoder(ec.n_vocab, ec.n_feats, ec.n_channels, ec.filter_channels, ec.n_heads, ec.n_layers, ec.kernel_size, 0.1,
                      window_size=ec.window_size, **kw)
        dp = DurationPredictor(pc.in_channels, pc.filter_channels, pc.kernel_size, 0.1, spk_emb_dim=pc.spk_emb_dim, **kw)
        enc.load_state_dict(esd, strict=True)
        dp.load_state_dict(psd, strict=True)
        enc, dp = enc.cuda().eval(), dp.cuda().eval()
        with torch.no_grad():
            mu_x, h, mask = enc(ids, lens)
            outs.append((mu_x, dp(h, mask, g=spk, reverse=True)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][1]).all())


def test_bench_tts_step_quick_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tts_step.py"), "--quick"], capture_output=True, text=True, timeout=900,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["bench"] == "tts_step1" and d["predictor"] and d["step1"]["median_ms"] > 0
    for row in d["predictor"]:
        assert row["hip"]["median_ms"] > 0 and row["eager"]["median_ms"] > 0 and {"min_ms", "max_ms"} <= set(row["hip"])
    assert set(d["step1"]["stages_ms"]) == {"encoder_fwd", "predictor_fwd", "alignment", "decoder_loss", "backward", "optimiser"}
