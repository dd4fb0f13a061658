"""The HIP WavLM encoder (csrc/hubert.hip, us_wavlm_*) on the GPU against fp64: the goldens written from transformers.WavLMModel, and the
torch restatement (tools/wavlm_torch.py, pinned to those goldens by tests/test_wavlm.py) where the weights are made on the spot; and the
speaker chain wav -> WavLM -> ECAPA-TDNN.

Accuracy bar, for every compared tensor (the rule of test_hubert_gpu.py): the library's max distance from fp64 is at most 10 x the distance of
the restatement run in fp32 on the same input, with a floor of 1e-5 * max |fp64|.  Every test prints the two distances.

A ragged batch is compared with its items run alone for BIT equality, as for HuBERT: the gate is one fixed-order sum per (item, head, frame)
and the bias a table read, so neither depends on the batch."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402
from wavlm_torch import first_saturated_distance, frames, large_config, synthetic_wavlm_state_dict, wavlm_forward_torch  # noqa: E402

from unitspeech_amd.speaker_encoder import ECAPA_TDNN, synthetic_ecapa_state_dict  # noqa: E402
from unitspeech_amd.wavlm import WavLMModel  # noqa: E402

pytestmark = pytest.mark.gpu

COMMON = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
              intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
              num_buckets=32, max_bucket_distance=40)
FORMS = {"large": dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True),
         "base": dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)}
QT = KT = 64                                                            # hb_attn_kernel's query and key tiles


def samples_for(model, f):
    n = 400 + 320 * (f - 1)
    assert model.frames(n) == f and model.frames(n - 1) == f - 1
    return n


def waveform(n, seed, dc=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    y = 0.3 * torch.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * torch.sin(2 * np.pi * 3.0 * t)) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    return (y + dc).to(torch.float32)


def model_of(cfg, sd):
    m = WavLMModel(**cfg)
    m.load_state_dict(sd)
    return m.cuda().eval()


def check(tag, got, r64, r32):
    """got, r64, r32: the same tensor from the library, the fp64 reference and the fp32 restatement"""
    r64 = torch.as_tensor(r64).double().cpu()
    e = float((got.double().cpu() - r64).abs().max())
    s = float((torch.as_tensor(r32).double().cpu() - r64).abs().max())
    mag = float(r64.abs().max())
    print(f"{tag}: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.2f}")
    assert np.isfinite(e) and e <= max(10 * s, 1e-5 * mag), (tag, e, s, mag)


def batch_of(wavs, fill=float("nan")):
    x = torch.full((len(wavs), max(len(w) for w in wavs)), fill)
    for b, w in enumerate(wavs):
        x[b, :len(w)] = w
    return x


def check_batch(tag, model, cfg, sd, wavs, normalize=False):
    """One ragged call (NaN past every item's samples) against the restatement in fp64 and fp32, every hidden state of every item."""
    lens = [len(w) for w in wavs]
    x = batch_of(wavs)
    out, hs = model(x.cuda(), lens if len(wavs) > 1 else None, output_hidden_states=True, normalize=normalize)
    r64 = wavlm_forward_torch(sd, cfg, x, lens, torch.float64, normalize)
    r32 = wavlm_forward_torch(sd, cfg, x, lens, torch.float32, normalize)
    assert torch.isfinite(hs).all() and torch.equal(out, hs[:, -1])
    for b, n in enumerate(lens):
        f = frames(cfg, n)
        assert (hs[b, :, f:] == 0).all()
        for l in range(len(r64)):
            check(f"{tag} item {b} ({n} samples, {f} frames) hidden state {l}", hs[b, l, :f], r64[l][b, :f], r32[l][b, :f])
    return out, hs


@pytest.mark.parametrize("name", ["a", "b"])
def test_goldens(golden, name):
    g = golden("wavlm_" + name)
    cfg = json.loads(str(g["config"]))
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}
    model = model_of(cfg, sd)
    for i in range(int(g["n_items"])):
        wav, norm = torch.from_numpy(g[f"wav_{i}"]), bool(g[f"normalize_{i}"])
        out, hs = model(wav[None].cuda(), output_hidden_states=True, normalize=norm)
        r32 = wavlm_forward_torch(sd, cfg, wav[None], None, torch.float32, norm)
        ref = g[f"hs_{i}"]
        assert tuple(hs.shape) == (1,) + ref.shape and torch.equal(out[0], hs[0, -1])
        for l in range(ref.shape[0]):
            check(f"golden {name} item {i} ({len(wav)} samples{', normalize' if norm else ''}) hidden state {l}", hs[0, l], ref[l], r32[l][0])


@pytest.fixture(scope="module", params=["large-d20", "large-d64", "base-d20", "base-d64"])
def tiny(request):
    form, width = request.param.split("-")
    cfg = dict(COMMON, **FORMS[form])
    if width == "d64":                                                  # head dimension 64, the shipped one
        cfg.update(hidden_size=128, intermediate_size=160)
    sd = synthetic_wavlm_state_dict(cfg, 5)
    return cfg, sd, model_of(cfg, sd)


def test_attention_tile_edges(tiny):
    """One below, at and one above the 64-query / 64-key tile, and three key tiles with the last partial; the buckets saturate at 33 frames, so
    every tile pair holds exact, logarithmic and clamped differences"""
    cfg, sd, model = tiny
    fr = (QT - 1, QT, QT + 1, 2 * KT + 22)
    wavs = [waveform(samples_for(model, f), 10 + f) for f in fr]
    _, hs = check_batch("edges", model, cfg, sd, wavs)
    # each item alone: the same bits as in the batch
    for b, w in enumerate(wavs):
        _, alone = model(w[None].cuda(), output_hidden_states=True)
        assert torch.equal(alone[0], hs[b, :, :alone.shape[2]]), b
    # a normalised ragged batch: per item over its own samples
    shifted = [w + 0.25 for w in wavs]
    _, hn = check_batch("edges normalize", model, cfg, sd, shifted, normalize=True)
    for b, w in enumerate(shifted):
        _, alone = model(w[None].cuda(), output_hidden_states=True, normalize=True)
        assert torch.equal(alone[0], hn[b, :, :alone.shape[2]]), b


@pytest.mark.parametrize("form", ["large", "base"])
def test_table_clamp_at_the_shipped_buckets(form):
    """num_buckets = 320, max_bucket_distance = 800: the table spans [-778, 778]; one item of 253,200 samples (400 + 320 x 790: 791 frames)
    reaches below, through and beyond it"""
    cfg = dict(COMMON, **FORMS[form], num_buckets=320, max_bucket_distance=800)
    assert first_saturated_distance(320, 800) == 778
    sd = synthetic_wavlm_state_dict(cfg, 6)
    model = model_of(cfg, sd)
    wav = waveform(253200, 61)
    assert model.frames(len(wav)) == 791
    check_batch(f"clamp {form}", model, cfg, sd, [wav])


@pytest.fixture(scope="module")
def wide():
    cfg = dict(large_config(), num_hidden_layers=2)
    sd = synthetic_wavlm_state_dict(cfg, 7)
    return cfg, sd, model_of(cfg, sd)


def test_large_widths(wide):
    cfg, sd, model = wide
    check_batch("large widths 2 s", model, cfg, sd, [waveform(32000, 1)])


def test_large_widths_ragged(wide):
    cfg, sd, model = wide
    wavs = [waveform(32000, 2), waveform(400, 3, dc=0.5), waveform(20800, 4)]
    assert [frames(cfg, len(w)) for w in wavs] == [99, 1, 64]
    check_batch("large widths ragged", model, cfg, sd, wavs)


def test_output_layer_and_layers_first(tiny):
    cfg, sd, model = tiny
    wav = waveform(5000, 21)
    x = wav[None].cuda()
    L = cfg["num_hidden_layers"]
    _, hs = model(x, output_hidden_states=True)
    r64 = wavlm_forward_torch(sd, cfg, wav[None], None, torch.float64)
    r32 = wavlm_forward_torch(sd, cfg, wav[None], None, torch.float32)
    for n in (0, 1, L):
        out, h = model(x, output_layer=n, output_hidden_states=True)
        assert h.shape[1] == n + 1 and torch.equal(out, hs[:, n]) and torch.equal(h, hs[:, :n + 1])
        assert torch.equal(model(x, output_layer=n), out)
        check(f"output_layer {n}", out[0], r64[n][0], r32[n][0])                 # pre-LN: the restatement's entry n is un-normalised below L, normalised at L
    with pytest.raises(RuntimeError, match="n_layers_out"):
        model(x, output_layer=L + 1)
    batch = batch_of([wav, waveform(1100, 22)]).cuda()
    for n in (1, L):
        out, h = model(batch, [5000, 1100], output_layer=n, output_hidden_states=True)
        out2, hf = model(batch, [5000, 1100], output_layer=n, output_hidden_states=True, layers_first=True)
        assert tuple(hf.shape) == (n + 1, 2) + tuple(h.shape[2:]) and torch.equal(hf, h.permute(1, 0, 2, 3)) and torch.equal(out, out2)


def test_short_item_is_refused(tiny):
    cfg, sd, model = tiny
    with pytest.raises(RuntimeError, match="receptive field"):
        model(torch.zeros(1, 399).cuda())
    with pytest.raises(RuntimeError, match=r"lengths\[1\] = 399"):
        model(torch.zeros(2, 800).cuda(), [800, 399])


def test_guard_regions_and_determinism(tiny):
    """The raw entry point with sentinels after `out` and `hidden_states`, and garbage in the workspace, in both hidden-state layouts: the same
    bits every time, nothing written past the tensors, rows past an item's frames exactly 0."""
    cfg, sd, model = tiny
    wavs = [waveform(3000, 31), waveform(1100, 32)]
    x, lens = batch_of(wavs).cuda(), [3000, 1100]
    lib, stream = model._sync(x.device)
    B, T, H, L = 2, x.shape[1], cfg["hidden_size"], cfg["num_hidden_layers"]
    F, guard = model.frames(T), 4096
    fh = F * H
    ws = model._workspace(lib, x.device, B, T)
    results = []
    for layers_first in (False, True):
        item, layer = (fh, B * fh) if layers_first else ((L + 1) * fh, fh)
        for fill in (float("nan"), 1e30):
            ws.view(torch.float32).fill_(fill)
            out = torch.full((B * fh + guard,), -7.0, device="cuda")
            hs = torch.full((B * (L + 1) * fh + guard,), -7.0, device="cuda")
            assert x.is_cuda and out.is_cuda and hs.is_cuda and ws.is_cuda          # the entry point takes device pointers on trust
            rc = lib.us_wavlm_forward(model._h, x.data_ptr(), (C.c_int64 * B)(*lens), B, T, 0, L, out.data_ptr(), hs.data_ptr(), item, layer,
                                      ws.data_ptr(), ws.numel(), stream)
            assert rc == 0
            assert (out[B * fh:] == -7.0).all() and (hs[B * (L + 1) * fh:] == -7.0).all()
            o = out[:B * fh].view(B, F, H)
            h = hs[:B * (L + 1) * fh].view(L + 1, B, F, H).permute(1, 0, 2, 3) if layers_first else hs[:B * (L + 1) * fh].view(B, L + 1, F, H)
            assert torch.isfinite(o).all() and torch.isfinite(h).all()
            assert (h[1, :, model.frames(1100):] == 0).all() and (o[1, model.frames(1100):] == 0).all()
            results.append((o.clone(), h.clone()))
    for o, h in results[1:]:
        assert torch.equal(results[0][0], o) and torch.equal(results[0][1], h)
    assert torch.equal(model(x, lens), results[0][0])


def test_train_mode_is_refused(tiny):
    cfg, sd, _ = tiny
    m = WavLMModel(**cfg).cuda()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 800).cuda())


def test_speaker_chain():
    """wav -> WavLM (tiny, large form) -> ECAPA-TDNN in one call: the bits of forward_features on the model's own hidden states, within the bar
    of the trunk's restatement applied to the fp64 WavLM restatement, and embed_wav of unit norm"""
    cfg = dict(COMMON, **FORMS["large"])
    sd = synthetic_wavlm_state_dict(cfg, 8)
    spk_cfg = dict(feat_dim=40, channels=16, emb_dim=8, global_context_att=False, n_layers=3)
    ssd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(spk_cfg, 3).items()}
    trunk = ECAPA_TDNN(feat_dim=40, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)
    trunk.load_state_dict(ssd)
    wavlm = WavLMModel(**cfg)
    wavlm.load_state_dict(sd)
    trunk = trunk.attach_upstream(wavlm, normalize=True).cuda().eval()
    assert trunk.upstream is wavlm and next(wavlm.parameters()).is_cuda
    wavs = torch.stack([waveform(16000, 71), waveform(16000, 72, dc=0.3)])
    emb = trunk(wavs.cuda())
    _, hs = wavlm(wavs.cuda(), output_hidden_states=True, normalize=True, layers_first=True)
    assert tuple(hs.shape) == (3, 2, 49, 40) and tuple(emb.shape) == (2, 8)
    assert torch.equal(emb, trunk.forward_features(hs))
    r64 = ecapa_forward(spk_cfg, ssd, torch.stack(wavlm_forward_torch(sd, cfg, wavs, None, torch.float64, True)), torch.float64)
    r32 = ecapa_forward(spk_cfg, ssd, torch.stack(wavlm_forward_torch(sd, cfg, wavs, None, torch.float32, True)), torch.float32)
    check("speaker chain embedding", emb, r64, r32)
    one = trunk.embed_wav(wavs[:1].cuda())
    assert tuple(one.shape) == (1, 8) and abs(float(one.norm()) - 1.0) < 1e-5
    check("speaker chain embed_wav", one, r64[:1] / r64[:1].norm(), r32[:1] / r32[:1].norm())
