"""The HIP HuBERT encoder (csrc/hubert.hip) on the GPU against fp64: the goldens written from transformers.HubertModel, and the torch
restatement (tools/hubert_torch.py, pinned to those goldens by tests/test_hubert.py) where the weights are made on the spot.

Accuracy bar, for every compared tensor: the library's max distance from fp64 is at most 10 x the distance of the restatement run in fp32 on the
same input, with a floor of 1e-5 * max |fp64| (the rule of test_duration_train_gpu.py).  Every test prints the two distances.

A ragged batch is compared with its items run alone for BIT equality: every reduction of the library has a fixed order that depends on the
item's own length only, a GEMM column's products are added in the same order wherever its tile lies, and no tile depends on B."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hubert_torch import base_config, frames, hubert_forward_torch, synthetic_hubert_state_dict  # noqa: E402
from units_numpy import kmeans_argmin, run_lengths  # noqa: E402

from unitspeech_amd.hubert import HubertFeatureReader, HubertModel  # noqa: E402
from unitspeech_amd.units import KMeansQuantizer, SpeechEncoder  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
            intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)
TINY64 = dict(TINY, hidden_size=128, intermediate_size=160)          # head dimension 64, the shipped one
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
    m = HubertModel(**cfg)
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


def check_batch(tag, model, cfg, sd, wavs, normalize=False, device="cpu"):
    """One ragged call (NaN past every item's samples) against the restatement in fp64 and fp32, every hidden state of every item."""
    lens = [len(w) for w in wavs]
    x = batch_of(wavs)
    out, hs = model(x.cuda(), lens if len(wavs) > 1 else None, output_hidden_states=True, normalize=normalize)
    r64 = hubert_forward_torch(sd, cfg, x.to(device), lens, torch.float64, normalize)
    r32 = hubert_forward_torch(sd, cfg, x.to(device), lens, torch.float32, normalize)
    assert torch.isfinite(hs).all() and torch.equal(out, hs[:, -1])
    for b, n in enumerate(lens):
        f = frames(cfg, n)
        assert (hs[b, :, f:] == 0).all()
        for l in range(len(r64)):
            check(f"{tag} item {b} ({n} samples, {f} frames) hidden state {l}", hs[b, l, :f], r64[l][b, :f], r32[l][b, :f])
    return out, hs


@pytest.mark.parametrize("name", ["a", "b"])
def test_goldens(golden, name):
    g = golden("hubert_" + name)
    cfg = json.loads(str(g["config"]))
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}
    model = model_of(cfg, sd)
    for i in range(int(g["n_items"])):
        wav, norm = torch.from_numpy(g[f"wav_{i}"]), bool(g[f"normalize_{i}"])
        out, hs = model(wav[None].cuda(), output_hidden_states=True, normalize=norm)
        r32 = hubert_forward_torch(sd, cfg, wav[None], None, torch.float32, norm)
        ref = g[f"hs_{i}"]
        assert tuple(hs.shape) == (1,) + ref.shape and torch.equal(out[0], hs[0, -1])
        for l in range(ref.shape[0]):
            check(f"golden {name} item {i} ({len(wav)} samples{', normalize' if norm else ''}) hidden state {l}", hs[0, l], ref[l], r32[l][0])


@pytest.fixture(scope="module")
def base():
    cfg = base_config()
    sd = synthetic_hubert_state_dict(cfg, 7)
    return cfg, sd, model_of(cfg, sd)


def test_base_configuration(base):
    cfg, sd, model = base
    check_batch("base 2 s", model, cfg, sd, [waveform(32000, 1)])


def test_base_configuration_ragged(base):
    cfg, sd, model = base
    wavs = [waveform(32000, 2), waveform(400, 3, dc=0.5), waveform(20800, 4)]
    assert [frames(cfg, len(w)) for w in wavs] == [99, 1, 64]
    check_batch("base ragged", model, cfg, sd, wavs)


@pytest.fixture(scope="module", params=["d20", "d64"])
def tiny(request):
    cfg = TINY if request.param == "d20" else TINY64
    sd = synthetic_hubert_state_dict(cfg, 5)
    return cfg, sd, model_of(cfg, sd)


def test_attention_tile_edges(tiny):
    """One below, at and one above the 64-query / 64-key tile, and three key tiles with the last partial"""
    cfg, sd, model = tiny
    fr = (QT - 1, QT, QT + 1, 2 * KT + 22)
    wavs = [waveform(samples_for(model, f), 10 + f) for f in fr]
    _, hs = check_batch("edges", model, cfg, sd, wavs)
    # each item alone: the same bits as in the batch
    for b, w in enumerate(wavs):
        _, alone = model(w[None].cuda(), output_hidden_states=True)
        assert torch.equal(alone[0], hs[b, :, :alone.shape[2]]), b
    # a normalised ragged batch: per item over its own samples
    check_batch("edges normalize", model, cfg, sd, [w + 0.25 for w in wavs[:2]], normalize=True)


def test_output_layer(tiny):
    cfg, sd, model = tiny
    wav = waveform(5000, 21)[None].cuda()
    _, hs = model(wav, output_hidden_states=True)
    for n in (0, 1, cfg["num_hidden_layers"]):
        out, h = model(wav, output_layer=n, output_hidden_states=True)
        assert h.shape[1] == n + 1 and torch.equal(out, hs[:, n]) and torch.equal(h, hs[:, :n + 1])
        assert torch.equal(model(wav, output_layer=n), out)
    with pytest.raises(RuntimeError, match="n_layers_out"):
        model(wav, output_layer=cfg["num_hidden_layers"] + 1)


def test_short_item_is_refused(tiny):
    cfg, sd, model = tiny
    with pytest.raises(RuntimeError, match="receptive field"):
        model(torch.zeros(1, 399).cuda())
    with pytest.raises(RuntimeError, match=r"lengths\[1\] = 399"):
        model(torch.zeros(2, 800).cuda(), [800, 399])


def test_guard_regions_and_determinism(tiny):
    """The raw entry point with sentinels after `out` and `hidden_states`, and garbage in the workspace: the same bits twice, nothing written past
    the tensors, rows past an item's frames exactly 0."""
    cfg, sd, model = tiny
    wavs = [waveform(3000, 31), waveform(1100, 32)]
    x, lens = batch_of(wavs).cuda(), [3000, 1100]
    lib, stream = model._sync(x.device)
    B, T, H, L = 2, x.shape[1], cfg["hidden_size"], cfg["num_hidden_layers"]
    F, guard = model.frames(T), 4096
    ws = model._workspace(lib, x.device, B, T)
    results = []
    for fill in (float("nan"), 1e30):
        ws.view(torch.float32).fill_(fill)
        out = torch.full((B * F * H + guard,), -7.0, device="cuda")
        hs = torch.full((B * (L + 1) * F * H + guard,), -7.0, device="cuda")
        assert x.is_cuda and out.is_cuda and hs.is_cuda and ws.is_cuda          # the entry point takes device pointers on trust
        rc = lib.us_hubert_forward(model._h, x.data_ptr(), (C.c_int64 * B)(*lens), B, T, 0, L, out.data_ptr(), hs.data_ptr(), ws.data_ptr(), ws.numel(),
                                   stream)
        assert rc == 0
        assert (out[B * F * H:] == -7.0).all() and (hs[B * (L + 1) * F * H:] == -7.0).all()
        o, h = out[:B * F * H].view(B, F, H), hs[:B * (L + 1) * F * H].view(B, L + 1, F, H)
        assert torch.isfinite(o).all() and torch.isfinite(h).all()
        assert (h[1, :, model.frames(1100):] == 0).all() and (o[1, model.frames(1100):] == 0).all()
        results.append((o.clone(), h.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert torch.equal(model(x, lens), results[0][0])


def test_train_mode_is_refused(tiny):
    cfg, sd, _ = tiny
    m = HubertModel(**cfg).cuda()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 800).cuda())


def test_feature_reader_chunks(tiny):
    cfg, sd, model = tiny
    wav = waveform(7000, 41)
    reader = HubertFeatureReader(model, layer=1, max_chunk=3000).cuda()
    got = reader(wav)
    chunks = [wav[s:s + 3000] for s in range(0, 7000, 3000)]
    assert [len(c) for c in chunks] == [3000, 3000, 1000]
    r64 = torch.cat([hubert_forward_torch(sd, cfg, c[None], None, torch.float64)[1][0] for c in chunks])
    r32 = torch.cat([hubert_forward_torch(sd, cfg, c[None], None, torch.float32)[1][0] for c in chunks])
    assert got.is_cuda and tuple(got.shape) == tuple(r64.shape) == (2 * frames(cfg, 3000) + frames(cfg, 1000), cfg["hidden_size"])
    check("reader, 3 chunks", got, r64, r32)
    whole = HubertFeatureReader(model, layer=1, normalize=True).cuda()(wav)
    n64 = hubert_forward_torch(sd, cfg, wav[None], None, torch.float64, normalize=True)[1][0]
    n32 = hubert_forward_torch(sd, cfg, wav[None], None, torch.float32, normalize=True)[1][0]
    check("reader, one chunk, normalize", whole, n64, n32)


UNITS_SEED = 3          # chosen on the CPU: the smallest fp64 margin over the frames is then about 1e-2 (see the test)


def test_speech_encoder_units():
    cfg = TINY
    sd = synthetic_hubert_state_dict(cfg, 5)
    model = model_of(cfg, sd)
    wav = waveform(20000, 51)
    ref = hubert_forward_torch(sd, cfg, wav[None], None, torch.float64)[2][0].numpy()
    g = np.random.Generator(np.random.Philox(key=UNITS_SEED))
    centers = (ref[g.choice(len(ref), 16, replace=False)] + 0.3 * g.standard_normal((16, ref.shape[1]))).astype(np.float32)
    enc = SpeechEncoder(HubertFeatureReader(model, layer=2), KMeansQuantizer.from_centers(centers), True).cuda()
    got = enc(wav.cuda())
    # a frame's unit is safe when its two nearest centres (fp64) differ in distance by more than twice the feature error: the
    # distance to a centre is 1-Lipschitz in the feature vector
    dist = np.sqrt(((ref[:, None, :] - centers.astype(np.float64)[None]) ** 2).sum(-1))
    two = np.sort(dist, axis=1)[:, :2]
    err = float(np.linalg.norm(got["dense"].double().cpu().numpy() - ref, axis=1).max())
    margin = float((two[:, 1] - two[:, 0]).min())
    print(f"units: {len(ref)} frames, smallest margin {margin:.3e}, largest feature error (L2 per frame) {err:.3e}")
    assert margin > 2 * err, "a frame would have to be excluded"
    want_u, want_d = run_lengths(kmeans_argmin(ref.astype(np.float32), centers))
    assert np.array_equal(kmeans_argmin(ref.astype(np.float32), centers), dist.argmin(1))
    assert np.array_equal(got["units"].cpu().numpy(), want_u) and np.array_equal(got["durations"].cpu().numpy(), want_d)
