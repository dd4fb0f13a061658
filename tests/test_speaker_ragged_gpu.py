"""Ragged batches through the HIP ECAPA-TDNN trunk (us_speaker_forward_lengths) on the GPU: every item of a padded batch against the
same item run alone (bit for bit) and against the fp64 torch restatement, NaN past every item's end and in the reused workspace,
permutations, refusals, the waveform chain with per-item sample counts, and extract_speaker_embeddings.py.

Lengths 130 / 101 / 65 / 64 / 9 / 2 (and 1 without the global context, where the reference itself gives NaN at T = 1): 130 needs three
64-step convolution tiles and two Res2 tiles at every dilation (100 / 86 / 72 output steps), 101 ends one step into the second
dilation-2 Res2 tile, 65 and 64 straddle the convolution tile, 9, 2 and 1 are shorter than every receptive field.

Accuracy bar against fp64: max(2e-5, 1e-5 * max|ref|), the edge-length bar of tests/test_speaker_encoder_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speaker_encoder_torch import ecapa_forward  # noqa: E402
from wavlm_torch import frames, synthetic_wavlm_state_dict, wavlm_forward_torch  # noqa: E402

from unitspeech_amd.speaker_encoder import ECAPA_TDNN, synthetic_ecapa_state_dict, synthetic_hidden_states  # noqa: E402
from unitspeech_amd.wavlm import WavLMModel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL = {"feat_dim": 1024, "channels": 512, "emb_dim": 256, "global_context_att": False, "n_layers": 25}
LENGTHS = [130, 101, 65, 64, 9, 2]


def _model(cfg, seed):
    m = ECAPA_TDNN(feat_dim=cfg["feat_dim"], channels=cfg["channels"], emb_dim=cfg["emb_dim"], global_context_att=cfg["global_context_att"],
                   feat_type="wavlm_large", feat_num=cfg["n_layers"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg, seed).items()})
    return m.to(DEV).eval()


def _alone(m, hid, lens, fn="forward_features"):
    return torch.cat([getattr(m, fn)(hid[:, b:b + 1, :n].contiguous()) for b, n in enumerate(lens)])


class Case:
    """One tiny model, its padded batch, and the results every test compares with: computed once, never written to."""

    def __init__(self, gca):
        self.cfg = {"feat_dim": 16, "channels": 16, "emb_dim": 8, "global_context_att": gca, "n_layers": 3}
        self.lens = LENGTHS + ([] if gca else [1])
        self.seed = 4 + int(gca)
        self.m = _model(self.cfg, self.seed)
        B, T = len(self.lens), max(self.lens)
        self.hid = torch.from_numpy(synthetic_hidden_states(3, B, T, 16, 40 + int(gca))).to(DEV)
        self.alone = _alone(self.m, self.hid, self.lens)
        self.ragged = self.m.forward_features(self.hid, self.lens)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "global_context"])
def case(request):
    return Case(request.param)


def test_each_item_has_the_bits_it_has_alone(case):
    m, hid, lens = case.m, case.hid, case.lens
    assert tuple(case.ragged.shape) == (len(lens), 8) and torch.isfinite(case.ragged).all()
    for b in range(len(lens)):
        assert torch.equal(case.ragged[b], case.alone[b]), (b, lens[b])
    unit = m.embed(hid, lens)
    want = _alone(m, hid, lens, "embed")
    for b in range(len(lens)):
        assert torch.equal(unit[b], want[b]), (b, lens[b])
    assert float((unit.norm(dim=1) - 1).abs().max()) <= 1e-6
    # the combined [B, C, T] input (L = 0), through a module without feature_weight
    cfg0 = dict(case.cfg, n_layers=0)
    m0 = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, global_context_att=case.cfg["global_context_att"], feat_type="fbank")
    m0.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(cfg0, 9).items()})
    m0 = m0.to(DEV).eval()
    x = hid[0].transpose(1, 2).contiguous()
    got = m0.forward_features(x, lens)
    for b, n in enumerate(lens):
        assert torch.equal(got[b:b + 1], m0.forward_features(x[b:b + 1, :, :n].contiguous())), (b, n)


def test_reference_size_items_have_the_bits_they_have_alone():
    m = _model(FULL, 5)
    lens = [211, 150, 87]
    hid = torch.from_numpy(synthetic_hidden_states(25, 3, 211, 1024, 7)).to(DEV)
    got = m.forward_features(hid, lens)
    assert torch.equal(got, _alone(m, hid, lens))
    assert torch.equal(m.embed(hid, lens), _alone(m, hid, lens, "embed"))


def test_each_item_matches_the_fp64_restatement_of_the_item_alone(case):
    """Ignoring the lengths misses this bar by 5.6e-3 or more on such inputs (padded frames in the instance norm, the SE means, the global
    context and the pooling)."""
    sd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(case.cfg, case.seed).items()}
    hid = case.hid.cpu()
    bad = []
    for b, n in enumerate(case.lens):
        with torch.no_grad():
            ref = ecapa_forward(case.cfg, sd, hid[:, b:b + 1, :n], torch.float64)
        err, tol = float((case.ragged[b:b + 1].cpu().double() - ref).abs().max()), max(2e-5, 1e-5 * float(ref.abs().max()))
        print(f"\nitem {b} ({n} frames): max|HIP - fp64 restatement| = {err:.2e} (max|ref| {float(ref.abs().max()):.3f}, tolerance {tol:.1e})")
        if not err <= tol:
            bad.append((b, n, err))
    assert not bad, bad


def test_nothing_past_an_items_end_is_used(case):
    m, lens = case.m, case.lens
    nan = torch.full_like(case.hid, float("nan"))
    m.forward_features(nan)                                        # a uniform call on NaN alone: the workspace the next call reuses is what it left,
    m._ws.view(torch.float32).fill_(float("nan"))                  # and (ReLU turns a NaN into 0) NaN written over all of it as well
    hid = case.hid.clone()
    for b, n in enumerate(lens):
        hid[:, b, n:] = float("nan")
    got = m.forward_features(hid, lens)
    assert torch.isfinite(got).all() and torch.equal(got, case.ragged)
    feat = m.stage("feat")
    for b, n in enumerate(lens):
        assert torch.isfinite(feat[b, :, :n]).all() and (feat[b, :, n:] == 0).all(), b


def test_permutations_full_lengths_and_repeats(case):
    m, hid, lens = case.m, case.hid, case.lens
    perm = [3, 0, 5, 1, 4, 2] + list(range(6, len(lens)))
    got = m.forward_features(hid[:, perm].contiguous(), [lens[i] for i in perm])
    assert torch.equal(got, case.ragged[perm])
    T = hid.shape[2]
    assert torch.equal(m.forward_features(hid, [T] * len(lens)), m.forward_features(hid))
    assert torch.equal(m.forward_features(hid, torch.tensor(lens)), case.ragged)
    # more than one launch group of 32 items: item 32 + k is item k again
    reps = 6
    wide = hid.repeat(1, reps, 1, 1)[:, :35].contiguous()
    got = m.forward_features(wide, (lens * reps)[:35])
    assert torch.equal(got, case.ragged.repeat(reps, 1)[:35])


def test_refusals_name_the_item(case):
    m, hid, lens = case.m, case.hid, case.lens
    T = hid.shape[2]
    with pytest.raises(RuntimeError, match=r"lengths\[2\] = 0"):
        m.forward_features(hid, lens[:2] + [0] + lens[3:])
    with pytest.raises(RuntimeError, match=rf"lengths\[4\] = {T + 1}"):
        m.forward_features(hid, lens[:4] + [T + 1] + lens[5:])
    with pytest.raises(ValueError, match=rf"{len(lens) - 1} lengths for {len(lens)} items \(item {len(lens) - 1} has none\)"):
        m.forward_features(hid, lens[:-1])
    with pytest.raises(ValueError, match="item 1"):
        m.embed(hid)
    assert torch.equal(m.forward_features(hid, lens), case.ragged)          # a refused call leaves the module as it was


# the tiny WavLM (large form) and trunk of tests/test_wavlm_gpu.py::test_speaker_chain
WAVLM = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
             intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5,
             num_buckets=32, max_bucket_distance=40, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
SPK = dict(feat_dim=40, channels=16, emb_dim=8, global_context_att=False, n_layers=3)


def _waveform(n, seed, dc=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    y = 0.3 * torch.sin(2 * torch.pi * 180.0 * t) * (0.6 + 0.4 * torch.sin(2 * torch.pi * 3.0 * t)) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    return (y + dc).to(torch.float32)


def test_waveform_chain_with_sample_counts():
    sd = synthetic_wavlm_state_dict(WAVLM, 8)
    ssd = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(SPK, 3).items()}
    trunk = ECAPA_TDNN(feat_dim=40, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)
    trunk.load_state_dict(ssd)
    wavlm = WavLMModel(**WAVLM)
    wavlm.load_state_dict(sd)
    trunk = trunk.attach_upstream(wavlm, normalize=True).cuda().eval()
    wavs, lens = [_waveform(16000, 71), _waveform(9000, 72, dc=0.3)], [16000, 9000]
    x = torch.full((2, 16000), float("nan"))
    for b, w in enumerate(wavs):
        x[b, :len(w)] = w
    fr = [frames(WAVLM, n) for n in lens]
    assert fr == [49, 27] and [wavlm.frames(n) for n in lens] == fr
    emb = trunk(x.cuda(), lens)
    _, hs = wavlm(x.cuda(), lens, output_hidden_states=True, normalize=True, layers_first=True)
    assert tuple(hs.shape) == (3, 2, 49, 40) and tuple(emb.shape) == (2, 8) and torch.isfinite(emb).all()
    assert torch.equal(emb, trunk.forward_features(hs, fr))
    bad = []
    for b, w in enumerate(wavs):
        ref = ecapa_forward(SPK, ssd, torch.stack(wavlm_forward_torch(sd, WAVLM, w[None], None, torch.float64, True)), torch.float64)
        err, tol = float((emb[b:b + 1].cpu().double() - ref).abs().max()), max(2e-5, 1e-5 * float(ref.abs().max()))
        print(f"\nchain item {b} ({lens[b]} samples, {fr[b]} frames): max|HIP - fp64 restatements| = {err:.2e} (max|ref| "
              f"{float(ref.abs().max()):.3f}, tolerance {tol:.1e})")
        if not err <= tol:
            bad.append((b, err, tol))
        assert torch.equal(emb[b:b + 1], trunk(w[None].cuda())), b                 # and the bits of the waveform alone
    assert not bad, bad
    unit = trunk.embed_wav(x.cuda(), lens)
    assert tuple(unit.shape) == (2, 8) and float((unit.norm(dim=1) - 1).abs().max()) <= 1e-5
    assert torch.equal(unit[1:], trunk.embed_wav(wavs[1][None].cuda()))


def test_extract_speaker_embeddings_tool(tmp_path):
    import extract_speaker_embeddings as X
    out = tmp_path / "embs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "extract_speaker_embeddings.py"), "--synthetic", "12", "--speakers", "3", "--batch", "4",
                        "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "12 utterances in 3 batches" in r.stdout and "3 speakers" in r.stdout
    data = X.synthetic_dataset(12, 3, 0)
    embedder = X.synthetic_embedder(torch.device(DEV), 0)
    rows, resamplers = {}, {}
    for _, spk, wav in data:
        w16 = X.to_16k(wav, X.SYNTHETIC_RATE, torch.device(DEV), resamplers)
        rows.setdefault(spk, []).append(embedder(w16[None])[0].cpu())               # one utterance at a time, no lengths
    assert sorted(os.listdir(out)) == sorted([f"{s}.pt" for s in rows] + ["spk_uncond.pt"]) and len(rows) == 3
    means = []
    for spk, v in rows.items():
        got = torch.load(out / f"{spk}.pt", map_location="cpu")
        assert tuple(got.shape) == (1, 8) and got.dtype == torch.float32
        assert torch.equal(got, torch.stack(v).mean(0)[None]), spk
        ref = X.running_mean(v)
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), spk
        means.append(got)
    uncond = torch.load(out / "spk_uncond.pt", map_location="cpu")
    assert tuple(uncond.shape) == (1, 1, 8) and torch.equal(uncond, torch.stack(means).mean(0, keepdim=True))
