"""The recogniser's end on the GPU (csrc/ctc.hip, unitspeech_amd/asr.py, evaluate.py).

Accuracy bar for every compared float tensor, the rule of test_hubert_gpu.py: the library's max distance from fp64 is at most 10 x the
distance of the fp32 torch restatement on the same input, with a floor of 1e-5 * max |fp64|.  Every test prints the two distances.
Every integer (ids against the written logits, tokens, first frames, counts, distances) is compared for equality with the numpy yardstick
(tools/ctc_numpy.py).  An item of a ragged batch is compared with the item run alone for BIT equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_numpy as Y  # noqa: E402
from hubert_torch import hubert_forward_torch  # noqa: E402

from unitspeech_amd import _lib, asr  # noqa: E402

pytestmark = pytest.mark.gpu


def check(tag, got, r64, r32):
    """got, r64, r32: the same tensor from the library, the fp64 reference and the fp32 restatement"""
    r64 = torch.as_tensor(r64).double().cpu()
    e = float((got.double().cpu() - r64).abs().max())
    s = float((torch.as_tensor(r32).double().cpu() - r64).abs().max())
    mag = float(r64.abs().max())
    print(f"{tag}: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.2f}")
    assert np.isfinite(e) and e <= max(10 * s, 1e-5 * mag), (tag, e, s, mag)
    return e


# (B, Tmax, H, V, lengths): one row; three tiles of 64 rows with a partial one; V off every tile multiple; the largest H with V across
# five vocabulary tiles.  The lengths hold 0 and Tmax.
HEAD_CASES = [(1, 1, 4, 2, [1]), (1, 1, 4, 2, [0]), (3, 70, 40, 12, [70, 0, 33]), (2, 130, 48, 33, [0, 130]), (2, 65, 1024, 257, [65, 0])]


@pytest.mark.parametrize("B,T,H,V,lens", HEAD_CASES)
def test_head_alone(B, T, H, V, lens):
    g = torch.Generator().manual_seed(100 * H + V + sum(lens))
    x = torch.randn(B, T, H, generator=g)
    head = asr.CTCHead(H, V)
    head.load_state_dict({"weight": torch.randn(V, H, generator=g), "bias": torch.randn(V, generator=g)})
    xd = x.clone()
    for b, n in enumerate(lens):
        xd[b, n:] = float("nan")                       # rows past an item's frames are never read
    head = head.cuda()
    logits, lp = head(xd.cuda(), lens, log_probs=True)
    logits2, ids = head.argmax(xd.cuda(), lens)
    assert torch.equal(logits, logits2) and tuple(logits.shape) == tuple(lp.shape) == (B, T, V) and tuple(ids.shape) == (B, T)
    for b, n in enumerate(lens):
        assert (logits[b, n:] == 0).all() and (lp[b, n:] == 0).all() and (ids[b, n:] == -1).all()
        if n == 0:
            continue
        tag = f"head B{B} T{T} H{H} V{V} item {b} ({n} frames)"
        W, bias = head.weight.cpu(), head.bias.cpu()
        r64 = x[b, :n].double() @ W.double().T + bias.double()
        r32 = F.linear(x[b, :n], W, bias)
        check(tag + " logits", logits[b, :n], r64, r32)
        check(tag + " log_probs", lp[b, :n], F.log_softmax(r64, -1), F.log_softmax(r32, -1))
        # the argmax of the logits as written, exactly
        assert torch.equal(ids[b, :n], logits[b, :n].argmax(-1))
        # log_probs is normalised: logsumexp is 0, by the same rule against torch's fp32 log_softmax of the same logits
        lse = torch.logsumexp(lp[b, :n].double().cpu(), -1)
        lse32 = torch.logsumexp(F.log_softmax(logits[b, :n].cpu(), -1).double(), -1)
        e, s, mag = float(lse.abs().max()), float(lse32.abs().max()), float(F.log_softmax(r64, -1).abs().max())
        print(f"{tag} logsumexp(log_probs): library {e:.3e}  fp32 log_softmax {s:.3e}  max|ref| {mag:.2f}")
        assert e <= max(10 * s, 1e-5 * mag)
        # the item alone: the same bits
        a_logits, a_lp = head(x[b:b + 1, :n].cuda(), log_probs=True)
        _, a_ids = head.argmax(x[b:b + 1, :n].cuda())
        assert torch.equal(a_logits[0], logits[b, :n]) and torch.equal(a_lp[0], lp[b, :n]) and torch.equal(a_ids[0], ids[b, :n])


def test_head_ties_take_the_lower_index():
    head = asr.CTCHead(4, 70).cuda()                    # zero weights: every logit is the bias
    bias = torch.zeros(70)
    bias[[5, 68]] = 2.0
    head.load_state_dict({"weight": torch.zeros(70, 4), "bias": bias})
    _, ids = head.argmax(torch.randn(1, 3, 4).cuda())
    assert ids.tolist() == [[5, 5, 5]]


@pytest.mark.parametrize("name,cls", [("a", asr.HubertForCTC), ("b", asr.Wav2Vec2ForCTC)])
def test_goldens(golden, name, cls):
    g = golden("ctc_" + name)
    cfg = json.loads(str(g["config"]))
    sd = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}
    model = cls(**cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    prefix = cls._prefix + "."
    enc_sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    blank, margin = cfg["pad_token_id"], float(g["min_margin"])
    wavs, want = [], []
    for i in range(int(g["n_items"])):
        wav = torch.from_numpy(g[f"wav_{i}"])
        logits = model(wav[None].cuda())
        r32 = F.linear(hubert_forward_torch(enc_sd, cfg, wav[None], None, torch.float32)[-1][0], sd["lm_head.weight"], sd["lm_head.bias"])
        assert tuple(logits.shape) == (1,) + g[f"logits_{i}"].shape
        e = check(f"golden {name} item {i} ({len(wav)} samples) logits", logits[0], g[f"logits_{i}"], r32)
        print(f"golden {name} item {i}: min_margin {margin:.3e} against 100 x error {100 * e:.3e}")
        assert margin > 100 * e
        assert np.array_equal(logits[0].argmax(-1).cpu().numpy(), g[f"ids_{i}"])
        tokens, n, first = model.transcribe_ids(wav[None].cuda(), first_frame=True)
        wt, wf = Y.ctc_collapse(g[f"ids_{i}"], blank)
        assert int(n[0]) == len(wt) and np.array_equal(tokens[0, :len(wt)].cpu().numpy(), wt)
        assert np.array_equal(first[0, :len(wt)].cpu().numpy(), wf) and (tokens[0, len(wt):] == 0).all()
        wavs.append(wav)
        want.append(wt)
    # the four items as one ragged batch: the same tokens
    lens = [len(w) for w in wavs]
    x = torch.full((len(wavs), max(lens)), float("nan"))
    for b, w in enumerate(wavs):
        x[b, :lens[b]] = w
    tokens, n = model.transcribe_ids(x.cuda(), lens)
    for b, wt in enumerate(want):
        assert int(n[b]) == len(wt) and np.array_equal(tokens[b, :len(wt)].cpu().numpy(), wt) and (tokens[b, len(wt):] == 0).all()


def check_collapse(ids, lens, blank):
    """ids [B, Tmax] (numpy, anything past the lengths) against the yardstick, first frames included"""
    B, T = ids.shape
    tokens, n, first = asr.ctc_collapse(torch.from_numpy(ids).cuda(), None if lens is None else torch.tensor(lens), blank, first_frame=True)
    tokens2, n2 = asr.ctc_collapse(torch.from_numpy(ids).cuda(), None if lens is None else lens, blank)
    assert torch.equal(tokens, tokens2) and torch.equal(n, n2)
    tokens, n, first = tokens.cpu().numpy(), n.cpu().numpy(), first.cpu().numpy()
    for b in range(B):
        wt, wf = Y.ctc_collapse(ids[b, :T if lens is None else lens[b]], blank)
        assert n[b] == len(wt), b
        assert np.array_equal(tokens[b, :len(wt)], wt) and np.array_equal(first[b, :len(wt)], wf), b
        assert (tokens[b, len(wt):] == 0).all() and (first[b, len(wt):] == 0).all(), b
    return n


def test_collapse_crafted_rows():
    a, c, blank = 5, 7, 0
    ids = np.array([[blank, blank, blank, blank], [a, c, a, c], [a, a, blank, a], [-1, -1, -1, -1], [c, -1, -1, -1]], dtype=np.int64)
    n = check_collapse(ids, [4, 4, 4, 0, 1], blank)
    assert n.tolist() == [0, 4, 2, 0, 1]
    n = check_collapse(np.array([[a, blank, blank]], dtype=np.int64), None, blank)
    assert n.tolist() == [1]


def test_collapse_random_rows():
    g = np.random.Generator(np.random.Philox(key=43))
    lens = [255, 256, 257, 1000, 999]
    ids = g.integers(0, 3, size=(5, 1000)).astype(np.int64)
    for b, n in enumerate(lens):
        ids[b, n:] = -1
    check_collapse(ids, lens, 0)
    check_collapse(ids[3:4], None, 2)


def pairs_for_distance():
    g = np.random.Generator(np.random.Philox(key=47))
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 700]
    pairs = []
    for i in range(40):
        n = sizes[i % 10] if i < 20 else int(g.choice(sizes))
        a = g.integers(0, 4, size=n)
        kind = i % 4
        if kind == 0:                                   # a noisy copy: substitutions, then a few deletions
            b = a.copy()
            flip = g.random(n) < 0.1
            b[flip] = g.integers(0, 4, size=int(flip.sum()))
            b = b[g.random(n) > 0.05]
        elif kind == 1:                                 # unrelated, of another length
            b = g.integers(0, 4, size=int(g.choice(sizes)))
        elif kind == 2:                                 # equal
            b = a.copy()
        else:                                           # one side empty or far shorter
            b = a[:int(g.choice([0, 1, 2]))]
        pairs.append((a, b) if i % 8 < 4 else (b, a))
    pairs.append((g.integers(0, 4, size=700), g.integers(0, 4, size=3)))         # n_hyp >> n_ref
    pairs.append((np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    return pairs


def run_distance(pairs, Lh=None, Lr=None):
    Lh = Lh or max(1, max(len(a) for a, _ in pairs))
    Lr = Lr or max(1, max(len(b) for _, b in pairs))
    hyp, ref = np.full((len(pairs), Lh), -5, dtype=np.int64), np.full((len(pairs), Lr), -6, dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        hyp[p, :len(a)], ref[p, :len(b)] = a, b
    d = asr.edit_distance(torch.from_numpy(hyp).cuda(), torch.from_numpy(ref).cuda(), [len(a) for a, _ in pairs], [len(b) for _, b in pairs])
    assert d.dtype == torch.int64 and d.is_cuda
    return d.cpu().tolist()


def test_edit_distance_pairs():
    pairs = pairs_for_distance()
    got = run_distance(pairs)
    want = [Y.edit_distance(a, b) for a, b in pairs]
    assert got == want
    assert any(w == 0 and len(a) for w, (a, _) in zip(want, pairs)) and any(len(a) == 0 and len(b) for a, b in pairs)
    # the padded widths do not matter
    assert run_distance(pairs[:6], 4096, 701) == want[:6]


def test_edit_distance_largest_pair_and_refusal():
    g = np.random.Generator(np.random.Philox(key=53))
    a = g.integers(0, 4, size=4096)
    b = a.copy()
    flip = g.random(4096) < 0.2
    b[flip] = g.integers(0, 4, size=int(flip.sum()))
    b = np.concatenate((b[300:], g.integers(0, 4, size=300)))
    assert run_distance([(a, b)]) == [Y.edit_distance(a, b)]
    z = torch.zeros(1, 4097, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match="EINVAL.*4096"):
        asr.edit_distance(z, z[:, :8], [4097], [8])
    with pytest.raises(RuntimeError, match="EINVAL.*4096"):
        asr.edit_distance(z[:, :8], z, [8], [4097])
    assert asr.edit_distance(z[:0, :8], z[:0, :8], [], []).shape == (0,)


def test_error_rates_hand_computed():
    r = asr.error_rates(["the cat sat", "hello"], ["the cat sat", "hallo world"])
    assert r["cer"] == 7 / 22 and r["wer"] == 2 / 5
    assert [p["char_distance"] for p in r["per_utterance"]] == [0, 7] and [p["word_distance"] for p in r["per_utterance"]] == [0, 2]
    r = asr.error_rates(["a", "b c"], ["", "b d"])
    assert np.isnan(r["per_utterance"][0]["cer"]) and np.isnan(r["per_utterance"][0]["wer"])
    assert r["cer"] == 2 / 3 and r["wer"] == 1.0
    hyps, refs = ["kitten", "", "sunday morning rain"], ["sitting", "abc", "saturday morning"]
    r = asr.error_rates(hyps, refs)
    assert [p["char_distance"] for p in r["per_utterance"]] == [3, 3, 8] and r["cer"] == 14 / 26 and r["wer"] == 4 / 4
    w = Y.error_rates(hyps, refs)
    assert r["cer"] == w["cer"] and r["wer"] == w["wer"] and r["per_utterance"] == w["per_utterance"]


def test_evaluate_from_files(golden, tmp_path, capsys):
    """The file path of evaluate.py, in this process: wavs at two rates, a checkpoint, config.json and vocab.json of the tiny golden
    model, a tiny speaker embedder.  The transcripts are those of each file transcribed alone, the rates the yardstick's, and a file is
    at similarity 1 from itself."""
    from scipy.io import wavfile
    from wavlm_torch import synthetic_wavlm_state_dict

    import evaluate
    from unitspeech_amd.mel import synthetic_waveform
    from unitspeech_amd.speaker_encoder import synthetic_ecapa_state_dict
    from voice_conversion import read_wav
    g = golden("ctc_a")
    cfg = json.loads(str(g["config"]))
    torch.save({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}, tmp_path / "ctc.pt")
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, architectures=["HubertForCTC"])))
    vocab = {"<pad>": 0, "|": 1, **{c: i + 2 for i, c in enumerate("abcdefghij")}}
    (tmp_path / "vocab.json").write_text(json.dumps(vocab))
    wcfg = dict(evaluate.TINY, num_buckets=320, max_bucket_distance=800, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
    ck = {k: torch.from_numpy(v) for k, v in synthetic_ecapa_state_dict(dict(feat_dim=40, channels=16, emb_dim=8, global_context_att=False,
                                                                             n_layers=3), 4).items()}
    ck.update({"feature_extract.model." + k: v for k, v in synthetic_wavlm_state_dict(wcfg, 9, masked_spec_embed=False).items()})
    torch.save({"model": ck}, tmp_path / "embedder.pt")
    specs = [(22050, 15000), (16000, 9000), (22050, 21000)]
    for i, (rate, n) in enumerate(specs):
        wavfile.write(tmp_path / f"{i}.wav", rate, (synthetic_waveform(n, 60 + i, rate) * 32767).astype(np.int16))
    texts = ["Abc, DEF ghij!", "xyz", "j  a"]
    lines = [f"{tmp_path / '0.wav'}|{texts[0]}|{tmp_path / '0.wav'}", f"{tmp_path / '1.wav'}|{texts[1]}", f"{tmp_path / '2.wav'}|{texts[2]}|{tmp_path / '1.wav'}"]
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    evaluate.main(["--filelist", str(tmp_path / "list.txt"), "--ctc_path", str(tmp_path / "ctc.pt"), "--vocab_path", str(tmp_path / "vocab.json"),
                   "--config_path", str(tmp_path / "config.json"), "--speaker_encoder_path", str(tmp_path / "embedder.pt"), "--batch", "2",
                   "--out", str(tmp_path / "out.json")])
    print(capsys.readouterr().out)
    res = json.loads((tmp_path / "out.json").read_text())
    assert res["files"] == 3 and res["batches"] == 2 and len(res["per_file"]) == 3
    # each file alone
    v = asr.CTCVocabulary(vocab)
    model = asr.load_ctc_checkpoint(str(tmp_path / "ctc.pt"), **{k: x for k, x in cfg.items() if k != "vocab_size"}).cuda()
    hyps, wavs16 = [], []
    for i in range(3):
        w = evaluate.to_16k(*read_wav(str(tmp_path / f"{i}.wav")), torch.device("cuda", 0), {})
        hyps += v.decode(*[t.cpu() for t in model.transcribe_ids(w[None])])
        wavs16.append(w)
    refs = ["abc def ghij", "", "j a"]
    assert [f["hypothesis"] for f in res["per_file"]] == hyps and [f["reference"] for f in res["per_file"]] == refs
    assert any(hyps), "the tiny model wrote nothing: the test would compare empty strings"
    want = Y.error_rates(hyps, refs)
    assert res["cer"] == want["cer"] and res["wer"] == want["wer"]
    for f, p in zip(res["per_file"], want["per_utterance"]):
        assert f["char_distance"] == p["char_distance"] and f["word_distance"] == p["word_distance"] and f["chars"] == p["chars"]
    secs = [f.get("secs") for f in res["per_file"]]
    from unitspeech_amd.speaker_encoder import load_speaker_embedder_checkpoint
    embedder = load_speaker_embedder_checkpoint(str(tmp_path / "embedder.pt"), torch.device("cuda", 0))
    alone = float((embedder.embed_wav(wavs16[2][None]) * embedder.embed_wav(wavs16[1][None])).sum())
    print("SECS", secs, "file 2 against file 1, each embedded alone:", alone)
    # unit vectors of 8 entries: a dot product's own rounding is below 1e-6, on whichever side it is taken
    assert abs(secs[0] - 1.0) < 1e-5 and secs[1] is None and abs(secs[2] - alone) < 1e-5 and abs(res["secs"] - (secs[0] + secs[2]) / 2) < 1e-6


def test_evaluate_synthetic_prints_the_cer_of_its_edits():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--batch", "4"], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert len(lines) == 7 and all("CER" in ln and "WER" in ln for ln in lines[:6])
    res = json.loads(lines[-1])
    assert res["files"] == 6 and res["batches"] == 2
    assert res["cer"] == res["expected_cer"] and 0 < res["cer"] < 1
