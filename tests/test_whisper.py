"""The Whisper recogniser's host side (no GPU): the fp64 restatement (tools/whisper_torch.py) against the goldens (a, b, long, wide) written from
transformers.WhisperForConditionalGeneration, the feature extraction against transformers.WhisperFeatureExtractor, the vocabulary, and what
the library and the module refuse before any device is touched."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.whisper import (WhisperForConditionalGeneration, WhisperVocabulary, log_mel_spectrogram,  # noqa: E402
                                    synthetic_whisper_state_dict)

TINY = dict(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
            decoder_ffn_dim=128, num_mel_bins=16, max_source_positions=50, max_target_positions=24, vocab_size=96)


def golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
        d = {k: g[k] for k in g.files if not k.startswith(("w:", "q:"))}
        return d, json.loads(str(g["config"])), golden_state_dict(g)


def stored_enc(name, g):
    """(`enc` as the goldens hold it, the rows it holds or None for all): whisper_long keeps it in a file of its own, at `enc_rows`"""
    if "enc" in g:
        return g["enc"], None
    path = os.path.join(ROOT, "tests", "golden", f"whisper_{name}_enc.npz")
    assert os.path.getsize(path) < (1 << 20)
    with np.load(path) as e:
        return e["enc"], e["enc_rows"]


@pytest.mark.parametrize("name", ["a", "b", "long", "wide"])
def test_restatement_fp64_reproduces_golden(name):
    g, c, sd = golden(name)
    m = WhisperTorch(sd, c, torch.float64)
    x = torch.from_numpy(g["features"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) < (1 << 20)
    want, rows = stored_enc(name, g)
    enc = m.encode(x)[:len(want)]                     # whisper_wide holds `enc` and `logits` of its first two items
    assert len(want) == len(x) or name == "wide"
    if rows is not None:
        S = c["max_source_positions"]
        assert set(range(64)) | set(range(992, S)) <= set(rows.tolist()) and int(np.diff(rows).max()) <= 5
        enc = enc[:, torch.from_numpy(rows)]
    assert enc.shape == want.shape and float((enc - torch.from_numpy(want)).abs().max()) <= 1e-10 * float(np.abs(want).max())
    k = len(g["logits"])
    assert g["logits"].shape == (k, c["max_target_positions"], c["vocab_size"]) and (k == len(x) or name == "wide")
    lg = m.logits(x[:k], torch.from_numpy(g["ids"][:k]))
    assert float((lg - torch.from_numpy(g["logits"])).abs().max()) <= 1e-10 * float(np.abs(g["logits"]).max())
    tokens, n = m.generate(x, torch.from_numpy(g["prompt"]), g["tokens"].shape[1], int(g["eos"]))
    assert np.array_equal(tokens.numpy(), g["tokens"]) and np.array_equal(n.numpy(), g["lengths"])
    # the three conditions the golden was written under
    stops = sorted(int(v) for v in g["lengths"] if v < g["tokens"].shape[1])
    assert float(g["margin"]) >= 1e-3
    if name == "long":                                # two items: one never stops, the other fills the cache beyond 64 positions first
        assert len(g["lengths"]) == 2 and len(stops) == 1 and stops[0] >= 70 and g["tokens"].shape[1] == 132
    else:
        assert len(stops) == 2 and stops[1] - stops[0] >= 5
    assert max(len(set(r.tolist())) for r in g["top_idx"][:, :, 0]) >= 8
    assert len({tuple(r.tolist()) for r in g["top_idx"][:, :, 0]}) == len(x)
    big = float(np.abs(g["top_val"]).max())
    assert float((g["top_val"][:, 0, 1] - g["top_val"][:, 0, 2]).max()) >= 1e-3 * big
    # and one item alone is the item in the batch (the restatement's cache is per item)
    t1, n1 = m.generate(x[1:2], torch.from_numpy(g["prompt"][1:2]), g["tokens"].shape[1], int(g["eos"]))
    assert np.array_equal(t1.numpy(), g["tokens"][1:2]) and int(n1) == int(g["lengths"][1])


def test_restatement_fp32_keeps_the_tokens():
    g, c, sd = golden("b")
    tokens, n = WhisperTorch(sd, c, torch.float32).generate(torch.from_numpy(g["features"]), torch.from_numpy(g["prompt"]), g["tokens"].shape[1],
                                                            int(g["eos"]))
    assert np.array_equal(tokens.numpy(), g["tokens"]) and np.array_equal(n.numpy(), g["lengths"])


def test_restatement_suppression():
    """suppressing the token greedy chose first gives the fp64 runner-up there, by either mask; begin_suppress holds for that position only"""
    g, c, sd = golden("a")
    m = WhisperTorch(sd, c, torch.float64)
    for b in range(3):
        x, prompt = torch.from_numpy(g["features"][b:b + 1]), torch.from_numpy(g["prompt"][b:b + 1])
        mask = torch.zeros(c["vocab_size"], dtype=torch.bool)
        mask[int(g["top_idx"][b, 0, 0])] = True
        for kw in (dict(suppress=mask), dict(begin_suppress=mask)):
            tokens, _ = m.generate(x, prompt, 2, c["vocab_size"] - 1, **kw)
            assert int(tokens[0, 0]) == int(g["top_idx"][b, 0, 1])


def waveform(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    return (0.3 * torch.sin(2 * np.pi * 220.0 * t) + 0.1 * torch.sin(2 * np.pi * 2310.0 * t + 0.5) + 0.05 * torch.randn(n, generator=gen, dtype=torch.float64)).float()


def test_log_mel_matches_the_feature_extractor():
    """The bar comes from the extractor's own arithmetic: it keeps the spectrum as complex64, so a component carries an absolute error of
    about 2^-24 of the frame's largest component.  The per-item clamp at 8 decades of power below the maximum bounds how far below that a
    band can lie: an amplitude ratio of 1e-4, so a relative amplitude error of at most 2^-24 * 1e4, twice that in power, / ln 10 in log10,
    / 4 by the final scaling: 1.3e-4.  This side computes in fp64 and rounds once (2^-23 at values up to 1.5), far below that."""
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor()
    waves = [waveform(16000, 1), waveform(31 * 16000, 2)]
    want = fe([w.numpy() for w in waves], sampling_rate=16000, return_tensors="np")["input_features"]
    x = torch.zeros(2, 31 * 16000)
    x[0, :16000], x[1] = waves[0], waves[1]
    x[0, 16000:] = float("nan")                       # never read
    got = log_mel_spectrogram(torch.nan_to_num(x, nan=7.0), [16000, 31 * 16000])
    assert tuple(got.shape) == (2, 80, 3000) == want.shape and got.dtype == torch.float32
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print(f"log-mel vs WhisperFeatureExtractor: max |diff| {err:.3e}")
    assert err <= 2.0 ** -24 * 1e4 * 2 / np.log(10) / 4
    alone = log_mel_spectrogram(waves[0])
    assert torch.equal(alone[0], got[0])


def test_vocabulary_decodes_multibyte_characters():
    table = {b: c for b, c in __import__("unitspeech_amd.whisper", fromlist=["_bytes_to_unicode"])._bytes_to_unicode().items()}
    enc = lambda s: "".join(table[b] for b in s.encode("utf-8"))
    raw = "ț".encode("utf-8")
    vocab = {enc(" bun"): 0, enc("ă"): 1, enc(" ziua"): 2, table[raw[0]]: 3, table[raw[1]]: 4, enc(" ș"): 5, enc("i"): 6, "<|endoftext|>": 7}
    added = {"<|startoftranscript|>": 8, "<|ro|>": 9, "<|en|>": 10, "<|transcribe|>": 11, "<|notimestamps|>": 12}
    v = WhisperVocabulary(vocab, added)
    assert v.decode([8, 9, 11, 12, 0, 1, 2, 7]) == " bună ziua"
    assert v.decode([3, 4, 5, 6, 99]) == "ț și"                  # a character split over two tokens; an unknown id is dropped
    assert v.decode(torch.tensor([[0, 1, 7, 7], [5, 6, 3, 4]]), torch.tensor([2, 4])) == [" bună", " șiț"]
    assert (v.start_id, v.language_id("ro"), v.transcribe_id, v.notimestamps_id, v.end_id) == (8, 9, 11, 12, 7)
    assert v.language_ids() == [9, 10] and all(ch in v.characters for ch in "ățșb 7") and "B" not in v.characters and "," not in v.characters
    with pytest.raises(KeyError):
        v.language_id("xx")


def create(**over):
    m = WhisperForConditionalGeneration(**TINY)
    lib = _lib.load()
    s = _lib.us_whisper_config()
    c = m.config
    s.n_mels, s.d_model, s.vocab_size = c["num_mel_bins"], c["d_model"], c["vocab_size"]
    s.encoder_layers, s.encoder_heads, s.encoder_ffn = c["encoder_layers"], c["encoder_attention_heads"], c["encoder_ffn_dim"]
    s.decoder_layers, s.decoder_heads, s.decoder_ffn = c["decoder_layers"], c["decoder_attention_heads"], c["decoder_ffn_dim"]
    s.max_source_positions, s.max_target_positions = c["max_source_positions"], c["max_target_positions"]
    for k, v in over.items():
        setattr(s, k, v)
    h = C.c_void_p()
    return lib, h, lib.us_whisper_create(C.byref(h), C.byref(s))


def test_create_and_key_list():
    lib, h, rc = create()
    assert rc == _lib.US_OK and h
    keys = [lib.us_whisper_weight_key(h, i).decode() for i in range(lib.us_whisper_num_weights(h))]
    g, c, sd = golden("a")
    assert c == TINY and sorted(keys) == sorted(sd) == sorted(WhisperForConditionalGeneration(**TINY).state_dict())
    assert "proj_out.weight" not in keys
    assert lib.us_whisper_workspace_bytes(h, 0) == 0 and 0 < lib.us_whisper_workspace_bytes(h, 1) < lib.us_whisper_workspace_bytes(h, 17)
    assert lib.us_whisper_destroy(h) == _lib.US_OK


@pytest.mark.parametrize("over, text", [
    (dict(decoder_heads=3), b"divisible"),
    (dict(d_model=256, encoder_heads=2, decoder_heads=2), b"head dimension"),        # d_head 128
    (dict(d_model=60, encoder_heads=10, decoder_heads=10), b"head dimension"),       # d_head 6
    (dict(max_target_positions=4096), b"max_target_positions"),
    (dict(decoder_ffn=130), b"multiple of 4"),
])
def test_create_refuses(over, text):
    lib, h, rc = create(**over)
    assert rc == -1 and not h and text in lib.us_last_error(None)


def test_module_refusals():
    with pytest.raises(ValueError, match="divisible"):
        WhisperForConditionalGeneration(**dict(TINY, decoder_attention_heads=3))
    with pytest.raises(ValueError, match="head dimension"):
        WhisperForConditionalGeneration(**dict(TINY, d_model=256))
    m = WhisperForConditionalGeneration(**TINY).eval()
    sd = synthetic_whisper_state_dict(TINY, 0)
    m.load_state_dict(dict(sd, **{"proj_out.weight": sd["model.decoder.embed_tokens.weight"].clone()}))
    with pytest.raises(ValueError, match="proj_out"):
        m.load_state_dict(dict(sd, **{"proj_out.weight": sd["model.decoder.embed_tokens.weight"] + 1}))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 16, 100))
    with pytest.raises(ValueError, match="expected features"):
        m.encode(torch.zeros(1, 17, 100))
    with pytest.raises(ValueError, match="30 s"):
        m.transcribe_ids(torch.zeros(1, 480001))


def test_load_whisper_checkpoint(tmp_path):
    from unitspeech_amd.whisper import load_whisper_checkpoint
    sd = synthetic_whisper_state_dict(TINY, 3)
    full = dict(sd, **{"proj_out.weight": sd["model.decoder.embed_tokens.weight"]})
    d = tmp_path / "ckpt"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(TINY, model_type="whisper", eos_token_id=5, suppress_tokens=[1, 2])))
    (d / "generation_config.json").write_text(json.dumps(dict(begin_suppress_tokens=[7], suppress_tokens=[1, 2, 3])))
    torch.save(full, d / "pytorch_model.bin")
    m = load_whisper_checkpoint(str(d))
    assert m.config == TINY and not m.training and m.eos_token_id == 5 and m.suppress_tokens == [1, 2, 3] and m.begin_suppress_tokens == [7]
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and set(m.state_dict()) == set(sd)
    torch.save({"config": TINY, "state_dict": full}, tmp_path / "one.pt")
    m2 = load_whisper_checkpoint(str(tmp_path / "one.pt"))
    assert m2.config == TINY and torch.equal(m2.state_dict()["model.decoder.layers.1.fc2.bias"], sd["model.decoder.layers.1.fc2.bias"])
    (d / "pytorch_model.bin").unlink()
    with pytest.raises(FileNotFoundError):
        load_whisper_checkpoint(str(d))
