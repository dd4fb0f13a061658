"""Host side of the recogniser (unitspeech_amd/asr.py, tools/ctc_numpy.py, evaluate.py): the numpy yardsticks against a naive DP and known
cases, the text handling, the classes' keys against the goldens written from transformers, the refusals, and the C ABI's new symbols.
No device work is launched here."""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ctc_numpy import ctc_collapse, edit_distance, error_rates  # noqa: E402

import evaluate  # noqa: E402
from unitspeech_amd import _build, _lib, asr  # noqa: E402

SYMBOLS = ["us_ctc_packed_bytes", "us_ctc_pack_head", "us_ctc_logits", "us_ctc_collapse", "us_edit_distance"]


def naive_distance(a, b):
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                d[i][j] = i + j
            else:
                d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def test_edit_distance_yardstick_against_naive_dp():
    g = np.random.Generator(np.random.Philox(key=41))
    for _ in range(200):
        a = g.integers(0, 3, size=int(g.integers(0, 12))).tolist()
        b = g.integers(0, 3, size=int(g.integers(0, 12))).tolist()
        assert edit_distance(a, b) == naive_distance(a, b), (a, b)


def test_edit_distance_yardstick_known_cases():
    s = lambda t: [ord(c) for c in t]  # noqa: E731
    assert edit_distance(s("kitten"), s("sitting")) == 3
    assert edit_distance(s("flaw"), s("lawn")) == 2
    assert edit_distance([], []) == 0 and edit_distance([], s("abc")) == 3 and edit_distance(s("abcd"), []) == 4
    assert edit_distance(s("abc"), s("abc")) == 0
    assert edit_distance(s("a" * 50), s("b" * 20)) == 50


def test_collapse_yardstick_cases():
    a, blank = 5, 0
    for ids, want, frames in [([a, a, blank, a], [a, a], [0, 3]), ([a, blank, blank], [a], [0]), ([blank] * 4, [], []), ([], [], []),
                              ([3, 3, 4, 4, 0, 0, 4, 3], [3, 4, 4, 3], [0, 2, 6, 7]), ([7], [7], [0]), ([0], [], []),
                              ([1, 2, 3], [1, 2, 3], [0, 1, 2])]:
        tokens, first = ctc_collapse(ids, blank)
        assert tokens.tolist() == want and first.tolist() == frames, ids
    tokens, _ = ctc_collapse([2, 2, 1, 2], blank=2)          # another blank
    assert tokens.tolist() == [1]


def test_error_rates_yardstick_hand_computed():
    r = error_rates(["the cat sat", "hello"], ["the cat sat", "hallo world"])
    # chars: 0 / 11 and ("hello" -> "hallo world": one substitution, six insertions) 7 / 11; words: 0 / 3 and 2 / 2
    assert r["per_utterance"][0]["cer"] == 0.0 and r["per_utterance"][1]["char_distance"] == 7
    assert r["cer"] == 7 / 22 and r["wer"] == 2 / 5
    r = error_rates(["a", "b c"], ["", "b d"])
    assert math.isnan(r["per_utterance"][0]["cer"]) and math.isnan(r["per_utterance"][0]["wer"])
    assert r["cer"] == (1 + 1) / 3 and r["wer"] == (1 + 1) / 2
    with pytest.raises(ValueError):
        error_rates(["a"], [""])


VOCAB = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, **{c: i + 5 for i, c in enumerate("abcdefghijklmnopqrstuvwxyzăâîșț")}}


def test_vocabulary_round_trip():
    v = asr.CTCVocabulary(VOCAB)
    assert len(v) == len(VOCAB) and v.blank_id == 0
    text = "și țara mea"
    ids = v.encode(text)
    assert ids[2] == VOCAB["|"] and len(ids) == len(text)
    assert v.decode([ids]) == [text]
    assert v.decode(torch.tensor([ids + [0, 0]]), torch.tensor([len(ids)])) == [text]
    # special tokens are dropped, delimiters collapse
    assert v.decode([[VOCAB["<s>"], VOCAB["a"], VOCAB["|"], VOCAB["|"], VOCAB["b"], VOCAB["|"], VOCAB["</s>"]]]) == ["a b"]
    with pytest.raises(ValueError):
        v.encode("A")
    with pytest.raises(ValueError):
        asr.CTCVocabulary({"a": 0, "b": 1})                     # no blank
    with pytest.raises(ValueError):
        asr.CTCVocabulary({"<pad>": 0, "a": 0})


def test_vocabulary_from_path(tmp_path):
    p = tmp_path / "vocab.json"
    p.write_text(json.dumps(VOCAB), encoding="utf-8")
    assert asr.CTCVocabulary(str(p)).token_to_id == VOCAB


def test_normalize_text():
    v = asr.CTCVocabulary(VOCAB)
    assert asr.normalize_text("  Şi  ţara\tMEA, 2024! ", v) == "și țara mea"
    assert asr.normalize_text("Ţ Ş", v) == "ț ș"
    upper = asr.CTCVocabulary({"<pad>": 0, "|": 1, "A": 2, "B": 3, "'": 4})
    assert asr.normalize_text("a'b c?", upper) == "A'B"
    assert asr.normalize_text("", v) == ""


def test_apply_edits_distance_is_exact():
    s = lambda t: [ord(c) for c in t]  # noqa: E731
    for text in ["", "a", "abc ab", "abcd efg hij", "ab cdefg"]:
        for cut in (False, True):
            ref = evaluate.apply_edits(text, 2, cut)
            assert edit_distance(s(text), s(ref)) == 2 and not ref.endswith(" ")


def test_parse_filelist():
    assert evaluate.parse_filelist("a.wav|hello there\n\nb.wav|x|ref.wav\n") == [("a.wav", "hello there", None), ("b.wav", "x", "ref.wav")]
    with pytest.raises(ValueError):
        evaluate.parse_filelist("a.wav")


@pytest.mark.parametrize("name,cls", [("a", asr.HubertForCTC), ("b", asr.Wav2Vec2ForCTC)])
def test_keys_and_shapes_equal_transformers(golden, name, cls, tmp_path):
    g = golden("ctc_" + name)
    assert str(g["class"]) == cls.__name__
    model = cls(**json.loads(str(g["config"])))
    sd = model.state_dict()
    assert list(sd.keys()) == json.loads(str(g["keys"]))
    for k, v in sd.items():
        assert tuple(v.shape) == g["w:" + k].shape, k
    weights = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w:")}
    model.load_state_dict(weights)
    assert torch.equal(model.lm_head.weight, weights["lm_head.weight"])
    with pytest.raises(RuntimeError):
        model.load_state_dict(dict(weights, extra=torch.zeros(1)))
    # the loader picks the class from the prefix and the vocabulary size from the head
    path = tmp_path / "ctc.pt"
    torch.save(weights, path)
    cfg = {k: v for k, v in json.loads(str(g["config"])).items() if k != "vocab_size"}
    loaded = asr.load_ctc_checkpoint(str(path), **cfg)
    assert type(loaded) is cls and loaded.vocab_size == weights["lm_head.weight"].shape[0] and not loaded.training
    torch.save({"lm_head.weight": torch.zeros(4, 8)}, path)
    with pytest.raises(ValueError):
        asr.load_ctc_checkpoint(str(path))


def test_refusals():
    tiny = dict(evaluate.TINY)
    for bad in (dict(add_adapter=True), dict(feat_extract_norm="layer"), dict(do_stable_layer_norm=True), dict(conv_bias=True),
                dict(vocab_size=1), dict(vocab_size=2049), dict(pad_token_id=12, vocab_size=12), dict(hidden_size=42, num_attention_heads=2)):
        with pytest.raises(ValueError):
            asr.HubertForCTC(**dict(tiny, **bad))
        with pytest.raises(ValueError):
            asr.Wav2Vec2ForCTC(**dict(tiny, **bad))
    for h, v in ((40, 1), (40, 2049), (42, 12), (1028, 12), (0, 12)):
        with pytest.raises(ValueError):
            asr.CTCHead(h, v)
    head = asr.CTCHead(8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(1, 3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.edit_distance(torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.int64), torch.tensor([3]), torch.tensor([3]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.ctc_collapse(torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        asr.error_rates(["a"], ["a", "b"])
    with pytest.raises(ValueError):
        asr.error_rates(["a"], [" "])


def test_symbols_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "unitspeech_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(us_[a-z_0-9]+)\s*\(", txt))
    lib = C.CDLL(_build.build_library())
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert "ctc.hip" in _build.SOURCES
    assert {"CTCHead", "HubertForCTC", "Wav2Vec2ForCTC", "load_ctc_checkpoint", "CTCVocabulary", "normalize_text", "edit_distance",
            "error_rates"} <= set(asr.__all__)


def test_size_functions_refuse_without_a_device():
    lib = _lib.load()
    assert lib.us_ctc_packed_bytes(12, 40) == (48 * 64 + 64) * 4
    assert lib.us_ctc_packed_bytes(2048, 1024) == (1024 * 2048 + 2048) * 4
    for v, h in ((1, 40), (2049, 40), (12, 42), (12, 1028), (12, 0)):
        assert lib.us_ctc_packed_bytes(v, h) == 0
    # the size checks come before any launch
    assert lib.us_ctc_logits(None, None, None, 1, 1, 1, 4, None, None, None, None) == -1
    assert b"V must be" in lib.us_last_error(None)
    assert lib.us_edit_distance(None, None, 4097, None, None, 1, 1, None, None) == -1
    assert b"4096" in lib.us_last_error(None)
    assert lib.us_edit_distance(None, None, 1, None, None, 4097, 1, None, None) == -1
    assert lib.us_edit_distance(None, None, 8, None, None, 8, 0, None, None) == 0          # P = 0: nothing to do
