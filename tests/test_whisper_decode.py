"""Decoding under the timestamp rules without a GPU: the fp64 numpy statement of one selection step (tools/whisper_decode_numpy.py) against
transformers' three processor classes, the torch restatement's `decode` against the goldens (tests/golden/whisper_decode_{a,b,long,wide}.npz),
`WhisperVocabulary.segments`, and the refusals that need no device."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_decode_numpy as rules  # noqa: E402
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd.whisper import WhisperForConditionalGeneration, WhisperVocabulary  # noqa: E402

V = 203
LAYOUTS = (dict(eos=178, no_timestamps=190, max_initial_timestamp_index=2, suppress=[5, 179, 189], begin_suppress=[7, 178, 192]),
           dict(eos=60, no_timestamps=150, max_initial_timestamp_index=-1, suppress=[3, 70, 160], begin_suppress=[151]))
KINDS = ("first", "one_ts", "ts_text", "text_ts", "ts_ts", "exhausted", "text_only", "all_text_masked", "text_ts_at_end")
_CACHE = {}


def history(g, lay, kind):
    eos, tb = lay["eos"], lay["no_timestamps"] + 1
    text = lambda: int(g.integers(0, eos))
    ts = lambda lo=tb: int(g.integers(lo, V))
    a = ts()
    return {"first": [], "one_ts": [a], "ts_text": [a, text()], "text_ts": [a, text(), ts(a)], "ts_ts": [a, text(), ts(a), ts(a)],
            "exhausted": [tb, text(), V - 1, V - 1, text()], "text_only": [text(), text()], "all_text_masked": [tb, text()],
            "text_ts_at_end": [tb, text(), V - 1]}[kind]


def cases():
    """a few hundred seeded (logits, tokens sampled so far, layout, masks), every branch of the rules in turn, each with |d| >= 1e-3"""
    if "cases" not in _CACHE:
        g = np.random.Generator(np.random.Philox(key=4242))
        out = []
        for n in range(360):
            lay = LAYOUTS[n % 2]
            kind = KINDS[(n // 2) % len(KINDS)]
            tb = lay["no_timestamps"] + 1
            x = g.standard_normal(V) * (0.3 if n % 3 else 3.0)
            sup, beg = rules.masks(lay, V)
            if kind == "all_text_masked":
                sup = sup.copy()
                sup[:tb] = True
            hist = history(g, lay, kind)
            r = rules.select(x, hist, lay, sup, beg)
            if r["free"] and abs(r["d"]) < 1e-3:                 # move the timestamp side off the tie: never skipped
                x[tb:] += 0.01
            out.append((x, hist, lay, sup, beg, kind))
        _CACHE["cases"] = out
    return _CACHE["cases"]


def transformers_step(x, hist, lay, sup, beg):
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    P, cap = 3, lay["max_initial_timestamp_index"]
    gen = SimpleNamespace(no_timestamps_token_id=lay["no_timestamps"], eos_token_id=lay["eos"], bos_token_id=lay["eos"],
                          max_initial_timestamp_index=cap if cap >= 0 else None, _detect_timestamp_from_logprob=True)
    ids = torch.tensor([[1, 2, 3] + list(hist)])
    scores = torch.from_numpy(x)[None]
    for p in (SuppressTokensLogitsProcessor(np.flatnonzero(sup).tolist()), SuppressTokensAtBeginLogitsProcessor(np.flatnonzero(beg).tolist(), P),
              WhisperTimeStampLogitsProcessor(gen, begin_index=P)):
        scores = p(ids, scores)
    tok = int(scores[0].argmax())
    return tok, float(torch.log_softmax(scores[0], -1)[tok])


def test_numpy_step_against_transformers_processors():
    seen = set()
    for x, hist, lay, sup, beg, kind in cases():
        r = rules.select(x, hist, lay, sup, beg)
        assert not r["free"] or abs(r["d"]) >= 1e-3, (kind, r)
        tok, lp = transformers_step(x, hist, lay, sup, beg)
        assert r["token"] == tok, (kind, hist, r, tok)
        assert abs(r["logprob"] - lp) <= 1e-12, (kind, r, lp)
        seen.add((kind, r["free"], r["decided"]))
    kinds = {k for k, _, _ in seen}
    assert kinds == set(KINDS)
    assert {(True, True), (True, False)} <= {(f, d) for _, f, d in seen}                 # both outcomes of a free decision
    assert ("all_text_masked", False, True) in seen and ("exhausted", False, False) in seen and ("ts_ts", False, False) in seen


def test_numpy_step_history_and_empty_vocabulary():
    lay = LAYOUTS[0]
    assert rules.history([], lay) == (0, -1, -1, -1, 0)
    assert rules.history([191, 4, 195], lay, done=True) == (3, 195, 4, 195, 1)
    sup = np.ones(V, dtype=bool)
    r = rules.select(np.zeros(V), [], lay, sup)
    assert r["token"] == lay["eos"] and r["logprob"] == 0.0 and not r["free"]
    # an exact tie of the decision keeps text; the lower index wins the argmax
    x = np.full(V, -5.0)
    x[[20, 150]] = 2.5
    x[V - 1] = 2.5
    r = rules.select(x, [191, 3, V - 2, V - 2, 5], lay)
    assert r["d"] == 0.0 and not r["decided"] and r["token"] == 20


def golden(name):
    if name not in _CACHE:
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
            x, prompt = torch.from_numpy(g["features"]), torch.from_numpy(g["prompt"])
            c, sd = json.loads(str(g["config"])), golden_state_dict(g)
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) as g:
            d = {k: g[k] for k in g.files}
        _CACHE[name] = (x, prompt, c, sd, d, json.loads(str(d["layout"])))
    return _CACHE[name]


NAMES = ["a", "b", "long", "wide"]


@pytest.mark.parametrize("name", NAMES)
def test_goldens_keep_their_conditions(name):
    x, prompt, c, sd, d, lay = golden(name)
    free = np.isfinite(d["d"])
    assert float(np.abs(d["d"][free]).min()) >= 1e-2 and float(d["min_gap"]) >= 1e-3
    assert int((free & (d["decided"] == 1)).sum()) >= 5 and int((free & (d["decided"] == 0)).sum()) >= 5
    stops = [int(v) for v in d["lengths"] if v < int(d["max_new"])]
    if name == "long":                                # two items: they end differently and one runs past step 70
        assert int(d["max_new"]) == 132 and len(set(d["lengths"].tolist())) == 2 and int(d["lengths"].max()) > 70
    else:
        assert len(set(stops)) >= 2 and len(stops) < len(d["lengths"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) < 16384


@pytest.mark.parametrize("name", NAMES)
def test_torch_decode_reproduces_the_golden(name):
    x, prompt, c, sd, d, lay = golden(name)
    trace = []
    r = WhisperTorch(sd, c, torch.float64).decode(x, prompt, int(d["max_new"]), lay, int(d["sot_index"]), trace=trace)
    assert np.array_equal(r["tokens"], d["tokens"]) and np.array_equal(r["lengths"], d["lengths"])
    assert float(np.abs(r["sum_logprob"] - d["sum_logprob"]).max()) <= 1e-9
    assert float(np.abs(r["no_speech_prob"] - d["no_speech_prob"]).max()) <= 1e-9
    assert float(np.abs(r["logprobs"] - d["logprobs"]).max()) <= 1e-9
    # the loop over the recorded logits (numpy alone) gives the same
    for b in range(len(x)):
        n = rules.decode(np.stack([t[b].numpy() for t in trace]), lay)
        k = int(d["lengths"][b])
        assert n["length"] == min(k, len(trace)) and np.array_equal(n["tokens"][:k], d["tokens"][b, :k])
        assert abs(n["sum_logprob"] - d["sum_logprob"][b]) <= 1e-9
    # the fp32 restatement keeps the tokens
    r32 = WhisperTorch(sd, c, torch.float32).decode(x, prompt, int(d["max_new"]), lay, int(d["sot_index"]))
    assert np.array_equal(r32["tokens"], d["tokens"]) and np.array_equal(r32["lengths"], d["lengths"])


def vocabulary():
    vocab = {"a": 0, "b": 1, "Ġ": 2}
    added = {"<|endoftext|>": 3, "<|startoftranscript|>": 4, "<|nocaptions|>": 5, "<|notimestamps|>": 6,
             **{f"<|{0.02 * i:.2f}|>": 7 + i for i in range(6)}}
    return WhisperVocabulary(vocab, added)


def test_segments_and_vocabulary_ids():
    v = vocabulary()
    assert v.timestamp_begin == 7 and v.nospeech_id == 5
    assert WhisperVocabulary({"a": 0}, {"<|nospeech|>": 1, "<|nocaptions|>": 2, "<|notimestamps|>": 3}).nospeech_id == 1
    with pytest.raises(KeyError, match="nospeech"):
        WhisperVocabulary({"a": 0}, {"<|notimestamps|>": 1}).nospeech_id
    assert v.segments([7, 0, 1, 9, 9, 1, 2, 0, 12]) == [(0.0, 0.04, "ab"), (0.04, 0.1, "b a")]              # pairs
    assert v.segments([7, 0, 9, 9, 1]) == [(0.0, 0.04, "a"), (0.04, None, "b")]                              # an unclosed tail
    assert v.segments([8, 10, 0, 11]) == [(0.06, 0.08, "a")]                                                 # consecutive timestamps: the later opens
    assert v.segments(torch.tensor([7, 8])) == [] and v.segments([]) == []
    assert v.segments([0, 7, 1, 8]) == [(None, 0.0, "a"), (None, 0.02, "b")]
    assert v.segments([7, 0, 3, 5, 8]) == [(0.0, 0.02, "a")]                                                  # other special tokens are dropped
    assert v.decode([7, 0, 1, 9]) == "ab"                                                                    # decode drops the timestamps


def test_decode_refusals_without_a_device():
    m = WhisperForConditionalGeneration(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=1, decoder_layers=1,
                                        encoder_ffn_dim=64, decoder_ffn_dim=64, num_mel_bins=8, max_source_positions=10, max_target_positions=12,
                                        vocab_size=40).eval()
    x = torch.zeros(1, 8, 20)
    with pytest.raises(ValueError, match="no eos_token_id"):
        m.decode(x, [1, 2, 3], no_timestamps_id=30)
    with pytest.raises(ValueError, match="max_initial_timestamp"):
        m.decode(x, [1, 2, 3], no_timestamps_id=30, eos_token_id=5, max_initial_timestamp=-1.0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        m.decode(x, [1, 2, 3], no_timestamps_id=30, eos_token_id=5, max_new_tokens=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decode(x, [1, 2, 3], no_timestamps_id=30, eos_token_id=5)
    with pytest.raises(TypeError):
        m.decode(x, [1, 2, 3], 30)                                       # no_timestamps_id is keyword-only
    m.prompt_ids = [1, 2, 3, 30]
    with pytest.raises(ValueError, match="needs no_timestamps_id"):
        m.transcribe_ids(torch.zeros(1, 1600), timestamps=True)


def test_evaluate_flag_argument_checks():
    import evaluate
    with pytest.raises(SystemExit, match="--whisper_timestamps belongs to --recogniser whisper"):
        evaluate.main(["--synthetic", "2", "--whisper_timestamps"])
    with pytest.raises(SystemExit, match="--whisper_timestamps belongs to --recogniser whisper"):
        evaluate.main(["--synthetic", "2", "--recogniser", "ctc", "--whisper_timestamps"])
