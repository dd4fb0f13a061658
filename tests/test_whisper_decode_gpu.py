"""Greedy decoding under the timestamp rules on the GPU (csrc/whisper.hip: us_whisper_decode, us_whisper_select) against the goldens written
from transformers in fp64 (tests/golden/whisper_decode_{a,b}.npz over the models of whisper_{a,b}.npz) and against the fp64 numpy statement
of one selection step (tools/whisper_decode_numpy.py).

Tokens, lengths and decisions are compared exactly: the goldens and the seeded cases keep every free decision |d| >= 1e-2 / 1e-3 away from a
tie and the top-1 / top-2 gap 1e-3 of the largest logit.  sum_logprob and no_speech_prob follow the project's rule: the library's distance
from fp64 is at most max(10 x the fp32 restatement's distance, 1e-5 x max |golden|); both distances are printed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_decode_numpy as rules  # noqa: E402
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.whisper import WhisperForConditionalGeneration, select_tokens  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}
REAL = dict(eos=50257, no_timestamps=50363, max_initial_timestamp_index=50)
V_REAL = 51865


def setup(name):
    """the two goldens of a model, the model on the device and the fp32 restatement's decoding: made once, never changed"""
    if name not in _CACHE:
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
            base = {k: g[k] for k in ("features", "prompt", "tokens", "lengths", "eos")}
            c, sd = json.loads(str(g["config"])), golden_state_dict(g)
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) as g:
            d = {k: g[k] for k in g.files}
        lay = json.loads(str(d["layout"]))
        m = WhisperForConditionalGeneration(**c, eos_token_id=lay["eos"], suppress_tokens=lay["suppress"], begin_suppress_tokens=lay["begin_suppress"])
        m.load_state_dict(sd)
        r32 = WhisperTorch(sd, c, torch.float32).decode(torch.from_numpy(base["features"]), torch.from_numpy(base["prompt"]), int(d["max_new"]),
                                                        lay, int(d["sot_index"]))
        _CACHE[name] = (base, d, lay, c, m.cuda().eval(), r32)
    return _CACHE[name]


def decode(m, lay, d, x, prompt, **kw):
    cap = lay["max_initial_timestamp_index"]
    return m.decode(x, prompt, no_timestamps_id=lay["no_timestamps"], max_initial_timestamp=None if cap < 0 else 0.02 * cap,
                    no_speech_id=lay["no_speech"], max_new_tokens=int(d["max_new"]), sot_index=int(d["sot_index"]), **kw)


def check(tag, got, r64, r32):
    e, s, mag = float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
    print(f"{tag}: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.3f}")
    assert np.isfinite(e) and e <= max(10 * s, 1e-5 * mag), (tag, e, s, mag)


@pytest.mark.parametrize("name", ["a", "b"])
def test_decode_matches_the_golden(name):
    base, d, lay, c, m, r32 = setup(name)
    assert np.array_equal(r32["tokens"], d["tokens"])
    r = decode(m, lay, d, torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"]))
    assert r.tokens.dtype == r.lengths.dtype == torch.int64
    assert np.array_equal(r.lengths.cpu().numpy(), d["lengths"]), (r.lengths, d["lengths"])
    assert np.array_equal(r.tokens.cpu().numpy(), d["tokens"])
    check(f"whisper_decode_{name} sum_logprob", r.sum_logprob.double().cpu().numpy(), d["sum_logprob"], r32["sum_logprob"])
    check(f"whisper_decode_{name} no_speech_prob", r.no_speech_prob.double().cpu().numpy(), d["no_speech_prob"], r32["no_speech_prob"])
    want = d["sum_logprob"] / (d["lengths"] + 1)
    assert np.allclose(r.avg_logprob.double().cpu().numpy(), want, rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", ["a", "b"])
def test_item_alone_in_3_and_in_17_and_repeated(name):
    base, d, lay, c, m, _ = setup(name)
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    r = decode(m, lay, d, x, prompt)
    r2 = decode(m, lay, d, x, prompt)
    for a, b in ((r.tokens, r2.tokens), (r.lengths, r2.lengths), (r.sum_logprob, r2.sum_logprob), (r.no_speech_prob, r2.no_speech_prob)):
        assert torch.equal(a, b)
    idx = [(3 * i + 1) % 3 for i in range(17)]                  # item 1 first and at place 16: both launch groups
    big = decode(m, lay, d, x[idx].contiguous(), prompt[idx].contiguous())
    for j, b in enumerate(idx):
        assert torch.equal(big.tokens[j], r.tokens[b]) and int(big.lengths[j]) == int(r.lengths[b])
        assert big.sum_logprob[j].item() == r.sum_logprob[b].item() and big.no_speech_prob[j].item() == r.no_speech_prob[b].item()
    for b in range(3):
        one = decode(m, lay, d, x[b:b + 1], prompt[b:b + 1])
        assert torch.equal(one.tokens[0], r.tokens[b]) and int(one.lengths[0]) == int(r.lengths[b])
        assert one.sum_logprob[0].item() == r.sum_logprob[b].item() and one.no_speech_prob[0].item() == r.no_speech_prob[b].item()


@pytest.mark.parametrize("name", ["a", "b"])
def test_generate_keeps_its_tokens_after_decode(name):
    base, d, lay, c, m, _ = setup(name)
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    decode(m, lay, d, x, prompt)
    tokens, n = m.generate(x, prompt, base["tokens"].shape[1], eos_token_id=int(base["eos"]), suppress_tokens=[], begin_suppress_tokens=[])
    assert np.array_equal(tokens.cpu().numpy(), base["tokens"]) and np.array_equal(n.cpu().numpy(), base["lengths"])


# ---- us_whisper_select alone -------------------------------------------------------------------------------------------------------


def random_history(g, lay, V, kind):
    """the tokens sampled so far for one of the rules' branches"""
    eos, tb = lay["eos"], lay["no_timestamps"] + 1
    text = lambda: int(g.integers(0, eos))
    ts = lambda lo=tb: int(g.integers(lo, V))
    if kind == "first":
        return []
    if kind == "one_ts":                 # last_ts, pen_ts (fewer than two)
        return [ts()]
    if kind == "ts_text":                # neither
        return [ts(), text()]
    if kind == "text_ts":                # last_ts, not pen_ts
        a = ts()
        return [a, text(), ts(a)]
    if kind == "ts_ts":                  # last_ts, pen_ts
        a = ts()
        return [a, text(), ts(a), ts(a)]
    if kind == "exhausted":              # the last timestamp token of all was sampled twice: no timestamp is left
        return [tb, text(), V - 1, V - 1, text()]
    if kind == "text_only":              # no timestamp yet (a history the loop cannot reach, but the rules cover)
        return [text(), text()]
    raise KeyError(kind)


KINDS = ("ts_text", "text_ts", "text_only", "first", "one_ts", "ts_ts", "exhausted")       # the first three leave the decision free


def shifted_cases(seed, B, V, lay, want_decided, sup=None, beg=None):
    """seeded logits, histories over every branch, and the timestamp side shifted so that a free decision falls as `want_decided[b]` with
    |d| >= 1e-3 (asserted in fp64)"""
    g = np.random.Generator(np.random.Philox(key=seed))
    x = g.standard_normal((B, V)).astype(np.float32) * 3
    tb = lay["no_timestamps"] + 1
    hist = [random_history(g, lay, V, KINDS[b % len(KINDS)]) for b in range(B)]
    for b in range(B):
        r = rules.select(x[b], hist[b], lay, sup, beg)
        if r["free"]:
            x[b, tb:] += np.float32((0.5 if want_decided[b] else -0.5) - r["d"])
            r = rules.select(x[b], hist[b], lay, sup, beg)
            assert r["decided"] == bool(want_decided[b])
        assert not r["free"] or abs(r["d"]) >= 1e-3
    return x, hist


def run_select(x, hist, lay, suppress=None, begin_suppress=None):
    dev = lambda m: None if m is None else torch.from_numpy(m.astype(np.uint8)).cuda()
    tok, lp, dec = select_tokens(torch.from_numpy(x).cuda(), [rules.history(h, lay) for h in hist], eos_token_id=lay["eos"],
                                 no_timestamps_id=lay["no_timestamps"], max_initial_timestamp_index=lay["max_initial_timestamp_index"],
                                 suppress=dev(suppress), begin_suppress=dev(begin_suppress))
    return tok.cpu().numpy(), lp.cpu().numpy(), dec.cpu().numpy()


@pytest.mark.parametrize("B", [3, 17])
def test_select_at_the_real_vocabulary(B):
    """Log-probability within 6.5e-6 absolute of the fp64 statement: ten times the fp32 numpy statement's own error on these cases
    (5.5e-7 at B = 3, 6.5e-7 at B = 17; the library measured the same two figures).  Both are printed."""
    want = [(b // len(KINDS) + b) % 2 for b in range(B)]
    sup = np.zeros(V_REAL, dtype=bool)
    sup[[1, 2, 7, 8, 9, 50258, 50259, 50358, 50359, 50360, 50361, 50362]] = True
    beg = np.zeros(V_REAL, dtype=bool)
    beg[[220, 50257]] = True
    x, hist = shifted_cases(5100 + B, B, V_REAL, REAL, want, sup, beg)
    ref = [rules.select(x[b], hist[b], REAL, sup, beg) for b in range(B)]
    r32 = [rules.select(x[b], hist[b], REAL, sup, beg, np.float32) for b in range(B)]
    assert {r["decided"] for r in ref if r["free"]} == {True, False}
    assert all(abs(r["d"]) >= 1e-3 for r in ref if r["free"])
    tok, lp, dec = run_select(x, hist, REAL, sup, beg)
    assert tok.tolist() == [r["token"] for r in ref]
    assert dec.tolist() == [int(r["decided"]) for r in ref]
    e = max(abs(float(lp[b]) - ref[b]["logprob"]) for b in range(B))
    s = max(abs(r32[b]["logprob"] - ref[b]["logprob"]) for b in range(B))
    print(f"select V={V_REAL} B={B}: library {e:.3e}  fp32 numpy statement {s:.3e}")
    assert e <= 6.5e-6


@pytest.mark.parametrize("V,lay", [(96, dict(eos=35, no_timestamps=87, max_initial_timestamp_index=2)),
                                   (203, dict(eos=178, no_timestamps=190, max_initial_timestamp_index=-1)),
                                   (1300, dict(eos=400, no_timestamps=700, max_initial_timestamp_index=30))])
def test_select_small_vocabularies_every_branch(V, lay):
    """V below one chunk of 512 (96, 203) and over three chunks with timestamp_begin inside the second (1300)"""
    B = 4 * len(KINDS)
    want = [(b // len(KINDS)) % 2 for b in range(B)]
    sup = np.zeros(V, dtype=bool)
    sup[[5, lay["eos"] + 1, lay["no_timestamps"] - 1]] = True
    beg = np.zeros(V, dtype=bool)
    beg[[7, lay["eos"], lay["no_timestamps"] + 2]] = True
    x, hist = shifted_cases(6000 + V, B, V, lay, want, sup, beg)
    ref = [rules.select(x[b], hist[b], lay, sup, beg) for b in range(B)]
    tok, lp, dec = run_select(x, hist, lay, sup, beg)
    assert tok.tolist() == [r["token"] for r in ref]
    assert dec.tolist() == [int(r["decided"]) for r in ref]
    assert max(abs(float(lp[b]) - ref[b]["logprob"]) for b in range(B)) <= 1e-5
    # a done item returns eos at no cost
    h = [rules.history(hist[0], lay, done=True)]
    t1, l1, d1 = select_tokens(torch.from_numpy(x[:1]).cuda(), h, eos_token_id=lay["eos"], no_timestamps_id=lay["no_timestamps"])
    assert int(t1[0]) == lay["eos"] and float(l1[0]) == 0.0 and int(d1[0]) == 0


def test_select_planted_ties_and_empty_sides():
    V, lay = 203, dict(eos=178, no_timestamps=190, max_initial_timestamp_index=-1)
    tb = 191
    g = np.random.Generator(np.random.Philox(key=77))
    x = (g.standard_normal((5, V)) * 0.5).astype(np.float32)
    hist = [[tb, 3], [tb, 3], [tb + 3, 4, V - 2], [tb, tb], []]
    # 0: an exact tie of two text maxima: the lower index wins
    x[0, [150, 20]] = 4.0
    x[0, tb:] = -9.0
    # 1: d = 0 exactly: one timestamp left allowed (the last one, after V - 2 was sampled twice) with the best text logit's value: text wins
    hist[1] = [tb, 3, V - 2, V - 2, 5]
    x[1, 60] = 2.5
    x[1, V - 1] = 2.5
    # 2: text -> timestamp: text below eos masked, [eos, tb) allowed
    # 3: two timestamps: the timestamp side is empty
    # 4: the first position with every timestamp suppressed: nothing survives, eos at log-probability 0
    sup = np.zeros((5, V), dtype=bool)
    sup[4, tb:] = True
    ref = [rules.select(x[b], hist[b], lay, sup[b]) for b in range(5)]
    assert ref[0]["token"] == 20 and ref[1]["token"] == 60 and ref[1]["d"] == 0.0 and not ref[1]["decided"]
    assert abs(ref[0]["d"]) >= 1e-3 and abs(ref[2]["d"]) >= 1e-3
    assert not ref[3]["free"] and ref[3]["token"] < tb and ref[4]["token"] == lay["eos"] and ref[4]["logprob"] == 0.0
    for b in range(5):
        tok, lp, dec = run_select(x[b:b + 1], hist[b:b + 1], lay, sup[b])
        assert int(tok[0]) == ref[b]["token"] and int(dec[0]) == int(ref[b]["decided"]), (b, tok, ref[b])
        assert abs(float(lp[0]) - ref[b]["logprob"]) <= 1e-5


def test_select_item_alone_and_in_batches_bit_equal():
    want = [b % 2 for b in range(17)]
    x, hist = shifted_cases(5300, 17, V_REAL, REAL, want)
    tok, lp, dec = run_select(x, hist, REAL)
    for b in (0, 5, 16):
        t1, l1, d1 = run_select(x[b:b + 1], hist[b:b + 1], REAL)
        assert t1[0] == tok[b] and l1[0] == lp[b] and d1[0] == dec[b]
    t3, l3, d3 = run_select(x[[16, 0, 5]], [hist[16], hist[0], hist[5]], REAL)
    assert t3.tolist() == tok[[16, 0, 5]].tolist() and l3.tolist() == lp[[16, 0, 5]].tolist()
    t2, l2, _ = run_select(x, hist, REAL)
    assert np.array_equal(t2, tok) and np.array_equal(l2, lp)


def test_library_refusals():
    base, d, lay, c, m, _ = setup("a")
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    V, Tm, P = c["vocab_size"], c["max_target_positions"], prompt.shape[1]
    kw = dict(no_timestamps_id=lay["no_timestamps"], max_new_tokens=4)
    with pytest.raises(RuntimeError, match="us_whisper_decode.*EINVAL.*eos"):
        m.decode(x, prompt, eos_token_id=lay["no_timestamps"], **kw)
    with pytest.raises(RuntimeError, match="us_whisper_decode.*EINVAL.*no timestamp token"):
        m.decode(x, prompt, no_timestamps_id=V - 1, max_new_tokens=4)
    with pytest.raises(RuntimeError, match="us_whisper_decode.*EINVAL.*sot_index"):
        m.decode(x, prompt, sot_index=P, **kw)
    with pytest.raises(RuntimeError, match="us_whisper_decode.*EINVAL.*max_target_positions"):
        m.decode(x, prompt, no_timestamps_id=lay["no_timestamps"], max_new_tokens=Tm - P + 1)
    with pytest.raises(RuntimeError, match="us_whisper_decode.*EINVAL.*outside the vocabulary"):
        m.decode(x, torch.tensor([[1, V]] * 3), **kw)
    lg = torch.zeros(1, V, device="cuda")
    with pytest.raises(RuntimeError, match="us_whisper_select.*EINVAL.*eos"):
        select_tokens(lg, [(0, -1, -1, -1, 0)], eos_token_id=50, no_timestamps_id=50)
    with pytest.raises(RuntimeError, match="us_whisper_select.*EINVAL.*no timestamp token"):
        select_tokens(lg, [(0, -1, -1, -1, 0)], eos_token_id=5, no_timestamps_id=V - 1)
    lib = _lib.load()
    assert lib.us_whisper_select_scratch_bytes(0) == 0
    # the suite goes on from a working model
    r = decode(m, lay, d, x, prompt)
    assert np.array_equal(r.tokens.cpu().numpy(), d["tokens"])


def test_evaluate_synthetic_whisper_timestamps_end_to_end(tmp_path):
    out = tmp_path / "result.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--batch", "4", "--recogniser", "whisper",
                        "--whisper_timestamps", "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(out.read_text())
    assert res["files"] == 6 and len(res["per_file"]) == 6
    assert abs(res["cer"] - res["expected_cer"]) <= 1e-12
    for rec in res["per_file"]:
        assert isinstance(rec["segments"], list)
        assert np.isfinite(rec["avg_logprob"]) and 0.0 <= rec["no_speech_prob"] <= 1.0
