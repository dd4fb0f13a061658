"""Beam search under the timestamp rules on the GPU (csrc/whisper.hip: us_whisper_decode_beam, us_whisper_beam_select) against the goldens
tests/golden/whisper_beam_{a,b}.npz (tools/make_goldens_whisper_beam.py, fp64) and against the fp64 numpy statement of one step
(tools/whisper_beam_numpy.py).

Tokens, lengths, parents and the order of the new rows are compared exactly: the goldens keep every comparison the search makes 1e-3 of the
largest |logit| away from a tie, and the seeded steps are asserted to keep their sorted totals 1e-4 apart in fp64.  Scores follow the project's
rule: the library's distance from fp64 is at most max(10 x the fp32 restatement's distance, 1e-5 x max |golden|); both are printed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_beam_numpy as beam  # noqa: E402
import whisper_decode_numpy as rules  # noqa: E402
from make_goldens_whisper_beam import draw  # noqa: E402
from test_whisper_decode_gpu import KINDS, random_history  # noqa: E402
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd.whisper import WhisperForConditionalGeneration, select_beams  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}
REAL = dict(eos=50257, no_timestamps=50363, max_initial_timestamp_index=50)
V_REAL = 51865


def setup(name):
    """the goldens of a model, the model on the device and the fp32 restatement's beam search of every case: made once, never changed"""
    if name not in _CACHE:
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
            base = {k: g[k] for k in ("features", "prompt", "tokens", "lengths", "eos")}
            c, sd = json.loads(str(g["config"])), golden_state_dict(g)
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) as g:
            d = {k: g[k] for k in g.files}
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_beam_{name}.npz")) as g:
            b = {k: g[k] for k in g.files}
        lay = json.loads(str(d["layout"]))
        m = WhisperForConditionalGeneration(**c, eos_token_id=lay["eos"], suppress_tokens=lay["suppress"], begin_suppress_tokens=lay["begin_suppress"])
        m.load_state_dict(sd)
        t32 = WhisperTorch(sd, c, torch.float32)
        r32 = [t32.decode_beam(torch.from_numpy(draw(seed, base["features"])), torch.from_numpy(base["prompt"][seed % 3:seed % 3 + 1]),
                               int(b["max_new"][i]), lay, int(b["n"][i]), int(b["C"][i]), int(d["sot_index"]))
               for i, seed in enumerate(b["seeds"].tolist())]
        _CACHE[name] = (base, d, b, lay, c, m.cuda().eval(), r32)
    return _CACHE[name]


def decode(m, lay, d, x, prompt, max_new=None, **kw):
    cap = lay["max_initial_timestamp_index"]
    return m.decode(x, prompt, no_timestamps_id=lay["no_timestamps"], max_initial_timestamp=None if cap < 0 else 0.02 * cap,
                    no_speech_id=lay["no_speech"], max_new_tokens=int(d["max_new"]) if max_new is None else max_new, sot_index=int(d["sot_index"]),
                    **kw)


def same(a, b):
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.sum_logprob, b.sum_logprob)
            and torch.equal(a.no_speech_prob, b.no_speech_prob))


@pytest.mark.parametrize("name", ["a", "b"])
def test_beam_matches_the_golden(name):
    base, d, b, lay, c, m, r32 = setup(name)
    got, s32 = [], []
    for i, seed in enumerate(b["seeds"].tolist()):
        n, C, max_new = int(b["n"][i]), int(b["C"][i]), int(b["max_new"][i])
        assert np.array_equal(r32[i]["tokens"][0], b["tokens"][i, :max_new])
        x, prompt = torch.from_numpy(draw(seed, base["features"])).cuda(), torch.from_numpy(base["prompt"][seed % 3:seed % 3 + 1])
        r = decode(m, lay, d, x, prompt, max_new, beam_size=n, patience=C / n)
        assert r.tokens.dtype == r.lengths.dtype == torch.int64 and tuple(r.tokens.shape) == (1, max_new)
        assert int(r.lengths[0]) == int(b["lengths"][i]), (i, r.lengths, b["lengths"][i])
        assert np.array_equal(r.tokens[0].cpu().numpy(), b["tokens"][i, :max_new]), (i, r.tokens, b["tokens"][i])
        assert torch.equal(r.no_speech_prob, decode(m, lay, d, x, prompt, max_new).no_speech_prob)           # the bits of `decode`
        assert np.isclose(float(r.avg_logprob[0]), b["sum_logprob"][i] / (b["lengths"][i] + 1), rtol=1e-5, atol=0)
        got.append(float(r.sum_logprob[0]))
        s32.append(float(r32[i]["sum_logprob"][0]))
    e, s, mag = float(np.abs(np.asarray(got) - b["sum_logprob"]).max()), float(np.abs(np.asarray(s32) - b["sum_logprob"]).max()), float(np.abs(b["sum_logprob"]).max())
    print(f"whisper_beam_{name} sum_logprob: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.3f}")
    assert np.isfinite(e) and e <= max(10 * s, 1e-5 * mag), (e, s, mag)


@pytest.mark.parametrize("name", ["a", "b"])
def test_one_beam_is_greedy_decode(name):
    base, d, b, lay, c, m, _ = setup(name)
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    r, g = decode(m, lay, d, x, prompt, beam_size=1), decode(m, lay, d, x, prompt)
    assert np.array_equal(g.tokens.cpu().numpy(), d["tokens"])
    assert torch.equal(r.tokens, g.tokens) and torch.equal(r.lengths, g.lengths) and torch.equal(r.no_speech_prob, g.no_speech_prob)
    assert torch.allclose(r.sum_logprob, g.sum_logprob, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("name", ["a", "b"])
def test_item_alone_in_3_and_in_17_and_repeated(name, n):
    base, d, b, lay, c, m, _ = setup(name)
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    r = decode(m, lay, d, x, prompt, beam_size=n)
    assert same(r, decode(m, lay, d, x, prompt, beam_size=n))
    idx = [(2 * i + 1) % 3 for i in range(17)]           # groups of 16 // n items: every item first and last in a group, and in a last, short group
    big = decode(m, lay, d, x[idx].contiguous(), prompt[idx].contiguous(), beam_size=n)
    for j, k in enumerate(idx):
        assert torch.equal(big.tokens[j], r.tokens[k]) and int(big.lengths[j]) == int(r.lengths[k]), (j, k)
        assert big.sum_logprob[j].item() == r.sum_logprob[k].item() and big.no_speech_prob[j].item() == r.no_speech_prob[k].item()
    for k in range(3):
        one = decode(m, lay, d, x[k:k + 1], prompt[k:k + 1], beam_size=n)
        assert torch.equal(one.tokens[0], r.tokens[k]) and int(one.lengths[0]) == int(r.lengths[k])
        assert one.sum_logprob[0].item() == r.sum_logprob[k].item() and one.no_speech_prob[0].item() == r.no_speech_prob[k].item()


@pytest.mark.parametrize("name", ["a", "b"])
def test_greedy_keeps_its_tokens_after_a_beam_call(name):
    base, d, b, lay, c, m, _ = setup(name)
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    decode(m, lay, d, x, prompt, beam_size=5)
    r = decode(m, lay, d, x, prompt)
    assert np.array_equal(r.tokens.cpu().numpy(), d["tokens"]) and np.array_equal(r.lengths.cpu().numpy(), d["lengths"])
    tokens, cnt = m.generate(x, prompt, base["tokens"].shape[1], eos_token_id=int(base["eos"]), suppress_tokens=[], begin_suppress_tokens=[])
    assert np.array_equal(tokens.cpu().numpy(), base["tokens"]) and np.array_equal(cnt.cpu().numpy(), base["lengths"])


# ---- us_whisper_beam_select alone ------------------------------------------------------------------------------------------------------


def seeded_step(seed0, B, n, V, lay, sup=None, beg=None):
    """seeded logits [B n][V], histories over every branch of KINDS, scores and live flags, every free decision moved 0.5 away from a tie;
    the first seed whose sorted totals are 1e-4 apart in fp64 (asserted)"""
    tb = lay["no_timestamps"] + 1
    for seed in range(seed0, seed0 + 40):
        g = np.random.Generator(np.random.Philox(key=seed))
        R = B * n
        x = g.standard_normal((R, V)).astype(np.float32) * 3
        x[::3, lay["eos"]] += np.float32(9)              # eos among the candidates of every third row: entries finish
        hist = [random_history(g, lay, V, KINDS[m % len(KINDS)]) for m in range(R)]
        live = [bool(m % n == 0 or g.integers(0, 5)) for m in range(R)]
        scores = [float(np.float32(g.standard_normal() * 2)) for _ in range(R)]
        for m in range(R):
            r = rules.select(x[m], hist[m], lay, sup, beg)
            if r["free"]:
                x[m, tb:] += np.float32((0.5 if (m // len(KINDS) + m) % 2 else -0.5) - r["d"])
                assert abs(rules.select(x[m], hist[m], lay, sup, beg)["d"]) >= 1e-3
        ref = [beam.beam_step(x[b * n:(b + 1) * n], hist[b * n:(b + 1) * n], scores[b * n:(b + 1) * n], live[b * n:(b + 1) * n], [], n, 64, lay, sup, beg)
               for b in range(B)]
        if min(r["sort_gap"] for r in ref) >= 1e-4:
            return x, hist, scores, live, ref
    raise AssertionError("no seed keeps the sorted totals apart")


def run_select(x, hist, scores, live, n, lay, suppress=None, begin_suppress=None):
    dev = lambda m: None if m is None else torch.from_numpy(m.astype(np.uint8)).cuda()
    out = select_beams(torch.from_numpy(x).cuda(), [rules.history(h, lay, done=not a) for h, a in zip(hist, live)], scores, n, eos_token_id=lay["eos"],
                       no_timestamps_id=lay["no_timestamps"], max_initial_timestamp_index=lay["max_initial_timestamp_index"], suppress=dev(suppress),
                       begin_suppress=dev(begin_suppress))
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(out, ref, n, eos):
    """parents, tokens, counts and the finished rows exactly -> the largest score distance"""
    e = 0.0
    for b, r in enumerate(ref):
        rows, fin = r["rows"], r["finished"]
        assert int(out["n_live"][b]) == len(rows) and int(out["n_fin"][b]) == len(fin), (b, out["n_live"][b], len(rows), out["n_fin"][b], len(fin))
        assert out["parent"][b].tolist() == [p for p, _, _ in rows] + [-1] * (n - len(rows)), (b, out["parent"][b], rows)
        assert out["token"][b].tolist() == [t for _, t, _ in rows] + [eos] * (n - len(rows)), (b, out["token"][b], rows)
        assert out["fin_parent"][b].tolist() == [p for p, _ in fin] + [-1] * (n - len(fin)), (b, out["fin_parent"][b], fin)
        for k, (_, _, s) in enumerate(rows):
            e = max(e, abs(float(out["score"][b, k]) - s))
        for k, (_, s) in enumerate(fin):
            e = max(e, abs(float(out["fin_score"][b, k]) - s))
    return e


@pytest.mark.parametrize("n,B", [(5, 3), (3, 17)])
def test_select_beams_at_the_real_vocabulary(n, B):
    """Scores within ten times the fp32 numpy statement's own error on these cases.  Measured here on the CPU, the statement's error is
    6.8e-7 at B n = 15 and 5.3e-7 at B n = 51; the library's figure is printed beside it."""
    sup = np.zeros(V_REAL, dtype=bool)
    sup[[1, 2, 7, 8, 9, 50258, 50259, 50358, 50359, 50360, 50361, 50362]] = True
    beg = np.zeros(V_REAL, dtype=bool)
    beg[[220, 50257]] = True
    x, hist, scores, live, ref = seeded_step(8100 + B, B, n, V_REAL, REAL, sup, beg)
    assert any(len(r["rows"]) == n for r in ref) and any(r["finished"] for r in ref)
    r32 = [beam.beam_step(x[b * n:(b + 1) * n], hist[b * n:(b + 1) * n], scores[b * n:(b + 1) * n], live[b * n:(b + 1) * n], [], n, 64, REAL, sup, beg,
                          np.float32) for b in range(B)]
    s = max(abs(s32 - s64) for a, r in zip(r32, ref) for (_, _, s32), (_, _, s64) in zip(a["rows"], r["rows"]))
    out = run_select(x, hist, scores, live, n, REAL, sup, beg)
    e = compare(out, ref, n, REAL["eos"])
    print(f"select_beams V={V_REAL} B={B} n={n}: library {e:.3e}  fp32 numpy statement {s:.3e}")
    assert e <= 10 * s


@pytest.mark.parametrize("n,B", [(5, 3), (3, 17)])
@pytest.mark.parametrize("V,lay", [(96, dict(eos=35, no_timestamps=87, max_initial_timestamp_index=2)),
                                   (203, dict(eos=178, no_timestamps=190, max_initial_timestamp_index=-1)),
                                   (1300, dict(eos=400, no_timestamps=700, max_initial_timestamp_index=30))])
def test_select_beams_small_vocabularies_every_branch(V, lay, n, B):
    """V below one chunk of 512 (96, 203) and over three chunks with timestamp_begin inside the second (1300)"""
    sup = np.zeros(V, dtype=bool)
    sup[[5, lay["eos"] + 1, lay["no_timestamps"] - 1]] = True
    beg = np.zeros(V, dtype=bool)
    beg[[7, lay["eos"], lay["no_timestamps"] + 2]] = True
    x, hist, scores, live, ref = seeded_step(9000 + V + B, B, n, V, lay, sup, beg)
    out = run_select(x, hist, scores, live, n, lay, sup, beg)
    assert compare(out, ref, n, lay["eos"]) <= 1e-5
    again = run_select(x, hist, scores, live, n, lay, sup, beg)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    # an item alone has the bits it has in the batch
    b = B - 1
    one = run_select(x[b * n:(b + 1) * n], hist[b * n:(b + 1) * n], scores[b * n:(b + 1) * n], live[b * n:(b + 1) * n], n, lay, sup, beg)
    assert all(np.array_equal(one[k][0], out[k][b]) for k in out)


def test_select_beams_planted_chunk_edges_ties_and_short_rows():
    V, lay, n = 1300, dict(eos=400, no_timestamps=700, max_initial_timestamp_index=-1), 3
    tb = 701
    g = np.random.Generator(np.random.Philox(key=78))
    base = (g.standard_normal(V) * 0.5).astype(np.float32)
    base[tb:] = -9.0
    hist = [[tb, 3]] * n
    scores, live = [0.0, -0.25, -0.5], [True] * n

    def step(x, hist=hist, sup=None):
        x = np.stack([x] * n)
        ref = beam.beam_step(x, hist, scores, live, [], n, 64, lay, sup)
        out = run_select(x, hist, scores, live, n, lay, sup)
        assert compare(out, [ref], n, lay["eos"]) <= 1e-5
        return ref
    # the top n + 1 of a row on both sides of the chunk edges 511 | 512 and 1023 | 1024 (text and timestamps of a free decision that text wins)
    x = base.copy()
    x[[511, 512, 300, 699]] = [6.0, 5.5, 5.0, 4.5]
    x[[1023, 1024]] = [4.0, 3.5]
    r = step(x)
    assert [t for _, t, _ in r["cands"][:4]] == [511, 512, 300, 699]
    # all of them in one chunk
    x = base.copy()
    x[[10, 20, 30, 40]] = [6.0, 5.5, 5.0, 4.5]
    assert [t for _, t, _ in step(x)["cands"][:4]] == [10, 20, 30, 40]
    # an exact tie of two values in different chunks: the lower id first
    x = base.copy()
    x[[600, 100, 30, 1000]] = [6.0, 6.0, 5.0, 5.0]
    assert [t for _, t, _ in step(x)["cands"][:4]] == [100, 600, 30, 1000]
    # fewer survivors than n + 1: two text tokens and eos are all that is left; the rest is suppressed
    sup = np.ones(V, dtype=bool)
    sup[[100, 600, lay["eos"]]] = False
    r = step(base.copy(), sup=sup)
    assert len(r["cands"]) == 3 * n and len(r["rows"]) == n
    # -inf is never a candidate, and a row with nothing left offers (eos, 0)
    x = np.full(V, -np.inf, dtype=np.float32)
    x[100] = 1.0
    assert [(t, lp) for _, t, lp in step(x)["cands"]] == [(100, 0.0), (100, -0.25), (100, -0.5)]
    r = step(np.full(V, -np.inf, dtype=np.float32))
    assert not r["rows"] and [p for p, _ in r["finished"]] == [0, 1, 2]
    # an empty timestamp side (two timestamps in a row)
    x = base.copy()
    x[[10, 600]] = [3.0, 2.0]
    r = step(x, hist=[[tb, tb]] * n)
    assert all(t < tb for _, t, _ in r["cands"])


# ---- refusals and the command line -----------------------------------------------------------------------------------------------------


def test_library_refusals():
    base, d, b, lay, c, m, _ = setup("a")
    x, prompt = torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"])
    with pytest.raises(RuntimeError, match="us_whisper_decode_beam.*EINVAL.*beam_size"):
        decode(m, lay, d, x, prompt, beam_size=0)
    with pytest.raises(RuntimeError, match="us_whisper_decode_beam.*EINVAL.*beam_size"):
        decode(m, lay, d, x, prompt, beam_size=17)
    with pytest.raises(RuntimeError, match="us_whisper_decode_beam.*EINVAL.*max_candidates"):
        decode(m, lay, d, x, prompt, beam_size=3, patience=0.0)
    with pytest.raises(RuntimeError, match="us_whisper_decode_beam.*EINVAL.*max_candidates"):
        decode(m, lay, d, x, prompt, beam_size=16, patience=5.0)
    with pytest.raises(ValueError, match="patience.*beam_size"):
        decode(m, lay, d, x, prompt, patience=2.0)
    short = torch.empty(4096, dtype=torch.uint8, device="cuda")
    keep, m._beam_workspace = m._beam_workspace, lambda lib, device, B, n: short
    try:
        with pytest.raises(RuntimeError, match="us_whisper_decode_beam.*EINVAL.*workspace too small"):
            decode(m, lay, d, x, prompt, beam_size=3)
    finally:
        m._beam_workspace = keep
    with pytest.raises(RuntimeError, match="us_whisper_beam_select.*EINVAL.*beam_size"):
        select_beams(torch.zeros(17, 96, device="cuda"), [(0, -1, -1, -1, 0)] * 17, [0.0] * 17, 17, eos_token_id=35, no_timestamps_id=87)
    # the suite goes on from a working model
    i = 0
    seed, n, C, max_new = int(b["seeds"][i]), int(b["n"][i]), int(b["C"][i]), int(b["max_new"][i])
    r = decode(m, lay, d, torch.from_numpy(draw(seed, base["features"])).cuda(), torch.from_numpy(base["prompt"][seed % 3:seed % 3 + 1]), max_new,
               beam_size=n, patience=C / n)
    assert np.array_equal(r.tokens[0].cpu().numpy(), b["tokens"][i, :max_new])


def evaluate(tmp_path, tag, *flags):
    out = tmp_path / f"{tag}.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--batch", "4", "--recogniser", "whisper",
                        "--whisper_timestamps", "--out", str(out), *flags], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(out.read_text())


def test_evaluate_synthetic_whisper_beam_end_to_end(tmp_path):
    res = evaluate(tmp_path, "beam3", "--whisper_beam_size", "3")
    assert res["files"] == 6 and len(res["per_file"]) == 6 and res["whisper_beam_size"] == 3 and res["whisper_patience"] == 1.0
    for rec in res["per_file"]:
        assert np.isfinite(rec["avg_logprob"]) and 0.0 <= rec["no_speech_prob"] <= 1.0 and isinstance(rec["segments"], list)
    one, plain = evaluate(tmp_path, "beam1", "--whisper_beam_size", "1"), evaluate(tmp_path, "greedy")
    assert "whisper_beam_size" not in plain
    assert [rec["hypothesis"] for rec in one["per_file"]] == [rec["hypothesis"] for rec in plain["per_file"]]
    assert [rec["segments"] for rec in one["per_file"]] == [rec["segments"] for rec in plain["per_file"]]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--recogniser", "whisper", "--whisper_beam_size", "3"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "--whisper_timestamps" in r.stderr
