"""Whisper's beam search under the timestamp rules as tools/whisper_beam_numpy.py states it (the yardstick of us_whisper_decode_beam), over toy
logits; the walk / pool / ranking functions of csrc/whisper_beam.h, built into tools/whisper_beam_check.cpp under AddressSanitizer and UBSan,
against that statement; and the goldens tests/golden/whisper_beam_{a,b,wide}.npz against `WhisperTorch(float64).decode_beam`."""
import json
import os
import shutil
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
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

# text 0 1 2, eos 3, no_timestamps 4, timestamps 5 6 7
TOY = dict(eos=3, no_timestamps=4, max_initial_timestamp_index=-1)
V_TOY = 8
NINF = float("-inf")


def logp(**p):
    """logits [V_TOY]: log of the given probabilities by token (t5=0.6), -inf elsewhere"""
    x = np.full(V_TOY, NINF)
    for k, v in p.items():
        x[int(k[1:])] = np.log(v)
    return x


class Table:
    """a logits callback that reads a table by the row's sequence and follows the parents beam_search reports"""

    def __init__(self, table, n, default=None):
        self.table, self.n, self.default, self.seqs = table, n, default, [()] * n

    def __call__(self, i, tokens, parents):
        if i > 0:
            self.seqs = [self.seqs[p] + (t,) for p, t in zip(parents, tokens)]
        return np.stack([self.table.get(s, self.default if self.default is not None else np.full(V_TOY, NINF)) for s in self.seqs])


HAND = {(): logp(t5=0.6, t6=0.4),
        (5,): logp(t0=0.55, t1=0.45), (6,): logp(t2=0.9, t0=0.1),
        (5, 0): logp(t3=0.6, t1=0.4), (6, 2): logp(t3=0.9, t1=0.1), (5, 1): logp(t3=0.5, t2=0.5), (6, 0): logp(t3=0.5, t2=0.5)}


def test_beam_of_one_is_greedy_decode():
    lay = dict(eos=30, no_timestamps=33, max_initial_timestamp_index=2, suppress=[31], begin_suppress=[7, 30])
    V, steps, ended = 40, 12, set()
    for seed in range(12):
        g = np.random.Generator(np.random.Philox(key=900 + seed))
        x = g.standard_normal((steps, V)) * 3
        x[:, 30] += 1.5 + 0.3 * np.arange(steps) if seed % 3 else -20.0       # eos becomes likely, or never is: some items end, some do not
        want = rules.decode(x, lay)
        got = beam.beam_search(lambda i, tokens, parents: x[i][None], 1, 1, steps, lay, V)
        assert np.array_equal(got["tokens"], want["tokens"]) and got["length"] == want["length"]
        assert abs(got["sum_logprob"] - want["sum_logprob"]) <= 1e-12
        ended.add(want["length"] < steps)
    assert ended == {True, False}


def test_two_beams_find_what_greedy_misses():
    greedy = beam.beam_search(Table(HAND, 1), 1, 1, 3, TOY, V_TOY)
    assert greedy["tokens"].tolist() == [5, 0, 3] and greedy["length"] == 2
    assert abs(greedy["sum_logprob"] - np.log(0.6 * 0.55 * 0.6)) <= 1e-12
    r = beam.beam_search(Table(HAND, 2), 2, 2, 3, TOY, V_TOY)
    assert r["tokens"].tolist() == [6, 2, 3] and r["length"] == 2 and r["ended_by"] == "pool"
    assert abs(r["sum_logprob"] - np.log(0.4 * 0.9 * 0.9)) <= 1e-12
    # step 1: [6, 2] at 0.36 in front of [5, 0] at 0.33, a parent that moves (row 0 continues row 1)
    assert [(p, t) for p, t, _ in r["steps"][1]["rows"]] == [(1, 2), (0, 0)]
    assert [e[0] for e in r["pool"]] == [(6, 2), (5, 0)]


def test_step_0_reads_row_0_alone():
    x = np.stack([HAND[()], np.full(V_TOY, np.nan), np.full(V_TOY, np.nan)])
    r = beam.beam_step(x, [[], [], []], [0.0] * 3, [True, False, False], [], 3, 3, TOY)
    assert [c[0] for c in r["cands"]] == [0, 0] and r["rows"] == [(0, 5, np.log(0.6)), (0, 6, np.log(0.4))]
    assert r["live"] == [True, True, False] and r["parents"] == [0, 0, -1]


def test_a_dead_row_offers_nothing_is_never_finalised_and_is_refilled():
    r0 = beam.beam_step(np.stack([HAND[()]] * 3), [[], [], []], [0.0] * 3, [True, False, False], [], 3, 3, TOY)
    assert r0["live"] == [True, True, False] and not r0["ended"]
    assert len(beam.finalise([], r0["seqs"], r0["scores"], r0["live"], 3)) == 2
    x = np.stack([HAND[(5,)], HAND[(6,)], np.full(V_TOY, np.nan)])
    r1 = beam.beam_step(x, r0["seqs"], r0["scores"], r0["live"], r0["pool"], 3, 3, TOY)
    assert {c[0] for c in r1["cands"]} == {0, 1}
    assert r1["live"] == [True, True, True] and r1["seqs"] == [[6, 2], [5, 0], [5, 1]] and r1["parents"] == [1, 0, 0]


def test_eos_in_front_of_the_stop_is_recorded_and_behind_it_ignored():
    eos = 3
    cands = [(0, eos, -0.1), (0, 1, -0.2), (1, 2, -0.3), (1, eos, -0.4), (0, 2, -0.5)]
    w = beam.walk(cands, 2, 2, eos, 0)
    assert w["finished"] == [(0, -0.1)] and w["rows"] == [(0, 1, -0.2), (1, 2, -0.3)] and w["walked"] == 3 and w["added"] == 1
    w = beam.walk(cands, 3, 2, eos, 0)
    assert w["finished"] == [(0, -0.1), (1, -0.4)] and len(w["rows"]) == 3 and w["walked"] == 5 and w["added"] == 2
    assert beam.walk(cands, 3, 2, eos, 1)["added"] == 1 and beam.walk(cands, 3, 2, eos, 2)["added"] == 0


def test_patience():
    assert beam.max_candidates(5, 0.5) == 2 and beam.max_candidates(2, 2.0) == 4 and beam.max_candidates(3) == 3 and beam.max_candidates(5, 0.5) == round(5 * 0.5)
    # n = 2, C = 4: two entries finish at step 2 and the search goes on
    table = dict(HAND)
    table[(5, 0, 1)] = logp(t3=0.7, t2=0.3)
    table[(6, 2, 1)] = logp(t3=0.8, t0=0.2)
    r = beam.beam_search(Table(table, 2, default=logp(t3=0.5, t1=0.5)), 2, 4, 5, TOY, V_TOY)
    assert len(r["steps"]) > 3 and len(r["steps"][2]["pool"]) == 2 and not r["steps"][2]["ended"]
    assert r["ended_by"] == "pool" and len(r["pool"]) == 4
    # n = 3, C = 1: the first finished entry ends the item and finalise tops the pool up to 3 with live rows
    r = beam.beam_search(Table(HAND, 3), 3, 1, 3, TOY, V_TOY)
    assert r["ended_by"] == "pool" and len(r["steps"][-1]["pool"]) == 1 and len(r["pool"]) == 3
    assert all(len(seq) == len(r["steps"]) for seq, _ in r["pool"][1:])


def test_equal_totals_keep_row_then_rank_order():
    eos = 3
    cands = [(0, 1, -1.0), (0, 2, -1.0), (1, 0, -1.0), (1, 2, -0.5), (2, 1, -1.0)]
    w = beam.walk(cands, 4, 4, eos, 0)
    assert w["order"] == [3, 0, 1, 2, 4] and [(p, t) for p, t, _ in w["rows"]] == [(1, 2), (0, 1), (0, 2), (1, 0)]
    # the top n + 1 of a row: the lower id first on equal logits
    x = np.full(V_TOY, NINF)
    x[[0, 1, 2]] = 0.0
    top, _ = beam.row_candidates(x, [5, 0], TOY, k=2)
    assert [t for t, _ in top] == [0, 1]
    x[:] = NINF
    assert beam.row_candidates(x, [5, 0], TOY, k=3)[0] == [(3, 0.0)]                # nothing survives: (eos, 0)
    x[1] = 0.0
    assert beam.row_candidates(x, [5, 0], TOY, k=3)[0] == [(1, 0.0)]                # -inf is never a candidate


def test_the_ranker_divides_by_length():
    assert beam.rank([((1, 2, 0, 1), -4.0), ((1, 2), -3.0)]) == 0
    assert beam.rank([((1, 2), -3.0), ((1, 2, 0, 1), -4.0)]) == 1
    assert beam.rank([((), 0.0), ((1,), -5.0)]) == 1 and beam.rank([((1,), -5.0), ((), 0.0)]) == 0
    assert beam.rank([((1, 2), -2.0), ((2,), -1.0)]) == 0                           # a tie: the earlier entry


# ---- csrc/whisper_beam.h under the sanitizers ------------------------------------------------------------------------------------------


def random_sequence(g, lay, V):
    eos, tb = lay["eos"], lay["no_timestamps"] + 1
    kind = int(g.integers(0, 5))
    text = lambda: int(g.integers(0, eos))
    a = int(g.integers(tb, V - 1))
    return [[], [a], [a, text()], [a, text(), int(g.integers(a, V))], [a, text(), a + 1, a + 1][:2 + 2 * (a + 1 < V)]][kind]


def test_the_header_under_sanitizers_agrees_with_numpy(tmp_path):
    cxx = next((c for c in (shutil.which(n) for n in ("c++", "g++", "clang++")) if c), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "whisper_beam_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "unitspeech_amd", "csrc"), os.path.join(ROOT, "tools", "whisper_beam_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    lay, V = dict(eos=20, no_timestamps=23, max_initial_timestamp_index=3), 40
    g = np.random.Generator(np.random.Philox(key=4242))
    lines, want = [], []
    for case in range(260):
        n = [1, 2, 3, 5, 16][case % 5]
        C = int(g.integers(1, 2 * n + 1))
        pool = int(g.integers(0, C))
        live = [bool(g.integers(0, 4)) for _ in range(n)]
        live[int(g.integers(0, n))] = True
        seqs = [random_sequence(g, lay, V) for _ in range(n)]
        coarse = case % 3 == 0                          # logits and scores on a grid: equal totals within and across rows
        x = np.round(g.standard_normal((n, V)) * 2) / 2 if coarse else g.standard_normal((n, V)) * 3
        x[:, lay["eos"]] += 2.0
        if coarse and n > 1:
            x[1], seqs[1] = x[0], list(seqs[0])
        scores = [float(np.round(g.standard_normal()) if coarse else g.standard_normal() * 2) for _ in range(n)]
        if coarse and n > 1:
            scores[1] = scores[0]
        r = beam.beam_step(x, seqs, scores, live, [((1,), -1.0)] * pool, n, C, lay)
        line = [f"S {n} {C} {lay['eos']} {pool}"]
        for j in range(n):
            top, _ = beam.row_candidates(x[j], seqs[j], lay, k=n + 1)
            line.append(f"{int(live[j])} {scores[j]!r} {len(top)} " + " ".join(f"{t} {lp!r}" for t, lp in top))
        lines.append(" ".join(line))
        want.append("S rows %d" % len(r["rows"]) + "".join(" %d %d %.17g" % row for row in r["rows"]) + " fin %d" % len(r["finished"])
                    + "".join(" %d %.17g" % f for f in r["finished"]) + " added %d walked %d ended %d" % (r["added"], r["walked"], int(r["ended"])))
        # finalise and rank over the step's result and a random pool
        k = int(g.integers(0, n + 3))
        entries = [(tuple(range(int(g.integers(0, 6)))), float(np.round(g.standard_normal() * 4) / 2)) for _ in range(k)]
        if not entries and not any(r["live"]):
            entries = [((), 0.0)]
        full = beam.finalise(entries, r["seqs"], r["scores"], r["live"], n)
        top = sorted((j for j in range(n) if r["live"][j]), key=lambda j: -r["scores"][j])[:max(0, n - len(entries))]
        assert full[len(entries):] == [(tuple(r["seqs"][j]), r["scores"][j]) for j in top]
        lines.append(f"F {n} {len(entries)} " + " ".join(f"{s!r} {len(q)}" for q, s in entries) + " "
                     + " ".join(f"{int(r['live'][j])} {r['scores'][j]!r} {len(r['seqs'][j])}" for j in range(n)))
        want.append("F top %d" % len(top) + "".join(" %d" % j for j in top) + " winner %d" % beam.rank(full))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.strip().split("\n")
    assert len(got) == len(want) == 520
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, lines[i], a, b)
    # the same cases through stdin
    again = subprocess.run([exe], input=path.read_text(), capture_output=True, text=True)
    assert again.returncode == 0 and again.stdout == run.stdout


# ---- the goldens ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["a", "b", "wide"])
def test_goldens_are_what_the_fp64_restatement_decodes(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
        c, sd, feats, prompts = json.loads(str(g["config"])), golden_state_dict(g), g["features"], torch.from_numpy(g["prompt"])
    with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) as g:
        lay, sot = json.loads(str(g["layout"])), int(g["sot_index"])
    with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_beam_{name}.npz")) as g:
        b = {k: g[k] for k in g.files}
    assert float(b["min_gap"]) >= 1e-3 and float(b["min_abs_d"]) >= 1e-2
    assert {(3, 3), (5, 5), (2, 4)} <= set(zip(b["n"].tolist(), b["C"].tolist()))
    assert b["differs_from_greedy"].any() and {"pool", "max_new"} <= set(b["ended_by"].tolist())
    assert {"differs", "pool_end", "max_new_topup", "eos_behind", "eos_recorded", "dead_row", "parent_moves", "two_children"} <= \
        {k for case in json.loads(str(b["covers"])) for k in case}
    m = WhisperTorch(sd, c, torch.float64)
    for i, seed in enumerate(b["seeds"].tolist()):
        n, C, max_new = int(b["n"][i]), int(b["C"][i]), int(b["max_new"][i])
        r = m.decode_beam(torch.from_numpy(draw(seed, feats)), prompts[seed % 3:seed % 3 + 1], max_new, lay, n, C, sot)
        assert np.array_equal(r["tokens"][0], b["tokens"][i, :max_new]) and int(r["lengths"][0]) == int(b["lengths"][i])
        assert (b["tokens"][i, max_new:] == lay["eos"]).all()
        assert abs(r["sum_logprob"][0] - b["sum_logprob"][i]) <= 1e-12 and abs(r["no_speech_prob"][0] - b["no_speech_prob"][i]) <= 1e-12
        assert r["items"][0]["ended_by"] == str(b["ended_by"][i])


# ---- the Python interface's own refusals (no device is touched) ------------------------------------------------------------------------


def test_patience_needs_a_beam_size_and_beams_need_timestamps():
    from unitspeech_amd.whisper import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(num_mel_bins=16, d_model=64, encoder_layers=1, encoder_attention_heads=2, encoder_ffn_dim=64, decoder_layers=1,
                                        decoder_attention_heads=2, decoder_ffn_dim=64, max_source_positions=50, max_target_positions=24, vocab_size=96,
                                        eos_token_id=25).eval()
    with pytest.raises(ValueError, match="patience.*beam_size"):
        m.decode(torch.zeros(1, 16, 100), [1, 2], no_timestamps_id=87, patience=2.0)
    m.prompt_ids, m.no_timestamps_id = [1, 2, 87], 87
    with pytest.raises(ValueError, match="beam_size.*timestamps=True"):
        m.transcribe_ids(torch.zeros(1, 1600), beam_size=3)
