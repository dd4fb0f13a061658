#!/usr/bin/env python3
"""Writes tests/golden/whisper_beam_{a,b,wide}.npz: beam search under the timestamp rules over the tiny models of
tests/golden/whisper_{a,b,wide}.npz with the layouts of whisper_decode_{a,b,wide}.npz (weights, prompts and layouts are read from those files and not
stored again), from tools/whisper_torch.py's `WhisperTorch(float64).decode_beam`, which is tools/whisper_beam_numpy.py over the model.

    python tools/make_goldens_whisper_beam.py [name ...]          # no name: all of them

There is no file for whisper_long: over its 132 steps no seed keeps every comparison of the search 1e-3 of the largest |logit| from a tie
(0 of 24 at n = 3 and n = 5; the smallest gaps were 1e-6 to 4e-4), so its beam search is tested by scoring the returned sequence again.

A case is one item: features drawn as seeded N(mean, std) of the stored features (`draw`), the prompt of stored item seed % 3, a beam size n,
max_candidates C and max_new.  Seeds are searched per (n, C, max_new); a case is kept only when, in fp64, with `big` the largest |logit| any
live row saw:
 1. every two neighbours of every step's sorted candidate list, up to and including (last walked, first ignored), are 1e-3 big apart;
 2. the (n + 1)-th and (n + 2)-th survivor of every live row are 1e-3 big apart;
 3. the winner's score / length is 1e-3 big from the runner-up's;
 4. every free timestamp decision of a live row has |d| >= 1e-2;
 5. the fp32 `decode_beam` gives the fp64 tokens;
and a file is written only when its cases cover: n = 3 (C = 3), n = 5 (C = 5), n = 2 with patience 2 (C = 4); a winner that differs from
greedy `decode`; an end by a full pool; an end at max_new with finalise topping the pool up; a step with an eos candidate behind the stop and
one with an eos candidate recorded; a step that leaves a dead row; a new row k whose parent is not k; a parent with two children.

Each file holds per case `seeds`, `n`, `C`, `max_new`, `tokens` [cases][max max_new] (eos at and after the end), `lengths`, `sum_logprob`,
`no_speech_prob`, `ended_by`, `differs_from_greedy`, `covers` (json: the list of what the case shows), and `min_gap` (relative, over 1 - 3),
`min_abs_d`, `max_logit`.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

# (n, C, max_new to try in turn until a seed meets the conditions; None: the decode golden's)
CONFIGS = ((3, 3, (None,)), (5, 5, (None, 12, 8)), (2, 4, (None, 12)), (3, 3, (7,)))
NEEDS = ("differs", "pool_end", "max_new_topup", "eos_behind", "eos_recorded", "dead_row", "parent_moves", "two_children")
MAX_SEEDS = 400


def draw(seed, features):
    """the features of a case: N(mean, std) of the stored features, one item [1][n_mels][T] fp32"""
    g = np.random.Generator(np.random.Philox(key=7700 + int(seed)))
    f = np.asarray(features, dtype=np.float64)
    return (f.mean() + f.std() * g.standard_normal(f.shape[1:])).astype(np.float32)[None]


def covers(item, n, eos, greedy_tokens):
    out = set()
    steps = item["steps"]
    if not np.array_equal(item["tokens"], greedy_tokens):
        out.add("differs")
    if item["ended_by"] == "pool":
        out.add("pool_end")
    if item["ended_by"] == "max_new" and len(steps[-1]["pool"]) < n:
        out.add("max_new_topup")
    for i, s in enumerate(steps):
        if any(s["cands"][c][1] == eos for c in s["order"][s["walked"]:]):
            out.add("eos_behind")
        if s["finished"]:
            out.add("eos_recorded")
        if 0 < len(s["rows"]) < n and i + 1 < len(steps):
            out.add("dead_row")
        parents = [p for p, _, _ in s["rows"]]
        if any(p != k for k, p in enumerate(parents)):
            out.add("parent_moves")
        if len(set(parents)) < len(parents):
            out.add("two_children")
    return out


def gaps(item):
    """(the smallest of conditions 1 - 3, min |d|, the largest |logit|)"""
    infos = [inf for s in item["steps"] for inf in s["info"]]
    g = min([s["sort_gap"] for s in item["steps"]] + [inf["tail_gap"] for inf in infos] + [item["runner_gap"]])
    d = [abs(inf["d"]) for inf in infos if inf["free"]]
    return g, (min(d) if d else float("inf")), max(inf["max_logit"] for inf in infos)


NAMES = ("a", "b", "wide")


def main():
    names = sys.argv[1:] or list(NAMES)
    if set(names) - set(NAMES):
        raise SystemExit(f"unknown model among {names}: the tool knows {list(NAMES)}")
    for name in names:
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
            c, sd, feats, prompts = json.loads(str(g["config"])), golden_state_dict(g), g["features"], torch.from_numpy(g["prompt"])
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")) as g:
            layout, full, sot = json.loads(str(g["layout"])), int(g["max_new"]), int(g["sot_index"])
        m64, m32 = WhisperTorch(sd, c, torch.float64), WhisperTorch(sd, c, torch.float32)
        eos = layout["eos"]
        cases, have = [], set()
        for n, C, max_new in ((n, C, full if v is None else v) for n, C, tries in CONFIGS for v in tries):
            if max_new != full and any(k["n"] == n and k["C"] == C for k in cases) and (n, C, (max_new,)) not in CONFIGS:
                continue                                # a shorter max_new is the way out only where the longer one gave nothing
            kept = 0
            for seed in range(MAX_SEEDS):
                if kept and not (set(NEEDS) - have):
                    break
                if kept >= 3:
                    break
                x, prompt = torch.from_numpy(draw(seed, feats)), prompts[seed % 3:seed % 3 + 1]
                r = m64.decode_beam(x, prompt, max_new, layout, n, C, sot)
                item = r["items"][0]
                gap, d, big = gaps(item)
                if gap < 1e-3 * big or d < 1e-2:
                    continue
                greedy = m64.decode(x, prompt, max_new, layout, sot)["tokens"][0]
                cov = covers(item, n, eos, greedy)
                if kept and not (cov - have):
                    continue
                if not np.array_equal(m32.decode_beam(x, prompt, max_new, layout, n, C, sot)["tokens"], r["tokens"]):
                    continue
                kept += 1
                have |= cov
                cases.append(dict(seed=seed, n=n, C=C, max_new=max_new, tokens=r["tokens"][0], length=int(r["lengths"][0]),
                                  sum_logprob=float(r["sum_logprob"][0]), no_speech_prob=float(r["no_speech_prob"][0]), ended_by=item["ended_by"],
                                  differs="differs" in cov, covers=sorted(cov), gap=gap / big, d=d, big=big))
                print(name, f"n={n} C={C} max_new={max_new} seed={seed} length={cases[-1]['length']} {item['ended_by']} gap={gap / big:.1e} "
                      f"|d|={d:.2e} {sorted(cov)}", flush=True)
            if not kept:
                print(name, f"no seed below {MAX_SEEDS} met the conditions at n={n} C={C} max_new={max_new}", flush=True)
        for n, C, _ in CONFIGS:
            if not any(k["n"] == n and k["C"] == C for k in cases):
                raise SystemExit(f"model {name}: no case at n={n} C={C}")
        if set(NEEDS) - have:
            raise SystemExit(f"model {name}: not covered: {sorted(set(NEEDS) - have)}")
        tokens = np.full((len(cases), full), eos, dtype=np.int64)
        for i, k in enumerate(cases):
            tokens[i, :k["max_new"]] = k["tokens"]
        ds = [k["d"] for k in cases if np.isfinite(k["d"])]
        out = dict(seeds=np.asarray([k["seed"] for k in cases], dtype=np.int64), n=np.asarray([k["n"] for k in cases], dtype=np.int64),
                   C=np.asarray([k["C"] for k in cases], dtype=np.int64), max_new=np.asarray([k["max_new"] for k in cases], dtype=np.int64),
                   tokens=tokens, lengths=np.asarray([k["length"] for k in cases], dtype=np.int64),
                   sum_logprob=np.asarray([k["sum_logprob"] for k in cases]), no_speech_prob=np.asarray([k["no_speech_prob"] for k in cases]),
                   ended_by=np.asarray([k["ended_by"] for k in cases]), differs_from_greedy=np.asarray([k["differs"] for k in cases]),
                   covers=json.dumps([k["covers"] for k in cases]), min_gap=np.float64(min(k["gap"] for k in cases)),
                   min_abs_d=np.float64(min(ds) if ds else np.inf), max_logit=np.float64(max(k["big"] for k in cases)))
        path = os.path.join(ROOT, "tests", "golden", f"whisper_beam_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes", len(cases), "cases")


if __name__ == "__main__":
    main()
