#!/usr/bin/env python3
"""Writes tests/golden/whisper_decode_{a,b,long,wide}.npz: greedy decoding under the timestamp rules of the tiny models of
tests/golden/whisper_{a,b,long,wide}.npz (their weights, features and prompts; nothing of those is stored again), from the installed
`transformers.WhisperForConditionalGeneration` in fp64 on the CPU (the whole prefix again at every step, no cache) and transformers'
SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and WhisperTimeStampLogitsProcessor, then argmax and log_softmax.

    python tools/make_goldens_whisper_decode.py [name ...]          # no name: all of them

The token layout (eos, no_timestamps, the cap of the first timestamp, the suppressed ids) is searched, LAYOUTS first, and a file is written
only when all of these hold:
 1. over all free decisions (both sides finite, item not done) |d| >= 1e-2, with d = logsumexp(surviving timestamps) - max(surviving text);
 2. the top-1 / top-2 gap of the surviving logits is at least 1e-3 of the largest |logit| at every step (the rule of whisper_{a,b}.npz);
 3. both outcomes of a free decision occur at least 5 times each;
 4. some item returns to a timestamp after text by a free decision;
 5. two items have different timestamp patterns;
 6. two items stop at different steps and one never stops (`long`, which has two items: their lengths differ and one of them runs past
    step 70, so that the rules are applied over a cache of more than 64 positions).
A layout is given up at the first step that misses condition 1 or 2.
Every step is also computed by tools/whisper_decode_numpy.py and must give transformers' token and log-probability (1e-12).

Each file holds `layout` (json: eos, no_timestamps, max_initial_timestamp_index, no_speech, suppress, begin_suppress), `sot_index`, `max_new`,
`tokens` [items][max_new] (eos at and after an item's end), `lengths` [3], `logprobs` [3][max_new] fp64 (0 after the end), `sum_logprob` [3],
`no_speech_prob` [3], `d` [3][max_new] (nan where the decision is not free), `decided` [3][max_new] (1: the timestamps won), `gap`
[3][max_new], `min_abs_d`, `min_gap` (relative) and `max_logit`.
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_decode_numpy as rules  # noqa: E402
from whisper_torch import golden_state_dict  # noqa: E402

LAYOUTS = {"a": dict(no_timestamps=87, eos=35, max_initial_timestamp_index=2), "b": dict(no_timestamps=190, eos=178, max_initial_timestamp_index=2),
           "long": dict(no_timestamps=60, eos=40, max_initial_timestamp_index=2),
           "wide": dict(no_timestamps=520, eos=252, max_initial_timestamp_index=2, also_suppress=(526, 529))}
LONG_PAST = 70


def load(name):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
        c, sd = json.loads(str(g["config"])), golden_state_dict(g)
        x, prompt = torch.from_numpy(g["features"]).double(), torch.from_numpy(g["prompt"])
    cfg = WhisperConfig(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0,
                        activation_function="gelu", scale_embedding=False, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                        decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None, **c)
    model = WhisperForConditionalGeneration(cfg).eval()
    sd = dict(sd)
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd)
    model = model.double()
    with torch.no_grad():                 # the encoder once per item, not once per step: the same numbers
        enc = [model.model.encoder(x[b:b + 1]).last_hidden_state for b in range(x.shape[0])]
    return c, model, enc, prompt


def run(model, c, enc, prompt, layout, name=None):
    """-> (the file's arrays, None) or (None, why not)"""
    from transformers.modeling_outputs import BaseModelOutput
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    V, P = c["vocab_size"], prompt.shape[1]
    max_new = c["max_target_positions"] - P
    eos, cap = layout["eos"], layout["max_initial_timestamp_index"]
    gen = SimpleNamespace(no_timestamps_token_id=layout["no_timestamps"], eos_token_id=eos, bos_token_id=eos,
                          max_initial_timestamp_index=cap if cap >= 0 else None, _detect_timestamp_from_logprob=True)
    procs = [SuppressTokensLogitsProcessor(layout["suppress"]), SuppressTokensAtBeginLogitsProcessor(layout["begin_suppress"], P),
             WhisperTimeStampLogitsProcessor(gen, begin_index=P)]
    sup, beg = rules.masks(layout, V)
    B = len(enc)
    tokens, lps = np.full((B, max_new), eos, dtype=np.int64), np.zeros((B, max_new))
    d, decided, gap = np.full((B, max_new), np.nan), np.zeros((B, max_new), dtype=np.int8), np.full((B, max_new), np.inf)
    lengths, nsp, big = np.full(B, max_new, dtype=np.int64), np.zeros(B), 0.0
    with torch.no_grad():
        for b in range(B):
            seq = prompt[b:b + 1].clone()
            for i in range(max_new):
                lg = model(encoder_outputs=BaseModelOutput(last_hidden_state=enc[b]), decoder_input_ids=seq, use_cache=False).logits[0]
                if i == 0:
                    nsp[b] = float(torch.softmax(lg[0], -1)[layout["no_speech"]])
                row = lg[-1]
                big = max(big, float(row.abs().max()))
                scores = row[None]
                for p in procs:
                    scores = p(seq, scores)
                tok = int(scores[0].argmax())
                lp = float(torch.log_softmax(scores[0], -1)[tok])
                r = rules.select(row.numpy(), seq[0, P:].tolist(), layout, sup, beg)
                assert r["token"] == tok and abs(r["logprob"] - lp) <= 1e-12, (b, i, r, tok, lp)
                tokens[b, i], lps[b, i], d[b, i], decided[b, i], gap[b, i] = tok, lp, r["d"], r["decided"], r["gap"]
                if (r["free"] and abs(r["d"]) < 1e-2) or r["gap"] < 1e-3 * big:          # conditions 1 and 2: `big` only grows
                    return None, f"item {b} step {i}: |d| {abs(r['d']):.1e}, gap {r['gap'] / big:.1e}"
                seq = torch.cat([seq, torch.tensor([[tok]])], dim=1)
                if tok == eos:
                    lengths[b] = i
                    break
    tb = layout["no_timestamps"] + 1
    free = np.isfinite(d)
    if not free.any() or float(np.abs(d[free]).min()) < 1e-2:
        return None, f"min |d| {float(np.abs(d[free]).min()) if free.any() else None}"
    if float(gap.min()) < 1e-3 * big:
        return None, f"gap {float(gap.min()) / big:.1e}"
    wins, keeps = int((free & (decided == 1)).sum()), int((free & (decided == 0)).sum())
    if wins < 5 or keeps < 5:
        return None, f"free decisions: {wins} timestamp, {keeps} text"
    back = any(free[b, i] and decided[b, i] and i > 0 and tokens[b, i - 1] < tb for b in range(B) for i in range(int(lengths[b])))
    if not back:
        return None, "no free return to a timestamp after text"
    patterns = {tuple((tokens[b, :lengths[b]] >= tb).tolist()) for b in range(B)}
    if len(patterns) < 2:
        return None, "one timestamp pattern"
    stops = sorted(int(v) for v in lengths if v < max_new)
    if (len(set(lengths.tolist())) < 2 or int(lengths.max()) <= LONG_PAST) if name == "long" else (len(set(stops)) < 2 or len(stops) == B):
        return None, f"stops {lengths.tolist()}"
    out = dict(layout=json.dumps(layout), sot_index=np.int64(0), max_new=np.int64(max_new), tokens=tokens, lengths=lengths, logprobs=lps,
               sum_logprob=lps.sum(1), no_speech_prob=nsp, d=d, decided=decided, gap=gap, min_abs_d=np.float64(np.abs(d[free]).min()),
               min_gap=np.float64(gap.min() / big), max_logit=np.float64(big))
    return out, (f"free decisions {int(free.sum())}, timestamp wins {wins}, min |d| {float(np.abs(d[free]).min()):.3f}, "
                 f"min gap {float(gap.min()) / big:.1e}, lengths {lengths.tolist()}, max |logit| {big:.2f}")


def candidates(name, V):
    """LAYOUTS[name] first, then its neighbours: one more suppressed text token (none, 3, 4, ...), every eos below no_timestamps, and only
    then another cap or another no_timestamps (5 to 15 timestamp tokens)"""
    first = LAYOUTS[name]
    seen = set()
    if name in SPREAD:
        yield from spread(first, V)
        return
    for nt in [first["no_timestamps"]] + list(range(V - 7, V - 17, -1)):
        for cap in (first["max_initial_timestamp_index"], -1):
            for extra in [None] + list(range(3, nt - 1)):
                for eos in [first["eos"]] + list(range(3, nt - 2)):
                    if eos == extra or (nt, cap, extra, eos) in seen:
                        continue
                    seen.add((nt, cap, extra, eos))
                    # what a real vocabulary has there: no-speech right below no_timestamps and suppressed, as the special token after eos
                    # is; eos and a text token suppressed at the first position
                    yield dict(eos=eos, no_timestamps=nt, max_initial_timestamp_index=cap, no_speech=nt - 1,
                               suppress=[eos + 1, nt - 1] + ([extra] if extra is not None else []), begin_suppress=[7, eos])


SPREAD = ("long", "wide")


def spread(first, V):
    """The search of the models with more steps or more tokens than a and b: a run of many steps uses up a handful of timestamp tokens long
    before it ends (they only grow), and the timestamps then never win again.  So the number of timestamp tokens is searched in front of
    everything else, from the first layout's down to a third of the vocabulary; then eos, then one more suppressed text token.
    whisper_wide's two largest timestamp logits are those of two of its last tokens, 526 and 529, at every step: chosen at the first free
    decisions, they leave no timestamp for the rest of the run, whatever the other fields are.  Its first layout suppresses them
    (`also_suppress`), as a real vocabulary's list suppresses single tokens."""
    for extra in [tuple(first.get("also_suppress", ()))] + [(t,) for t in range(3, 12)]:
        for eos in [first["eos"]] + list(range(3, V // 3)):
            for cap in (first["max_initial_timestamp_index"], -1):
                for nt in [first["no_timestamps"]] + list(range(V - 7, V // 3, -max(1, V // 50))):
                    if eos in extra or eos >= nt - 2:
                        continue
                    yield dict(eos=eos, no_timestamps=nt, max_initial_timestamp_index=cap, no_speech=nt - 1,
                               suppress=[eos + 1, nt - 1] + list(extra), begin_suppress=[7, eos])


def main():
    names = sys.argv[1:] or list(LAYOUTS)
    if set(names) - set(LAYOUTS):
        raise SystemExit(f"unknown model among {names}: the tool knows {list(LAYOUTS)}")
    for name in names:
        c, model, enc, prompt = load(name)
        for layout in candidates(name, c["vocab_size"]):
            out, msg = run(model, c, enc, prompt, layout, name)
            print(name, {k: layout[k] for k in ("no_timestamps", "eos", "max_initial_timestamp_index", "suppress")}, msg, flush=True)
            if out is not None:
                break
        else:
            raise SystemExit(f"no layout met the conditions for model {name}")
        path = os.path.join(ROOT, "tests", "golden", f"whisper_decode_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
