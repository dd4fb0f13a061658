#!/usr/bin/env python3
"""Writes tests/golden/whisper_decode_{a,b}.npz: greedy decoding under the timestamp rules of the two tiny models of
tests/golden/whisper_{a,b}.npz (their weights, features and prompts; nothing of those is stored again), from the installed
`transformers.WhisperForConditionalGeneration` in fp64 on the CPU (the whole prefix again at every step, no cache) and transformers'
SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and WhisperTimeStampLogitsProcessor, then argmax and log_softmax.

    python tools/make_goldens_whisper_decode.py

The token layout (eos, no_timestamps, the cap of the first timestamp, the suppressed ids) is searched, LAYOUTS first, and a file is written
only when all of these hold:
 1. over all free decisions (both sides finite, item not done) |d| >= 1e-2, with d = logsumexp(surviving timestamps) - max(surviving text);
 2. the top-1 / top-2 gap of the surviving logits is at least 1e-3 of the largest |logit| at every step (the rule of whisper_{a,b}.npz);
 3. both outcomes of a free decision occur at least 5 times each;
 4. some item returns to a timestamp after text by a free decision;
 5. two items have different timestamp patterns;
 6. two items stop at different steps and one never stops.
Every step is also computed by tools/whisper_decode_numpy.py and must give transformers' token and log-probability (1e-12).

Each file holds `layout` (json: eos, no_timestamps, max_initial_timestamp_index, no_speech, suppress, begin_suppress), `sot_index`, `max_new`,
`tokens` [3][max_new] (eos at and after an item's end), `lengths` [3], `logprobs` [3][max_new] fp64 (0 after the end), `sum_logprob` [3],
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

LAYOUTS = {"a": dict(no_timestamps=87, eos=35, max_initial_timestamp_index=2), "b": dict(no_timestamps=190, eos=178, max_initial_timestamp_index=2)}


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
    return c, model.double(), x, prompt


def run(model, c, x, prompt, layout):
    """-> (the file's arrays, None) or (None, why not)"""
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
    B = x.shape[0]
    tokens, lps = np.full((B, max_new), eos, dtype=np.int64), np.zeros((B, max_new))
    d, decided, gap = np.full((B, max_new), np.nan), np.zeros((B, max_new), dtype=np.int8), np.full((B, max_new), np.inf)
    lengths, nsp, big = np.full(B, max_new, dtype=np.int64), np.zeros(B), 0.0
    with torch.no_grad():
        for b in range(B):
            seq = prompt[b:b + 1].clone()
            for i in range(max_new):
                lg = model(input_features=x[b:b + 1], decoder_input_ids=seq, use_cache=False).logits[0]
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
    if len(set(stops)) < 2 or len(stops) == B:
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


def main():
    for name in ("a", "b"):
        c, model, x, prompt = load(name)
        for layout in candidates(name, c["vocab_size"]):
            out, msg = run(model, c, x, prompt, layout)
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
