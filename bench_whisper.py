#!/usr/bin/env python3
"""Whisper benchmark at whisper-medium's geometry (d 1024, 24 + 24 layers, 16 heads, V 51,865, S 1500; seeded weights).

    python bench_whisper.py [--runs 5] [--warmup 2] [--quick] [--json PATH]
    python bench_whisper.py --decode [--runs 5] [--warmup 2] [--quick] [--json PATH]
    python bench_whisper.py --beam 5 [--runs 5] [--warmup 2] [--quick] [--json PATH]

  encoder       `encode` at B = 1 and 8
  decode        time per token at B = 1 and 8: greedy decoding of 65 tokens minus greedy decoding of 1 token (both hold the encoder and
                the cross keys / values), over the 64 steps between them; eos is suppressed so every item runs them all
  transcribe    the whole `transcribe_ids` at B = 8 x 30 s (log-mel, encoder, 4 prompt tokens, 128 new tokens)
  --decode      instead of the above: time per token of `decode` (the timestamp rules, `us_whisper_decode`) against `generate` (plain greedy,
                `us_whisper_generate`) at B = 1 and 8, measured the same way, and one selection step alone (`us_whisper_select`: the host's
                call and its three launches) at V tokens for B = 1, 8 and 16
  --beam N      instead of the above, at B = 1: time per step of `decode(beam_size=N)` (`us_whisper_decode_beam`, N rows in one launch group)
                against `decode` on the same build, measured the same way, beside the weight-streaming floor and the launches of a step, and
                one step of selection and bookkeeping alone (`us_whisper_beam_select`: the host's call and its four launches) as a share of
                the beam step
Two legs, alternating run by run on the same GPU after the warm-up, timed by device events; median [min, max]:
  hip           the library (unitspeech_amd.whisper.WhisperForConditionalGeneration)
  eager         the fp32 torch restatement with its key/value cache (tools/whisper_torch.py) on the device
Beside the per-token time stands the weight-streaming floor: the bytes of the decoder's weights and the token embedding over the measured
rate of a plain device copy (bytes read plus bytes written per second), and the launches of one step (1 embedding + 8 per layer + logits +
argmax).  The tokens of the two legs are compared.  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from whisper_torch import WhisperTorch  # noqa: E402
from unitspeech_amd.whisper import (MEDIUM, WhisperForConditionalGeneration, log_mel_spectrogram, select_beams, select_tokens,  # noqa: E402
                                    synthetic_whisper_state_dict)

QUICK = dict(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
             decoder_ffn_dim=128, num_mel_bins=80, max_source_positions=1500, max_target_positions=448, vocab_size=203)
STEPS, TRANSCRIBE_NEW = 64, 128


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def alternate(legs, runs, warmup):
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            ts[k].append(timed(fn))
    return ts


def features(B, c, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 * torch.randn(B, c["num_mel_bins"], 2 * c["max_source_positions"], generator=g)).to(dev)


def decoder_bytes(c):
    H, I, L = c["d_model"], c["decoder_ffn_dim"], c["decoder_layers"]
    per_layer = 8 * H * H + 7 * H + 2 * H * I + I + H + 6 * H          # two attentions, the MLP, three LayerNorms
    return 4 * (L * per_layer + c["vocab_size"] * H + 2 * H)


def copy_rate(dev):
    """bytes read plus bytes written per second of a device copy of 1 GiB"""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    ms = statistics.median(timed(lambda: b.copy_(a)) for _ in range(10))
    return 2 * a.numel() * 4 / (ms * 1e-3)


def decode_legs(a, c, dev):
    """`decode` against `generate`, per token, and the selection step alone"""
    V = c["vocab_size"]
    eos, nt = (50257, 50363) if V == 51865 else (V - 25, V - 13)
    hip = WhisperForConditionalGeneration(**c, eos_token_id=eos)
    hip.load_state_dict(synthetic_whisper_state_dict(c, 0))
    hip = hip.to(dev).eval()
    rows, box = [], {}
    for B in (1, 8):
        x = features(B, c, dev, B)
        legs = {"generate": lambda n: box.__setitem__("g", hip.generate(x, [1, 2, 3, nt], n, suppress_tokens=[eos])[0]),
                "decode": lambda n: box.__setitem__("d", hip.decode(x, [1, 2, 3], no_timestamps_id=nt, no_speech_id=nt - 1, max_new_tokens=n,
                                                                   suppress_tokens=[eos]).tokens)}
        ts = alternate({f"{k}_{n}": (lambda k=k, n=n: legs[k](n)) for n in (1, STEPS + 1) for k in legs}, a.runs, a.warmup)
        per = {k: [(n - o) / STEPS for n, o in zip(ts[f"{k}_{STEPS + 1}"], ts[f"{k}_1"])] for k in legs}
        stamps = int((box["d"] > nt).sum())
        rows.append(dict(stage="decode_per_token", B=B, steps=STEPS, **{k: stats(v) for k, v in per.items()},
                         first_token={k: stats(ts[f"{k}_1"]) for k in legs}, timestamps_emitted=stamps, tokens=int(box["d"].numel())))
        print(f"per token B={B}: decode {statistics.median(per['decode']):.4f} ms  generate {statistics.median(per['generate']):.4f} ms  "
              f"({stamps} of {box['d'].numel()} tokens are timestamps)", flush=True)
    g = torch.Generator().manual_seed(7)
    reps = 50
    for B in (1, 8, 16):
        lg = (3 * torch.randn(B, V, generator=g)).to(dev)
        hist = [(2, nt + 3, 5, nt + 3, 0)] * B

        def sel():
            for _ in range(reps):
                select_tokens(lg, hist, eos_token_id=eos, no_timestamps_id=nt)

        ts = alternate(dict(select=sel), a.runs, a.warmup)
        rows.append(dict(stage="select_call", B=B, V=V, calls=reps, **{k: stats([t / reps for t in v]) for k, v in ts.items()}))
        print(f"select B={B} V={V}: {statistics.median(ts['select']) / reps * 1e3:.1f} us per call (host call + 3 launches)", flush=True)
    return rows


def beam_legs(a, c, dev):
    """`decode(beam_size=n)` against `decode` per step at B = 1, and the beam's selection and bookkeeping alone"""
    V, n = c["vocab_size"], a.beam
    eos, nt = (50257, 50363) if V == 51865 else (V - 25, V - 13)
    hip = WhisperForConditionalGeneration(**c, eos_token_id=eos)
    hip.load_state_dict(synthetic_whisper_state_dict(c, 0))
    hip = hip.to(dev).eval()
    rate = copy_rate(dev)
    floor_ms = decoder_bytes(c) / rate * 1e3
    x, box = features(1, c, dev, 1), {}

    def run(k, steps):                                  # eos suppressed: no entry finishes, every row stays live, every step runs
        box[k] = hip.decode(x, [1, 2, 3], no_timestamps_id=nt, no_speech_id=nt - 1, max_new_tokens=steps, suppress_tokens=[eos],
                            beam_size=n if k == "beam" else None)

    ts = alternate({f"{k}_{s}": (lambda k=k, s=s: run(k, s)) for s in (1, STEPS + 1) for k in ("greedy", "beam")}, a.runs, a.warmup)
    per = {k: [(m - o) / STEPS for m, o in zip(ts[f"{k}_{STEPS + 1}"], ts[f"{k}_1"])] for k in ("greedy", "beam")}
    g = torch.Generator().manual_seed(7)
    lg, reps = (3 * torch.randn(n, V, generator=g)).to(dev), 50
    hist, scores = [(2, nt + 3, 5, nt + 3, 0)] * n, [-0.5 * j for j in range(n)]

    def sel():
        for _ in range(reps):
            select_beams(lg, hist, scores, n, eos_token_id=eos, no_timestamps_id=nt)

    sel_ms = [t / reps for t in alternate(dict(select=sel), a.runs, a.warmup)["select"]]
    beam_ms, greedy_ms, s_ms = (statistics.median(v) for v in (per["beam"], per["greedy"], sel_ms))
    launches = dict(greedy=1 + 8 * c["decoder_layers"] + 1 + 2, beam=1 + 8 * c["decoder_layers"] + 1 + 3)
    row = dict(stage="beam_per_step", B=1, beam_size=n, steps=STEPS, beam=stats(per["beam"]), greedy=stats(per["greedy"]),
               ratio=round(beam_ms / greedy_ms, 3), floor_ms=round(floor_ms, 4), launches_per_step=launches, select_call=stats(sel_ms),
               select_share=round(s_ms / beam_ms, 4), beam_length=int(box["beam"].lengths[0]), greedy_length=int(box["greedy"].lengths[0]))
    print(f"per step B=1: decode(beam_size={n}) {beam_ms:.4f} ms  decode {greedy_ms:.4f} ms  ratio {beam_ms / greedy_ms:.2f}  floor {floor_ms:.4f} ms  "
          f"launches {launches['beam']} / {launches['greedy']}  selection + bookkeeping {s_ms * 1e3:.1f} us per call ({100 * s_ms / beam_ms:.1f} % of a step, "
          f"the host's call and an init launch included)", flush=True)
    return [row], rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a tiny geometry: a functional check, not a measurement")
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--decode", action="store_true", help="only `decode` against `generate` and the selection step alone")
    ap.add_argument("--beam", type=int, default=None, metavar="N", help="only `decode(beam_size=N)` against `decode` at B = 1")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the recogniser has no CPU fallback")
    dev = torch.device("cuda", 0)
    c = dict(QUICK if a.quick else MEDIUM)
    if a.beam is not None:
        rows, rate = beam_legs(a, c, dev)
        out = {"bench": "whisper_beam", "geometry": "quick" if a.quick else "whisper-medium", "config": c, "runs": a.runs, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0), "copy_rate_GBps": round(rate / 1e9, 1), "decoder_weight_bytes": decoder_bytes(c), "rows": rows}
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        print(json.dumps(out))
        return
    if a.decode:
        out = {"bench": "whisper_decode", "geometry": "quick" if a.quick else "whisper-medium", "config": c, "runs": a.runs, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0), "rows": decode_legs(a, c, dev)}
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        print(json.dumps(out))
        return
    V, eos = c["vocab_size"], c["vocab_size"] - 1
    sd = synthetic_whisper_state_dict(c, 0)
    hip = WhisperForConditionalGeneration(**c, eos_token_id=eos)
    hip.load_state_dict(sd)
    hip = hip.to(dev).eval()
    eager = WhisperTorch(sd, c, torch.float32, dev)
    del sd
    prompt = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    mask = torch.zeros(V, dtype=torch.bool)
    mask[eos] = True
    rate = copy_rate(dev)
    floor_ms = decoder_bytes(c) / rate * 1e3
    launches = 1 + 8 * c["decoder_layers"] + 2
    rows, box = [], {}
    for B in (1, 8):
        x = features(B, c, dev, B)
        pr = prompt[None].expand(B, -1).contiguous()
        ts = alternate(dict(hip=lambda: hip.encode(x), eager=lambda: eager.encode(x)), a.runs, a.warmup)
        rows.append(dict(stage="encoder", B=B, **{k: stats(v) for k, v in ts.items()}))
        print(f"encoder B={B}: hip {statistics.median(ts['hip']):.3f} ms  eager {statistics.median(ts['eager']):.3f} ms", flush=True)

        def gen_hip(n):
            box["hip"] = hip.generate(x, pr, n, suppress_tokens=[eos])[0]

        def gen_eager(n):
            box["eager"] = eager.generate(x, pr, n, eos, suppress=mask, stop_early=False)[0]

        ts = alternate({"hip_1": lambda: gen_hip(1), "eager_1": lambda: gen_eager(1), "hip_n": lambda: gen_hip(STEPS + 1),
                        "eager_n": lambda: gen_eager(STEPS + 1)}, a.runs, a.warmup)
        per = {k: [(n - o) / STEPS for n, o in zip(ts[k + "_n"], ts[k + "_1"])] for k in ("hip", "eager")}
        same = int((box["hip"] == box["eager"]).sum())
        rows.append(dict(stage="decode_per_token", B=B, steps=STEPS, **{k: stats(v) for k, v in per.items()},
                         first_token={k: stats(ts[k + "_1"]) for k in ("hip", "eager")}, floor_ms=round(floor_ms, 4),
                         launches_per_step=launches, tokens_equal=same, tokens=int(box["hip"].numel())))
        print(f"decode B={B}: hip {statistics.median(per['hip']):.4f} ms/token  eager {statistics.median(per['eager']):.4f} ms/token  "
              f"floor {floor_ms:.4f} ms  ({launches} launches per step; {same} of {box['hip'].numel()} tokens equal)", flush=True)
    B = 8
    g = torch.Generator().manual_seed(99)
    wav = (0.1 * torch.randn(B, 480000, generator=g)).to(dev)
    hip.prompt_ids, hip.suppress_tokens = [1, 2, 3, 4], [eos]

    def tr_hip():
        box["hip"] = hip.transcribe_ids(wav, None, max_new_tokens=TRANSCRIBE_NEW)[0]

    def tr_eager():
        feats = log_mel_spectrogram(wav, None, c["num_mel_bins"])
        box["eager"] = eager.generate(feats, prompt[None].expand(B, -1), TRANSCRIBE_NEW, eos, suppress=mask, stop_early=False)[0]

    ts = alternate(dict(hip=tr_hip, eager=tr_eager), max(a.runs // 2, 1), 1)
    same = int((box["hip"] == box["eager"]).sum())
    rows.append(dict(stage="transcribe_ids", B=B, seconds=30, new_tokens=TRANSCRIBE_NEW, **{k: stats(v) for k, v in ts.items()}, tokens_equal=same,
                     tokens=int(box["hip"].numel())))
    print(f"transcribe B={B}: hip {statistics.median(ts['hip']):.2f} ms  eager {statistics.median(ts['eager']):.2f} ms  "
          f"({same} of {box['hip'].numel()} tokens equal)", flush=True)
    out = {"bench": "whisper", "geometry": "quick" if a.quick else "whisper-medium", "config": c, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "copy_rate_GBps": round(rate / 1e9, 1), "decoder_weight_bytes": decoder_bytes(c), "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
