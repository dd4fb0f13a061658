#!/usr/bin/env python3
"""Recogniser benchmark: 16 kHz waveform -> CTC tokens at HuBERT-base size with V = 32, and the edit distance.

    python bench_asr.py [--runs 10] [--warmup 3] [--quick] [--json PATH]

  wav -> tokens   `HubertForCTC.transcribe_ids` (encoder, CTC head, greedy collapse, nothing read back) at B = 1 x 10 s and at B = 8
                  ragged, 2 to 10 s, timed with device events; beside it the encoder alone and head + collapse alone on the encoder's
                  output, whose share of the sum is reported.
  eager leg       the same GPU through torch: tools/hubert_torch.py in fp32, `F.linear`, `argmax`, then per item `unique_consecutive`
                  and the blank dropped (each item's result has its own size, so this leg synchronises with the host once per item).
  edit distance   `us_edit_distance` for 256 pairs of 100 to 200 tokens and for one pair of 4096 x 4096, with device events, beside the
                  numpy yardstick (tools/ctc_numpy.py) on the host with a host clock.
The legs run interleaved, run by run, after the warm-up; median [min, max].  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_numpy as Y  # noqa: E402
from hubert_torch import base_config, frames, hubert_forward_torch, synthetic_hubert_state_dict  # noqa: E402

from unitspeech_amd import asr  # noqa: E402

V = 32
SHAPES = {
    "B1x10s": [160000],
    "B8x2-10s_ragged": [160000, 32000, 96000, 143999, 64000, 120000, 48123, 80000],
}
QUICK = {"B1x1s": [16000], "B3x1s_ragged": [16000, 4000, 9999]}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def transcribe_case(name, lens, model, sd_dev, cfg, head_w, head_b, runs, warmup, dev):
    g = torch.Generator().manual_seed(len(lens))
    wav = (0.3 * torch.randn(len(lens), max(lens), generator=g)).to(dev)
    lengths = lens if len(lens) > 1 else None
    nfr = [frames(cfg, n) for n in lens]
    fr = torch.tensor(nfr, dtype=torch.int64, device=dev)
    feats = model.encoder(wav, lengths)
    box = {}

    def hip():
        box["hip"] = model.transcribe_ids(wav, lengths)

    def encoder():
        model.encoder(wav, lengths)

    def head():
        model.lm_head.decode(feats, fr, model.pad_token_id)

    def eager():
        ids = F.linear(hubert_forward_torch(sd_dev, cfg, wav, lengths, torch.float32)[-1], head_w, head_b).argmax(-1)
        out = []
        for b, n in enumerate(nfr):
            u = torch.unique_consecutive(ids[b, :n])
            out.append(u[u != model.pad_token_id])
        box["eager"] = out

    legs = dict(hip=hip, encoder=encoder, head_collapse=head, eager=eager)
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            ts[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ts.items()}
    tokens, n = box["hip"]
    differ = sum(int(not torch.equal(tokens[b, :int(n[b])], box["eager"][b])) for b in range(len(lens)))
    row = dict(shape=name, B=len(lens), samples=max(lens), frames=max(nfr), tokens=int(n.sum()), **{k: stats(v) for k, v in ts.items()})
    row["head_collapse_share"] = round(med["head_collapse"] / (med["encoder"] + med["head_collapse"]), 4)
    row["speedup_vs_eager"] = round(med["eager"] / med["hip"], 2)
    row["items_whose_tokens_differ_from_eager"] = differ
    print(f"{name:16s} wav->tokens {med['hip']:8.3f} ms  = encoder {med['encoder']:.3f} + head and collapse {med['head_collapse']:.3f} "
          f"({100 * row['head_collapse_share']:.2f} %)   eager {med['eager']:8.3f} ms  x{row['speedup_vs_eager']:.2f}   "
          f"{row['tokens']} tokens, {differ} items differ from eager", flush=True)
    return row


def distance_case(name, pairs, runs, warmup, dev):
    Lh, Lr = max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs)
    hyp, ref = np.zeros((len(pairs), Lh), dtype=np.int64), np.zeros((len(pairs), Lr), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        hyp[p, :len(a)], ref[p, :len(b)] = a, b
    hyp, ref = torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev)
    nh = torch.tensor([len(a) for a, _ in pairs], dtype=torch.int64, device=dev)
    nr = torch.tensor([len(b) for _, b in pairs], dtype=torch.int64, device=dev)
    box = {}

    def hip():
        box["d"] = asr.edit_distance(hyp, ref, nh, nr)

    def host():
        t0 = time.perf_counter()
        box["want"] = [Y.edit_distance(a, b) for a, b in pairs]
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(warmup):
        hip()
    host()
    th, tn = [], []
    for _ in range(runs):
        th.append(timed(hip))
        tn.append(host())
    assert box["d"].tolist() == box["want"], "the device distances differ from the yardstick's"
    cells = sum(len(a) * len(b) for a, b in pairs)
    row = dict(case=name, pairs=len(pairs), cells=cells, hip=stats(th), numpy=stats(tn),
               speedup_vs_numpy=round(statistics.median(tn) / statistics.median(th), 1),
               gcells_per_s=round(cells / (statistics.median(th) * 1e-3) / 1e9, 3))
    print(f"edit distance {name:12s} hip {row['hip']['median_ms']:8.4f} ms ({row['gcells_per_s']:.2f} Gcell/s)   numpy "
          f"{row['numpy']['median_ms']:8.2f} ms  x{row['speedup_vs_numpy']:.1f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes: a functional check, not a measurement")
    ap.add_argument("--json", type=str, default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the recogniser has no CPU fallback")
    dev = torch.device("cuda", 0)
    cfg = base_config()
    sd = synthetic_hubert_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(1)
    head_w, head_b = torch.randn(V, cfg["hidden_size"], generator=g), 0.1 * torch.randn(V, generator=g)
    model = asr.HubertForCTC.base(vocab_size=V, pad_token_id=0)
    model.load_state_dict(dict({"hubert." + k: v for k, v in sd.items()}, **{"lm_head.weight": head_w, "lm_head.bias": head_b}))
    model = model.to(dev).eval()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    runs = max(a.runs, 1)
    rows = [transcribe_case(name, lens, model, sd_dev, cfg, head_w.to(dev), head_b.to(dev), runs, a.warmup, dev)
            for name, lens in (QUICK if a.quick else SHAPES).items()]
    r = np.random.Generator(np.random.Philox(key=5))

    def noisy_pair(n):
        x = r.integers(0, 30, size=n)
        y = x.copy()
        flip = r.random(n) < 0.1
        y[flip] = r.integers(0, 30, size=int(flip.sum()))
        return x, y[r.random(n) > 0.05]

    many = [noisy_pair(int(r.integers(100, 201))) for _ in range(32 if a.quick else 256)]
    big = [noisy_pair(512 if a.quick else 4096)]
    dist = [distance_case(f"{len(many)}x100-200", many, runs, a.warmup, dev), distance_case(f"1x{len(big[0][0])}", big, runs, a.warmup, dev)]
    out = {"bench": "asr_hubert_base_ctc", "V": V, "runs": a.runs, "warmup": a.warmup, "quick": a.quick,
           "device": torch.cuda.get_device_name(0), "rows": rows, "edit_distance": dist}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
