#!/usr/bin/env python3
"""CTC training benchmark: loss + gradient, the head's backward and the forced alignment at V = 32 with character-length targets.

    python bench_ctc_loss.py [--runs 10] [--warmup 3] [--quick] [--json PATH]

  loss + grad     `asr.ctc_loss(logits, ..., reduction="sum")` and its `.backward()` (the library call twice: the loss, then the
                  gradient scaled by the incoming per-item gradient) at B = 8 ragged, 2 to 10 s of 20 ms frames, and at B = 32 x 5 s,
                  timed with device events; beside it eager `F.ctc_loss(F.log_softmax(logits, -1), ...)` forward and backward on the
                  same GPU.  The largest difference between the two gradients is reported.
  head backward   `us_ctc_head_backward` (dW, db, dX) of that gradient at H = 768; beside it the three eager products.
  alignment       `asr.forced_align` of the same targets on the log-probabilities (no eager counterpart: time only).
The legs run interleaved, run by run, after the warm-up; median [min, max].  The last line is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from unitspeech_amd import _lib, asr  # noqa: E402

V, H = 32, 768
FRAMES_PER_SECOND = 50
TOKENS_PER_FRAME = 0.25          # about 12 characters a second
SHAPES = {
    "B8x2-10s_ragged": [10.0, 2.0, 6.0, 9.0, 4.0, 7.5, 3.0, 5.0],
    "B32x5s": [5.0] * 32,
}
QUICK = {"B3x1s_ragged": [1.0, 0.3, 0.6]}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def case(name, seconds, runs, warmup, dev):
    r = np.random.Generator(np.random.Philox(key=len(seconds)))
    nfr = [int(s * FRAMES_PER_SECOND) for s in seconds]
    ntok = [max(1, int(n * TOKENS_PER_FRAME)) for n in nfr]
    B, T, L = len(nfr), max(nfr), max(ntok)
    g = torch.Generator().manual_seed(B)
    logits = (2.0 * torch.randn(B, T, V, generator=g)).to(dev)
    feats = torch.randn(B, T, H, generator=g).to(dev)
    weight = (0.05 * torch.randn(V, H, generator=g)).to(dev)
    targets = torch.from_numpy(r.integers(1, V, size=(B, L))).to(dev)
    fl, tl = torch.tensor(nfr, dtype=torch.int64, device=dev), torch.tensor(ntok, dtype=torch.int64, device=dev)
    lib = _lib.load()
    nws = int(lib.us_ctc_head_backward_workspace_bytes(B, T, V, H))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dw, db, dx = torch.empty(V, H, device=dev), torch.empty(V, device=dev), torch.empty(B, T, H, device=dev)
    live = (torch.arange(T, device=dev)[None, :] < fl[:, None])
    box = {}

    def hip_loss():
        x = logits.detach().requires_grad_(True)
        loss = asr.ctc_loss(x, targets, fl, tl, reduction="sum")
        loss.backward()
        box["hip"] = (loss.detach(), x.grad)

    def eager_loss():
        x = logits.detach().requires_grad_(True)
        loss = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), targets, fl, tl, blank=0, reduction="sum")
        loss.backward()
        box["eager"] = (loss.detach(), x.grad)

    hip_loss()
    grad = box["hip"][1].contiguous()
    lp = F.log_softmax(logits, -1)

    def hip_head():
        rc = lib.us_ctc_head_backward(grad.data_ptr(), feats.data_ptr(), fl.data_ptr(), weight.data_ptr(), B, T, V, H, dw.data_ptr(),
                                      db.data_ptr(), dx.data_ptr(), ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, None, "us_ctc_head_backward")

    def eager_head():
        g2 = grad.reshape(-1, V)
        box["eager_head"] = (g2.t() @ feats.reshape(-1, H), g2.sum(0), grad @ weight)

    def hip_align():
        box["align"] = asr.forced_align(lp, targets, fl, tl)

    legs = dict(hip_loss=hip_loss, eager_loss=eager_loss, hip_head=hip_head, eager_head=eager_head, hip_align=hip_align)
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ts = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            ts[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ts.items()}
    loss_diff = float((box["hip"][0] - box["eager"][0]).abs() / box["eager"][0].abs())
    grad_diff = float((box["hip"][1] - box["eager"][1]).abs().max())
    ew, eb, ex = box["eager_head"]
    head_diff = max(float((dw - ew).abs().max() / ew.abs().max()), float((db - eb).abs().max() / eb.abs().max()),
                    float((dx - ex * live[..., None]).abs().max() / ex.abs().max()))
    row = dict(shape=name, B=B, frames=T, tokens=L, V=V, H=H, **{k: stats(v) for k, v in ts.items()},
               loss_speedup_vs_eager=round(med["eager_loss"] / med["hip_loss"], 2),
               head_speedup_vs_eager=round(med["eager_head"] / med["hip_head"], 2),
               loss_rel_diff_vs_eager=loss_diff, grad_max_diff_vs_eager=grad_diff, head_max_rel_diff_vs_eager=head_diff,
               aligned_items=int(torch.isfinite(box["align"][1]).sum()))
    print(f"{name:16s} loss+grad hip {med['hip_loss']:8.3f} ms  eager {med['eager_loss']:8.3f} ms  x{row['loss_speedup_vs_eager']:.2f}  "
          f"(grad diff {grad_diff:.2e})   head backward hip {med['hip_head']:7.3f} ms  eager {med['eager_head']:7.3f} ms  "
          f"x{row['head_speedup_vs_eager']:.2f}   align {med['hip_align']:7.3f} ms", flush=True)
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
    rows = [case(name, seconds, max(a.runs, 1), a.warmup, dev) for name, seconds in (QUICK if a.quick else SHAPES).items()]
    out = {"bench": "ctc_loss_head_backward_align", "V": V, "H": H, "runs": a.runs, "warmup": a.warmup, "quick": a.quick,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
