#!/usr/bin/env python3
"""Active-speech-level normalisation of a directory of wavs on the HIP library: what the reference's `sv56.py` does with the ITU `sv56demo`
binary, one process per file, done here on the device in length-sorted ragged batches (`unitspeech_amd.level`, ITU-T P.56 method B).

    python normalize_level.py --in_dir IN --out_dir OUT [--ndb -26] [--batch 16]
    python normalize_level.py --synthetic 4 --batch 3 --out_dir OUT

Every `*.wav` of IN is read with scipy.io.wavfile (several channels are averaged), brought to --ndb dB relative to full scale and written
to OUT under its own name as int16.  int16 files go in as they are; a float file first takes the reference's route to int16,
`(x * 32767).astype(int16)`; other integer widths are scaled to full scale and take the same route.  One batch holds files of one
sampling rate.  Per file one line: the level before, the gain, the clipped samples.  A file without measurable speech (level -100) or with
a non-finite sample (level nan) is written unchanged.

--synthetic N needs no files: N seeded int16 burst signals of different lengths at 22050 Hz (`synthetic_items`) go through the same path.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.audio import read_wav  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402

SYNTHETIC_RATE = 22050


def read_samples(path):
    """-> (int16 or float32 mono samples, sampling rate): int16 stays int16, everything else becomes float32 in units of full scale."""
    return read_wav(path, keep_int16=True)


def synthetic_items(n: int, seed: int = 0):
    """-> [(name, int16 samples, rate)]: n seeded burst signals of 0.3 to 1.2 s, all of different lengths."""
    if n < 1:
        raise ValueError("--synthetic N: N must be at least 1")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from level_numpy import burst_signal
    g = np.random.Generator(np.random.Philox(key=6000 + seed))
    out = []
    for i in range(n):
        samples = int(g.integers(int(0.3 * SYNTHETIC_RATE), int(1.2 * SYNTHETIC_RATE))) + i
        out.append((f"synthetic_{i:04d}", burst_signal(samples, SYNTHETIC_RATE, seed * 1000 + i), SYNTHETIC_RATE))
    return out


@torch.no_grad()
def normalize_items(items, ndb, max_batch, device):
    """[(name, int16 or float32 samples, rate)] -> [(int16 samples, level_db, gain, clipped)] in the order given.  A batch holds items of one
    rate and one sample type."""
    from unitspeech_amd.level import normalize_level
    out = [None] * len(items)
    for key in sorted({(r, w.dtype == np.int16) for _, w, r in items}):
        group = [i for i, (_, w, r) in enumerate(items) if (r, w.dtype == np.int16) == key]
        for batch in plan_batches([len(items[i][1]) for i in group], max_batch):
            idx = [group[j] for j in batch]
            x, n = pad_batch([items[i][1] for i in idx])
            if max(n) == 0:
                for i in idx:
                    out[i] = (np.zeros(0, dtype=np.int16), -100.0, 1.0, 0)
                continue
            y, lv = normalize_level(x.to(device), key[0], ndb, lengths=n, via_int16=True, out_int16=True)
            y = y.cpu().numpy()
            for b, (i, level, gain, clipped) in enumerate(zip(idx, lv.level_db.tolist(), lv.gain.tolist(), lv.clipped.tolist())):
                out[i] = (y[b, :n[b]].copy(), level, gain, clipped)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--in_dir", default=None, help="input wav directory")
    ap.add_argument("--out_dir", required=True, help="output wav directory")
    ap.add_argument("--ndb", type=float, default=-26.0, help="the target level in dB relative to full scale")
    ap.add_argument("--batch", type=int, default=16, metavar="K", help="most files in one batch")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded burst signals; needs no files")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP library has no CPU fallback")
    if args.synthetic:
        items = synthetic_items(args.synthetic, args.seed)
    else:
        if not args.in_dir:
            raise SystemExit("give --in_dir (a directory of wavs), or --synthetic N")
        paths = sorted(glob.glob(os.path.join(args.in_dir, "*.wav")))
        if not paths:
            raise SystemExit(f"{args.in_dir}: no wav files")
        items = [(os.path.splitext(os.path.basename(p))[0],) + read_samples(p) for p in paths]
    results = normalize_items(items, args.ndb, args.batch, torch.device(args.device))
    from scipy.io.wavfile import write
    os.makedirs(args.out_dir, exist_ok=True)
    for (name, _, rate), (y, level, gain, clipped) in zip(items, results):
        write(os.path.join(args.out_dir, name + ".wav"), rate, y)
        print(f"{name}: level {level:.2f} dB, gain {gain:.4f}, {clipped} clipped samples")
    print(f"{len(items)} files -> {args.out_dir} at {args.ndb:g} dB")


if __name__ == "__main__":
    main()
