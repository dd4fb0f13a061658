#!/usr/bin/env python3
"""Fit the unit codebook on the device: k-means over dense features (unitspeech_amd.units.KMeansQuantizer.fit / partial_fit).

    python fit_units.py --synthetic 20000 --n_clusters 100 --out codebook.pt
    python fit_units.py --features feats_0.pt feats_1.npy --n_clusters 1000 --out km.bin
    python fit_units.py --wav_list wavs.txt --hubert_checkpoint hubert_base.pt --hubert_layer 11 --n_clusters 1000 --out km.bin

  --features   .pt files (a tensor, or a dictionary with `dense`) or .npy files of dense features [N, D] or [B, T, D]; every file is one
               chunk of the fit, so the files together may hold more rows than one library call takes.
  --wav_list   a text file with one wav path per line: the waveforms are brought to 16 kHz on the device and go through the library's
               HuBERT (--hubert_checkpoint, --hubert_layer) in ragged batches of --wav_batch; every batch is one chunk.
  --synthetic  N rows of seeded synthetic features around --n_clusters planted centres (D = --synthetic_dim), no files.
  --minibatch  N rows per `partial_fit` call over a seeded permutation of the rows, --epochs times: the update is scikit-learn's
               `MiniBatchKMeans.partial_fit` with reassignment_ratio = 0; the batch order is this tool's own, not scikit-learn's sampler.
  --n_init     R fits from the seeds --seed .. --seed + R - 1; the one with the lowest inertia is kept.
  --out        .bin / .joblib: a joblib-saved scikit-learn KMeans (what --kmeans_checkpoint and textless read; needs scikit-learn);
               anything else: a torch file with `centers` and the fit attributes.

One line per iteration (iteration, inertia against the centres it started from, shift2, empty centres), then one line with K, D, rows
used and skipped and n_iter.  This is the fairseq recipe (learn_kmeans.py: MiniBatchKMeans, tol = 0) with the device doing the work; see
the docstrings of unitspeech_amd.units for what is scikit-learn's and what is not.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.audio import read_wav, to_16k  # noqa: E402
from unitspeech_amd.batching import pad_batch  # noqa: E402
from unitspeech_amd.units import KMeansQuantizer, synthetic_centers, synthetic_dense  # noqa: E402


def load_features(path):
    if path.endswith(".npy"):
        x = torch.from_numpy(np.load(path))
    else:
        x = torch.load(path, map_location="cpu")
        if isinstance(x, dict):
            if "dense" not in x:
                raise SystemExit(f"--features {path}: a dictionary needs `dense`")
            x = x["dense"]
    x = torch.as_tensor(x).float()
    if x.dim() not in (2, 3):
        raise SystemExit(f"--features {path}: dense features must be [N, D] or [B, T, D], got {tuple(x.shape)}")
    return x


def hubert_chunks(args, device):
    """-> ([features [B, Fmax, D]], [frames [B]]): one ragged batch of --wav_batch waveforms per chunk."""
    from unitspeech_amd.hubert import load_hubert_checkpoint
    if not args.hubert_checkpoint:
        raise SystemExit("--wav_list needs --hubert_checkpoint")
    hubert, normalize = load_hubert_checkpoint(args.hubert_checkpoint)
    hubert = hubert.to(device)
    with open(args.wav_list) as f:
        paths = [p.strip() for p in f if p.strip()]
    resamplers, xs, ls = {}, [], []
    for s in range(0, len(paths), args.wav_batch):
        wavs = []
        for p in paths[s:s + args.wav_batch]:
            wav = to_16k(*read_wav(p), device, resamplers)
            if hubert.frames(wav.numel()) < 1:
                print(f"skipping {p}: shorter than one frame")
                continue
            wavs.append(wav)
        if not wavs:
            continue
        batch, n = pad_batch(wavs)
        xs.append(hubert(batch, lengths=n, output_layer=args.hubert_layer, normalize=normalize))
        ls.append(torch.tensor([hubert.frames(v) for v in n], dtype=torch.int64, device=device))
    if not xs:
        raise SystemExit(f"--wav_list {args.wav_list}: no usable waveform")
    return xs, ls


def report(history, first=1):
    for i, r in enumerate(history, first):
        print(f"iter {i:3d}  inertia {r['inertia']:.6f}  shift2 {r['shift2']:.6e}  empty {r['n_empty']}", flush=True)


def fit_minibatch(args, xs, ls, seed):
    """`partial_fit` over a seeded permutation of the valid rows, after an init on all of them."""
    from unitspeech_amd.units import _fit_chunks, _valid_rows
    chunks, _, _ = _fit_chunks(xs, ls, args.n_clusters, "fit_units")
    rows = torch.cat([x[_valid_rows(x, lens)] for x, lens in chunks])
    init = args.init if args.init in ("k-means++", "random") else torch.load(args.init, map_location="cpu")["centers"]
    q = KMeansQuantizer.fit(rows, n_clusters=args.n_clusters, init=init, max_iter=0, seed=seed)
    q.counts_ = None
    g = np.random.Generator(np.random.Philox(key=[seed, 0x6d62]))
    it = 0
    for _ in range(args.epochs):
        perm = torch.from_numpy(g.permutation(rows.shape[0])).to(rows.device)
        for s in range(0, rows.shape[0], args.minibatch):
            q.partial_fit(rows[perm[s:s + args.minibatch]])
            it += 1
            report(q.history_[-1:], it)
    q.n_iter_ = it
    final = KMeansQuantizer.fit(rows, init=q.centers, max_iter=0)          # one assignment pass: the inertia of the final centres
    q.inertia_ = final.inertia_
    total = sum(x.numel() // x.shape[-1] for x in xs)
    return q, rows.shape[0], total - rows.shape[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--features", nargs="+", default=None)
    ap.add_argument("--wav_list", type=str, default=None)
    ap.add_argument("--hubert_checkpoint", type=str, default=None)
    ap.add_argument("--hubert_layer", type=int, default=11)
    ap.add_argument("--wav_batch", type=int, default=8)
    ap.add_argument("--synthetic", type=int, default=None, metavar="N")
    ap.add_argument("--synthetic_dim", type=int, default=64)
    ap.add_argument("--n_clusters", type=int, required=True)
    ap.add_argument("--init", type=str, default="k-means++", help="k-means++, random, or a .pt file with `centers`")
    ap.add_argument("--max_iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n_init", type=int, default=1, metavar="R")
    ap.add_argument("--minibatch", type=int, default=None, metavar="N")
    ap.add_argument("--epochs", type=int, default=1, metavar="E")
    ap.add_argument("--out", type=str, required=True)
    args = ap.parse_args()
    if sum(v is not None for v in (args.features, args.wav_list, args.synthetic)) != 1:
        raise SystemExit("give one of --features, --wav_list, --synthetic")
    if not torch.cuda.is_available():
        raise SystemExit("CUDA/ROCm is not available: the codebook fit has no CPU fallback")
    device = torch.device("cuda", 0)
    if args.synthetic is not None:
        planted = synthetic_centers(args.n_clusters, args.synthetic_dim, args.seed & 0xffff)
        xs, ls = [torch.from_numpy(synthetic_dense(planted, args.synthetic, (args.seed + 1) & 0xffff, noise=0.5)).to(device)], [None]
    elif args.features is not None:
        xs = [load_features(p).to(device) for p in args.features]
        ls = [None] * len(xs)
    else:
        xs, ls = hubert_chunks(args, device)
    best = None
    for r in range(max(1, args.n_init)):
        seed = args.seed + r
        if args.n_init > 1:
            print(f"run {r + 1} of {args.n_init}, seed {seed}")
        if args.minibatch:
            q, used, skipped = fit_minibatch(args, xs, ls, seed)
        else:
            init = args.init if args.init in ("k-means++", "random") else torch.load(args.init, map_location="cpu")["centers"]
            q = KMeansQuantizer.fit(xs, ls, n_clusters=args.n_clusters, init=init, max_iter=args.max_iter, tol=args.tol, seed=seed)
            report(q.history_)
            total = sum(x.numel() // x.shape[-1] for x in xs)
            used = int(q.counts_.sum())
            skipped = total - used
        if best is None or q.inertia_ < best[0].inertia_:
            best = (q, used, skipped)
    q, used, skipped = best
    q.save(args.out)
    K, D = q.centers.shape
    print(f"K {K}  D {D}  rows used {used}  skipped {skipped}  n_iter {q.n_iter_}  inertia {q.inertia_:.6f}  -> {args.out}")


if __name__ == "__main__":
    main()
