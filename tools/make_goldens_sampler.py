#!/usr/bin/env python3
"""Sampler golden vectors from the REFERENCE decoder (build container only; see tools/make_goldens.py for the loader).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_sampler.py [names...]

  tiny_scales   sampler_tiny_scales.npz  TINY, B=2, T=16, lengths [16, 11], N=10, four unequal guidance-scale pairs
  tiny_steps    sampler_tiny_steps.npz   TINY, B=3, T=16, lengths [16, 11, 8], w=(1.3, 0.7), N in {64, 65, 130}: the loop past one
                                         block of precomputed time projections (64 steps)
  full_seeds    sampler_full_seeds.npz   FULL, B=1, T=64, length 60, N=10, w=(1.7, 0.4), weight seeds 1 and 2

Every item runs alone through the reference's `UnitSpeech.forward` (its schedule is only right for B=1), in fp32
(`out*`) and in fp64 (`out_fp64*`), with `torch.randn` replayed from `synthetic_inputs(...)["noise"]`.  The files keep checksums of z
and of the noise, not the tensors: the tests regenerate both from the stored seed.

Condition on every stored case (asserted here; it is a condition on the inputs, not a tolerance of any test): the reference's own
fp32-vs-fp64 mean-L1 is <= 2e-4, a fifth of the 1e-3 loop bar.  A case that misses it gets another input (or weight) seed below.
Every file is written and the whole table printed before the assertion, so a miss is seen next to the rows that hold.

Known miss: tiny N=130 gives 2.75e-4, and 2.7e-4 ... 2.9e-4 at every input seed (22, 24-28) and weight seed (0-4) tried.  It is the
schedule, not the seed: the reference's fp64 run reads tables rounded once from fp64, its fp32 run tables that carry an fp32 exp, a
division and a 130-term fp32 cumprod (an fp64 run on the fp32 tables lies 8.8e-5 from `out` and 2.6e-4 from
`out_fp64`).  The case and the bar stay as they are; the run ends with the failed assertion naming that row.

The files are written with fixed zip timestamps, so a rerun on the same host reproduces them byte for byte."""
from __future__ import annotations

import io
import os
import sys
import time
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import FULL, OUT, TINY, build, load_reference, run_loop, tt  # noqa: E402
from unitspeech_amd.params import synthetic_inputs  # noqa: E402

GAP_MAX = 2e-4

SCALES = ((1.7, 0.4), (0.4, 1.7), (2.5, 0.0), (0.0, 0.3))
SCALES_IN = dict(B=2, T=16, lengths=[16, 11], n_steps=10, seed=21)
STEPS = (64, 65, 130)
STEPS_W = (1.3, 0.7)
STEPS_IN = dict(B=3, T=16, lengths=[16, 11, 8], seed=22)
FULL_WEIGHT_SEEDS = (1, 2)
FULL_W = (1.7, 0.4)
FULL_IN = dict(B=1, T=64, lengths=[60], n_steps=10, seed=23)

ROWS = []          # (case, fp32-vs-fp64 mean-L1, mean|out|)


def save_fixed(name, **arrs):
    """np.savez_compressed with a fixed timestamp on every member: the same arrays give the same bytes."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrs.items():
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"  wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def per_item(m32, m64, inp, n, wt, ws):
    """Independent B=1 reference runs of every item, fp32 and fp64."""
    o32, o64 = [], []
    for b in range(inp["z"].shape[0]):
        one = {k: (v[:, b:b + 1] if k == "noise" else v[b:b + 1]) for k, v in inp.items()}
        o32.append(run_loop(m32, one, n, wt, ws))
        o64.append(run_loop(m64, {k: v.double() for k, v in one.items()}, n, wt, ws))
    return torch.cat(o32, 0), torch.cat(o64, 0)


def record(case, out, out64):
    gap = (out.double() - out64).abs().mean().item()
    ROWS.append((case, gap, out64.abs().mean().item()))
    print(f"   {case}: reference fp32 vs fp64 mean-L1 {gap:.3e}  mean|out| {ROWS[-1][2]:.1f}", flush=True)
    assert torch.isfinite(out).all(), case


def checksums(inp):
    return dict(z_abs_sum=inp["z"].double().abs().sum(), noise_abs_sum=inp["noise"].double().abs().sum())


def g_tiny_scales(U):
    c = SCALES_IN
    inp = tt(synthetic_inputs(TINY, c["B"], c["T"], seed=c["seed"], n_steps=c["n_steps"], lengths=c["lengths"]))
    m32, m64 = build(U, TINY, 0), build(U, TINY, 0, torch.float64)
    outs, outs64 = [], []
    for wt, ws in SCALES:
        o, o64 = per_item(m32, m64, inp, c["n_steps"], wt, ws)
        record(f"tiny N=10 w=({wt}, {ws})", o, o64)
        outs.append(o); outs64.append(o64)
    save_fixed("sampler_tiny_scales", out=torch.stack(outs), out_fp64=torch.stack(outs64), w_text=np.array([s[0] for s in SCALES]),
               w_spk=np.array([s[1] for s in SCALES]), lengths=np.array(c["lengths"]), seed=c["seed"], weight_seed=0,
               n_steps=c["n_steps"], **checksums(inp))


def g_tiny_steps(U):
    c = STEPS_IN
    m32, m64 = build(U, TINY, 0), build(U, TINY, 0, torch.float64)
    arrs = {}
    for n in STEPS:
        inp = tt(synthetic_inputs(TINY, c["B"], c["T"], seed=c["seed"], n_steps=n, lengths=c["lengths"]))
        o, o64 = per_item(m32, m64, inp, n, *STEPS_W)
        record(f"tiny N={n} w={STEPS_W}", o, o64)
        arrs[f"out_N{n}"], arrs[f"out_fp64_N{n}"] = o, o64
        arrs[f"noise_abs_sum_N{n}"] = inp["noise"].double().abs().sum()
    save_fixed("sampler_tiny_steps", **arrs, n_steps=np.array(STEPS), w_text=STEPS_W[0], w_spk=STEPS_W[1],
               lengths=np.array(c["lengths"]), seed=c["seed"], weight_seed=0, z_abs_sum=inp["z"].double().abs().sum())


def g_full_seeds(U):
    c = FULL_IN
    inp = tt(synthetic_inputs(FULL, c["B"], c["T"], seed=c["seed"], n_steps=c["n_steps"], lengths=c["lengths"]))
    arrs = {}
    for ws in FULL_WEIGHT_SEEDS:
        t0 = time.time()
        o, o64 = per_item(build(U, FULL, ws), build(U, FULL, ws, torch.float64), inp, c["n_steps"], *FULL_W)
        print(f"   weight seed {ws}: {time.time() - t0:.0f} s", flush=True)
        record(f"full N=10 w={FULL_W} weight seed {ws}", o, o64)
        arrs[f"out_s{ws}"], arrs[f"out_fp64_s{ws}"] = o, o64
    save_fixed("sampler_full_seeds", **arrs, weight_seeds=np.array(FULL_WEIGHT_SEEDS), w_text=FULL_W[0], w_spk=FULL_W[1],
               lengths=np.array(c["lengths"]), seed=c["seed"], n_steps=c["n_steps"], **checksums(inp))


ALL = {"tiny_scales": g_tiny_scales, "tiny_steps": g_tiny_steps, "full_seeds": g_full_seeds}

if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    U = load_reference()
    for name in (sys.argv[1:] or list(ALL)):
        print(name, flush=True)
        ALL[name](U)
    print("\n| case | reference fp32 vs fp64, mean-L1 | mean \\|out\\| |\n|---|---|---|")
    for case, gap, scale in ROWS:
        print(f"| {case} | {gap:.2e} | {scale:.1f} |")
    missed = [case for case, gap, _ in ROWS if not gap <= GAP_MAX]
    assert not missed, f"reference fp32-vs-fp64 mean-L1 above {GAP_MAX}: {missed}: change the seed, not the bar"
