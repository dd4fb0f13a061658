"""Unit extraction on the GPU (csrc/units.hip, unitspeech_amd/units.py): every integer equal to the yardstick -- the fp64 argmin, the
run-length encoding and the closed-form process_unit of tools/units_numpy.py, and the reference's own outputs in the goldens
(tools/make_goldens_units.py).  No tolerance and no excluded rows anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import units_numpy as UN  # noqa: E402
from unitspeech_amd import units as U  # noqa: E402
from unitspeech_amd.util import generate_path, sequence_mask  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def golden_inputs(g):
    if "centers" in g:
        return g["centers"], g["dense"]
    centers = U.synthetic_centers(int(g["K"]), int(g["D"]), int(g["seed"]))
    return centers, U.synthetic_dense(centers, int(g["T"]), int(g["seed"]), float(g["noise"]))


def quantizer_for(centers):
    return U.KMeansQuantizer.from_centers(torch.from_numpy(np.ascontiguousarray(centers))).to(DEV)


class PresetDense(torch.nn.Module):
    """Stand-in for the caller's dense model: returns the preset features whatever the waveform."""

    def __init__(self, dense):
        super().__init__()
        self.register_buffer("dense", torch.from_numpy(dense))

    def forward(self, waveform):
        return self.dense


WAV = torch.zeros(2, 160)          # two channels: averaged away by the encoder, as in the reference


def counters(q):
    return [int(v) for v in q.last_counters.cpu()]


@pytest.mark.parametrize("name", ["units_tiny", "units_full"])
def test_goldens_quantize_dedup_and_process_equal_the_reference(golden, name):
    g = golden(name)
    centers, dense = golden_inputs(g)
    q = quantizer_for(centers)
    units = q(torch.from_numpy(dense).to(DEV))
    assert units.dtype == torch.int64 and units.shape == (dense.shape[0],) and units.device.type == "cuda"
    assert np.array_equal(units.cpu().numpy(), g["units"])
    assert counters(q)[0] == 0
    enc = U.SpeechEncoder(PresetDense(dense), q, deduplicate=True).to(DEV)
    out = enc(WAV.to(DEV))
    assert set(out) == {"units", "durations", "dense"} and out["units"].dtype == torch.int64 and out["durations"].dtype == torch.int64
    assert np.array_equal(out["units"].cpu().numpy(), g["dedup_units"]) and np.array_equal(out["durations"].cpu().numpy(), g["dedup_durations"])
    assert out["dense"].shape == dense.shape
    plain = U.SpeechEncoder(PresetDense(dense), q, deduplicate=False).to(DEV)(WAV.to(DEV))
    for i, (sr, hop) in enumerate(g["rates"]):
        for encoded in (out, plain):
            pu, pd = U.process_unit(encoded, int(sr), int(hop))
            assert pu.dtype == torch.int64 and pd.dtype == torch.int64 and pu.dim() == 1 and pu.shape == pd.shape and pu.device.type == "cuda"
            assert np.array_equal(pu.cpu().numpy(), g[f"proc_unit_{i}"]) and np.array_equal(pd.cpu().numpy(), g[f"proc_duration_{i}"]), (sr, hop)
    # the same from an `encoded` without "dense" (the sum of the durations is read back instead)
    pu, pd = U.process_unit({"units": out["units"], "durations": out["durations"]}, 16000, 256)
    assert np.array_equal(pu.cpu().numpy(), g["proc_unit_0"]) and np.array_equal(pd.cpu().numpy(), g["proc_duration_0"])


@pytest.mark.parametrize("K", [50, 1000, 2000])
@pytest.mark.parametrize("D", [256, 768, 1024])
def test_units_equal_the_fp64_argmin_on_every_row(K, D):
    centers = U.synthetic_centers(K, D, 10 + K + D)
    dense = U.synthetic_dense(centers, 200, 11 + K + D, noise=1.0)
    q = quantizer_for(centers)
    got = q(torch.from_numpy(dense).to(DEV)).cpu().numpy()
    want = UN.kmeans_argmin(dense, centers)
    print(f"\nK {K} D {D}: rows decided in fp64 {counters(q)[1]} of {len(want)}")
    assert np.array_equal(got, want)


def test_ragged_batch_padding_item_alone_and_repeatability():
    K, D, B, Tmax = 200, 256, 32, 120
    centers = U.synthetic_centers(K, D, 5)
    g = np.random.default_rng(5)
    lengths = g.integers(1, Tmax + 1, size=B)
    lengths[0], lengths[1], lengths[2] = 1, Tmax, 64
    dense = np.stack([U.synthetic_dense(centers, Tmax, 100 + b, noise=1.0) for b in range(B)])
    q = quantizer_for(centers)
    x, lens = torch.from_numpy(dense).to(DEV), torch.from_numpy(lengths).to(DEV)
    got = q.quantize(x, lens).cpu().numpy()
    again = q.quantize(x, lens).cpu().numpy()
    assert np.array_equal(got, again)
    want = UN.kmeans_argmin(dense.reshape(-1, D), centers).reshape(B, Tmax)
    for b in range(B):
        assert np.array_equal(got[b, :lengths[b]], want[b, :lengths[b]]), b
        assert (got[b, lengths[b]:] == -1).all(), b
    for b in (0, 1, 7, 31):
        alone = q.quantize(x[b:b + 1, :lengths[b]].contiguous()).cpu().numpy()[0]
        assert np.array_equal(alone, got[b, :lengths[b]]), b
    # the batched mel-rate path against one item at a time through the drop-ins
    unit, dur, n = q.encode(x, lens, 16000, 256)
    unit2, dur2, n2 = q.encode(x, lens, 16000, 256)
    assert torch.equal(unit, unit2) and torch.equal(dur, dur2) and torch.equal(n, n2)
    assert dur.dtype == torch.float32 and unit.dtype == torch.int64 and n.dtype == torch.int64
    for b in range(B):
        wu, wd = UN.process_unit(want[b, :lengths[b]], np.ones(lengths[b], dtype=np.int64), 16000, 256)
        nb = int(n[b])
        assert nb == len(wu) and np.array_equal(unit[b, :nb].cpu().numpy(), wu) and np.array_equal(dur[b, :nb].cpu().numpy(), wd.astype(np.float32)), b
        assert not unit[b, nb:].any() and not dur[b, nb:].any()
    assert int(n[0]) == 1 and lengths[0] * 320 // 256 == 1


def test_duplicated_centres_give_the_lower_index():
    K, D = 64, 256
    centers = U.synthetic_centers(K, D, 8)
    centers[40] = centers[3]
    centers[5] = centers[50]
    g = np.random.default_rng(8)
    ids = np.array([3, 40, 50, 5] * 8)
    dense = (centers[ids] + 0.3 * g.standard_normal((len(ids), D))).astype(np.float32)
    dense[:4] = centers[ids[:4]]                            # rows exactly on a duplicated centre: both scores are exactly 0
    q = quantizer_for(centers)
    got = q(torch.from_numpy(dense).to(DEV)).cpu().numpy()
    assert np.array_equal(got, UN.kmeans_argmin(dense, centers))
    assert set(got.tolist()) == {3, 5} and counters(q)[1] == len(ids)     # an exact tie has no gap: every row went through fp64


@pytest.mark.parametrize("D", [256, 768])
def test_rows_on_a_bisector_are_decided_by_both_paths(D):
    """Rows on the bisector of two centres, displaced towards one of them so that the gap between the two best scores is 1e-9 ... 1e-3
    of |x| max|c|: the fp32 error bound is about (D + 1) 2^-24 of that (5e-5 at D = 768), so the small gaps must go through fp64 and
    the large ones must not -- and every row must come out as the fp64 argmin."""
    K = 1000
    centers = U.synthetic_centers(K, D, 20 + D)
    g = np.random.default_rng(D)
    cmax = np.linalg.norm(centers.astype(np.float64), axis=1).max()
    rows = []
    for r in (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3):
        for _ in range(16):
            a, b = g.choice(K, size=2, replace=False)
            ca, cb = centers[a].astype(np.float64), centers[b].astype(np.float64)
            mid, delta = (ca + cb) / 2, ca - cb
            t = r * np.linalg.norm(mid) * cmax / (2 * delta @ delta) * g.choice([-1.0, 1.0])      # score gap = 2 t |delta|^2
            rows.append((mid + t * delta).astype(np.float32))
    dense = np.stack(rows)
    q = quantizer_for(centers)
    got = q(torch.from_numpy(dense).to(DEV)).cpu().numpy()
    want = UN.kmeans_argmin(dense, centers)
    flagged = counters(q)[1]
    print(f"\nD {D}: {flagged} of {len(rows)} bisector rows decided in fp64")
    assert np.array_equal(got, want)
    assert 16 * 3 <= flagged <= len(rows) - 16                # 1e-9 ... 1e-7 are far below the bound, 1e-3 is far above it


def test_a_nan_row_gives_minus_one_and_leaves_its_neighbours_alone():
    K, D, T = 1000, 768, 70
    centers = U.synthetic_centers(K, D, 30)
    dense = U.synthetic_dense(centers, T, 31)
    clean = UN.kmeans_argmin(dense, centers)
    dense[33, 700] = np.nan
    q = quantizer_for(centers)
    got = q(torch.from_numpy(dense).to(DEV)).cpu().numpy()
    assert got[33] == -1 and counters(q)[0] == 1
    keep = np.arange(T) != 33
    assert np.array_equal(got[keep], clean[keep])
    dense[34, 0] = np.inf
    got = q(torch.from_numpy(dense).to(DEV)).cpu().numpy()
    assert got[33] == -1 and got[34] == -1 and counters(q)[0] == 2 and np.array_equal(got[:33], clean[:33]) and np.array_equal(got[35:], clean[35:])


def sticky_batch(g, B, Lin, vocab):
    units = np.zeros((B, Lin), dtype=np.int64)
    n = g.integers(1, Lin + 1, size=B)
    n[0], n[-1] = 1, Lin
    for b in range(B):
        units[b, :n[b]] = np.repeat(g.integers(0, vocab, size=Lin), g.integers(1, 5, size=Lin))[:n[b]]
    return units, n


def test_dedup_equals_unique_consecutive():
    g = np.random.default_rng(3)
    units, n = sticky_batch(g, 9, 700, 5)
    out_u, out_d, out_n = U.dedup_units(torch.from_numpy(units).to(DEV), torch.from_numpy(n).to(DEV))
    assert out_u.dtype == torch.int64 and out_d.dtype == torch.int64 and out_n.dtype == torch.int64
    for b in range(len(n)):
        wu, wd = torch.unique_consecutive(torch.from_numpy(units[b, :n[b]]), return_counts=True)
        k = int(out_n[b])
        assert k == len(wu) and torch.equal(out_u[b, :k].cpu(), wu) and torch.equal(out_d[b, :k].cpu(), wd), b
        assert not out_u[b, k:].any() and not out_d[b, k:].any()


@pytest.mark.parametrize("rate,hop", [(16000, 256), (16000, 320), (16000, 512), (16000, 1000), (22050, 256), (16000, 97), (8000, 2000),
                                      (16000, 320 * 63 + 1)])
def test_process_equals_the_numpy_statement(rate, hop):
    """Tie frames (320 / 256), hop > spf (a frame over several 50 Hz frames, up to the limit of 64), items shorter than one hop
    (no output frame: length 0, not an error), deduplicated and plain input."""
    g = np.random.default_rng(rate + hop)
    B, Lin = 12, 300
    units, n = sticky_batch(g, B, Lin, 4)
    dev_u, dev_n = torch.from_numpy(units).to(DEV), torch.from_numpy(n).to(DEV)
    unit, dur, dur_f, n_out = U.process_units_batch(dev_u, None, dev_n, rate, hop)
    assert torch.equal(dur_f, dur.to(torch.float32))
    du, dd, dn = U.dedup_units(dev_u, dev_n)
    unit2, dur2, _, n_out2 = U.process_units_batch(du, dd, dn, rate, hop, max_frames=Lin)
    assert torch.equal(unit, unit2) and torch.equal(dur, dur2) and torch.equal(n_out, n_out2)
    for b in range(B):
        wu, wd = UN.process_unit(units[b, :n[b]], np.ones(n[b], dtype=np.int64), rate, hop)
        k = int(n_out[b])
        assert k == len(wu) and np.array_equal(unit[b, :k].cpu().numpy(), wu) and np.array_equal(dur[b, :k].cpu().numpy(), wd), (b, n[b])
    assert int(n_out[0]) == (1 if 1 * (rate // 50) >= hop else 0)
    if (rate // 50) < hop:
        pu, pd = U.process_unit({"units": dev_u[0, :1], "durations": torch.ones(1, dtype=torch.int64, device=DEV)}, rate, hop)
        assert pu.shape == (0,) and pd.shape == (0,) and pu.dtype == torch.int64


def test_process_refuses_a_span_of_more_than_64_and_flags_an_overfull_item():
    u = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="64"):
        U.process_units_batch(u, None, None, 16000, 320 * 63 + 2)
    # durations that cover more 50 Hz frames than max_frames promises: the item is marked, nothing is written out of bounds
    d = torch.full((1, 8), 10, dtype=torch.int64, device=DEV)
    _, _, _, n = U.process_units_batch(u, d, None, 16000, 256, max_frames=8)
    assert int(n[0]) == -1


def test_bos_eos_and_generate_path_from_the_produced_durations(golden):
    g = golden("units_tiny")
    centers, dense = golden_inputs(g)
    q = quantizer_for(centers)
    enc = U.SpeechEncoder(PresetDense(dense), q, deduplicate=True, add_bos_eos=True).to(DEV)
    out = enc(WAV.to(DEV))
    K = int(g["K"])
    assert out["units"][0] == K and out["units"][-1] == K + 1 and out["durations"][0] == 0 and out["durations"][-1] == 0
    assert np.array_equal(out["units"][1:-1].cpu().numpy(), g["dedup_units"]) and out["dense"].shape[0] == dense.shape[0] + 2
    # mel-rate durations into the alignment the unit encoder's output is expanded with (finetune.py:125-128)
    unit, duration, n = q.encode(torch.from_numpy(dense).to(DEV).unsqueeze(0), None, 16000, 256)
    frames = dense.shape[0] * 320 // 256
    assert int(duration.sum()) == frames
    x_mask = sequence_mask(n, unit.shape[1]).to(torch.float32)
    y_mask = torch.ones(1, frames + 5, device=DEV)
    attn = generate_path(duration, x_mask.unsqueeze(-1) * y_mask.unsqueeze(1))
    cols = attn.sum(1)[0]
    assert torch.equal(cols[:frames], torch.ones(frames, device=DEV)) and not cols[frames:].any()
    assert torch.equal(attn.sum(2)[0], duration[0])


def _losses(stdout):
    return [float(line.split()[-1]) for line in stdout.splitlines() if line.startswith("iter ")]


def test_finetune_cli_with_the_hip_unit_extraction(tmp_path):
    """`finetune.py --synthetic --learned_frontend --hip_units`: dense features -> units -> mel-rate durations -> unit encoder -> three
    fine-tune iterations.  The iteration losses are finite; "decreasing or equal" is read off the probe loss (the diffusion loss at 8
    fixed (t, z) draws before and after the run), because an iteration's own loss is taken at a fresh random t and varies several-fold
    with it whatever the weights do."""
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--synthetic", "--learned_frontend", "--hip_units", "--n_iters", "3",
                        "--ID", "5", "--report_memory", "--out_dir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"hip units: (\d+) dense frames -> (\d+) units over (\d+) mel frames", r.stdout)
    assert m and int(m.group(1)) == 480 and 1 <= int(m.group(2)) <= 480 and int(m.group(3)) == 600
    losses = _losses(r.stdout)
    pb, pa = (float(re.search(rf"probe loss {w} ([0-9.]+)", r.stdout).group(1)) for w in ("before", "after"))
    print(f"\nfinetune.py --hip_units: iteration losses {losses}, probe loss {pb:.5f} -> {pa:.5f}")
    assert len(losses) == 2 and all(np.isfinite(losses)) and np.isfinite(pa) and pa <= pb
    assert os.path.exists(tmp_path / "5.pt")
