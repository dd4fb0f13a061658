"""Unit extraction, the parts that need no GPU: the numpy yardstick (tools/units_numpy.py) against the reference goldens
(tools/make_goldens_units.py: the reference's KMeansQuantizer, unique_consecutive and process_unit) and against a brute-force
statement of process_unit, and the argument checks of the library and its Python drop-ins."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import units_numpy as UN  # noqa: E402
from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd import units as U  # noqa: E402


def golden_inputs(g):
    if "centers" in g:
        return g["centers"], g["dense"]
    centers = U.synthetic_centers(int(g["K"]), int(g["D"]), int(g["seed"]))
    return centers, U.synthetic_dense(centers, int(g["T"]), int(g["seed"]), float(g["noise"]))


@pytest.mark.parametrize("name", ["units_tiny", "units_full"])
def test_units_numpy_reproduces_the_reference_goldens(golden, name):
    g = golden(name)
    centers, dense = golden_inputs(g)
    assert centers.shape == (int(g["K"]), int(g["D"])) and dense.shape == (int(g["T"]), int(g["D"]))
    units = UN.kmeans_argmin(dense, centers)
    assert np.array_equal(units, g["units"])
    du, dd = UN.run_lengths(units)
    assert np.array_equal(du, g["dedup_units"]) and np.array_equal(dd, g["dedup_durations"])
    assert len(g["rates"]) == 5
    for i, (sr, hop) in enumerate(g["rates"]):
        for pu, pd in (UN.process_unit(du, dd, int(sr), int(hop)), UN.process_unit(units, np.ones_like(units), int(sr), int(hop))):
            assert np.array_equal(pu, g[f"proc_unit_{i}"]) and np.array_equal(pd, g[f"proc_duration_{i}"]), (sr, hop)


def sticky_stream(g, vocab):
    """A ragged, sticky unit stream: few distinct units, so that neighbouring runs repeat and frames tie."""
    n = int(g.integers(1, 40))
    units = g.integers(0, vocab, size=n)
    durations = g.integers(1, 6, size=n)
    return units, durations


@pytest.mark.parametrize("rate,hop", [(16000, 256), (16000, 320), (16000, 512), (16000, 1000), (22050, 256), (16000, 97), (8000, 2000)])
def test_closed_form_process_unit_equals_the_sample_expansion(rate, hop):
    g = np.random.default_rng(rate + hop)
    for case in range(60):
        units, durations = sticky_stream(g, vocab=int(g.integers(2, 6)))
        if case % 2:
            units, durations = np.repeat(units, durations), np.ones(int(durations.sum()), dtype=np.int64)     # not deduplicated
        got, want = UN.process_unit(units, durations, rate, hop), UN.process_unit_expanded(units, durations, rate, hop)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, units, durations)
        assert got[1].sum() == durations.sum() * (rate // 50) // hop


def test_tie_frames_take_the_smallest_unit_like_torch_mode():
    """320 samples per 50 Hz frame against a hop of 256: the frame over samples [512, 768) holds 128 samples each of 50 Hz frames 1
    and 2 -- a tie, which `torch.mode` on the CPU gives to the smaller value whichever comes first."""
    for a, b in ((7, 2), (2, 7)):
        units = np.array([1, a, b, 1, 1, 1, 1, 1])
        frames = UN.frame_units(units, np.ones(8, dtype=np.int64), 16000, 256)
        assert frames[2] == 2
        row = torch.from_numpy(np.repeat(units, 320)[:2560]).reshape(-1, 256)
        assert np.array_equal(frames, row.mode(1)[0].numpy())


def test_input_shorter_than_one_hop_gives_no_frames():
    pu, pd = UN.process_unit(np.array([5]), np.array([1]), 16000, 1000)
    assert pu.size == 0 and pd.size == 0


def test_kmeans_argmin_takes_the_first_index_on_exact_ties_and_marks_bad_rows():
    centers = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]], dtype=np.float32)
    x = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [np.nan, 0, 0, 0], [0, 2, 0, 0]], dtype=np.float32)
    assert UN.kmeans_argmin(x, centers).tolist() == [0, 0, -1, 1]


def test_library_refuses_unsupported_sizes():
    lib = _lib.load()
    assert lib.us_units_packed_bytes(1000, 768) == (768 * 1024 + 1024 + 4) * 4
    assert lib.us_units_packed_bytes(2049, 768) == 0 and lib.us_units_packed_bytes(100, 770) == 0 and lib.us_units_packed_bytes(100, 1028) == 0
    assert lib.us_units_workspace_bytes(1, 500, 2049, 768, 0) == 0 and lib.us_units_workspace_bytes(1, 500, 1000, 766, 0) == 0
    assert lib.us_units_workspace_bytes(1, 500, 1000, 768, 625) > 0
    buf = (C.c_float * 16)()
    # K > 2048 and D not a multiple of 4 are refused before anything is launched
    rc = lib.us_units_pack_centers(buf, 2049, 768, buf, 1 << 30, None)
    assert rc == -1 and b"2048" in lib.us_last_error(None)
    rc = lib.us_units_pack_centers(buf, 50, 18, buf, 1 << 30, None)
    assert rc == -1 and b"multiple of 4" in lib.us_last_error(None)
    rc = lib.us_units_quantize(buf, buf, buf, 1, 4, 50, 18, buf, buf, buf, 1 << 30, None)
    assert rc == -1 and b"multiple of 4" in lib.us_last_error(None)
    # an output frame over more than 64 frames of the 50 Hz stream: 16000 // 50 = 320 samples per frame, hop 320 * 64 spans 64, + 2 spans 65
    rc = lib.us_units_process(buf, None, buf, 1, 4, 16000, 320 * 63 + 2, buf, buf, None, buf, 4, buf, 1 << 30, None)
    assert rc == -1 and b"64" in lib.us_last_error(None)
    rc = lib.us_units_process(buf, None, buf, 1, 4, 16000, 0, buf, buf, None, buf, 4, buf, 1 << 30, None)
    assert rc == -1
    # a workspace that is too small is its own error code
    rc = lib.us_units_process(buf, None, buf, 1, 4, 16000, 256, buf, buf, None, buf, 4, buf, 8, None)
    assert rc == -5


def test_python_drop_ins_refuse_what_the_library_does_not_do():
    with pytest.raises(ValueError, match="2048"):
        U.KMeansQuantizer.from_centers(torch.zeros(2049, 16))
    with pytest.raises(ValueError, match="multiple of 4"):
        U.KMeansQuantizer.from_centers(torch.zeros(50, 18))
    q = U.KMeansQuantizer.from_centers(torch.from_numpy(U.synthetic_centers(50, 16, 0)))
    assert q.vocab_size == 50 and q.device == torch.device("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q(torch.zeros(3, 16))
    with pytest.raises(NotImplementedError, match="need_f0=False"):
        U.SpeechEncoder(torch.nn.Identity(), q, deduplicate=True, need_f0=True)
    with pytest.raises(NotImplementedError, match="KMeansQuantizer"):
        U.SpeechEncoder.by_name("mhubert-base-25hz", "kmeans", 1000, True)
    enc = U.SpeechEncoder(torch.nn.Identity(), q, deduplicate=True, add_bos_eos=True)
    assert enc.vocab_size == 50 and int(enc.bos) == 50 and int(enc.eos) == 51 and enc.need_f0 is False
    with pytest.raises(ValueError, match="64"):
        U._check_rates(16000, 320 * 63 + 2)
    assert U._check_rates(16000, 320 * 63 + 1) == (16000, 320 * 63 + 1, 320)


def test_quantizer_reads_a_scikit_learn_checkpoint(tmp_path):
    joblib = pytest.importorskip("joblib")
    cluster = pytest.importorskip("sklearn.cluster")
    centers = U.synthetic_centers(8, 4, 1)
    km = cluster.KMeans(n_clusters=8, n_init=1, max_iter=1, random_state=0).fit(centers)
    km.cluster_centers_ = centers
    joblib.dump(km, tmp_path / "km.bin")
    q = U.KMeansQuantizer(str(tmp_path / "km.bin"))
    assert q.vocab_size == 8 and torch.equal(q.centers, torch.from_numpy(centers))
