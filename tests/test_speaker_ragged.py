"""Ragged speaker-encoder batches, the parts that need no GPU: the batch planner and file-list parser of extract_speaker_embeddings.py, the
speaker means against the reference's running mean, and the new entry point's prototype, registration and host-side refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from extract_speaker_embeddings import parse_filelist, plan_batches, running_mean, speaker_means  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.speaker_encoder import ECAPA_TDNN  # noqa: E402


def _check_plan(lengths, max_batch, max_padded):
    batches = plan_batches(lengths, max_batch, max_padded)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(len(lengths))), "every utterance exactly once"
    for b in batches:
        assert 1 <= len(b) <= max_batch
        longest = max(lengths[i] for i in b)
        assert len(b) * longest <= max_padded or len(b) == 1, (b, longest)
    # sorted by length: no batch holds an utterance shorter than one of an earlier batch
    for prev, nxt in zip(batches, batches[1:]):
        assert max(lengths[i] for i in prev) <= min(lengths[i] for i in nxt)
    return batches


def test_plan_batches_covers_every_utterance_within_both_bounds():
    g = np.random.Generator(np.random.Philox(key=11))
    for n, max_batch, max_padded in ((1, 4, 1000), (7, 1, 10 ** 9), (64, 8, 10 ** 9), (64, 32, 400000), (100, 5, 90000), (33, 32, 16000 * 40)):
        lengths = [int(v) for v in g.integers(400, 160000, size=n)]
        batches = _check_plan(lengths, max_batch, max_padded)
        if max_padded >= 10 ** 9:
            assert len(batches) == -(-n // max_batch)              # only the item bound cuts: full batches, then the rest
    assert plan_batches([], 4, 100) == []
    with pytest.raises(ValueError):
        plan_batches([5], 0, 100)
    with pytest.raises(ValueError, match="utterance 1"):
        plan_batches([5, 0], 2, 100)


def test_plan_batches_keeps_an_utterance_longer_than_the_sample_bound():
    lengths = [500, 90000, 700, 600, 50000]
    batches = _check_plan(lengths, 4, 2000)
    assert [1] in batches and [4] in batches                      # each alone, not dropped
    assert batches[0] == [0, 3] and batches[1] == [2]             # 3 x 700 > 2000 closes the first batch
    # equal lengths keep file order, and the indices map results back to it
    batches = _check_plan([800] * 5, 2, 10 ** 6)
    assert batches == [[0, 1], [2, 3], [4]]
    rows = [None] * 5
    for b in batches:
        for pos, i in enumerate(b):
            rows[i] = (b, pos)
    assert all(r is not None for r in rows)


def test_parse_filelist():
    text = "a/one.pt|hello there|spk7\n\n  b/two.npz|with | a bar|spk7  \nc/three.pt||other\n"
    assert parse_filelist(text) == [("a/one.pt", "hello there", "spk7"), ("b/two.npz", "with | a bar", "spk7"), ("c/three.pt", "", "other")]
    with pytest.raises(ValueError, match="line 2"):
        parse_filelist("a.pt|x|s\nb.pt|only two\n")


@pytest.mark.parametrize("n", [1, 4, 12])
def test_speaker_mean_is_the_running_mean_up_to_rounding(n):
    """stack(...).mean(0) against process_spkr_embs.py's (m * count + e) / (count + 1): the bar is 1e-6 of the largest entry, 17 fp32 ulp;
    the running mean rounds three times per update (product, sum, quotient) and each update scales the error so far by count / (count + 1)."""
    g = torch.Generator().manual_seed(n)
    rows = [0.15 * torch.randn(256, generator=g) for _ in range(n)]
    means, uncond = speaker_means(rows + rows[:1], ["a"] * n + ["b"])
    assert list(means) == ["a", "b"] and tuple(means["a"].shape) == (1, 256) and tuple(uncond.shape) == (1, 1, 256)
    assert torch.equal(means["a"], torch.stack(rows).mean(0)[None]) and torch.equal(means["b"], rows[0][None])
    assert torch.equal(uncond, torch.stack([means["a"], means["b"]]).mean(0, keepdim=True))
    ref = running_mean(rows)
    assert float((means["a"] - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    exact = torch.stack(rows).double().mean(0)[None]
    assert float((means["a"].double() - exact).abs().max()) <= 1e-6 * float(exact.abs().max())


def test_prototype_is_declared_and_registered():
    with open(os.path.join(ROOT, "include", "unitspeech_hip.h")) as f:
        header = f.read()
    m = re.search(r"int us_speaker_forward_lengths\(([^;]*)\);", header)
    assert m, "us_speaker_forward_lengths is not declared in include/unitspeech_hip.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["us_speaker_handle h", "const float* hidden_states", "int L", "int B", "int Tmax", "const int64_t* lengths", "float* emb_out",
                    "int normalize", "void* workspace", "size_t workspace_bytes", "us_stream stream"]
    res, argtypes = _lib.SIGNATURES["us_speaker_forward_lengths"]
    assert res is C.c_int and len(argtypes) == len(args) and argtypes[5] == C.POINTER(C.c_int64)
    # us_speaker_forward keeps its signature
    assert len(_lib.SIGNATURES["us_speaker_forward"][1]) == 10
    assert hasattr(_lib.load(), "us_speaker_forward_lengths")


def test_lengths_are_refused_on_the_host_before_any_device_work():
    """Null, too short and too long lengths are US_EINVAL with the item named; lengths in range pass on to the next check, the weights
    (never loaded here), so nothing was launched on the way."""
    lib = _lib.load()
    h = C.c_void_p()
    c = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)._config_struct()
    assert lib.us_speaker_create(C.byref(h), C.byref(c)) == 0
    p, T = 4096, 9                   # never dereferenced
    EINVAL, EWEIGHTS = -1, -4

    def run(lengths, B=3, Tmax=T, L=3):
        arr = None if lengths is None else (C.c_int64 * len(lengths))(*lengths)
        return lib.us_speaker_forward_lengths(h, p, L, B, Tmax, arr, p, 0, p, 1 << 30, None)

    assert run(None) == EINVAL and b"lengths is null" in lib.us_speaker_last_error(h)
    assert run([9, 0, 4]) == EINVAL and b"lengths[1] = 0" in lib.us_speaker_last_error(h)
    assert run([9, 4, 10]) == EINVAL and b"lengths[2] = 10" in lib.us_speaker_last_error(h)
    assert run([-1, 4, 4]) == EINVAL and b"lengths[0] = -1" in lib.us_speaker_last_error(h)
    assert run([9, 4, 1], B=0) == EINVAL and run([9, 4, 1], Tmax=0) == EINVAL
    assert run([9, 4, 1], L=2) == EINVAL and b"n_layers" in lib.us_speaker_last_error(h)
    assert run([9, 4, 1]) == EWEIGHTS and run([1, 1, 1], L=0) == EWEIGHTS
    lib.us_speaker_destroy(h)
    # the module: the number of lengths is checked before the device is
    m = ECAPA_TDNN(feat_dim=16, channels=16, emb_dim=8, feat_type="wavlm_large", feat_num=3)
    with pytest.raises(ValueError, match=r"2 lengths for 3 items \(item 2 has none\)"):
        m.forward_features(torch.zeros(3, 3, 5, 16), [5, 5])
    with pytest.raises(ValueError, match="item 1"):
        m.embed(torch.zeros(3, 2, 5, 16))
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.embed(torch.zeros(3, 2, 5, 16), [5, 4])
