"""Monotonic alignment search and the duration loss of the text-to-speech training step on the CPU: the numpy restatement
(tools/mas_numpy.py) against brute-force enumeration of every monotonic path and against a scalar transcription of the
algorithm, and the C ABI of csrc/tts_train.hip (no device work is launched here)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mas_numpy as M  # noqa: E402
from unitspeech_amd import _build, _lib  # noqa: E402


def scalar_mas(value, tx, ty):
    """One-cell-at-a-time transcription of the algorithm (fp32 scalars), independent of mas_numpy's column vectorisation."""
    v = [[np.float32(value[x, y]) for y in range(value.shape[1])] for x in range(value.shape[0])]
    neg = np.float32(-1e9)
    for y in range(ty):
        for x in range(max(0, tx + y - ty), min(tx, y + 1)):
            v_cur = neg if x == y else v[x][y - 1]
            v_prev = (np.float32(0.0) if y == 0 else neg) if x == 0 else v[x - 1][y - 1]
            v[x][y] = np.float32(v[x][y] + max(v_prev, v_cur))
    path = np.zeros(value.shape, np.int32)
    index = tx - 1
    for y in range(ty - 1, -1, -1):
        path[index, y] = 1
        if y > 0 and index != 0 and (index == y or v[index][y - 1] < v[index - 1][y - 1]):
            index -= 1
    return path


def monotonic_paths(tx, ty):
    """Every row sequence r[0..ty-1] with r[0] = 0, r[ty-1] = tx-1 and steps of 0 or +1."""
    for steps in itertools.combinations(range(1, ty), tx - 1):
        rows, r, s = [], 0, set(steps)
        for y in range(ty):
            if y in s:
                r += 1
            rows.append(r)
        yield rows


def brute_force(value, tx, ty):
    """The best monotonic path in exact (float64) arithmetic; among equal scores the one MAS's backtrack takes: staying on the
    row wins a tie, i.e. the row sequence read from the last frame backwards is the largest."""
    best = None
    for rows in monotonic_paths(tx, ty):
        score = sum(float(value[r, y]) for y, r in enumerate(rows))
        key = (score, tuple(reversed(rows)))
        if best is None or key > best[0]:
            best = (key, rows)
    path = np.zeros(value.shape, np.int32)
    for y, r in enumerate(best[1]):
        path[r, y] = 1
    return path


@pytest.mark.parametrize("seed", range(6))
def test_mas_numpy_finds_the_best_monotonic_path(seed):
    rng = np.random.default_rng(seed)
    for _ in range(12):
        tx = int(rng.integers(1, 6))
        ty = int(rng.integers(tx, 10))
        value = rng.standard_normal((tx + 2, ty + 3)).astype(np.float32)     # padding beyond (tx, ty) must be ignored
        got = M.maximum_path_each(value, tx, ty)
        np.testing.assert_array_equal(got, brute_force(value, tx, ty))
        np.testing.assert_array_equal(got, scalar_mas(value, tx, ty))
        assert got[:tx, :ty].sum(0).tolist() == [1] * ty and got[tx:].sum() == 0 and got[:, ty:].sum() == 0


@pytest.mark.parametrize("seed", range(4))
def test_mas_numpy_tie_rule(seed):
    """Small integers make many paths score exactly the same: the backtrack's strict comparison keeps the row on a tie."""
    rng = np.random.default_rng(100 + seed)
    for _ in range(15):
        tx = int(rng.integers(2, 6))
        ty = int(rng.integers(tx, 9))
        value = rng.integers(-1, 2, size=(tx, ty)).astype(np.float32)
        got = M.maximum_path_each(value, tx, ty)
        np.testing.assert_array_equal(got, brute_force(value, tx, ty))
        np.testing.assert_array_equal(got, scalar_mas(value, tx, ty))
    flat = np.zeros((3, 6), np.float32)          # all paths tie: stay on each row as long as possible walking back
    np.testing.assert_array_equal(M.maximum_path_each(flat, 3, 6).argmax(0), [0, 1, 2, 2, 2, 2])


def test_mas_numpy_degenerate_items():
    """tx > ty (more symbols than frames): no monotonic path exists; the algorithm's sweep visits nothing and its walk compares
    input values.  mas_numpy must do exactly what the algorithm does."""
    rng = np.random.default_rng(7)
    for tx, ty in [(3, 1), (4, 2), (7, 3), (9, 8), (2, 1)]:
        value = rng.standard_normal((tx + 1, ty + 2)).astype(np.float32)
        got = M.maximum_path_each(value, tx, ty)
        np.testing.assert_array_equal(got, scalar_mas(value, tx, ty))
        assert got[:, :ty].sum(0).tolist() == [1] * ty
    assert M.maximum_path_each(np.zeros((3, 3), np.float32), 0, 3).sum() == 0


def test_mas_numpy_masked_call_form():
    rng = np.random.default_rng(3)
    B, Tx, Ty = 3, 5, 9
    xl, yl = np.array([5, 2, 4]), np.array([9, 6, 4])
    mask = (np.arange(Tx)[None, :, None] < xl[:, None, None]) & (np.arange(Ty)[None, None, :] < yl[:, None, None])
    value = rng.standard_normal((B, Tx, Ty)).astype(np.float32)
    got = M.maximum_path_masked(value, mask.astype(np.float32))
    for b in range(B):
        np.testing.assert_array_equal(got[b], M.maximum_path_each(value[b], xl[b], yl[b]))
    assert (got * ~mask).sum() == 0


def test_abi_exports_the_tts_train_symbols():
    lib = C.CDLL(_build.build_library())
    for s in ("us_mas_log_prior", "us_maximum_path", "us_maximum_path_workspace_bytes", "us_duration_loss"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


def test_maximum_path_workspace_is_needed_only_beyond_lds():
    lib = _lib.load()
    assert lib.us_maximum_path_workspace_bytes(32, 512, 2048) == 0        # 512 x 64 words: the table fits in LDS
    assert lib.us_maximum_path_workspace_bytes(32, 300, 900) == 0
    assert lib.us_maximum_path_workspace_bytes(4, 1000, 2048) == 4 * 1000 * 64 * 4
    assert lib.us_maximum_path_workspace_bytes(0, 10, 10) == 0


def test_maximum_path_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.us_maximum_path(None, None, None, None, None, 1, 4, 4, None, 0, None) == -1
    p = C.c_void_p(16)            # never dereferenced: refused on shape / workspace before a launch
    assert lib.us_maximum_path(p, p, p, p, p, 1, 1025, 8, None, 0, None) == -1
    assert lib.us_maximum_path(p, p, p, p, p, 2, 1000, 2048, None, 0, None) == -5
    assert lib.us_mas_log_prior(p, p, p, p, p, 1, 0, 4, 4, None) == -1
    assert lib.us_duration_loss(p, p, p, p, None, None, 1, 4, None) == -1


def test_save_pretrained_checkpoint_writes_the_trainer_layout(tmp_path):
    """The writer's file equals, key for key and tensor for tensor, the trainer-layout file the reference itself wrote
    (train_STEP1.py:297-304), and load_decoder_checkpoint reads it back."""
    import torch
    from unitspeech_amd.checkpoint import build_decoder, load_decoder_checkpoint, save_pretrained_checkpoint
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_pretrained_small.pt")
    ref = torch.load(golden, map_location="cpu", weights_only=True)
    ck = load_decoder_checkpoint(golden)
    emb = torch.nn.Embedding(*ref["spk_emb"]["weight"].shape)
    emb.load_state_dict(ref["spk_emb"])
    path = str(tmp_path / "pretrained_decoder.pt")
    save_pretrained_checkpoint(path, build_decoder(ck), emb, ref["mel_min"], ref["mel_max"], ref["iteration"])
    got = torch.load(path, map_location="cpu", weights_only=True)
    assert list(got) == list(ref) == ["model", "spk_emb", "mel_min", "mel_max", "iteration"]
    assert list(got["model"]) == list(ref["model"]) and list(got["spk_emb"]) == ["weight"]
    for k in ref["model"]:
        assert torch.equal(got["model"][k], ref["model"][k]), k
    assert torch.equal(got["spk_emb"]["weight"], ref["spk_emb"]["weight"])
    assert float(got["mel_min"]) == float(ref["mel_min"]) and float(got["mel_max"]) == float(ref["mel_max"])
    assert got["iteration"] == ref["iteration"]
    back = load_decoder_checkpoint(path)
    assert back.iteration == ck.iteration and torch.equal(back.speaker_embedding(2), ck.speaker_embedding(2))
