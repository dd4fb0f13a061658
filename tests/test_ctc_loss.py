"""Host side of fitting the CTC head (tools/ctc_loss_numpy.py, unitspeech_amd/asr.py, csrc/ctc_train.hip's host functions): the fp64
numpy yardstick against torch's fp64 CPU path, finite differences and a brute-force enumeration of all paths; the tie rule on hand-built
ties; the C ABI's new symbols; the refusals.  No device work is launched here."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_loss_numpy as Y  # noqa: E402

from unitspeech_amd import _build, _lib, asr  # noqa: E402

SYMBOLS = ["us_ctc_loss_workspace_bytes", "us_ctc_loss", "us_ctc_head_backward_workspace_bytes", "us_ctc_head_backward",
           "us_ctc_align_workspace_bytes", "us_ctc_forced_align"]


def torch_fp64(logits, targets, frame_lengths, target_lengths, blank):
    """torch's CPU path in fp64: log_softmax, ctc_loss (zero_infinity, so that an infeasible item is 0 with a zero gradient), autograd."""
    x = torch.from_numpy(np.asarray(logits, dtype=np.float64)).requires_grad_(True)
    loss = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), torch.as_tensor(targets), torch.as_tensor(frame_lengths),
                      torch.as_tensor(target_lengths), blank=blank, reduction="none", zero_infinity=True)
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


# (blank, T, V, frame lengths, targets): ragged frames, L = 0, repeated labels, an item at its minimum feasible T and an infeasible one
CASES = [
    (0, 12, 5, [12, 7, 9, 5, 4, 3], [[1, 2, 3], [4, 4], [], [2, 2, 1, 1], [1, 2, 2], [1, 1, 3]]),       # item 4: T = L + 1; item 5: 3 < 4
    (4, 9, 5, [9, 9, 1, 6], [[0, 1, 0, 1], [3, 3, 3], [2], [0, 1, 2, 3, 3]]),                           # blank = V - 1; item 3: 6 = 5 + 1
    (2, 20, 7, [20, 0, 15], [[0, 1, 3, 4, 5, 6, 6, 0, 1], [], [6]]),                                   # blank in the middle; T = 0 with L = 0
]


@pytest.mark.parametrize("blank,T,V,flen,tg", CASES)
def test_yardstick_equals_torch_fp64(blank, T, V, flen, tg):
    g = np.random.Generator(np.random.Philox(key=7 * T + V))
    B, Lmax = len(tg), max(1, max(len(t) for t in tg))
    logits = g.normal(size=(B, T, V)) * 2.0
    targets = np.full((B, Lmax), (blank + 1) % V, dtype=np.int64)
    for b, t in enumerate(tg):
        targets[b, :len(t)] = t
    tlen = np.array([len(t) for t in tg], dtype=np.int64)
    loss, grad = Y.ctc_loss_batch(logits, targets, flen, tlen, blank, zero_infinity=True)
    rl, rg = torch_fp64(logits, targets, np.array(flen, dtype=np.int64), tlen, blank)
    np.testing.assert_allclose(loss, rl, rtol=1e-10, atol=0)
    np.testing.assert_allclose(grad, rg, rtol=1e-10, atol=1e-10 * np.abs(rg).max())
    for b in range(B):
        assert not grad[b, flen[b]:].any()
    # without zero_infinity an item with no path is +inf, and only such an item
    raw, _ = Y.ctc_loss_batch(logits, targets, flen, tlen, blank)
    for b, t in enumerate(tg):
        need = len(t) + sum(1 for i in range(1, len(t)) if t[i] == t[i - 1])
        assert np.isinf(raw[b]) == (flen[b] < need), b
    for red in ("none", "sum", "mean"):
        want = F.ctc_loss(F.log_softmax(torch.from_numpy(logits), -1).transpose(0, 1), torch.from_numpy(targets), torch.tensor(flen),
                          torch.from_numpy(tlen), blank=blank, reduction=red, zero_infinity=True).numpy()
        np.testing.assert_allclose(Y.reduce_loss(loss, tlen, red), want, rtol=1e-10)


def test_yardstick_gradient_by_finite_differences():
    g = np.random.Generator(np.random.Philox(key=3))
    T, V, tgt, blank = 6, 4, [1, 1, 2], 3
    x = g.normal(size=(T, V))
    _, grad = Y.ctc_loss(x, tgt, blank)
    h = 1e-6
    num = np.zeros_like(x)
    for t in range(T):
        for v in range(V):
            d = np.zeros_like(x)
            d[t, v] = h
            num[t, v] = (Y.ctc_loss(x + d, tgt, blank)[0] - Y.ctc_loss(x - d, tgt, blank)[0]) / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=0, atol=1e-8)           # central differences: O(h^2) + rounding / h


def collapse(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def test_alignment_score_equals_brute_force():
    g = np.random.Generator(np.random.Philox(key=11))
    V, blank = 4, 0
    n = 0
    for T in range(1, 8):
        for tgt in ([], [1], [2, 2], [1, 3], [3, 3, 3], [1, 2, 1], [2, 2, 3]):
            scores = -g.integers(0, 32, size=(T, V)) / 8.0              # multiples of 1 / 8: sums are exact and ties happen
            best = -np.inf
            for p in itertools.product(range(V), repeat=T):
                if collapse(p, blank) == tgt:
                    best = max(best, float(scores[np.arange(T), list(p)].sum()))
            path, score, start, frames = Y.forced_align(scores, tgt, blank)
            assert score == best, (T, tgt)
            if np.isfinite(best):
                n += 1
                assert collapse(path.tolist(), blank) == tgt and float(scores[np.arange(T), path].sum()) == score
                for i, v in enumerate(tgt):
                    assert frames[i] >= 1 and (path[start[i]:start[i] + frames[i]] == v).all()
                    assert start[i] == 0 or path[start[i] - 1] != v
            else:
                assert (path == -1).all() and not frames.any()
    assert n > 30


def test_alignment_tie_rule_on_hand_built_ties():
    z = np.zeros((4, 3))
    # every path scores 0.  The end: the last label, not the final blank.  Backwards: stay as long as the state is reachable.
    path, score, start, frames = Y.forced_align(z, [1], 0)
    assert path.tolist() == [1, 1, 1, 1] and score == 0 and start.tolist() == [0] and frames.tolist() == [4]
    path, _, start, frames = Y.forced_align(z, [1, 2], 0)
    assert path.tolist() == [1, 2, 2, 2] and start.tolist() == [0, 1] and frames.tolist() == [1, 3]
    # a repeated label needs the blank between: state 3 is first reachable at frame 2, through the blank at frame 1
    path, _, start, frames = Y.forced_align(z, [1, 1], 0)
    assert path.tolist() == [1, 0, 1, 1] and start.tolist() == [0, 2] and frames.tolist() == [1, 2]
    path, _, _, _ = Y.forced_align(z, [], 0)
    assert path.tolist() == [0, 0, 0, 0]
    # s - 1 wins over s - 2: at frame 1 state 3 (label 2) is reached from the blank (state 2)?  It is not reachable at frame 0, so the only
    # tie of that kind is at frame 2: state 3 from state 2 (blank at frame 1) or from state 1 (label 1 at frame 1)
    s = np.zeros((3, 3))
    s[2, 0] = s[2, 1] = -1.0                                           # the last frame must be label 2
    s[0, 0] = -1.0                                                     # the first frame must be label 1
    s[1, 2] = -1.0                                                     # frame 1 is label 1 or the blank: a tie between s - 2 and s - 1
    path, score, _, _ = Y.forced_align(s, [1, 2], 0)
    assert path.tolist() == [1, 0, 2] and score == 0
    # the final blank wins only when it is strictly better
    e = np.zeros((2, 2))
    e[1, 1] = -0.5
    assert Y.forced_align(e, [1], 0)[0].tolist() == [1, 0]
    assert np.isinf(Y.forced_align(np.zeros((2, 3)), [1, 1], 0)[1])      # infeasible: 2 frames for 1 _ 1


def test_symbols_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "unitspeech_hip.h")).read()
    assert "staying in s wins over s - 1" in txt                       # the tie rule is part of the header's contract
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(us_[a-z_0-9]+)\s*\(", txt))
    lib = C.CDLL(_build.build_library())
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert "ctc_train.hip" in _build.SOURCES and "ctc.hip" in _build.SOURCES
    assert {"ctc_loss", "forced_align", "CTCHead", "HubertForCTC", "Wav2Vec2ForCTC"} <= set(asr.__all__)


def test_size_functions_and_refusals_without_a_device():
    lib = _lib.load()
    stat = 4 * 64 * 8 + 256                                             # (max, logsumexp) per row and a log-likelihood per item, in 256-byte units
    assert lib.us_ctc_loss_workspace_bytes(4, 64, 10, 0) == stat
    assert lib.us_ctc_loss_workspace_bytes(4, 64, 10, 1) == stat + 4 * 64 * 21 * 8
    assert lib.us_ctc_loss_workspace_bytes(4, 50, 10, 0) == 1792 + 256
    assert lib.us_ctc_loss_workspace_bytes(1, 1, 0, 1) == 256 + 256 + 8
    assert lib.us_ctc_align_workspace_bytes(2, 30, 10) == 2 * 30 * 64 * 4 and lib.us_ctc_align_workspace_bytes(2, 30, 1024) == 2 * 30 * 256 * 4
    assert lib.us_ctc_head_backward_workspace_bytes(1, 150, 12, 8) == 3 * (12 * 8 + 12) * 4          # chunks of 64 rows
    assert lib.us_ctc_head_backward_workspace_bytes(64, 256, 32, 768) == 64 * (32 * 768 + 32) * 4   # never more than 64 chunks
    for fn, args in ((lib.us_ctc_loss_workspace_bytes, (1, 10, 1025, 0)), (lib.us_ctc_loss_workspace_bytes, (0, 10, 4, 0)),
                     (lib.us_ctc_align_workspace_bytes, (1, 10, 1025)), (lib.us_ctc_align_workspace_bytes, (1, 0, 4)),
                     (lib.us_ctc_head_backward_workspace_bytes, (1, 10, 1, 8)), (lib.us_ctc_head_backward_workspace_bytes, (1, 10, 4, 6)),
                     (lib.us_ctc_head_backward_workspace_bytes, (1, 10, 2049, 8)), (lib.us_ctc_head_backward_workspace_bytes, (1, 10, 4, 1028))):
        assert fn(*args) == 0, args
    # the size checks come before any launch
    assert lib.us_ctc_loss(None, None, None, None, None, 1, 10, 4, 1025, 0, 0, 0, None, None, None, 0, None) == -1
    assert b"1024" in lib.us_last_error(None)
    assert lib.us_ctc_forced_align(None, None, None, None, 1, 10, 4, 1025, 0, None, None, None, None, None, 0, None) == -1
    assert b"1024" in lib.us_last_error(None)
    assert lib.us_ctc_loss(None, None, None, None, None, 1, 10, 4, 2, 4, 0, 0, None, None, None, 0, None) == -1
    assert b"blank" in lib.us_last_error(None)
    for stage in (3, -1, _lib.US_CTC_BACKWARD):                         # no such stage; the backward stage without grad_logits
        assert lib.us_ctc_loss(None, None, None, None, None, 1, 10, 4, 2, 0, 0, stage, None, None, None, 0, None) == -1
        assert b"stage" in lib.us_last_error(None)
    assert lib.us_ctc_head_backward(None, None, None, None, 1, 10, 4, 6, None, None, None, None, 0, None) == -1
    assert b"H a multiple of 4" in lib.us_last_error(None)


def test_cpu_refusals_are_todays():
    x, tg, n = torch.zeros(1, 3, 4), torch.ones(1, 1, dtype=torch.int64), torch.tensor([1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.ctc_loss(x, tg, torch.tensor([3]), n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.forced_align(x, tg, torch.tensor([3]), n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.CTCHead(8, 4, trainable=True)(torch.zeros(1, 3, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asr.CTCHead(8, 4)(torch.zeros(1, 3, 8))
    with pytest.raises(ValueError):
        asr.ctc_loss(x, tg, torch.tensor([3]), n, reduction="batchmean")


def test_default_head_is_unchanged():
    head = asr.CTCHead(8, 4)
    assert list(head.state_dict().keys()) == ["weight", "bias"]
    assert not head.weight.requires_grad and not head.bias.requires_grad and not head.trainable
    fit = asr.CTCHead(8, 4, trainable=True)
    assert list(fit.state_dict().keys()) == ["weight", "bias"] and fit.weight.requires_grad and fit.bias.requires_grad
    import evaluate
    model = asr.HubertForCTC(**dict(evaluate.TINY, trainable=True))
    assert model.lm_head.trainable and [n for n, p in model.named_parameters() if p.requires_grad] == ["lm_head.weight", "lm_head.bias"]
    assert not asr.HubertForCTC(**evaluate.TINY).lm_head.trainable
