"""Fitting the CTC head on the GPU (csrc/ctc_train.hip, unitspeech_amd/asr.py, train_ctc_head.py) against the fp64 numpy yardstick
(tools/ctc_loss_numpy.py).

Loss and gradient.  The bar follows the inputs: torch's own fp32 CPU path (log_softmax, ctc_loss, autograd) is compared with its fp64
path on the same logits, and the library must be within TWICE that error of the yardstick (a different but equally valid summation order
can double a rounding error), with a floor of 1e-6 absolute on gradients and 1e-6 relative on losses for the cases where the fp32
reference happens to be exact.  Every test prints both errors.

A case (B, T, V, L) is B regular items of L tokens (the first at the full T frames, the others at 0.6 T, the second with a repeated pair)
followed by three special ones: L = 0; an item at exactly its minimum feasible T; an infeasible item, one frame short of that.

Head backward.  dW, db and dX against fp64 matmuls of the same operands, elementwise within K * 2^-23 * sum |a_i| |b_i|: the bound of
a length-K fp32 chain with a factor of 2 of slack; K is the number of live rows for dW and db, and V for dX.

Alignment.  On scores that are multiples of 2^-6 in [-8, 0] every path sum is exact in fp32 and fp64 alike and ties do occur: path,
score, start and frames must then equal the yardstick's exactly."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_loss_numpy as Y  # noqa: E402

import evaluate  # noqa: E402
from unitspeech_amd import _lib, asr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(4, 50, 12, 10), (3, 120, 37, 40), (2, 300, 32, 150)]      # S = 21; S = 81 crosses a wave, V no multiple of 64; S = 301 crosses the stride


def need_frames(t):
    return len(t) + sum(1 for i in range(1, len(t)) if t[i] == t[i - 1])


@functools.lru_cache(maxsize=None)
def case(B, T, V, L, blank):
    """-> dict of the case's host arrays and its three references (yardstick fp64, torch fp64, torch fp32), computed once."""
    g = np.random.Generator(np.random.Philox(key=1000 * T + 10 * V + (blank != 0)))
    entries = np.array([v for v in range(V) if v != blank])
    tgs = [entries[g.integers(0, V - 1, size=L)].tolist() for _ in range(B)]
    tgs[1][1] = tgs[1][0]                                            # one repeated pair
    flen = [T] + [int(0.6 * T)] * (B - 1)
    short = entries[g.integers(0, V - 1, size=max(3, L // 2))].tolist()
    short[2] = short[1]
    tgs += [[], list(short), list(short)]
    flen += [int(0.6 * T), need_frames(short), need_frames(short) - 1]
    n = len(tgs)
    targets = np.full((n, L), entries[0], dtype=np.int64)
    for b, t in enumerate(tgs):
        targets[b, :len(t)] = t
    tlen = np.array([len(t) for t in tgs], dtype=np.int64)
    flen = np.array(flen, dtype=np.int64)
    logits = (2.0 * g.standard_normal((n, T, V))).astype(np.float32)
    loss64, grad64 = Y.ctc_loss_batch(logits, targets, flen, tlen, blank)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x = torch.from_numpy(logits).to(dt).requires_grad_(True)
        l = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(targets), torch.from_numpy(flen), torch.from_numpy(tlen),
                       blank=blank, reduction="none", zero_infinity=True)
        l.sum().backward()
        ref[dt] = (l.detach().double().numpy(), x.grad.double().numpy())
    feasible = np.isfinite(loss64)
    assert feasible.tolist() == [True] * (n - 1) + [False]
    # the yardstick and torch's fp64 agree far below anything compared here
    np.testing.assert_allclose(loss64[feasible], ref[torch.float64][0][feasible], rtol=1e-10)
    np.testing.assert_allclose(grad64, ref[torch.float64][1], rtol=1e-9, atol=1e-12)
    return dict(logits=logits, targets=targets, flen=flen, tlen=tlen, loss64=loss64, grad64=grad64, feasible=feasible,
                torch_loss_err=float(np.max(np.abs(ref[torch.float32][0] - ref[torch.float64][0])[feasible] / ref[torch.float64][0][feasible])),
                torch_grad_err=float(np.abs(ref[torch.float32][1] - ref[torch.float64][1]).max()))


def run(c, blank, idx=None, zero_infinity=False):
    """The library's (loss [n], grad [n, T, V]) for the case, or for item `idx` alone, cut to its own frames and tokens."""
    if idx is None:
        x, tg, fl, tl = c["logits"], c["targets"], c["flen"], c["tlen"]
    else:
        T, L = int(c["flen"][idx]), int(c["tlen"][idx])
        x, tg, fl, tl = c["logits"][idx:idx + 1, :T], c["targets"][idx:idx + 1, :L], c["flen"][idx:idx + 1], c["tlen"][idx:idx + 1]
    x = torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(True)
    loss = asr.ctc_loss(x, torch.from_numpy(np.ascontiguousarray(tg)).cuda(), torch.from_numpy(fl).cuda(), torch.from_numpy(tl).cuda(),
                        blank=blank, reduction="none", zero_infinity=zero_infinity)
    loss.backward(torch.ones_like(loss))
    return loss.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("B,T,V,L", SHAPES)
def test_loss_and_gradient_against_the_yardstick(B, T, V, L, blank_last):
    blank = V - 1 if blank_last else 0
    c = case(B, T, V, L, blank)
    loss, grad = run(c, blank)
    ok = c["feasible"]
    loss_err = float(np.max(np.abs(loss.double().numpy()[ok] - c["loss64"][ok]) / c["loss64"][ok]))
    grad_err = float(np.abs(grad.double().numpy() - c["grad64"]).max())
    print(f"B{B} T{T} V{V} L{L} blank {blank}: loss rel err library {loss_err:.3e} torch fp32 {c['torch_loss_err']:.3e} | "
          f"grad abs err library {grad_err:.3e} torch fp32 {c['torch_grad_err']:.3e} | max loss {c['loss64'][ok].max():.1f}")
    assert loss_err <= max(2 * c["torch_loss_err"], 1e-6)
    assert grad_err <= max(2 * c["torch_grad_err"], 1e-6)
    # exact: the infeasible item, the rows beyond the frames, the second run
    assert torch.isposinf(loss[-1]) and not grad[-1].any()
    for b, n in enumerate(c["flen"]):
        assert not grad[b, n:].any(), b
    loss2, grad2 = run(c, blank)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    lz, gz = run(c, blank, zero_infinity=True)
    assert lz[-1] == 0 and torch.equal(lz[:-1], loss[:-1]) and torch.equal(gz, grad)


@pytest.mark.parametrize("B,T,V,L", SHAPES)
def test_item_alone_has_the_bits_it_has_in_the_batch(B, T, V, L):
    c = case(B, T, V, L, 0)
    loss, grad = run(c, 0)
    for b in range(len(c["flen"])):
        la, ga = run(c, 0, idx=b)
        n = int(c["flen"][b])
        assert torch.equal(la[0], loss[b]) and torch.equal(ga[0], grad[b, :n]), b


def test_whole_call_has_the_bits_of_forward_then_backward():
    """`asr.ctc_loss` splits the library's call in two around autograd (US_CTC_FORWARD keeps alpha, US_CTC_BACKWARD runs the backward sweep
    with the incoming gradient); the one-call form, US_CTC_WHOLE with grad_logits, must write the same loss and gradient."""
    B, T, V, L = SHAPES[1]
    c = case(B, T, V, L, 0)
    loss, grad = run(c, 0)
    x = torch.from_numpy(c["logits"]).cuda()
    tg, fl, tl = (torch.from_numpy(c[k]).cuda() for k in ("targets", "flen", "tlen"))
    go = torch.linspace(0.5, 2.0, len(c["flen"])).cuda()
    lw, gw, _ = asr._ctc_loss_call(x, tg, fl, tl, 0, False, _lib.US_CTC_WHOLE, None, None, with_grad=True)
    assert torch.equal(lw.cpu(), loss) and torch.equal(gw.cpu(), grad)
    _, gs, _ = asr._ctc_loss_call(x, tg, fl, tl, 0, False, _lib.US_CTC_WHOLE, go, None, with_grad=True)
    xs = x.clone().requires_grad_(True)
    asr.ctc_loss(xs, tg, fl, tl, reduction="none").backward(go)
    assert torch.equal(gs, xs.grad) and not torch.equal(gs, gw)


def test_reductions_are_torchs():
    B, T, V, L = SHAPES[0]
    c = case(B, T, V, L, 0)
    x = torch.from_numpy(c["logits"]).cuda()
    args = (torch.from_numpy(c["targets"]).cuda(), torch.from_numpy(c["flen"]).cuda(), torch.from_numpy(c["tlen"]).cuda())
    for zi in (True, False):
        for red in ("none", "sum", "mean"):
            want = F.ctc_loss(F.log_softmax(torch.from_numpy(c["logits"]).double(), -1).transpose(0, 1), torch.from_numpy(c["targets"]),
                              torch.from_numpy(c["flen"]), torch.from_numpy(c["tlen"]), blank=0, reduction=red, zero_infinity=zi)
            got = asr.ctc_loss(x, *args, blank=0, reduction=red, zero_infinity=zi).double().cpu()
            assert got.shape == want.shape
            fin = torch.isfinite(want) & (want != 0)
            assert torch.equal(torch.isposinf(got), torch.isposinf(want))           # without zero_infinity the infeasible item is +inf
            assert torch.equal(got == 0, want == 0)                                 # and with it exactly 0
            err = float(((got - want)[fin].abs() / want[fin].abs()).max()) if fin.any() else 0.0
            print(f"reduction {red} zero_infinity {zi}: rel err {err:.3e}")
            assert err <= max(2 * c["torch_loss_err"], 1e-6)
    # the mean's gradient is the per-item gradient scaled by 1 / (clamp(L, 1) * n): grad_out reaches the kernel
    xg = x.clone().requires_grad_(True)
    asr.ctc_loss(xg, *args, blank=0, reduction="mean", zero_infinity=True).backward()
    _, grad = run(c, 0)
    scale = 1.0 / (np.maximum(c["tlen"], 1) * len(c["tlen"]))
    want = grad.double().numpy() * scale[:, None, None]
    assert np.abs(xg.grad.double().cpu().numpy() - want).max() <= 2.0 ** -22 * np.abs(want).max()


# ---- the head's backward ----------------------------------------------------------------------------------------------------------
# (B, F, V, H, lengths): H = 8; 150 rows (three chunks of 64, the last partial) at H = 72, no multiple of 16, with an empty item; V over
# three vocabulary tiles with a partial reduction slice for dX, H over three tiles
HEAD_CASES = [(2, 40, 12, 8, [40, 25]), (3, 50, 37, 72, [50, 0, 31]), (2, 70, 130, 136, [70, 64])]


def head_backward(g, x, lens, w, want_dx=True):
    B, Fr, V = g.shape
    H = x.shape[-1]
    lib = _lib.load()
    n = int(lib.us_ctc_head_backward_workspace_bytes(B, Fr, V, H))
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    dw, db = torch.full((V, H), float("nan"), device="cuda"), torch.full((V,), float("nan"), device="cuda")
    dx = torch.full((B, Fr, H), float("nan"), device="cuda") if want_dx else None
    rc = lib.us_ctc_head_backward(g.data_ptr(), x.data_ptr(), lens.data_ptr(), w.data_ptr(), B, Fr, V, H, dw.data_ptr(), db.data_ptr(),
                                  None if dx is None else dx.data_ptr(), ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, None, "us_ctc_head_backward")
    return dw, db, dx


@pytest.mark.parametrize("B,Fr,V,H,lens", HEAD_CASES)
def test_head_backward_against_fp64(B, Fr, V, H, lens):
    gen = torch.Generator().manual_seed(100 * H + V)
    g, x, w = torch.randn(B, Fr, V, generator=gen), torch.randn(B, Fr, H, generator=gen), torch.randn(V, H, generator=gen)
    live = torch.zeros(B, Fr, dtype=torch.bool)
    for b, n in enumerate(lens):
        live[b, :n] = True
    g64, x64 = (g.double() * live[..., None]).reshape(-1, V), (x.double() * live[..., None]).reshape(-1, H)
    gd, xd = g.clone(), x.clone()
    gd[~live], xd[~live] = float("nan"), float("nan")               # rows beyond an item's frames are never read
    args = (gd.cuda(), xd.cuda(), torch.tensor(lens, dtype=torch.int64).cuda(), w.cuda())
    dw, db, dx = head_backward(*args)
    K = int(live.sum())
    u = 2.0 ** -23
    for tag, got, want, bound in (("dW", dw, g64.T @ x64, K * u * (g64.abs().T @ x64.abs())), ("db", db, g64.sum(0), K * u * g64.abs().sum(0)),
                                  ("dX", dx.reshape(-1, H), g64 @ w.double(), V * u * (g64.abs() @ w.double().abs()))):
        err = (got.double().cpu() - want).abs()
        print(f"{tag} V{V} H{H} rows {B * Fr} live {K}: max err {float(err.max()):.3e}  smallest bound/err margin "
              f"{float((bound - err).min()):.3e}  max bound {float(bound.max()):.3e}")
        assert torch.isfinite(got).all() and bool((err <= bound).all()), tag
    assert not dx.cpu()[~live].any()                                 # dead rows: exactly 0
    dw2, db2, dx2 = head_backward(*args)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dx, dx2)
    dw3, db3, none = head_backward(*args, want_dx=False)
    assert none is None and torch.equal(dw, dw3) and torch.equal(db, db3)


def test_autograd_chains_the_two_pieces():
    B, Fr, V, H, lens = 3, 50, 12, 40, [50, 0, 31]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, Fr, H, generator=gen).cuda()
    head = asr.CTCHead(H, V, trainable=True)
    head.load_state_dict({"weight": 0.3 * torch.randn(V, H, generator=gen), "bias": 0.1 * torch.randn(V, generator=gen)})
    head = head.cuda()
    fl = torch.tensor(lens, dtype=torch.int64).cuda()
    tg = torch.randint(1, V, (B, 6), generator=gen).cuda()
    tl = torch.tensor([6, 0, 4], dtype=torch.int64).cuda()
    # the default head's forward bits are the trainable head's
    frozen = asr.CTCHead(H, V)
    frozen.load_state_dict(head.state_dict())
    frozen = frozen.cuda()
    logits = head(x, fl)
    assert logits.requires_grad and torch.equal(logits, frozen(x, fl)) and not frozen(x, fl).requires_grad
    with torch.no_grad():
        assert not head(x, fl).requires_grad
    asr.ctc_loss(logits, tg, fl, tl).backward()
    assert x.grad is None
    # piece by piece: the loss's gradient in the logits, then the head's backward of it
    leaf = logits.detach().clone().requires_grad_(True)
    asr.ctc_loss(leaf, tg, fl, tl).backward()
    dw, db, dx = head_backward(leaf.grad, x, fl, head.weight.detach())
    assert torch.equal(head.weight.grad, dw) and torch.equal(head.bias.grad, db)
    # the features get a gradient only when they ask for one
    head.zero_grad()
    xr = x.clone().requires_grad_(True)
    asr.ctc_loss(head(xr, fl), tg, fl, tl).backward()
    assert torch.equal(xr.grad, dx) and torch.equal(head.weight.grad, dw)
    # and a frozen-parameter trainable head still passes the gradient on
    lp_logits, lp = head(xr, fl, log_probs=True)
    assert lp_logits.requires_grad and not lp.requires_grad and torch.equal(lp, frozen(x, fl, log_probs=True)[1])


def test_synthetic_training_lowers_the_loss(tmp_path):
    import train_ctc_head
    out = tmp_path / "ctc.pt"
    hist = train_ctc_head.main(["--synthetic", "8", "--batch", "8", "--epochs", "30", "--steps", "30", "--out", str(out)])
    print([round(h["loss"], 4) for h in hist], [round(h["cer"], 3) for h in hist])
    assert len(hist) == 30 and hist[-1]["steps"] == 30
    assert all(np.isfinite(h["loss"]) for h in hist) and hist[-1]["loss"] < hist[0]["loss"]
    model = asr.load_ctc_checkpoint(str(out), **evaluate.TINY)
    assert type(model) is asr.HubertForCTC and model.vocab_size == len(evaluate.TINY_VOCAB)
    assert model.lm_head.weight.abs().sum() > 0 and not model.lm_head.weight.requires_grad


def test_model_loss_and_align():
    model, vocabulary = evaluate.synthetic_model(torch.device("cuda"), 0)
    items = evaluate.synthetic_waves(3, 0)
    res = {}
    wavs = [evaluate.to_16k(w, r, torch.device("cuda"), res) for _, w, r in items]
    x, n = evaluate.padded_batch(wavs, [0, 1, 2])
    tokens, count = model.transcribe_ids(x, n)
    L = int(count.max())
    tg = tokens[:, :max(L, 1)].clone()
    tg[tg == 0] = 1                                                  # the padding beyond count: any entry but the blank
    loss = model.loss(x, n, tg, count, reduction="none")
    assert loss.shape == (3,) and torch.isfinite(loss).all() and not loss.requires_grad           # the default head does not train
    path, score, start, frames = model.align(x, n, tg, count)
    # the greedy path is the best path of its own collapse: the alignment reproduces the argmax ids
    _, ids = model.lm_head.argmax(model.encoder(x, n), model._frames(x, n)[1])
    assert torch.equal(path, ids) and torch.isfinite(score).all()
    for b in range(3):
        assert int(frames[b, :int(count[b])].min()) >= 1 if int(count[b]) else True


def test_evaluate_timestamps(tmp_path):
    import json
    out = tmp_path / "result.json"
    evaluate.main(["--synthetic", "4", "--batch", "2", "--timestamps", "--out", str(out)])
    with open(out, encoding="utf-8") as f:
        result = json.load(f)
    assert result["files"] == 4
    timed = 0
    for rec in result["per_file"]:
        words = rec["word_times"]
        if words is None:                                            # the edited transcript does not fit the frames: no alignment
            continue
        timed += 1
        assert [w["word"] for w in words] == rec["reference"].split()
        t = 0.0
        for w in words:
            assert t <= w["start"] < w["end"] <= 2.0, w                # seeded waveforms of at most 1.6 s; words in order, none empty
            t = w["end"]
    assert timed >= 1
    evaluate.main(["--synthetic", "2", "--batch", "2", "--out", str(out)])
    with open(out, encoding="utf-8") as f:
        assert all("word_times" not in rec and isinstance(rec["words"], int) for rec in json.load(f)["per_file"])     # without the flag the records are what they were


# ---- alignment --------------------------------------------------------------------------------------------------------------------
def align_case(B, T, V, L, blank, dyadic):
    c = case(B, T, V, L, blank)
    g = np.random.Generator(np.random.Philox(key=77 * T + V + (blank != 0) + 2 * dyadic))
    n = len(c["flen"])
    if dyadic:
        scores = (-g.integers(0, 8 * 64 + 1, size=(n, T, V)) / 64.0).astype(np.float32)        # multiples of 2^-6 in [-8, 0]
        scores[:, :, ::3] = np.round(scores[:, :, ::3])              # coarser still: more ties
    else:
        scores = np.log(g.dirichlet(np.ones(V), size=(n, T))).astype(np.float32)
    return c, scores


def align(c, scores, blank, idx=None):
    if idx is None:
        x, tg, fl, tl = scores, c["targets"], c["flen"], c["tlen"]
    else:
        T, L = int(c["flen"][idx]), int(c["tlen"][idx])
        x, tg, fl, tl = scores[idx:idx + 1, :T], c["targets"][idx:idx + 1, :L], c["flen"][idx:idx + 1], c["tlen"][idx:idx + 1]
    out = asr.forced_align(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(tg)).cuda(),
                           torch.from_numpy(fl).cuda(), torch.from_numpy(tl).cuda(), blank=blank)
    return [o.cpu() for o in out]


@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("B,T,V,L", SHAPES)
def test_alignment_is_the_yardsticks_on_exact_scores(B, T, V, L, blank_last):
    blank = V - 1 if blank_last else 0
    c, scores = align_case(B, T, V, L, blank, True)
    path, score, start, frames = align(c, scores, blank)
    for b in range(len(c["flen"])):
        n, l = int(c["flen"][b]), int(c["tlen"][b])
        p, s, st, fr = Y.forced_align(scores[b, :n], c["targets"][b, :l], blank)
        assert path[b, :n].tolist() == p.tolist() and (path[b, n:] == -1).all(), b
        assert float(score[b]) == s, b
        assert start[b, :l].tolist() == st.tolist() and frames[b, :l].tolist() == fr.tolist(), b
        assert not start[b, l:].any() and not frames[b, l:].any()
    assert torch.isneginf(score[-1]) and (path[-1] == -1).all() and not frames[-1].any()
    # ragged items equal the same items alone
    for b in range(len(c["flen"])):
        pa, sa, sta, fra = align(c, scores, blank, idx=b)
        n, l = int(c["flen"][b]), int(c["tlen"][b])
        assert torch.equal(pa[0], path[b, :n]) and torch.equal(sa[0], score[b]) and torch.equal(sta[0], start[b, :l]) and \
            torch.equal(fra[0], frames[b, :l]), b


@pytest.mark.parametrize("B,T,V,L", SHAPES)
def test_alignment_on_float_scores(B, T, V, L):
    blank = 0
    c, scores = align_case(B, T, V, L, blank, False)
    path, score, start, frames = align(c, scores, blank)
    for b in range(len(c["flen"]) - 1):
        n, l = int(c["flen"][b]), int(c["tlen"][b])
        _, s64, _, _ = Y.forced_align(scores[b, :n], c["targets"][b, :l], blank)
        p = path[b, :n].numpy()
        picked = scores[b, np.arange(n), p]
        # within the bound of a length-n fp32 chain (with the factor of 2) of the best score: the library's path may differ from the
        # yardstick's only where fp32 cannot tell them apart
        bound = n * 2.0 ** -23 * float(np.abs(picked.astype(np.float64)).sum())
        assert abs(float(score[b]) - s64) <= bound, (b, float(score[b]), s64, bound)
        # a valid path: it collapses to the target, and its own sum in frame order is the score, bit for bit
        keep = (p != blank) & np.concatenate(([True], p[1:] != p[:-1]))
        assert p[keep].tolist() == c["targets"][b, :l].tolist(), b
        acc = np.float32(0)
        for v in picked:
            acc = np.float32(acc + v)
        assert float(score[b]) == float(acc), b
        for i in range(l):
            a, k = int(start[b, i]), int(frames[b, i])
            assert k >= 1 and (p[a:a + k] == c["targets"][b, i]).all() and (a == 0 or p[a - 1] != c["targets"][b, i] or frames[b, i - 1] == 0)
        assert (path[b, n:] == -1).all()


def test_refusals():
    x = torch.zeros(2, 8, 5).cuda()
    fl, tl = torch.tensor([8, 8]).cuda(), torch.tensor([2, 2]).cuda()
    long = torch.ones(2, asr.MAX_TARGET + 1, dtype=torch.int64).cuda()
    for fn in (asr.ctc_loss, asr.forced_align):
        with pytest.raises(RuntimeError, match="EINVAL.*at most 1024 tokens"):
            fn(x, long, fl, tl)
        with pytest.raises(ValueError):
            fn(x, long[:, :4], fl[:1], tl)                           # mismatched lengths
        with pytest.raises(ValueError):
            fn(x, long[:, :4], fl, torch.tensor([2, 2, 2]).cuda())
        with pytest.raises(ValueError):
            fn(x, long[:1, :4], fl, tl)
        with pytest.raises(RuntimeError, match="EINVAL"):
            fn(x, long[:, :4], fl, tl, blank=5)
    # a target outside the vocabulary, or the blank itself: NaN for that item alone, nothing read out of bounds
    tg = torch.tensor([[1, 2], [7, 0]]).cuda()
    xg = torch.randn(2, 8, 5).cuda().requires_grad_(True)
    loss = asr.ctc_loss(xg, tg, fl, tl, reduction="none")
    loss.backward(torch.ones_like(loss))
    assert torch.isfinite(loss[0]) and torch.isnan(loss[1]) and not xg.grad[1].any() and xg.grad[0].any()
    assert torch.isnan(asr.forced_align(xg.detach(), tg, fl, tl)[1][1])
    # the largest target is taken
    full = torch.ones(1, asr.MAX_TARGET, dtype=torch.int64).cuda()
    full[0, 1::2] = 2
    big = torch.zeros(1, asr.MAX_TARGET + 5, 5).cuda().requires_grad_(True)
    loss = asr.ctc_loss(big, full, None, torch.tensor([asr.MAX_TARGET]).cuda(), reduction="none")
    loss.backward()
    loss = loss.detach()
    # uniform rows: every one of the C(T + L, 2 L) paths has probability 5^-T
    T, L = asr.MAX_TARGET + 5, asr.MAX_TARGET
    import math
    want = T * math.log(5.0) - math.log(math.comb(T + L, 2 * L))
    print(f"L = 1024 on uniform rows: loss {float(loss[0]):.6f}  closed form {want:.6f}")
    assert abs(float(loss[0]) - want) <= 1e-6 * want and torch.isfinite(big.grad).all()
    assert float(big.grad.sum(-1).abs().max()) <= 1e-5               # softmax - occupancy sums to 0 over a row
