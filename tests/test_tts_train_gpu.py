"""Monotonic alignment search and the duration loss on the MI355X (csrc/tts_train.hip): the log-prior against fp64, the path
bit for bit against tools/mas_numpy.py on the GPU's own log-prior (LDS and workspace decision tables, ragged batches, degenerate
items, exact ties), a planted alignment recovered exactly, and the duration loss with its gradient."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mas_numpy as M  # noqa: E402
from unitspeech_amd import _lib, tts_train  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def masks(x_lengths, y_lengths, Tx, Ty):
    xl, yl = torch.as_tensor(x_lengths), torch.as_tensor(y_lengths)
    xm = (torch.arange(Tx)[None, :] < xl[:, None]).float()[:, None, :]
    ym = (torch.arange(Ty)[None, :] < yl[:, None]).float()[:, None, :]
    return xm, ym


def random_batch(seed, x_lengths, y_lengths, F=80):
    g = torch.Generator().manual_seed(seed)
    B, Tx, Ty = len(x_lengths), max(x_lengths), max(y_lengths)
    mu = torch.randn(B, F, Tx, generator=g)
    y = torch.randn(B, F, Ty, generator=g) * 1.5 + 0.3
    xm, ym = masks(x_lengths, y_lengths, Tx, Ty)
    return mu, y, xm, ym


def log_prior_fp64(mu, y, xm, ym):
    mu, y = mu.double(), y.double()
    F = mu.shape[1]
    lp = (-0.5 * (y ** 2).sum(1)[:, None, :] + torch.einsum("bfx,bfy->bxy", mu, y) - 0.5 * (mu ** 2).sum(1)[:, :, None]
          - 0.5 * math.log(2 * math.pi) * F)
    return lp * (xm.double().transpose(1, 2) * ym.double())


def check_path(lp_gpu, x_lengths, y_lengths):
    attn, dur = tts_train.maximum_path_lengths(lp_gpu, torch.tensor(x_lengths), torch.tensor(y_lengths))
    lp = lp_gpu.cpu().numpy()
    want = M.maximum_path(lp, x_lengths, y_lengths)
    got = attn.cpu().numpy()
    for b in range(len(x_lengths)):
        assert np.array_equal(got[b], want[b]), f"item {b} (tx={x_lengths[b]}, ty={y_lengths[b]}): " \
            f"{int((got[b] != want[b]).sum())} cells differ"
    np.testing.assert_array_equal(dur.cpu().numpy(), want.sum(-1))
    return attn, dur


@pytest.mark.parametrize("shape", [(3, 37, 150), (2, 300, 900), (2, 512, 2048)])
def test_log_prior_matches_fp64(shape):
    B, Tx, Ty = shape
    xl = [Tx] + [max(1, Tx - 7 * i) for i in range(1, B)]
    yl = [Ty] + [max(1, Ty - 31 * i) for i in range(1, B)]
    mu, y, xm, ym = random_batch(1, xl, yl)
    got = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV)).cpu().double()
    want = log_prior_fp64(mu, y, xm, ym)
    rel = (got - want).abs().max() / want.abs().max()
    assert rel < 1e-6, rel
    off = (xm.transpose(1, 2) * ym) == 0
    assert (got[off.expand_as(got)] == 0).all()


@pytest.mark.parametrize("x_lengths,y_lengths", [
    ([5, 1, 7, 3, 4], [12, 9, 20, 2, 4]),                                    # tiny, incl. tx > ty and tx == ty
    ([300, 211, 64, 65, 129, 17, 300, 250], [900, 640, 128, 300, 129, 40, 301, 899]),
    ([512, 480, 333, 511], [2048, 2047, 1500, 700]),                          # decision tables in LDS
])
def test_maximum_path_equals_numpy_exactly(x_lengths, y_lengths):
    mu, y, xm, ym = random_batch(2, x_lengths, y_lengths)
    lp = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV))
    attn, dur = check_path(lp, x_lengths, y_lengths)
    assert attn.sum().item() == sum(y_lengths)


def test_maximum_path_workspace_tables():
    """Items whose decision table does not fit LDS (1000 x 2048: 256 KB) keep it in the workspace; shorter items of the same
    launch still use LDS."""
    x_lengths, y_lengths = [1000, 900, 130, 777], [2048, 1900, 2000, 1100]
    lib = _lib.load()
    assert lib.us_maximum_path_workspace_bytes(4, 1000, 2048) > 0
    mu, y, xm, ym = random_batch(3, x_lengths, y_lengths)
    lp = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV))
    check_path(lp, x_lengths, y_lengths)


def test_maximum_path_ties_and_degenerate_items():
    """Small integer log-priors make many paths tie exactly; tx > ty items walk input values.  Both must match bit for bit."""
    g = torch.Generator().manual_seed(4)
    x_lengths, y_lengths = [6, 40, 70, 9, 128], [30, 40, 200, 4, 1000]
    lp = torch.randint(-1, 2, (5, 128, 1000), generator=g).float()
    check_path(lp.to(DEV), x_lengths, y_lengths)
    check_path(torch.zeros(2, 70, 130, device=DEV), [70, 3], [130, 130])


def test_maximum_path_drop_in_call_form():
    x_lengths, y_lengths = [9, 4, 13], [40, 17, 13]
    mu, y, xm, ym = random_batch(5, x_lengths, y_lengths)
    lp = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV))
    mask = (xm.transpose(1, 2) * ym).to(DEV)
    got = tts_train.maximum_path(lp, mask)
    assert got.dtype == lp.dtype and got.device == lp.device
    np.testing.assert_array_equal(got.cpu().numpy(), M.maximum_path_masked(lp.cpu().numpy(), mask.cpu().numpy()))


def test_planted_alignment_is_recovered_exactly():
    """The mel is mu_x expanded by known durations plus noise: MAS must give those durations back."""
    g = torch.Generator().manual_seed(6)
    B, F, Tx = 6, 80, 60
    x_lengths = [60, 41, 17, 60, 33, 5]
    dur = torch.zeros(B, Tx, dtype=torch.int64)
    for b, n in enumerate(x_lengths):
        dur[b, :n] = torch.randint(1, 9, (n,), generator=g)
    y_lengths = dur.sum(1).tolist()
    Ty = max(y_lengths)
    mu = torch.randn(B, F, Tx, generator=g)
    y = torch.zeros(B, F, Ty)
    for b in range(B):
        idx = torch.repeat_interleave(torch.arange(Tx), dur[b])
        y[b, :, :len(idx)] = mu[b][:, idx] + 0.1 * torch.randn(F, len(idx), generator=g)
    xm, ym = masks(x_lengths, y_lengths, Tx, Ty)
    attn, got = tts_train.align(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV), torch.tensor(x_lengths), torch.tensor(y_lengths))
    np.testing.assert_array_equal(got.cpu().numpy(), dur.float().numpy())


def test_maximum_path_is_deterministic():
    x_lengths, y_lengths = [200, 150], [700, 420]
    mu, y, xm, ym = random_batch(8, x_lengths, y_lengths)
    lp = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV))
    lp2 = tts_train.mas_log_prior(mu.to(DEV), y.to(DEV), xm.to(DEV), ym.to(DEV))
    assert torch.equal(lp, lp2)
    a1, d1 = tts_train.maximum_path_lengths(lp, torch.tensor(x_lengths), torch.tensor(y_lengths))
    a2, d2 = tts_train.maximum_path_lengths(lp2, torch.tensor(x_lengths), torch.tensor(y_lengths))
    assert torch.equal(a1, a2) and torch.equal(d1, d2)


def test_duration_loss_and_gradient():
    g = torch.Generator().manual_seed(9)
    B, Tx = 5, 37
    x_lengths = torch.tensor([37, 20, 1, 30, 12])
    xm = (torch.arange(Tx)[None, :] < x_lengths[:, None]).float()[:, None, :]
    logw = (torch.randn(B, 1, Tx, generator=g) * xm)
    dur = (torch.randint(0, 12, (B, Tx), generator=g).float() * xm[:, 0])
    ref_logw = logw.double().requires_grad_(True)
    logw_ = torch.log(1e-8 + dur.double()[:, None, :]) * xm.double()
    ref = torch.sum((ref_logw - logw_) ** 2) / torch.sum(x_lengths)
    ref.backward()
    lw = logw.to(DEV).requires_grad_(True)
    loss = tts_train.duration_loss(lw, dur.to(DEV), xm.to(DEV), x_lengths.to(DEV))
    (3.0 * loss).backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    err = (lw.grad.cpu().double() - 3.0 * ref_logw.grad).norm() / (3.0 * ref_logw.grad).norm()
    assert err < 1e-6, err
    with pytest.raises(TypeError):
        tts_train.duration_loss(lw.detach().half(), dur.to(DEV), xm.to(DEV), x_lengths.to(DEV))


def test_fused_adam_clips_each_group_on_its_own_norm():
    """train_STEP1.py:244-249: three clip_grad_norm_ calls with their own max_norm, then one Adam step.  Groups that carry
    "max_norm" match that; a group without the key is unclipped (step() without max_norm), as before."""
    from unitspeech_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(11)
    shapes = [[(40, 3), (7,)], [(25,), (5, 5, 2)], [(300,), (17, 4)], [(9,)]]
    norms = [5.0, 5.0, 2.0, None]
    init = [[torch.randn(s, generator=g) for s in grp] for grp in shapes]
    grads = [[torch.randn(s, generator=g) * 3.0 for s in grp] for grp in shapes]
    ref = [[t.clone().double().requires_grad_(True) for t in grp] for grp in init]
    hip = [[t.clone().to(DEV).requires_grad_(True) for t in grp] for grp in init]
    ropt = torch.optim.Adam([{"params": grp} for grp in ref], lr=1e-2)
    groups = []
    for grp, mn in zip(hip, norms):
        groups.append({"params": grp} if mn is None else {"params": grp, "max_norm": mn})
    hopt = FusedAdam(groups, lr=1e-2)
    for it in range(3):
        ref_norms = []
        for grp, gr, mn in zip(ref, grads, norms):
            for p, gg in zip(grp, gr):
                p.grad = (gg * (it + 1)).double()
            if mn is not None:
                ref_norms.append(float(torch.nn.utils.clip_grad_norm_(grp, max_norm=mn)))
        ropt.step()
        for grp, gr in zip(hip, grads):
            for p, gg in zip(grp, gr):
                p.grad = (gg * (it + 1)).to(DEV)
        hopt.step()
        assert sorted(hopt.last_grad_norms) == [0, 1, 2]
        for gi, want in enumerate(ref_norms):
            assert abs(float(hopt.last_grad_norms[gi]) - want) <= 1e-5 * want
    for rg, hg in zip(ref, hip):
        for r, h in zip(rg, hg):
            err = (h.detach().cpu().double() - r.detach()).abs().max().item()
            assert err < 2e-6, err
