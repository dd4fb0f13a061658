"""Training of the DurationPredictor on the GPU (csrc/duration_train.hip) against the reference goldens of
tools/make_goldens_tts_train.py and the torch restatement (tools/duration_torch.py)."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import duration_torch as DT  # noqa: E402
from test_duration_train import FULL, TINY, full_golden  # noqa: E402
from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.encoder import DurationPredictor, _DurationTrain, synthetic_duration_predictor_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu


def make(cfg, p=0.1, trainable=True):
    dp = DurationPredictor(cfg.in_channels, cfg.filter_channels, cfg.kernel_size, p, spk_emb_dim=cfg.spk_emb_dim, trainable=trainable)
    dp.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_duration_predictor_state_dict(cfg, 0).items()}, strict=True)
    return dp.cuda()


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def grads_of(dp):
    return {k: p.grad.detach().clone() for k, p in dp.named_parameters()}


def check_against(g, cfg, spread):
    """logw within 2e-5, the loss within 1e-5 relative, every gradient within max(10 x the reference's own fp32-to-fp64 distance, 1e-5)
    of the key's fp64 norm.  Returns the worst key."""
    T = lambda k: torch.from_numpy(g[k]).cuda()
    dp = make(cfg).eval()
    logw = dp(T("x"), T("x_mask"), g=T("g"), reverse=True)
    loss = dp(T("x"), T("x_mask"), w=T("w"), g=T("g"), reverse=False)
    loss.backward()
    ref_logw = g["logw64"] if "logw64" in g else g["logw"]
    ref_loss = float(g["loss64"] if "loss64" in g else g["loss"])
    err = float(np.abs(logw.detach().cpu().numpy() - ref_logw).max())
    print(f"logw max abs error {err:.3e}; loss {float(loss.detach()):.7f} vs {ref_loss:.7f}")
    assert err <= 2e-5
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
    worst = ("", 0.0, 0.0)
    grads = grads_of(dp)
    assert len(grads) == 10
    for k, v in grads.items():
        e, s = rel(v, g["g64/" + k]), spread(k)
        print(f"  {k:16s} rel {e:.3e}  reference fp32-vs-fp64 {s:.3e}")
        if e > worst[1]:
            worst = (k, e, s)
        assert e <= max(10 * s, 1e-5), (k, e, s)
    return worst


def test_gradients_match_the_tiny_fp64_golden(golden):
    g = golden("duration_train_tiny")
    check_against(g, TINY, lambda k: rel(g["g32/" + k], g["g64/" + k]))


def test_gradients_match_the_full_size_fp64_golden(golden):
    g = full_golden(golden)
    print("worst key", check_against(g, FULL, lambda k: float(g["spread/" + k])))


def hook_masks(dp, seed, B, L, p):
    lib = _lib.load()
    out = {}
    for site in (0, 1):
        m = torch.empty(B, dp.cfg.filter_channels, L, device="cuda")
        assert lib.us_duration_predictor_dropout_mask(dp._h, seed, site, B, L, p, m.data_ptr(), None) == 0
        out[site] = m
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_is_the_restatement_with_the_hook_masks(golden, p):
    g = golden("duration_train_tiny")
    T = lambda k: torch.from_numpy(g[k]).cuda()
    dp = make(TINY, p).train()
    B, L, seed = 3, 11, 12345
    params = list(dp.state_dict(keep_vars=True).values())
    logw = _DurationTrain.apply(dp, T("x"), T("x_mask"), T("g"), seed, p, *params)
    gl = torch.from_numpy(np.random.Generator(np.random.Philox(key=9)).standard_normal((B, 1, L), dtype=np.float32)).cuda()
    (logw * gl).sum().backward()
    masks = hook_masks(dp, seed, B, L, p)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in dp.state_dict().items()}
    ref = DT.duration_forward(sd, T("x").double(), T("x_mask").double(), T("g").double(), {s: m.double() for s, m in masks.items()})
    (ref * gl.double()).sum().backward()
    assert float((logw.detach().double() - ref.detach()).abs().max()) <= 2e-5
    for k, v in grads_of(dp).items():
        assert rel(v, sd[k].grad) <= 1e-5, k
    for site, m in masks.items():
        vals = set(torch.unique(m).tolist())
        assert vals <= {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}, vals      # kept values scaled by exactly 1 / (1 - p)
        n = m.numel()
        assert abs(float((m > 0).float().mean()) - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5, site
    other = hook_masks(dp, seed + 1, B, L, p)
    assert not torch.equal(other[0], masks[0]) and not torch.equal(masks[0], masks[1])
    assert torch.equal(hook_masks(dp, seed, B, L, p)[0], masks[0])                                   # a pure function of its arguments


def test_keep_fraction_over_a_large_site():
    dp = make(FULL).train()
    dp._sync(torch.device("cuda"), training_ok=True)
    for p in (0.1, 0.5):
        m = hook_masks(dp, 77, 8, 200, p)
        for site in (0, 1):
            n = m[site].numel()
            assert abs(float((m[site] > 0).float().mean()) - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5


def test_p_zero_equals_the_eval_mode_forward_bit_for_bit(golden):
    g = golden("duration_train_tiny")
    T = lambda k: torch.from_numpy(g[k]).cuda()
    dp = make(TINY, 0.0).train()
    params = list(dp.state_dict(keep_vars=True).values())
    a = _DurationTrain.apply(dp, T("x"), T("x_mask"), T("g"), 5, 0.0, *params)
    b = _DurationTrain.apply(dp, T("x"), T("x_mask"), T("g"), 9, -1.0, *params)
    c = dp.eval()(T("x"), T("x_mask"), g=T("g"), reverse=True)           # eval mode, grad enabled: differentiated without dropout
    assert c.requires_grad and torch.equal(a, b) and torch.equal(a, c)


def test_determinism_and_batch_independence(golden):
    g = full_golden(golden)
    T = lambda k: torch.from_numpy(g[k]).cuda()
    runs = []
    for _ in range(2):
        dp = make(FULL).eval()
        dp(T("x"), T("x_mask"), w=T("w"), g=T("g"), reverse=False).backward()
        runs.append(grads_of(dp))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    dp = make(FULL).eval()
    logw = dp(T("x"), T("x_mask"), g=T("g"), reverse=True).detach()
    for b, n in enumerate(g["lengths"]):
        n = int(n)
        alone = dp(T("x")[b:b + 1, :, :n].contiguous(), T("x_mask")[b:b + 1, :, :n].contiguous(), g=T("g")[b:b + 1], reverse=True).detach()
        assert torch.equal(alone[0, 0], logw[b, 0, :n]), b
        assert float(logw[b, 0, n:].abs().max()) == 0.0 if n < logw.shape[-1] else True


def test_autograd_behaviour(golden):
    g = golden("duration_train_tiny")
    T = lambda k: torch.from_numpy(g[k]).cuda()
    dp = make(TINY, 0.0).train()
    loss = lambda: dp(T("x"), T("x_mask"), w=T("w"), g=T("g"), reverse=False)
    loss().backward()
    once = grads_of(dp)
    loss().backward()                                                    # accumulation
    for k, v in grads_of(dp).items():
        assert torch.allclose(v, 2 * once[k], rtol=1e-6, atol=0), k
    dp.zero_grad(set_to_none=True)
    dp.conv_1.weight.requires_grad_(False)
    dp.norm_2.beta.requires_grad_(False)
    loss().backward()                                                    # frozen parameters get none
    assert dp.conv_1.weight.grad is None and dp.norm_2.beta.grad is None
    for k, p in dp.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, once[k]), k
    dp.requires_grad_(True)
    opt = torch.optim.SGD(dp.parameters(), lr=1e-2)
    first = float(loss())
    for _ in range(5):                                                   # an optimiser step is followed by the next forward
        opt.zero_grad()
        l = loss()
        l.backward()
        opt.step()
    assert float(loss()) < first
    l = loss()
    with torch.no_grad():
        dp.proj.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        l.backward()
    with pytest.raises(RuntimeError, match="g requires grad"):
        dp(T("x"), T("x_mask"), g=T("g").requires_grad_(True), reverse=True)
    x = T("x").requires_grad_(True)
    dp(x, T("x_mask"), g=T("g"), reverse=True).sum().backward()
    assert x.grad is None                                                # the reference detaches x


def test_a_stale_or_released_tape_is_refused():
    lib = _lib.load()
    dp = make(TINY, 0.0).train()
    B, L = 2, 7
    x, m, g = torch.randn(B, 16, L).cuda(), torch.ones(B, 1, L).cuda(), torch.randn(B, 1, 12).cuda()
    dp._sync(torch.device("cuda"), training_ok=True)
    n = int(lib.us_duration_predictor_train_workspace_bytes(dp._h, B, L))
    ws, logw, gl = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(B, 1, L).cuda(), torch.ones(B, 1, L).cuda()
    bwd = lambda w, b=B: lib.us_duration_predictor_backward(dp._h, gl.data_ptr(), b, L, None, None, 0, w.data_ptr(), n, None)
    err = lambda h: lib.us_frontend_last_error(h).decode()
    no_tape = "us_duration_predictor_backward: the workspace holds no us_duration_predictor_forward_train of this B and L"
    assert bwd(ws) == -1 and err(dp._h) == no_tape                       # never run
    assert lib.us_duration_predictor_forward_train(dp._h, x.data_ptr(), m.data_ptr(), g.data_ptr(), logw.data_ptr(), B, L, 0.0, 0,
                                                   ws.data_ptr(), n, None) == 0
    assert bwd(ws) == 0
    assert bwd(ws, 1) == -1 and err(dp._h) == no_tape                    # another B
    other = make(TINY, 0.0).train()
    other._sync(torch.device("cuda"), training_ok=True)
    assert lib.us_duration_predictor_backward(other._h, gl.data_ptr(), B, L, None, None, 0, ws.data_ptr(), n, None) == -1      # foreign
    assert err(other._h) == no_tape
    # the gradient list's refusals, as whole sentences; every one returns before anything is launched
    gb = torch.empty(1, device="cuda")
    keys, ptrs = (C.c_char_p * 1)(b"proj.bias"), (C.c_void_p * 1)(gb.data_ptr())
    lst = lambda k=keys, q=ptrs, nk=1, gp=gl.data_ptr(): lib.us_duration_predictor_backward(dp._h, gp, B, L, k, q, nk, ws.data_ptr(), n, None)
    assert lst(gp=None) == -1 and err(dp._h) == "us_duration_predictor_backward: null grad_logw"
    for bad in (dict(nk=-1), dict(k=None), dict(q=None)):
        assert lst(**bad) == -1 and err(dp._h) == "us_duration_predictor_backward: bad gradient list", bad
    for bad in (dict(k=(C.c_char_p * 1)(None)), dict(q=(C.c_void_p * 1)(None))):
        assert lst(**bad) == -1 and err(dp._h) == "us_duration_predictor_backward: null key or gradient buffer", bad
    assert lst(k=(C.c_char_p * 1)(b"nope")) == -2 and err(dp._h) == "us_duration_predictor_backward: unknown key 'nope'"
    assert lst() == 0                                                    # the refusals left the tape alone
    assert lib.us_duration_predictor_tape_release(dp._h, ws.data_ptr()) == 0
    assert bwd(ws) == -1 and err(dp._h) == no_tape                       # released
    torch.cuda.synchronize()
    # the module releases a call's tape with its workspace
    out = dp(x, m, g=g, reverse=True)
    ptr = out.grad_fn.ws.data_ptr() if hasattr(out.grad_fn, "ws") else None
    del out
    gc.collect()
    if ptr is not None:
        assert lib.us_duration_predictor_backward(dp._h, gl.data_ptr(), B, L, None, None, 0, C.c_void_p(ptr), n, None) == -1


def test_the_non_trainable_module_is_unchanged(golden):
    g = golden("duration_train_tiny")
    T = lambda k: torch.from_numpy(g[k]).cuda()
    lib = _lib.load()
    plain, tr = make(TINY, trainable=False).eval(), make(TINY).eval()
    a = plain(T("x"), T("x_mask"), g=T("g"), reverse=True)
    with torch.no_grad():
        b = tr(T("x"), T("x_mask"), g=T("g"), reverse=True)              # eval + no_grad: the inference path
    B, L = 3, 11
    ws = torch.empty(int(lib.us_frontend_workspace_bytes(plain._h, B, L)), dtype=torch.uint8, device="cuda")
    raw = torch.empty(B, 1, L, device="cuda")
    assert lib.us_duration_predictor_forward(plain._h, T("x").data_ptr(), T("x_mask").data_ptr(), T("g").data_ptr(), raw.data_ptr(), B, L,
                                             ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert not a.requires_grad and torch.equal(a, raw) and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="inference-only"):
        plain.train()(T("x"), T("x_mask"), g=T("g"), reverse=True)
    with pytest.raises(NotImplementedError):
        plain.eval()(T("x"), T("x_mask"), w=T("w"), g=T("g"))


def test_mse_loss_against_torch_fp64():
    lib = _lib.load()
    gen = np.random.Generator(np.random.Philox(key=21))
    for B, L in ((1, 1), (3, 11), (32, 300)):
        lens = gen.integers(1, L + 1, size=B)
        lens[0] = L
        mask = torch.from_numpy((np.arange(L)[None] < lens[:, None]).astype(np.float32)).view(B, 1, L).cuda()
        logw = torch.from_numpy(gen.standard_normal((B, 1, L), dtype=np.float32)).cuda() * mask
        w = torch.from_numpy(gen.integers(0, 9, size=(B, 1, L)).astype(np.float32)).cuda() * mask
        loss, d = torch.empty((), device="cuda"), torch.empty(B, 1, L, device="cuda")
        assert lib.us_duration_predictor_mse_loss(logw.data_ptr(), w.data_ptr(), mask.data_ptr(), loss.data_ptr(), d.data_ptr(), B, L, None) == 0
        torch.cuda.synchronize()
        lw = logw.double().cpu().requires_grad_(True)
        ref = DT.duration_mse(lw, w.double().cpu(), mask.double().cpu())
        ref.backward()
        assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref)), (B, L)
        assert float((d.double().cpu() - lw.grad).abs().max()) <= 1e-6 * float(lw.grad.abs().max()), (B, L)
