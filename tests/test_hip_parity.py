"""GPU parity tests: the HIP decoder (through the C ABI, via the Python mirror) against the CPU oracle and the
golden vectors captured from the reference.  Tolerances: single estimator evaluation mean-L1 <= 2e-6 (fp32 noise
floor measured in SURVEY.md §8(c): 2.5e-7); sampler loops mel-L1 <= 1e-3 (north-star tolerance)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import decoder_oracle as O
from unitspeech_amd import DecoderConfig, GradLogPEstimator2d, UnitSpeech, _lib, synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu

TINY = DecoderConfig(dim=16)
FULL = DecoderConfig()
DEV = "cuda:0"


def make_model(cfg, seed=0):
    m = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, seed).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny():
    return make_model(TINY), O.to_torch(synthetic_state_dict(TINY, 0))


@pytest.fixture(scope="module")
def full():
    return make_model(FULL), O.to_torch(synthetic_state_dict(FULL, 0))


def G(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def l1(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().mean().item()


def test_native_library_is_loaded():
    lib = _lib.load()
    assert os.path.basename(lib._name) == "libunitspeech_hip.so"
    assert os.path.dirname(lib._name).endswith("unitspeech_amd")      # in-tree, not site-packages


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_estimator_eval_vs_golden_and_oracle(golden, tag, tiny, full):
    model, sd = tiny if tag == "tiny" else full
    g = G(golden(f"estimator_{tag}"))
    with torch.no_grad():
        out = model.estimator(g["x"].to(DEV), g["mask"].to(DEV), g["mu"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    e_gold, e_64 = l1(out, g["out"]), l1(out, g["out_fp64"])
    ref = O.estimator_forward(sd, g["x"], g["mask"], g["mu"], g["t"], g["spk_emb"])
    e_or = l1(out, ref)
    print(f"\n[{tag}] estimator L1 vs golden {e_gold:.3e}  vs fp64 {e_64:.3e}  vs oracle {e_or:.3e}  (mean|out| {g['out'].abs().mean():.3f})")
    assert e_gold <= 2e-6 and e_or <= 2e-6 and e_64 <= 2e-6
    # masked frames are exactly zero (output * mask, unitspeech.py:201)
    assert (out.cpu() * (1 - g["mask"])).abs().max().item() == 0.0


def test_estimator_standalone_module(golden, tiny):
    """GradLogPEstimator2d used on its own (no UnitSpeech parent) gives the same result."""
    g = G(golden("estimator_tiny"))
    est = GradLogPEstimator2d(TINY.dim, dim_mults=TINY.dim_mults, pe_scale=TINY.pe_scale, spk_emb_dim=TINY.spk_emb_dim)
    sd = {k[len("estimator."):]: torch.from_numpy(v) for k, v in synthetic_state_dict(TINY, 0).items() if k.startswith("estimator.")}
    est.load_state_dict(sd, strict=True)
    est = est.to(DEV).eval()
    with torch.no_grad():
        out = est(g["x"].to(DEV), g["mask"].to(DEV), g["mu"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV))
    assert l1(out, g["out"]) <= 2e-6


@pytest.mark.parametrize("T", [8, 24, 136])
def test_estimator_ragged_lengths_vs_oracle(tiny, T):
    """T not a multiple of the 128-pixel tile at any level, partially and fully padded items."""
    model, sd = tiny
    inp = G(synthetic_inputs(TINY, 3, T, seed=11, lengths=[T, max(T - 7, 1), 0]))
    t = torch.tensor([0.37, 0.9, 0.05])
    with torch.no_grad():
        out = model.estimator(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), t.to(DEV), inp["spk_emb"].to(DEV))
    ref = O.estimator_forward(sd, inp["z"], inp["mask"], inp["cond"], t, inp["spk_emb"])
    assert l1(out, ref) <= 2e-6
    assert out[2].abs().max().item() == 0.0            # fully padded item


def _model_with_env(cfg, exact=False, **env):
    """A fresh handle created under the given environment (the library reads its tuning switches at us_decoder_create); exact: the
    exact-fp32 handle (US_CREATE_EXACT_FP32)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        m = make_model(cfg)
        m.exact = exact
        with torch.no_grad():      # creates the handle and uploads the weights now, while the environment is in place
            x = torch.zeros(1, 80, 8, device=DEV)
            m.estimator(x, torch.ones(1, 1, 8, device=DEV), x, torch.full((1,), 0.5, device=DEV), torch.zeros(1, 1, cfg.spk_emb_dim, device=DEV))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return m


@pytest.mark.parametrize("T", [8, 200])
def test_winograd_forms_agree_bitwise_and_match_direct_convolution(tiny, T):
    """The three executions of a 3x3 convolution -- Winograd with the output transform inside the GEMM kernel, Winograd with
    separate transform passes, direct implicit GEMM -- on a ragged input whose level-3 width is odd (partial last tile):
    the two Winograd forms agree bit for bit (the library picks between them by launch size, i.e. by batch), the direct form
    agrees to rounding, and all match the CPU oracle."""
    _, sd = tiny                                                              # T = 200: widths 200 / 100 / 50 / 25; T = 8: 8 / 4 / 2 / 1
    inp = G(synthetic_inputs(TINY, 3, T, seed=31, lengths=[T, max(T - 13, 3), min(64, T)]))
    t = torch.tensor([0.21, 0.55, 0.93])
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond")] + [t.to(DEV), inp["spk_emb"].to(DEV)]
    outs = {}
    for name, env in (("fused", {"US_WINO_FUSE": 1}), ("separate", {"US_WINO_FUSE": 0}),
                      ("direct", {"US_WINO_MIN_LEVEL": 99}), ("gn_apart", {"US_WINO_FUSE_GN": 0}), ("default", {})):
        m = _model_with_env(TINY, **env)
        with torch.no_grad():
            outs[name] = m.estimator(*args).cpu()
    assert torch.equal(outs["fused"], outs["separate"])
    assert torch.equal(outs["default"], outs["fused"])
    ref = O.estimator_forward(sd, inp["z"], inp["mask"], inp["cond"], t, inp["spk_emb"])
    for name, o in outs.items():
        assert l1(o, ref) <= 2e-6, name
    assert l1(outs["direct"], outs["fused"]) <= 1e-6
    assert l1(outs["gn_apart"], outs["default"]) <= 1e-6      # block1's GroupNorm+Mish inside / outside block2's input transform


@pytest.mark.parametrize("w", ["11", "10", "01", "00"])
def test_loop_tiny_cfg_variants(golden, tiny, w):
    model, _ = tiny
    g = G(golden(f"loop_tiny_N10_w{w}"))
    out = model(g["z"].to(DEV), g["mask"].to(DEV), g["cond"].to(DEV), g["spk_emb"].to(DEV), 10,
                float(g["w_text"]), float(g["w_spk"]), noise=g["noise"].to(DEV))
    e = l1(out, g["out"])
    print(f"\nloop tiny w={w}: mel-L1 {e:.3e} (mean|out| {g['out'].abs().mean():.2f})")
    assert e <= 1e-3


def test_loop_tiny_batched_equals_independent_reference_runs(golden, tiny):
    model, _ = tiny
    g = G(golden("loop_tiny_N10_B2"))
    for mb in (1, 2):
        model.micro_batch = mb
        out = model(g["z"].to(DEV), g["mask"].to(DEV), g["cond"].to(DEV), g["spk_emb"].to(DEV), 10, 1.0, 1.0,
                    noise=g["noise"].to(DEV))
        assert l1(out, g["out"]) <= 1e-3
    model.micro_batch = 0


@pytest.mark.parametrize("n", [10, 50])
def test_loop_full_vs_reference_golden(golden, full, n):
    """BASELINE config: full-size decoder, text+spk CFG; T=64 so the reference run that made the golden took seconds."""
    model, _ = full
    g = G(golden(f"loop_full_N{n}"))
    T = g["z"].shape[-1]
    inp = G(synthetic_inputs(FULL, 1, T, seed=5, n_steps=n, lengths=[T - 4]))
    assert abs(inp["noise"].double().abs().sum().item() - float(g["noise_abs_sum"])) < 1e-6 * float(g["noise_abs_sum"])
    out = model(g["z"].to(DEV), g["mask"].to(DEV), g["cond"].to(DEV), g["spk_emb"].to(DEV), n, 1.0, 1.0,
                noise=inp["noise"].to(DEV))
    e = l1(out, g["out"])
    scale = g["out"].abs().mean().item()
    print(f"\nloop full N={n}: mel-L1 {e:.3e}  relative {e / scale:.3e}  (mean|out| {scale:.1f})")
    assert torch.isfinite(out).all()
    assert e <= 1e-3


def test_full_size_eval_at_baseline_shape_vs_oracle(full):
    """One 3-branch evaluation at the BASELINE shape 80x1024 against the CPU oracle (~10 s of CPU)."""
    model, sd = full
    T = 1024
    inp = G(synthetic_inputs(FULL, 1, T, seed=21, lengths=[T - 40]))
    x3 = inp["z"].repeat(3, 1, 1)
    mask3 = inp["mask"].repeat(3, 1, 1)
    mu3 = torch.cat([sd["text_uncon"].repeat(1, 1, T), inp["cond"], inp["cond"]], 0)
    spk_un = sd["spk_uncon"] / sd["spk_uncon"].norm()
    spk3 = torch.cat([inp["spk_emb"], spk_un, inp["spk_emb"]], 0)
    t3 = torch.full((3,), 0.63)
    with torch.no_grad():
        out = model.estimator(x3.to(DEV), mask3.to(DEV), mu3.to(DEV), t3.to(DEV), spk3.to(DEV))
    ref = O.estimator_forward(sd, x3, mask3, mu3, t3, spk3)
    e = l1(out, ref)
    print(f"\nfull-size eval T=1024: L1 {e:.3e} (mean|ref| {ref.abs().mean():.3f})")
    assert e <= 2e-6


def test_builtin_generator_statistics_and_shard_independence(tiny):
    model, _ = tiny
    lib = _lib.load()
    n = 1 << 20
    buf = torch.empty(n, device=DEV)
    assert lib.us_fill_normal(C.c_void_p(buf.data_ptr()), n, 7, 3, None) == 0
    torch.cuda.synchronize()
    assert abs(buf.mean().item()) < 5e-3 and abs(buf.std().item() - 1) < 5e-3
    assert abs((buf ** 4).mean().item() - 3) < 0.05
    # same (seed, utterance, step) stream whatever the batch composition: item 1 of a B=2 run == B=1 run at offset 1
    T = 16
    inp = G(synthetic_inputs(TINY, 2, T, seed=9))
    a = model(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), 4, 1.0, 1.0,
              rng="philox", seed=5)
    b = model(inp["z"][1:].to(DEV), inp["mask"][1:].to(DEV), inp["cond"][1:].to(DEV), inp["spk_emb"][1:].to(DEV), 4, 1.0, 1.0,
              rng="philox", seed=5, utt_offset=1)
    assert torch.equal(a[1:], b)
    c = model(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), 4, 1.0, 1.0,
              rng="philox", seed=6)
    assert not torch.equal(a, c)


def test_flop_model_matches_survey(full):
    model, _ = full
    eng = model._get_engine()
    for T in (64, 128, 1024):
        fl = eng.lib.us_estimator_flops(eng.handle, T)
        assert fl == pytest.approx(649_461_760 * T + 6_160_384, rel=1e-3)


def test_errors_are_reported_not_swallowed(tiny):
    model, _ = tiny
    z = torch.zeros(1, 80, 12, device=DEV)          # 12 is not a multiple of 8
    with pytest.raises(RuntimeError, match="EINVAL"):
        model(z, torch.ones(1, 1, 12, device=DEV), z, torch.zeros(1, 1, 256, device=DEV), 2, 1.0, 1.0, rng="philox")


# ---------------------------------------------------------------------------------------------------------------
# training path: loss_t forward + backward through the HIP score network vs the reference's autograd (goldens)
# ---------------------------------------------------------------------------------------------------------------
class _ReplayRandn:
    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def __enter__(self):
        self.orig = torch.randn
        torch.randn = self
        return self

    def __exit__(self, *a):
        torch.randn = self.orig

    def __call__(self, *shape, **kw):
        d = self.draws[self.i]
        self.i += 1
        return d.to(device=kw.get("device", d.device), dtype=kw.get("dtype", d.dtype))


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_loss_and_gradients_vs_reference_autograd(golden, tag):
    cfg = TINY if tag == "tiny" else FULL
    g = G(golden(f"loss_{tag}"))
    model = make_model(cfg).train()
    with _ReplayRandn([g["z"].to(DEV)]):
        loss, xt = model.loss_t(g["x0"].to(DEV), g["mask"].to(DEV), g["cond"].to(DEV), g["t"].to(DEV), g["spk_emb"].to(DEV))
    assert abs(loss.item() - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    assert l1(xt, g["xt"]) <= 1e-6
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    worst = 0.0
    for k, ref in g.items():
        if not k.startswith("grad:"):
            continue
        got = params[k[5:]].grad.cpu()
        scale = ref.abs().max().item() + 1e-12
        err = (got - ref).abs().max().item() / scale
        worst = max(worst, err)
        assert err <= 2e-4, (k, err)
    sq = 0.0
    for name, p in params.items():
        if name in ("text_uncon", "spk_uncon"):
            assert p.grad is None          # not on the compute_loss path (unitspeech.py:393-411)
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        sq += float((p.grad.double() ** 2).sum())
    gn = sq ** 0.5
    print(f"\n[{tag}] loss {loss.item():.6f} (ref {float(g['loss']):.6f})  grad-norm {gn:.6f} (ref {float(g['grad_norm']):.6f})  worst sampled-grad rel err {worst:.2e}")
    assert abs(gn - float(g["grad_norm"])) <= 1e-4 * float(g["grad_norm"])


@pytest.mark.parametrize("fused", [False, True])
def test_fine_tune_step_matches_oracle_and_updates_weights(golden, fused):
    """One full fine-tune iteration (finetune.py:131-165: fine_tune -> backward -> clip_grad_norm_(1) -> Adam) on the tiny
    config against the reference goldens: loss, total gradient norm, clipped gradients and updated parameters; with torch's
    optimiser and with the HIP clip+Adam (`FusedAdam.step(max_norm=1)`); a second forward sees the updated weights."""
    import random
    from unitspeech_amd import FusedAdam
    g = G(golden("finetune_tiny"))
    a = golden("finetune_tiny_adam")
    model = make_model(TINY).train()
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = (FusedAdam if fused else torch.optim.Adam)(model.parameters(), lr=2e-5)
    random.seed(int(g["py_seed"]))
    orig_rand = torch.rand
    torch.rand = lambda *a, **k: g["t_draw"].to(DEV)
    try:
        with _ReplayRandn([g["z_draw"].to(DEV)]):
            loss = model.fine_tune(g["cond_x"].to(DEV), g["y"].to(DEV), g["y_mask"].to(DEV), g["y_lengths"].to(DEV),
                                   g["y"].shape[-1], g["attn"].to(DEV), g["spk_emb"].to(DEV), int(g["segment_size"]), 80)
    finally:
        torch.rand = orig_rand
    assert abs(loss.item() - float(g["loss"])) <= 2e-6
    loss.backward()
    if fused:
        opt.step(max_norm=1)
        norm = float(opt.last_grad_norm)
    else:
        norm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1))
        opt.step()
    assert abs(norm - float(a["grad_norm"])) <= 1e-4 * float(a["grad_norm"])
    params = dict(model.named_parameters())
    for i, k in enumerate([str(x) for x in a["keys"]]):
        gr, pr = torch.from_numpy(np.asarray(a[f"grad_{i}"])), torch.from_numpy(np.asarray(a[f"param_{i}"]))
        assert (params[k].grad.cpu() - gr).abs().max() <= 2e-4 * gr.abs().max() + 1e-9, k      # clipped in place
        d_ref, d_got = pr - start[k].cpu(), params[k].detach().cpu() - start[k].cpu()
        # The first Adam step moves an element by lr * g / (|g| + eps): ~lr = 2e-5 wherever |g| >> eps = 1e-8, but an element whose
        # gradient is itself ~eps turns an absolute gradient error of 1e-9 (fp32 atomics order) into a few % of lr.
        err = (d_got - d_ref).abs()
        solid = gr.abs() > 1e-6
        assert err[solid].max() <= 2e-7 if solid.any() else True, k
        assert err.max() <= 2e-6, k
    with torch.no_grad():          # the engine must pick the new weights up
        x = torch.zeros(1, 80, 16, device=DEV)
        out = model.estimator(x, torch.ones(1, 1, 16, device=DEV), x, torch.full((1,), 0.5, device=DEV), g["spk_emb"].to(DEV))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = O.estimator_forward(sd, x.cpu(), torch.ones(1, 1, 16), x.cpu(), torch.full((1,), 0.5), g["spk_emb"])
    assert l1(out, ref) <= 2e-6


def test_fused_adam_matches_torch_adam_over_steps():
    """HIP clip+Adam vs torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the same device: odd sizes, a 4-byte-aligned view,
    three steps with fresh gradients (bias corrections), clipping active and inactive."""
    from unitspeech_amd import FusedAdam
    gen = torch.Generator().manual_seed(5)
    base = torch.randn(100003 + 1, generator=gen)
    shapes = [(1,), (7,), (4096,), (4097,), (64, 33, 3, 3), (1, 1, 256)]
    def make():
        ps = [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(DEV)) for i, s in enumerate(shapes)]
        ps.append(torch.nn.Parameter(base.to(DEV)[1:]))            # storage offset 1: not 16-byte aligned
        return ps
    pa, pb = make(), make()
    oa, ob = torch.optim.Adam(pa, lr=2e-5), FusedAdam(pb, lr=2e-5)
    for step in range(3):
        scale = [3.0, 1e-3, 1.0][step]                              # norm >> 1, << 1, ~
        for i, (x, y) in enumerate(zip(pa, pb)):
            gr = (torch.randn(x.shape, generator=torch.Generator().manual_seed(100 * step + i)) * scale).to(DEV)
            x.grad, y.grad = gr.clone(), gr.clone()
        na = torch.nn.utils.clip_grad_norm_(pa, 1)
        oa.step()
        ob.step(max_norm=1)
        assert abs(float(na) - float(ob.last_grad_norm)) <= 1e-5 * float(na)
        for x, y in zip(pa, pb):
            assert (x.grad - y.grad).abs().max() <= 1e-6 * x.grad.abs().max() + 1e-12
            assert (x.detach() - y.detach()).abs().max() <= 1e-7          # updates are ~2e-5: 0.5 %
            sa, sb = oa.state[x], ob.state[y]
            assert (sa["exp_avg"] - sb["exp_avg"]).abs().max() <= 1e-6 * sa["exp_avg"].abs().max() + 1e-12
            assert (sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max() <= 1e-6 * sa["exp_avg_sq"].abs().max() + 1e-20
            assert int(sb["step"]) == step + 1


# ---------------------------------------------------------------------------------------------------------------
# sampler edge cases: ragged batch with a fully padded item, single step, minimum length, properties at BASELINE size
# ---------------------------------------------------------------------------------------------------------------
def test_loop_ragged_batch_vs_oracle(tiny):
    model, sd = tiny
    T, N = 40, 6
    inp = G(synthetic_inputs(TINY, 3, T, seed=31, n_steps=N, lengths=[T, 17, 0]))
    for mb in (1, 2, 3):
        model.micro_batch = mb
        out = model(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), N, 1.0, 1.0,
                    noise=inp["noise"].to(DEV))
        ref = O.reverse_diffusion(sd, inp["z"], inp["mask"], inp["cond"], inp["spk_emb"], N, 1.0, 1.0, noise=inp["noise"])
        assert l1(out, ref) <= 1e-4
        assert out[2].abs().max().item() == 0.0                       # fully padded utterance stays zero
        assert (out.cpu() * (1 - inp["mask"])).abs().max().item() == 0.0
    model.micro_batch = 0


@pytest.mark.parametrize("T,N", [(8, 1), (8, 3), (16, 2)])
def test_loop_minimum_sizes_vs_oracle(tiny, T, N):
    """T = 8 is the smallest legal length (fix_len_compatibility); N = 1 is a case the reference itself cannot run
    (its `.squeeze()` turns the 1-step schedule into a 0-d tensor, unitspeech.py:344)."""
    model, sd = tiny
    inp = G(synthetic_inputs(TINY, 1, T, seed=41, n_steps=N))
    out = model(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), N, 1.0, 1.0,
                noise=inp["noise"].to(DEV))
    ref = O.reverse_diffusion(sd, inp["z"], inp["mask"], inp["cond"], inp["spk_emb"], N, 1.0, 1.0, noise=inp["noise"])
    assert l1(out, ref) <= 1e-4


def test_baseline_size_sampler_properties(full):
    """Size-independent properties at the BASELINE shape (B=1, 80x1024, full-size weights), 2 steps:
    determinism of the built-in generator, batch-composition independence (bit-exact), masked frames exactly zero."""
    model, _ = full
    T = 1024
    inp = G(synthetic_inputs(FULL, 2, T, seed=51, lengths=[T, T - 96]))
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond", "spk_emb")]
    a = model(*args, 2, 1.0, 1.0, rng="philox", seed=9)
    b = model(*args, 2, 1.0, 1.0, rng="philox", seed=9)
    assert torch.equal(a, b)
    one = model(*(t[1:] for t in args), 2, 1.0, 1.0, rng="philox", seed=9, utt_offset=1)
    assert torch.equal(a[1:], one)
    assert torch.isfinite(a).all()
    assert (a.cpu() * (1 - inp["mask"])).abs().max().item() == 0.0


def test_long_utterance_properties(full):
    """4x the BASELINE length (80x4096, full-size weights, ragged pair): finite, masked frames exactly zero, run-to-run identical,
    and the first item equal to its single-utterance run (per-item offsets stay below the 2 GiB buffer-descriptor range)."""
    model, _ = full
    T = 4096
    inp = G(synthetic_inputs(FULL, 2, T, seed=77, lengths=[T, T - 1000]))
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond", "spk_emb")]
    a = model(*args, 1, 1.0, 1.0, rng="philox", seed=3)
    b = model(*args, 1, 1.0, 1.0, rng="philox", seed=3)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert (a.cpu() * (1 - inp["mask"])).abs().max().item() == 0.0
    one = model(*(t[:1] for t in args), 1, 1.0, 1.0, rng="philox", seed=3)
    assert torch.equal(a[:1], one)


def test_f16x3_winograd_gemms_match_the_fp32_path(full):
    """Default path: Winograd GEMMs as three fp16 MFMA products of two-plane split operands (fp32 accumulation) against the same
    GEMMs on the exact-fp32 matrix instruction (the US_CREATE_EXACT_FP32 handle) and the oracle: same error level, batch composition stays out of the
    result, and the fused / separate output-transform forms still agree bit for bit."""
    _, sd = full
    T = 64
    inp = G(synthetic_inputs(FULL, 3, T, seed=41, lengths=[T, T - 5, 40]))
    t = torch.tensor([0.3, 0.6, 0.9])
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond")] + [t.to(DEV), inp["spk_emb"].to(DEV)]
    ref = O.estimator_forward(sd, inp["z"], inp["mask"], inp["cond"], t, inp["spk_emb"])
    outs = {}
    for name, env in (("f16x3", {}), ("fp32", {"exact": True}), ("f16x3_fused", {"US_WINO_FUSE": 1}),
                      ("f16x3_separate", {"US_WINO_FUSE": 0}), ("f16x3_tm64", {"US_F16_TM": 64})):
        m = _model_with_env(FULL, **env)
        with torch.no_grad():
            outs[name] = m.estimator(*args)
            if name == "f16x3":
                one = m.estimator(*(a[1:2] for a in args))
    e16, e32 = l1(outs["f16x3"], ref), l1(outs["fp32"], ref)
    print(f"\nestimator L1 vs oracle: f16x3 {e16:.3e}, fp32 MFMA {e32:.3e}; f16x3 vs fp32 {l1(outs['f16x3'], outs['fp32']):.3e}")
    assert e16 <= 2e-6 and e32 <= 2e-6
    assert e16 <= 1.5 * e32 + 1e-7
    assert torch.equal(outs["f16x3"][1:2], one)
    assert torch.equal(outs["f16x3_fused"], outs["f16x3_separate"])
    assert torch.equal(outs["f16x3_tm64"], outs["f16x3_separate"])
