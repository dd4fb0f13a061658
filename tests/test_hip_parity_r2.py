"""GPU parity tests added in round 2 (all through the C ABI): the two BASELINE configurations that had no GPU test (B=64 on one
GPU; the 50-step loop at the BASELINE length against a reference golden), every parameter gradient and the input gradients
against the reference's autograd, evaluations where attention dominates, the reference's per-module outputs through
`us_debug_block`, the reference's own `execute_text_to_speech` with the fused mel de-normalisation, tape ownership, argument
validation."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import decoder_oracle as O
from unitspeech_amd import DecoderConfig, UnitSpeech, _lib, synthetic_inputs, synthetic_state_dict
from unitspeech_amd.frontend import SyntheticFrontEnd, text_to_ids

pytestmark = pytest.mark.gpu

TINY = DecoderConfig(dim=16)
FULL = DecoderConfig()
DEV = "cuda:0"
GRAD_SAMPLE = 8192


def make_model(cfg, seed=0, **recipe):
    m = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, seed, **recipe).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def full():
    return make_model(FULL)


def G(d):
    return {k: (torch.from_numpy(np.asarray(v)) if np.asarray(v).dtype.kind != "U" else str(v)) for k, v in d.items()}


def l1(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().mean().item()


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


# ---------------------------------------------------------------------------------------------------------------
# BASELINE.json configs[2]: B = 64 utterances on one GPU, 80x1024, default micro-batch (8)
# ---------------------------------------------------------------------------------------------------------------
def test_config2_batch64_crosses_micro_batches_and_matches_single_runs(full):
    T, B, N = 1024, 64, 2
    lengths = [T - 8 * (b % 5) for b in range(B)]
    inp = G(synthetic_inputs(FULL, B, T, seed=61, lengths=lengths))
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond", "spk_emb")]
    assert full.micro_batch == 0                                       # library default: 8 utterances per micro-batch
    out = full(*args, N, 1.0, 1.0, rng="philox", seed=17)
    assert torch.isfinite(out).all()
    assert (out.cpu() * (1 - inp["mask"])).abs().max().item() == 0.0   # masked frames exactly zero (:373)
    for b in (0, 7, 8, 63):                                            # last of micro-batch 0, first of 1, last of 7
        one = full(*(t[b:b + 1] for t in args), N, 1.0, 1.0, rng="philox", seed=17, utt_offset=b)
        assert torch.equal(out[b:b + 1], one), b


# ---------------------------------------------------------------------------------------------------------------
# BASELINE.json configs[1] at full length: 50 steps at 80x1024 against the reference (fp32 and fp64 columns)
# ---------------------------------------------------------------------------------------------------------------
def test_loop_50_steps_at_baseline_length_vs_reference_golden(golden, full):
    g = G(golden("loop_full_N50_T1024"))
    T, N = 1024, 50
    inp = G(synthetic_inputs(FULL, 1, T, seed=int(g["seed"]), n_steps=N, lengths=[int(g["lengths"][0])]))
    assert abs(inp["noise"].double().abs().sum().item() - float(g["noise_abs_sum"])) < 1e-9 * float(g["noise_abs_sum"])
    assert abs(inp["z"].double().abs().sum().item() - float(g["z_abs_sum"])) < 1e-9 * float(g["z_abs_sum"])
    out = full(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), inp["spk_emb"].to(DEV), N, 1.0, 1.0, noise=inp["noise"].to(DEV))
    e32, e64, ref_gap = l1(out, g["out"]), l1(out, g["out_fp64"]), l1(g["out"], g["out_fp64"])
    scale = g["out"].abs().mean().item()
    print(f"\nloop full N=50 T=1024: mel-L1 vs reference fp32 {e32:.3e}, vs fp64 {e64:.3e} (reference fp32 vs fp64 {ref_gap:.3e}); mean|out| {scale:.1f}")
    assert torch.isfinite(out).all()
    assert e32 <= 1e-3 and e64 <= 1e-3                                 # north-star tolerance


# ---------------------------------------------------------------------------------------------------------------
# every gradient; input gradients; attention-dominated weights
# ---------------------------------------------------------------------------------------------------------------
def sample_stride(numel):       # tools/make_goldens_r2.py
    return (numel // GRAD_SAMPLE + 1) | 1


@pytest.mark.parametrize("tag,recipe", [("", {}), ("_attn", dict(rezero_g=1.0, qkv_scale=1.0))])
def test_every_parameter_gradient_and_input_gradients_vs_reference_autograd(golden, tag, recipe):
    g = G(golden(f"loss_tiny_allgrads{tag}"))
    model = make_model(TINY, **recipe).train()
    inp = G(synthetic_inputs(TINY, 2, 32, seed=6, lengths=[32, 24]))
    x0, cond, spk = (inp[k].to(DEV).requires_grad_(True) for k in ("z", "cond", "spk_emb"))
    with _ReplayRandn([g["z"].to(DEV)]):
        loss, xt = model.loss_t(x0, inp["mask"].to(DEV), cond, g["t"].to(DEV), spk)
    assert abs(loss.item() - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    assert l1(xt, g["xt"]) <= 1e-6
    loss.backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    worst, n = 0.0, 0
    for k, ref in g.items():
        if not k.startswith("grad:"):
            continue
        name = k[5:]
        got = params[name].grad.double().cpu().reshape(-1)
        ref = ref.double().reshape(-1)
        rms = float(np.sqrt(float(g["gradsq:" + name]) / got.numel())) + 1e-12
        samp = got if got.numel() <= GRAD_SAMPLE else got[::sample_stride(got.numel())]
        err = float((samp - ref).abs().max()) / max(rms, float(ref.abs().max()))
        worst = max(worst, err)
        assert err <= 2e-4, (name, err)
        assert abs(float((got ** 2).sum()) - float(g["gradsq:" + name])) <= 4e-4 * float(g["gradsq:" + name]) + 1e-18, name
        n += 1
    assert n == 228
    sq = sum(float((p.grad.double() ** 2).sum()) for k, p in params.items() if p.grad is not None)
    assert abs(sq ** 0.5 - float(g["grad_norm"])) <= 1e-4 * float(g["grad_norm"])
    for name, got in (("grad_x0", x0.grad), ("grad_cond", cond.grad), ("grad_spk_emb", spk.grad)):
        ref = g[name]
        err = float((got.cpu() - ref).abs().max()) / float(ref.abs().max())
        worst = max(worst, err)
        assert err <= 2e-4, (name, err)
    print(f"\n[tiny{tag}] 228 parameter gradients + 3 input gradients: worst relative error {worst:.2e}")


def test_full_size_input_gradients_and_frozen_decoder(golden):
    """d loss / d (x0, cond, spk_emb) at full size; with the decoder frozen (train_STEP2.py:130-131: only the unit encoder
    trains, through mu) the same gradients still flow."""
    g = G(golden("loss_full_inputgrads"))
    model = make_model(FULL).train()
    inp = G(synthetic_inputs(FULL, 2, 64, seed=6, lengths=[64, 56]))
    for frozen in (False, True):
        for p in model.parameters():
            p.requires_grad_(not frozen)
            p.grad = None
        x0, cond, spk = (inp[k].to(DEV).requires_grad_(True) for k in ("z", "cond", "spk_emb"))
        with _ReplayRandn([g["z"].to(DEV)]):
            loss, _ = model.loss_t(x0, inp["mask"].to(DEV), cond, g["t"].to(DEV), spk)
        assert loss.requires_grad
        loss.backward()
        assert abs(loss.item() - float(g["loss"])) <= 4e-6
        for name, got in (("grad_x0", x0.grad), ("grad_cond", cond.grad), ("grad_spk_emb", spk.grad)):
            assert (got.cpu() - g[name]).abs().max() <= 2e-4 * g[name].abs().max(), (name, frozen)
        assert all((p.grad is None) == frozen for n_, p in model.named_parameters() if n_ not in ("text_uncon", "spk_uncon"))


@pytest.mark.parametrize("tag,cfg,Tn", [("tiny", TINY, 32), ("full", FULL, 64)])
def test_strong_attention_evaluation_vs_reference(golden, tag, cfg, Tn):
    """Rezero gain 1 and unscaled to_qkv: attention contributes mean-L1 0.23-0.30 of an output of mean |.| 0.29-0.37 (with the
    shipped recipe it is 0.3 % of the signal), so an attention error of 1e-5 relative is visible at this tolerance."""
    g = G(golden(f"estimator_{tag}_attn"))
    model = make_model(cfg, rezero_g=1.0, qkv_scale=1.0)
    inp = G(synthetic_inputs(cfg, 3, Tn, seed=2, lengths=[int(v) for v in g["lengths"]]))
    with torch.no_grad():
        out = model.estimator(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), g["t"].to(DEV), inp["spk_emb"].to(DEV))
    e, e64 = l1(out, g["out"]), l1(out, g["out_fp64"])
    print(f"\n[{tag}] strong-attention evaluation: L1 vs reference {e:.3e}, vs fp64 {e64:.3e}")
    assert e <= 2e-6 and e64 <= 2e-6


# ---------------------------------------------------------------------------------------------------------------
# per-module outputs of the reference (tests/golden/blocks_tiny.npz) through us_debug_block
# ---------------------------------------------------------------------------------------------------------------
def _debug_block(model, kind, prefix, level, x_nchw, mask_full, temb, cout, hw_out):
    eng = model._sync(torch.device(DEV))
    lib = eng.lib
    B, T = mask_full.shape[0], mask_full.shape[-1]
    x = x_nchw.permute(0, 2, 3, 1).contiguous().to(DEV)                 # pixel-major, the library's activation layout
    out = torch.empty(B, hw_out[0], hw_out[1], cout, device=DEV)
    ws = torch.empty(int(lib.us_workspace_bytes(eng.handle, B, T)), dtype=torch.uint8, device=DEV)
    m = mask_full.reshape(B, T).contiguous().to(DEV)
    te = temb.contiguous().to(DEV) if temb is not None else None
    rc = lib.us_debug_block(eng.handle, kind, prefix.encode(), level, C.c_void_p(x.data_ptr()), C.c_void_p(m.data_ptr()),
                            C.c_void_p(te.data_ptr()) if te is not None else None, C.c_void_p(out.data_ptr()), B, T,
                            C.c_void_p(ws.data_ptr()), ws.numel(), None)
    _lib.check(rc, eng.handle, "us_debug_block")
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


def test_building_blocks_vs_reference_modules(golden):
    """Block, ResnetBlock (identity and 1x1 residual), Residual(Rezero(LinearAttention)), Downsample, Upsample: the reference's
    module outputs on [2, C, 20, 12] inputs with a padded item, each reproduced by the library's own launch sequence."""
    g = G(golden("blocks_tiny"))
    model = make_model(TINY)
    B, H, W, level = 2, 20, 12, 2                                       # 80 >> 2 = 20 rows, T = 48 -> 12 columns
    T = W << level
    mask = g["mask"].reshape(B, W)
    mask_full = mask.repeat_interleave(1 << level, dim=1).reshape(B, 1, T)      # level mask = mask_full[..., ::4]
    ones = torch.ones(B, 1, T)
    mm = g["mask"]                                                      # [B,1,1,W]
    tol = 2e-6
    got = _debug_block(model, 0, "estimator.downs.1.1", level, g["x32"] * mm, mask_full, None, 32, (H, W))
    assert l1(got, g["block"]) <= tol
    got = _debug_block(model, 1, "estimator.downs.1.1", level, g["x32"] * mm, mask_full, g["temb"], 32, (H, W))
    assert l1(got, g["resnet_same"]) <= tol
    got = _debug_block(model, 1, "estimator.downs.1.0", level, g["x16"] * mm, mask_full, g["temb"], 32, (H, W))
    assert l1(got, g["resnet_proj"]) <= tol
    got = _debug_block(model, 2, "estimator.downs.1.2", level, g["x32"], ones, None, 32, (H, W))
    e_attn = l1(got, g["attn"])
    assert e_attn <= tol
    got = _debug_block(model, 3, "estimator.downs.1.3", level, g["x32"] * mm, ones, None, 32, (H // 2, W // 2))
    assert l1(got, g["down"]) <= tol
    got = _debug_block(model, 4, "estimator.ups.1.3", level, g["x32"] * mm, ones, None, 32, (2 * H, 2 * W))
    assert l1(got, g["up"]) <= tol
    # the attention module's own share: out - x is the Rezero branch alone (mean |.| of the branch printed for the record)
    branch = (g["attn"] - g["x32"]).abs().mean().item()
    print(f"\nblocks: attention L1 {e_attn:.2e} on a Rezero branch of mean |.| {branch:.2e}")


@pytest.mark.parametrize("tag,cfg", [("tiny", TINY), ("full", FULL)])
def test_time_embedding_vs_reference_golden(golden, tag, cfg):
    """`SinusoidalPosEmb` + mlp (unitspeech/unitspeech.py:109-121,133-134,165-166) on its own: `pos_emb_kernel` and the two `linear_kernel`
    launches of time_embedding() through us_debug_block(US_DEBUG_TEMB), against the reference module's outputs at t = 1e-5 ... 0.995
    (tests/golden/temb_*.npz; arguments of sin / cos up to 995: the range reduction is what this pins)."""
    g = G(golden(f"temb_{tag}"))
    model = make_model(cfg)
    eng = model._sync(torch.device(DEV))
    lib = eng.lib
    t = g["t"].to(DEV).contiguous()
    B, T, dim = t.shape[0], 8, cfg.dim
    out = torch.empty(B, 2 * dim, device=DEV)
    ws = torch.empty(int(lib.us_workspace_bytes(eng.handle, B, T)), dtype=torch.uint8, device=DEV)
    mask = torch.ones(B, T, device=DEV)
    rc = lib.us_debug_block(eng.handle, 5, b"", 0, C.c_void_p(t.data_ptr()), C.c_void_p(mask.data_ptr()), None, C.c_void_p(out.data_ptr()), B, T,
                            C.c_void_p(ws.data_ptr()), ws.numel(), None)
    _lib.check(rc, eng.handle, "us_debug_block(US_DEBUG_TEMB)")
    torch.cuda.synchronize()
    pe, mlp = out[:, :dim].cpu(), out[:, dim:].cpu()
    e_pe, e_mlp = (pe - g["posemb"]).abs().max().item(), (mlp - g["mlp"]).abs().max().item()
    print(f"\n[{tag}] time embedding: max |posemb - reference| {e_pe:.2e}, max |mlp - reference| {e_mlp:.2e} (mean |mlp| {g['mlp'].abs().mean():.3f})")
    # sin / cos of arguments up to 995 in fp32: one ulp of the ARGUMENT is 6e-5, the reference (libm sinf of the fp32 product) and a device
    # sinf of the same product agree to a few 1e-7
    assert e_pe <= 2e-6 and e_mlp <= 2e-6


# ---------------------------------------------------------------------------------------------------------------
# the reference's own execute_text_to_speech (same seeded front-end stand-ins) + fused de-normalisation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,cfg", [("tiny", TINY), ("full", FULL)])
def test_execute_text_to_speech_vs_reference(golden, tag, cfg):
    g = G(golden(f"tts_{tag}"))
    model = make_model(cfg)
    fe = SyntheticFrontEnd(cfg.n_feats, DEV)
    n, ylen = int(g["n_steps"]), int(g["y_length"])
    Tp = O.fix_len_compatibility(ylen, 3)
    rng = np.random.Generator(np.random.Philox(key=4242))
    z = torch.from_numpy(rng.standard_normal((1, cfg.n_feats, Tp), dtype=np.float32)).to(DEV)
    noise = torch.from_numpy(rng.standard_normal((n, 1, cfg.n_feats, Tp), dtype=np.float32)).to(DEV)
    ph, pl = text_to_ids(g["text"], DEV)
    orig = torch.randn_like
    torch.randn_like = lambda *a, **k: z.clone()
    try:
        enc, dec, attn = model.execute_text_to_speech(ph, pl, g["spk_emb"].to(DEV), fe.text_encoder, fe.duration_predictor, 3,
                                                      diffusion_steps=n, noise=noise)
        _, mel, _ = model.execute_text_to_speech(ph, pl, g["spk_emb"].to(DEV), fe.text_encoder, fe.duration_predictor, 3, diffusion_steps=n,
                                                 noise=noise, mel_range=(float(g["mel_min"]), float(g["mel_max"])))
    finally:
        torch.randn_like = orig
    assert tuple(dec.shape) == tuple(g["dec_out"].shape) and tuple(attn.shape) == tuple(g["attn"].shape)
    assert torch.equal(enc.cpu(), g["enc_out"])                         # a gather of cond_x columns: bit-exact
    assert torch.equal(attn.cpu(), g["attn"])
    e = l1(dec, g["dec_out"])
    print(f"\n[{tag}] execute_text_to_speech: decoder mel-L1 {e:.3e} (mean|out| {g['dec_out'].abs().mean():.1f})")
    assert e <= 1e-3
    # fused de-normalisation == inference.py:140 applied to this run's own normalised output, bit for bit; and within the
    # loop tolerance (scaled by (mel_max - mel_min) / 2) of the reference's de-normalised mel
    want = (dec + 1) / 2 * (g["mel_max"].to(DEV) - g["mel_min"].to(DEV)) + g["mel_min"].to(DEV)
    assert torch.equal(mel, want)
    assert l1(mel, g["mel"]) <= 1e-3 * float(g["mel_max"] - g["mel_min"]) / 2


def test_alignment_batched_ragged_vs_oracle():
    """us_tts_durations / us_tts_align on a ragged batch (masked symbols, zero-length tails, length_scale != 1) against the
    reference's `generate_path` + matmul formulation (oracle)."""
    lib = _lib.load()
    B, F, L = 3, 80, 23
    gen = np.random.Generator(np.random.Philox(key=99))
    cond_x = torch.from_numpy(gen.standard_normal((B, F, L), dtype=np.float32))
    frames = torch.from_numpy(gen.integers(1, 9, size=(B, 1, L)).astype(np.float32)) - 0.5
    x_mask = torch.ones(B, 1, L)
    x_mask[1, :, 15:] = 0
    x_mask[2, :, 1:] = 0
    logw = torch.log(frames) * x_mask
    for scale in (1.0, 1.5):
        cy, ym, at, n = O.align_conditioning(cond_x * x_mask, logw, x_mask, scale, 3)
        Tp = cy.shape[-1]
        d = lambda t: t.contiguous().to(DEV)
        w_ceil = torch.empty(B, L, device=DEV)
        ylen = torch.empty(B, dtype=torch.int64, device=DEV)
        lw, xm, cx = d(logw.reshape(B, L)), d(x_mask.reshape(B, L)), d(cond_x * x_mask)
        p = lambda t: C.c_void_p(t.data_ptr())
        assert lib.us_tts_durations(p(lw), p(xm), p(w_ceil), p(ylen), B, L, scale, None) == 0
        assert int(ylen.max()) == n
        cond_y = torch.empty(B, F, Tp, device=DEV)
        attn = torch.empty(B, L, Tp, device=DEV)
        y_mask = torch.empty(B, Tp, device=DEV)
        assert lib.us_tts_align(p(cx), p(w_ceil), p(xm), p(ylen), p(cond_y), p(attn), p(y_mask), B, F, L, Tp, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(cond_y.cpu(), cy) and torch.equal(attn.cpu(), at.squeeze(1)) and torch.equal(y_mask.cpu(), ym.squeeze(1))


# ---------------------------------------------------------------------------------------------------------------
# tape ownership, argument validation, weight invalidation
# ---------------------------------------------------------------------------------------------------------------
def test_backward_runs_on_its_own_forward():
    """forward A, forward B (different shape), backward A, backward B: each backward uses its own tape (one slot per handle used
    to make A's backward read B's activations); a consumed tape cannot be replayed."""
    model = make_model(TINY).train()

    def run(T, seed):
        inp = G(synthetic_inputs(TINY, 2, T, seed=seed))
        z = torch.from_numpy(np.random.Generator(np.random.Philox(key=seed)).standard_normal((2, 80, T), dtype=np.float32))
        with _ReplayRandn([z.to(DEV)]):
            loss, _ = model.loss_t(inp["z"].to(DEV), inp["mask"].to(DEV), inp["cond"].to(DEV), torch.tensor([0.3, 0.7], device=DEV),
                                   inp["spk_emb"].to(DEV))
        return loss

    def grads_of(loss, retain=False):
        for p in model.parameters():
            p.grad = None
        loss.backward(retain_graph=retain)
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    ref_a = grads_of(run(32, 1))
    ref_b = grads_of(run(16, 2))
    la, lb = run(32, 1), run(16, 2)          # A then B recorded ...
    ga = grads_of(la, retain=True)           # ... A's backward first
    gb = grads_of(lb)
    for k in ref_a:
        assert (ga[k] - ref_a[k]).abs().max() <= 1e-5 * ref_a[k].abs().max() + 1e-9, k      # fp32 atomics order only
        assert (gb[k] - ref_b[k]).abs().max() <= 1e-5 * ref_b[k].abs().max() + 1e-9, k
    with pytest.raises(RuntimeError, match="not live"):
        la.backward()                         # the tape was consumed


def test_shapes_are_validated_before_the_abi(full):
    z = torch.zeros(2, 80, 16, device=DEV)
    ok = dict(mask=torch.ones(2, 1, 16, device=DEV), cond=z, spk=torch.zeros(2, 1, 256, device=DEV))
    with pytest.raises(ValueError, match="mask"):
        full(z, torch.ones(1, 1, 16, device=DEV), ok["cond"], ok["spk"], 2, 1.0, 1.0, rng="philox")       # broadcastable in torch, not here
    with pytest.raises(ValueError, match="spk_emb"):
        full(z, ok["mask"], ok["cond"], torch.zeros(1, 1, 256, device=DEV), 2, 1.0, 1.0, rng="philox")
    with pytest.raises(ValueError, match="cond"):
        full(z, ok["mask"], torch.zeros(2, 80, 8, device=DEV), ok["spk"], 2, 1.0, 1.0, rng="philox")
    with pytest.raises(ValueError, match="z must be"):
        full(torch.zeros(2, 40, 16, device=DEV), ok["mask"], ok["cond"], ok["spk"], 2, 1.0, 1.0, rng="philox")
    with pytest.raises(ValueError, match="t must"):
        full.estimator(z, ok["mask"], z, torch.zeros(1, device=DEV), ok["spk"])


def test_invalidate_weights_after_in_place_data_write():
    model = make_model(TINY)
    inp = G(synthetic_inputs(TINY, 1, 16, seed=3))
    args = [inp[k].to(DEV) for k in ("z", "mask", "cond")] + [torch.full((1,), 0.4, device=DEV), inp["spk_emb"].to(DEV)]
    with torch.no_grad():
        a = model.estimator(*args).clone()
        model.estimator.final_conv.bias.data.add_(1.0)        # does not bump _version: the engine cannot see it
        model.invalidate_weights()
        b = model.estimator(*args)
    diff = (b - a) * inp["mask"].to(DEV)
    assert (diff - inp["mask"].to(DEV)).abs().max().item() <= 1e-6     # final_conv bias + 1 on every valid frame


# ---------------------------------------------------------------------------------------------------------------
# the fine-tune iteration as one HIP graph: same loss trajectory and parameters as the eager launches
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["graph", "eager"])
def test_finetune_graph_replay_matches_eager_iterations(backward):
    """backward="graph": forward + backward of an iteration replayed as one HIP graph; "eager" (FineTuneGraph's default): the forward
    replayed, `loss.backward(retain_graph=True)` launched per iteration on the tape the library keeps live (US_BACKWARD_KEEP_TAPE)."""
    import random
    from unitspeech_amd import FusedAdam
    from unitspeech_amd.graph import FineTuneGraph
    from unitspeech_amd.util import generate_path, sequence_mask
    gen = np.random.Generator(np.random.Philox(key=321))
    L, Lu, seg = 96, 32, 32
    y = torch.from_numpy(gen.standard_normal((1, 80, L), dtype=np.float32)).clamp(-1, 1).to(DEV)
    cond_x = torch.from_numpy(gen.standard_normal((1, 80, Lu), dtype=np.float32) * 0.5).to(DEV)
    y_len = torch.LongTensor([L]).to(DEV)
    y_mask = sequence_mask(y_len, L).unsqueeze(1).float()
    attn = generate_path(torch.full((1, Lu), 3.0, device=DEV), (torch.ones(1, 1, Lu, device=DEV).unsqueeze(-1) * y_mask.unsqueeze(2)).squeeze(1))
    spk = G(synthetic_inputs(TINY, 1, 8, seed=12))["spk_emb"].to(DEV)

    def run(use_graph, iters=5):
        model = make_model(TINY).train()
        opt = FusedAdam(model.parameters(), lr=1e-3)         # large enough that a missed weight re-pack would show in the next loss
        random.seed(7); torch.manual_seed(7)
        graph = FineTuneGraph(model, spk, 1, seg, 80, backward=backward) if use_graph else None
        losses = []
        for _ in range(iters):
            if graph is not None:
                loss = graph.step(cond_x, y, y_len, attn)
            else:
                loss = model.fine_tune(cond_x, y, y_mask, y_len, L, attn, spk, seg, 80)
                opt.zero_grad(set_to_none=True)
                loss.backward()
            opt.step(max_norm=1)
            losses.append(loss.item())
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    le, pe = run(False)
    lg, pg = run(True)
    print(f"\neager losses {le}\ngraph losses {lg}")
    assert len(set(le)) == len(le)                            # the iterations differ (new crop, new noise, new weights)
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a))           # fp32 atomics order is the only difference
    for k in pe:
        d = (pe[k] - pg[k]).abs()
        # Adam divides by sqrt(v): where a gradient is itself rounding noise (fp32 atomics order in the weight gradients) the update is
        # +-lr in either run; such elements may differ by a fraction of a step (lr = 1e-3), the tensors as a whole may not
        assert d.max() <= 2e-4 and d.mean() <= 1e-7, (k, d.max().item(), d.mean().item())


def test_f16x3_backward_matches_the_exact_fp32_backward_at_a_pretraining_batch():
    """Every parameter gradient of one full-size loss over 8 crops of 176 frames: the default backward (f16x3 GEMMs for forward, data
    and weight gradients, incoming gradient scaled by an exact power of two) against the exact-fp32 MFMA backward (the US_CREATE_EXACT_FP32 handle) of the
    same weights and draws.  dL/dscore is ~1e-5 here, below fp16's normal range: without the scaling the whole-gradient error is
    1.2e-6 and the median tensor is at 3.7e-6 (tools/grad_accuracy.py)."""
    import random
    cfg = FULL
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()}
    g = np.random.Generator(np.random.Philox(key=99))
    B, T = 8, 176
    x0 = torch.from_numpy(g.standard_normal((B, cfg.n_feats, T), dtype=np.float32)).clamp(-1, 1).to(DEV)
    cond = torch.from_numpy(g.standard_normal((B, cfg.n_feats, T), dtype=np.float32) * 0.5).to(DEV)
    mask = torch.ones(B, 1, T, device=DEV)
    spk = torch.from_numpy(g.standard_normal((B, 1, cfg.spk_emb_dim), dtype=np.float32)).to(DEV)
    spk = spk / spk.norm(dim=-1, keepdim=True)

    def grads(exact=False, loss_factor=1.0):
        m = UnitSpeech(cfg.n_feats, cfg.dim, list(cfg.dim_mults), cfg.beta_min, cfg.beta_max, cfg.pe_scale, cfg.spk_emb_dim)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        m.exact = exact
        random.seed(0); torch.manual_seed(0)
        loss, _ = m.compute_loss(x0, mask, cond, spk)
        (loss * loss_factor).backward()
        torch.cuda.synchronize()
        return float(loss), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}

    l_ref, ref = grads(exact=True)
    l_new, new = grads()
    assert len(ref) == 228 and abs(l_ref - l_new) <= 1e-6
    whole = float(torch.sqrt(sum(((new[n] - ref[n]) ** 2).sum() for n in ref)) / torch.sqrt(sum((ref[n] ** 2).sum() for n in ref)))
    per = sorted(float((new[n] - ref[n]).norm() / (ref[n].norm() + 1e-300)) for n in ref)
    median, worst = per[len(per) // 2], per[-1]
    print(f"\nf16x3 vs exact-fp32 backward, 8 crops: whole-gradient relative L2 {whole:.2e}, median tensor {median:.2e}, worst {worst:.2e}")
    # (the worst tensors are the scalar Rezero gains, sums with heavy cancellation whose last digits also move with the order of the
    # fp32 atomics in either run; without the scaling: whole 1.2e-6, median 3.7e-6)
    assert whole <= 6e-7 and median <= 1.5e-6 and worst <= 1e-4
    # the factor is taken from the data, so a caller's own (power-of-two) loss scaling changes nothing but the exponent: a summed
    # instead of a mean-reduced loss cannot push the scaled gradients out of fp16's range
    _, big = grads(loss_factor=float(2 ** 17))
    drift = float(torch.sqrt(sum(((big[n] * 2.0 ** -17 - new[n]) ** 2).sum() for n in new)) / torch.sqrt(sum((new[n] ** 2).sum() for n in new)))
    assert drift <= 3e-7, drift          # two runs differ by the order of their fp32 atomics only
