"""Voice conversion on the MI355X: the ContentVec encoder (Linear front on the fp32 matrix cores, csrc/encoder_train.hip; forward in
csrc/frontend.hip), the mel-rate alignment `us_vc_align` (csrc/glue.hip), `UnitSpeech.execute_voice_conversion`, the encoder's
training, and voice_conversion.py.  Goldens from the reference: tools/make_goldens_vc.py; fp64 yardsticks: tools/encoder_torch.py
and tools/vc_numpy.py (pinned to the reference by tests/test_vc.py).

Encoder bound: max(2e-5, 4 g) absolute, 2e-5 being the bar the id Encoder holds (tests/test_frontend.py) and g the reference's own
fp32-vs-fp64 gap stored with each golden (1.0e-6 tiny, 2.1e-6 full): 2e-5 in every case here.
Alignment bound: 4 * 2^-23 * max|x| against tools/vc_numpy.py in fp64.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import encoder_torch as ET  # noqa: E402
import vc_numpy as VN  # noqa: E402
from unitspeech_amd import DecoderConfig, UnitSpeech, _lib, synthetic_state_dict  # noqa: E402
from unitspeech_amd.encoder import ContentVecEncoder, EncoderConfig, _ContentVecEncoderTrain, synthetic_encoder_state_dict  # noqa: E402
from unitspeech_amd.unitspeech import vc_align  # noqa: E402

pytestmark = pytest.mark.gpu

TINY_E = EncoderConfig(n_vocab=20, n_feats=8, n_channels=16, filter_channels=32, n_heads=2, n_layers=2, kernel_size=3, window_size=4,
                       n_contentvec=12)
FULL_E = EncoderConfig(n_vocab=150, n_feats=80, n_channels=192, filter_channels=768, n_heads=2, n_layers=6, kernel_size=3, window_size=4,
                       n_contentvec=768)
CASES = {"vc_encoder_tiny": TINY_E, "vc_encoder_full": FULL_E}
TOL = 2e-5


def tol(g):
    return max(TOL, 4.0 * float(g))


def features(key, B, L, n):
    """tools/make_goldens_vc.py `features`."""
    g = np.random.Generator(np.random.Philox(key=key))
    return torch.from_numpy((g.standard_normal((B, L, n)) / np.sqrt(n)).astype(np.float32))


def make(cfg, seed=0, **kw):
    enc = ContentVecEncoder(cfg.n_vocab, cfg.n_feats, cfg.n_channels, cfg.filter_channels, cfg.n_heads, cfg.n_layers, cfg.kernel_size, 0.1,
                            n_contentvec=cfg.n_contentvec, window_size=cfg.window_size, **kw)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(cfg, seed).items()}, strict=True)
    return enc.cuda().train() if kw.get("trainable") else enc.cuda().eval()


def nan_past_lengths(feats, lengths):
    out = feats.clone()
    for b, n in enumerate(lengths):
        out[b, n:] = float("nan")
    return out


def maxerr(a, b):
    return float((a.double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


# ---- front and encoder ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_encoder_matches_the_reference_golden_and_never_reads_padded_rows(golden, name):
    g, cfg = golden(name), CASES[name]
    lens = [int(n) for n in g["lengths"]]
    B, L = len(lens), max(lens)
    feats = torch.from_numpy(g["feats"]) if "feats" in g else features(int(g["features"]), B, L, cfg.n_contentvec)
    enc, bound = make(cfg), tol(g["g"])
    lengths = torch.LongTensor(lens).cuda()
    mu_x, x, x_mask = enc(feats.cuda(), lengths)
    assert torch.equal(x_mask.cpu(), torch.from_numpy(g["x_mask"]).float())
    e_mu, e_x = maxerr(mu_x, g["mu_x"]), maxerr(x, g["x"])
    print(f"\n{name}: max |mu_x - fp64| {e_mu:.3e}, max |x - fp64| {e_x:.3e}, bound {bound:.1e} (g = {float(g['g']):.2e})")
    assert e_mu <= bound and e_x <= bound
    pad = x_mask == 0
    assert float(mu_x.abs().mul(pad).max()) == 0.0 and float(x.abs().mul(pad).max()) == 0.0
    # rows past each length hold NaN: they are not read
    mu_n, x_n, m_n = enc(nan_past_lengths(feats, lens).cuda(), lengths)
    assert torch.isfinite(mu_n).all() and torch.isfinite(x_n).all() and torch.equal(m_n, x_mask)
    assert maxerr(mu_n, g["mu_x"]) <= bound and maxerr(x_n, g["x"]) <= bound
    assert torch.equal(mu_n, mu_x) and torch.equal(x_n, x)
    # each item of the ragged batch against the same item alone
    for b, n in enumerate(lens):
        mu1, x1, _ = enc(feats[b:b + 1, :n].cuda(), lengths[b:b + 1])
        assert maxerr(mu1, mu_n[b:b + 1, :, :n]) <= bound and maxerr(x1, x_n[b:b + 1, :, :n]) <= bound


@pytest.mark.parametrize("n_contentvec,B,L,lens", [(40, 2, 35, [35, 20]), (12, 2, 9, [9, 4])])
def test_encoder_matches_the_fp64_restatement_on_other_reduction_lengths(n_contentvec, B, L, lens):
    """n_contentvec = 40: 2.5 reduction slices of 16, and 70 rows cross a 64-row tile; 12: below one slice."""
    cfg = EncoderConfig(20, 8, 16, 32, 2, 2, 3, 4, n_contentvec)
    feats = features(500 + n_contentvec, B, L, n_contentvec)
    sd = {k: torch.from_numpy(v) for k, v in synthetic_encoder_state_dict(cfg, 0).items()}
    lengths = torch.LongTensor(lens)
    r_mu, r_x, r_mask = ET.encoder_forward({k: v.double() for k, v in sd.items()}, cfg.n_heads, feats.double(), lengths)
    f_mu, f_x, _ = ET.encoder_forward(sd, cfg.n_heads, feats, lengths)
    bound = tol(max(maxerr(f_mu, r_mu), maxerr(f_x, r_x)))
    mu_x, x, x_mask = make(cfg)(nan_past_lengths(feats, lens).cuda(), lengths.cuda())
    assert torch.equal(x_mask.cpu(), r_mask.float())
    print(f"\nn_contentvec {n_contentvec}: max |mu_x - fp64| {maxerr(mu_x, r_mu):.3e}, max |x - fp64| {maxerr(x, r_x):.3e}, bound {bound:.1e}")
    assert maxerr(mu_x, r_mu) <= bound and maxerr(x, r_x) <= bound


def test_encoder_bits_do_not_depend_on_the_batch():
    """The reduction order of the front and the choice of convolution belong to the handle, never to B or L: an item alone has the
    bits it has in a batch."""
    cfg = EncoderConfig(20, 8, 16, 32, 2, 2, 3, 4, 40)
    feats, lens = features(77, 3, 70, 40), [70, 33, 1]
    enc = make(cfg)
    mu_x, x, _ = enc(feats.cuda(), torch.LongTensor(lens).cuda())
    for b, n in enumerate(lens):
        mu1, x1, _ = enc(feats[b:b + 1, :n].cuda(), torch.LongTensor([n]).cuda())
        assert torch.equal(mu1, mu_x[b:b + 1, :, :n]) and torch.equal(x1, x[b:b + 1, :, :n])


# ---- alignment --------------------------------------------------------------------------------------------------------------

def align_bound(x):
    return 4 * 2.0 ** -23 * float(np.abs(np.asarray(x)).max())


def test_align_ragged_batch_is_each_item_alone():
    x = np.random.Generator(np.random.Philox(key=91)).standard_normal((3, 5, 12)).astype(np.float32)
    xl, yl, Tp = [12, 7, 3], [21, 12, 5], 24
    dirty = x.copy()
    for b, n in enumerate(xl):
        dirty[b, :, n:] = np.nan                       # frames past an item's own length are not part of it
    cond_y, y_mask, y_lengths = vc_align(torch.from_numpy(dirty).cuda(), xl, torch.LongTensor(yl).cuda(), Tp)
    assert y_lengths.tolist() == yl and cond_y.shape == (3, 5, Tp) and y_mask.shape == (3, 1, Tp)
    ref_y, ref_m = VN.vc_align(x, xl, yl, Tp)
    assert torch.equal(y_mask.cpu().double(), torch.from_numpy(ref_m))
    assert maxerr(cond_y, ref_y) <= align_bound(x)
    for b in range(3):
        one, m1, _ = vc_align(torch.from_numpy(x[b:b + 1, :, :xl[b]]).cuda(), xl[b:b + 1], yl[b:b + 1], Tp)
        assert torch.equal(one, cond_y[b:b + 1]) and torch.equal(m1, y_mask[b:b + 1])
        assert float(cond_y[b, :, yl[b]:].abs().max()) == 0.0 and not torch.signbit(cond_y[b, :, yl[b]:]).any()


@pytest.mark.parametrize("lx,ly", [(1, 5), (12, 7), (13, 13), (37, 64), (499, 860), (1499, 2583)])
def test_align_matches_the_fp64_statement(lx, ly):
    x = np.random.Generator(np.random.Philox(key=lx * 10007 + ly)).standard_normal((1, 3, lx)).astype(np.float32)
    Tp = ly + 3
    cond_y, y_mask, _ = vc_align(torch.from_numpy(x).cuda(), [lx], [ly], Tp)
    ref_y, ref_m = VN.vc_align(x, [lx], [ly], Tp)
    err = maxerr(cond_y, ref_y)
    print(f"\n{lx} -> {ly}: max err {err:.3e} = {err / (2.0 ** -23 * np.abs(x).max()):.2f} x 2^-23 max|x|")
    assert err <= align_bound(x)
    assert torch.equal(y_mask.cpu().double(), torch.from_numpy(ref_m)) and float(cond_y[:, :, ly:].abs().max()) == 0.0
    if lx == ly:
        assert torch.equal(cond_y[:, :, :ly].cpu(), torch.from_numpy(x))


def test_align_refuses_lengths_out_of_range_before_any_launch():
    x = torch.zeros(2, 4, 12, device="cuda")
    for xl, yl, Tp in (([0, 5], [8, 8], 8), ([13, 5], [8, 8], 8), ([12, 5], [9, 8], 8), ([12, 5], [8, 0], 8), ([12], [8], 8), ([12, 5], [8, 8], 0)):
        with pytest.raises(ValueError):
            vc_align(x, xl, yl, Tp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vc_align(x.cpu(), [12, 5], [8, 8], 8)


# ---- end to end -------------------------------------------------------------------------------------------------------------

DEC = DecoderConfig(dim=16)
VC_E = EncoderConfig(n_vocab=20, n_feats=DEC.n_feats, n_channels=16, filter_channels=32, n_heads=2, n_layers=2, kernel_size=3, window_size=4,
                     n_contentvec=12)


@pytest.fixture(scope="module")
def decoder():
    m = UnitSpeech(DEC.n_feats, DEC.dim, list(DEC.dim_mults), DEC.beta_min, DEC.beta_max, DEC.pe_scale, DEC.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(DEC, 0).items()})
    return m.cuda().eval()


class fixed_randn_like:
    """torch.randn_like replaced by a given draw: z of execute_voice_conversion (the reference's randn_like, :35)."""

    def __init__(self, z):
        self.z = z

    def __enter__(self):
        self.orig = torch.randn_like
        torch.randn_like = lambda t, *a, **k: self.z[:, :, :t.shape[-1]].clone()

    def __exit__(self, *a):
        torch.randn_like = self.orig


def test_execute_voice_conversion_matches_the_reference_function(golden, decoder):
    """The reference's voice_conversion() with its own Encoder(n_contentvec=12) and decoder against the same call on the HIP modules.

    cond_y is held to the alignment bound against the fp64 statement applied to the HIP encoder's own output, and to that bound plus
    the encoder's 2e-5 plus the reference's fp32 coordinate error (59 * 2^-24 max|x| at 9 -> 15, derived in tests/test_vc.py) against
    the golden; decoder_outputs to mean-L1 1e-3, the bar of the tiny loop tests (tests/test_hip_parity.py, loop_tiny_N10_*)."""
    g = golden("vc_tiny")
    enc = make(VC_E, seed=1)
    feats, lens, spk = (torch.from_numpy(g[k]).cuda() for k in ("feats", "lengths", "spk_emb"))
    n_steps, tp, mel_length = int(g["n_steps"]), int(g["tp"]), int(g["mel_length"])
    gz = np.random.Generator(np.random.Philox(key=int(g["noise_key"])))
    z = torch.from_numpy(gz.standard_normal((1, DEC.n_feats, tp), dtype=np.float32)).cuda()
    noise = torch.from_numpy(np.stack([gz.standard_normal((1, DEC.n_feats, tp), dtype=np.float32) for _ in range(n_steps)])).cuda()
    with fixed_randn_like(z):
        cond_y, dec = decoder.execute_voice_conversion(feats, lens, [mel_length], spk, enc, len(DEC.dim_mults) - 1, diffusion_steps=n_steps,
                                                       text_gradient_scale=1.0, spk_gradient_scale=1.0, noise=noise)
    assert cond_y.shape == (1, DEC.n_feats, mel_length) and dec.shape == (1, DEC.n_feats, mel_length)
    cond_x = enc(feats, lens)[0].cpu().numpy()
    own, _ = VN.vc_align(cond_x, [feats.shape[1]], [mel_length], tp)
    a = align_bound(cond_x)
    e_own, e_gold = maxerr(cond_y, own[:, :, :mel_length]), maxerr(cond_y, g["cond_y"][:, :, :mel_length])
    e_dec = float((dec.double().cpu() - torch.from_numpy(g["decoder_outputs"]).double()).abs().mean())
    print(f"\ncond_y vs fp64 of own encoder output {e_own:.3e} (bound {a:.3e}); vs golden {e_gold:.3e}; decoder mel-L1 {e_dec:.3e}")
    assert e_own <= a
    assert e_gold <= a + TOL + 59 * 2.0 ** -24 * float(np.abs(g["cond_x"]).max())
    assert e_dec <= 1e-3


def test_execute_voice_conversion_ragged_batch_equals_single_runs(decoder):
    """B = 2 of different ContentVec and mel lengths under rng="philox": each item's frames equal its B = 1 run (utt_offset = its index,
    the same z).  Both mel lengths pad to the same U-Net length, so the B = 1 runs draw the same z rows."""
    enc = make(VC_E, seed=1)
    feats, cv, mel = features(61, 2, 9, 12).cuda(), [9, 8], [15, 13]
    spk = torch.from_numpy(np.random.Generator(np.random.Philox(key=62)).standard_normal((2, 1, DEC.spk_emb_dim), dtype=np.float32)).cuda()
    z = torch.from_numpy(np.random.Generator(np.random.Philox(key=63)).standard_normal((2, DEC.n_feats, 16), dtype=np.float32)).cuda()
    n_down = len(DEC.dim_mults) - 1
    with fixed_randn_like(z):
        cond_y, dec, y_lengths = decoder.execute_voice_conversion(feats, torch.LongTensor(cv).cuda(), mel, spk, enc, n_down, diffusion_steps=3,
                                                                  return_lengths=True, rng="philox", seed=11)
    assert y_lengths.tolist() == mel and dec.shape[-1] == max(mel) and torch.isfinite(dec).all()
    for b in range(2):
        with fixed_randn_like(z[b:b + 1]):
            c1, d1, l1 = decoder.execute_voice_conversion(feats[b:b + 1, :cv[b]], torch.LongTensor(cv[b:b + 1]).cuda(), mel[b:b + 1], spk[b:b + 1],
                                                          enc, n_down, diffusion_steps=3, return_lengths=True, rng="philox", seed=11, utt_offset=b)
        assert l1.tolist() == [mel[b]]
        assert torch.equal(c1, cond_y[b:b + 1, :, :mel[b]]) and torch.equal(d1, dec[b:b + 1, :, :mel[b]])


# ---- training ---------------------------------------------------------------------------------------------------------------

def err(a, b, floor):
    a, b = torch.as_tensor(a).double().cuda(), torch.as_tensor(b).double().cuda()
    return float((a - b).norm() / b.norm().clamp_min(floor))


def worst_key(grads, rgrads):
    """tests/test_encoder_train_gpu.py `worst_key`: per key relative to its norm (floored at 1e-6 of the largest key norm); the key
    bias's gradient is analytically zero and is bounded against the largest key norm instead."""
    scale = max(float(v.norm()) for v in rgrads.values() if v is not None)
    out = []
    for k, g in grads.items():
        r = rgrads[k] if rgrads[k] is not None else torch.zeros_like(g, dtype=torch.float64)
        if k.endswith("conv_k.bias"):
            out.append((float((g.double() - r).norm()) / scale * 10, k))
        else:
            out.append((err(g, r, 1e-6 * scale), k))
    return max(out)


def hip_grads(enc, feats, lens, g_mu, g_x, p, seed=0):
    for t in enc.parameters():
        t.grad = None
    params = list(enc.state_dict(keep_vars=True).values())
    mu_x, x, _ = _ContentVecEncoderTrain.apply(enc, feats, lens, seed, p, *params)
    ((mu_x * g_mu).sum() + (x * g_x).sum()).backward()
    return mu_x.detach(), x.detach(), {k: t.grad for k, t in enc.named_parameters()}


def ref_grads(cfg, feats, lens, g_mu, g_x, masks=None):
    sd = {k: torch.from_numpy(v).cuda().double().requires_grad_(True) for k, v in synthetic_encoder_state_dict(cfg, 0).items()}
    mu_x, x, _ = ET.encoder_forward(sd, cfg.n_heads, feats.double(), lens, {k: v.double() for k, v in (masks or {}).items()})
    ((mu_x * g_mu.double()).sum() + (x * g_x.double()).sum()).backward()
    return mu_x.detach(), x.detach(), {k: v.grad for k, v in sd.items()}


def test_gradients_match_the_reference_golden_in_eval_mode(golden):
    """Every key against the reference class in fp64; the bar of tests/test_encoder_train_gpu.py's tiny golden test: relative to the
    key's norm, max(10 x the reference's own fp32-vs-fp64 distance, 1e-5)."""
    g = golden("vc_encoder_train_tiny")
    enc = make(TINY_E, trainable=True)
    T = lambda k: torch.from_numpy(g[k]).cuda()
    lens = [int(n) for n in g["lengths"]]
    mu_x, x, grads = hip_grads(enc, nan_past_lengths(T("feats"), lens), T("lengths"), T("g_mu"), T("g_x"), -1.0)
    assert maxerr(mu_x, g["mu_x"]) <= TOL and maxerr(x, g["x"]) <= TOL
    worst = {}
    for k, v in grads.items():
        ref = g["g64/" + k]
        assert torch.isfinite(v).all(), k
        if np.linalg.norm(ref) < 1e-10:                       # analytically zero (key bias)
            assert float(v.norm()) < 1e-4, k
            continue
        spread = err(g["g32/" + k], ref, 1e-3)
        worst[k] = err(v, ref, 1e-3)
        assert worst[k] <= max(10 * spread, 1e-5), (k, worst[k], spread)
    assert grads["emb.weight"].shape == (16, 12)
    print("\ntiny golden, worst key:", max(worst.items(), key=lambda kv: kv[1]), "emb.weight:", worst["emb.weight"])


def dropout_masks(enc, seed, B, L):
    lib, c, out = _lib.load(), enc.cfg, {}
    for site in range(3 + 4 * c.n_layers):
        w = (site - 3) % 4
        shape = (B, c.n_heads, L, L) if site >= 3 and w == 0 else (B, c.filter_channels if site >= 3 and w == 2 else c.n_channels, L)
        m = torch.empty(shape, device="cuda")
        enc._check(lib, lib.us_encoder_dropout_mask(enc._h, seed, site, B, L, enc.p_dropout, m.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "us_encoder_dropout_mask")
        out[site] = m
    return out


def test_dropout_masks_reproduce_outputs_and_gradients():
    """Dropout on: against the fp64 restatement fed the kernel's own keep masks (bar of tests/test_encoder_train_gpu.py: 1e-4 of the
    key's norm, outputs 5e-5)."""
    cfg, B, L = TINY_E, 3, 19
    gen = torch.Generator().manual_seed(5)
    feats = features(71, B, L, cfg.n_contentvec).cuda()
    lens = torch.LongTensor([19, 12, 5]).cuda()
    g_mu, g_x = torch.randn(B, cfg.n_feats, L, generator=gen).cuda(), torch.randn(B, cfg.n_channels, L, generator=gen).cuda()
    enc = make(cfg, trainable=True)
    mu_x, x, grads = hip_grads(enc, feats, lens, g_mu, g_x, 0.1, seed=1234)
    rmu, rx, rgrads = ref_grads(cfg, feats, lens, g_mu, g_x, dropout_masks(enc, 1234, B, L))
    assert maxerr(mu_x, rmu) <= 5e-5 and maxerr(x, rx) <= 5e-5
    worst = worst_key(grads, rgrads)
    print("\ndropout, worst key:", worst)
    assert worst[0] <= 1e-4, worst
    # the module's own call: train mode draws a seed from torch's generator, and autograd reaches every parameter
    torch.manual_seed(3)
    a = enc(feats, lens)
    torch.manual_seed(3)
    b = enc(feats, lens)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    (a[0].sum() + a[1].sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters())


def test_front_weight_gradient_across_slices_and_row_tiles():
    """emb.weight.grad at n_contentvec = 40 (2.5 slices), B = 2, L = 35 (70 rows: two row tiles of the forward, a partial reduction slice
    of the weight-gradient GEMM), padded feature rows NaN, against the fp64 restatement at 1e-4 of the key's norm."""
    cfg = EncoderConfig(20, 8, 16, 32, 2, 2, 3, 4, 40)
    B, L, lens = 2, 35, [35, 20]
    gen = torch.Generator().manual_seed(9)
    feats = features(540, B, L, 40)
    g_mu, g_x = torch.randn(B, cfg.n_feats, L, generator=gen).cuda(), torch.randn(B, cfg.n_channels, L, generator=gen).cuda()
    lengths = torch.LongTensor(lens).cuda()
    _, _, grads = hip_grads(make(cfg, trainable=True), nan_past_lengths(feats, lens).cuda(), lengths, g_mu, g_x, -1.0)
    _, _, rgrads = ref_grads(cfg, feats.cuda(), lengths, g_mu, g_x)
    e = err(grads["emb.weight"], rgrads["emb.weight"], 1e-6)
    print(f"\nemb.weight.grad [16, 40]: relative error {e:.3e}; worst key {worst_key(grads, rgrads)}")
    assert torch.isfinite(grads["emb.weight"]).all() and e <= 1e-4
    assert worst_key(grads, rgrads)[0] <= 1e-4


# ---- command line -----------------------------------------------------------------------------------------------------------

def test_voice_conversion_cli_synthetic(tmp_path):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    from voice_conversion import synthetic_sources
    r = subprocess.run([sys.executable, os.path.join(ROOT, "voice_conversion.py"), "--synthetic", "3", "--batch", "2", "--diffusion_step", "4",
                        "--out", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("batch of ")]
    assert len(lines) == 2 and "batch of 2 sources" in lines[0] and "batch of 1 sources" in lines[1]
    assert all("contentvec frames" in ln and "mel frames" in ln and "samples written" in ln for ln in lines)
    for name, w in synthetic_sources(3, 0):
        rate, data = wavfile.read(str(tmp_path / f"{name}.wav"))
        assert rate == 22050 and data.dtype == np.float32 and data.shape == ((len(w) // 256) * 256,)
        assert np.isfinite(data).all() and np.abs(data).max() <= 1.0
