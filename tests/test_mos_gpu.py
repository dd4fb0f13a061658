"""The MOS predictor on the GPU (csrc/mos.hip, unitspeech_amd/mos.py).

Accuracy bar: the yardstick is tools/mos_torch.py's `mos_head_numpy` in fp64 (the unfolded model, step by step), never the library itself.
For every case and every compared tensor (the case's scores, every mu entry, every alpha entry) each entry's distance from fp64 is at most
10 x the largest distance the same restatement run in fp32 has on that tensor of that case, with a floor of 1e-6 * max |fp64 value|.
Every check prints the two distances.  An item of a ragged batch is compared with the item run alone for BIT equality.

Shapes: H in {4, 40, 768} (one piece in 1 lane; 10 pieces; 3 pieces per lane), n_states in {1, 3, 13} (a tail alone; a tail of 3; three
groups of four and a tail), B = 3 and B = 17 with lengths drawn from {1, 2, 63, 64, 65, 255, 256, 257, 600} at Tmax = 600: the seams of
the pool's stride of 256, one and several frames per thread.  Each case runs both layouts, both poolings and the clipping on and off on one
set of hidden states; rows past an item's length hold NaN throughout."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mos_torch as M  # noqa: E402

from unitspeech_amd import _args, _lib, mos  # noqa: E402
from unitspeech_amd.hubert import HubertModel  # noqa: E402

pytestmark = pytest.mark.gpu

TMAX = 600
SEAMS = [1, 2, 63, 64, 65, 255, 256, 257, 600]
P_OF = {4: 8, 40: 16, 768: 256}


def check(tag, got, r64, r32):
    """got, r64, r32: the same values from the library, the fp64 yardstick and its fp32 run; every entry of `got` is held to the bar"""
    got, r64, r32 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, r64, r32))
    e = float(np.abs(got - r64).max())
    s = float(np.abs(r32 - r64).max())
    mag = float(np.abs(r64).max())
    print(f"{tag}: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.3f}")
    assert np.isfinite(got).all() and e <= max(10 * s, 1e-6 * mag), (tag, e, s, mag)
    return e, s


def lengths_of(H, n, B):
    g = np.random.Generator(np.random.Philox(key=1000 * H + 10 * n + B))
    if B >= len(SEAMS):                                     # every seam at least once
        return [int(v) for v in g.permutation(SEAMS + [int(v) for v in g.choice(SEAMS, B - len(SEAMS))])]
    return [int(v) for v in g.choice(SEAMS, B, replace=False)]


def make_head(w, H, n, P, attention, clipping=False):
    head = mos.MOSHead(H, n, P, attention_pooling=attention, clipping=clipping)
    head.load_state_dict({k: v for k, v in w.items() if attention or not k.startswith(M.ATT)})
    return head.cuda()


@functools.lru_cache(maxsize=2)
def case(H, n, B):
    """One set of hidden states [B, n, TMAX, H] (NaN past each length), weights, and per item the yardstick in fp64 and fp32, unclipped,
    for both poolings: ref[attention][dtype][b] = (score, mu, alpha)."""
    P, lens = P_OF[H], lengths_of(H, n, B)
    g = torch.Generator().manual_seed(7 * H + n + B)
    hs = torch.full((B, n, TMAX, H), float("nan"))
    for b, F in enumerate(lens):
        hs[b, :, :F] = torch.randn(n, F, H, generator=g)
    w = M.synthetic_mos_weights(n, H, P, seed=H + n)
    ref = {a: {d: [M.mos_head_numpy(w, hs[b, :, :F].numpy(), d, a, False) for b, F in enumerate(lens)] for d in (np.float64, np.float32)}
           for a in (True, False)}
    return hs, w, lens, ref


def clip(score, dtype):
    return dtype(dtype(2.0) * np.tanh(dtype(score)) + dtype(3.0))


def padded(rows, lens):
    out = np.zeros((len(lens), TMAX))
    for b, F in enumerate(lens):
        out[b, :F] = rows[b]
    return out


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("n", [1, 3, 13])
@pytest.mark.parametrize("H", [4, 40, 768])
def test_head_against_the_fp64_restatement(H, n, B):
    hs, w, lens, ref = case(H, n, B)
    dev = hs.cuda()
    by_layout = {"blhd": dev, "lbhd": dev.transpose(0, 1).contiguous()}
    for attention in (True, False):
        head = make_head(w, H, n, P_OF[H], attention)
        r64, r32 = ref[attention][np.float64], ref[attention][np.float32]
        first = None
        for layout, x in by_layout.items():
            for clipping in (False, True):
                head.clipping = clipping
                scores, mu, alpha = head(x, lens, layout, return_frames=True)
                assert tuple(scores.shape) == (B,) and tuple(mu.shape) == tuple(alpha.shape) == (B, TMAX)
                tag = f"H{H} n{n} B{B} {layout} {'attention' if attention else 'mean'}{' clipped' if clipping else ''}"
                want = [[clip(r[b][0], d) if clipping else r[b][0] for b in range(B)] for r, d in ((r64, np.float64), (r32, np.float32))]
                check(tag + " score", scores.cpu().numpy(), want[0], want[1])
                check(tag + " mu", mu.cpu().numpy(), padded([r[1] for r in r64], lens), padded([r[1] for r in r32], lens))
                check(tag + " alpha", alpha.cpu().numpy(), padded([r[2] for r in r64], lens), padded([r[2] for r in r32], lens))
                for b, F in enumerate(lens):               # 0.0 past each length
                    assert (mu[b, F:] == 0).all() and (alpha[b, F:] == 0).all()
                assert torch.equal(head(x, lens, layout), scores)                                    # without the optional outputs
                if not clipping:                           # the two layouts hold the same numbers: the same bits
                    if first is None:
                        first = (scores, mu, alpha)
                    else:
                        assert all(torch.equal(u, v) for u, v in zip(first, (scores, mu, alpha)))


def test_folded_pack_against_fp64():
    """The pack itself: s, v_e, v_m, k_e, k_m are the fp64 fold rounded to fp32 once (half an ulp, plus the device's exp in the softmax)."""
    n, H, P = 13, 768, 256
    w = M.synthetic_mos_weights(n, H, P, seed=3)
    head = make_head(w, H, n, P, True)
    s, ve, vm, k = (t.cpu().double().numpy() for t in head.folded(torch.device("cuda:0")))
    fs, fve, fvm, fke, fkm = M.mos_fold_numpy(w)
    for tag, got, want in (("s", s, fs), ("v_e", ve, fve), ("v_m", vm, fvm), ("k", k, np.array([fke, fkm]))):
        e, mag = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"pack {tag}: {e:.3e} of max |value| {mag:.3f}")
        assert e <= 2.0 ** -23 * mag, (tag, e, mag)


def test_a_shift_of_the_attention_bias_changes_nothing():
    H, n, B = 40, 3, 17
    hs, w, lens, ref = case(H, n, B)
    shifted = dict(w)
    shifted[M.ATT + "bias"] = w[M.ATT + "bias"] + 100.0
    r64, r32 = ref[True][np.float64], ref[True][np.float32]
    scores, mu, alpha = make_head(shifted, H, n, P_OF[H], True)(hs.cuda(), lens, return_frames=True)
    assert torch.isfinite(scores).all()
    check("a0 + 100 score", scores.cpu().numpy(), [r[0] for r in r64], [r[0] for r in r32])
    check("a0 + 100 alpha", alpha.cpu().numpy(), padded([r[2] for r in r64], lens), padded([r[2] for r in r32], lens))


@pytest.mark.parametrize("H,n", [(40, 3), (768, 13)])
def test_an_item_has_the_same_bits_wherever_it_lies(H, n):
    hs, w, lens, _ = case(H, n, 17)
    head = make_head(w, H, n, P_OF[H], True, clipping=True)
    dev = hs.cuda()
    scores, mu, alpha = head(dev, lens, return_frames=True)
    again = head(dev, lens, return_frames=True)
    assert all(torch.equal(u, v) for u, v in zip((scores, mu, alpha), again))                          # a repeated call
    three = [0, 8, 16]
    s3, mu3, al3 = head(dev[three], [lens[b] for b in three], return_frames=True)                    # in B = 3
    assert torch.equal(s3, scores[three]) and torch.equal(mu3, mu[three]) and torch.equal(al3, alpha[three])
    wide = torch.full((17, n, TMAX + 101, H), float("nan"), device="cuda")                           # at a larger Tmax
    wide[:, :, :TMAX] = dev
    sw, muw, alw = head(wide, lens, return_frames=True)
    assert torch.equal(sw, scores) and torch.equal(muw[:, :TMAX], mu) and torch.equal(alw[:, :TMAX], alpha) and (muw[:, TMAX:] == 0).all()
    for b in sorted({lens.index(F) for F in set(lens)}):                                             # alone, at Tmax = its own frames
        F = lens[b]
        s1, mu1, al1 = head(dev[b:b + 1, :, :F], None, return_frames=True)
        assert torch.equal(s1[0], scores[b]) and torch.equal(mu1[0], mu[b, :F]) and torch.equal(al1[0], alpha[b, :F]), (b, F)


def raw_score(hs, lens, head, B, T, n, H, scores, mu, alpha, ws, ws_bytes, clipping=0):
    """us_mos_score itself on blhd hidden states -> its return code"""
    lib = _lib.load()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    return lib.us_mos_score(ptr(hs), n * T * H, T * H, ptr(lens), ptr(head.packed(hs.device)), B, T, n, H, clipping, ptr(scores), ptr(mu),
                            ptr(alpha), ptr(ws), ws_bytes, _args.stream())


def test_padding_and_canaries():
    H, n, P, T = 40, 3, 16, 300
    lens = [257, 1, 64]
    B, G, canary = len(lens), 64, 1234.5
    g = torch.Generator().manual_seed(11)
    clean = torch.randn(B, n, T, H, generator=g)
    w = M.synthetic_mos_weights(n, H, P, seed=2)
    head = make_head(w, H, n, P, True)
    want = head(clean.cuda(), lens, return_frames=True)
    dirty = clean.clone()
    for b, F in enumerate(lens):
        dirty[b, :, F:] = float("nan")                    # rows past an item's length: never read
    lens_d = torch.tensor(lens, dtype=torch.int64).cuda()
    bufs = [torch.full((G + m + G,), canary, device="cuda") for m in (B, B * T, B * T)]
    scores, mu, alpha = (buf[G:-G] for buf in bufs)
    nbytes = int(_lib.load().us_mos_workspace_bytes(B, T))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert raw_score(dirty.cuda(), lens_d, head, B, T, n, H, scores, mu, alpha, ws, nbytes) == 0
    torch.cuda.synchronize()
    for buf in bufs:                                      # nothing before the first row, nothing past the last
        assert (buf[:G] == canary).all() and (buf[-G:] == canary).all()
    assert torch.equal(scores, want[0]) and torch.equal(mu.view(B, T), want[1]) and torch.equal(alpha.view(B, T), want[2])
    for b, F in enumerate(lens):
        assert (mu.view(B, T)[b, F:] == 0).all() and (alpha.view(B, T)[b, F:] == 0).all()
        assert abs(float(alpha.view(B, T)[b].double().sum()) - 1.0) <= 1e-5
    # one output alone: the other buffer is not touched
    bufs[2].fill_(canary)
    assert raw_score(dirty.cuda(), lens_d, head, B, T, n, H, scores, mu, None, ws, nbytes) == 0
    torch.cuda.synchronize()
    assert (bufs[2] == canary).all()


def test_an_item_of_no_frames_gets_nan_and_its_neighbours_keep_their_bits():
    H, n, P, T = 40, 3, 16, 70
    g = torch.Generator().manual_seed(12)
    hs = torch.randn(3, n, T, H, generator=g).cuda()
    head = make_head(M.synthetic_mos_weights(n, H, P, seed=2), H, n, P, True)
    for clipping in (False, True):
        head.clipping = clipping
        scores, mu, alpha = head(hs, [65, 0, 5], return_frames=True)
        assert torch.isnan(scores[1]) and (mu[1] == 0).all() and (alpha[1] == 0).all()
        for b, F in ((0, 65), (2, 5)):
            s1, mu1, al1 = head(hs[b:b + 1, :, :F], None, return_frames=True)
            assert torch.equal(s1[0], scores[b]) and torch.equal(mu1[0], mu[b, :F]) and torch.equal(al1[0], alpha[b, :F])
    mean = make_head(M.synthetic_mos_weights(n, H, P, seed=2), H, n, P, False)
    assert torch.isnan(mean(hs, [65, 0, 5])[1])


def test_refusals_write_nothing():
    lib = _lib.load()
    assert lib.us_mos_packed_bytes(3, 40, 16) == (8 + 32 + 2 * 40) * 4 and lib.us_mos_workspace_bytes(3, 70) == 3 * 70 * 8
    for bad in ((3, 6, 16), (3, 1028, 16), (33, 40, 16), (0, 40, 16), (3, 40, 0), (3, 40, 4097), (3, 0, 16)):
        assert lib.us_mos_packed_bytes(*bad) == 0, bad
    assert lib.us_mos_workspace_bytes(0, 5) == 0 and lib.us_mos_workspace_bytes(70000, 5) == 0
    H, n, P, T, B, canary = 40, 3, 16, 70, 2, 77.0
    head = make_head(M.synthetic_mos_weights(n, H, P, seed=2), H, n, P, True)
    hs = torch.randn(B, n, T, 1032).cuda()
    nbytes = int(lib.us_mos_workspace_bytes(B, T))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    scores, mu = torch.full((B,), canary).cuda(), torch.full((B, T), canary).cuda()
    for what, (nn, HH, wsb) in {"H = 6": (n, 6, nbytes), "H = 1028": (n, 1028, nbytes), "33 states": (33, H, nbytes),
                                "a short workspace": (n, H, nbytes - 1)}.items():
        assert raw_score(hs, None, head, B, T, nn, HH, scores, mu, None, ws, wsb) == -1, what
        assert lib.us_last_error(None)
    # the pack of the same sizes
    packed = torch.full((1024,), canary).cuda()
    z = torch.zeros(4096 * 8).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for nn, HH, PP in ((3, 6, 16), (3, 1028, 16), (33, 40, 16), (3, 40, 4097)):
        assert lib.us_mos_pack_head(ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), nn, HH, PP, ptr(packed), 4096, _args.stream()) == -1
    assert lib.us_mos_pack_head(ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), 3, 40, 16, ptr(packed), 100, _args.stream()) == -1
    torch.cuda.synchronize()
    assert (scores == canary).all() and (mu == canary).all() and (packed == canary).all()
    # a head packed for other sizes than the call names: NaN, not a read past the pack
    out = torch.zeros(B).cuda()
    assert raw_score(hs, None, head, B, T, n, 44, out, None, None, ws, nbytes) == 0
    assert torch.isnan(out).all()
    with pytest.raises(RuntimeError, match="GPU only"):
        head(torch.zeros(1, n, 5, H))
    with pytest.raises(ValueError, match="hidden_states"):
        head(torch.zeros(1, n + 1, 5, H).cuda())


@pytest.mark.parametrize("name", ["mos_a", "mos_b"])
def test_predictor_end_to_end_on_the_golden(golden, name):
    """Waveform -> score through `MOSPredictor`, one ragged batch of four and one by one: within max(10 x the distance of the fp32
    restatement (tools/hubert_torch.py + MosTorch) from the fp64 golden, 1e-5), all four variants; batch and solo bits equal."""
    g = golden(name)
    cfg, hc = json.loads(str(g["config"])), json.loads(str(g["head"]))
    up_sd = {k[2:]: torch.from_numpy(g[k]) for k in g if k.startswith("w:")}
    hw = {k[2:]: torch.from_numpy(g[k]) for k in g if k.startswith("h:")}
    items = int(g["n_items"])
    wavs = [torch.from_numpy(g[f"wav_{i}"]) for i in range(items)]
    lens = [int(w.shape[0]) for w in wavs]
    batch = torch.zeros(items, max(lens))
    for i, w in enumerate(wavs):
        batch[i, :lens[i]] = w
    upstream = HubertModel(**cfg)
    upstream.load_state_dict(up_sd)
    upstream = upstream.cuda().eval()
    m32 = M.MosTorch(hw, torch.float32)
    for v, (attention, clipping) in enumerate(((True, False), (True, True), (False, False), (False, True))):
        pred = mos.MOSPredictor(upstream, make_head(hw, hc["hidden_size"], hc["n_states"], hc["projector_dim"], attention, clipping)).eval()
        got = pred(batch.cuda(), lens)
        r32 = [float(m32.predict(up_sd, cfg, w, clipping, attention)) for w in wavs]
        e = float(np.abs(got.cpu().double().numpy() - g["scores"][:, v]).max())
        s = float(np.abs(np.array(r32) - g["scores"][:, v]).max())
        print(f"{name} predictor {'attention' if attention else 'mean'}{' clipped' if clipping else ''}: library {e:.3e}  fp32 restatement {s:.3e}")
        assert np.isfinite(e) and e <= max(10 * s, 1e-5), (e, s)
        for i, w in enumerate(wavs):
            assert torch.equal(pred(w[None].cuda())[0], got[i]), i
        if attention and not clipping:
            sc, mu, alpha = pred.score_frames(batch.cuda(), lens)
            assert torch.equal(sc, got)
            F = g[f"mu_{items - 1}"].shape[0]
            assert tuple(mu.shape) == (items, F) and (mu[0, 1:] == 0).all() and (alpha[0, 1:] == 0).all()
            assert float(np.abs(alpha[items - 1].cpu().double().numpy() - g[f"alpha_{items - 1}"]).max()) <= max(10 * s, 1e-5)
