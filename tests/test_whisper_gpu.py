"""The HIP Whisper recogniser (csrc/whisper.hip, the encoder schedule in csrc/hubert.hip, us_whisper_*) on the GPU against the goldens written
from transformers.WhisperForConditionalGeneration in fp64.

Accuracy bar for the encoder's hidden states and the teacher-forced logits (the rule of test_hubert_gpu.py and smoke()): the library's max
distance from the golden is at most 10 x the distance of the restatement (tools/whisper_torch.py) run in fp32 on the same input, with a floor
of 1e-5 * max |golden|.  Both distances are printed.  Tokens and lengths are compared exactly: the goldens were written only where the worst
top-1 / top-2 margin is 1e-3 of the largest logit, a hundred times the bar above.

An item in a batch is compared with the item alone for BIT equality (logits and tokens), as everywhere in this library."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd import _lib  # noqa: E402
from unitspeech_amd.whisper import WhisperForConditionalGeneration, detect_language  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}


def setup(name):
    """the golden, its configuration, the model on the device and the fp32 restatement's encoder states and logits: made once, never changed"""
    if name not in _CACHE:
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as g:
            d = {k: g[k] for k in g.files if not k.startswith(("w:", "q:"))}
            c, sd = json.loads(str(g["config"])), golden_state_dict(g)
        m = WhisperForConditionalGeneration(**c, eos_token_id=int(d["eos"]))
        m.load_state_dict(sd)
        r32 = WhisperTorch(sd, c, torch.float32)
        x = torch.from_numpy(d["features"])
        _CACHE[name] = (d, c, m.cuda().eval(), r32.encode(x), r32.logits(x, torch.from_numpy(d["ids"])))
    return _CACHE[name]


def check(tag, got, r64, r32):
    r64 = torch.as_tensor(r64).double().cpu()
    e = float((got.double().cpu() - r64).abs().max())
    s = float((torch.as_tensor(r32).double().cpu() - r64).abs().max())
    mag = float(r64.abs().max())
    print(f"{tag}: library {e:.3e}  fp32 restatement {s:.3e}  ratio {e / max(s, 1e-30):.2f}  max|ref| {mag:.2f}")
    assert np.isfinite(e) and e <= max(10 * s, 1e-5 * mag), (tag, e, s, mag)


@pytest.mark.parametrize("name", ["a", "b"])
def test_encoder_and_logits_match_the_golden(name):
    g, c, m, enc32, lg32 = setup(name)
    x = torch.from_numpy(g["features"]).cuda()
    enc = m.encode(x)
    assert tuple(enc.shape) == g["enc"].shape
    check(f"whisper_{name} encoder", enc, g["enc"], enc32)
    lg = m.logits(x, torch.from_numpy(g["ids"]))
    assert tuple(lg.shape) == g["logits"].shape
    check(f"whisper_{name} logits", lg, g["logits"], lg32)


@pytest.mark.parametrize("name", ["a", "b"])
def test_generate_gives_the_golden_tokens(name):
    g, c, m, _, _ = setup(name)
    x = torch.from_numpy(g["features"]).cuda()
    tokens, n = m.generate(x, torch.from_numpy(g["prompt"]), g["tokens"].shape[1])
    assert tokens.dtype == n.dtype == torch.int64
    assert np.array_equal(n.cpu().numpy(), g["lengths"]), (n, g["lengths"])
    assert np.array_equal(tokens.cpu().numpy(), g["tokens"])
    for b, k in enumerate(g["lengths"]):
        assert (tokens[b, int(k):] == int(g["eos"])).all()
    # a shorter budget is the head of the longer one
    t8, n8 = m.generate(x, torch.from_numpy(g["prompt"]), 9)
    assert torch.equal(t8, tokens[:, :9]) and torch.equal(n8, torch.clamp(n, max=9))


@pytest.mark.parametrize("name", ["a", "b"])
def test_item_alone_and_repeated_calls_give_the_same_bits(name):
    g, c, m, _, _ = setup(name)
    x, ids, prompt = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["ids"]), torch.from_numpy(g["prompt"])
    enc, lg = m.encode(x), m.logits(x, ids)
    tokens, n = m.generate(x, prompt, g["tokens"].shape[1])
    for b in range(3):
        assert torch.equal(m.encode(x[b:b + 1])[0], enc[b])
        assert torch.equal(m.logits(x[b:b + 1], ids[b:b + 1])[0], lg[b])
        tb, nb = m.generate(x[b:b + 1], prompt[b:b + 1], g["tokens"].shape[1])
        assert torch.equal(tb[0], tokens[b]) and int(nb) == int(n[b])
    assert torch.equal(m.encode(x), enc) and torch.equal(m.logits(x, ids), lg)
    t2, n2 = m.generate(x, prompt, g["tokens"].shape[1])
    assert torch.equal(t2, tokens) and torch.equal(n2, n)
    # reversed order in the batch: the rows move with their items
    assert torch.equal(m.logits(x.flip(0), ids.flip(0)), lg.flip(0))


@pytest.mark.parametrize("name", ["a", "b"])
def test_suppression_masks_take_effect(name):
    """Suppress the token greedy chose first: the fp64 runner-up stands there, for an item whose runner-up lies 1e-3 of the largest logit
    above the third (the goldens' own condition).  begin_suppress holds at the first generated position only."""
    g, c, m, _, _ = setup(name)
    big = float(np.abs(g["top_val"]).max())
    gap = g["top_val"][:, 0, 1] - g["top_val"][:, 0, 2]
    b = int(gap.argmax())
    assert gap[b] >= 1e-3 * big
    x, prompt = torch.from_numpy(g["features"][b:b + 1]).cuda(), torch.from_numpy(g["prompt"][b:b + 1])
    first, second = int(g["top_idx"][b, 0, 0]), int(g["top_idx"][b, 0, 1])
    never = c["vocab_size"] - 1 if c["vocab_size"] - 1 not in (first, second) else c["vocab_size"] - 2       # an eos nobody chooses here
    plain, _ = m.generate(x, prompt, 3, eos_token_id=never)
    assert int(plain[0, 0]) == first
    for kw in (dict(suppress_tokens=[first]), dict(begin_suppress_tokens=[first])):
        got, _ = m.generate(x, prompt, 3, eos_token_id=never, **kw)
        assert int(got[0, 0]) == second, (kw, got)
    # a begin mask on a token chosen later leaves that later choice alone; the same token in `suppress` removes it
    later = int(plain[0, 1])
    if later not in (first, never):
        got, _ = m.generate(x, prompt, 3, eos_token_id=never, begin_suppress_tokens=[later])
        assert torch.equal(got, plain)
        got, _ = m.generate(x, prompt, 3, eos_token_id=never, suppress_tokens=[later])
        assert int(got[0, 0]) == first and int(got[0, 1]) != later


def test_detect_language():
    g, c, m, _, _ = setup("b")
    x = torch.from_numpy(g["features"]).cuda()
    assert (g["ids"][:, 0] == 1).all()
    lg = g["logits"][:, 0]                                   # fp64: the distribution after the start token 1
    cand = [int(v) for v in np.argsort(-lg[0])[[0, 3, 7, 20, 50]]]
    order = np.sort(lg[:, cand], axis=1)
    assert float((order[:, -1] - order[:, -2]).min()) >= 1e-3 * float(np.abs(g["logits"]).max())
    got = detect_language(m, x, cand, start_id=1)
    assert got.cpu().tolist() == [cand[int(i)] for i in lg[:, cand].argmax(1)]


def test_two_launch_groups_give_equal_rows():
    g, c, m, _, _ = setup("a")
    x = torch.from_numpy(g["features"][1:2]).cuda().expand(17, -1, -1).contiguous()
    tokens, n = m.generate(x, torch.from_numpy(g["prompt"][1]), g["tokens"].shape[1])
    assert (tokens == tokens[:1]).all() and (n == n[0]).all()
    assert np.array_equal(tokens[16].cpu().numpy(), g["tokens"][1]) and int(n[16]) == int(g["lengths"][1])
    lg = m.logits(x, torch.from_numpy(g["ids"][1, :5]))
    assert (lg == lg[:1]).all()


def test_library_refusals():
    g, c, m, _, _ = setup("a")
    x = torch.from_numpy(g["features"]).cuda()
    V, Tm = c["vocab_size"], c["max_target_positions"]
    with pytest.raises(RuntimeError, match="EINVAL.*exactly 2 \\* max_source_positions"):
        m.encode(x[:, :, :-2].contiguous())
    with pytest.raises(RuntimeError, match="EINVAL.*outside the vocabulary"):
        m.logits(x, torch.tensor([[1, V, 2]] * 3))
    with pytest.raises(RuntimeError, match="EINVAL.*outside the vocabulary"):
        m.generate(x, torch.tensor([[1, -1]] * 3), 4)
    with pytest.raises(RuntimeError, match="EINVAL.*max_target_positions"):
        m.generate(x, torch.from_numpy(g["prompt"]), Tm - g["prompt"].shape[1] + 1)
    with pytest.raises(RuntimeError, match="EINVAL.*max_target_positions"):
        m.logits(x, torch.ones(3, Tm + 1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="EINVAL.*eos"):
        m.generate(x, torch.from_numpy(g["prompt"]), 4, eos_token_id=V)
    lib = _lib.load()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    out = torch.empty(3, c["max_source_positions"], c["d_model"], device="cuda")
    rc = lib.us_whisper_encode(m._h, x.data_ptr(), 3, x.shape[2], out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert _lib.ERRORS[rc] == "EWORKSPACE"
    fresh = WhisperForConditionalGeneration(**c)
    h = C.c_void_p()
    fresh._h = h
    fresh._create(lib, torch.device("cuda:0"))
    rc = lib.us_whisper_encode(fresh._h, x.data_ptr(), 3, x.shape[2], out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert _lib.ERRORS[rc] == "EWEIGHTS" and b"has not been loaded" in lib.us_whisper_last_error(fresh._h)
    # the suite goes on from a working model
    assert torch.equal(m.encode(x), m.encode(x))


def test_evaluate_synthetic_whisper_end_to_end():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--synthetic", "6", "--batch", "4", "--recogniser", "whisper"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["files"] == 6 and out["batches"] == 2
    assert abs(out["cer"] - out["expected_cer"]) <= 1e-12, out
