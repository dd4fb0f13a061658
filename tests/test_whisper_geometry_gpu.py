"""The HIP Whisper recogniser at the geometries the goldens a and b do not reach (csrc/whisper.hip, Whisper's encoder schedule in
csrc/hubert.hip): whisper_long (1100 encoder frames, 136 target positions, 4 encoder heads against 1 decoder head, 1 encoder layer against 3
decoder layers, ffn 96 against 132), whisper_wide (d_model 144, decoder ffn 1028, 530 tokens), more than 32 items of whisper_a, a model at
the cap of 2048 positions made here, and what `us_whisper_create` refuses.  DESIGN.md, section 23.3, has the table of
which kernel branch each of them reaches and of which test fails for which planted defect.

Floats follow the project's rule, by `check` of the Whisper GPU tests: the library's max distance from fp64 is at most max(10 x the fp32
restatement's distance on the same input, 1e-5 x max |fp64|); both distances are printed.  Tokens and lengths are compared exactly where a
golden's margin conditions say they may be (1e-3 of the largest |logit| between the choices, |d| >= 1e-2 at a free timestamp decision).
Where no golden can be written, because no seed keeps a beam search over 132 steps that far from a tie, the sequence the library returns is
scored again in fp64 (`replay`): whatever the search chose, a key or value read from a wrong row or position changes that score."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import test_whisper_beam_gpu as BG  # noqa: E402
import test_whisper_decode_gpu as DG  # noqa: E402
import whisper_decode_numpy as rules  # noqa: E402
from make_goldens_whisper import features, seeded_model  # noqa: E402
from test_whisper import create  # noqa: E402
from test_whisper_decode_gpu import check as check_np  # noqa: E402
from test_whisper_gpu import check, setup  # noqa: E402
from whisper_torch import WhisperTorch, golden_state_dict  # noqa: E402

from unitspeech_amd.whisper import WhisperForConditionalGeneration  # noqa: E402

pytestmark = pytest.mark.gpu
_CACHE = {}
NAMES = ["long", "wide"]
LONG_PROMPT_SEED = 0          # planted(): chosen on the CPU so that greedy decoding after it stays 1e-3 from a tie for 8 steps and more


def ref64(name):
    """WhisperTorch(float64)'s encoder states and teacher-forced logits of every item of a golden, with the golden's own numbers wherever it
    stores them (asserted equal to 1e-10 first): whisper_long keeps `enc` at `enc_rows` in a file of its own, whisper_wide keeps the floats
    of its first two items.  Made once, never changed."""
    if ("ref", name) not in _CACHE:
        g, c, _, _, _ = setup(name)
        with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}.npz")) as f:
            r64 = WhisperTorch(golden_state_dict(f), c, torch.float64)
        x = torch.from_numpy(g["features"])
        enc, lg = r64.encode(x), r64.logits(x, torch.from_numpy(g["ids"]))
        if "enc" in g:
            want, rows = torch.from_numpy(g["enc"]), slice(None)
        else:
            with np.load(os.path.join(ROOT, "tests", "golden", f"whisper_{name}_enc.npz")) as f:
                want, rows = torch.from_numpy(f["enc"]), torch.from_numpy(f["enc_rows"])
        k = len(want)
        assert float((enc[:k, rows] - want).abs().max()) <= 1e-10 * float(want.abs().max())
        enc[:k, rows] = want
        k = len(g["logits"])
        assert float((lg[:k] - torch.from_numpy(g["logits"])).abs().max()) <= 1e-10 * float(np.abs(g["logits"]).max())
        lg[:k] = torch.from_numpy(g["logits"])
        _CACHE["ref", name] = (r64, enc, lg)
    return _CACHE["ref", name]


# ---- 1. encoder and teacher-forced logits ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_encoder_and_logits_match_the_golden(name):
    g, c, m, enc32, lg32 = setup(name)
    _, enc64, lg64 = ref64(name)
    x = torch.from_numpy(g["features"]).cuda()
    enc = m.encode(x)
    assert tuple(enc.shape) == tuple(enc64.shape) == (len(x), c["max_source_positions"], c["d_model"])
    check(f"whisper_{name} encoder", enc, enc64, enc32)
    lg = m.logits(x, torch.from_numpy(g["ids"]))
    assert tuple(lg.shape) == tuple(lg64.shape) == (len(x), c["max_target_positions"], c["vocab_size"])
    check(f"whisper_{name} logits", lg, lg64, lg32)
    if name == "long":
        # a lane of the self attention takes keys lane, lane + 64, lane + 128: each trip against the fp32 distance of its own positions
        for lo, hi in ((0, 64), (64, 128), (128, 136)):
            check(f"whisper_long logits, positions {lo} - {hi - 1}", lg[:, lo:hi], lg64[:, lo:hi], lg32[:, lo:hi])


# ---- 2. greedy and timestamp-rule decoding -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", NAMES)
def test_generate_gives_the_golden_tokens(name):
    g, c, m, _, _ = setup(name)
    x = torch.from_numpy(g["features"]).cuda()
    tokens, n = m.generate(x, torch.from_numpy(g["prompt"]), g["tokens"].shape[1])
    assert np.array_equal(n.cpu().numpy(), g["lengths"]), (n, g["lengths"])
    assert np.array_equal(tokens.cpu().numpy(), g["tokens"])
    if name == "long":
        assert g["tokens"].shape[1] == 132 and int(g["lengths"].min()) >= 70           # both items read a cache of more than 64 positions
    for b, k in enumerate(g["lengths"]):
        assert (tokens[b, int(k):] == int(g["eos"])).all()
    # a shorter budget is the head of the longer one
    t8, n8 = m.generate(x, torch.from_numpy(g["prompt"]), 9)
    assert torch.equal(t8, tokens[:, :9]) and torch.equal(n8, torch.clamp(n, max=9))


@pytest.mark.parametrize("name", NAMES)
def test_decode_matches_the_golden(name):
    """`decode` returns the sum of the log-probabilities, not each step's: the sum and the no-speech probability are what is compared"""
    base, d, lay, c, m, r32 = DG.setup(name)
    DG.test_decode_matches_the_golden(name)
    if name == "long":
        assert int(d["max_new"]) == 132 and int(d["lengths"].max()) > 70
    r = DG.decode(m, lay, d, torch.from_numpy(base["features"]).cuda(), torch.from_numpy(base["prompt"]), beam_size=1)
    assert np.array_equal(r.tokens.cpu().numpy(), d["tokens"]) and np.array_equal(r.lengths.cpu().numpy(), d["lengths"])


# ---- 3. beam search on wide ----------------------------------------------------------------------------------------------------------------


def test_beam_matches_the_golden_wide():
    BG.test_beam_matches_the_golden("wide")


# ---- 4. beam search on long, by replay -------------------------------------------------------------------------------------------------------


def planted(B, P, sot, lay, V, seed):
    """a previous-text prompt: seeded text ids in front of the start token 1 at `sot`, three more ids behind it"""
    g = np.random.Generator(np.random.Philox(key=5200 + seed))
    ids = g.integers(3, lay["no_timestamps"] - 1, (B, P))
    ids[ids == lay["eos"]] = 3
    ids[:, sot] = 1
    assert ids.min() >= 0 and ids.max() < V
    return torch.from_numpy(ids)


def replay(t, enc, prompt, tokens, length, max_new, lay, sot):
    """One item's sequence scored again by the restatement `t`: teacher-forced on prompt + tokens, and per step the log-softmax, over what the
    masks and the timestamp rules of tools/whisper_decode_numpy.py leave, at the token of the sequence (the eos that ended it included)
    -> dict(sum, finite: every token was one the rules leave finite, nsp, steps: select()'s dicts (the restatement's own choice), big)"""
    np_dtype = {torch.float64: np.float64, torch.float32: np.float32}[t.dtype]
    V, P = t.c["vocab_size"], prompt.shape[0]
    sup, beg = rules.masks(lay, V)
    tb = lay["no_timestamps"] + 1
    state = t.start(enc[None])
    nsp = None
    for p in range(P - 1):
        lg = t.step(state, prompt[p:p + 1], p, logits=p == sot)
        if lg is not None:
            nsp = rules.no_speech_prob(lg[0].numpy(), lay["no_speech"], np_dtype)
    seq = [int(v) for v in tokens[:length]] + ([lay["eos"]] if length < max_new else [])
    cur, sampled, total, finite, steps, big = prompt[P - 1:], [], 0.0, True, [], 0.0
    for i, tok in enumerate(seq):
        row = t.step(state, cur, P - 1 + i)[0].numpy()
        if i == 0 and sot == P - 1:
            nsp = rules.no_speech_prob(row, lay["no_speech"], np_dtype)
        r = rules.select(row, sampled, lay, sup, beg, np_dtype)
        ok = rules.allowed(V, sampled, lay, sup, beg)
        if r["decided"]:
            ok[:tb] = False
        y = row.astype(np_dtype)
        finite = finite and bool(ok[tok]) and bool(np.isfinite(y[tok]))
        total += float(y[tok] - rules._lse(y[ok], np_dtype)) if ok[tok] else float("-inf")
        big = max(big, float(np.abs(row).max()))
        steps.append(r)
        sampled.append(tok)
        cur = torch.tensor([tok])
    return dict(sum=total, finite=finite, nsp=nsp, steps=steps, big=big)


def long_setup():
    """the decode golden's model and layout, and the two restatements with their encoder states of the golden's two items"""
    if "long" not in _CACHE:
        base, d, lay, c, m, _ = DG.setup("long")
        with np.load(os.path.join(ROOT, "tests", "golden", "whisper_long.npz")) as f:
            sd = golden_state_dict(f)
        x = torch.from_numpy(base["features"])
        ts = [WhisperTorch(sd, c, dt) for dt in (torch.float64, torch.float32)]
        _CACHE["long"] = (base, lay, c, m, x, [(t, t.encode(x)) for t in ts])
    return _CACHE["long"]


def decode_long(m, lay, x, prompt, max_new, sot, **kw):
    cap = lay["max_initial_timestamp_index"]
    return m.decode(x, prompt, no_timestamps_id=lay["no_timestamps"], max_initial_timestamp=None if cap < 0 else 0.02 * cap, no_speech_id=lay["no_speech"],
                    max_new_tokens=max_new, sot_index=sot, **kw)


def replay_both(r, prompt, max_new, lay, sot, ts):
    """the library's result `r` of a batch scored by the fp64 and the fp32 restatement -> (the fp64 replays, the fp32 replays, sums64, sums32)"""
    out = []
    for t, enc in ts:
        out.append([replay(t, enc[b], prompt[b], r.tokens[b].cpu().numpy(), int(r.lengths[b]), max_new, lay, sot) for b in range(len(prompt))])
    assert all(k["finite"] for k in out[0]), "a token the rules mask at its step"
    return out[0], out[1], np.asarray([k["sum"] for k in out[0]]), np.asarray([k["sum"] for k in out[1]])


def test_beam_on_long_scores_what_it_returns():
    """n = 3 and 5; the golden's prompt of 4 with max_new 132, and a previous-text prompt of 100 (start token at 96) with max_new 32.  The
    tokens are the library's own; their score in fp64 must be the sum_logprob it returns.  A key or value read through a wrong ancestry row
    at any position moves that score by far more than the bar."""
    base, lay, c, m, x, ts = long_setup()
    xd = x.cuda()
    differs, n_long = 0, 0
    for tag, prompt, max_new, sot in (("P=4", torch.from_numpy(base["prompt"]), 132, 0),
                                      ("P=100", planted(len(x), 100, 96, lay, c["vocab_size"], LONG_PROMPT_SEED), 32, 96)):
        greedy = decode_long(m, lay, xd, prompt, max_new, sot)
        for n in (3, 5):
            r = decode_long(m, lay, xd, prompt, max_new, sot, beam_size=n)
            assert tuple(r.tokens.shape) == (len(x), max_new) and int(r.lengths.max()) <= max_new
            assert torch.equal(r.no_speech_prob, greedy.no_speech_prob)
            _, _, s64, s32 = replay_both(r, prompt, max_new, lay, sot, ts)
            print(f"whisper_long beam n={n} {tag}: lengths {r.lengths.cpu().tolist()} (greedy {greedy.lengths.cpu().tolist()})")
            check_np(f"whisper_long beam n={n} {tag} sum_logprob", r.sum_logprob.double().cpu().numpy(), s64, s32)
            differs += int(not torch.equal(r.tokens, greedy.tokens))
            if tag == "P=4":
                assert int(r.lengths.max()) > 64, r.lengths
                n_long += 1
    assert differs >= 1 and n_long == 2


def test_greedy_decode_after_a_long_prompt():
    """A prompt of 100 tokens with the start token at 96 (previous text): the no-speech probability is read at position 96 and the first
    generated token attends to 100 cached positions.  sum_logprob and no_speech_prob by replay; the tokens against fp64's own choice up to
    the first step whose fp64 margin falls below 1e-3 of the largest |logit| (or whose free timestamp decision has |d| < 1e-2)."""
    base, lay, c, m, x, ts = long_setup()
    P, sot, max_new = 100, 96, 32
    prompt = planted(len(x), P, sot, lay, c["vocab_size"], LONG_PROMPT_SEED)
    r = decode_long(m, lay, x.cuda(), prompt, max_new, sot)
    r64, r32, s64, s32 = replay_both(r, prompt, max_new, lay, sot, ts)
    check_np("whisper_long greedy P=100 sum_logprob", r.sum_logprob.double().cpu().numpy(), s64, s32)
    check_np("whisper_long greedy P=100 no_speech_prob", r.no_speech_prob.double().cpu().numpy(), np.asarray([k["nsp"] for k in r64]),
             np.asarray([k["nsp"] for k in r32]))
    for b, k in enumerate(r64):
        safe = 0
        for s in k["steps"]:
            if s["gap"] < 1e-3 * k["big"] or (s["free"] and abs(s["d"]) < 1e-2):
                break
            safe += 1
        print(f"whisper_long greedy P=100 item {b}: {safe} of {len(k['steps'])} steps keep their margin")
        assert safe >= 8
        assert r.tokens[b, :safe].cpu().tolist() == [s["token"] for s in k["steps"][:safe]]


# ---- 5. the same bits alone, in a batch, repeated, reversed ------------------------------------------------------------------------------------


@pytest.mark.parametrize("what", ["logits", "generate", "decode", "beam3", "beam5"])
@pytest.mark.parametrize("name", NAMES)
def test_item_alone_in_a_batch_among_17_and_repeated(name, what):
    base, d, lay, c, m, _ = DG.setup(name)
    g = setup(name)[0]
    x, prompt, ids = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["prompt"]), torch.from_numpy(g["ids"])
    B = len(x)
    if what == "logits":
        run = lambda i: [m.encode(x[i]), m.logits(x[i], ids[i])]
    elif what == "generate":
        run = lambda i: list(m.generate(x[i], prompt[i], g["tokens"].shape[1], eos_token_id=int(g["eos"]), suppress_tokens=[], begin_suppress_tokens=[]))
    else:
        kw = {} if what == "decode" else dict(beam_size=int(what[4:]))

        def run(i):
            r = DG.decode(m, lay, d, x[i], prompt[i], **kw)
            return [r.tokens, r.lengths, r.sum_logprob, r.no_speech_prob]
    every = list(range(B))
    whole = run(every)
    assert all(torch.equal(a, b) for a, b in zip(run(every), whole))
    flipped = run(every[::-1])
    assert all(torch.equal(a.flip(0), b) for a, b in zip(flipped, whole))
    idx = [(i + 1) % B for i in range(17)]               # both launch groups of 16; a beam's groups of 16 // n items, the last one short
    many = run(idx)
    assert all(torch.equal(a, b[idx]) for a, b in zip(many, whole))
    for b in every:
        assert all(torch.equal(a[0], w[b]) for a, w in zip(run([b]), whole)), b


# ---- 6. more than 32 items: the second launch group of the encoder schedule --------------------------------------------------------------------


def test_33_items_keep_the_bits_of_the_item_alone():
    g, c, m, enc32, lg32 = setup("a")
    base, d, lay, _, md, _ = DG.setup("a")
    idx = [(i + 1) % 3 for i in range(33)]               # item 31 is stored item 2, item 32 (the second group's only one) stored item 0
    x3, ids3, prompt3 = torch.from_numpy(g["features"]).cuda(), torch.from_numpy(g["ids"][:, :6]), torch.from_numpy(g["prompt"])
    x, ids, prompt = x3[idx].contiguous(), ids3[idx].contiguous(), prompt3[idx].contiguous()
    enc, lg = m.encode(x), m.logits(x, ids)
    tokens, n = m.generate(x, prompt, g["tokens"].shape[1])
    r = DG.decode(md, lay, d, x, prompt, beam_size=3)
    one = {}
    for b in range(3):
        k = DG.decode(md, lay, d, x3[b:b + 1], prompt3[b:b + 1], beam_size=3)
        t1, n1 = m.generate(x3[b:b + 1], prompt3[b:b + 1], g["tokens"].shape[1])
        one[b] = [m.encode(x3[b:b + 1])[0], m.logits(x3[b:b + 1], ids3[b:b + 1])[0], t1[0], n1[0], k.tokens[0], k.lengths[0], k.sum_logprob[0],
                  k.no_speech_prob[0]]
    for j, b in enumerate(idx):
        got = [enc[j], lg[j], tokens[j], n[j], r.tokens[j], r.lengths[j], r.sum_logprob[j], r.no_speech_prob[j]]
        assert all(torch.equal(a, w) for a, w in zip(got, one[b])), (j, b)
    assert np.array_equal(tokens[32].cpu().numpy(), g["tokens"][idx[32]]) and int(n[32]) == int(g["lengths"][idx[32]])
    check("whisper_a item 32 of 33, encoder", enc[32], g["enc"][idx[32]], enc32[idx[32]])
    check("whisper_a item 32 of 33, logits", lg[32], g["logits"][idx[32], :6], lg32[idx[32], :6])


# ---- 7. the cap of 2048 positions, 8. what creation refuses ------------------------------------------------------------------------------------


def runtime_model(seed, feature_seed, **c):
    """a model of the golden tool's weight law made here, on the device, with one item of the tool's features and the two restatements"""
    _, sd = seeded_model(c, seed)
    m = WhisperForConditionalGeneration(**c)
    m.load_state_dict(sd)
    return m.cuda().eval(), features(c, feature_seed, 1), WhisperTorch(sd, c, torch.float64), WhisperTorch(sd, c, torch.float32)


def test_the_cap_of_2048_positions():
    c = dict(d_model=16, encoder_attention_heads=1, decoder_attention_heads=1, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=16, decoder_ffn_dim=16,
             num_mel_bins=4, max_source_positions=2048, max_target_positions=2048, vocab_size=32)
    m, x, r64, r32 = runtime_model(700, 701, **c)
    ids = torch.from_numpy(np.random.Generator(np.random.Philox(key=702)).integers(0, 32, (1, 2048)))
    check("whisper cap encoder", m.encode(x.cuda()), r64.encode(x), r32.encode(x))
    lg, lg64, lg32 = m.logits(x.cuda(), ids), r64.logits(x, ids), r32.logits(x, ids)
    assert tuple(lg.shape) == (1, 2048, 32)
    check("whisper cap logits", lg, lg64, lg32)
    for lo in range(0, 2048, 512):
        check(f"whisper cap logits, positions {lo} - {lo + 511}", lg[:, lo:lo + 512], lg64[:, lo:lo + 512], lg32[:, lo:lo + 512])
    for field in ("max_source_positions", "max_target_positions"):
        lib, h, rc = create(**{field: 2049})
        assert rc == -1 and not h and b"max_source_positions and max_target_positions must lie in [1, 2048]" in lib.us_last_error(None)
        lib, h, rc = create(**{field: 2048})
        assert rc == 0 and h and lib.us_whisper_destroy(h) == 0


@pytest.mark.parametrize("over, text", [
    (dict(d_model=136, encoder_heads=2, decoder_heads=2), b"head dimension must be a multiple of 4, at most 64 (got 68)"),
    (dict(d_model=60, encoder_heads=10, decoder_heads=10), b"head dimension must be a multiple of 4, at most 64 (got 6)"),
    (dict(decoder_ffn=130), b"the decoder's a multiple of 4"),
    (dict(decoder_heads=3), b"d_model must be divisible by the number of heads"),
    (dict(encoder_heads=3), b"d_model must be divisible by the number of heads"),
])
def test_create_refuses(over, text):
    lib, h, rc = create(**over)
    assert rc == -1 and not h and text in lib.us_last_error(None)


def test_an_encoder_ffn_that_is_no_multiple_of_4():
    """The encoder's GEMMs run on packed operands: K is padded to 16 rows and the outputs to 64 columns with zeros, so encoder_ffn_dim = 202
    is built (the decoder's fc2 reads its K in float4s and so refuses 130 above)."""
    c = dict(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=1, encoder_ffn_dim=202, decoder_ffn_dim=64,
             num_mel_bins=8, max_source_positions=70, max_target_positions=8, vocab_size=40)
    m, x, r64, r32 = runtime_model(710, 711, **c)
    check("whisper encoder_ffn_dim 202 encoder", m.encode(x.cuda()), r64.encode(x), r32.encode(x))
    ids = torch.tensor([[1, 5, 9, 13, 2, 30, 39, 0]])
    check("whisper encoder_ffn_dim 202 logits", m.logits(x.cuda(), ids), r64.logits(x, ids), r32.logits(x, ids))
