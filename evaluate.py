#!/usr/bin/env python3
"""Scoring synthesised speech on the HIP library: the counterpart of the reference's evaluation/ (transcribe every sample, compare with
its text by character and word error rate, compare its speaker embedding with the reference recording's).

    python evaluate.py --filelist LIST --ctc_path CTC.pt --vocab_path vocab.json [--config_path config.json]
                       [--speaker_encoder_path EMBEDDER.pt] [--batch 16] [--timestamps] [--out RESULT.json]
    python evaluate.py --synthetic 12 --batch 4
    python evaluate.py --filelist LIST --recogniser whisper --whisper_checkpoint DIR [--language ro]
    python evaluate.py --synthetic 6 --batch 4 --recogniser whisper [--whisper_timestamps [--whisper_beam_size 5 [--whisper_patience 1.0]]]
    python evaluate.py --filelist LIST ... --mos_path MOS.ckpt [--mos_upstream WAV2VEC2.pt] [--mos_clipping 0|1]
    python evaluate.py --synthetic 12 --batch 4 --mos

LIST holds one `wav|transcript[|reference_wav]` line per sample.  CTC.pt is a `torch.save`d state dict of `transformers.HubertForCTC` or
`Wav2Vec2ForCTC` in the base form (the class is taken from the keys; nothing is fetched by name; the base size unless --config_path
names the model's config.json) and vocab.json its tokenizer's vocabulary.  The wavs are read with `unitspeech_amd.audio.read_wav`,
resampled to 16 kHz by the library's `Resample`, sorted by length and transcribed in ragged batches of --batch (`transcribe_ids`: encoder, CTC head, greedy collapse; an item has the ids it has alone).  The
transcripts are brought to the vocabulary by `normalize_text`; CER and WER are `unitspeech_amd.asr.error_rates` (corpus rates: sum of
distances over sum of reference lengths).  With --speaker_encoder_path and the third column, SECS is the cosine similarity of
`ECAPA_TDNN.embed_wav` between each wav and its reference.  One line per file, then the corpus line; --out writes all of it as JSON.
--timestamps adds `word_times` to each file's record: the reference text's words with start and end in seconds (20 ms frames), from the forced
alignment of the text to the recogniser's log-probabilities (`align`); null for a text that is empty or longer than its audio allows.
--sv56 [--ndb N] first brings every loaded sample to N dB active speech level (ITU-T P.56, default -26) on the device, in length-sorted
ragged batches at the file's own rate and by the reference's int16 route (`unitspeech_amd.level.normalize_level(..., via_int16=True,
out_int16=True)`), before the recogniser and the speaker encoder see it: the reference notebook's "with sv56" row.  The reference
recordings of the third column are left as they are.

--recogniser whisper transcribes with `unitspeech_amd.whisper.WhisperForConditionalGeneration` instead, as the reference's notebook does
(`whisper.load_model("medium")`, `pad_or_trim`, `log_mel_spectrogram`, `decode`).  The notebook's `DecodingOptions()` are greedy decoding
under the timestamp rules (`without_timestamps=False`): that is --whisper_timestamps; without the flag the decoding is plain greedy with
<|notimestamps|> in the prompt, which can give another transcript.  DIR holds
`config.json`, the weights (`pytorch_model.bin`, or `model.safetensors` where that package imports), `vocab.json` and `added_tokens.json`
(and `generation_config.json` for the suppression lists).  The prompt is <|startoftranscript|>, the language, <|transcribe|>,
<|notimestamps|>; without --language the language is detected per file.  With --whisper_timestamps the prompt ends at <|transcribe|>, every
step applies the timestamp rules (`WhisperForConditionalGeneration.decode`), and each file's record gains `avg_logprob`, `no_speech_prob`
(where the vocabulary has <|nospeech|> or <|nocaptions|>) and `segments` ([start_s, end_s, text] from the timestamp pairs).  The same length-sorted batches feed it; hypotheses and references are
brought to lower-case letters, digits, apostrophes and single spaces before scoring.  Files longer than 30 s are refused.
--whisper_beam_size N (with --whisper_timestamps) decodes by beam search under the same rules, `DecodingOptions(beam_size=N, patience=P)` with
--whisper_patience P (default 1.0): what the `whisper` command line runs with N = 5.  `avg_logprob` is then the winning sequence's; the values
used go into the result as `whisper_beam_size` and `whisper_patience`.

--mos_path adds the reference notebook's third figure, a predicted mean opinion score (`s3prl.hub.mos_wav2vec2()` applied to every file
at 16 kHz): MOS.ckpt is s3prl's checkpoint (Featurizer, Downstream and their arguments), --mos_upstream the wav2vec2-base weights (a
`transformers.Wav2Vec2Model` state dict or fairseq's `wav2vec_small.pt`); --mos_clipping says whether the score is 2 tanh(score) + 3 when the
checkpoint does not.  Every file's 16 kHz waveform goes through `unitspeech_amd.mos.MOSPredictor` in the same length-sorted ragged batches as
the recogniser (after --sv56 when that is given: the notebook's two rows differ in exactly that; --normalize does not touch it): each
file's record gains `mos`, the corpus line `mos` (the mean), `mos_min` and `mos_max`.  With --synthetic N --mos and no path a seeded tiny
predictor (the TINY geometry, a connector of 16) runs.

--synthetic N runs without files: a seeded tiny CTC model, N seeded waveforms, and as transcripts the model's own decodings with a known
number of edits applied (characters appended, or cut from the end): the distance of each pair is then exactly that number, so the CER
printed must equal the `expected_cer` printed next to it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from unitspeech_amd.audio import read_wav, to_16k  # noqa: E402
from unitspeech_amd.batching import pad_batch, plan_batches  # noqa: E402

MIN_SAMPLES_16K = 400            # the receptive field of the feature extractor: one frame
SYNTHETIC_RATE = 22050
SYNTHETIC_EDITS = 2              # per utterance
TINY = dict(conv_dim=[24] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=40, num_attention_heads=2,
            intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layer_norm_eps=1e-5)
TINY_VOCAB = {"<pad>": 0, "|": 1, **{c: i + 2 for i, c in enumerate("abcdefghij")}}


def parse_filelist(text: str):
    """`wav|transcript[|reference_wav]` lines -> [(wav, transcript, reference_wav or None)]; blank lines are skipped."""
    out = []
    for no, line in enumerate(text.splitlines(), start=1):
        line = line.strip()
        if not line:
            continue
        parts = line.split("|")
        if len(parts) not in (2, 3) or not parts[0]:
            raise ValueError(f"file list line {no}: expected `wav|transcript[|reference_wav]`, got {line!r}")
        out.append((parts[0], parts[1], parts[2] if len(parts) == 3 and parts[2] else None))
    return out


def apply_edits(text: str, edits: int, cut: bool, letter: str = "a"):
    """A string at Levenshtein distance exactly `edits` from `text`: `edits` characters cut from its end (when asked, and when that leaves
    a longer, tidy string) or `edits` letters appended: the lengths then differ by `edits`, which no alignment can beat."""
    if cut and len(text) > 2 * edits and not text[:-edits].endswith(" "):
        return text[:-edits]
    return text + letter * edits


@torch.no_grad()
def normalize_items(items, ndb, max_batch, device):
    """[(name, waveform, rate)] -> the same with every waveform brought to `ndb` dB active speech level as the int16 file the reference's
    sv56 step leaves would read back (s / 32768, fp32, on the device), and per item (level_db, gain, clipped)."""
    from unitspeech_amd.level import normalize_level
    out, levels = list(items), [None] * len(items)
    for rate in sorted({r for _, _, r in items}):
        group = [i for i, it in enumerate(items) if it[2] == rate]
        for batch in plan_batches([len(items[i][1]) for i in group], max_batch):
            idx = [group[j] for j in batch]
            x, n = pad_batch([torch.as_tensor(items[i][1]).float().to(device) for i in idx])
            y, lv = normalize_level(x, rate, ndb, lengths=n, via_int16=True, out_int16=True)
            y = y.to(torch.float32) / 32768.0
            for b, (i, level, gain, clipped) in enumerate(zip(idx, lv.level_db.tolist(), lv.gain.tolist(), lv.clipped.tolist())):
                out[i] = (items[i][0], y[b, :n[b]].clone(), rate)
                levels[i] = (level, gain, clipped)
    return out, levels


def padded_batch(wavs16, idx):
    """`pad_batch` of the items of `wavs16` that `idx` names."""
    return pad_batch([wavs16[i] for i in idx])


@torch.no_grad()
def transcribe_all(model, vocabulary, wavs16, max_batch, scores=None, beam=None):
    """16 kHz waveforms [T_i] on the device -> their transcripts, in the order given; one read back per batch, of the tokens.
    scores: a list that makes Whisper decode under the timestamp rules and receives per file dict(avg_logprob, no_speech_prob, segments);
    beam: dict(beam_size, patience) for beam search under those rules."""
    texts = [None] * len(wavs16)
    batches = plan_batches([int(w.shape[0]) for w in wavs16], max_batch)
    if scores is not None:
        scores[:] = [None] * len(wavs16)
    for idx in batches:
        x, n = padded_batch(wavs16, idx)
        if scores is None:
            tokens, count = model.transcribe_ids(x, n)
            tokens, count = tokens.cpu(), count.cpu()
        else:
            r = model.transcribe_ids(x, n, timestamps=True, **(beam or {}))
            tokens, count, avg = r.tokens.cpu(), r.lengths.cpu(), r.avg_logprob.cpu().tolist()
            ns = r.no_speech_prob.cpu().tolist() if r.no_speech_prob is not None else [None] * len(idx)
            for b, i in enumerate(idx):
                scores[i] = dict(avg_logprob=avg[b], no_speech_prob=ns[b],
                                 segments=[list(sg) for sg in vocabulary.segments(tokens[b, :int(count[b])])])
        for i, t in zip(idx, vocabulary.decode(tokens, count)):
            texts[i] = t
    return texts, batches


@torch.no_grad()
def similarities(embedder, wavs16, refs16, max_batch):
    """Cosine similarity of `embed_wav` (unit norm) between wavs16[i] and refs16[i] (None: no reference) -> list of float or None."""
    pairs = [i for i, r in enumerate(refs16) if r is not None]
    emb = {}
    for which, src in (("wav", wavs16), ("ref", refs16)):
        for idx in plan_batches([int(src[i].shape[0]) for i in pairs], max_batch):
            idx = [pairs[j] for j in idx]
            x, n = padded_batch(src, idx)
            e = embedder.embed_wav(x, n).cpu()
            for b, i in enumerate(idx):
                emb[which, i] = e[b]
    return [float((emb["wav", i] * emb["ref", i]).sum()) if r is not None else None for i, r in enumerate(refs16)]


FRAME_SECONDS = 0.02             # one encoder frame: 320 samples at 16 kHz


def word_spans(text: str):
    """[(word, first character index, one past its last)] of a normalised transcript, whose characters are its tokens one for one."""
    spans, i = [], 0
    for w in text.split(" "):
        if w:
            spans.append((w, i, i + len(w)))
        i += len(w) + 1
    return spans


@torch.no_grad()
def word_timestamps(model, vocabulary, wavs16, transcripts, batches):
    """Per file the reference transcript's words with start and end in seconds, from the forced alignment of the transcript to the
    head's log-probabilities (`align`); None for a file whose transcript is empty or does not fit its frames."""
    out = [None] * len(wavs16)
    for idx in batches:
        x, n = padded_batch(wavs16, idx)
        ids = [vocabulary.encode(transcripts[i]) for i in idx]
        tg = torch.zeros(len(idx), max(1, max(len(t) for t in ids)), dtype=torch.int64)
        for b, t in enumerate(ids):
            tg[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
            tg[b, len(t):] = (vocabulary.blank_id + 1) % len(vocabulary)
        _, score, start, frames = model.align(x, n, tg.to(x.device), torch.tensor([len(t) for t in ids], dtype=torch.int64).to(x.device))
        score, start, frames = score.cpu(), start.cpu(), frames.cpu()
        for b, i in enumerate(idx):
            if not ids[b] or not np.isfinite(float(score[b])):
                continue
            out[i] = [{"word": w, "start": round(float(start[b, a]) * FRAME_SECONDS, 2),
                       "end": round(float(start[b, e - 1] + frames[b, e - 1]) * FRAME_SECONDS, 2)} for w, a, e in word_spans(transcripts[i])]
    return out


def synthetic_model(device, seed: int = 0):
    """A seeded tiny `HubertForCTC` over TINY_VOCAB (the head drawn with unit scale, so that the ids vary) and its vocabulary."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hubert_torch import synthetic_hubert_state_dict
    from unitspeech_amd.asr import CTCVocabulary, HubertForCTC
    V = len(TINY_VOCAB)
    model = HubertForCTC(vocab_size=V, pad_token_id=0, **TINY)
    sd = {"hubert." + k: v for k, v in synthetic_hubert_state_dict(TINY, seed).items()}
    g = np.random.Generator(np.random.Philox(key=9000 + seed))
    sd["lm_head.weight"] = torch.from_numpy(g.standard_normal((V, TINY["hidden_size"]), dtype=np.float32))
    sd["lm_head.bias"] = torch.from_numpy(0.1 * g.standard_normal(V, dtype=np.float32))
    model.load_state_dict(sd)
    return model.to(device).eval(), CTCVocabulary(TINY_VOCAB)


MOS_PROJECTOR = 16               # --synthetic N --mos: the tiny head's connector


def synthetic_mos(device, seed: int = 0):
    """A seeded tiny `MOSPredictor`: the TINY upstream (wav2vec2's base form is HuBERT's) and a head with a connector of MOS_PROJECTOR."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hubert_torch import synthetic_hubert_state_dict
    from mos_torch import synthetic_mos_weights
    from unitspeech_amd.hubert import HubertModel
    from unitspeech_amd.mos import MOSHead, MOSPredictor
    upstream = HubertModel(**TINY)
    upstream.load_state_dict(synthetic_hubert_state_dict(TINY, seed))
    head = MOSHead(TINY["hidden_size"], TINY["num_hidden_layers"] + 1, MOS_PROJECTOR)
    head.load_state_dict(synthetic_mos_weights(head.n_states, head.hidden_size, MOS_PROJECTOR, seed))
    return MOSPredictor(upstream, head).to(device).eval()


@torch.no_grad()
def mos_all(predictor, wavs16, max_batch):
    """16 kHz waveforms [T_i] on the device -> their predicted scores as floats, in the order given; one read back per batch."""
    out = [None] * len(wavs16)
    for idx in plan_batches([int(w.shape[0]) for w in wavs16], max_batch):
        x, n = padded_batch(wavs16, idx)
        for i, v in zip(idx, predictor(x, n).cpu().tolist()):
            out[i] = v
    return out


TINY_WHISPER = dict(d_model=64, encoder_attention_heads=2, decoder_attention_heads=2, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=128,
                    decoder_ffn_dim=128, num_mel_bins=80, max_source_positions=1500, max_target_positions=32, vocab_size=36)


SYNTHETIC_TIMESTAMPS = 8         # --whisper_timestamps: <|0.00|> ... <|0.14|> behind <|notimestamps|>


def synthetic_whisper(device, seed: int = 0, timestamps: bool = False):
    """A seeded tiny Whisper over the letters, the space and the special tokens, and its vocabulary.  timestamps: a vocabulary (and an
    embedding) longer by <|nospeech|> in front of <|notimestamps|> and SYNTHETIC_TIMESTAMPS timestamp tokens behind it."""
    from unitspeech_amd.whisper import WhisperForConditionalGeneration, WhisperVocabulary, synthetic_whisper_state_dict
    vocab = {**{c: i for i, c in enumerate("abcdefghijklmnopqrstuvwxyz")}, "\u0120": 26}          # GPT-2's spelling of the space
    special = ("<|endoftext|>", "<|startoftranscript|>", "<|ro|>", "<|en|>", "<|transcribe|>", "<|notimestamps|>")
    config = dict(TINY_WHISPER)
    if timestamps:
        special = special[:-1] + ("<|nospeech|>", "<|notimestamps|>") + tuple(f"<|{0.02 * i:.2f}|>" for i in range(SYNTHETIC_TIMESTAMPS))
        config["vocab_size"] = 27 + len(special)
    added = {t: 27 + i for i, t in enumerate(special)}
    vocabulary = WhisperVocabulary(vocab, added)
    suppress = [i for t, i in sorted(added.items(), key=lambda kv: kv[1])[1:] if not t[2:-2].replace(".", "").isdigit()]
    model = WhisperForConditionalGeneration(**config, eos_token_id=vocabulary.end_id, suppress_tokens=suppress)
    model.load_state_dict(synthetic_whisper_state_dict(config, seed))
    return model.to(device).eval(), vocabulary


def whisper_prompt(model, vocabulary, language):
    """Transcribe, <|notimestamps|> last (`transcribe_ids(timestamps=True)`, the notebook's default options, leaves it out); the language
    given, or detected among the vocabulary's."""
    model.prompt_ids = [vocabulary.start_id, vocabulary.language_id(language) if language else None, vocabulary.transcribe_id,
                        vocabulary.notimestamps_id]
    model.language_ids = vocabulary.language_ids()
    model.no_timestamps_id = vocabulary.notimestamps_id
    try:
        model.no_speech_id = vocabulary.nospeech_id
    except KeyError:
        model.no_speech_id = None
    if model.eos_token_id is None:
        model.eos_token_id = vocabulary.end_id


def synthetic_waves(n: int, seed: int = 0):
    from unitspeech_amd.mel import synthetic_waveform
    if n < 1:
        raise ValueError("--synthetic N: N must be at least 1")
    g = np.random.Generator(np.random.Philox(key=7000 + seed))
    lens = g.integers(int(0.4 * SYNTHETIC_RATE), int(1.6 * SYNTHETIC_RATE), size=n)
    return [(f"synthetic_{i:04d}", synthetic_waveform(int(lens[i]), seed * 1000 + i, SYNTHETIC_RATE), SYNTHETIC_RATE) for i in range(n)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--filelist", default=None, help="`wav|transcript[|reference_wav]` lines")
    ap.add_argument("--ctc_path", default=None, help="state dict of a HubertForCTC / Wav2Vec2ForCTC (base form)")
    ap.add_argument("--vocab_path", default=None, help="the tokenizer's vocab.json")
    ap.add_argument("--config_path", default=None, help="the model's config.json, when it is not the base size")
    ap.add_argument("--recogniser", choices=("ctc", "whisper"), default="ctc")
    ap.add_argument("--whisper_checkpoint", default=None, help="--recogniser whisper: directory with config.json, weights, vocab.json, added_tokens.json")
    ap.add_argument("--language", default=None, help="--recogniser whisper: the language token's name (ro); detected per file when absent")
    ap.add_argument("--whisper_timestamps", action="store_true",
                    help="--recogniser whisper: decode under the timestamp rules (whisper.decode's defaults); adds avg_logprob, no_speech_prob, segments")
    ap.add_argument("--whisper_beam_size", type=int, default=None, metavar="N",
                    help="--whisper_timestamps: beam search with N beams (whisper.decode's DecodingOptions(beam_size=N)), N in [1, 16]")
    ap.add_argument("--whisper_patience", type=float, default=None, metavar="P",
                    help="--whisper_beam_size: the search ends after round(N * P) finished candidates (default 1.0)")
    ap.add_argument("--blank", default="<pad>")
    ap.add_argument("--word_delimiter", default="|")
    ap.add_argument("--normalize", action="store_true", help="zero mean, unit variance per waveform (a feature extractor with do_normalize)")
    ap.add_argument("--speaker_encoder_path", default=None, help="the whole speaker embedder's checkpoint: adds SECS against the third column")
    ap.add_argument("--batch", type=int, default=16, help="most files in one call")
    ap.add_argument("--out", default=None, help="JSON file for the result")
    ap.add_argument("--timestamps", action="store_true", help="per-word start and end times of the reference text (forced alignment)")
    ap.add_argument("--sv56", action="store_true", help="normalise every sample's active speech level before it is scored")
    ap.add_argument("--ndb", type=float, default=-26.0, help="--sv56: the target level in dB relative to full scale")
    ap.add_argument("--mos_path", default=None, help="s3prl's mos_wav2vec2 checkpoint: adds a predicted mean opinion score per file")
    ap.add_argument("--mos_upstream", default=None, help="--mos_path: the wav2vec2-base weights (transformers state dict or fairseq's wav2vec_small.pt)")
    ap.add_argument("--mos_clipping", type=int, choices=(0, 1), default=None, help="--mos_path: 2 tanh(score) + 3, when the checkpoint does not say")
    ap.add_argument("--mos", action="store_true", help="--synthetic N: a seeded tiny MOS predictor when no --mos_path is given")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded waveforms through a seeded tiny model")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.whisper_timestamps and args.recogniser != "whisper":
        raise SystemExit("--whisper_timestamps belongs to --recogniser whisper")
    if args.whisper_beam_size is not None and not (args.recogniser == "whisper" and args.whisper_timestamps):
        raise SystemExit("--whisper_beam_size needs --recogniser whisper --whisper_timestamps: beam search is built under the timestamp rules only")
    if args.whisper_patience is not None and args.whisper_beam_size is None:
        raise SystemExit("--whisper_patience belongs to --whisper_beam_size")
    if args.whisper_beam_size is not None and not 1 <= args.whisper_beam_size <= 16:
        raise SystemExit("--whisper_beam_size must lie in [1, 16]")
    if args.mos and not args.mos_path and not args.synthetic:
        raise SystemExit("--mos without --mos_path belongs to --synthetic N: give --mos_path CKPT")
    if (args.mos_upstream or args.mos_clipping is not None) and not args.mos_path:
        raise SystemExit("--mos_upstream and --mos_clipping belong to --mos_path")
    if not torch.cuda.is_available():
        raise SystemExit("no ROCm device: the HIP recogniser has no CPU fallback")
    from unitspeech_amd.asr import CTCVocabulary, error_rates, load_ctc_checkpoint, normalize_text
    device = torch.device(args.device)
    resamplers, embedder = {}, None
    whisper = args.recogniser == "whisper"
    if whisper and (args.timestamps or args.normalize):
        raise SystemExit("--timestamps and --normalize belong to the CTC recogniser")
    if args.synthetic:
        model, vocabulary = synthetic_whisper(device, args.seed, args.whisper_timestamps) if whisper else synthetic_model(device, args.seed)
        items = synthetic_waves(args.synthetic, args.seed)
        transcripts, references = None, [None] * len(items)
    else:
        if whisper and not (args.filelist and args.whisper_checkpoint):
            raise SystemExit("--recogniser whisper: give --filelist and --whisper_checkpoint, or --synthetic N")
        if not whisper and (not args.filelist or not args.ctc_path or not args.vocab_path):
            raise SystemExit("give --filelist, --ctc_path and --vocab_path, or --synthetic N")
        with open(args.filelist, encoding="utf-8") as f:
            entries = parse_filelist(f.read())
        if not entries:
            raise SystemExit(f"{args.filelist}: no files")
        if whisper:
            from unitspeech_amd.whisper import WhisperVocabulary, load_whisper_checkpoint
            added = os.path.join(args.whisper_checkpoint, "added_tokens.json")
            vocabulary = WhisperVocabulary(os.path.join(args.whisper_checkpoint, "vocab.json"), added if os.path.exists(added) else None)
            model = load_whisper_checkpoint(args.whisper_checkpoint).to(device)
        else:
            vocabulary = CTCVocabulary(args.vocab_path, args.blank, args.word_delimiter)
            config = {}
            if args.config_path:
                with open(args.config_path, encoding="utf-8") as f:
                    config = {k: v for k, v in json.load(f).items() if k not in ("vocab_size", "pad_token_id")}
            model = load_ctc_checkpoint(args.ctc_path, pad_token_id=vocabulary.blank_id, **config).to(device)
        items = [(path,) + read_wav(path) for path, _, _ in entries]
        transcripts = [normalize_text(text, vocabulary) for _, text, _ in entries]
        references = [ref for _, _, ref in entries]
        if args.speaker_encoder_path and any(references):
            from unitspeech_amd.speaker_encoder import load_speaker_embedder_checkpoint
            embedder = load_speaker_embedder_checkpoint(args.speaker_encoder_path, device)
    if args.sv56:
        items, levels = normalize_items(items, args.ndb, args.batch, device)
        for (name, _, _), (level, gain, clipped) in zip(items, levels):
            print(f"{name}: sv56 level {level:.2f} dB, gain {gain:.4f}, {clipped} clipped samples")
    wavs16 = []
    for name, wav, rate in items:
        w = to_16k(wav, rate, device, resamplers)
        if w.shape[0] < MIN_SAMPLES_16K:
            raise SystemExit(f"{name}: {w.shape[0]} samples at 16 kHz are fewer than the receptive field ({MIN_SAMPLES_16K})")
        wavs16.append(w)
    if whisper:
        whisper_prompt(model, vocabulary, args.language)
    else:
        model.pad_token_id = vocabulary.blank_id
    mos = None
    if args.mos_path or args.mos:
        if args.mos_path:
            from unitspeech_amd.mos import load_mos_checkpoint
            extra = {} if args.mos_clipping is None else {"clipping": bool(args.mos_clipping)}
            predictor = load_mos_checkpoint(args.mos_path, args.mos_upstream, **extra).to(device)
        else:
            predictor = synthetic_mos(device, args.seed)
        mos = mos_all(predictor, wavs16, args.batch)
    if args.normalize:
        wavs16 = [(w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7) for w in wavs16]
    scores = [] if args.whisper_timestamps else None
    beam = None
    if args.whisper_beam_size is not None:
        beam = dict(beam_size=args.whisper_beam_size, patience=args.whisper_patience)
    hyps, batches = transcribe_all(model, vocabulary, wavs16, args.batch, scores, beam)
    if whisper:
        hyps = [normalize_text(h, vocabulary) for h in hyps]
    result = {}
    if beam is not None:
        result.update(whisper_beam_size=args.whisper_beam_size, whisper_patience=1.0 if args.whisper_patience is None else args.whisper_patience)
    if args.synthetic:
        transcripts = [apply_edits(h, SYNTHETIC_EDITS, cut=bool(i & 1)) for i, h in enumerate(hyps)]
        result["expected_cer"] = SYNTHETIC_EDITS * len(hyps) / sum(len(t) for t in transcripts)
    rates = error_rates(hyps, transcripts, device)
    secs = [None] * len(items)
    if embedder is not None:
        refs16 = [to_16k(*read_wav(r), device, resamplers) if r else None for r in references]
        secs = similarities(embedder, wavs16, refs16, args.batch)
    words = word_timestamps(model, vocabulary, wavs16, transcripts, batches) if args.timestamps else None
    files = []
    for k, ((name, _, _), h, t, p, s) in enumerate(zip(items, hyps, transcripts, rates["per_utterance"], secs)):
        rec = dict(file=name, hypothesis=h, reference=t, **p)
        if s is not None:
            rec["secs"] = s
        if words is not None:
            rec["word_times"] = words[k]
        if scores is not None:
            rec.update(scores[k])
        if mos is not None:
            rec["mos"] = mos[k]
        files.append(rec)
        print(f"{name}: CER {p['cer']:.4f} ({p['char_distance']}/{p['chars']})  WER {p['wer']:.4f} ({p['word_distance']}/{p['words']})"
              + (f"  SECS {s:.4f}" if s is not None else "") + (f"  MOS {mos[k]:.4f}" if mos is not None else "") + f"  | {h!r} <- {t!r}")
    result.update(cer=rates["cer"], wer=rates["wer"], files=len(files), batches=len(batches), per_file=files)
    have = [s for s in secs if s is not None]
    if have:
        result["secs"] = float(np.mean(have))
    if mos is not None:
        result.update(mos=float(np.mean(mos)), mos_min=float(np.min(mos)), mos_max=float(np.max(mos)))
    print(json.dumps({k: v for k, v in result.items() if k != "per_file"}))
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            json.dump(result, f, ensure_ascii=False, indent=1)


if __name__ == "__main__":
    main()
