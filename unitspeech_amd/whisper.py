"""Whisper on the HIP library (`csrc/whisper.hip`, the encoder schedule in `csrc/hubert.hip`): what the reference's evaluation notebook does
with `whisper.load_model`, `pad_or_trim`, `log_mel_spectrogram` and `decode(model, mel, DecodingOptions())`.

`WhisperForConditionalGeneration` takes transformers' configuration fields by keyword and its state_dict; `log_mel_spectrogram` is Whisper's
feature extraction in torch ops; `WhisperVocabulary` turns ids into text.  `generate` is plain greedy decoding (no timestamp rules: put `<|notimestamps|>` in
the prompt); `decode` is greedy decoding under the timestamp rules, with `avg_logprob` and `no_speech_prob`: what
`whisper.decode(model, mel, DecodingOptions())` runs by default (`without_timestamps=False`); with `beam_size` (and `patience`) it is beam
search under the same rules, `DecodingOptions(beam_size=n, patience=p)`, what the `whisper` command line runs with n = 5.  No temperature
fallback, no window beyond 30 s (a longer item is refused), fp32 weights.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._handle import HandleModule
from ._wav_encoder import _set
from .mel import mel_filterbank

SAMPLE_RATE, N_FFT, HOP, N_SAMPLES = 16000, 400, 160, 480000
_FIELDS = ("num_mel_bins", "d_model", "encoder_layers", "encoder_attention_heads", "encoder_ffn_dim", "decoder_layers", "decoder_attention_heads",
           "decoder_ffn_dim", "max_source_positions", "max_target_positions", "vocab_size")
_DEFAULTS = dict(num_mel_bins=80, d_model=384, encoder_layers=4, encoder_attention_heads=6, encoder_ffn_dim=1536, decoder_layers=4,
                 decoder_attention_heads=6, decoder_ffn_dim=1536, max_source_positions=1500, max_target_positions=448, vocab_size=51865)
MEDIUM = dict(num_mel_bins=80, d_model=1024, encoder_layers=24, encoder_attention_heads=16, encoder_ffn_dim=4096, decoder_layers=24,
              decoder_attention_heads=16, decoder_ffn_dim=4096, max_source_positions=1500, max_target_positions=448, vocab_size=51865)


def log_mel_spectrogram(wav16, lengths=None, n_mels: int = 80):
    """16 kHz waveform [B, T] (or [T]) with per-item lengths -> Whisper's input features [B, n_mels, 3000] (fp32, on the waveform's device):
    pad / trim to 480,000 samples (samples at and past an item's length count as silence), n_fft 400, hop 160, periodic Hann, reflect-centred
    frames with the last one dropped, power spectrum, the Slaney mel bank, log10(max(x, 1e-10)), per-item max(x, x.max() - 8), (x + 4) / 4.
    Computed in fp64 and rounded once: the stage is far below 1 % of a transcription."""
    x = torch.as_tensor(wav16)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError(f"log_mel_spectrogram: expected a waveform [B, T], got {tuple(x.shape)}")
    B, T = x.shape
    x = x.to(torch.float64)
    if lengths is not None:
        n = torch.as_tensor(lengths, device=x.device).to(torch.int64).view(B, 1)
        x = torch.where(torch.arange(T, device=x.device)[None] < n, x, torch.zeros((), dtype=x.dtype, device=x.device))
    x = x[:, :N_SAMPLES] if T >= N_SAMPLES else torch.nn.functional.pad(x, (0, N_SAMPLES - T))
    window = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64, device=x.device)
    spec = torch.stft(x, N_FFT, HOP, window=window, center=True, pad_mode="reflect", return_complex=True)[..., :-1]
    power = spec.real ** 2 + spec.imag ** 2
    bank = torch.from_numpy(np.asarray(mel_filterbank(SAMPLE_RATE, N_FFT, n_mels), dtype=np.float64)).to(x.device)
    mel = torch.log10(torch.clamp(bank @ power, min=1e-10))
    mel = torch.maximum(mel, mel.amax(dim=(1, 2), keepdim=True) - 8.0)
    return ((mel + 4.0) / 4.0).to(torch.float32)


def _bytes_to_unicode():
    """GPT-2's table: every byte as a printable character"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


class _ScoringAlphabet:
    def __contains__(self, c):
        return c in " '" or (c.isalnum() and c == c.lower())

    def __iter__(self):                  # normalize_text looks at the letters' case: all lower
        return iter("abcdefghijklmnopqrstuvwxyz '")


TIME_PRECISION = 0.02           # seconds per timestamp index


@dataclass
class WhisperDecoding:
    """what `WhisperForConditionalGeneration.decode` returns, on the device: tokens [B, L] int64 (eos at and after an item's end), lengths
    [B] int64, sum_logprob [B] fp32 (every generated token, the closing eos included), no_speech_prob [B] fp32 or None"""
    tokens: torch.Tensor
    lengths: torch.Tensor
    sum_logprob: torch.Tensor
    no_speech_prob: torch.Tensor | None

    @property
    def avg_logprob(self):
        """openai's: sum_logprob / (length + 1)"""
        return self.sum_logprob / (self.lengths + 1).to(self.sum_logprob.dtype)


class WhisperVocabulary:
    """`vocab.json` (token -> id, tokens in GPT-2's byte alphabet) and optionally `added_tokens.json` (the special tokens) of a Whisper
    tokenizer; either may be a path or a dict.  `decode(ids)` drops the special tokens (anything written `<|...|>`, every added token and
    every id the vocabulary lacks) and turns the rest into text."""

    def __init__(self, vocab, added_tokens=None):
        def read(v):
            if isinstance(v, (str, os.PathLike)):
                with open(v, encoding="utf-8") as f:
                    return json.load(f)
            return dict(v or {})
        vocab, added = read(vocab), read(added_tokens)
        self.token_to_id = {**vocab, **added}
        self.special = {i for t, i in self.token_to_id.items() if t in added or (t.startswith("<|") and t.endswith("|>"))}
        self.id_to_token = {i: t for t, i in self.token_to_id.items()}
        self._byte = {c: b for b, c in _bytes_to_unicode().items()}

    def __len__(self):
        return len(self.token_to_id)

    def token_id(self, token: str) -> int:
        if token not in self.token_to_id:
            raise KeyError(f"WhisperVocabulary: no token {token!r}")
        return self.token_to_id[token]

    start_id = property(lambda self: self.token_id("<|startoftranscript|>"))
    transcribe_id = property(lambda self: self.token_id("<|transcribe|>"))
    notimestamps_id = property(lambda self: self.token_id("<|notimestamps|>"))
    end_id = property(lambda self: self.token_id("<|endoftext|>"))
    timestamp_begin = property(lambda self: self.notimestamps_id + 1)

    @property
    def nospeech_id(self) -> int:
        for t in ("<|nospeech|>", "<|nocaptions|>"):     # the older vocabularies spell it the second way
            if t in self.token_to_id:
                return self.token_to_id[t]
        raise KeyError("WhisperVocabulary: neither <|nospeech|> nor <|nocaptions|>")

    def segments(self, ids):
        """ids with timestamp tokens (>= timestamp_begin, 0.02 s per index) -> [(start_s, end_s, text)]: the text between a timestamp and
        the next one.  Text in front of any timestamp starts at None; an unclosed last segment ends at None; of two timestamps in a
        row the first closes a segment and the second opens the next."""
        tb = self.timestamp_begin
        out, start, text = [], None, []
        for i in (int(v) for v in (ids.tolist() if hasattr(ids, "tolist") else ids)):
            if i >= tb:
                t = round((i - tb) * TIME_PRECISION, 2)
                if text:
                    out.append((start, t, self.decode(text)))
                    start, text = None, []
                else:
                    start = t
            elif i not in self.special and i in self.id_to_token:
                text.append(i)
        if text:
            out.append((start, None, self.decode(text)))
        return out

    def language_id(self, language: str) -> int:
        return self.token_id(f"<|{language}|>")

    def language_ids(self):
        """the ids of the two- and three-letter `<|xx|>` tokens"""
        return sorted(i for t, i in self.token_to_id.items() if t.startswith("<|") and t.endswith("|>") and t[2:-2].isalpha() and t[2:-2].islower()
                      and len(t) in (6, 7))

    @property
    def characters(self):
        """what `asr.normalize_text` keeps of a transcript: a byte-level vocabulary can write any character, so the scoring alphabet is
        chosen here: lower-case letters and digits of any script, the apostrophe and the space"""
        return _ScoringAlphabet()

    def decode(self, ids, n=None):
        """ids: a sequence of ints -> str; or [B, L] with counts `n` [B] -> list of str"""
        if n is not None:
            return [self.decode(row[:int(k)]) for row, k in zip(torch.as_tensor(ids).tolist(), torch.as_tensor(n).tolist())]
        raw = bytearray()
        for i in (int(v) for v in (ids.tolist() if hasattr(ids, "tolist") else ids)):
            t = self.id_to_token.get(i)
            if t is None or i in self.special:
                continue
            raw.extend(self._byte[c] for c in t)
        return raw.decode("utf-8", errors="replace")


class WhisperForConditionalGeneration(HandleModule):
    """`transformers.WhisperForConditionalGeneration` in eval mode on the HIP library: the configuration's fields by keyword, the
    state_dict's keys (`proj_out.weight` is the tied `model.decoder.embed_tokens.weight`: accepted when equal, refused when not)."""
    _abi = "whisper"
    _what = "Whisper recogniser"
    _cache_sources = True

    def __init__(self, **config):
        super().__init__()
        unknown = sorted(k for k in config if k not in _FIELDS)
        self.config = c = {k: int(config.get(k, _DEFAULTS[k])) for k in _FIELDS}
        self.extra_config = {k: config[k] for k in unknown}        # eos_token_id, suppress_tokens ...: kept for the caller, not used here
        H = c["d_model"]
        for side in ("encoder", "decoder"):
            nh = c[side + "_attention_heads"]
            if nh < 1 or H % nh:
                raise ValueError(f"WhisperForConditionalGeneration: d_model = {H} must be divisible by the {side}'s {nh} heads")
            if (H // nh) > 64 or (H // nh) % 4:
                raise ValueError(f"WhisperForConditionalGeneration: the head dimension must be a multiple of 4, at most 64 (got {H // nh})")
        self.prompt_ids = None           # transcribe_ids: [start, language or None, task, notimestamps]
        self.language_ids = None         # transcribe_ids: the candidates of detect_language when the prompt's language is None
        self.no_timestamps_id = None     # transcribe_ids(timestamps=True): left out of the prompt; the token in front of the first timestamp
        self.no_speech_id = None         # transcribe_ids(timestamps=True): when set, no_speech_prob is computed
        self.eos_token_id = self.extra_config.get("eos_token_id")
        self.suppress_tokens = self.extra_config.get("suppress_tokens")
        self.begin_suppress_tokens = self.extra_config.get("begin_suppress_tokens")
        self._masks = {}

        def affine(p):
            _set(self, p + ".weight", torch.ones(H))
            _set(self, p + ".bias", torch.zeros(H))

        def linear(p, o, i, bias=True):
            _set(self, p + ".weight", torch.zeros(o, i))
            if bias:
                _set(self, p + ".bias", torch.zeros(o))

        def attention(p):
            linear(p + ".k_proj", H, H, False)
            linear(p + ".v_proj", H, H)
            linear(p + ".q_proj", H, H)
            linear(p + ".out_proj", H, H)

        _set(self, "model.encoder.conv1.weight", torch.zeros(H, c["num_mel_bins"], 3))
        _set(self, "model.encoder.conv1.bias", torch.zeros(H))
        _set(self, "model.encoder.conv2.weight", torch.zeros(H, H, 3))
        _set(self, "model.encoder.conv2.bias", torch.zeros(H))
        _set(self, "model.encoder.embed_positions.weight", torch.zeros(c["max_source_positions"], H))
        for i in range(c["encoder_layers"]):
            p = f"model.encoder.layers.{i}"
            attention(p + ".self_attn")
            affine(p + ".self_attn_layer_norm")
            linear(p + ".fc1", c["encoder_ffn_dim"], H)
            linear(p + ".fc2", H, c["encoder_ffn_dim"])
            affine(p + ".final_layer_norm")
        affine("model.encoder.layer_norm")
        _set(self, "model.decoder.embed_tokens.weight", torch.zeros(c["vocab_size"], H))
        _set(self, "model.decoder.embed_positions.weight", torch.zeros(c["max_target_positions"], H))
        for i in range(c["decoder_layers"]):
            p = f"model.decoder.layers.{i}"
            attention(p + ".self_attn")
            affine(p + ".self_attn_layer_norm")
            attention(p + ".encoder_attn")
            affine(p + ".encoder_attn_layer_norm")
            linear(p + ".fc1", c["decoder_ffn_dim"], H)
            linear(p + ".fc2", H, c["decoder_ffn_dim"])
            affine(p + ".final_layer_norm")
        affine("model.decoder.layer_norm")

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = dict(state_dict)
        tied = sd.pop("proj_out.weight", None)
        if tied is not None and "model.decoder.embed_tokens.weight" in sd and not torch.equal(tied, sd["model.decoder.embed_tokens.weight"]):
            raise ValueError("WhisperForConditionalGeneration: proj_out.weight differs from model.decoder.embed_tokens.weight; only the tied "
                             "projection is built")
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- engine ----------------------------------------------------------------------------------------------------------------

    def _create(self, lib, device):
        c, s = self.config, _lib.us_whisper_config()
        s.n_mels, s.d_model, s.vocab_size = c["num_mel_bins"], c["d_model"], c["vocab_size"]
        s.encoder_layers, s.encoder_heads, s.encoder_ffn = c["encoder_layers"], c["encoder_attention_heads"], c["encoder_ffn_dim"]
        s.decoder_layers, s.decoder_heads, s.decoder_ffn = c["decoder_layers"], c["decoder_attention_heads"], c["decoder_ffn_dim"]
        s.max_source_positions, s.max_target_positions = c["max_source_positions"], c["max_target_positions"]
        _lib.check(lib.us_whisper_create(C.byref(self._h), C.byref(s)), None, "us_whisper_create")

    def _precondition(self):
        if self.training:
            raise RuntimeError("WhisperForConditionalGeneration is inference-only: call .eval()")

    def _features(self, input_features):
        x = input_features
        if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] != self.config["num_mel_bins"]:
            raise ValueError(f"WhisperForConditionalGeneration: expected features [B, {self.config['num_mel_bins']}, T], got {tuple(x.shape)}")
        lib, stream = self._sync(x.device)
        x = x.detach().to(torch.float32).contiguous()
        B, T = int(x.shape[0]), int(x.shape[2])
        return lib, stream, x, B, T, self._workspace(lib, x.device, B)

    def _ids(self, ids, B, name):
        t = torch.as_tensor(ids).detach().to("cpu", torch.int64)
        if t.dim() == 1:
            t = t[None].expand(B, -1)
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1:
            raise ValueError(f"WhisperForConditionalGeneration: {name} must be [B, N] (or [N] for every item) with N >= 1, got {tuple(t.shape)}")
        t = t.contiguous()
        return t, (C.c_int64 * t.numel())(*t.view(-1).tolist())

    @torch.no_grad()
    def encode(self, input_features):
        """[B, n_mels, 2 S] -> the encoder's last hidden state [B, S, d_model]"""
        lib, stream, x, B, T, ws = self._features(input_features)
        out = torch.empty(B, self.config["max_source_positions"], self.config["d_model"], device=x.device)
        self._call(lib, x.device, "encode", self._h, x.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return out

    @torch.no_grad()
    def logits(self, input_features, decoder_input_ids):
        """teacher forcing: decoder_input_ids [B, N] -> [B, N, V]"""
        lib, stream, x, B, T, ws = self._features(input_features)
        t, ids = self._ids(decoder_input_ids, B, "decoder_input_ids")
        out = torch.empty(B, t.shape[1], self.config["vocab_size"], device=x.device)
        self._call(lib, x.device, "decoder_logits", self._h, x.data_ptr(), B, T, ids, int(t.shape[1]), out.data_ptr(), ws.data_ptr(), ws.numel(),
                   stream)
        return out

    def _mask(self, tokens, device):
        if tokens is None or len(tokens) == 0:
            return None
        key = (tuple(int(t) for t in tokens), device)
        if key not in self._masks:
            V = self.config["vocab_size"]
            if min(key[0]) < 0 or max(key[0]) >= V:
                raise ValueError(f"WhisperForConditionalGeneration: a suppressed token lies outside the vocabulary [0, {V})")
            m = torch.zeros(V, dtype=torch.uint8)
            m[list(key[0])] = 1
            self._masks = {key: m.to(device), **dict(list(self._masks.items())[-3:])}
        return self._masks[key]

    @torch.no_grad()
    def generate(self, input_features, prompt_ids, max_new_tokens=None, suppress_tokens=None, begin_suppress_tokens=None, eos_token_id=None):
        """greedy decoding after the teacher-forced prompt [B, P] (or [P]) -> (tokens [B, max_new_tokens] int64 with eos at and after an
        item's end, lengths [B] int64: the tokens in front of it)"""
        lib, stream, x, B, T, ws = self._features(input_features)
        t, ids = self._ids(prompt_ids, B, "prompt_ids")
        P = int(t.shape[1])
        eos = self.eos_token_id if eos_token_id is None else eos_token_id
        if eos is None:
            raise ValueError("WhisperForConditionalGeneration.generate: no eos_token_id (give it here or in the configuration)")
        max_new = self.config["max_target_positions"] - P if max_new_tokens is None else int(max_new_tokens)
        sup, beg = self._mask(suppress_tokens, x.device), self._mask(begin_suppress_tokens, x.device)
        tokens = torch.empty(B, max(max_new, 1), dtype=torch.int64, device=x.device)
        n = torch.empty(B, dtype=torch.int64, device=x.device)
        self._call(lib, x.device, "generate", self._h, x.data_ptr(), B, T, ids, P, max_new, int(eos), _ptr(sup), _ptr(beg), tokens.data_ptr(),
                   n.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return tokens, n

    @torch.no_grad()
    def decode(self, input_features, prompt_ids, *, no_timestamps_id, max_initial_timestamp=1.0, no_speech_id=None, max_new_tokens=None,
               suppress_tokens=None, begin_suppress_tokens=None, eos_token_id=None, sot_index=0, beam_size=None, patience=None):
        """Greedy decoding under the timestamp rules after the teacher-forced prompt [B, P] (or [P]; no `<|notimestamps|>` in it): what
        `whisper.decode(model, mel, DecodingOptions())` does.  `no_timestamps_id + 1` is the first timestamp token; the first generated token
        is a timestamp of at most `max_initial_timestamp` seconds (None: any); `no_speech_id` asks for `no_speech_prob`, read after the
        prompt's token `sot_index`; `max_new_tokens` defaults to max_target_positions // 2, openai's sample_len.  -> WhisperDecoding.
        `beam_size` n in [1, 16]: beam search under the same rules (`us_whisper_decode_beam`) with max_candidates = round(n * patience),
        patience 1.0 by default; `sum_logprob` is the winning sequence's score.  `patience` alone is refused."""
        what = "WhisperForConditionalGeneration.decode"
        if patience is not None and beam_size is None:
            raise ValueError(f"{what}: patience belongs to beam search: give beam_size")
        eos = self.eos_token_id if eos_token_id is None else eos_token_id
        if eos is None:
            raise ValueError(f"{what}: no eos_token_id (give it here or in the configuration)")
        if max_initial_timestamp is not None and not max_initial_timestamp >= 0:
            raise ValueError(f"{what}: max_initial_timestamp must be None or at least 0 seconds")
        max_new = self.config["max_target_positions"] // 2 if max_new_tokens is None else int(max_new_tokens)
        if max_new < 1:
            raise ValueError(f"{what}: max_new_tokens must be at least 1")
        lib, stream, x, B, T, ws = self._features(input_features)
        t, ids = self._ids(prompt_ids, B, "prompt_ids")
        P = int(t.shape[1])
        o = _lib.us_whisper_decode_options()
        o.eos, o.no_timestamps, o.sot_index, o.max_new = int(eos), int(no_timestamps_id), int(sot_index), max_new
        o.max_initial_timestamp_index = -1 if max_initial_timestamp is None else int(round(max_initial_timestamp / TIME_PRECISION))
        o.no_speech = -1 if no_speech_id is None else int(no_speech_id)
        suppress_tokens = self.suppress_tokens if suppress_tokens is None else suppress_tokens
        begin_suppress_tokens = self.begin_suppress_tokens if begin_suppress_tokens is None else begin_suppress_tokens
        sup, beg = self._mask(suppress_tokens, x.device), self._mask(begin_suppress_tokens, x.device)
        tokens = torch.empty(B, max(max_new, 1), dtype=torch.int64, device=x.device)
        n = torch.empty(B, dtype=torch.int64, device=x.device)
        lp = torch.empty(B, dtype=torch.float32, device=x.device)
        ns = torch.empty(B, dtype=torch.float32, device=x.device) if no_speech_id is not None else None
        name, beam = "decode", ()
        if beam_size is not None:
            nb = int(beam_size)
            name, beam = "decode_beam", (nb, int(round(nb * (1.0 if patience is None else float(patience)))))
            ws = self._beam_workspace(lib, x.device, B, nb)
        self._call(lib, x.device, name, self._h, x.data_ptr(), B, T, ids, P, C.byref(o), *beam, _ptr(sup), _ptr(beg), tokens.data_ptr(), n.data_ptr(),
                   lp.data_ptr(), _ptr(ns), ws.data_ptr(), ws.numel(), stream)
        return WhisperDecoding(tokens, n, lp, ns)

    def _beam_workspace(self, lib, device, B, beam_size):
        """the call's scratch grown to us_whisper_beam_workspace_bytes (0 for a beam size the library refuses: the call reports it)"""
        n = int(lib.us_whisper_beam_workspace_bytes(self._h, B, beam_size))
        if self._ws.numel() < n:
            self._ws = None
            self._ws = torch.empty(n, dtype=torch.uint8, device=device)
        return self._ws

    @torch.no_grad()
    def detect_language(self, input_features, language_ids, start_id=None):
        """One step from the start token, argmax over `language_ids` -> [B] int64 (on the device): the first thing `whisper.decode` does
        when no language is set."""
        start = self.extra_config.get("decoder_start_token_id") if start_id is None else start_id
        if start is None:
            start = self.prompt_ids[0] if self.prompt_ids else None
        if start is None:
            raise ValueError("detect_language: no start token (start_id, decoder_start_token_id or prompt_ids[0])")
        cand = torch.as_tensor(list(language_ids), dtype=torch.int64, device=input_features.device)
        lg = self.logits(input_features, torch.full((input_features.shape[0], 1), int(start), dtype=torch.int64))[:, 0]
        return cand[lg[:, cand].argmax(-1)]

    @torch.no_grad()
    def transcribe_ids(self, wav16, lengths=None, language_id=None, prompt_ids=None, max_new_tokens=None, timestamps=False, beam_size=None,
                       patience=None):
        """16 kHz waveforms [B, T] with per-item lengths -> (tokens [B, L], count [B]): log-mel features, the prompt (`prompt_ids`, default
        `self.prompt_ids`: [start, language, task, notimestamps]; a language of None is `language_id`, or detected per item among
        `self.language_ids`), greedy decoding with the configuration's suppression lists.  An item longer than 30 s is refused.
        timestamps=True: the three-token prompt (the prompt without `self.no_timestamps_id`) and `decode` under the timestamp rules, with
        `no_speech_prob` when `self.no_speech_id` is set -> WhisperDecoding; `beam_size` / `patience` go to `decode` and need timestamps=True
        (beam search is built under the timestamp rules only)."""
        if (beam_size is not None or patience is not None) and not timestamps:
            raise ValueError("WhisperForConditionalGeneration.transcribe_ids: beam_size / patience need timestamps=True: beam search is built "
                             "under the timestamp rules only, not for the prompt with <|notimestamps|>")
        x = torch.as_tensor(wav16)
        if x.dim() == 1:
            x = x[None]
        B = x.shape[0]
        n = [int(v) for v in (torch.as_tensor(lengths).tolist() if lengths is not None else [x.shape[1]] * B)]
        if max(n) > N_SAMPLES:
            raise ValueError(f"WhisperForConditionalGeneration.transcribe_ids: item {n.index(max(n))} has {max(n)} samples, more than one 30 s "
                             f"window ({N_SAMPLES}); longer items are not cut")
        feats = log_mel_spectrogram(x, n, self.config["num_mel_bins"])
        prompt = list(self.prompt_ids if prompt_ids is None else prompt_ids)
        if not prompt:
            raise ValueError("WhisperForConditionalGeneration.transcribe_ids: no prompt_ids")
        if timestamps:
            if self.no_timestamps_id is None:
                raise ValueError("WhisperForConditionalGeneration.transcribe_ids: timestamps=True needs no_timestamps_id")
            prompt = [p for p in prompt if p is None or int(p) != int(self.no_timestamps_id)]
        rows = torch.tensor([[0 if p is None else int(p) for p in prompt]] * B, dtype=torch.int64)
        for j, p in enumerate(prompt):
            if p is None:
                if language_id is None and not self.language_ids:
                    raise ValueError("WhisperForConditionalGeneration.transcribe_ids: no language_id and no language_ids to detect one among")
                rows[:, j] = int(language_id) if language_id is not None else self.detect_language(feats, self.language_ids, prompt[0]).cpu()
        if timestamps:
            return self.decode(feats, rows, no_timestamps_id=int(self.no_timestamps_id), no_speech_id=self.no_speech_id, max_new_tokens=max_new_tokens,
                               beam_size=beam_size, patience=patience)
        return self.generate(feats, rows, max_new_tokens, self.suppress_tokens, self.begin_suppress_tokens)


_select_scratch = {}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _select_call(what, logits, history, options, suppress, begin_suppress, scores=None, n=1):
    """What `select_tokens` and `select_beams` (scores, n rows per item) check and marshal alike -> (lib, x, R, V, `us_whisper_history[R]`, the
    options struct of (eos, no_timestamps, max_initial_timestamp_index), the device's cached scratch, the stream)."""
    if logits.device.type != "cuda" or logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"{what}: expected fp32 logits {'[B, V]' if scores is None else '[B * n, V]'} on a ROCm device, got {logits.dtype} "
                         f"{tuple(logits.shape)} on {logits.device}")
    lib = _lib.load()
    x = logits.contiguous()
    R, V = int(x.shape[0]), int(x.shape[1])
    if scores is None and len(history) != R:
        raise ValueError(f"{what}: {len(history)} histories for {R} items")
    if scores is not None and (n < 1 or R % n or len(history) != R or len(scores) != R):
        raise ValueError(f"{what}: {R} rows of logits, {len(history)} histories and {len(scores)} scores do not make items of {n} rows")
    for m in (suppress, begin_suppress):
        if m is not None and (m.dtype != torch.uint8 or m.numel() != V or m.device != x.device):
            raise ValueError(f"{what}: a mask must be uint8 [V] on the logits' device")
    hist = (_lib.us_whisper_history * R)(*[_lib.us_whisper_history(*[int(v) for v in h]) for h in history])
    o = _lib.us_whisper_decode_options(*[int(v) for v in options], -1, 0, 1)
    nbytes = int(lib.us_whisper_select_scratch_bytes(V) if scores is None else lib.us_whisper_beam_select_scratch_bytes(V, n))
    ws = _select_scratch.get(x.device)
    if ws is None or ws.numel() < nbytes:
        _select_scratch[x.device] = ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    return lib, x, R, V, hist, o, ws, C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


@torch.no_grad()
def select_tokens(logits, history, *, eos_token_id, no_timestamps_id, max_initial_timestamp_index=-1, suppress=None, begin_suppress=None):
    """One selection step of `decode` on its own (`us_whisper_select`): logits [B, V] fp32 on the device, history: per item (n_sampled, last,
    penultimate, last_timestamp, done), suppress / begin_suppress: uint8 masks [V] on the device or None -> (token [B] int64, logprob [B]
    fp32, decided_timestamp [B] int32) on the device."""
    lib, x, B, V, hist, o, ws, stream = _select_call("select_tokens", logits, history, (eos_token_id, no_timestamps_id, max_initial_timestamp_index),
                                                     suppress, begin_suppress)
    token = torch.empty(B, dtype=torch.int64, device=x.device)
    logprob = torch.empty(B, dtype=torch.float32, device=x.device)
    decided = torch.empty(B, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.us_whisper_select(x.data_ptr(), B, V, hist, C.byref(o), _ptr(suppress), _ptr(begin_suppress), token.data_ptr(), logprob.data_ptr(),
                                   decided.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc, None, "us_whisper_select")
    return token, logprob, decided


@torch.no_grad()
def select_beams(logits, history, scores, beam_size, *, eos_token_id, no_timestamps_id, max_initial_timestamp_index=-1, suppress=None,
                 begin_suppress=None):
    """One step of `decode(beam_size=n)`'s selection and bookkeeping on its own (`us_whisper_beam_select`): logits [B * n, V] fp32 on the device,
    rows item-major; history: per row (n_sampled, last, penultimate, last_timestamp, dead); scores: per row, floats -> dict on the device:
    parent [B, n] int32 (-1: dead), token [B, n] int64, score [B, n] fp64, n_live [B], fin_parent [B, n] int32 and fin_score [B, n] fp64 (the
    newly finished entries in walk order), n_fin [B]."""
    n = int(beam_size)
    lib, x, R, V, hist, o, ws, stream = _select_call("select_beams", logits, history, (eos_token_id, no_timestamps_id, max_initial_timestamp_index),
                                                     suppress, begin_suppress, scores, n)
    B = R // n
    sc = (C.c_double * R)(*[float(v) for v in scores])
    new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=x.device)
    out = dict(parent=new(torch.int32, B, n), token=new(torch.int64, B, n), score=new(torch.float64, B, n), n_live=new(torch.int32, B),
               fin_parent=new(torch.int32, B, n), fin_score=new(torch.float64, B, n), n_fin=new(torch.int32, B))
    with torch.cuda.device(x.device):
        rc = lib.us_whisper_beam_select(x.data_ptr(), B, V, n, hist, sc, C.byref(o), _ptr(suppress), _ptr(begin_suppress),
                                        *[t.data_ptr() for t in out.values()], ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc, None, "us_whisper_beam_select")
    return out


def detect_language(model, input_features, language_ids, start_id=None):
    return model.detect_language(input_features, language_ids, start_id)


def load_whisper_checkpoint(path):
    """A `torch.save`d state dict (the `openai/whisper-medium` size unless the file is a dict with `config` and `state_dict`), or a directory
    with `config.json` and `pytorch_model.bin` / `model.safetensors` (the latter only where `safetensors` imports) -> the model, with
    eos_token_id and the suppression lists of `generation_config.json` (else `config.json`) set."""
    config, extra = dict(MEDIUM), {}
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
            config = json.load(f)
        gen = os.path.join(path, "generation_config.json")
        if os.path.exists(gen):
            with open(gen, encoding="utf-8") as f:
                extra = json.load(f)
        if os.path.exists(os.path.join(path, "pytorch_model.bin")):
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        elif os.path.exists(os.path.join(path, "model.safetensors")):
            try:
                from safetensors.torch import load_file
            except ImportError as e:
                raise RuntimeError(f"{path} holds model.safetensors only and `safetensors` does not import: save it with torch.save") from e
            sd = load_file(os.path.join(path, "model.safetensors"))
        else:
            raise FileNotFoundError(f"{path}: neither pytorch_model.bin nor model.safetensors")
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "state_dict" in sd and "config" in sd:
            config, sd = dict(sd["config"]), sd["state_dict"]
    keep = {k: config[k] for k in _FIELDS if k in config}
    for k in ("eos_token_id", "decoder_start_token_id", "suppress_tokens", "begin_suppress_tokens"):
        v = extra.get(k, config.get(k))
        if v is not None:
            keep[k] = v
    model = WhisperForConditionalGeneration(**keep)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    return model.eval()


def synthetic_whisper_state_dict(config, seed: int = 0):
    """Seeded weights under transformers' keys at scales where greedy decoding moves: embeddings std 0.03, decoder positions 0.7, the
    encoder's sinusoids, matrices N(0, 1.7^2 / fan_in), LayerNorm weights 1 +- 0.1, biases 0.1."""
    m = WhisperForConditionalGeneration(**config)
    g = np.random.Generator(np.random.Philox(key=11000 + seed))
    sd = {}
    for k, p in m.state_dict().items():
        r = torch.from_numpy(g.standard_normal(tuple(p.shape), dtype=np.float32))
        if k == "model.encoder.embed_positions.weight":
            S, H = p.shape
            inc = np.log(10000.0) / (H // 2 - 1)
            t = torch.arange(S)[:, None] * torch.exp(-inc * torch.arange(H // 2))[None]
            sd[k] = torch.cat([t.sin(), t.cos()], dim=1).float()
        elif k.endswith("embed_tokens.weight"):
            sd[k] = 0.03 * r
        elif k.endswith("embed_positions.weight"):
            sd[k] = 0.7 * r
        elif "layer_norm" in k:
            sd[k] = (1.0 if k.endswith(".weight") else 0.0) + 0.1 * r
        elif k.endswith(".bias"):
            sd[k] = 0.1 * r
        else:
            sd[k] = r * (1.7 / float(np.sqrt(p[0].numel())))
    return sd
