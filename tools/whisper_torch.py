"""A torch restatement of `transformers.WhisperForConditionalGeneration` in eval mode, at a chosen dtype: the encoder, the decoder one
position at a time over a key/value cache, the greedy loop of `us_whisper_generate` and the loop under the timestamp rules of
`us_whisper_decode` (`decode`; the rules are tools/whisper_decode_numpy.py's, at the same dtype) and beam search under them
(`decode_beam`; tools/whisper_beam_numpy.py over this model, the cache gathered by parent).  In fp64 it is the yardstick the goldens are checked
with (tests/test_whisper.py), in fp32 its distance to the golden sets the bar of the GPU tests, and on the device it is bench_whisper.py's
eager leg.

`sd`: the state_dict (keys `model.encoder.*`, `model.decoder.*`); `c`: transformers' configuration fields by name.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import whisper_decode_numpy as rules  # noqa: E402


def golden_state_dict(g):
    """The weights of a tests/golden/whisper_*.npz file `g`: `w:<key>` as it stands, or an int8 grid index times its step `q:<key>`."""
    return {k[2:]: torch.from_numpy(g[k]).float() * float(g["q:" + k[2:]]) if "q:" + k[2:] in g.files else torch.from_numpy(g[k])
            for k in g.files if k.startswith("w:")}


class WhisperTorch:
    def __init__(self, sd, c, dtype=torch.float64, device="cpu"):
        self.c = c
        self.w = {k: v.detach().to(device=device, dtype=dtype) for k, v in sd.items() if k.startswith("model.")}
        self.dtype, self.device = dtype, device

    def _lin(self, x, p, bias=True):
        return F.linear(x, self.w[p + ".weight"], self.w[p + ".bias"] if bias else None)

    def _ln(self, x, p):
        return F.layer_norm(x, x.shape[-1:], self.w[p + ".weight"], self.w[p + ".bias"], 1e-5)

    def _heads(self, x, nh):                     # [B, T, H] -> [B, nh, T, d]
        B, T, H = x.shape
        return x.view(B, T, nh, H // nh).transpose(1, 2)

    def _attend(self, q, k, v):                  # q scaled already; all keys visible
        p = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        o = p @ v
        return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)

    def encode(self, feats):
        """feats [B, n_mels, 2 S] -> [B, S, H]"""
        c, w = self.c, self.w
        if feats.shape[-1] != 2 * c["max_source_positions"]:
            raise ValueError("the features must have exactly 2 * max_source_positions frames")
        x = feats.to(device=self.device, dtype=self.dtype)
        x = F.gelu(F.conv1d(x, w["model.encoder.conv1.weight"], w["model.encoder.conv1.bias"], padding=1))
        x = F.gelu(F.conv1d(x, w["model.encoder.conv2.weight"], w["model.encoder.conv2.bias"], stride=2, padding=1))
        x = x.transpose(1, 2) + w["model.encoder.embed_positions.weight"]
        nh = c["encoder_attention_heads"]
        scale = (c["d_model"] // nh) ** -0.5
        for i in range(c["encoder_layers"]):
            p = f"model.encoder.layers.{i}."
            y = self._ln(x, p + "self_attn_layer_norm")
            q = self._heads(self._lin(y, p + "self_attn.q_proj") * scale, nh)
            k = self._heads(self._lin(y, p + "self_attn.k_proj", False), nh)
            v = self._heads(self._lin(y, p + "self_attn.v_proj"), nh)
            x = x + self._lin(self._attend(q, k, v), p + "self_attn.out_proj")
            y = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(F.gelu(self._lin(y, p + "fc1")), p + "fc2")
        return self._ln(x, "model.encoder.layer_norm")

    def start(self, enc):
        """The decoding state of a batch: the cross keys / values of every layer and an empty self cache."""
        c = self.c
        B, nh, H, Tm = enc.shape[0], c["decoder_attention_heads"], c["d_model"], c["max_target_positions"]
        cross = []
        for i in range(c["decoder_layers"]):
            p = f"model.decoder.layers.{i}.encoder_attn."
            cross.append((self._heads(self._lin(enc, p + "k_proj", False), nh), self._heads(self._lin(enc, p + "v_proj"), nh)))
        cache = torch.zeros(c["decoder_layers"], 2, B, nh, Tm, H // nh, dtype=self.dtype, device=self.device)
        return {"cross": cross, "cache": cache}

    def step(self, state, tokens, pos, logits=True):
        """tokens [B] at position `pos` -> logits [B, V] of the next token (None when logits is False); the cache takes the position"""
        c, w = self.c, self.w
        nh = c["decoder_attention_heads"]
        scale = (c["d_model"] // nh) ** -0.5
        x = (w["model.decoder.embed_tokens.weight"][tokens] + w["model.decoder.embed_positions.weight"][pos])[:, None]
        cache = state["cache"]
        for i in range(c["decoder_layers"]):
            p = f"model.decoder.layers.{i}."
            y = self._ln(x, p + "self_attn_layer_norm")
            q = self._heads(self._lin(y, p + "self_attn.q_proj") * scale, nh)
            cache[i, 0, :, :, pos] = self._heads(self._lin(y, p + "self_attn.k_proj", False), nh)[:, :, 0]
            cache[i, 1, :, :, pos] = self._heads(self._lin(y, p + "self_attn.v_proj"), nh)[:, :, 0]
            x = x + self._lin(self._attend(q, cache[i, 0, :, :, :pos + 1], cache[i, 1, :, :, :pos + 1]), p + "self_attn.out_proj")
            y = self._ln(x, p + "encoder_attn_layer_norm")
            q = self._heads(self._lin(y, p + "encoder_attn.q_proj") * scale, nh)
            x = x + self._lin(self._attend(q, *state["cross"][i]), p + "encoder_attn.out_proj")
            y = self._ln(x, p + "final_layer_norm")
            x = x + self._lin(F.gelu(self._lin(y, p + "fc1")), p + "fc2")
        if not logits:
            return None
        return F.linear(self._ln(x, "model.decoder.layer_norm"), w["model.decoder.embed_tokens.weight"])[:, 0]

    def logits(self, feats, ids):
        """teacher forcing: ids [B, N] -> [B, N, V]"""
        state = self.start(self.encode(feats))
        ids = ids.to(self.device)
        return torch.stack([self.step(state, ids[:, t], t) for t in range(ids.shape[1])], dim=1)

    def generate(self, feats, prompt, max_new, eos, suppress=None, begin_suppress=None, stop_early=True, trace=None):
        """-> (tokens [B, max_new] with eos at and after an item's end, lengths [B]).  suppress / begin_suppress: bool [V] masks.
        trace: a list that receives every step's unmasked logits."""
        state = self.start(self.encode(feats))
        prompt = prompt.to(self.device)
        B, P = prompt.shape
        for t in range(P - 1):
            self.step(state, prompt[:, t], t, logits=False)
        tokens = torch.full((B, max_new), eos, dtype=torch.long, device=self.device)
        n = torch.zeros(B, dtype=torch.long, device=self.device)
        done = torch.zeros(B, dtype=torch.bool, device=self.device)
        cur = prompt[:, P - 1]
        for i in range(max_new):
            lg = self.step(state, cur, P - 1 + i)
            if trace is not None:
                trace.append(lg.clone())
            if suppress is not None:
                lg = lg.masked_fill(suppress.to(self.device), float("-inf"))
            if i == 0 and begin_suppress is not None:
                lg = lg.masked_fill(begin_suppress.to(self.device), float("-inf"))
            tok = torch.where(done, torch.full_like(cur, eos), lg.argmax(-1))
            tokens[:, i] = tok
            done = done | (tok == eos)
            n += (~done).long()
            cur = tok
            if stop_early and (i + 1) % 8 == 0 and bool(done.all()):
                break
        return tokens, n

    def decode(self, feats, prompt, max_new, layout, sot_index=0, trace=None):
        """Greedy decoding under the timestamp rules (`layout`: see tools/whisper_decode_numpy.py), the selection in this object's dtype
        -> dict(tokens [B, max_new] with eos at and after an item's end, lengths [B], logprobs [B, max_new] fp64 (0 after the end),
        sum_logprob [B] fp64, no_speech_prob [B] fp64 or None).  trace: a list that receives every step's unmasked logits [B, V]."""
        np_dtype = {torch.float64: np.float64, torch.float32: np.float32}[self.dtype]
        state = self.start(self.encode(feats))
        prompt = prompt.to(self.device)
        B, P = prompt.shape
        eos, ns = int(layout["eos"]), layout.get("no_speech")
        sup, beg = rules.masks(layout, self.c["vocab_size"])
        nsp = None
        for t in range(P - 1):
            lg = self.step(state, prompt[:, t], t, logits=ns is not None and t == sot_index)
            if lg is not None:
                nsp = np.asarray([rules.no_speech_prob(r, int(ns), np_dtype) for r in lg.cpu().numpy()])
        tokens = np.full((B, max_new), eos, dtype=np.int64)
        lps, lengths, sampled, done = np.zeros((B, max_new)), np.full(B, max_new, dtype=np.int64), [[] for _ in range(B)], [False] * B
        cur = prompt[:, P - 1]
        for i in range(max_new):
            lg = self.step(state, cur, P - 1 + i)
            if trace is not None:
                trace.append(lg.clone())
            rows = lg.cpu().numpy()
            if i == 0 and ns is not None and sot_index == P - 1:
                nsp = np.asarray([rules.no_speech_prob(r, int(ns), np_dtype) for r in rows])
            for b in range(B):
                if done[b]:
                    continue
                r = rules.select(rows[b], sampled[b], layout, sup, beg, np_dtype)
                tokens[b, i], lps[b, i] = r["token"], r["logprob"]
                sampled[b].append(r["token"])
                if r["token"] == eos:
                    done[b], lengths[b] = True, i
            cur = torch.from_numpy(tokens[:, i]).to(self.device)
            if all(done):
                break
        return dict(tokens=tokens, lengths=lengths, logprobs=lps, sum_logprob=lps.sum(1), no_speech_prob=nsp)

    def decode_beam(self, feats, prompt, max_new, layout, beam_size, max_candidates, sot_index=0):
        """Beam search under the timestamp rules (tools/whisper_beam_numpy.py, the selection in this object's dtype), one item after the
        other: its beam_size rows share the encoder output, and the self cache is gathered by parent after each step
        -> dict(tokens [B, max_new], lengths [B], sum_logprob [B] fp64, no_speech_prob [B] fp64 or None, items: beam_search's dicts)."""
        import whisper_beam_numpy as beam
        np_dtype = {torch.float64: np.float64, torch.float32: np.float32}[self.dtype]
        enc = self.encode(feats)
        prompt = prompt.to(self.device)
        B, P = prompt.shape
        n, V, ns = int(beam_size), self.c["vocab_size"], layout.get("no_speech")
        nsp, items = (np.zeros(B) if ns is not None else None), []
        for b in range(B):
            state = self.start(enc[b:b + 1].expand(n, -1, -1))
            for t in range(P - 1):
                lg = self.step(state, prompt[b, t].expand(n), t, logits=ns is not None and t == sot_index)
                if lg is not None:
                    nsp[b] = rules.no_speech_prob(lg[0].cpu().numpy(), int(ns), np_dtype)

            def logits_fn(i, tokens, parents, b=b, state=state):
                if i == 0:
                    cur = prompt[b, P - 1].expand(n)
                else:
                    state["cache"] = state["cache"][:, :, torch.as_tensor(parents, device=self.device)]
                    cur = torch.as_tensor(tokens, dtype=torch.long, device=self.device)
                rows = self.step(state, cur, P - 1 + i).cpu().numpy()
                if i == 0 and ns is not None and sot_index == P - 1:
                    nsp[b] = rules.no_speech_prob(rows[0], int(ns), np_dtype)
                return rows

            items.append(beam.beam_search(logits_fn, n, int(max_candidates), max_new, layout, V, np_dtype))
        return dict(tokens=np.stack([r["tokens"] for r in items]), lengths=np.asarray([r["length"] for r in items], dtype=np.int64),
                    sum_logprob=np.asarray([r["sum_logprob"] for r in items]), no_speech_prob=nsp, items=items)
