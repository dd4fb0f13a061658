"""A restatement of s3prl's MOS predictor (`s3prl.hub.mos_wav2vec2`: upstream/mos_prediction) layer by layer, with nothing folded: the
fp64 yardstick of tests/test_mos*.py and the eager leg of bench_mos.py.  It needs torch and numpy only.

Per item, with hidden states h_l[t], l = 0..L (transformers' `hidden_states`), t over the item's own F frames:

  1. Featurizer   s = softmax(weights) over the L + 1 states, x[t] = sum_l s_l h_l[t]       (the optional per-layer layer_norm is not built)
  2. connector    z[t] = C x[t] + c, C [P][H]; no activation follows
  3. head         attention pooling: e[t] = a . z[t] + a0, alpha = softmax_t(e), u = sum_t alpha_t z[t], score = m . u + m0
                  without it:        score = mean_t(m . z[t] + m0)
  4. clipping     score = 2 tanh(score) + 3

The weights are a dict under the keys of `unitspeech_amd.mos.MOSHead`: `featurizer.weights` [L+1], `connector.{weight,bias}`,
`model.mean_net_pooling.W.{weight [1][P], bias [1]}` (absent: no attention pooling), `model.mean_net_linear.{weight [1][P], bias [1]}`.

    MosTorch(weights, dtype).head(hs [L+1, F, H], clipping) -> dict(score, e, mu, alpha, z)       (mu[t] = m . z[t] + m0, reported alongside)
    MosTorch(weights, dtype).predict(upstream_sd, cfg, wav [T], clipping, attention) -> score     (tools/hubert_torch.py in front)
    mos_head_numpy(weights, hs, dtype, attention=None, clipping=False) -> (score, mu, alpha)      (numpy, every step in `dtype`)
    mos_fold_numpy(weights) -> (s, v_e, v_m, k_e, k_m) in fp64: the folded form the library packs
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hubert_torch import hubert_forward_torch  # noqa: E402

ATT = "model.mean_net_pooling.W."
MEAN = "model.mean_net_linear."


class MosTorch:
    def __init__(self, weights, dtype=torch.float64):
        self.dtype = dtype
        self.w = {k: torch.as_tensor(v).to(dtype) for k, v in weights.items()}
        self.has_attention = ATT + "weight" in self.w

    @torch.no_grad()
    def head(self, hs, clipping=False, attention=None):
        """hs [L+1, F, H] of one item -> dict of the score and the intermediate values; `attention` None: as the weights have it."""
        w = self.w
        attention = self.has_attention if attention is None else bool(attention)
        hs = torch.as_tensor(hs).to(self.dtype)
        s = torch.softmax(w["featurizer.weights"], dim=-1)                              # 1
        x = (s[:, None, None] * hs).sum(0)
        z = x @ w["connector.weight"].t() + w["connector.bias"]                          # 2
        mu = (z @ w[MEAN + "weight"].t() + w[MEAN + "bias"])[:, 0]
        out = dict(z=z, mu=mu)
        if attention:                                                                    # 3
            e = (z @ w[ATT + "weight"].t() + w[ATT + "bias"])[:, 0]
            alpha = torch.softmax(e, dim=0)
            u = (alpha[:, None] * z).sum(0)
            score = (u @ w[MEAN + "weight"].t() + w[MEAN + "bias"])[0]
            out.update(e=e, alpha=alpha)
        else:
            score = mu.mean()
            out.update(e=torch.zeros_like(mu), alpha=torch.full_like(mu, 1.0 / max(int(mu.shape[0]), 1)))
        if clipping:                                                                     # 4
            score = 2.0 * torch.tanh(score) + 3.0
        out["score"] = score
        return out

    @torch.no_grad()
    def predict(self, upstream_sd, cfg, wav, clipping=False, attention=None):
        """wav [T] at 16 kHz -> the score, the upstream being tools/hubert_torch.py on the item alone."""
        hs = hubert_forward_torch(upstream_sd, cfg, torch.as_tensor(wav)[None], None, self.dtype)
        return self.head(torch.stack([h[0] for h in hs]), clipping, attention)["score"]


def mos_head_numpy(weights, hs, dtype=np.float64, attention=None, clipping=False):
    """The same four steps in numpy, every array and operation in `dtype`: hs [L+1, F, H] -> (score, mu [F], alpha [F])."""
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items()}
    attention = (ATT + "weight" in w) if attention is None else bool(attention)
    hs = np.asarray(hs).astype(dtype)
    fw = w["featurizer.weights"]
    s = np.exp(fw - fw.max())
    s = (s / s.sum()).astype(dtype)
    x = (s[:, None, None] * hs).sum(0, dtype=dtype)
    z = (x @ w["connector.weight"].T + w["connector.bias"]).astype(dtype)
    mu = (z @ w[MEAN + "weight"][0] + w[MEAN + "bias"][0]).astype(dtype)
    F = hs.shape[1]
    if F == 0:
        return dtype(np.nan), mu, np.zeros(0, dtype)
    if attention:
        e = (z @ w[ATT + "weight"][0] + w[ATT + "bias"][0]).astype(dtype)
        alpha = np.exp(e - e.max())
        alpha = (alpha / alpha.sum(dtype=dtype)).astype(dtype)
        u = (alpha[:, None] * z).sum(0, dtype=dtype)
        score = dtype(u @ w[MEAN + "weight"][0] + w[MEAN + "bias"][0])
    else:
        alpha = np.full(F, 1.0 / F, dtype)
        score = dtype(mu.mean(dtype=dtype))
    if clipping:
        score = dtype(dtype(2.0) * np.tanh(score) + dtype(3.0))
    return score, mu, alpha


def mos_fold_numpy(weights):
    """fp64: s = softmax(weights), v_e = C^T a, v_m = C^T m, k_e = a . c + a0, k_m = m . c + m0 (v_e and k_e are 0 without attention)."""
    w = {k: np.asarray(v).astype(np.float64) for k, v in weights.items()}
    fw = w["featurizer.weights"]
    s = np.exp(fw - fw.max())
    s /= s.sum()
    C, c = w["connector.weight"], w["connector.bias"]
    m, m0 = w[MEAN + "weight"][0], w[MEAN + "bias"][0]
    if ATT + "weight" in w:
        a, a0 = w[ATT + "weight"][0], w[ATT + "bias"][0]
        v_e, k_e = C.T @ a, a @ c + a0
    else:
        v_e, k_e = np.zeros(C.shape[1]), 0.0
    return s, v_e, C.T @ m, float(k_e), float(m @ c + m0)


def mos_folded_numpy(weights, hs, clipping=False):
    """The score from the folded form in fp64: what the library computes, in exact-enough arithmetic."""
    s, v_e, v_m, k_e, k_m = mos_fold_numpy(weights)
    hh = (s[:, None, None] * np.asarray(hs, np.float64)).sum(0)
    e, mu = hh @ v_e + k_e, hh @ v_m + k_m
    alpha = np.exp(e - e.max())
    alpha /= alpha.sum()
    score = float((alpha * mu).sum())
    return (2.0 * np.tanh(score) + 3.0 if clipping else score), mu, alpha


def synthetic_mos_weights(n_states, H, P, seed=0, attention=True):
    """Seeded head weights under `MOSHead`'s keys (fp32 tensors): layer weights spread enough that the mix is not uniform, projections of
    scale 1 / sqrt(fan-in), so that e and mu are of order 1 on hidden states of order 1."""
    g = np.random.Generator(np.random.Philox(key=4200 + int(seed)))

    def t(shape, scale):
        return torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32))

    w = {"featurizer.weights": t((n_states,), 1.0), "connector.weight": t((P, H), H ** -0.5), "connector.bias": t((P,), 0.1)}
    if attention:
        w[ATT + "weight"], w[ATT + "bias"] = t((1, P), 2.0 * P ** -0.5), t((1,), 0.1)
    w[MEAN + "weight"], w[MEAN + "bias"] = t((1, P), P ** -0.5), t((1,), 0.1)
    return w
