"""The MOS predictor without a GPU: the restatement against the goldens, the fold, the loader, the command line and the ABI's declarations
(tools/mos_torch.py, tools/make_goldens_mos.py, unitspeech_amd/mos.py, evaluate.py, include/unitspeech_hip.h)."""
import argparse
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mos_torch as M  # noqa: E402
from make_goldens_mos import conditions  # noqa: E402

from unitspeech_amd import _lib, mos  # noqa: E402
from unitspeech_amd.hubert import from_fairseq_wav2vec2_state_dict  # noqa: E402

ABI = ("us_mos_packed_bytes", "us_mos_pack_head", "us_mos_unpack_head", "us_mos_workspace_bytes", "us_mos_score")


def head_weights(g):
    return {k[2:]: g[k] for k in g if k.startswith("h:")}


@pytest.mark.parametrize("name", ["mos_a", "mos_b"])
def test_restatement_reproduces_the_golden(golden, name):
    g = golden(name)
    m = M.MosTorch(head_weights(g), torch.float64)
    cfg = json.loads(str(g["config"]))
    up = {k[2:]: torch.from_numpy(g[k]) for k in g if k.startswith("w:")}
    for i in range(int(g["n_items"])):
        hs = g[f"hs_{i}"]
        r = m.head(hs)
        for k in ("e", "mu", "alpha"):
            assert np.abs(r[k].numpy() - g[f"{k}_{i}"]).max() <= 1e-12, (name, i, k)
        got = [float(m.head(hs, clipping=c, attention=a)["score"]) for a in (True, False) for c in (False, True)]
        assert np.abs(np.array(got) - g["scores"][i]).max() <= 1e-12, (name, i)
        for a in (True, False):
            for c in (False, True):
                s, mu, alpha = M.mos_head_numpy(head_weights(g), hs, np.float64, a, c)
                assert abs(s - g["scores"][i][2 * (not a) + c]) <= 1e-12 and np.abs(mu - g[f"mu_{i}"]).max() <= 1e-12
        # the whole predictor: tools/hubert_torch.py in front, on the waveform
        assert abs(float(m.predict(up, cfg, g[f"wav_{i}"])) - g["scores"][i][0]) <= 1e-12
        assert abs(float(m.predict(up, cfg, g[f"wav_{i}"], True, False)) - g["scores"][i][3]) <= 1e-12


def test_folded_form_equals_the_unfolded_one():
    n, H, P, F = 13, 768, 256, 37
    w = M.synthetic_mos_weights(n, H, P, seed=5)
    hs = np.random.Generator(np.random.Philox(key=77)).standard_normal((n, F, H))
    for clipping in (False, True):
        s, mu, alpha = M.mos_head_numpy(w, hs, np.float64, True, clipping)
        fs, fmu, falpha = M.mos_folded_numpy(w, hs, clipping)
        assert abs(s - fs) <= 1e-12 and np.abs(mu - fmu).max() <= 1e-12 and np.abs(alpha - falpha).max() <= 1e-12
    # the mean variant is the plain mean of mu
    wm = {k: v for k, v in w.items() if not k.startswith(M.ATT)}
    s, mu, alpha = M.mos_head_numpy(wm, hs, np.float64)
    _, v_e, v_m, k_e, k_m = M.mos_fold_numpy(wm)
    hh = (M.mos_fold_numpy(wm)[0][:, None, None] * hs).sum(0)
    assert not v_e.any() and k_e == 0.0 and abs(s - (hh @ v_m + k_m).mean()) <= 1e-12 and np.abs(alpha - 1.0 / F).max() == 0.0


@pytest.mark.parametrize("name", ["mos_a", "mos_b"])
def test_committed_goldens_meet_the_writing_conditions(golden, name):
    g = golden(name)
    last = int(g["n_items"]) - 1
    assert g[f"hs_{last}"].shape[1] == 18 and [g[f"hs_{i}"].shape[1] for i in range(last + 1)] == [1, 2, 5, 18]
    fw = g["h:featurizer.weights"].astype(np.float64)
    s = np.exp(fw - fw.max())
    s /= s.sum()
    ok, line = conditions(g[f"alpha_{last}"], s, g["scores"])
    assert ok, line
    top = g[f"alpha_{last}"].max()
    assert 2.0 / 18 <= top <= 0.9 and s.max() / s.min() >= 3.0
    assert (np.abs(g["scores"][:, [0, 2]]) < 1.5).all() and (np.abs(g["scores"][:, 0] - g["scores"][:, 2]) >= 0.05).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20)


# ---- the loader ------------------------------------------------------------------------------------------------------------------------

def checkpoint(tmp_path, n=3, H=40, P=16, attention=True, args=None, config=None, extra_down=None, extra_feat=None):
    w = M.synthetic_mos_weights(n, H, P, seed=1, attention=attention)
    feat = {"weights": w.pop("featurizer.weights"), **(extra_feat or {})}
    ck = {"Featurizer": feat, "Downstream": {**w, **(extra_down or {})}}
    if args is not None:
        ck["Args"] = args
    if config is not None:
        ck["Config"] = config
    path = str(tmp_path / "mos.ckpt")
    torch.save(ck, path)
    return path, {**w, "featurizer.weights": feat["weights"]}


TINY = dict(conv_dim=[24] * 7, hidden_size=40, num_attention_heads=2, intermediate_size=72, num_hidden_layers=2, num_conv_pos_embeddings=16,
            num_conv_pos_embedding_groups=4)


def test_loader_reads_shapes_and_ignores_the_judge_branch(tmp_path):
    judge = {"model.bias_net_linear.weight": torch.zeros(1, 16), "model.judge_embedding.weight": torch.zeros(5, 16)}
    path, w = checkpoint(tmp_path, extra_down=judge, config={"downstream_expert": {"modelrc": {"clipping": True}}})
    p = mos.load_mos_checkpoint(path, **TINY)
    assert isinstance(p, mos.MOSPredictor) and not p.training
    h = p.head
    assert (h.hidden_size, h.n_states, h.projector_dim, h.attention_pooling, h.clipping) == (40, 3, 16, True, True)
    sd = h.state_dict()
    assert set(sd) == set(w) and all(torch.equal(sd[k], w[k]) for k in w)
    # no pooling layer in the file: mean pooling; an object for the arguments; a keyword wins over the file
    path, _ = checkpoint(tmp_path, attention=False, args=argparse.Namespace(clipping=False, projector_dim=16))
    h = mos.load_mos_checkpoint(path, **TINY).head
    assert (h.attention_pooling, h.clipping) == (False, False) and not any("pooling" in k for k in h.state_dict())
    assert mos.load_mos_checkpoint(path, clipping=True, **TINY).head.clipping is True


def test_loader_refusals(tmp_path):
    path, _ = checkpoint(tmp_path)
    with pytest.raises(ValueError, match="clipping"):
        mos.load_mos_checkpoint(path, **TINY)
    path, _ = checkpoint(tmp_path, args={"clipping": False, "normalize": True})
    with pytest.raises(ValueError, match="normalize"):
        mos.load_mos_checkpoint(path, **TINY)
    path, _ = checkpoint(tmp_path, args={"clipping": False}, extra_feat={"layer_norm.weight": torch.ones(40)})
    with pytest.raises(ValueError, match="normalize"):
        mos.load_mos_checkpoint(path, **TINY)
    path, _ = checkpoint(tmp_path, args={"clipping": False}, extra_down={"model.something_else.weight": torch.zeros(3)})
    with pytest.raises(RuntimeError, match="something_else"):
        mos.load_mos_checkpoint(path, **TINY)
    path, _ = checkpoint(tmp_path, args={"clipping": False})
    with pytest.raises(ValueError, match="`downstream`"):
        mos.load_mos_checkpoint(path, downstream_key="downstream", **TINY)
    with pytest.raises(ValueError, match="3 states"):             # an upstream that gives 5
        mos.load_mos_checkpoint(path, **{**TINY, "num_hidden_layers": 4})
    for bad in (dict(hidden_size=6), dict(hidden_size=1028), dict(n_states=33), dict(projector_dim=4097)):
        with pytest.raises(ValueError):
            mos.MOSHead(**{**dict(hidden_size=40, n_states=3, projector_dim=16), **bad})


def test_fairseq_wav2vec2_rename():
    t = torch.zeros(1)
    sd = {"mask_emb": t, "feature_extractor.conv_layers.0.0.weight": t, "feature_extractor.conv_layers.0.2.weight": t,
          "feature_extractor.conv_layers.0.2.bias": t, "feature_extractor.conv_layers.1.0.weight": t, "post_extract_proj.weight": t,
          "post_extract_proj.bias": t, "quantizer.vars": t, "quantizer.weight_proj.weight": t, "quantizer.weight_proj.bias": t,
          "project_q.weight": t, "project_q.bias": t, "encoder.pos_conv.0.bias": t, "encoder.pos_conv.0.weight_g": t,
          "encoder.pos_conv.0.weight_v": t, "encoder.layers.0.self_attn.k_proj.weight": t, "encoder.layers.0.self_attn.out_proj.bias": t,
          "encoder.layers.0.self_attn_layer_norm.weight": t, "encoder.layers.0.fc1.weight": t, "encoder.layers.0.fc2.bias": t,
          "encoder.layers.0.final_layer_norm.bias": t, "encoder.layer_norm.weight": t, "layer_norm.weight": t, "layer_norm.bias": t,
          "final_proj.weight": t, "final_proj.bias": t}
    out = from_fairseq_wav2vec2_state_dict(sd)
    assert list(out) == ["feature_extractor.conv_layers.0.conv.weight", "feature_extractor.conv_layers.0.layer_norm.weight",
                         "feature_extractor.conv_layers.0.layer_norm.bias", "feature_extractor.conv_layers.1.conv.weight",
                         "feature_projection.projection.weight", "feature_projection.projection.bias", "encoder.pos_conv_embed.conv.bias",
                         "encoder.pos_conv_embed.conv.weight_g", "encoder.pos_conv_embed.conv.weight_v",
                         "encoder.layers.0.attention.k_proj.weight", "encoder.layers.0.attention.out_proj.bias",
                         "encoder.layers.0.layer_norm.weight", "encoder.layers.0.feed_forward.intermediate_dense.weight",
                         "encoder.layers.0.feed_forward.output_dense.bias", "encoder.layers.0.final_layer_norm.bias", "encoder.layer_norm.weight",
                         "feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias"]
    with pytest.raises(ValueError, match="target_glu"):
        from_fairseq_wav2vec2_state_dict({**sd, "target_glu.0.weight": t})


# ---- the command line and the ABI -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv,needle", [(["--mos"], "--mos_path"), (["--synthetic", "2", "--mos_upstream", "x.pt"], "--mos_path"),
                                         (["--synthetic", "2", "--mos_clipping", "1"], "--mos_path")])
def test_evaluate_argument_checks(argv, needle):
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(argv)
    assert needle in str(e.value)


def test_header_declares_and_the_binding_lists_the_calls():
    with open(os.path.join(ROOT, "include", "unitspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ABI:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES
    assert sorted(set(re.findall(r"\bus_mos_\w+(?=\()", header))) == sorted(ABI)
    assert "QUIET NaN" in header                     # the zero-length item's score is stated there
    from unitspeech_amd import _build
    assert "mos.hip" in _build.SOURCES
    import unitspeech_amd
    assert all(hasattr(unitspeech_amd, n) and n in unitspeech_amd.__all__ for n in ("MOSHead", "MOSPredictor", "load_mos_checkpoint"))
