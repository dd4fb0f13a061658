"""The decoder's training backward, every gradient ELEMENT BY ELEMENT against the fp64 oracle, at the shapes T = 176 does not reach.

Every older comparison of a full-width parameter gradient with a reference runs at T = 176 (level widths 176 / 88 / 44 / 22) and judges a
tensor by its L2 norm or by an odd-strided sample (tests/test_decoder_grads.py plants what those let through).  Here: `loss_t` of the
full-size model through the public module, `.backward()`, and all 228 estimator gradients plus grad_x0 / grad_cond / grad_spk_emb WHOLE against
`oracle.decoder_oracle.loss_t` under torch autograd on the CPU in fp64, the same in fp32 giving the floor:

    max |library - fp64| <= max(10 x max |fp32 oracle - fp64|, 1e-5 x max |fp64|)        (tools/grad_parity.py)

and for the eight one-element Rezero gains the larger of that and 1e-4 of the gain's own magnitude.  A miss lists every failing tensor in
the order the backward produces them: the first names the kernel.

Cases (tools/grad_parity.py CASES; which weight-gradient variant each reaches: DESIGN.md section 26): T = 8 alone, with a shorter and with a
fully padded item; T = 16 (level-0 width on the switch between the two f16x3 weight-gradient kernels); T = 24, B = 3 with a one-frame item;
T = 40 (odd width 5 at level 3); T = 128 (level-3 width 16); T = 136 (17, partial Winograd tiles); [8, 5] and [24, 17, 1] once more with every
Rezero gain 1.  Both the default (f16x3) and the exact-fp32 handle in every case; at [8] and [24, 17, 1] also a NaN-filled gradient blob and
the one-stream backward, each against the fp64 reference.

The oracle's gradients of a case are computed once and shared by all runs of that case (the parametrisation keeps a case's runs together, so
the cache holds one case at a time: a full set of fp64 gradients is 1 GB)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from unitspeech_amd import UnitSpeech

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import grad_parity as GP      # noqa: E402

pytestmark = pytest.mark.gpu

FULL = GP.FULL
DEV = "cuda:0"
SIDE_CASES = ("T8_8", "T24_24_17_1")            # the NaN-filled blob and the one-stream backward
RUNS = [(c, v) for c in GP.CASES for v in ("f16x3", "exact") + (("nan_blob", "one_stream") if c in SIDE_CASES else ())]

_oracle = {}       # case -> (inputs, loss64, ref64, floors); one case at a time
_models = {}       # gain-one weights? -> the module (both engines behind it)


def oracle(case):
    if case not in _oracle:
        _oracle.clear()
        t0 = time.time()
        sd_np, inputs = GP.case_weights(case), GP.case_inputs(case)
        l64, r64 = GP.oracle_grads(sd_np, inputs, torch.float64)
        l32, r32 = GP.oracle_grads(sd_np, inputs, torch.float32)
        floors = GP.floors_of(r32, r64)
        del r32
        # nothing is skipped, sampled or excluded, and no tensor is compared with a bar of zero
        assert len(r64) == 228 + 3 and set(r64) == set(GP.backward_order())
        zero = [n for n, g in r64.items() if not float(g.abs().max()) > 0]
        assert not zero, zero
        assert abs(l32 - l64) <= 1e-6 * max(1.0, abs(l64))
        # the oracle itself: exactly 0 in every masked column of the two frame-shaped input gradients
        pad = (inputs[1] == 0).expand_as(r64["grad_x0"])
        for n in ("grad_x0", "grad_cond"):
            assert not bool(pad.any()) or float(r64[n][pad].abs().max()) == 0.0, n
        print(f"\n{case}: oracle fp64 + fp32 autograd on the CPU {time.time() - t0:.1f} s, loss {l64:.9f}")
        _oracle[case] = (inputs, l64, r64, floors)
    return _oracle[case]


def make_model(sd_np):
    m = UnitSpeech(FULL.n_feats, FULL.dim, list(FULL.dim_mults), FULL.beta_min, FULL.beta_max, FULL.pe_scale, FULL.spk_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    return m.to(DEV).train()


def model_of(case):
    key = GP.CASES[case][3]
    if key not in _models:
        _models[key] = make_model(GP.case_weights(case))
    return _models[key]


def library_grads(m, inputs, exact):
    """loss_t and .backward() through the public module: (loss, {name: gradient on the device})."""
    x0, mask, cond, spk, t, z = (v.to(DEV) for v in inputs)
    x0, cond, spk = (v.requires_grad_(True) for v in (x0, cond, spk))
    m.exact = exact
    for p in m.parameters():
        p.grad = None
    try:
        with GP.ReplayRandn([z]):
            loss, _ = m.loss_t(x0, mask, cond, t, spk)
        loss.backward()
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"the device reported an error, nothing more is started on it: {e}", returncode=3)
        raise
    assert m.range_status() == 0
    got = {n: p.grad.detach() for n, p in m.named_parameters() if p.grad is not None and n.startswith("estimator.")}
    got.update(grad_x0=x0.grad, grad_cond=cond.grad, grad_spk_emb=spk.grad)
    return float(loss.detach()), got


def check(case, tag, loss, got):
    inputs, l64, r64, floors = oracle(case)
    print(f"{case} {tag}: loss {loss:.9f}, fp64 oracle {l64:.9f}: off by {abs(loss - l64):.2e} (bar {2e-6 * max(1.0, abs(l64)):.2e})")
    assert abs(loss - l64) <= 2e-6 * max(1.0, abs(l64))
    assert len([n for n in got if n.startswith("estimator.")]) == 228
    rows, misses = GP.judge(got, r64, floors, tag=f"{case} {tag}")
    if case in GP.SMALL:
        # exactly 0 in every masked column of every item (the oracle's are: oracle()); [8, 0]: the padded item's rows altogether
        pad = (inputs[1] == 0).expand_as(r64["grad_x0"])
        for n in ("grad_x0", "grad_cond"):
            leak = float(got[n].cpu()[pad].abs().max()) if bool(pad.any()) else 0.0
            if leak != 0.0:
                misses.append(f"{n}: masked columns hold {leak:.3e}, not 0")
    assert not misses, f"{case} {tag}: {len(misses)} tensor(s) off the bar, in backward order:\n  " + "\n  ".join(misses)
    return rows


@pytest.mark.parametrize("case,variant", RUNS, ids=[f"{c}-{v}" for c, v in RUNS])
def test_every_gradient_element_by_element_vs_the_fp64_oracle(case, variant, monkeypatch):
    """variant f16x3 / exact: the default and the exact-fp32 handle.  nan_blob: the gradient blob of the call arrives NaN-filled (the
    `torch.empty` wrapper of test_backward_needs_no_zero_fill_for_the_convolution_weight_gradients; us_grad_is_overwritten promises an
    overwrite at every shape).  one_stream: US_WGRAD_STREAM=0, read when the handle is created.  All four against the fp64 reference."""
    inputs = oracle(case)[0]
    if variant == "one_stream":
        monkeypatch.setenv("US_WGRAD_STREAM", "0")
        m = make_model(GP.case_weights(case))
    else:
        m = model_of(case)
    t0 = time.time()
    if variant == "nan_blob":
        library_grads(m, inputs, False)
        n = m._get_engine().last_grad_blob.numel()
        orig_empty, hits = torch.empty, []

        def poisoned_empty(*a, **kw):
            out = orig_empty(*a, **kw)
            if out.dtype == torch.float32 and out.numel() == n and out.is_cuda:
                out.fill_(float("nan"))
                hits.append(1)
            return out

        torch.empty = poisoned_empty
        try:
            loss, got = library_grads(m, inputs, False)
        finally:
            torch.empty = orig_empty
        assert hits, "the backward did not allocate its blob through torch.empty: the test proves nothing"
    else:
        loss, got = library_grads(m, inputs, variant == "exact")
    dt = time.time() - t0
    check(case, variant, loss, got)
    print(f"{case} {variant}: library forward + backward {dt:.2f} s (first call of a handle: with its weight packs)")
