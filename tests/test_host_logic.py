"""Host-side logic of the Python mirror that needs no GPU: state_dict contract, helpers, loud failure on CPU."""
import numpy as np
import pytest
import torch

from oracle import decoder_oracle as O
from unitspeech_amd import DecoderConfig, UnitSpeech, synthetic_state_dict
from unitspeech_amd.params import param_shapes
from unitspeech_amd import util

FULL = DecoderConfig()


def test_state_dict_keys_and_shapes_match_reference_contract():
    m = UnitSpeech(80, 32, [1, 2, 4, 8], 0.05, 20.0, 1000, 256)
    cfg = DecoderConfig(dim=32)
    want = param_shapes(cfg)
    got = m.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k, v in got.items():
        assert tuple(v.shape) == tuple(want[k]), k
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, 0).items()}
    m.load_state_dict(sd, strict=True)
    assert m.nparams == sum(v.numel() for v in sd.values())


def test_full_size_key_count():
    assert len(param_shapes(FULL)) == 230


def test_helpers_match_oracle():
    lengths = torch.LongTensor([3, 7, 5])
    assert torch.equal(util.sequence_mask(lengths, 8), O.sequence_mask(lengths, 8))
    assert torch.equal(util.sequence_mask(lengths), O.sequence_mask(lengths))
    for n in (1, 8, 9, 171, 172, 176, 1023, 1024):
        assert util.fix_len_compatibility(n, 3) == O.fix_len_compatibility(n, 3)
    dur = torch.tensor([[2., 0., 3., 1.], [1., 1., 1., 1.]])
    mask = torch.ones(2, 4, 7)
    mask[1, :, 4:] = 0
    assert torch.equal(util.generate_path(dur, mask), O.generate_path(dur, mask))


def test_cpu_tensors_fail_loudly_no_fallback():
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    z = torch.zeros(1, 80, 8)
    with pytest.raises(RuntimeError, match="ROCm device|HIP"):
        m.forward(z, torch.ones(1, 1, 8), z, torch.zeros(1, 1, 8), 2, 1.0, 1.0, noise=torch.zeros(2, 1, 80, 8))


def test_fused_adam_refuses_cpu_parameters_and_unsupported_options():
    from unitspeech_amd import FusedAdam
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdam([p], lr=1e-3).step(max_norm=1)
    with pytest.raises(ValueError):
        FusedAdam([p], lr=1e-3, weight_decay=0.1)


def test_submodules_are_parameter_containers_only():
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    with pytest.raises(RuntimeError, match="fused HIP decoder"):
        m.estimator.final_block(torch.zeros(1, 16, 80, 8), torch.ones(1, 1, 1, 8))


@pytest.mark.parametrize("n", [2, 10, 50, 500])
def test_host_step_coefficients_bit_exact_vs_oracle(n):
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    got = m._step_coefficients(n)
    ref = O.step_coefficients(n, 0.05, 20.0)
    np.testing.assert_array_equal(got.numpy(), ref.numpy())


def test_f16x3_split_gemm_is_at_fp32_accuracy():
    """The arithmetic the f16x3 kernels implement (two fp16 planes per operand, three products, fp32 accumulation), emulated in NumPy:
    its error against fp64 is the fp32 sgemm's, also with operands spanning 0.01 .. 30 in magnitude."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("f16x3_emulation", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "tools", "f16x3_emulation.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for K in (128, 1152):
        e32, e16 = m.errors(K)
        assert e16 <= 1.15 * e32 and e16 <= 5e-7, (K, e32, e16)
    # the representation alone: 22 significant bits
    x = np.random.default_rng(1).standard_normal(10000).astype(np.float32) * 100
    hi, lo = m.split16(x)
    assert np.abs((hi.astype(np.float64) + lo.astype(np.float64) / 2048) - x).max() <= np.abs(x).max() * 2.0 ** -22


# ---- round 3: the range fall-back of the mirror and the bench's self-description, without a GPU -------------------------------------
class _FakeEngine:
    def __init__(self, exact, status=0, stale=0):
        self.exact, self._status, self.status_reads = exact, status, 0
        self.stale, self.clears = stale, 0          # stale: an event an earlier TRAINING call left standing in the device word

    def range_clear(self):
        self.clears += 1
        self.stale = 0

    def range_status(self, reset=True):
        self.status_reads += 1
        st = self._status | self.stale
        if reset:
            self._status = self.stale = 0
        return st


def test_run_checked_repeats_a_flagged_inference_call_on_the_exact_engine(monkeypatch):
    """`_run_checked` (unitspeech_amd/unitspeech.py): a clean status returns the default engine's result; a range event warns and
    returns the exact engine's; an exact engine is never asked for its status; `range_check=False` skips the read."""
    import warnings
    from unitspeech_amd import unitspeech as US
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    runs = []

    def run(e):
        runs.append(e)
        return ("exact" if e.exact else "fast")

    fast, exact = _FakeEngine(False, 0), _FakeEngine(True)
    assert US._run_checked(fast, run, lambda: exact, True, "t") == "fast" and runs == [fast] and fast.status_reads == 1
    runs.clear()
    # an event left by the last training iteration must not send an in-range inference call to the exact engine
    fast = _FakeEngine(False, 0, stale=1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert US._run_checked(fast, run, lambda: exact, True, "t") == "fast" and runs == [fast] and fast.clears == 1
    runs.clear()
    fast = _FakeEngine(False, 1)
    with pytest.warns(RuntimeWarning, match="exact-fp32"):
        assert US._run_checked(fast, run, lambda: exact, True, "t") == "exact"
    assert runs == [fast, exact]
    runs.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert US._run_checked(exact, run, lambda: exact, True, "t") == "exact" and exact.status_reads == 0
        fast = _FakeEngine(False, 1)
        assert US._run_checked(fast, run, lambda: exact, False, "t") == "fast" and fast.status_reads == 0     # check switched off


def test_model_exposes_exact_and_range_check_switches(monkeypatch):
    monkeypatch.setenv("UNITSPEECH_EXACT", "1")
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    assert m.exact is True and m.range_check is True and m.estimator._flags() == (True, True)
    monkeypatch.delenv("UNITSPEECH_EXACT")
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    assert m.exact is False and m.range_status() == 0            # no engine yet: nothing to report
    m.exact = True
    assert m.estimator._flags() == (True, True)


def test_fine_tune_segment_refuses_lengths_beyond_the_mel(monkeypatch):
    """an inconsistent y_lengths must raise before the kernel sees it (the reference's slicing would raise a shape error)."""
    m = UnitSpeech(80, 16, [1, 2], 0.05, 20.0, 1000, 8)
    y = torch.zeros(1, 80, 40)
    with pytest.raises(ValueError, match="y_lengths"):
        m.fine_tune_segment(torch.zeros(1, 80, 10), y, torch.LongTensor([41]), torch.zeros(1, 10, 40), 16, 80)
    with pytest.raises(ValueError, match="y_lengths"):
        m.fine_tune_segment(torch.zeros(1, 80, 10), y, torch.LongTensor([0]), torch.zeros(1, 10, 40), 16, 80)


def test_bench_algorithmic_bytes_and_single_rank_census():
    import bench
    n = sum(int(np.prod(s)) for s in param_shapes(FULL).values())
    assert n == 119145177
    assert bench.algorithmic_bytes_per_eval(n, 3, 1024) == 4.0 * n + 3 * 1024 * 964.0          # weights once + B' T 964 B
    world, ranks = bench.rank_census(None, 0, 1, torch.device("cpu"), "nccl")
    assert world == 1 and ranks[0]["rank"] == 0


def test_winograd_4_wide_coefficients_are_exact_and_better_conditioned_than_the_standard_points(tmp_path):
    """csrc/wino4_coef.h is what tools/gen_wino4_coef.py writes (Cook-Toom on {0, +-5/8, +-3/2, inf}; the generator checks the convolution identity
    in exact rational arithmetic), and the fp32-pipeline emulation of tools/scratch/wino_points.py puts these points well below the standard
    {0, +-1, +-2}: the reason F(4x4,3x3) fits the 2e-6 per-evaluation bar."""
    import importlib.util
    import os
    import re
    from fractions import Fraction as Fr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    gen = load(os.path.join(root, "tools", "gen_wino4_coef.py"), "gen_wino4_coef")
    AT, Gm, BT = gen.cook_toom_exact([0, Fr(5, 8), Fr(-5, 8), Fr(3, 2), Fr(-3, 2)], 4)
    assert all(gen.is_dyadic(x) for row in AT + BT for x in row)              # exact in fp32
    header = open(os.path.join(root, "unitspeech_amd", "csrc", "wino4_coef.h")).read()
    bt4 = re.search(r"kBT4\[6\]\[6\] = \{(.*?)\};", header, re.S).group(1)
    vals = [float(v.rstrip("f")) for v in re.findall(r"-?\d+\.\d+f", bt4)]
    assert vals == [float(x) for row in BT for x in row]
    pts = load(os.path.join(root, "tools", "scratch", "wino_points.py"), "wino_points")
    ours = [0, Fr(5, 8), Fr(-5, 8), Fr(3, 2), Fr(-3, 2)]
    e_ours = pts.emulate(4, 4, ours, ours, C=128, Co=16, tiles=12, bias_mean=0.3)[0]
    e_std = pts.emulate(4, 4, [0, 1, -1, 2, -2], [0, 1, -1, 2, -2], C=128, Co=16, tiles=12, bias_mean=0.3)[0]
    e_22 = pts.emulate(2, 2, [0, 1, -1], [0, 1, -1], C=128, Co=16, tiles=12, bias_mean=0.3)[0]
    assert e_ours < 0.7 * e_std and e_ours < 4.0 * e_22 and e_ours < 8e-7, (e_ours, e_std, e_22)


def test_bench_refuses_counter_figures_collected_on_another_tree(monkeypatch):
    """VERDICT r3 (weak 8): `roofline.traffic` is a committed constant of the tree it was measured on.  The PMC summary carries a fingerprint of the
    inference kernels' sources; bench.py hands the figures out only while the tree it runs from has the same one, and says `"stale": true`
    (keeping the refused values visible) otherwise."""
    import bench
    from unitspeech_amd import _build
    per_launch, per_eval, src = bench.pmc_traffic()
    assert src is not None and src["file"].startswith("profiles/r04_pmc_summary")
    if src["stale"]:                                   # (a tree edited after the last collection: the refusal is what must hold)
        assert per_launch is None and per_eval is None and "stale_values" in src
    else:
        assert per_launch > 1e8 and per_eval > 1e10 and src["source_sha256"] == src["tree_sha256"]
    monkeypatch.setattr(_build, "source_fingerprint", lambda names: "0" * 16)
    per_launch, per_eval, src = bench.pmc_traffic()
    assert per_launch is None and per_eval is None and src["stale"] is True and src["stale_values"]["all_kernels_per_eval"] > 1e10


def test_an_up_to_date_library_is_used_without_writing_to_the_tree(tmp_path, monkeypatch):
    """The tree may be read-only to the account that runs it (built by another): a library newer than every source and header is
    returned without creating build/ or its lock; a newer source still goes through the locked rebuild."""
    import os
    from unitspeech_amd import _build
    csrc = tmp_path / "pkg" / "csrc"
    csrc.mkdir(parents=True)
    for name in ("a.hip", "k.h"):
        (csrc / name).write_text("//\n")
    lib = tmp_path / "pkg" / "lib.so"
    lib.write_bytes(b"")
    os.utime(csrc / "a.hip", (1000, 1000))
    os.utime(csrc / "k.h", (1000, 1000))
    os.utime(lib, (2000, 2000))
    monkeypatch.setattr(_build, "HERE", str(tmp_path / "pkg"))
    monkeypatch.setattr(_build, "CSRC", str(csrc))
    monkeypatch.setattr(_build, "LIB", str(lib))
    monkeypatch.setattr(_build, "SOURCES", ["a.hip"])
    monkeypatch.setattr(_build, "HEADERS", ["k.h"])
    rebuilt = []
    monkeypatch.setattr(_build, "_build_locked", lambda force, verbose: rebuilt.append(force) or str(lib))
    assert _build.build_library() == str(lib)
    assert rebuilt == [] and not (tmp_path / "pkg" / "build").exists()
    os.utime(csrc / "k.h", (3000, 3000))
    assert _build.build_library() == str(lib) and rebuilt == [False]
    assert _build.build_library(force=True) == str(lib) and rebuilt == [False, True]
    assert os.stat(tmp_path / "pkg" / "build" / ".lock").st_mode & 0o777 == 0o666


def test_the_three_handle_modules_share_one_base():
    """Encoder / DurationPredictor, BigVGAN and ECAPA_TDNN push their weights and report library errors through the one HandleModule."""
    from unitspeech_amd._handle import HandleModule
    from unitspeech_amd.encoder import DurationPredictor, Encoder
    from unitspeech_amd.speaker_encoder import ECAPA_TDNN
    from unitspeech_amd.vocoder import BigVGAN
    voc = {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": 4, "resblock_kernel_sizes": [3],
           "resblock_dilation_sizes": [[1, 3, 5]], "activation": "snake", "snake_logscale": False, "num_mels": 4}
    modules = [Encoder(20, 8, 16, 32, 2, 1, 3, 0.1, window_size=4), DurationPredictor(16, 24, 3, 0.1, spk_emb_dim=12), BigVGAN(voc),
               ECAPA_TDNN(feat_dim=8, channels=8, emb_dim=4)]
    assert sorted({m._abi for m in modules}) == ["frontend", "speaker", "vocoder"]
    for m in modules:
        assert isinstance(m, HandleModule)
        for f in ("_sync", "_check", "_close", "_workspace", "__del__"):
            assert getattr(type(m), f) is getattr(HandleModule, f), (type(m).__name__, f)
        with pytest.raises(RuntimeError, match=f"the HIP {m._what} needs tensors on a ROCm device"):
            m.eval()._sync(torch.device("cpu"))



@pytest.mark.parametrize("lengths", [[3, 5, 7], np.array([3, 5, 7], dtype=np.int64), torch.tensor([3, 5, 7], dtype=torch.int32),
                                     torch.tensor([[3], [5], [7]])], ids=["list", "np_int64", "int32_tensor", "Bx1_tensor"])
def test_host_lengths_takes_lists_arrays_and_tensors_of_any_shape(lengths):
    import ctypes
    from unitspeech_amd._args import c_lengths, host_lengths
    for strict in (False, True):
        v = host_lengths(lengths, 3, "X.forward", integers_only=strict)
        assert v == [3, 5, 7] and all(type(n) is int for n in v)
    assert list(c_lengths(v)) == [3, 5, 7] and c_lengths(v)._type_ is ctypes.c_int64
    assert host_lengths(None, 3, "X.forward") is None and c_lengths(None) is None


def test_host_lengths_refuses_a_wrong_count_both_ways():
    from unitspeech_amd._args import host_lengths
    with pytest.raises(ValueError) as e:
        host_lengths([3, 5], 3, "X.forward")
    assert str(e.value) == "X.forward: 2 lengths for 3 items (item 2 has none)"
    with pytest.raises(ValueError) as e:
        host_lengths(torch.tensor([3, 5, 7, 9]), 3, "X.forward")
    assert str(e.value) == "X.forward: 4 lengths for 3 items"


def test_host_lengths_integers_only_is_the_vocoders_refusal():
    from unitspeech_amd._args import host_lengths
    with pytest.raises(ValueError) as e:
        host_lengths(torch.tensor([3.0, 5.5]), 2, "BigVGAN.forward", integers_only=True)
    assert str(e.value) == "BigVGAN.forward: lengths must be integers, got dtype torch.float32"
    with pytest.raises(ValueError) as e:
        host_lengths([3, True], 2, "BigVGAN.forward", integers_only=True)
    assert str(e.value) == "BigVGAN.forward: lengths must be integers, item 1 has True"
    with pytest.raises(ValueError) as e:
        host_lengths([2.0, 3], 2, "BigVGAN.forward", integers_only=True)
    assert str(e.value) == "BigVGAN.forward: lengths must be integers, item 0 has 2.0"
    assert host_lengths(torch.tensor([3.0, 5.5]), 2, "Resample") == [3, 5]          # without the flag: int(), as every other wrapper had it


def test_device_lengths_of_none_is_none():
    from unitspeech_amd._args import device_lengths
    assert device_lengths(None, 3, torch.device("cpu"), "X") is None


@pytest.mark.parametrize("name", ["HubertModel", "WavLMModel"])
def test_waveform_encoders_refuse_training_mode_under_their_own_name(name):
    from unitspeech_amd._wav_encoder import _WaveformEncoder
    from unitspeech_amd.hubert import HubertModel
    from unitspeech_amd.wavlm import WavLMModel
    cls = {"HubertModel": HubertModel, "WavLMModel": WavLMModel}[name]
    m = cls(hidden_size=8, num_hidden_layers=1, num_attention_heads=2, intermediate_size=16, conv_dim=(4, 4), conv_kernel=(4, 2),
            conv_stride=(2, 2), num_conv_pos_embeddings=4, num_conv_pos_embedding_groups=2, num_buckets=8)
    assert type(m)._precondition is _WaveformEncoder._precondition and not issubclass(WavLMModel, HubertModel)
    m.eval()._precondition()
    with pytest.raises(RuntimeError) as e:
        m.train()._precondition()
    assert str(e.value) == f"{name} is inference-only (dropout, time masking and the backward pass are not built): call .eval()"
