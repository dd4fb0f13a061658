"""From the dense upstream features to the unit sequence, on the device (csrc/units.hip).

Drop-ins with the reference's names and signatures for the three host steps of finetune.py:112-128:

  KMeansQuantizer   textless/data/kmeans_quantizer.py: scikit-learn `KMeans.predict`  -> `us_units_quantize`
  SpeechEncoder     textless/data/speech_encoder.py: dense model + quantizer + `unique_consecutive`  -> `us_units_dedup`
  process_unit      unitspeech/util.py:69-102: 50 Hz units to mel-rate (unit, duration)  -> `us_units_process`

The dense model (mHuBERT through fairseq) stays the caller's torch module.  All results are integers and exact: the units are the fp64
argmin of the squared distance over the fp32 inputs (first index on ties), whatever the fp32 GEMM rounds.  There is no CPU fallback:
a tensor that is not on a GPU raises.

The codebook itself is fitted here too (csrc/units_fit.hip; tools/kmeans_numpy.py is the fp64 statement): `KMeansQuantizer.fit`,
`KMeansQuantizer.partial_fit`, `lloyd_step`, `kmeans_plusplus`.  The assignment of every iteration is the exact `quantize` above, the
per-centre sums are fp64 in a fixed order, the means are rounded once to fp32: a fit is deterministic.  From the same initial centres
`fit` follows scikit-learn's `KMeans(init=array, n_init=1, algorithm="lloyd", tol=0)` label for label, and `partial_fit` follows
`MiniBatchKMeans.partial_fit` with `reassignment_ratio=0`.  Not scikit-learn's, so do not expect its results from its own init: the
greedy k-means++ with local trials and its RNG stream (the seeding here is plain D^2 sampling), the relocation of empty clusters (an
empty centre keeps its value), sample weights, `tol` scaled by the data's variance (`tol` here is absolute), `MiniBatchKMeans.fit`'s
sampler and early-stopping heuristics, and Elkan's algorithm.
"""
from __future__ import annotations

import warnings
from typing import Optional

import torch

from . import _lib
from ._args import call as _call, i64 as _i64, need_gpu as _need_gpu

__all__ = ["KMeansQuantizer", "SpeechEncoder", "process_unit", "process_units_batch", "dedup_units", "lloyd_step", "kmeans_plusplus"]

MAX_K, MAX_D, MAX_SPAN = 2048, 1024, 64
MAX_ROWS = 1 << 24                         # rows of one library call; more go in as a list of chunks


def _workspace(dev, B, Tmax, K, D, Lout):
    n = int(_lib.load().us_units_workspace_bytes(B, Tmax, K, D, Lout))
    if n == 0:
        raise ValueError(f"unit extraction: unsupported sizes B = {B}, T = {Tmax}, K = {K}, D = {D}, output frames = {Lout}")
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def _check_rates(sampling_rate, hop_length):
    sampling_rate, hop_length = int(sampling_rate), int(hop_length)
    if sampling_rate < 50 or hop_length < 1:
        raise ValueError(f"process_unit: sampling_rate {sampling_rate} must be at least 50 and hop_length {hop_length} at least 1")
    spf = sampling_rate // 50
    if (hop_length + spf - 2) // spf + 1 > MAX_SPAN:
        raise ValueError(f"process_unit: with sampling_rate {sampling_rate} and hop_length {hop_length} an output frame spans more than "
                         f"{MAX_SPAN} frames of the 50 Hz stream")
    return sampling_rate, hop_length, spf


def synthetic_centers(K: int, D: int, seed: int):
    """Seeded stand-in for a k-means codebook: [K, D] fp32 numpy, unit-variance entries."""
    import numpy as np
    g = np.random.Generator(np.random.Philox(key=[seed, 0x6b6d]))
    return g.standard_normal((K, D), dtype=np.float32)


def synthetic_dense(centers, T: int, seed: int, noise: float = 0.5, mean_run: float = 3.0):
    """Seeded stand-in for upstream features: a sticky unit stream (geometric run lengths of mean `mean_run`) whose frames are their
    centre plus Gaussian noise, so the rows look like real features and not like an isotropic cloud.  -> [T, D] fp32 numpy."""
    import numpy as np
    g = np.random.Generator(np.random.Philox(key=[seed, 0x6465]))
    K, D = centers.shape
    runs = g.geometric(1.0 / mean_run, size=T)
    ids = np.repeat(g.integers(0, K, size=T), runs)[:T]
    return (centers[ids] + noise * g.standard_normal((T, D), dtype=np.float32)).astype(np.float32)


class KMeansQuantizer(torch.nn.Module):
    """`KMeansQuantizer(checkpoint_path)` reads the joblib file of a scikit-learn KMeans and keeps its `cluster_centers_` (or the
    `.pt` file `save` writes); `from_centers(tensor [K, D])` takes them directly; `fit(dense, ...)` computes them on the device.
    K <= 2048, D a multiple of 4 up to 1024."""

    def __init__(self, checkpoint_path=None, *, centers=None):
        super().__init__()
        if centers is None:
            if checkpoint_path is None:
                raise ValueError("KMeansQuantizer: give checkpoint_path or use KMeansQuantizer.from_centers(tensor)")
            if str(checkpoint_path).endswith(".pt"):                      # written by `save`
                centers = torch.load(checkpoint_path, map_location="cpu")["centers"]
            else:
                centers = torch.from_numpy(self.load_kmeans_model(checkpoint_path).cluster_centers_)
        centers = torch.as_tensor(centers).detach().to(torch.float32).contiguous()
        if centers.dim() != 2:
            raise ValueError(f"KMeansQuantizer: centres must be [K, D], got {tuple(centers.shape)}")
        K, D = centers.shape
        if not 1 <= K <= MAX_K:
            raise ValueError(f"KMeansQuantizer: K = {K} centres; the library takes 1 to {MAX_K}")
        if D % 4 or not 4 <= D <= MAX_D:
            raise ValueError(f"KMeansQuantizer: D = {D}; the library takes a multiple of 4 up to {MAX_D}")
        if not bool(torch.isfinite(centers).all()):
            raise ValueError("KMeansQuantizer: the centres must be finite")
        self.register_buffer("centers", centers)
        self.register_buffer("_float_tensor", torch.tensor([0], dtype=torch.float))
        self._packed = None
        self.last_counters = None          # device int32 [2] of the last call: rows with a non-finite feature, rows decided in fp64
        self.n_iter_, self.inertia_, self.counts_, self.history_ = None, None, None, []      # set by `fit` / `partial_fit`

    @classmethod
    def from_centers(cls, centers) -> "KMeansQuantizer":
        return cls(centers=centers)

    @staticmethod
    def load_kmeans_model(checkpoint_path: str):
        import joblib
        with open(checkpoint_path, "rb") as fd, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return joblib.load(fd)

    @property
    def vocab_size(self) -> int:
        return int(self.centers.shape[0])

    @property
    def device(self):
        return self._float_tensor.device

    def _apply(self, fn, *a, **kw):
        self._packed = None
        return super()._apply(fn, *a, **kw)

    def packed(self, dev):
        """The centres in the library's operand form on `dev` (packed once per device placement)."""
        if self._packed is None or self._packed.device != dev:
            K, D = self.centers.shape
            n = int(_lib.load().us_units_packed_bytes(K, D))
            buf = torch.empty(n, dtype=torch.uint8, device=dev)
            _call(dev, "us_units_pack_centers", self.centers.to(dev), K, D, buf, n)
            self._packed = buf
        return self._packed

    def _dense(self, dense, lengths):
        _need_gpu(dense, "KMeansQuantizer", "the unit extraction")
        K, D = self.centers.shape
        if dense.dim() != 3 or dense.shape[-1] != D:
            raise ValueError(f"KMeansQuantizer: features must be [B, T, {D}], got {tuple(dense.shape)}")
        dev = dense.device
        x = dense.detach().to(torch.float32).contiguous()
        B, T = x.shape[:2]
        lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else _i64(lengths, dev)
        if lens.shape != (B,):
            raise ValueError(f"KMeansQuantizer: lengths {tuple(lens.shape)} must hold {B} values")
        return x, lens, B, T, K, D, dev

    @torch.no_grad()
    def quantize(self, dense, lengths=None):
        """dense [B, Tmax, D], lengths [B] -> units [B, Tmax] int64 (-1 at t >= lengths[b] and on rows with a non-finite feature).
        Nothing is read back; `last_counters` holds the two device counters."""
        x, lens, B, T, K, D, dev = self._dense(dense, lengths)
        units = torch.empty(B, T, dtype=torch.int64, device=dev)
        if B * T == 0:
            return units
        ws, n = _workspace(dev, B, T, K, D, 0)
        self.last_counters = torch.empty(2, dtype=torch.int32, device=dev)
        _call(dev, "us_units_quantize", x, lens, self.packed(dev), B, T, K, D, units, self.last_counters, ws, n)
        return units

    def forward(self, x):
        """x [T, D] -> units [T] int64 on x's device (`KMeans.predict`)."""
        if x.dim() != 2:
            raise ValueError(f"KMeansQuantizer: features must be [T, D], got {tuple(x.shape)}")
        return self.quantize(x.unsqueeze(0))[0]

    @torch.no_grad()
    def encode(self, dense, lengths=None, sampling_rate: int = 16000, hop_length: int = 256):
        """dense [B, Tmax, D], lengths [B] -> (unit [B, Lu] int64, duration [B, Lu] fp32, unit_lengths [B] int64) at the mel rate:
        quantize and `process_unit` in one library call, with no host synchronisation.  Lu is the largest possible frame count;
        entries beyond unit_lengths[b] are 0."""
        sampling_rate, hop_length, spf = _check_rates(sampling_rate, hop_length)
        x, lens, B, T, K, D, dev = self._dense(dense, lengths)
        Lout = max(1, T * spf // hop_length)
        ws, n = _workspace(dev, B, T, K, D, Lout)
        unit = torch.empty(B, Lout, dtype=torch.int64, device=dev)
        dur = torch.empty(B, Lout, dtype=torch.int64, device=dev)
        dur_f = torch.empty(B, Lout, dtype=torch.float32, device=dev)
        n_out = torch.empty(B, dtype=torch.int64, device=dev)
        self.last_counters = torch.empty(2, dtype=torch.int32, device=dev)
        _call(dev, "us_units_encode", x, lens, self.packed(dev), B, T, K, D, sampling_rate, hop_length, unit, dur, dur_f, n_out, Lout,
              self.last_counters, ws, n)
        return unit, dur_f, n_out

    # ---- fitting the centres (csrc/units_fit.hip) ---------------------------------------------------------------------------------
    @classmethod
    @torch.no_grad()
    def fit(cls, dense, lengths=None, *, n_clusters=None, init="k-means++", max_iter=100, tol=0.0, seed=0) -> "KMeansQuantizer":
        """Lloyd's k-means on the device -> a quantiser with `n_iter_`, `inertia_`, `counts_` (device int64 [K]) and `history_` (one
        record per iteration: inertia against the centres the iteration started from, shift2, n_empty, rows_used, rows_skipped).

        dense: [B, T, D] with lengths [B], or [N, D], or a list of such tensors (with a list of lengths or None), which is accumulated
        chunk by chunk: more than 2^24 rows, or the batches of a data set, need no concatenation.  Rows beyond lengths[b] and rows with a
        non-finite feature take no part.  init: "k-means++" (plain D^2 sampling from `seed`, see `kmeans_plusplus`), "random" (K distinct
        valid rows from a seeded host permutation) or a [K, D] tensor.  The loop stops when shift2 = sum (c_new - c_old)^2 <= tol, an
        absolute bound, or at max_iter; with tol = 0 that is exactly when the labels stop changing (scikit-learn's strict convergence,
        the same `n_iter_`).  One 40-byte record per iteration is read back for that decision; nothing else leaves the device.
        `inertia_` and `counts_` belong to the final centres.  See the module docstring for what is not scikit-learn's."""
        K = None if n_clusters is None else int(n_clusters)
        if isinstance(init, str):
            if init not in ("k-means++", "random"):
                raise ValueError(f"KMeansQuantizer.fit: init must be 'k-means++', 'random' or a [K, D] tensor, got {init!r}")
            if K is None:
                raise ValueError("KMeansQuantizer.fit: n_clusters is needed unless init is a [K, D] tensor")
        else:
            init = torch.as_tensor(init)
            if init.dim() != 2 or (K is not None and init.shape[0] != K):
                raise ValueError(f"KMeansQuantizer.fit: init must be [K, D]{'' if K is None else f' with K = {K}'}, got {tuple(init.shape)}")
            K = int(init.shape[0])
            first = dense[0] if isinstance(dense, (list, tuple)) and len(dense) else dense
            if isinstance(first, torch.Tensor) and first.dim() in (2, 3) and init.shape[1] != first.shape[-1]:
                raise ValueError(f"KMeansQuantizer.fit: init must be [{K}, {first.shape[-1]}], got {tuple(init.shape)}")
        chunks, D, dev = _fit_chunks(dense, lengths, K, "KMeansQuantizer.fit")
        if int(max_iter) < 0 or not float(tol) >= 0.0:
            raise ValueError(f"KMeansQuantizer.fit: max_iter {max_iter} and tol {tol} must not be negative")
        _need_valid_rows(chunks, K, "KMeansQuantizer.fit")
        if isinstance(init, str):
            x, lens = _one_chunk(chunks)
            centers = _seed_pp(x, lens, K, seed)[0] if init == "k-means++" else _seed_random(x, lens, K, seed)
        else:
            centers = init
        q = cls.from_centers(centers.detach().clone()).to(dev)      # updated in place: never the caller's tensor
        st = _FitState(K, D, dev)
        q.history_ = []
        q.n_iter_ = 0
        counts = torch.zeros(K, dtype=torch.int64, device=dev)
        for it in range(1, int(max_iter) + 1):
            rec = q._fit_pass(chunks, st, _LLOYD, None, counts, q.centers)
            q.history_.append(rec)
            q.n_iter_ = it
            if rec["shift2"] <= float(tol):
                break
        if q.history_ and q.history_[-1]["shift2"] == 0.0:
            q.inertia_ = q.history_[-1]["inertia"]         # the centres did not move: the last pass is the final assignment
        else:
            q.inertia_ = q._fit_pass(chunks, st, _LLOYD, None, counts, torch.empty_like(q.centers))["inertia"]
        q.counts_ = counts
        return q

    def _fit_pass(self, chunks, st, mode, totals_in, totals_out, centers_out):
        """quantize + accumulate every chunk against the current centres, then one update into centers_out -> the record."""
        for x, lens in chunks:
            st.accumulate(x, self.quantize(x, lens), self.centers)
        rec = st.update(mode, self.centers, centers_out, totals_in, totals_out)
        if centers_out is self.centers:
            self._packed = None
        return rec

    @torch.no_grad()
    def partial_fit(self, dense, lengths=None) -> "KMeansQuantizer":
        """One mini-batch update in place: c_k = fp32((c_k total_k + sum_k) / (total_k + count_k)) with the running `counts_` as totals
        (zero on a quantiser that was not fitted), then counts_ += the batch's counts: scikit-learn's `MiniBatchKMeans.partial_fit` with
        `reassignment_ratio=0`.  `inertia_` is the batch's inertia against the centres before the update."""
        K, D = self.centers.shape
        chunks, _, dev = _fit_chunks(dense, lengths, K, "KMeansQuantizer.partial_fit", D=D, need_rows=False)
        if self.centers.device != dev:
            raise RuntimeError(f"KMeansQuantizer.partial_fit: the centres are on {self.centers.device}, the features on {dev}")
        if self.counts_ is None:
            self.counts_ = torch.zeros(K, dtype=torch.int64, device=dev)
        self.counts_ = self.counts_.to(dev)
        rec = self._fit_pass(chunks, _FitState(K, D, dev), _MINIBATCH, self.counts_, self.counts_, self.centers)
        self._packed = None
        self.history_ = list(self.history_) + [rec]
        self.inertia_ = rec["inertia"]
        return self

    def save(self, path) -> None:
        """A path ending in .bin or .joblib gets a joblib-saved `sklearn.cluster.KMeans` with `cluster_centers_` set, which
        `KMeansQuantizer(path)`, --kmeans_checkpoint and textless read (needs scikit-learn and joblib).  Any other path gets a torch file
        with `centers` [K, D] and the fit attributes, which `KMeansQuantizer(path)` reads when it ends in .pt and finetune.py reads as
        the `centers` of a features file."""
        path = str(path)
        centers = self.centers.detach().cpu()
        if path.endswith((".bin", ".joblib")):
            try:
                import joblib
                from sklearn.cluster import KMeans
            except ImportError as e:
                raise RuntimeError(f"KMeansQuantizer.save: {path} asks for a joblib-saved scikit-learn KMeans, which needs scikit-learn and "
                                   f"joblib ({e}); save to a .pt path instead") from e
            K, D = centers.shape
            km = KMeans(n_clusters=K, init=centers.numpy(), n_init=1, max_iter=1)
            km.cluster_centers_ = centers.numpy().copy()
            km._n_features_out = K
            km.n_features_in_ = D
            km._n_threads = 1
            km.n_iter_ = int(self.n_iter_ or 0)
            km.inertia_ = float(self.inertia_) if self.inertia_ is not None else float("nan")
            km.labels_ = None
            joblib.dump(km, path)
            return
        torch.save({"centers": centers, "n_iter": self.n_iter_, "inertia": self.inertia_,
                    "counts": None if self.counts_ is None else self.counts_.cpu(), "history": list(self.history_)}, path)


@torch.no_grad()
def dedup_units(units, lengths=None):
    """units [B, Tmax] int64 with lengths [B] -> (units, durations [B, Tmax] int64, zero padded, n [B] int64): per item
    `torch.unique_consecutive(return_counts=True)`, without a host synchronisation."""
    _need_gpu(units, "dedup_units", "the unit extraction")
    dev = units.device
    u = _i64(units, dev)
    B, T = u.shape
    lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else _i64(lengths, dev)
    out_u = torch.zeros(B, T, dtype=torch.int64, device=dev)
    out_d = torch.zeros(B, T, dtype=torch.int64, device=dev)
    n_out = torch.zeros(B, dtype=torch.int64, device=dev)
    if B * T == 0:
        return out_u, out_d, n_out
    ws, n = _workspace(dev, B, T, 0, 0, 0)
    _call(dev, "us_units_dedup", u, lens, B, T, out_u, out_d, n_out, ws, n)
    return out_u, out_d, n_out


@torch.no_grad()
def process_units_batch(units, durations, n_in, sampling_rate, hop_length, max_frames: Optional[int] = None):
    """`process_unit` for a padded batch, without a host synchronisation.  units [B, Lin] int64, durations [B, Lin] (None: all ones),
    n_in [B] valid entries per item (None: Lin).  max_frames bounds sum(durations) of every item; it sizes the outputs and is
    needed when durations are given (Lin otherwise).  Returns (unit [B, Lu] int64, duration [B, Lu] int64, duration as fp32,
    unit_lengths [B] int64); entries beyond unit_lengths[b] are 0, and unit_lengths[b] is -1 for an item with more than max_frames."""
    sampling_rate, hop_length, spf = _check_rates(sampling_rate, hop_length)
    _need_gpu(units, "process_units_batch", "the unit extraction")
    dev = units.device
    u = _i64(units, dev)
    B, Lin = u.shape
    if durations is not None and max_frames is None:
        raise ValueError("process_units_batch: max_frames (a bound on the sum of an item's durations) is needed with durations")
    fmax = Lin if max_frames is None else int(max_frames)
    d = None if durations is None else _i64(durations, dev)
    if d is not None and d.shape != u.shape:
        raise ValueError(f"process_units_batch: units {tuple(u.shape)} and durations {tuple(d.shape)} disagree")
    lens = torch.full((B,), Lin, dtype=torch.int64, device=dev) if n_in is None else _i64(n_in, dev)
    Lout = max(1, fmax * spf // hop_length)
    unit = torch.zeros(B, Lout, dtype=torch.int64, device=dev)
    dur = torch.zeros(B, Lout, dtype=torch.int64, device=dev)
    dur_f = torch.zeros(B, Lout, dtype=torch.float32, device=dev)
    n_out = torch.zeros(B, dtype=torch.int64, device=dev)
    if B * Lin == 0:
        return unit, dur, dur_f, n_out
    ws, n = _workspace(dev, B, Lin, 0, 0, Lout)
    _call(dev, "us_units_process", u, d, lens, B, Lin, sampling_rate, hop_length, unit, dur, dur_f, n_out, Lout, ws, n)
    return unit, dur, dur_f, n_out


@torch.no_grad()
def process_unit(encoded, sampling_rate, hop_length):
    """Drop-in for `unitspeech.util.process_unit`: encoded {"units", "durations"} (1-D, on the GPU) -> (unit, duration) LongTensors of
    exact length on the same device.  One count is read back, the only synchronisation when `encoded` carries the SpeechEncoder's
    "dense" [T, D] (its T bounds the output); without it the sum of the durations is read first.  An input shorter than one hop gives
    two empty tensors (the reference raises an IndexError there)."""
    units, durations = encoded["units"], encoded["durations"]
    _need_gpu(units, "process_unit", "the unit extraction")
    if units.dim() != 1 or durations.shape != units.shape:
        raise ValueError(f"process_unit: units {tuple(units.shape)} and durations {tuple(durations.shape)} must be 1-D and agree")
    dense = encoded.get("dense") if hasattr(encoded, "get") else None
    fmax = int(dense.shape[0]) if isinstance(dense, torch.Tensor) and dense.dim() == 2 else int(durations.sum())
    unit, dur, _, n_out = process_units_batch(units.unsqueeze(0), durations.unsqueeze(0), None, sampling_rate, hop_length, max_frames=max(fmax, 1))
    n = int(n_out[0])
    if n < 0:
        raise RuntimeError(f"process_unit: the durations cover more than the {fmax} frames of `dense`")
    return unit[0, :n], dur[0, :n]


# ---- codebook fit: plumbing around us_units_fit_* -----------------------------------------------------------------------------------
_LLOYD, _MINIBATCH = 0, 1
_RECORD_FIELDS = (("inertia", float), ("shift2", float), ("n_empty", int), ("rows_used", int), ("rows_skipped", int))


def _fit_chunks(dense, lengths, K, what, D=None, need_rows=True):
    """dense ([B, T, D] | [N, D] | a list of them) with lengths -> ([(x [B, T, D] fp32 contiguous, lens [B] int64)], D, device).  The
    sizes are checked first, then that everything is on one GPU."""
    many = isinstance(dense, (list, tuple))
    xs = list(dense) if many else [dense]
    ls = list(lengths) if many and lengths is not None else ([None] * len(xs) if many else [lengths])
    if not xs or len(ls) != len(xs):
        raise ValueError(f"{what}: {len(xs)} feature tensors and {len(ls)} lengths")
    total = 0
    for x in xs:
        if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
            raise ValueError(f"{what}: features must be [B, T, D] or [N, D] tensors, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        D = int(x.shape[-1]) if D is None else D
        if x.shape[-1] != D:
            raise ValueError(f"{what}: features must have D = {D}, got {tuple(x.shape)}")
        rows = x.numel() // max(D, 1)
        if rows > MAX_ROWS:
            raise ValueError(f"{what}: {rows} rows in one tensor; the library takes up to 2^24 per call: pass a list of chunks")
        total += rows
    if K is not None and not 1 <= K <= MAX_K:
        raise ValueError(f"{what}: K = {K} centres; the library takes 1 to {MAX_K}")
    if D % 4 or not 4 <= D <= MAX_D:
        raise ValueError(f"{what}: D = {D}; the library takes a multiple of 4 up to {MAX_D}")
    if need_rows and K is not None and K > total:
        raise ValueError(f"{what}: n_clusters = {K} is larger than the {total} rows")
    out, dev = [], None
    for x, l in zip(xs, ls):
        _need_gpu(x, what, "the unit extraction")
        dev = x.device if dev is None else dev
        if x.device != dev:
            raise RuntimeError(f"{what}: the chunks are on {dev} and {x.device}")
        if x.dim() == 2:
            if l is not None:
                raise ValueError(f"{what}: lengths go with [B, T, D] features; [N, D] features take None")
            x = x.unsqueeze(0)
        x = x.detach().to(torch.float32).contiguous()
        B, T = x.shape[:2]
        if B * T == 0:
            continue
        if B > 65535:
            raise ValueError(f"{what}: B = {B} items; the library takes up to 65535 per call")
        lens = torch.full((B,), T, dtype=torch.int64, device=dev) if l is None else _i64(l, dev)
        if lens.shape != (B,):
            raise ValueError(f"{what}: lengths {tuple(lens.shape)} must hold {B} values")
        out.append((x, lens))
    if not out:
        raise ValueError(f"{what}: no rows")
    return out, D, dev


def _valid_rows(x, lens):
    """[B, T] bool: the rows that take part (t < lengths[b], every feature finite)."""
    T = x.shape[1]
    return (torch.arange(T, device=x.device).unsqueeze(0) < lens.unsqueeze(1)) & torch.isfinite(x).all(dim=-1)


def _need_valid_rows(chunks, K, what):
    n = int(sum(_valid_rows(x, lens).sum() for x, lens in chunks))       # one scalar, once per fit: the refusal needs it
    if K > n:
        raise ValueError(f"{what}: n_clusters = {K} is larger than the {n} valid rows")


def _one_chunk(chunks):
    """The chunks as one (x, lens) for the seeding, which scans all rows at once: the concatenation of their valid rows."""
    if len(chunks) == 1:
        return chunks[0]
    x = torch.cat([x[_valid_rows(x, lens)] for x, lens in chunks]).unsqueeze(0)
    if x.shape[1] > MAX_ROWS:
        raise ValueError(f"the seeding scans all rows in one call and takes up to 2^24; the chunks hold {x.shape[1]}: pass init as a tensor")
    return x, torch.full((1,), x.shape[1], dtype=torch.int64, device=x.device)


class _FitState:
    """The device state accumulate calls add into, the scratch of the largest call so far, and the record buffer."""

    def __init__(self, K, D, dev):
        self.lib = _lib.load()
        self.K, self.D, self.dev = K, D, dev
        self.nstate = int(self.lib.us_units_fit_state_bytes(K, D))
        if self.nstate == 0:
            raise ValueError(f"codebook fit: unsupported sizes K = {K}, D = {D}")
        self.state = torch.zeros(self.nstate, dtype=torch.uint8, device=dev)
        self.record = torch.zeros(40, dtype=torch.uint8, device=dev)
        self.ws = None

    def workspace(self, rows):
        n = int(self.lib.us_units_fit_workspace_bytes(rows, self.K, self.D))
        if n == 0:
            raise ValueError(f"codebook fit: unsupported sizes rows = {rows}, K = {self.K}, D = {self.D}")
        if self.ws is None or self.ws.numel() < n:
            self.ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
        return self.ws

    def accumulate(self, x, labels, centers):
        rows = x.shape[0] * x.shape[1]
        ws = self.workspace(rows)
        _call(self.dev, "us_units_fit_accumulate", x, labels, centers, rows, self.K, self.D, self.state, self.nstate, ws, ws.numel())

    def update(self, mode, centers_in, centers_out, totals_in, totals_out):
        _call(self.dev, "us_units_fit_update", mode, centers_in, centers_out, totals_in, totals_out, self.K, self.D, self.state, self.nstate,
              self.record)
        import numpy as np
        raw = self.record.cpu().numpy().tobytes()                  # the one read-back of an iteration
        f, i = np.frombuffer(raw, dtype="<f8"), np.frombuffer(raw, dtype="<i8")
        return dict(inertia=float(f[0]), shift2=float(f[1]), n_empty=int(i[2]), rows_used=int(i[3]), rows_skipped=int(i[4]))


def seed_uniforms(K: int, seed: int):
    """The K doubles in [0, 1) of the seeding, from a seeded numpy Philox on the host (no device RNG)."""
    import numpy as np
    return np.random.Generator(np.random.Philox(key=[int(seed), 0x6b2b])).random(K)


def _seed_pp(x, lens, K, seed):
    dev, (B, T, D) = x.device, x.shape
    n = int(_lib.load().us_units_fit_workspace_bytes(B * T, K, D))
    if n == 0:
        raise ValueError(f"kmeans_plusplus: unsupported sizes rows = {B * T}, K = {K}, D = {D}")
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    mind = torch.empty(B * T, dtype=torch.float64, device=dev)
    centers = torch.zeros(K, D, dtype=torch.float32, device=dev)
    picked = torch.full((K,), -1, dtype=torch.int64, device=dev)
    for j, u in enumerate(seed_uniforms(K, seed)):
        _call(dev, "us_units_fit_seed_step", x, lens, B, T, K, D, j, float(u), mind, centers, picked, ws, n)
    return centers, picked


def _seed_random(x, lens, K, seed):
    import numpy as np
    rows = x.shape[0] * x.shape[1]
    perm = torch.from_numpy(np.random.Generator(np.random.Philox(key=[int(seed), 0x7270])).permutation(rows)).to(x.device)
    take = perm[_valid_rows(x, lens).reshape(-1)[perm]][:K]
    return x.reshape(rows, -1)[take].contiguous()


@torch.no_grad()
def lloyd_step(dense, lengths, centers):
    """One Lloyd iteration on the device -> (new centres [K, D] fp32, counts [K] int64, record): the exact assignment of `dense`
    ([B, T, D] with lengths, [N, D], or a list of them) to `centers`, fp64 sums in a fixed order, c_k = fp32(sum_k / count_k); a centre
    without rows keeps its value.  record: dict(inertia, shift2, n_empty, rows_used, rows_skipped), the inertia against `centers`.
    Rows beyond lengths[b] and rows with a non-finite feature are skipped and counted in rows_skipped."""
    centers = torch.as_tensor(centers)
    if centers.dim() != 2:
        raise ValueError(f"lloyd_step: centres must be [K, D], got {tuple(centers.shape)}")
    K, D = centers.shape
    chunks, _, dev = _fit_chunks(dense, lengths, K, "lloyd_step", D=D, need_rows=False)
    q = KMeansQuantizer.from_centers(centers).to(dev)
    new, counts = torch.empty_like(q.centers), torch.zeros(K, dtype=torch.int64, device=dev)
    rec = q._fit_pass(chunks, _FitState(K, D, dev), _LLOYD, None, counts, new)
    return new, counts, rec


@torch.no_grad()
def kmeans_plusplus(dense, lengths, n_clusters, seed=0):
    """Plain D^2 k-means++ seeding on the device -> (centres [K, D] fp32, row_indices [K] int64, both on the device).  Step 0 takes valid
    row floor(u_0 n_valid); step j keeps mind_i = min over the chosen centres of |x_i - c|^2 in fp64, takes its fixed-order inclusive
    cumulative sum P and picks the smallest valid i with P_i > u_j P_last, so a chosen row (mind = 0) is not chosen again; with
    P_last = 0 (fewer distinct rows than centres) it takes valid row floor(u_j n_valid).  The u_j are `seed_uniforms(K, seed)`.  Row
    indices count the rows of [B * T]; for a list of chunks they count the concatenation of the chunks' valid rows.  This is not
    scikit-learn's greedy variant with local trials, nor its RNG stream."""
    K = int(n_clusters)
    chunks, D, dev = _fit_chunks(dense, lengths, K, "kmeans_plusplus")
    _need_valid_rows(chunks, K, "kmeans_plusplus")
    x, lens = _one_chunk(chunks)
    return _seed_pp(x, lens, K, seed)


class SpeechEncoder(torch.nn.Module):
    """Drop-in for textless' SpeechEncoder with the quantisation and the run-length encoding on the device.  `dense_model` is the
    caller's torch module (waveform -> [T, D]); `quantizer_model` a `KMeansQuantizer` of this module."""

    def __init__(self, dense_model, quantizer_model, deduplicate: bool, add_bos_eos: bool = False, need_f0: bool = False,
                 f0_normalizer=None, f0_quantizer=None):
        super().__init__()
        if need_f0 or f0_normalizer is not None or f0_quantizer is not None:
            raise NotImplementedError("SpeechEncoder: the F0 stream is not part of this library (UnitSpeech does not use it): pass "
                                      "need_f0=False and no f0_normalizer / f0_quantizer")
        if not isinstance(quantizer_model, KMeansQuantizer):
            raise TypeError("SpeechEncoder: quantizer_model must be a unitspeech_amd.units.KMeansQuantizer")
        self.dense_model = dense_model
        self.quantizer_model = quantizer_model
        self.deduplicate = deduplicate
        self.add_bos_eos = add_bos_eos
        self.need_f0 = False
        self.unit_vocab_size = self.quantizer_model.vocab_size
        self.register_buffer("bos", torch.tensor([self.unit_vocab_size], dtype=torch.int))
        self.register_buffer("eos", torch.tensor([self.unit_vocab_size + 1], dtype=torch.int))
        self.register_buffer("_float_tensor", torch.tensor([0], dtype=torch.float))

    @classmethod
    def by_name(cls, *args, **kwargs):
        raise NotImplementedError("SpeechEncoder.by_name downloads pre-trained models by name, which this library does not do: build the "
                                  "dense model yourself and pass SpeechEncoder(dense_model, KMeansQuantizer(checkpoint_path), deduplicate, "
                                  "need_f0=False)")

    @property
    def device(self):
        return self._float_tensor.device

    @property
    def vocab_size(self) -> int:
        return self.quantizer_model.vocab_size

    @property
    def code_hop_size(self) -> int:
        return self.dense_model.code_hop_size

    @property
    def expected_sample_rate(self) -> int:
        return self.dense_model.expected_sample_rate

    @torch.no_grad()
    def encode_dense(self, dense, lengths=None):
        """dense [B, Tmax, D], lengths [B] -> {"units", "durations" [B, Tmax] int64, "lengths" [B] int64, "dense"}: the quantised
        (and, with deduplicate, run-length encoded, zero padded) streams of a batch, without a host synchronisation."""
        units = self.quantizer_model.quantize(dense, lengths)
        B, T = units.shape
        lens = torch.full((B,), T, dtype=torch.int64, device=units.device) if lengths is None else _i64(lengths, units.device)
        if self.deduplicate:
            units, durations, n = dedup_units(units, lens)
        else:
            valid = torch.arange(T, device=units.device).unsqueeze(0) < lens.unsqueeze(1)
            units, durations, n = torch.where(valid, units, torch.zeros_like(units)), valid.to(torch.int64), lens.clamp(0, T)
        return {"units": units, "durations": durations, "lengths": n, "dense": dense}

    @torch.no_grad()
    def forward(self, waveform, speaker=None):
        if waveform.ndim > 1:
            waveform = waveform.mean(0)
        dense = self.dense_model(waveform)
        units = self.quantizer_model(dense)
        if self.deduplicate:
            u, d, n = dedup_units(units.unsqueeze(0))
            n = int(n[0])                                   # the one read-back: the reference's outputs have the exact length
            units, durations = u[0, :n], d[0, :n]
        else:
            durations = torch.ones_like(units)
        if self.add_bos_eos:
            units = torch.cat([self.bos.to(units.device), units, self.eos.to(units.device)])
            z = torch.zeros_like(durations[0:1])
            durations = torch.cat([z, durations, z])
            z = torch.zeros_like(dense[0:1, :])
            dense = torch.cat([z, dense, z])
        return {"units": units.to(self.device), "durations": durations.to(self.device), "dense": dense}
