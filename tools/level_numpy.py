"""ITU-T P.56 method B (the "speech voltmeter") and the sv56 gain normalisation in fp64 numpy: the yardstick that unitspeech_amd.level
(csrc/level.hip) is tested against.  Nothing here touches a GPU or the library.

Samples are in units of full scale (an int16 sample s is s / 32768).  For a sample rate f:

    g = exp(-1 / (f T)), T = 0.03 s        p[k] = g p[k-1] + (1-g) |x[k]|,  q[k] = g q[k-1] + (1-g) p[k],  p = q = 0 before the item
    c[j] = 2^(j-15), j = 0..14             a[j] = #{k : k - last_j(k) <= I},  last_j(k) the last index <= k with q >= c[j] (none: not
    I = floor(0.2 f + 0.5)                 counted), which is the ITU loop with its hangover counters and its `break`
    A[j] = 10 log10(sq / a[j] + 1e-20), C[j] = 20 log10 c[j], D = A - C; the active level is A at the crossing D = M = 15.9 dB, found in
    closed form on the segment that brackets it (the ITU tool bisects the same segment).

Parity with the `sv56demo` binary is not claimed: the binary is not available to test against.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

T_ENV, HANG, MARGIN, N_THR = 0.03, 0.2, 15.9, 15
THRESHOLDS = np.array([2.0 ** (j - 15) for j in range(N_THR)], dtype=np.float64)
SILENT = -100.0

Level = namedtuple("Level", "level_db activity rms_db peak counts")


def constants(sample_rate):
    """-> (g, I): the envelope's pole and the hangover in samples."""
    f = float(sample_rate)
    if not f > 0:
        raise ValueError("the sample rate must be positive")
    return math.exp(-1.0 / (f * T_ENV)), int(math.floor(HANG * f + 0.5))


def to_full_scale(x):
    """int16 -> s / 32768 in fp64; a float array as it is, in fp64."""
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def quantize_reference(x):
    """The reference's float -> int16 route, `(x * 32767).astype(int16)`: an fp32 product truncated toward zero (held to the int16 range)."""
    v = np.asarray(x, dtype=np.float32) * np.float32(32767.0)
    return np.trunc(np.clip(v, -32768.0, 32767.0)).astype(np.int16)


def envelope(x, sample_rate):
    """-> q[0..n) in fp64, the literal sequential recurrence."""
    g, _ = constants(sample_rate)
    h = 1.0 - g
    q = np.empty(len(x), dtype=np.float64)
    p = qq = 0.0
    for k, v in enumerate(np.abs(np.asarray(x, dtype=np.float64)).tolist()):
        p = g * p + h * v
        qq = g * qq + h * p
        q[k] = qq
    return q


def activity_counts(q, hangover):
    """-> a[0..14] int64, vectorised: the distance to the last crossing by a running maximum of crossing indices."""
    n = len(q)
    k = np.arange(n, dtype=np.int64)
    a = np.zeros(N_THR, dtype=np.int64)
    for j, c in enumerate(THRESHOLDS):
        last = np.maximum.accumulate(np.where(q >= c, k, -1)) if n else k
        a[j] = int(np.count_nonzero((last >= 0) & (k - last <= hangover)))
    return a


def activity_counts_loop(q, hangover):
    """-> a[0..14]: the ITU loop as written, with hang[] starting at the hangover and the `break` at the first threshold not counted."""
    a = [0] * N_THR
    hang = [hangover] * N_THR
    for v in np.asarray(q, dtype=np.float64).tolist():
        for j in range(N_THR):
            if v >= THRESHOLDS[j]:
                a[j] += 1
                hang[j] = 0
            elif hang[j] < hangover:
                a[j] += 1
                hang[j] += 1
            else:
                break
    return np.array(a, dtype=np.int64)


def level_from_counts(sq, n, a):
    """-> (level_db, activity, rms_db) from sum x^2, the length and the 15 counts."""
    if n == 0:
        return SILENT, 0.0, SILENT
    rms_db = 10.0 * math.log10(sq / n + 1e-20)
    A = [10.0 * math.log10(sq / (float(v) if v > 0 else 1e-20) + 1e-20) for v in a]
    C = [20.0 * math.log10(c) for c in THRESHOLDS]
    D = [A[j] - C[j] for j in range(N_THR)]
    if a[0] == 0 or D[0] < MARGIN:
        return SILENT, 0.0, rms_db
    for j in range(1, N_THR):
        if D[j] <= MARGIN:
            den = D[j - 1] - D[j]
            w = (D[j - 1] - MARGIN) / den if den != 0.0 else 0.0
            level = A[j - 1] + w * (A[j] - A[j - 1])
            return level, 10.0 ** ((rms_db - level) / 10.0), rms_db
    return SILENT, 0.0, rms_db


def active_speech_level(x, sample_rate):
    """x: int16 or float samples of one item -> Level(level_db, activity, rms_db, peak, counts).  A non-finite sample: level NaN."""
    v = to_full_scale(x).reshape(-1)
    n = len(v)
    if n and not np.all(np.isfinite(v)):
        return Level(float("nan"), float("nan"), float("nan"), float("nan"), np.zeros(N_THR, dtype=np.int64))
    _, hang = constants(sample_rate)
    a = activity_counts(envelope(v, sample_rate), hang)
    sq = float(np.sum(v * v)) if n else 0.0
    level, act, rms = level_from_counts(sq, n, a)
    return Level(level, act, rms, float(np.abs(v).max()) if n else 0.0, a)


def gain_factor(level_db, ndb):
    """-> the linear gain; 1 where there is no measurable speech (-100) or the level is NaN: such an item comes back unchanged."""
    if not math.isfinite(level_db) or level_db <= SILENT:
        return 1.0
    return 10.0 ** ((float(ndb) - level_db) / 20.0)


def scaled_lsb(x, factor):
    """-> x * factor * 32768 in fp64: what the int16 output rounds."""
    return to_full_scale(x) * factor * 32768.0


def round_saturate(y):
    """fp64 -> (int16 rounded half away from zero and saturated, the number of saturated samples)."""
    r = np.where(y >= 0, np.floor(y + 0.5), np.ceil(y - 0.5))
    clipped = int(np.count_nonzero((r > 32767) | (r < -32768)))
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


def normalize(x, sample_rate, ndb=-26.0, out_int16=True):
    """-> (out, Level, factor, clipped): int16 out as above; float out = float32(float64(x) * factor), not clamped."""
    lv = active_speech_level(x, sample_rate)
    f = gain_factor(lv.level_db, ndb)
    if out_int16:
        out, clipped = round_saturate(scaled_lsb(x, f))
    else:
        out, clipped = (to_full_scale(x) * f).astype(np.float32), 0
    return out, lv, f, clipped


def sv56(x, sr, ndb):
    """The reference's `sv56(x, sr, ndb)`: int16 in, int16 of the same length out."""
    x = np.asarray(x)
    if x.dtype != np.int16:
        raise TypeError("sv56 takes int16 samples")
    return normalize(x, sr, ndb, out_int16=True)[0]


def threshold_margin(q):
    """The smallest relative distance of any q[k] to any threshold: what decides whether re-association noise can move a count."""
    q = np.asarray(q, dtype=np.float64)
    if not len(q):
        return float("inf")
    return float(min(np.min(np.abs(q - c)) / c for c in THRESHOLDS))


def tie_margin(y):
    """The smallest distance, in LSB, of any value about to be rounded to a rounding tie (k + 0.5)."""
    y = np.asarray(y, dtype=np.float64)
    if not len(y):
        return float("inf")
    fr = np.abs(y) - np.floor(np.abs(y))
    return float(np.min(np.abs(fr - 0.5)))


def burst_signal(n, sample_rate, seed, amplitudes=(0.001, 0.4, 0.02, 0.1, 0.005, 0.25), int16=True):
    """Seeded noise bursts of the given amplitudes spread over n samples, with gaps shorter and longer than the hangover: the test and
    --synthetic signal.  -> int16 (or float32 in full-scale units)."""
    g = np.random.Generator(np.random.Philox(key=7700 + int(seed)))
    x = np.zeros(n, dtype=np.float64)
    _, hang = constants(sample_rate)
    pos = int(g.integers(0, max(1, min(n, hang) // 4 + 1)))
    i = 0
    while pos < n:
        amp = amplitudes[i % len(amplitudes)]
        length = int(g.integers(max(1, hang // 2), 2 * hang + 2))
        end = min(n, pos + length)
        x[pos:end] = amp * g.uniform(-1.0, 1.0, size=end - pos)
        gap = int(g.integers(hang // 4, hang // 2 + 1)) if i % 2 == 0 else int(g.integers(hang + hang // 4, 2 * hang + 1))
        pos = end + max(1, gap)
        i += 1
    if int16:
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)
