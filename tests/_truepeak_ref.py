"""The contract of `st2_wave_level_ex` (include/st2.h) in plain numpy and fp64: the true peak of a row -- the
larger of its sample peak and the peak of the row interpolated U times by the polyphase sum of tests/_resample_ref.py with D = 1
-- and the level of a GROUP of rows measured as one programme (BS.1770-4's gates over the concatenated block lists of the
group's rows).  Written from the header, not from the kernel; everything about a single row's loudness is tests/_level_ref.py's.
Not product code."""
import math

import numpy as np

import _level_ref as R
import _resample_ref as RR

UP = 8  # 192 000 / 24 000: Annex 2's oversampled rate


def table():
    """-> (U, K, taps fp32 [U, K]): the package's design at 8 / 1."""
    from styletts2_amd import resample
    U, D, taps = resample._kaiser_table(UP, 1)
    assert (U, D) == (UP, 1)
    return U, taps.shape[1], taps


def clean32(x):
    """The row as the measurement stages it: fp32, a non-finite sample as 0."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


def interpolate(x, taps, chunk=8192):
    """x: a row's valid samples -> (y, bound) fp64 [U n]: `_resample_ref.polyphase` with D = 1 over the cleaned row, x = 0 outside
    it.  Made chunk by chunk (the function's K-wide product of a whole row is large): a chunk of positions is handed over with
    K samples of the row on either side, and the outputs of those extra positions -- the only ones its zero padding can touch --
    are dropped."""
    U, K = taps.shape
    x = clean32(x)
    n = len(x)
    ys, bs = [], []
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        lo, hi = max(0, a - K), min(n, b + K)
        y, bound = RR.polyphase(x[lo:hi], hi - lo, taps, U, 1)
        ys.append(y[(a - lo) * U:(b - lo) * U])
        bs.append(bound[(a - lo) * U:(b - lo) * U])
    return (np.concatenate(ys), np.concatenate(bs)) if ys else (np.zeros(0), np.zeros(0))


def true_peak(x, taps):
    """-> (tp, lo, hi): tp = max(sample peak, max |y|) in fp64, and the interval an fp32 fmaf evaluation of every y may report:
    [max(|y| - bound), max(|y| + bound)], joined with the sample peak, which is exact.  0 for an empty or all-zero row."""
    pk = float(R.peak(x))
    y, bound = interpolate(x, taps)
    if len(y) == 0:
        return pk, pk, pk
    a = np.abs(y)
    return max(pk, float(a.max())), max(pk, float((a - bound).max())), max(pk, float((a + bound).max()))


def deviation(taps, f_lo=0.0, f_hi=0.85, points=2049):
    """The passband ripple of the table as an interpolator: the largest |H_p(w) e^{-j w p / U} - 1| over every phase p and the
    frequencies w in [f_lo, f_hi] x Nyquist, H_p(w) = sum_k taps[p][k] e^{j w (k - (K - 1) // 2)}.  A steady sine in that band
    comes out of every phase within this fraction of its amplitude of the sine itself, delayed by p / U."""
    U, K = taps.shape
    w = np.pi * np.linspace(f_lo, f_hi, points)
    t = np.arange(K)[None, :] - (K - 1) // 2 - np.arange(U)[:, None] / U  # [U, K]: where tap k of phase p sits
    H = (taps.astype(np.float64)[:, :, None] * np.exp(1j * w[None, None, :] * t[:, :, None])).sum(axis=1)
    return float(np.abs(H - 1.0).max())


def groups(start, B):
    """-> [(first row, one past the last)]: a group is a flagged row and the unflagged rows behind it; row 0 begins one whatever
    its flag.  start None: every row its own group."""
    if start is None:
        return [(b, b + 1) for b in range(B)]
    first = [b for b in range(B) if b == 0 or int(start[b]) != 0]
    return [(a, e) for a, e in zip(first, first[1:] + [B])]


def level_group(zs, peaks, target, ceiling, max_gain_db):
    """The rows of one group: zs their block lists (fp64, row order), peaks their peaks (sample or true) -> (the four fp32 values
    every row of the group carries, (z, passed, l, rel, L) of the group's one list)."""
    z = np.concatenate([np.asarray(v, dtype=np.float64) for v in zs]) if zs else np.zeros(0)
    L, passed, l, rel = R.gate(z)
    pk = np.float32(max([np.float32(p) for p in peaks], default=np.float32(0.0)))
    g = R.gain(L, pk, target, ceiling, max_gain_db)
    return np.array([L, pk, g, passed.sum()], dtype=np.float32), (z, passed, l, rel, L)


def binding_terms(L, pk, target, ceiling, max_gain_db):
    """The three terms of the gain's minimum (target, limit, ceiling), inf where one does not apply; all inf where g is 1."""
    if math.isnan(float(target)) or L == -math.inf or float(pk) == 0.0:
        return [math.inf] * 3
    return [10.0 ** ((float(np.float32(target)) - L) / 20.0), 10.0 ** (max_gain_db / 20.0), ceiling / float(pk)]
