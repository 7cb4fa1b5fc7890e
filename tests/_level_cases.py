"""The rows tests/test_level_gpu.py measures, made once and K-weighted once by the fp64 contract of
tests/_level_ref.py, and what that contract says of them for a geometry.  Also here, from the contract alone: the check that no
block of any row lies within 0.01 LU of either gate -- a gate decision is discrete, so the cases must not sit on one -- and the
bound a measured loudness is held to.  Not product code."""
import functools
import math

import numpy as np

import _level_ref as R

FS, ROW = 24000, 72000  # the model rate; 600 samples x 120 frames
H = FS // 10
W = 4 * ((32 * FS + 999) // 1000)  # the kernel's warm-up, 3072 samples
CEILING, MAX_GAIN_DB = 10.0 ** (-1.0 / 20.0), 20.0
GUARD_LU = 0.01
# name: (valid samples the issue names, target LUFS)
ROWS = {"a": (0, -16.0), "b": (5000, -16.0), "c": (9600, -16.0), "d": (11999, -16.0), "e": (ROW, -16.0), "f": (ROW, -23.0),
        "g": (ROW, -16.0), "h": (ROW, -16.0), "impulse": (ROW, -16.0), "nan_target": (ROW, float("nan")), "nan_sample": (ROW, -20.0)}
MAIN = ("a", "b", "c", "d", "e", "f", "g", "h")
OTHER = ("impulse", "g", "nan_target", "e", "nan_sample", "b", "h", "f")  # the variants, and rows of MAIN at other places
GEOMETRIES = [(1, 0), (1, 50), (600, 0), (600, 50)]  # (samples per frame, trim): 1 gives the issue's sample counts exactly


@functools.lru_cache(maxsize=None)
def content():
    """name -> (x fp32 [ROW], y2 fp64 [ROW]): every row at capacity and its squared K-weighted samples; read-only."""
    g = np.random.default_rng(2317)
    noise = lambda rms: g.standard_normal(ROW) * rms
    t = np.arange(ROW) / FS
    rows = {}
    for name in ("a", "b", "c", "d", "e"):
        rows[name] = noise(10.0 ** (-30.0 / 20.0))  # -30 dBFS RMS
    speech = noise(0.05) * (0.65 + 0.35 * np.sin(2.0 * np.pi * 4.0 * t))  # syllable-rate envelope
    speech[:FS] = 0.0  # one second of exact zeros: the absolute gate
    rows["f"] = speech
    half = noise(0.1)
    half[ROW // 2:] *= 10.0 ** (-25.0 / 20.0)  # the relative gate drops the quiet half
    rows["g"] = half
    rows["h"] = np.zeros(ROW)
    imp = noise(10.0 ** (-50.0 / 20.0))
    imp[31337] = 1.0  # full scale: the ceiling wins, not the target
    rows["impulse"] = imp
    rows["nan_target"] = noise(0.02)
    rows["nan_sample"] = noise(0.03)
    out = {}
    for name, x in rows.items():
        x = x.astype(np.float32)
        if name == "nan_sample":
            x[20011] = np.nan
        y2 = R.k_weight(R.clean(x), FS) ** 2
        x.setflags(write=False)
        y2.setflags(write=False)
        out[name] = (x, y2)
    return out


def frames_of(name, spf, trim):
    """The frame count that gives the row the issue's sample count, or the nearest count above it that `spf` and `trim` allow."""
    n = ROWS[name][0]
    return 0 if n == 0 else min(-(-(n + trim) // spf), ROW // spf)


@functools.lru_cache(maxsize=None)
def expect(name, spf, trim):
    """-> (level fp32 [4], details) of a row at a geometry, by the contract; details = dict(n, z, passed, l, rel, L, peak)."""
    x, y2 = content()[name]
    n = R.row_samples([frames_of(name, spf, trim)], ROW // spf, spf, trim)[0]
    z = R.blocks_of(y2[:n], FS)
    L, passed, l, rel = R.gate(z)
    pk = R.peak(x[:n])
    g = R.gain(L, pk, ROWS[name][1], CEILING, MAX_GAIN_DB)
    return np.array([L, pk, g, passed.sum()], dtype=np.float32), dict(n=n, z=z, passed=passed, l=l, rel=rel, L=L, peak=float(pk))


def gate_distance(name, spf, trim):
    """The least distance in LU of any block of the row from the absolute gate and, where there is one, from the relative gate."""
    d = expect(name, spf, trim)[1]
    l = d["l"][np.isfinite(d["l"])]
    dist = [math.inf] + list(np.abs(l - R.ABS_GATE))
    if d["rel"] > -math.inf:
        dist += list(np.abs(l[l > R.ABS_GATE] - d["rel"]))
    return min(dist)


@functools.lru_cache(maxsize=None)
def error_model():
    """(T, eps_round): what a lane's fp64 chain may be off by per unit of the row's peak.  T = sum_{m >= W} |h_K[m]|, the start
    from zero state W samples early.  eps_round: the two chains round differently once they start at different samples -- at most
    64 roundings per sample (two stages of direct form I, generously), each 2^-53 of a value of at most 4 x the peak (the shelf's
    gain is 1.6, the high pass's numerator sums three terms), amplified by the l1 gain of the high pass's recursion 1 / A_2(z)."""
    T = R.tail_sum(FS, W)
    imp = np.zeros(8000)
    imp[0] = 1.0
    ar_gain = float(np.abs(R.biquad([1.0, 0.0, 0.0], R.coefficients(FS)[1][1], list(imp))).sum())
    return T, 64 * 2.0 ** -53 * 4.0 * ar_gain


def loudness_bound_db(name, spf, trim):
    """What the device's L_b (fp32) may differ from the contract's by, in dB.  A block of mean square z is off by at most
    delta = 2 eps peak / sqrt(z) + (eps peak)^2 / z relative, eps = T + eps_round (`error_model`), and by 8 h 2^-53 for the order of
    its fp64 sums; the mean over the passing blocks by no more than the worst of them, and 10 log10(1 + delta) <= 4.343 delta.
    Then one rounding of L_b to fp32 (half an ulp) and two fp64 library calls."""
    d = expect(name, spf, trim)[1]
    if not d["passed"].any():
        return 0.0
    eps = sum(error_model()) * d["peak"]
    zmin = d["z"][d["passed"]].min()
    delta = 2.0 * eps / math.sqrt(zmin) + eps * eps / zmin + 8 * H * 2.0 ** -53
    return 4.343 * delta + abs(d["L"]) * (2.0 ** -24 + 8 * 2.0 ** -53)
