"""The contract of `st2_wave_level` and of the gain of `st2_wave_pack_level` (include/st2.h) in plain numpy
and fp64: per-row integrated loudness by ITU-R BS.1770-4 (K-weighting, 400 ms blocks at 75 % overlap, absolute and relative
gate), sample peak, and the linear gain that brings a row to a target loudness under a peak ceiling.  Written from the
standard and the header, not from the kernel: what tests/test_level_gpu.py compares the kernel against.  Not product code."""
import math

import numpy as np

ABS_GATE, REL_GATE, OFFSET = -70.0, -10.0, -0.691
SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196, vb_exp=0.4996667741545416)
HIGHPASS = dict(f0=38.13547087602444, Q=0.5003270373238773)


def coefficients(fs):
    """-> ((b, a) of the high shelf, (b, a) of the high pass) at rate fs: the analog prototypes through the bilinear transform,
    K = tan(pi f0 / fs); a[0] = 1; the high pass's b = [1, -2, 1] is not normalised, as in the standard."""
    K = math.tan(math.pi * SHELF["f0"] / fs)
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** SHELF["vb_exp"]
    Q = SHELF["Q"]
    a0 = 1.0 + K / Q + K * K
    b1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a1 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * HIGHPASS["f0"] / fs)
    Q = HIGHPASS["Q"]
    a0 = 1.0 + K / Q + K * K
    a2 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return (b1, a1), ([1.0, -2.0, 1.0], a2)


def pole_radius(fs):
    """The larger pole radius of the cascade (the high pass's): what the kernel's warm-up length W is chosen from."""
    return max(max(abs(np.roots(a))) for _, a in coefficients(fs))


def biquad(b, a, x):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] from zero state, in fp64."""
    b0, b1, b2 = b
    _, a1, a2 = a
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for n, v in enumerate(x):
        r = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, v, y1, r
        y[n] = r
    return y


def k_weight(x, fs):
    """The two stages in cascade over fp64 samples, from zero state at x[0] -> fp64 array."""
    s1, s2 = coefficients(fs)
    return np.asarray(biquad(*s2, biquad(*s1, [float(v) for v in x])), dtype=np.float64)


def tail_sum(fs, W, span=None):
    """sum_{m >= W} |h[m]| of the cascade's impulse response h: what a chain that starts from zero state W samples early can be
    off by per unit of input peak.  (`span` samples of h are looked at; by default enough for r^span < 1e-30.)"""
    r = pole_radius(fs)
    span = int(W + math.log(1e-30) / math.log(r)) if span is None else span
    imp = np.zeros(span)
    imp[0] = 1.0
    return float(np.abs(k_weight(imp, fs)[W:]).sum())


def row_samples(frames, T_cap, spf, trim):
    """n_b = max(0, spf * clamp(frames[b], 0, T_cap) - trim): `pack_row_samples`."""
    return [max(0, spf * min(max(int(f), 0), T_cap) - trim) for f in frames]


def clean(x):
    """The valid samples as the measurement sees them: fp64, a non-finite sample counts as 0."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def blocks(x, fs):
    """x: a row's valid samples (fp32) -> z, the mean square of every gating block of the K-weighted row (fp64 [n_blocks])."""
    if fs <= 0 or fs % 10:
        raise ValueError("the hop is fs / 10 samples: fs=%r is refused" % (fs,))
    return blocks_of(k_weight(clean(x), fs) ** 2, fs)


def blocks_of(y2, fs):
    """The blocks of a row whose squared K-weighted samples are y2 (fp64 [n_b]).  The filter is causal and starts at x[0]: the y2
    of a row cut to its first n samples is y2[:n], so a test may weight a long row once and cut it where it likes."""
    h, n = fs // 10, len(y2)
    if n == 0:
        return np.zeros(0)
    if n < 4 * h:
        return np.array([y2.sum() / n])
    e = np.array([y2[j * h:(j + 1) * h].sum() for j in range(n // h)])
    return np.array([(e[k] + e[k + 1] + e[k + 2] + e[k + 3]) / (4 * h) for k in range(n // h - 3)])


def lufs(z):
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(z)


def gate(z):
    """-> (L, passed, l, rel): the integrated loudness of the blocks z, which of them passed both gates, every block's
    loudness and the relative gate (-inf where no block passed the absolute one)."""
    l = lufs(np.asarray(z, dtype=np.float64))
    absolute = l > ABS_GATE
    if not absolute.any():
        return -math.inf, absolute, l, -math.inf
    rel = float(lufs(np.mean(z[absolute]))) + REL_GATE
    passed = absolute & (l > rel)
    if not passed.any():
        return -math.inf, passed, l, rel
    return float(lufs(np.mean(z[passed]))), passed, l, rel


def peak(x):
    """max |x| over the valid, finite samples (fp32, exact); 0 for an empty row."""
    x = np.asarray(x, dtype=np.float32)
    x = np.abs(x[np.isfinite(x)])
    return np.float32(x.max()) if x.size else np.float32(0.0)


def gain(L, pk, target, ceiling, max_gain_db):
    """g = min(10^((target - L) / 20), 10^(max_gain_db / 20), ceiling / peak) in fp64, rounded once to fp32; exactly 1 for a NaN
    target, L = -inf or peak = 0."""
    target = float(np.float32(target))
    if math.isnan(target) or L == -math.inf or float(pk) == 0.0:
        return np.float32(1.0)
    return np.float32(min(10.0 ** ((target - L) / 20.0), 10.0 ** (max_gain_db / 20.0), ceiling / float(pk)))


def level_row(x, fs, target, ceiling, max_gain_db):
    """One row's valid samples -> (L, peak, gain, blocks passed) as the four fp32 values of `level[b]`, and the row's
    (z, passed, l, rel) for the tests' own bounds."""
    z = blocks(x, fs)
    L, passed, l, rel = gate(z)
    pk = peak(x)
    g = gain(L, pk, target, ceiling, max_gain_db)
    return np.array([L, pk, g, passed.sum()], dtype=np.float32), (z, passed, l, rel, L)


def wave_level(wave, frames, T_cap, spf, trim, fs, target, ceiling, max_gain_db):
    """wave fp32 [B, >= spf T_cap] -> (level fp32 [B, 4], per-row details)."""
    n = row_samples(frames, T_cap, spf, trim)
    rows = [level_row(np.asarray(wave[b], dtype=np.float32)[:n[b]], fs, target[b], ceiling, max_gain_db) for b in range(len(n))]
    return np.stack([r[0] for r in rows]), [r[1] for r in rows]


def apply_gain(wave, frames, T_cap, spf, trim, gains):
    """fl32(x * g_b) on every valid sample: the input the existing packing contracts (`_syncfree_ref`, `_resample_ref`,
    `_passage_ref`) see.  Samples at or past n_b are left as they are (nothing reads them)."""
    out = np.array(wave, dtype=np.float32, copy=True)
    for b, n_b in enumerate(row_samples(frames, T_cap, spf, trim)):
        out[b, :n_b] = out[b, :n_b] * np.float32(gains[b])
    return out
