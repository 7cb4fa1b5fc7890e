"""The contract of `st2_wave_limit` (include/st2.h) in plain numpy and fp64: the drive gain of a row from
its level, the envelope (sample peaks, or the larger of them and the row interpolated U times), the required gain, its sliding
minimum (the hold), the FIR smoother and the product.  Written from the header, not from the kernel; the level of a row is
tests/_level_ref.py's, the interpolation tests/_truepeak_ref.py's.  Not product code.

What the kernel rounds to fp32 by contract -- g', r -- is rounded here too; what it evaluates as an fp32 chain (rule 5, the
interpolation) is evaluated here in fp64, and `bound` / `envelope`'s second value say how far such a chain may be off."""
import math

import numpy as np

import _truepeak_ref as TP


def window(W):
    """The package's window: Hann over 2 W + 1 points without its zero end points, normalised in fp64, as fp32."""
    k = np.arange(1, 2 * W + 2, dtype=np.float64)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (2 * W + 2))
    return (h / h.sum()).astype(np.float32)


def drive_gain(L, pk, target, ceiling, max_gain_db, drive_db):
    """Rule 1 -> g' as fp32, or None where the row is left alone (NaN target, L = -inf, peak = 0)."""
    target, L, pk = float(np.float32(target)), float(np.float32(L)), float(np.float32(pk))
    if math.isnan(target) or L == -math.inf or pk == 0.0:
        return None
    return np.float32(min(10.0 ** ((target - L) / 20.0), 10.0 ** (max_gain_db / 20.0), 10.0 ** (drive_db / 20.0) * ceiling / pk))


def envelope(x, taps=None):
    """Rule 2 over a row's valid samples -> (e fp64 [n], how far an fp32 evaluation of e may be off [n]): |x| cleaned, exact;
    with taps [U, K] the larger of it and the U interpolated values of each position, off by the chain's bound at most."""
    a = np.abs(TP.clean32(x).astype(np.float64))
    if taps is None or len(a) == 0:
        return a, np.zeros(len(a))
    U = taps.shape[0]
    y, bound = TP.interpolate(x, taps)
    y, bound = np.abs(y).reshape(-1, U), bound.reshape(-1, U)
    e = np.maximum(a, y.max(axis=1))
    # the fp32 chain reads every |y| within its bound, so the maximum moves by no more than the largest bound of the position
    return e, bound.max(axis=1)


def required(e, ceiling, g):
    """Rule 3 -> r fp32 [n]: min(1, c / (e g')) in fp64, rounded once; 1 where e = 0."""
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(divide="ignore"):
        r = np.where(e > 0.0, np.minimum(1.0, ceiling / (e * float(g))), 1.0)
    return r.astype(np.float32)


def hold(r, W):
    """Rule 4 -> m [n + 2 W], m[j] for j = -W .. n + W - 1 (index j + W): the minimum of r over |d| <= W, r = 1 outside the row.
    Outside that range m is 1."""
    n = len(r)
    pad = np.concatenate([np.ones(2 * W, r.dtype), r, np.ones(2 * W, r.dtype)])
    return np.lib.stride_tricks.sliding_window_view(pad, 2 * W + 1).min(axis=1) if n + 2 * W > 0 else pad[:0]


def smooth(m, win, W, n):
    """Rule 5 in fp64 -> s [n]: 1 - sum_k win[k] (1 - m[i - W + k]); `m` as `hold` returns it."""
    d = 1.0 - m.astype(np.float64)
    return 1.0 - np.lib.stride_tricks.sliding_window_view(d, 2 * W + 1)[:n] @ win.astype(np.float64) if n else np.zeros(0)


def limit_row(x, g, ceiling, W, win, taps=None):
    """A row's valid samples and its drive gain -> dict(out fp64 [n], q, r fp32, m, s, e, e_bound, xg fp32 = fl32(x g'))."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    e, e_bound = envelope(x, taps)
    r = required(e, ceiling, g)
    m = hold(r, W)
    s = smooth(m, win, W, n)
    q = np.minimum(s, r.astype(np.float64))
    xg = TP.clean32(x) * np.float32(g)
    return dict(out=xg.astype(np.float64) * q, q=q, r=r, m=m, s=s, e=e, e_bound=e_bound, xg=xg)


def bound(ref, W):
    """The issue's bound on an fp32 evaluation of `out` from the same r: (2 W + 6) 2^-24 |x g'| -- the chain of 2 W + 1 fmaf over
    terms that sum to at most 1 (+ 1 for the rounding of each 1 - m, + 1 for the last difference), and the roundings of x g' and
    of its product with q."""
    return (2 * W + 6) * 2.0 ** -24 * np.abs(ref["xg"].astype(np.float64))


def q_interval(ref, g, ceiling, W, win):
    """With a table the fp32 envelope may sit anywhere in e +- e_bound: r, m, s and q are monotone in it, so q lies between the q of
    the two extreme envelopes -> (q_lo, q_hi)."""
    n = len(ref["r"])
    lo = required(ref["e"] + ref["e_bound"], ceiling, g)
    hi = required(np.maximum(ref["e"] - ref["e_bound"], 0.0), ceiling, g)
    both = []
    for r in (lo, hi):  # rule 3's one rounding is monotone: the kernel's r lies between these two, ends included
        both.append(np.minimum(smooth(hold(r, W), win, W, n), r.astype(np.float64)))
    return both[0], both[1]


def groups_target(target, start):
    """The target every row reads: its group's first row's (start None: its own)."""
    B = len(target)
    return [target[a] for a, e in TP.groups(start, B) for _ in range(a, e)]


def wave_limit(wave, n, level, target, ceiling, max_gain_db, drive_db, W, win, taps=None, start=None):
    """wave fp32 [B, >= n_b], level fp32 [B, 4] -> (rows: `limit_row`'s dict or None where left alone, limit fp32 [B, 2] with the
    minimum of the fp64 q)."""
    tg = groups_target(target, start)
    rows, lim = [], np.ones((len(n), 2), dtype=np.float32)
    for b, n_b in enumerate(n):
        g = drive_gain(level[b][0], level[b][1], tg[b], ceiling, max_gain_db, drive_db)
        if g is None:
            rows.append(None)
            continue
        ref = limit_row(np.asarray(wave[b], dtype=np.float32)[:n_b], g, ceiling, W, win, taps)
        rows.append(ref)
        lim[b] = (g, ref["q"].min() if n_b else 1.0)
    return rows, lim


def brute(x, g, ceiling, W, win):
    """`limit_row` without a table, one sample at a time in Python floats: what tests/test_limit_cpu.py checks the arrays against."""
    x = [float(v) if math.isfinite(float(v)) else 0.0 for v in np.asarray(x, dtype=np.float32)]
    n, g = len(x), float(np.float32(g))
    r = lambda i: 1.0 if i < 0 or i >= n or x[i] == 0.0 else float(np.float32(min(1.0, ceiling / (abs(x[i]) * g))))
    m = lambda j: min(r(j + d) for d in range(-W, W + 1))
    out, q = [], []
    for i in range(n):
        s = 1.0 - sum(float(win[k]) * (1.0 - m(i - W + k)) for k in range(2 * W + 1))
        q.append(min(s, r(i)))
        out.append(float(np.float32(np.float32(x[i]) * np.float32(g))) * q[-1])
    return np.array(out), np.array(q)
