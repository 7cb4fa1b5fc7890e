"""The contract of `st2_pitch_shape` (include/st2.h) in numpy fp64, with the order of every operation
written out, and once more as a plain per-column loop (`brute_row`).  Not a test module.

Everything is fixed bit for bit except the last ulp of fp64 `log2` / `exp2` and the order of the fp64 sum behind the row mean:
both forms here take the exactly rounded sum (`math.fsum`), which no order can be further than a few fp64 ulps from.  An fp64
ulp of y is 2^-29 of an fp32 ulp of exp2(y), so a device differs from these by at most one fp32 ulp, and only where the exact
value sits that close to a rounding boundary.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_POINTS = 8


def clamp_range(v):
    """range / tok_range as the kernel reads it: fp32, into [0, 4], NaN -> 1."""
    v = np.asarray(v, dtype=F32)
    return np.where(np.isnan(v), F32(1), np.minimum(np.maximum(v, F32(0)), F32(4))).astype(F32)


def clean_contour(points):
    """contour[b] fp32 [K][2] -> (p fp32 [n], v fp32 [n]) of the used points: NaN ones dropped, p clamped to [0, 1] and raised to
    the running maximum, v clamped to [-24, 24]."""
    ps, vs, run = [], [], F32(0)
    for p, v in np.asarray(points, dtype=F32).reshape(-1, 2):
        if np.isnan(p) or np.isnan(v):
            continue
        run = max(min(max(p, F32(0)), F32(1)), run)
        ps.append(run)
        vs.append(min(max(v, F32(-24)), F32(24)))
    return np.asarray(ps, dtype=F32), np.asarray(vs, dtype=F32)


def token_index(dur_row, T_b, T_cap, shift):
    """idx(b, t) for t < T_b as `prosody_controls_tok_kernel` finds it: cum[i] = min(T_cap, sum_{m <= i} clamp(dur[m], 0, T_cap)), the
    first m with cum[m] > ts (ts = max(t - 1, 0) under the shift), capped at N - 1."""
    d = np.clip(np.asarray(dur_row, dtype=np.int64), 0, int(T_cap))
    cum = np.minimum(np.cumsum(d), int(T_cap))
    t = np.arange(T_b, dtype=np.int64)
    ts = np.maximum(t - 1, 0) if shift else t
    return np.minimum(np.searchsorted(cum, ts, side="right"), len(d) - 1)


def contour_at(ps, vs, T_b):
    """c[t] in fp64 for t < T_b from the cleaned points."""
    n = len(ps)
    if n == 0:
        return np.zeros(T_b, dtype=F64)
    p, v = ps.astype(F64), vs.astype(F64)
    x = (np.arange(T_b, dtype=F64) + 0.5) / F64(T_b)
    j = np.searchsorted(p, x, side="right")  # the number of points with p <= x
    a, e = np.clip(j - 1, 0, n - 1), np.clip(j, 0, n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mid = v[a] + (v[e] - v[a]) * ((x - p[a]) / (p[e] - p[a]))
    return np.where(j == 0, v[0], np.where(j == n, v[n - 1], mid))


def is_voiced(x, voiced_hz):
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x > F32(voiced_hz))


def reference_row(x, T_b, r_b=None, tok=None, dur=None, shift=False, points=None, voiced_hz=10.0, lo_hz=40.0, hi_hz=1100.0,
                  info=None):
    """One row: x fp32 [L] (only the first 2 T_b columns are looked at) -> (out fp32 [L], pitch fp32 [4]).  `r_b`: the row's range
    or None; `tok`: its fp32 [N] token ranges or None, with `dur` int [N]; `points`: its fp32 [K][2] contour or None.  T_cap = L / 2.
    `info` (a dict): receives "exact", bool [L]: the columns the contract fixes by bits (the input's)."""
    x = np.asarray(x, dtype=F32)
    out = x.copy()
    if info is not None:
        info["exact"] = np.ones(len(x), dtype=bool)
    T_cap = len(x) // 2
    T_b = min(max(int(T_b), 0), T_cap)
    row = x[:2 * T_b]
    vo = is_voiced(row, voiced_hz)
    n_v = int(vo.sum())
    if n_v == 0:
        return out, np.array([np.nan, 0, np.nan, np.nan], dtype=F32)
    lg = np.log2(row[vo].astype(F64))
    m = F64(math.fsum(lg.tolist())) / F64(n_v)
    rb = F32(1) if r_b is None else clamp_range(r_b)
    if tok is None:
        r = np.full(T_b, rb, dtype=F32)
    else:
        q = clamp_range(tok)[token_index(dur, T_b, T_cap, shift)]
        r = np.minimum((rb * q).astype(F32), F32(4))
    c = contour_at(*clean_contour(np.zeros((0, 2)) if points is None else points), T_b)
    r2, c2 = np.repeat(r, 2)[vo], np.repeat(c, 2)[vo]
    y = (m + r2.astype(F64) * (lg - m)) + c2 / F64(12.0)
    with np.errstate(over="ignore"):
        shaped = np.minimum(np.maximum(np.exp2(y), F64(F32(lo_hz))), F64(F32(hi_hz))).astype(F32)
    res = np.where((r2 == F32(1)) & (c2 == 0.0), row[vo], shaped)
    out[np.flatnonzero(vo)] = res
    if info is not None:
        info["exact"][np.flatnonzero(vo)] = (r2 == F32(1)) & (c2 == 0.0)
    return out, np.array([F32(np.exp2(m)), F32(n_v), res.min(), res.max()], dtype=F32)


def reference(f0, frames=None, range=None, tok_range=None, dur=None, shift=False, contour=None, voiced_hz=10.0, lo_hz=40.0,
              hi_hz=1100.0):
    """The batch: f0 fp32 [B][L] -> (out [B][L], pitch [B][4]).  Columns at or past a row's end come back as they are.
    `reference.exact` then holds bool [B][L]: the columns of this call that the contract fixes by bits."""
    f0 = np.asarray(f0, dtype=F32)
    outs, pitches, exact = [], [], []
    for b in np.arange(f0.shape[0]):
        info = {}
        o, p = reference_row(f0[b], f0.shape[1] // 2 if frames is None else frames[b], None if range is None else range[b],
                             None if tok_range is None else tok_range[b], None if dur is None else dur[b], shift,
                             None if contour is None else contour[b], voiced_hz, lo_hz, hi_hz, info)
        outs.append(o)
        pitches.append(p)
        exact.append(info["exact"])
    reference.exact = np.stack(exact)  # of the last call: the columns fixed by bits
    return np.stack(outs), np.stack(pitches)


def brute_row(x, T_b, r_b=None, tok=None, dur=None, shift=False, points=None, voiced_hz=10.0, lo_hz=40.0, hi_hz=1100.0):
    """The contract once more as plain loops over columns, frames, tokens and points."""
    x = np.asarray(x, dtype=F32)
    out = x.copy()
    T_cap = len(x) // 2
    T_b = min(max(int(T_b), 0), T_cap)
    vh, lo, hi = F32(voiced_hz), F64(F32(lo_hz)), F64(F32(hi_hz))
    voiced = [bool(np.isfinite(x[l]) and x[l] > vh) for l in np.arange(2 * T_b)]
    logs = {l: np.log2(x[l:l + 1].astype(F64))[0] for l in np.arange(2 * T_b) if voiced[l]}
    if not logs:
        return out, np.array([np.nan, 0, np.nan, np.nan], dtype=F32)
    m = F64(math.fsum(float(v) for v in logs.values())) / F64(len(logs))
    one = lambda v: F32(1) if np.isnan(F32(v)) else min(max(F32(v), F32(0)), F32(4))
    rb = F32(1) if r_b is None else one(r_b)
    ps, vs, run = [], [], F32(0)
    for k in np.arange(0 if points is None else len(points)):
        p, v = F32(points[k][0]), F32(points[k][1])
        if np.isnan(p) or np.isnan(v):
            continue
        run = max(min(max(p, F32(0)), F32(1)), run)
        ps.append(F64(run))
        vs.append(F64(min(max(v, F32(-24)), F32(24))))
    cum, acc = [], 0
    for d in ([] if tok is None else dur):
        acc = min(acc + min(max(int(d), 0), T_cap), T_cap)
        cum.append(acc)
    lo_out, hi_out = None, None
    for t in np.arange(T_b):
        r = rb
        if tok is not None:
            ts = max(int(t) - 1, 0) if shift else int(t)
            idx = min(sum(1 for cm in cum if cm <= ts), len(cum) - 1)
            r = min(F32(rb * one(tok[idx])), F32(4))
        c = F64(0.0)
        if ps:
            xx = (F64(t) + F64(0.5)) / F64(T_b)
            j = sum(1 for p in ps if p <= xx)
            if j == 0:
                c = vs[0]
            elif j == len(ps):
                c = vs[-1]
            else:
                c = vs[j - 1] + (vs[j] - vs[j - 1]) * ((xx - ps[j - 1]) / (ps[j] - ps[j - 1]))
        for l in (2 * t, 2 * t + 1):
            if not voiced[l]:
                continue
            if not (r == F32(1) and c == 0.0):
                y = (m + F64(r) * (logs[l] - m)) + c / F64(12.0)
                with np.errstate(over="ignore"):
                    out[l] = F32(min(max(np.exp2(np.array([y]))[0], lo), hi))
            lo_out = out[l] if lo_out is None else min(lo_out, out[l])
            hi_out = out[l] if hi_out is None else max(hi_out, out[l])
    return out, np.array([F32(np.exp2(m)), F32(len(logs)), lo_out, hi_out], dtype=F32)


def ulp_diff(a, b):
    """|a - b| in fp32 ulps for finite fp32 arrays (the distance of their ordered bit patterns)."""
    a = np.ascontiguousarray(a, dtype=F32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=F32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
