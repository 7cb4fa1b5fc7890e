"""The numpy statement of the per-request controls contract (include/st2.h "per-request controls"): what
tests/test_controls_cpu.py pins on its tie cases and tests/test_controls_gpu.py compares the kernels against.  fp32 arithmetic
is numpy's (IEEE: one correctly rounded operation per `*`, `+`, `/`; np.rint rounds half to even)."""
import numpy as np

F32 = np.float32
RANGES = {"speed": (0.25, 4.0), "alpha": (0.0, 1.0), "beta": (0.0, 1.0), "t": (0.0, 1.0), "f0_scale": (0.5, 2.0),
          "n_shift": (-2.0, 2.0)}
NEUTRAL = {"speed": 1.0, "f0_scale": 1.0, "n_shift": 0.0}  # what NaN becomes (the mixing weights: the call's scalar)


def clamp(name, row, scalar=None):
    """The device clamp of a control row: into its range, NaN -> the neutral value (`scalar` for a mixing weight)."""
    row = np.asarray(row, dtype=F32)
    lo, hi = RANGES[name]
    out = np.minimum(np.maximum(row, F32(lo)), F32(hi))
    return np.where(np.isnan(row), F32(NEUTRAL.get(name, np.nan) if scalar is None else scalar), out).astype(F32)


def durations(total, speed, lengths=None, tail=0):
    """dur[b][n] = max(1, rint(total[b][n] / speed[b])): total fp32 [B, N] (the sigmoid sums), speed [B] (clamped here as the
    device clamps it) or None, one fp32 division; pad tokens (n >= lengths[b]) get 0; `tail` is added to the row's last token
    afterwards, unscaled."""
    total = np.asarray(total, dtype=F32)
    B, N = total.shape
    q = total if speed is None else (total / clamp("speed", speed)[:, None]).astype(F32)
    d = np.maximum(np.rint(q), F32(1.0)).astype(np.int64)
    lens = np.full((B,), N) if lengths is None else np.clip(np.asarray(lengths), 1, N)
    for b in range(B):
        d[b, lens[b]:] = 0
        d[b, lens[b] - 1] += tail
    return d


def _weight(name, row, b, scalar):
    """(w, 1 - w) of row b as the kernels form them: the scalar pair is ((float) w0, (float)(1.0 - w0)) in double; a row value is
    clamped to [0, 1] (NaN -> the scalar pair) and its complement is (float)(1.0 - (double) w)."""
    if row is None or np.isnan(F32(row[b])):
        return F32(scalar), F32(1.0 - float(scalar))
    w = clamp(name, [row[b]])[0]
    return w, F32(1.0 - float(w))


def _mix(a, x, b, y):
    v = (F32(a) * x).astype(F32)  # v = a x; v += b y: two roundings per product-sum, no FMA
    return (v + (F32(b) * y).astype(F32)).astype(F32)


def style_mix(s_pred, s_prev=None, ref_s=None, t=None, alpha=None, beta=None, t0=0.7, alpha0=0.3, beta0=0.7, carry=False,
              exact=False):
    """The front's style mixing, row b with its own weights -> (ref [B, sty], s [B, sty]).  `exact`: the same weights (as the
    fp32 values the kernels hold) applied in float64 -- the yardstick of the 2-ulp bound."""
    sp = np.asarray(s_pred, dtype=F32)
    B, C2 = sp.shape
    sty = C2 // 2
    out = np.zeros((B, C2), dtype=np.float64 if exact else F32)
    mix = (lambda a, x, b, y: float(a) * x.astype(np.float64) + float(b) * y.astype(np.float64)) if exact else _mix
    for b in range(B):
        cur = sp[b].astype(out.dtype)
        prev = (out[b - 1] if b > 0 else (None if s_prev is None else np.asarray(s_prev, dtype=F32)[0])) if carry else \
            (None if s_prev is None else np.asarray(s_prev, dtype=F32)[b])
        if prev is not None:
            w, cw = _weight("t", t, b, t0)
            cur = mix(w, prev.astype(out.dtype), cw, cur)
        if ref_s is not None:
            rs = np.asarray(ref_s, dtype=F32)[b].astype(out.dtype)
            wa, cwa = _weight("alpha", alpha, b, alpha0)
            wb, cwb = _weight("beta", beta, b, beta0)
            cur = np.concatenate([mix(wa, cur[:sty], cwa, rs[:sty]), mix(wb, cur[sty:], cwb, rs[sty:])])
        out[b] = cur
    return out[:, :sty], out[:, sty:]


def prosody(F0, N, f0_scale=None, n_shift=None, frames=None):
    """F0[b][l] *= f0_scale[b], N[b][l] += n_shift[b] for l < 2 frames[b] (every l without frames); the rest is untouched; a
    shift of 0 keeps x itself."""
    F0, N = np.array(F0, dtype=F32), np.array(N, dtype=F32)
    B, L = F0.shape
    for b in range(B):
        n = L if frames is None else min(2 * max(int(frames[b]), 0), L)
        if f0_scale is not None:
            F0[b, :n] = (F0[b, :n] * clamp("f0_scale", [f0_scale[b]])[0]).astype(F32)
        if n_shift is not None:
            sh = clamp("n_shift", [n_shift[b]])[0]
            if sh != 0:
                N[b, :n] = (N[b, :n] + sh).astype(F32)
    return F0, N
