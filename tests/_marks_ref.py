"""The numpy statement of the timing-marks and per-token controls contract (include/st2.h "timing marks
and per-token prosody controls"), written from the contract and not from the kernels: what tests/test_marks_cpu.py checks
against a brute-force per-frame expansion and tests/test_marks_gpu.py compares the kernels against.  Integer arithmetic is
Python's (unbounded); fp32 arithmetic is numpy's (IEEE: one correctly rounded operation per `*`, `+`, `/`; np.rint rounds half
to even)."""
import numpy as np

F32 = np.float32
TOK_RANGES = {"tok_speed": (0.25, 4.0), "tok_f0_scale": (0.5, 2.0), "tok_n_shift": (-2.0, 2.0)}
TOK_NEUTRAL = {"tok_speed": 1.0, "tok_f0_scale": 1.0, "tok_n_shift": 0.0}


def _rows(dur, lengths, frames, T_cap):
    dur = np.asarray(dur, dtype=np.int64)
    B, N = dur.shape
    n_b = [N if lengths is None else min(max(int(lengths[b]), 0), N) for b in range(B)]
    T_b = [int(T_cap) if frames is None else min(max(int(frames[b]), 0), int(T_cap)) for b in range(B)]
    return dur, B, N, n_b, T_b


def bounds(dur, lengths, frames, T_cap, shift):
    """bound[b][n], n = 0..N: the first frame of token n.  c[n] = min(T_cap, sum_{m < min(n, n_b)} dur[b][m]);
    bound[0] = 0, bound[n] = min(T_b, 0 if c[n] == 0 else c[n] + shift) for 1 <= n <= N - 1, bound[N] = T_b."""
    dur, B, N, n_b, T_b = _rows(dur, lengths, frames, T_cap)
    out = np.zeros((B, N + 1), dtype=np.int64)
    for b in range(B):
        c = 0  # Python int: the saturating 64-bit sum of the contract, without a width
        for n in range(1, N):
            if n - 1 < n_b[b]:
                c = min(int(T_cap), c + int(dur[b, n - 1]))
            out[b, n] = min(T_b[b], 0 if c == 0 else c + (1 if shift else 0))
        out[b, N] = T_b[b]
        out[b, 0] = 0
    return out


def marks(dur, lengths, frames, T_cap, shift, spf=600, trim=0, U=1, D=1):
    """marks[b][n] = ceil(min(spf * bound[b][n], n_smp) * U / D), n_smp = max(0, spf * T_b - trim)."""
    bd = bounds(dur, lengths, frames, T_cap, shift)
    _, B, N, _, T_b = _rows(dur, lengths, frames, T_cap)
    out = np.zeros((B, N + 1), dtype=np.int64)
    for b in range(B):
        n_smp = max(0, spf * T_b[b] - trim)
        for n in range(N + 1):
            s = min(spf * int(bd[b, n]), n_smp)
            out[b, n] = (s * U + D - 1) // D
    return out


def brute_index(dur_row, T_b, shift):
    """idx(b, t) for t < T_b, frame by frame, the way the expansion states it: the number of tokens whose inclusive prefix sum is
    <= ts (ts = max(t - 1, 0) with the shift, else t), capped at N - 1.  A loop per frame, no closed form."""
    d = [int(v) for v in dur_row]
    N = len(d)
    cum, acc = [], 0
    for v in d:
        acc += v
        cum.append(acc)
    idx = []
    for t in range(T_b):
        ts = max(t - 1, 0) if shift else t
        idx.append(min(sum(1 for c in cum if c <= ts), N - 1))
    return idx


def first_frame_at_or_past(idx, n, T_b):
    """The first frame whose index is >= n, T_b if there is none."""
    for t, i in enumerate(idx):
        if i >= n:
            return t
    return T_b


def clamp(name, v):
    """The device clamp of a per-token control: into its range, NaN -> neutral."""
    v = np.asarray(v, dtype=F32)
    lo, hi = TOK_RANGES[name]
    return np.where(np.isnan(v), F32(TOK_NEUTRAL[name]), np.minimum(np.maximum(v, F32(lo)), F32(hi))).astype(F32)


def _clamp_speed(v):
    v = np.asarray(v, dtype=F32)
    return np.where(np.isnan(v), F32(1.0), np.minimum(np.maximum(v, F32(0.25)), F32(4.0))).astype(F32)


def durations(total, speed, tok_speed, lengths=None, tail=0):
    """dur[b][n] = max(1, rint(total[b][n] / r)), r = clamp(clamp(speed[b]) * clamp(tok_speed[b][n])): one fp32 product, one fp32
    division; speed None = 1.  Pad tokens (n >= max(lengths[b], 1)) get 0; `tail` is added to the row's last token, unscaled."""
    total = np.asarray(total, dtype=F32)
    B, N = total.shape
    sp = np.ones((B,), dtype=F32) if speed is None else _clamp_speed(speed)
    r = _clamp_speed((sp[:, None] * clamp("tok_speed", tok_speed)).astype(F32))
    d = np.maximum(np.rint((total / r).astype(F32)), F32(1.0)).astype(np.int64)
    lens = np.full((B,), N) if lengths is None else np.clip(np.asarray(lengths), 1, N)
    for b in range(B):
        d[b, lens[b]:] = 0
        d[b, lens[b] - 1] += tail
    return d


def prosody_tok(F0, N, dur, shift, tok_f0_scale=None, tok_n_shift=None, frames=None):
    """F0[b][l] *= tok_f0_scale[b][idx(b, l // 2)], N[b][l] += tok_n_shift[b][idx(b, l // 2)] for l < 2 T_b; the rest is untouched; a
    shift of 0 keeps x itself."""
    F0, N = np.array(F0, dtype=F32), np.array(N, dtype=F32)
    B, L = F0.shape
    for b in range(B):
        T_b = L // 2 if frames is None else min(max(int(frames[b]), 0), L // 2)
        idx = np.repeat(np.asarray(brute_index(dur[b], T_b, shift), dtype=np.int64), 2)
        if tok_f0_scale is not None:
            F0[b, :2 * T_b] = (F0[b, :2 * T_b] * clamp("tok_f0_scale", tok_f0_scale[b])[idx]).astype(F32)
        if tok_n_shift is not None:
            sh = clamp("tok_n_shift", tok_n_shift[b])[idx]
            x = N[b, :2 * T_b]
            N[b, :2 * T_b] = np.where(sh == 0, x, (x + sh).astype(F32))
    return F0, N
