"""The contract of `st2_clip_ingest` (include/st2.h) restated in numpy fp64, and the constructed clips
that tests/test_ingest_cpu.py and tests/test_ingest_gpu.py share.  The polyphase sum is `_resample_ref.polyphase` over the
SAME fp32 table the kernel reads; the trim is librosa's `effects.trim(y, top_db, ref=max, frame_length=2048, hop_length=512)`
with centred, zero-padded frames written out (that library is not a dependency); G.711 expansion is the bit formula of the
standard's reference code (ITU-T G.191), independent of `_resample_ref`'s.  Not product code."""
import functools
import math

import numpy as np

import _resample_ref as R

HOP, FRAME = 512, 2048
NP_DTYPE = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}


# ---- decode -----------------------------------------------------------------------------------------------------------------
def ulaw_expand(code):
    """G.191 ulaw_expand: ((mantissa << 3) + 0x84) << exponent, less the bias, of the inverted byte."""
    inv = ~np.asarray(code, dtype=np.int64) & 0xFF
    lin = ((((inv & 0x0F) << 3) + 0x84) << ((inv >> 4) & 7)) - 0x84
    return np.where(inv & 0x80, -lin, lin)


def alaw_expand(code):
    """G.191 alaw_expand, on the 16-bit scale: mantissa with its half step, the hidden bit from segment 1 on."""
    ix = (np.asarray(code, dtype=np.int64) ^ 0x55)
    e, man = (ix >> 4) & 7, ix & 0x0F
    lin = np.where(e == 0, (man << 4) + 8, ((man << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(ix & 0x80, lin, -lin)


EXPAND = {"ulaw": ulaw_expand, "alaw": alaw_expand}


def decode(raw, fmt):
    """Samples of a client's clip -> fp32 (every value exact)."""
    raw = np.asarray(raw)
    if fmt == "f32":
        return raw.astype(np.float32)
    v = raw.astype(np.int64) if fmt == "s16" else EXPAND[fmt](raw)
    return (v / 32768.0).astype(np.float32)


def encode(x, fmt):
    """fp32 samples -> what a client would send (for building test inputs)."""
    if fmt == "f32":
        return np.asarray(x, dtype=np.float32)
    v = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int64)
    return v.astype(np.int16) if fmt == "s16" else R.ENCODE[fmt](v)


# ---- trim -------------------------------------------------------------------------------------------------------------------
def frame_energies(r):
    """e_f = max(sum r[512 f - 1024, 512 f + 1024)^2 / 2048, 1e-10), f = 0 .. len(r) // 512, zeros outside the clip."""
    m = len(r)
    nf = m // HOP + 1
    z = np.zeros(FRAME // 2 + HOP * nf + FRAME // 2, dtype=np.float64)
    z[FRAME // 2:FRAME // 2 + m] = np.asarray(r, dtype=np.float64) ** 2
    c = np.concatenate([[0.0], np.cumsum(z)])
    f = np.arange(nf)
    return np.maximum((c[HOP * f + FRAME] - c[HOP * f]) / FRAME, 1e-10)


def trim_bounds(r, top_db):
    """-> (start, end, margin): the cut, and how far the frame nearest the threshold is from it, as a ratio >= 1 (inf when no
    frame can flip: top_db <= 0)."""
    m = len(r)
    if top_db <= 0:
        return 0, m, math.inf
    e = frame_energies(r)
    lim = e.max() * 10.0 ** (-top_db / 10.0)
    loud = np.nonzero(e > lim)[0]
    ratio = np.where(e > lim, e / lim, lim / e)
    return HOP * int(loud[0]), min(m, HOP * (int(loud[-1]) + 1)), float(ratio.min())


def min_length(start, end, m, L_min):
    """-> (start, end, flagged)"""
    if end - start >= L_min:
        return start, end, False
    end = min(m, start + L_min)
    return max(0, end - L_min), end, True


def ingest_row(raw, n, fmt, taps, U, D, top_db, L_min, L_cap, N_cap=None):
    """One row -> dict(wave fp64 [len], bound fp64 [len], len, start, flags, margin, m)."""
    n = min(max(int(n), 0), len(raw) if N_cap is None else N_cap)
    y, bound = R.polyphase(decode(raw[:n], fmt), n, taps, U, D)
    full = len(y)
    m = min(L_cap, full)
    y, bound = y[:m], bound[:m]
    s0, s1, margin = trim_bounds(y, top_db)
    s0, s1, short = min_length(s0, s1, m, L_min)
    return dict(wave=y[s0:s1], bound=bound[s0:s1], len=s1 - s0, start=s0, flags=(1 if full > L_cap else 0) | (2 if short else 0),
                margin=margin, m=m)


# ---- the constructed clips of the trim and minimum-length tests --------------------------------------------------------------
TOP_DB = 30.0
L_MIN = 4096
TRIM_RATES = [(16000, "s16"), (8000, "ulaw")]
M_CAP = 9000  # samples at 24 kHz of a row at capacity: 17 whole hops and 296 samples


def _burst(x, a, b, rng, ramp=48, amp=0.5):
    """A tone with two partials and raised-cosine edges on x[a:b) (positions at 24 kHz)."""
    t = np.arange(b - a, dtype=np.float64)
    env = np.ones(b - a)
    k = min(ramp, (b - a) // 2)
    edge = 0.5 - 0.5 * np.cos(np.pi * (np.arange(k) + 0.5) / k)
    env[:k], env[b - a - k:] = edge, edge[::-1]
    x[a:b] += amp * env * (0.7 * np.sin(2 * np.pi * 220.0 / 24000 * t + rng.uniform(0, 6)) +
                           0.3 * np.sin(2 * np.pi * 1330.0 / 24000 * t))


def _clip24(m, bursts, seed, noise=2e-4):
    rng = np.random.default_rng(seed)
    x = noise * rng.standard_normal(m)
    for a, b in bursts:
        _burst(x, a, b, rng)
    return x


def _to_rate(x24, U, D, fmt):
    """A 24 kHz construction sampled at the client's rate (linear interpolation: only the positions matter) and encoded."""
    n = len(x24) * D // U
    t = np.arange(n, dtype=np.float64) * U / D
    return encode(np.interp(t, np.arange(len(x24)), x24), fmt)


@functools.lru_cache(maxsize=None)
def trim_cases(rate, fmt):
    """-> (names, rows): six clips, positions chosen at 24 kHz so that every burst edge lies 256 samples inside a frame."""
    from styletts2_amd import resample
    U, D, _ = resample.design_input(rate)
    cases = [
        ("burst at the very start", _clip24(M_CAP, [(0, 2816)], 1)),
        ("burst at the very end", _clip24(M_CAP - 217, [(4864, M_CAP - 217)], 2)),          # end = m_b, no multiple of 512
        ("two bursts, silence between", _clip24(M_CAP, [(1792, 3328), (5888, 7424)], 3)),
        ("all zero", np.zeros(7001)),
        ("shorter than one frame", _clip24(1500, [(0, 1500)], 5)),
        ("burst in mid-clip, row at capacity", _clip24(M_CAP, [(3840, 5376)], 6)),
    ]
    return [c[0] for c in cases], [_to_rate(c[1], U, D, fmt) for c in cases]


@functools.lru_cache(maxsize=None)
def short_cases(rate, fmt):
    """Bursts of 600 samples: the trim leaves less than L_MIN = 4096 and the minimum-length rule widens the cut -- in
    mid-clip, at the start (start stays 0) and at the end (end stays m_b)."""
    from styletts2_amd import resample
    U, D, _ = resample.design_input(rate)
    cases = [
        ("short burst in mid-clip", _clip24(M_CAP, [(4352, 4952)], 11)),
        ("short burst at the start", _clip24(M_CAP, [(0, 600)], 12)),
        ("short burst at the end", _clip24(M_CAP - 101, [(M_CAP - 701, M_CAP - 101)], 13)),
        ("a whole clip below the minimum", _clip24(3000, [(768, 1368)], 14)),
    ]
    return [c[0] for c in cases], [_to_rate(c[1], U, D, fmt) for c in cases]


def stack(rows, fmt, fill):
    """Rows of unequal length -> (buffer [B, N_cap] filled with `fill` past each row, n)."""
    n = [len(r) for r in rows]
    buf = np.full((len(rows), max(n)), fill, dtype=NP_DTYPE[fmt])
    for b, r in enumerate(rows):
        buf[b, :n[b]] = r
    return buf, n


@functools.lru_cache(maxsize=None)
def reference(kind, rate, fmt, L_min):
    """The fp64 reference of every row of trim_cases / short_cases, computed once and shared."""
    from styletts2_amd import resample
    U, D, taps = resample.design_input(rate)
    names, rows = (trim_cases if kind == "trim" else short_cases)(rate, fmt)
    L_cap = resample.output_samples(max(len(r) for r in rows), U, D)
    return names, [ingest_row(r, len(r), fmt, taps, U, D, TOP_DB, L_min, L_cap) for r in rows], L_cap
