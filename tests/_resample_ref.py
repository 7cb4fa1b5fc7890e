"""The contract of `st2_wave_resample_pack` (include/st2.h) restated in numpy fp64: what
tests/test_resample_gpu.py compares the kernel against.  The polyphase sum runs over the SAME fp32 table the kernel reads; the
16-bit conversion is `_syncfree_ref.pcm16`; G.711 is written out by the segment rule of the standard (the formulation of its
reference code, ITU-T G.191: the magnitude of a negative 16-bit sample is its one's complement).  Not product code."""
import numpy as np

from _syncfree_ref import pcm16  # noqa: F401  (re-exported: the tests take both conversions from here)

EPS = 2.0 ** -24  # fp32 unit roundoff


def row_counts(frames, T_cap, spf, trim, U, D):
    """-> (n, m): per row, the valid input samples n_b = max(0, spf * clamp(frames[b], 0, T_cap) - trim) and the output samples
    m_b = ceil(n_b U / D)."""
    n = [max(0, spf * min(max(int(f), 0), T_cap) - trim) for f in frames]
    return n, [(v * U + D - 1) // D for v in n]


def polyphase(x, n, taps, U, D):
    """One row.  x fp32 (only x[:n] is looked at), taps fp32 [U, K] -> (y, bound), both fp64 [m]:
    y[j] = sum_k taps[p][k] x[c - (K - 1) // 2 + k], c = j D // U, p = j D % U, x = 0 outside [0, n), and the bound on what fp32
    fmaf accumulation of those K terms may differ from it by: (K + 1) 2^-24 sum_k |taps[p][k] x[.]|."""
    K = taps.shape[1]
    h = (K - 1) // 2
    m = (n * U + D - 1) // D
    xz = np.zeros(h + n + K, dtype=np.float64)
    xz[h:h + n] = np.asarray(x[:n], dtype=np.float64)
    j = np.arange(m, dtype=np.int64)
    c, p = (j * D) // U, (j * D) % U
    prod = taps.astype(np.float64)[p] * xz[c[:, None] + np.arange(K)[None, :]]  # xz[c + k] is x[c - h + k]
    return prod.sum(axis=1), (K + 1) * EPS * np.abs(prod).sum(axis=1)


def wave_resample(wave, frames, T_cap, taps, U, D, spf=600, trim=0):
    """wave fp32 [B, L] -> (y, bound, offsets): every row's `polyphase`, back to back, and the int64 [B + 1] exclusive prefix
    sum of m_b."""
    n, m = row_counts(frames, T_cap, spf, trim, U, D)
    offsets = np.zeros(len(m) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(m)
    rows = [polyphase(np.asarray(wave[b], dtype=np.float32), n[b], taps, U, D) for b in range(len(n))]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), offsets


def pcm_interval(y, bound):
    """The int16 values a 16-bit conversion of a sample within `bound` of y may give: |v - 32767 clamp(y)| <= 0.5 + 32767
    bound.  -> (lo, hi) int64, lo <= hi."""
    t = 32767.0 * np.clip(y, -1.0, 1.0)
    w = 0.5 + 32767.0 * bound
    return np.maximum(np.ceil(t - w), -32767).astype(np.int64), np.minimum(np.floor(t + w), 32767).astype(np.int64)


# ---- ITU-T G.711 ------------------------------------------------------------------------------------------------------------
def _magnitude(v):
    v = np.asarray(v, dtype=np.int64)
    return np.where(v < 0, ~v, v), v < 0


def ulaw_encode(v):
    """int16 -> mu-law byte: 14-bit magnitude + bias 33, clipped at 0x1FFF; segment s is the one whose upper end 0x3F << s
    holds the value, the mantissa its four bits below the leading one; the byte is inverted, its top bit set for v >= 0."""
    mag, neg = _magnitude(v)
    a = np.minimum((mag >> 2) + 33, 0x1FFF)
    seg = np.zeros_like(a)
    for end in (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF):
        seg += a > end
    code = ((seg << 4) | ((a >> (seg + 1)) & 0xF)) ^ 0x7F
    return np.where(neg, code, code | 0x80).astype(np.uint8)


def ulaw_decode(code):
    """mu-law byte -> int16 (the centre of the code's interval, 16-bit scale)."""
    code = np.asarray(code, dtype=np.int64)
    inv = ~code & 0xFF
    exp, man = (inv >> 4) & 7, inv & 0xF
    step = 4 << (exp + 1)
    lin = (0x80 << exp) + step * man + step // 2 - 4 * 33
    return np.where(code < 0x80, -lin, lin)


def alaw_encode(v):
    """int16 -> A-law byte: 12-bit magnitude; below 16 it is the code (segment 0), above it segment e is the one whose upper
    end 0x1F << (e - 1) holds the value and the mantissa its four bits below the leading one; top bit set for v >= 0, then
    every other bit inverted (^ 0x55)."""
    mag, neg = _magnitude(v)
    ix = mag >> 4
    e = np.zeros_like(ix)
    for end in (0xF, 0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF):
        e += ix > end
    big = (ix >> np.maximum(e - 1, 0)) - 16 + (e << 4)
    code = np.where(e > 0, big, ix)
    return (np.where(neg, code, code | 0x80) ^ 0x55).astype(np.uint8)


def alaw_decode(code):
    code = np.asarray(code, dtype=np.int64)
    ix = (code ^ 0x55) & 0x7F
    exp, man = ix >> 4, ix & 0xF
    man = np.where(exp > 0, man + 16, man)
    lin = ((man << 4) + 8) << np.maximum(exp - 1, 0)
    return np.where(code > 127, lin, -lin)


ENCODE = {"ulaw": ulaw_encode, "alaw": alaw_encode}
DECODE = {"ulaw": ulaw_decode, "alaw": alaw_decode}


def half_step(code, law):
    """Half the quantisation step of the segment a code lies in, in 16-bit units."""
    code = np.asarray(code, dtype=np.int64)
    if law == "ulaw":
        return (4 << (((~code & 0xFF) >> 4 & 7) + 1)) // 2
    exp = ((code ^ 0x55) & 0x7F) >> 4
    return (16 << np.maximum(exp - 1, 0)) // 2


def rank(code, law):
    """A code's place in the order of the inputs that give it: non-decreasing in v for code = encode(v).  (Decoded values do
    not serve: mu-law has two codes for 0.)"""
    code = np.asarray(code, dtype=np.int64)
    u = code ^ (0xFF if law == "ulaw" else 0x55)  # bit 7: v < 0 for mu-law, v >= 0 for A-law; bits 0-6: the magnitude's index
    neg = (u & 0x80) != 0 if law == "ulaw" else (u & 0x80) == 0
    return np.where(neg, -1 - (u & 0x7F), u & 0x7F)
