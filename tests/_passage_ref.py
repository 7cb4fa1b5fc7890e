"""The contract of `st2_wave_pack_gaps` (include/st2.h) restated in numpy, from the contract and not from
the kernel: what tests/test_passage_gpu.py compares the kernel against.  A row's SPEECH is by contract byte for byte what the
wrapped entry (`st2_wave_pack` / `st2_wave_resample_pack`) writes for it, so the speech rows are an input here; what this file
states is the layout -- counts, clamps, 64-bit offsets, the write bound -- and the silence code of every format, taken from
the encoders of tests/_resample_ref.py / _syncfree_ref.py applied to a zero sample.  Not product code."""
import numpy as np

import _resample_ref as RR

DTYPES = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}


def silence(fmt):
    """cvt(0.0f) of a format: the element a gap is made of."""
    zero = np.zeros(1, dtype=np.float32)
    if fmt == "f32":
        return zero[0]
    v = RR.pcm16(zero)
    return v[0] if fmt == "s16" else RR.ENCODE[fmt](v)[0]


def clamp_gaps(gaps, gap_cap, B):
    """g_b = clamp(gaps[b], 0, gap_cap); None = no gaps."""
    if gaps is None or gap_cap == 0:
        return [0] * B
    return [min(max(int(g), 0), int(gap_cap)) for g in gaps]


def offsets(m, gaps, gap_cap):
    """offsets[b] = sum_{i < b} (m_i + g_i), int64 [B + 1]; offsets[B] includes the last row's gap."""
    g = clamp_gaps(gaps, gap_cap, len(m))
    off = np.zeros(len(m) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(m, dtype=np.int64) + np.asarray(g, dtype=np.int64))
    return off


def pack_gaps(rows, gaps, gap_cap, fmt, out_capacity=None):
    """rows: the speech of every row as the wrapped entry hands it over (arrays of the format's dtype, lengths m_b).
    -> (out, offsets, limit): out[:limit] is what the call must have written, limit = min(offsets[B], out_capacity); nothing
    at or past `limit` may be written."""
    dt = DTYPES[fmt]
    g = clamp_gaps(gaps, gap_cap, len(rows))
    off = offsets([len(r) for r in rows], gaps, gap_cap)
    z = silence(fmt)
    parts = []
    for r, g_b in zip(rows, g):
        parts.append(np.asarray(r, dtype=dt))
        parts.append(np.full(g_b, z, dtype=dt))
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    assert out.shape[0] == off[-1]
    limit = int(off[-1]) if out_capacity is None else min(int(off[-1]), int(out_capacity))
    return out[:limit], off, limit


def gap_samples(ms, rate):
    """rint(ms * rate / 1000), ties to even."""
    return int(np.rint(np.float64(ms) * rate / 1000.0))
