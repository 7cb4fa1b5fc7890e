"""fp64 reference of one operand-range telemetry row (include/st2.h `st2_debug_headroom_read`, columns [6]..[9]) and of the split
planes it is computed from, in plain numpy: no device code, nothing of the kernel's.  tests/test_headroom_ref_cpu.py proves it on
hand-made planes; tests/test_headroom_edges_gpu.py holds the device to it.

A row describes the two float16 planes of ONE launch, hi and lo, each [B][cg][Lp][8] (16-byte slots of 8 channels; the operand is
u = hi + lo, exact in fp32 and so in fp64 for planes a split wrote: lo is at most half an ulp of hi):
    [6] max |hi|                       [7] max |hi| / 65504
    [8] sqrt(sum ulp(lo)^2 / 12 / sum u^2), ulp(lo) = 2^(e - 10) for a normal lo = m 2^e (1 <= m < 2), 2^-24 for |lo| < 2^-14
    [9] sum of u^2 over the elements with |lo| < 2^-14 (a subnormal or zero lo half) / sum u^2
Elements with hi = lo = 0 (padding, exact zeros) enter no sum; a launch without any other element has [8] = [9] = 0.
Every sum is math.fsum over fp64 terms that are exact (u^2: a 48-bit product; ulp^2: a power of two) or rounded once (the
division by 12), so the reference carries an error of a few 2^-53 whatever the number of terms."""
import math

import numpy as np

from _prologue_ref import split_f16  # the numpy model of st2_split_f16 (proved by tests/test_prologue_ref_cpu.py)

F16_MAX = 65504.0
LO_NORMAL_MIN = 2.0 ** -14
PRO_NONE, PRO_LEAKY = 0, 1  # include/st2.h ST2_PRO_NONE / ST2_PRO_LEAKY: the two prologues numpy reproduces bit for bit


def ulp_lo(lo):
    """Spacing of the f16 grid at lo (fp64 array): 2^(e - 10) for |lo| = m 2^e >= 2^-14, 2^-24 below."""
    a = np.abs(np.asarray(lo, dtype=np.float64))
    _, e = np.frexp(np.maximum(a, LO_NORMAL_MIN))  # a = f 2^e with f in [0.5, 1): the exponent of m in [1, 2) is e - 1
    return np.where(a < LO_NORMAL_MIN, 2.0 ** -24, np.ldexp(1.0, e - 1 - 10))


def sums(hi, lo):
    """(max |hi|, sum u^2, sum ulp(lo)^2 / 12, sum u^2 over |lo| < 2^-14) of two float16 arrays of one shape."""
    hi = np.asarray(hi)
    lo = np.asarray(lo)
    assert hi.dtype == np.float16 and lo.dtype == np.float16 and hi.shape == lo.shape
    h, l = hi.astype(np.float64).ravel(), lo.astype(np.float64).ravel()
    m = float(np.abs(h).max()) if h.size else 0.0
    live = ~((h == 0.0) & (l == 0.0))
    h, l = h[live], l[live]
    u2 = (h + l) ** 2
    sub = np.abs(l) < LO_NORMAL_MIN
    e2 = ulp_lo(l) ** 2 * (1.0 / 12.0)
    return m, math.fsum(u2), math.fsum(e2), math.fsum(u2[sub])


def row(hi, lo):
    """{max_abs, frac, rel_err, sub_share}: columns [6]..[9] of the row the launch that wrote (hi, lo) leaves, under the names
    `ops.headroom` gives them."""
    m, su2, se2, ssub = sums(hi, lo)
    return {"max_abs": m, "frac": m / F16_MAX,
            "rel_err": math.sqrt(se2 / su2) if su2 > 0.0 else 0.0,
            "sub_share": ssub / su2 if su2 > 0.0 else 0.0}


def expected_planes(x, x_scale, halo=0, lengths=None, pro=PRO_NONE, slope=0.0, cg=None, Lp=None):
    """(hi, lo) float16 [B][cg][Lp][8] that st2_act_split writes for x [B, C, L] (fp32 array) under PRO_NONE / PRO_LEAKY:
    u = x_scale * pro(x) in fp32 (LeakyReLU: x >= 0 ? x : x * slope, then the scale: one fp32 rounding each), zero at and past
    lengths[b] (clamped to 0 .. L), in the `halo` columns in front, up to Lp and for channels >= C, clamped to +-65504 (a NaN
    becomes -65504), hi = f16(u), lo = f16(u - hi).  cg / Lp default to the smallest planes that hold the tensor: padding adds
    nothing to a row."""
    assert pro in (PRO_NONE, PRO_LEAKY)
    x = np.asarray(x, dtype=np.float32)
    B, C, L = x.shape
    cg = (C + 7) // 8 if cg is None else cg
    Lp = halo + L if Lp is None else Lp
    assert cg * 8 >= C and Lp >= halo + L
    with np.errstate(invalid="ignore", over="ignore"):
        v = x if pro == PRO_NONE else np.where(x >= 0, x, (x * np.float32(slope)).astype(np.float32))
        u = (v * np.float32(x_scale)).astype(np.float32)
    u = u.copy()
    for b in range(B):
        end = L if lengths is None else min(max(int(lengths[b]), 0), L)
        u[b, :, end:] = 0.0  # a select, not a multiply: a NaN or an inf past the row's end is padding like any other value
    h, l, _ = split_f16(u)
    hi = np.zeros((B, cg, Lp, 8), dtype=np.float16)
    lo = np.zeros((B, cg, Lp, 8), dtype=np.float16)
    for c in range(C):
        hi[:, c // 8, halo:halo + L, c % 8] = h[:, c]
        lo[:, c // 8, halo:halo + L, c % 8] = l[:, c]
    return hi, lo


def planes_of(data):
    """XsTensor.data [B, 2, cg, Lp, 8] (a CPU float16 tensor: what `ops.activate` returned for the same input and lengths) ->
    (hi, lo) numpy [B][cg][Lp][8]."""
    a = data.numpy()
    return a[:, 0], a[:, 1]
