"""The contract of `st2_wave_dynamics` (include/st2.h) in numpy, with the order of every fp32 and fp64
operation written out, and once more as a plain per-block and per-sample loop (`brute_row`).  Not a test module.

Everything is fixed bit for bit except the last ulp of fp64 `log10` (rule 3) and `pow` (rule 7): `lin` is held to one fp32 ulp,
and `out_bound` is what that ulp can do to a sample.
"""
import numpy as np

from _breaks_ref import block_sums

F32, F64 = np.float32, np.float64
BLOCK = 64
FLT_MAX = F32(np.finfo(np.float32).max)
LOG_ULPS = 4  # the ulps of L = 10 log10(.) that a device's log10 may differ from numpy's by: either is within 1 ulp of the true
#               value, the product by 10 rounds once more, and the argument is the same double -- 2 ulps each way, doubled


def row_params(p):
    """params[b] -> (alone, T, slope, knee, makeup) as the kernels read them: fp32 clamps, then fp64."""
    p = np.asarray(p, dtype=F32)
    alone = bool(not np.isfinite(p[0]) or np.isnan(p[1:]).any())
    if alone:
        return True, 0.0, 0.0, 0.0, 0.0
    return (False, F64(p[0]), F64(np.clip(p[1], F32(0), F32(1))), F64(np.clip(p[2], F32(0), F32(40))),
            F64(np.clip(p[3], F32(-24), F32(24))))


def detector(s):
    """Rule 3: E[k] = fl32(fl32(s[k - 1] + s[k]) + s[k + 1]) with +inf as FLT_MAX, L[k] = 10 log10((double)E / 192), -inf at 0."""
    s = np.minimum(np.asarray(s, dtype=F32), FLT_MAX)
    z = np.zeros(1, dtype=F32)
    with np.errstate(over="ignore"):
        E = ((np.concatenate([z, s[:-1]]) + s).astype(F32) + np.concatenate([s[1:], z])).astype(F32)
    E = np.minimum(E, FLT_MAX)
    with np.errstate(divide="ignore"):
        return F64(10.0) * np.log10(E.astype(F64) / F64(192.0))


def curve(L, T, slope, knee):
    """Rule 4 in fp64: the soft-knee gain reduction in dB, >= 0."""
    L = np.asarray(L, dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        o = L - T
        u = o + knee / 2.0
        quad = (slope * (u * u)) / (2.0 * knee) if knee > 0 else np.zeros_like(o)
        c = np.where(2.0 * o <= -knee, 0.0, np.where(np.abs(2.0 * o) < knee, quad, slope * o))
    return np.where(np.isneginf(L), 0.0, c)


def release(c, rho, chunk=None):
    """Rule 5: g[k] = P[k] - fl64(k rho), P the running maximum of z[m] = c[m] + fl64(m rho).  `chunk`: the scan cut into pieces
    of that many blocks with a carry, which must not change a bit."""
    k = np.arange(len(c), dtype=F64)
    z = c + k * F64(rho)
    if chunk is None:
        P = np.maximum.accumulate(z)
    else:
        P, carry = np.empty_like(z), -np.inf
        for a in range(0, len(z), chunk):
            P[a:a + chunk] = np.maximum(np.maximum.accumulate(z[a:a + chunk]), carry)
            carry = P[min(a + chunk, len(z)) - 1]
    return P - k * F64(rho)


def release_without_carry(c, rho, chunk, halo):
    """What a chunked evaluation of rule 5 that LOSES its carry would give: the blocks [k0, k0 + chunk) of every chunk from a
    scan that starts afresh `halo` blocks in front of k0.  Not the contract: tests use it to show that a row has a release that
    crosses a chunk's start, so that a device that passes on it carries the scan."""
    k = np.arange(len(c), dtype=F64)
    z = c + k * F64(rho)
    g = np.empty_like(z)
    for k0 in range(0, len(z), chunk):
        a = max(k0 - halo, 0)
        g[k0:k0 + chunk] = (np.maximum.accumulate(z[a:k0 + chunk]) - k[a:k0 + chunk] * F64(rho))[k0 - a:]
    return g


def attack(g, A, win):
    """Rule 6: the hold over |d| <= A, the smoother's fp64 chain with j ascending and the nearest valid entry outside the row,
    d' = max(d, g)."""
    K = len(g)
    if A == 0:
        return g.copy()
    pad = np.concatenate([np.full(A, -np.inf), g, np.full(A, -np.inf)])
    m = pad[:K].copy()
    for j in range(1, 2 * A + 1):
        m = np.maximum(m, pad[j:j + K])
    win = np.asarray(win, dtype=F32).astype(F64)
    d = np.zeros(K, dtype=F64)
    for j in range(2 * A + 1):
        d = d + win[j] * m[np.clip(np.arange(K) - A + j, 0, K - 1)]
    return np.maximum(d, g)


def block_gain(dp, makeup):
    """Rule 7: lin[k] = fl32(10^((makeup - d') / 20)), rounded once."""
    return np.power(F64(10.0), (makeup - dp) / 20.0).astype(F32)


def _fma32(t, d, a):
    """fl32(t * d + a) with one rounding, for fp32 arrays: t has 8 bits, so the product is exact in fp64; the sum is rounded to
    odd in fp64 (TwoSum tells which way the exact value lies), which the rounding to fp32 then cannot double."""
    p = t.astype(F64) * d.astype(F64)
    a = a.astype(F64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def sample_gain(lin, n):
    """Rule 8's gain of samples 0 .. n - 1 from lin fp32 [K]: linear between the block centres 64 k + 31.5, flat outside them."""
    lin = np.asarray(lin, dtype=F32)
    K = len(lin)
    i = np.arange(n, dtype=np.int64)
    ka = (i >> 6) - ((i & 63) < 32)  # i lies between the centres of blocks ka and ka + 1
    la, lb = lin[np.clip(ka, 0, K - 1)], lin[np.clip(ka + 1, 0, K - 1)]
    t = ((2 * (i - 64 * ka) - 63).astype(F32) * F32(1.0 / 128.0)).astype(F32)
    return _fma32(t, (lb - la).astype(F32), la)


def apply_gain(x, lin):
    """Rule 8: out[i] = fl32(x[i] * gain[i]), with x itself."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (x * sample_gain(lin, len(x))).astype(F32)


def row_stages(x, p, A, win, rho, dL=0.0):
    """Every stage of one row of valid samples x under params p -> dict, or None for a row that is left alone or empty.  `dL`
    is added to the detector's level: the brackets of `count_bounds`."""
    x = np.asarray(x, dtype=F32)
    alone, T, slope, knee, makeup = row_params(p)
    if alone or len(x) == 0:
        return None
    s = block_sums(x)
    L = detector(s) + dL
    c = curve(L, T, slope, knee)
    g = release(c, rho)
    dp = attack(g, A, win)
    return dict(s=s, L=L, c=c, g=g, dp=dp, lin=block_gain(dp, makeup))


def reference_row(x, p, A, win, rho):
    """-> (out fp32 [n], dyn fp32 [2], stages): the whole contract for one row.  A row left alone is its own bits, {0, 0}."""
    x = np.asarray(x, dtype=F32)
    st = row_stages(x, p, A, win, rho)
    if st is None:
        return x.copy(), np.zeros(2, dtype=F32), None
    return apply_gain(x, st["lin"]), np.array([st["dp"].max(), np.count_nonzero(st["dp"] > 0)], dtype=F32), st


def count_bounds(x, p, A, win, rho):
    """(lo, hi) of dyn[b][1].  d' does not fall when a level rises -- the curve, the rounded sum z, the maxima and the chain
    with non-negative weights are all monotone -- so the contract evaluated with every L lowered and raised by LOG_ULPS ulps
    brackets the d' of a device whose log10 is off by that much.  The blocks that are > 0 in the upper and not in the lower
    evaluation are exactly those whose d' sits within rounding of 0; lo == hi where there are none."""
    st = row_stages(x, p, A, win, rho)
    if st is None:
        return 0, 0
    fin = st["L"][np.isfinite(st["L"])]
    eps = LOG_ULPS * np.spacing(np.abs(fin).max()) if len(fin) else 0.0
    lo = row_stages(x, p, A, win, rho, -eps)["dp"] > 0
    hi = row_stages(x, p, A, win, rho, +eps)["dp"] > 0
    return int(np.count_nonzero(lo)), int(np.count_nonzero(hi))


def ulp_diff(a, b):
    """|a - b| in fp32 ulps for finite fp32 arrays of one sign pattern (the distance of their ordered bit patterns)."""
    a = np.ascontiguousarray(a, dtype=F32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=F32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def out_bound(x, lin):
    """What one fp32 ulp of every lin[k] can move a sample by.  gain = fl32(la + t (lb - la)) with 0 <= t <= 1: moving la and lb by
    one ulp each moves the exact value by at most (1 - t) ulp(la) + t ulp(lb) <= u = max ulp of the two, the difference lb - la
    (rounded: half an ulp of it, at most u / 2 again) by t u / 2, and the final rounding by at most u / 2 more -- 2 u in all;
    the product x gain then moves by |x| 2 u and rounds once more, half an ulp of the result.  -> fp32 [n]: |x| 2 u + ulp(|x| gain)."""
    x = np.asarray(x, dtype=F32)
    lin = np.asarray(lin, dtype=F32)
    K, n = len(lin), len(x)
    i = np.arange(n, dtype=np.int64)
    ka = (i >> 6) - ((i & 63) < 32)
    la, lb = lin[np.clip(ka, 0, K - 1)], lin[np.clip(ka + 1, 0, K - 1)]
    u = np.spacing(np.maximum(la, lb)).astype(F64)
    ax = np.abs(np.where(np.isfinite(x), x, F32(0))).astype(F64)
    return ax * 2.0 * u + np.spacing((ax * (np.maximum(la, lb).astype(F64) + 2.0 * u)).astype(F32)).astype(F64)


def brute_row(x, p, A, win, rho):
    """The contract once more as plain loops over blocks and samples, in Python floats (fp64) and explicit fp32 roundings."""
    x = np.asarray(x, dtype=F32)
    n = len(x)
    alone, T, slope, knee, makeup = row_params(p)
    if alone or n == 0:
        return x.copy(), np.zeros(2, dtype=F32)
    K = (n + BLOCK - 1) // BLOCK
    s = block_sums(x)
    c = []
    for k in range(K):
        sm = min(s[k - 1], FLT_MAX) if k > 0 else F32(0)
        sp = min(s[k + 1], FLT_MAX) if k + 1 < K else F32(0)
        with np.errstate(over="ignore"):
            E = min(F32(F32(sm + min(s[k], FLT_MAX)) + sp), FLT_MAX)
        if not E > 0:
            c.append(0.0)
            continue
        o = float(F64(10.0) * np.log10(F64(E) / F64(192.0))) - float(T)
        if 2.0 * o <= -knee:
            c.append(0.0)
        elif abs(2.0 * o) < knee:
            u = o + float(knee) / 2.0
            c.append((float(slope) * (u * u)) / (2.0 * float(knee)))
        else:
            c.append(float(slope) * o)
    g = []
    for k in range(K):  # the release as its definition says it: a maximum over every earlier block
        g.append(max(c[m] + m * float(rho) for m in range(k + 1)) - k * float(rho))
    dp = []
    for k in range(K):
        if A == 0:
            dp.append(g[k])
            continue
        d = 0.0
        for j in range(2 * A + 1):
            q = min(max(k - A + j, 0), K - 1)
            d = d + float(F64(F32(win[j]))) * max(g[e] for e in range(max(q - A, 0), min(q + A, K - 1) + 1))
        dp.append(max(d, g[k]))
    lin = [F32(np.power(F64(10.0), (F64(makeup) - F64(v)) / F64(20.0))) for v in dp]
    out = np.empty(n, dtype=F32)
    for i in range(n):
        k, r = divmod(i, BLOCK)
        ka = k - 1 if r < 32 else k
        la, lb = lin[min(max(ka, 0), K - 1)], lin[min(max(ka + 1, 0), K - 1)]
        t = F32(2 * (i - BLOCK * ka) - 63) / F32(128)
        gain = _fma32(np.array([t], dtype=F32), np.array([F32(lb - la)], dtype=F32), np.array([la], dtype=F32))[0]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            out[i] = F32(x[i] * gain)
    return out, np.array([max(dp), sum(1 for v in dp if v > 0)], dtype=F32)
