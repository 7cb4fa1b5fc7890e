"""The contract of `st2_wave_volume` (include/st2.h) in numpy, with the order of every fp32 and fp64
operation written out, and once more as a plain per-block and per-sample loop (`brute_row`).  Not a test module.

Everything is fixed bit for bit except the last ulp of fp64 `pow` (rule 4): `lin` is held to one fp32 ulp, and the samples to
bits over the device's own `lin` (`apply_gain`), the method of tests/_dynamics_ref.py, whose rule 8 is rule 5 here.
"""
import numpy as np

from _dynamics_ref import _fma32, sample_gain, ulp_diff  # noqa: F401 -- rule 5 is st2_wave_dynamics's rule 8, stated there

F32, F64 = np.float32, np.float64
BLOCK = 64
DB_LO, DB_HI = F32(-60.0), F32(20.0)


def clean(v):
    """Rule 1 in fp32: NaN -> 0, then clamped to [-60, +20]; -inf -> -60, +inf -> +20."""
    v = np.asarray(v, dtype=F32)
    return np.where(np.isnan(v), F32(0), np.minimum(np.maximum(v, DB_LO), DB_HI)).astype(F32)


def token_of_block(pos, Nb, n):
    """Rule 2's idx for every block of a row of n samples: the largest i in [0, Nb) with pos[i] <= c, c = min(64 k + 32, n - 1),
    0 if there is none.  pos does not decrease."""
    K = (n + BLOCK - 1) // BLOCK
    c = np.minimum(64 * np.arange(K, dtype=np.int64) + 32, n - 1)
    if Nb <= 0:
        return np.zeros(K, dtype=np.int64)
    return np.maximum(np.searchsorted(np.asarray(pos[:Nb], dtype=np.int64), c, side="right") - 1, 0)


def wanted(n, pos, Nb, db, tok_db):
    """Rule 2: d fp64 [K].  `db` a number or None, `tok_db` fp32 [N] or None."""
    K = (n + BLOCK - 1) // BLOCK
    row = F64(clean(db)) if db is not None else F64(0.0)
    tok = np.zeros(K, dtype=F64)
    if tok_db is not None and Nb > 0:
        tok = clean(tok_db)[token_of_block(pos, Nb, n)].astype(F64)
    return np.minimum(np.maximum(row + tok, F64(-60.0)), F64(20.0))


def smooth(d, A, win):
    """Rule 3: e[k] = d[k] + acc, acc = sum over j = -A .. A in order of fl64(win[j + A] * (d[clamp(k + j)] - d[k]))."""
    K = len(d)
    if A == 0:
        return d + F64(0.0)
    w = np.asarray(win, dtype=F32).astype(F64)
    k = np.arange(K)
    acc = np.zeros(K, dtype=F64)
    for j in range(-A, A + 1):
        acc = acc + w[j + A] * (d[np.clip(k + j, 0, K - 1)] - d)
    return d + acc


def block_gain(e):
    """Rule 4: 0 at or under -60 dB, else fl32(10^(e / 20)), rounded once."""
    return np.where(e <= -60.0, F32(0), np.power(F64(10.0), e / 20.0).astype(F32)).astype(F32)


def apply_gain(x, lin):
    """Rules 5 and 6 over a given lin fp32 [K]: out[i] = fl32(x[i] * gain[i]) with x itself, and x's own word where both block
    gains of the sample are exactly 1."""
    x = np.ascontiguousarray(x, dtype=F32)
    lin = np.asarray(lin, dtype=F32)
    n, K = len(x), len(lin)
    if n == 0:
        return x.copy()
    i = np.arange(n, dtype=np.int64)
    ka = (i >> 6) - ((i & 63) < 32)
    keep = (lin[np.clip(ka, 0, K - 1)] == 1) & (lin[np.clip(ka + 1, 0, K - 1)] == 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = (x * sample_gain(lin, n)).astype(F32)
    return np.where(keep, x.view(np.uint32), y.view(np.uint32)).astype(np.uint32).view(F32)


def report(out, lin):
    """Rule 8: {max |out| with NaN ignored, 0 for an empty row; the number of blocks with lin != 1} as fp32 [2]."""
    a = np.abs(np.asarray(out, dtype=F32))
    a = a[~np.isnan(a)]
    return np.array([a.max() if len(a) else 0.0, np.count_nonzero(np.asarray(lin, dtype=F32) != 1)], dtype=F32)


def row_stages(n, pos, Nb, db, tok_db, A, win):
    """d, e and lin of one row of n valid samples -> dict (empty arrays for n = 0)."""
    if n == 0:
        z = np.zeros(0, dtype=F64)
        return dict(d=z, e=z, lin=np.zeros(0, dtype=F32))
    d = wanted(n, pos, Nb, db, tok_db)
    e = smooth(d, A, win)
    return dict(d=d, e=e, lin=block_gain(e))


def reference_row(x, pos, Nb, db, tok_db, A, win):
    """-> (out fp32 [n], vol fp32 [2], stages): the whole contract for one row of valid samples x."""
    x = np.ascontiguousarray(x, dtype=F32)
    st = row_stages(len(x), pos, Nb, db, tok_db, A, win)
    out = apply_gain(x, st["lin"])
    return out, report(out, st["lin"]), st


def brute_row(x, pos, Nb, db, tok_db, A, win):
    """The contract once more as plain loops over blocks and samples, in Python floats (fp64) and explicit fp32 roundings."""
    x = np.ascontiguousarray(x, dtype=F32)
    n = len(x)
    if n == 0:
        return x.copy(), np.zeros(2, dtype=F32), np.zeros(0, dtype=F32)
    K = (n + BLOCK - 1) // BLOCK

    def cl(v):
        v = F32(v)
        return 0.0 if v != v else float(min(max(v, DB_LO), DB_HI))
    row = cl(db) if db is not None else 0.0
    d = []
    for k in range(K):
        c = min(64 * k + 32, n - 1)
        t = 0.0
        if tok_db is not None and Nb > 0:
            idx = 0
            for i in range(Nb):
                if int(pos[i]) <= c:
                    idx = i
            t = cl(tok_db[idx])
        d.append(min(max(row + t, -60.0), 20.0))
    lin = []
    for k in range(K):
        acc = 0.0
        if A > 0:
            for j in range(-A, A + 1):
                acc = acc + float(F64(F32(win[j + A]))) * (d[min(max(k + j, 0), K - 1)] - d[k])
        e = d[k] + acc
        lin.append(F32(0) if e <= -60.0 else F32(np.power(F64(10.0), F64(e) / F64(20.0))))
    out = np.empty(n, dtype=F32)
    peak = F32(0)
    for i in range(n):
        k, r = divmod(i, BLOCK)
        ka = k - 1 if r < 32 else k
        la, lb = lin[min(max(ka, 0), K - 1)], lin[min(max(ka + 1, 0), K - 1)]
        if la == 1 and lb == 1:
            out[i:i + 1].view(np.uint32)[0] = x[i:i + 1].view(np.uint32)[0]
        else:
            t = F32(2 * (i - BLOCK * ka) - 63) / F32(128)
            gain = _fma32(np.array([t], dtype=F32), np.array([F32(lb - la)], dtype=F32), np.array([la], dtype=F32))[0]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                out[i] = F32(x[i] * gain)
        if abs(out[i]) > peak:  # false for a NaN
            peak = abs(out[i])
    return out, np.array([peak, sum(1 for v in lin if v != 1)], dtype=F32), np.array(lin, dtype=F32)
