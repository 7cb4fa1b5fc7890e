"""The contract of `st2_wave_breaks` and `st2_token_marks_breaks` (include/st2.h) restated in numpy, and the
constructed rows that tests/test_breaks_cpu.py and tests/test_breaks_gpu.py share.  The fp32 order the kernels are bit-exact to
-- rule 2 of the header -- is written out: `block_sums` is one fp32 multiply per sample and the 6 butterfly steps of a block;
everything behind it is integers and single fp32 operations.  `brute_row` is the same contract as plain loops over samples, the
squares in exact rational arithmetic rounded by hand (`_edges_ref.round32`), the positions in Python integers: what the
vectorised form is checked against.  Not product code."""
import fractions
import functools

import numpy as np

from _edges_ref import NAN_PAYLOAD, SENTINEL, _tone, round32, row_samples

F32 = np.float32
BLOCK = 64


# ---- rules 1 - 4 -----------------------------------------------------------------------------------------------------------------
def clean(x):
    x = np.asarray(x, dtype=F32)
    return np.where(np.isfinite(x), x, F32(0.0)).astype(F32)


def block_sums(x):
    """fp32 [ceil(n / 64)]: lane l squares sample 64 k + l (zeros past n), the 64 squares are folded by a butterfly,
    t[l] += t[l ^ off] for off = 32, 16, ..., 1 (every lane ends with the same bits)."""
    x = clean(x)
    nblk = (len(x) + BLOCK - 1) // BLOCK
    v = np.zeros(nblk * BLOCK, dtype=F32)
    v[:len(x)] = x
    with np.errstate(over="ignore"):
        s = (v * v).astype(F32).reshape(nblk, BLOCK)
        lane = np.arange(BLOCK)
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, lane ^ off]).astype(F32)
    return s[:, 0]


def boundaries(pos, n):
    """q[0] = 0, q[N] = n, the rest clamped to 0..n, then the running maximum."""
    q = np.clip(np.asarray(pos, dtype=np.int64), 0, n)
    q[0], q[-1] = 0, n
    return np.maximum.accumulate(q)


def cut_of(s, p0, p1):
    """The cut of a span [p0, p1): 64 k for the smallest e_k = s[k - 1] + s[k] over 64 (k - 1) >= p0, 64 (k + 1) <= p1, ties to
    the smallest k; the middle without a candidate."""
    k_lo, k_hi = (p0 + BLOCK - 1) // BLOCK + 1, p1 // BLOCK - 1
    if k_hi < k_lo:
        return (p0 + p1) // 2
    k = np.arange(k_lo, k_hi + 1)
    with np.errstate(over="ignore"):
        e = (s[k - 1] + s[k]).astype(F32)
    return BLOCK * int(k[int(np.argmin(e))])  # argmin: the first of equal minima


def plan(x, pos, brk, max_break):
    """-> (ins int [N], cuts int [N]) of a row of len(x) valid samples."""
    n, N = len(x), len(brk)
    q = boundaries(pos, n)
    s = block_sums(x)
    ins, cuts, done = np.zeros(N, dtype=np.int64), np.full(N, -1, dtype=np.int64), 0
    for i in range(N):
        ins[i] = min(max(int(brk[i]), 0), max_break - done)
        done += int(ins[i])
        if ins[i] > 0:
            cuts[i] = cut_of(s, int(q[i]), int(q[i + 1]))
    return ins, cuts


# ---- rule 5 ----------------------------------------------------------------------------------------------------------------------
def move(x, ins, cuts, ramp):
    """The row with its breaks as uint32 bit patterns: the segments between the cuts copied, but for one fp32 multiply on the
    samples of a fade at a cut, and zeros behind every cut."""
    x = np.asarray(x, dtype=F32)
    n = len(x)
    live = [i for i in range(len(ins)) if ins[i] > 0]
    a = [0] + [int(cuts[i]) for i in live] + [n]
    m = len(live)
    F = 0 if ramp is None else len(ramp)
    parts = []
    for j in range(m + 1):
        if j > 0:
            parts.append(np.zeros(int(ins[live[j - 1]]), dtype=np.uint32))
        seg = x[a[j]:a[j + 1]].copy()
        bits = seg.view(np.uint32).copy()
        f = min(F, len(seg) // 2)
        if f and j > 0:
            bits[:f] = (seg[:f] * ramp[:f]).astype(F32).view(np.uint32)
        if f and j < m:
            bits[len(seg) - f:] = (seg[len(seg) - f:] * ramp[:f][::-1]).astype(F32).view(np.uint32)
        parts.append(bits)
    return np.concatenate(parts)


def breaks_row(x, pos, brk, max_break, ramp):
    """x: the row's n_b valid samples -> dict(ins, cuts, count, total, bits uint32 [count])."""
    ins, cuts = plan(x, pos, brk, max_break)
    bits = move(x, ins, cuts, ramp)
    assert len(bits) == len(x) + int(ins.sum())
    return dict(ins=ins, cuts=cuts, count=len(bits), total=int(ins.sum()), bits=bits)


def breaks_batch(wave, frames, T_cap, spf, trim, pos, brk, max_break, ramp):
    """wave [B, >= spf T_cap] -> the rows' dicts."""
    return [breaks_row(wave[b, :row_samples(frames[b], T_cap, spf, trim)], pos[b], brk[b], max_break, ramp) for b in range(len(frames))]


def marks(pos, ins, U=1, D=1):
    """marks[b][n] = ceil((pos[b][n] + sum_{m < n} ins[b][m]) U / D); a negative entry counts as 0."""
    pos, ins = np.maximum(np.asarray(pos, dtype=np.int64), 0), np.maximum(np.asarray(ins, dtype=np.int64), 0)
    before = np.concatenate([np.zeros((len(ins), 1), dtype=np.int64), np.cumsum(ins, axis=1)], axis=1)
    return np.minimum(((pos + before) * U + D - 1) // D, 2 ** 31 - 1)


# ---- the same contract, sample by sample -----------------------------------------------------------------------------------------
def brute_row(x, pos, brk, max_break, ramp):
    """`breaks_row` as plain loops: every block sum lane by lane, every candidate, every output sample."""
    xs = [F32(v) for v in np.asarray(x, dtype=F32)]
    n, N = len(xs), len(brk)
    q, top = [], 0
    for i in range(N + 1):
        v = 0 if i == 0 else n if i == N else min(max(int(pos[i]), 0), n)
        top = max(top, v)
        q.append(top)
    sums = []
    with np.errstate(over="ignore"):
        for blk in range((n + BLOCK - 1) // BLOCK):
            lanes = []
            for l in range(BLOCK):
                k = blk * BLOCK + l
                v = xs[k] if k < n and np.isfinite(xs[k]) else F32(0.0)
                sq = fractions.Fraction(float(v)) ** 2
                lanes.append(F32(np.inf) if sq >= fractions.Fraction(2) ** 128 else round32(sq))
            for off in (32, 16, 8, 4, 2, 1):
                lanes = [F32(lanes[l] + lanes[l ^ off]) for l in range(BLOCK)]
            sums.append(lanes[0])
    ins, cuts, done = [], [], 0
    for i in range(N):
        w = min(max(int(brk[i]), 0), max_break - done)
        done += w
        ins.append(w)
        if w == 0:
            cuts.append(-1)
            continue
        best = None
        k = 1
        while BLOCK * (k + 1) <= q[i + 1]:
            if BLOCK * (k - 1) >= q[i]:
                with np.errstate(over="ignore"):
                    e = F32(sums[k - 1] + sums[k])
                if best is None or e < best[0]:
                    best = (e, k)
            k += 1
        cuts.append(BLOCK * best[1] if best else (q[i] + q[i + 1]) // 2)
    at = sorted(set(c for c in cuts if c >= 0))  # where the row is cut
    F = 0 if ramp is None else len(ramp)
    bits = []
    for i in range(n + 1):
        for t in range(N):  # the silence of the cuts in front of sample i, in token order
            if cuts[t] == i:
                bits.extend([0] * ins[t])
        if i == n:
            break
        start = max([c for c in at if c <= i], default=None)
        end = min([c for c in at if c > i], default=None)
        lo, hi = 0 if start is None else start, n if end is None else end
        f = min(F, (hi - lo) // 2)
        v = xs[i]
        if start is not None and i - lo < f:
            v = F32(v * ramp[i - lo])
        elif end is not None and hi - 1 - i < f:
            v = F32(v * ramp[hi - 1 - i])
        bits.append(int(np.array(v, dtype=F32).view(np.uint32)))
    return dict(ins=np.array(ins, dtype=np.int64), cuts=np.array(cuts, dtype=np.int64), count=len(bits), total=done,
                bits=np.array(bits, dtype=np.uint32))


# ---- the constructed rows --------------------------------------------------------------------------------------------------------
GEOMETRY = (5, 700)  # (samples_per_frame, T_cap): 3 500 samples at capacity, more than one tile of the sums' launch
TRIM = 3
MAX_BREAK = 450
BATCHES = [1, 5, 17]
TOKENS = [1, 7, 512]
FADES = [0, 1, 48]
SIZES = [0, 63, 64, 127, 128, 129, 4095, 4096, 4097]
PLAIN = [0, 400, 900, 1000, 1800, 2500, 3000, 0]  # the last boundary is the row's end whatever stands here

# kind -> (pos of 7 tokens, brk): what the issue lists, one row each
KINDS = [
    ("plain", PLAIN, [0, 0, 240, 0, 0, 100, 0]),
    ("empty spans", [0, 500, 500, 500, 1200, 1201, 2000, 0], [0, 50, 60, 0, 70, 0, 0]),            # two cuts at 500, one in a 1-sample span
    ("short spans", [0, 64, 191, 300, 427, 1000, 1100, 0], [0, 10, 0, 20, 0, 30, 0]),              # 127 / 127 / 100 samples: no window
    ("128 samples", [0, 128, 256, 1000, 1128, 2000, 2129, 0], [5, 7, 0, 9, 0, 11, 0]),             # aligned: one candidate; unaligned: none
    ("whole row", [0, 0, 0, 0, 99999, 99999, 99999, 0], [0, 0, 0, 300, 0, 0, 0]),                  # token 3 covers the row
    ("none asked", PLAIN, [-5, 0, -1, 0, 0, 0, -2 ** 31]),
    ("adjacent", PLAIN, [0, 0, 100, 120, 0, 0, 0]),
    ("close cuts", [0, 1000, 1030, 1060, 1090, 2000, 3000, 0], [0, 33, 0, 44, 0, 0, 0]),            # cuts 60 samples apart: less than 2 F
    ("cap", PLAIN, [0, 100, 0, 0, 400, 0, 50]),                                                      # reached inside token 4, token 6 dropped
    ("zero span", PLAIN, [0, 0, 0, 77, 0, 0, 0]),                                                    # every window equal: the smallest k
    ("non-finite", PLAIN, [0, 0, 0, 60, 0, 0, 0]),
    ("no break", PLAIN, [0] * 7),
    ("frames 0", PLAIN, [0, 10, 0, 0, 0, 0, 20]),
    ("bad pos", [77, 900, 400, -5, 99999, 2500, 2400, 12], [40, 0, 50, 0, 0, 60, 0]),               # clamped, made monotone
    ("short row", [0, 10, 20, 50, 60, 90, 95, 0], [0, 0, 3, 0, 0, 4, 0]),
    ("plain", PLAIN, [90, 0, 0, 0, 110, 0, 250]),                                                    # the cap met exactly
    ("adjacent", PLAIN, [0, 0, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0]),                                  # a 64-bit sum of the asked breaks
]


def _signal(L, n, kind, seed):
    """Speech-like: a tone under a slow envelope with dips (quiet places inside every span), over a faint noise floor."""
    g = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    env = 0.05 + 0.95 * np.abs(np.sin(2 * np.pi * t / (300.0 + 7 * (seed % 13)) + g.uniform(0, 6)))
    x = np.zeros(L, dtype=np.float64)
    x[:n] = _tone(n, seed) * env + 2e-5 * g.standard_normal(n)
    if kind == "zero span":
        x[1000:2000] = 0.0
    out = x.astype(F32)
    if kind == "non-finite" and n > 1700:
        out[1500] = np.array([NAN_PAYLOAD], dtype=np.uint32).view(F32)[0]
        out[1600], out[1601] = np.inf, -np.inf
        out[1100] = F32(3e30)  # its square is past fp32: the window is +inf, never NaN
    out[n:] = np.nan  # nothing at or past n_b is read
    return out


def _tokens(kind_row, N, n, seed):
    """pos int [N + 1], brk int [N] of a row: the constructed kind at N = 7, one span at N = 1, seeded random ones at N = 512."""
    name, pos, brk = kind_row
    if N == 7:
        return list(pos), list(brk)
    if N == 1:
        return [5, 3], [[100, 0, 450, 500, -3][seed % 5]]  # both boundaries are replaced: 0 and n_b
    g = np.random.default_rng(seed)
    p = np.sort(g.integers(0, n + 1, size=N + 1))
    p[g.integers(1, N, size=6)] = g.integers(-50, n + 200, size=6)  # out of order and out of range
    b = np.zeros(N, dtype=np.int64)
    where = g.choice(N, size=14, replace=False)
    b[where] = g.integers(1, 70, size=14)
    b[g.integers(0, N, size=3)] = -7
    if name in ("no break", "none asked"):
        b = np.minimum(b, 0)
    return p.tolist(), b.tolist()


@functools.lru_cache(maxsize=None)
def batch(B, N):
    """-> dict(wave fp32 [B, 3500], frames, pos int32 [B, N + 1], brk int32 [B, N], names): row b is KINDS[b]."""
    spf, T_cap = GEOMETRY
    L = spf * T_cap
    wave, frames, pos, brk = np.zeros((B, L), dtype=F32), [], [], []
    for b in range(B):
        name = KINDS[b][0]
        fr = {"frames 0": 0, "short row": 20}.get(name, T_cap - (b % 3) * 77)
        n = row_samples(fr, T_cap, spf, TRIM)
        wave[b] = _signal(L, n, name, 100 * N + b)
        p, k = _tokens(KINDS[b], N, n, 100 * N + b)
        frames.append(fr), pos.append(p), brk.append(k)
    return dict(wave=wave, frames=np.array(frames, dtype=np.int32), pos=np.array(pos, dtype=np.int64).astype(np.int32),
                brk=np.array(brk, dtype=np.int64).astype(np.int32), names=[k[0] for k in KINDS[:B]], spf=spf, T_cap=T_cap, trim=TRIM,
                max_break=MAX_BREAK)


@functools.lru_cache(maxsize=None)
def sizes_batch():
    """Rows of exactly SIZES valid samples, as rows of one-sample frames (the geometry the hand-over runs the later steps in),
    seven tokens each at fixed fractions of the row, four of them with a break."""
    T_cap = 4100
    wave = np.zeros((len(SIZES), T_cap), dtype=F32)
    pos = []
    for b, n in enumerate(SIZES):
        wave[b] = _signal(T_cap, n, "plain", 900 + b)
        pos.append([0, n // 5, n // 3, n // 2, n // 2, 2 * n // 3, max(n - 1, 0), n])
    return dict(wave=wave, frames=np.array(SIZES, dtype=np.int32), pos=np.array(pos, dtype=np.int32),
                brk=np.tile(np.array([[0, 30, 0, 17, 9, 0, 5]], dtype=np.int32), (len(SIZES), 1)), names=["n = %d" % n for n in SIZES],
                spf=1, T_cap=T_cap, trim=0, max_break=MAX_BREAK)


def case(B, N):
    return batch(B, N) if B else sizes_batch()


@functools.lru_cache(maxsize=None)
def reference(B, N, F):
    """The rows' reference for `batch(B, N)` (B > 0) or `sizes_batch` (B = 0), computed once and shared."""
    from styletts2_amd import resample
    c = case(B, N)
    ramp = resample.edge_ramp_design(F) if F else None
    return breaks_batch(c["wave"], c["frames"], c["T_cap"], c["spf"], c["trim"], c["pos"], c["brk"], c["max_break"], ramp)
