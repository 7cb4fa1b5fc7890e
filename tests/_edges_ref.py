"""The contract of `st2_wave_edges` and `st2_token_marks_edges` (include/st2.h) restated in numpy, and the
constructed rows that tests/test_edges_cpu.py and tests/test_edges_gpu.py share.  The hop and the frame of the trim rule are
`_ingest_ref`'s; that file states the rule in fp64 (its tests allow for frames near the threshold), so the fp32 order the
kernels are bit-exact to -- rule 2 of the header -- is written out here: `fma32` is one correctly rounded fp32 fused
multiply-add, `block_sums` the 8 fmaf steps per lane and the 6 butterfly steps of a block.  `brute_*` is the same contract as
a plain loop over samples, with exact rational arithmetic rounded by hand: what the vectorised form is checked against.  Not
product code."""
import fractions
import functools

import numpy as np

import _marks_ref as M
from _ingest_ref import FRAME, HOP

F32 = np.float32
FLOOR = F32(1e-10)


# ---- rule 2: detection ---------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c) for non-negative fp32 arrays, one rounding: the product is exact in fp64 (48 bits), its sum with c is
    rounded to odd in fp64 (TwoSum gives the error's sign) and then to nearest-even in fp32 -- 53 >= 2 * 24 + 2 bits make the
    double rounding innocuous."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    hi = p + c
    bb = hi - p
    err = (p - (hi - bb)) + (c - bb)
    even = (hi.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even
    hi = np.where(fix, np.nextafter(hi, np.where(err > 0, np.inf, -np.inf)), hi)
    return hi.astype(F32)


def clean(x):
    """A non-finite sample counts as 0 for the measurement."""
    x = np.asarray(x, dtype=F32)
    return np.where(np.isfinite(x), x, F32(0.0)).astype(F32)


def block_sums(x):
    """fp32 [ceil(n / 512)]: lane l of a block sums its samples l, l + 64, ... ascending by fmaf from 0; the 64 partial sums are
    folded by a butterfly, s[l] += s[l ^ off] for off = 32, 16, ..., 1 (every lane ends with the same bits)."""
    x = clean(x)
    nblk = (len(x) + HOP - 1) // HOP
    v = np.zeros(nblk * HOP, dtype=F32)
    v[:len(x)] = x
    v = v.reshape(nblk, HOP // 64, 64)
    s = np.zeros((nblk, 64), dtype=F32)
    for i in range(HOP // 64):
        s = fma32(v[:, i], v[:, i], s)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lane ^ off]).astype(F32)
    return s[:, 0]


def frame_energies(sums, n):
    """fp32 [n // 512 + 1]: e_f = max(((s[f - 2] + s[f - 1]) + (s[f] + s[f + 1])) / 2048, 1e-10), s = 0 outside the row's blocks."""
    nf = n // HOP + 1
    s = np.zeros(nf + 3, dtype=F32)
    s[2:2 + len(sums)] = sums  # s[f + 2] = block f; len(sums) = ceil(n / 512) <= nf
    f = np.arange(nf)
    e = (((s[f] + s[f + 1]).astype(F32) + (s[f + 2] + s[f + 3]).astype(F32)).astype(F32) * F32(1.0 / FRAME)).astype(F32)
    return np.maximum(e, FLOOR)


def threshold(top_db):
    """(float) 10^(-top_db / 10): the power in double, rounded once."""
    return F32(10.0 ** (-float(F32(top_db)) / 10.0))


def detect(x, top_db):
    """-> (start, end) of a row of len(x) valid samples."""
    n = len(x)
    if not (top_db > 0) or n == 0:  # NaN: not > 0
        return 0, n
    e = frame_energies(block_sums(x), n)
    top = e.max()
    lim = F32(top * threshold(top_db))
    loud = np.nonzero((e > lim) | (e >= top))[0]
    return HOP * int(loud[0]), min(n, HOP * (int(loud[-1]) + 1))


# ---- rules 3 - 5 ------------------------------------------------------------------------------------------------------------------
def pads(start, end, n, keep):
    head = max(0, start - max(0, int(keep[0])))
    stop = min(n, end + max(0, int(keep[1])))
    return head, stop


def move(x, head, stop, ramp):
    """The cut row as uint32 bit patterns: a copy, but for one fp32 multiply on the samples of a fade at an edge that was cut."""
    n, count = len(x), stop - head
    out = np.array(x[head:stop], dtype=F32)
    bits = out.view(np.uint32).copy()
    F = 0 if ramp is None else len(ramp)
    f = min(F, count // 2)
    if f and head > 0:
        bits[:f] = (out[:f] * ramp[:f]).astype(F32).view(np.uint32)
    if f and stop < n:
        bits[count - f:] = (out[count - f:] * ramp[:f][::-1]).astype(F32).view(np.uint32)
    return bits


def edges_row(x, top_db, keep, ramp):
    """x: the row's n_b valid samples -> dict(head, count, bits uint32 [count])."""
    start, end = detect(x, top_db)
    head, stop = pads(start, end, len(x), keep)
    return dict(start=start, end=end, head=head, count=stop - head, bits=move(np.asarray(x, dtype=F32), head, stop, ramp))


def row_samples(frames, T_cap, spf, trim):
    return max(0, min(max(int(frames), 0), T_cap) * spf - trim)


def edges_batch(wave, frames, T_cap, spf, trim, top_db, keep, ramp):
    """wave [B, >= spf T_cap] -> the rows' dicts."""
    return [edges_row(wave[b, :row_samples(frames[b], T_cap, spf, trim)], top_db[b], keep[b], ramp) for b in range(len(frames))]


def marks(dur, lengths, frames, T_cap, shift, edges, spf=600, trim=0, U=1, D=1):
    """marks[b][n] = ceil(clamp(s - head, 0, count) * U / D), s = min(spf * bound[b][n], n_smp) of `_marks_ref`."""
    bd = M.bounds(dur, lengths, frames, T_cap, shift)
    B, N1 = bd.shape
    out = np.zeros((B, N1), dtype=np.int64)
    for b in range(B):
        T_b = int(T_cap) if frames is None else min(max(int(frames[b]), 0), int(T_cap))
        n_smp = max(0, spf * T_b - trim)
        head, count = max(int(edges[b][0]), 0), max(int(edges[b][1]), 0)
        for n in range(N1):
            s = min(spf * int(bd[b, n]), n_smp)
            out[b, n] = (min(max(s - head, 0), count) * U + D - 1) // D
    return out


# ---- the same contract, sample by sample -------------------------------------------------------------------------------------------
def round32(q):
    """A non-negative Fraction -> the nearest fp32, ties to even, by hand (subnormals included)."""
    if q == 0:
        return F32(0.0)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if fractions.Fraction(2) ** e > q:
        e -= 1  # 2^e <= q < 2^(e + 1)
    quantum = fractions.Fraction(2) ** max(e - 23, -149)
    m = q / quantum
    lo = m.numerator // m.denominator
    rest = m - lo
    if rest > fractions.Fraction(1, 2) or (rest == fractions.Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return F32(float(lo * quantum))  # lo < 2^25 and the quantum is a power of two: exact


def brute_row(x, top_db, keep, ramp):
    """`edges_row` as plain loops: every block sum lane by lane, every frame, every sample."""
    x = [F32(v) for v in np.asarray(x, dtype=F32)]
    n = len(x)
    start, end = 0, n
    if top_db > 0 and n > 0:
        sums = []
        for blk in range((n + HOP - 1) // HOP):
            lanes = []
            for l in range(64):
                s = F32(0.0)
                for i in range(HOP // 64):
                    k = blk * HOP + i * 64 + l
                    v = x[k] if k < n and np.isfinite(x[k]) else F32(0.0)
                    s = round32(fractions.Fraction(float(v)) ** 2 + fractions.Fraction(float(s)))
                lanes.append(s)
            for off in (32, 16, 8, 4, 2, 1):
                lanes = [F32(lanes[l] + lanes[l ^ off]) for l in range(64)]
            sums.append(lanes[0])
        blk = lambda i: sums[i] if 0 <= i < len(sums) else F32(0.0)
        e = [max(F32(F32(F32(blk(f - 2) + blk(f - 1)) + F32(blk(f) + blk(f + 1))) * F32(1.0 / 2048.0)), FLOOR) for f in range(n // HOP + 1)]
        top = max(e)
        lim = F32(top * threshold(top_db))
        loud = [f for f, v in enumerate(e) if v > lim or v >= top]
        start, end = HOP * loud[0], min(n, HOP * (loud[-1] + 1))
    head = max(0, start - max(0, int(keep[0])))
    stop = min(n, end + max(0, int(keep[1])))
    count = stop - head
    F = 0 if ramp is None else len(ramp)
    f = min(F, count // 2)
    bits = []
    for i in range(count):
        v = x[head + i]
        if head > 0 and i < f:
            v = F32(v * ramp[i])
        elif stop < n and i >= count - f:
            v = F32(v * ramp[count - 1 - i])
        bits.append(int(np.array(v, dtype=F32).view(np.uint32)))
    return dict(start=start, end=end, head=head, count=count, bits=np.array(bits, dtype=np.uint32))


# ---- the constructed rows ----------------------------------------------------------------------------------------------------------
NAN_PAYLOAD = 0x7FC12345  # a quiet NaN with a payload: the move copies bits
SENTINEL = F32(12345.0)
GEOMETRIES = [(5, 700), (600, 8)]  # (samples_per_frame, T_cap): 3 500 and 4 800 samples at capacity, both more than one tile
BATCHES = [1, 5, 17]
TRIMS = [0, 3]
FADES = [0, 1, 48]


def _tone(n, seed, amp=0.4):
    g = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    return amp * (0.7 * np.sin(2 * np.pi * 220.0 / 24000 * t + g.uniform(0, 6)) + 0.3 * np.sin(2 * np.pi * 1330.0 / 24000 * t))


def _row(L, n, kind, seed):
    """One constructed row of L samples, the first n valid -> (x fp32 [L] with NaN behind n, top_db, keep)."""
    g = np.random.default_rng(seed)
    x = np.zeros(L, dtype=np.float64)
    noise = lambda: 2e-5 * g.standard_normal(n)  # 86 dB under the bursts: silence at 60 dB too
    top_db, keep = 20.0, (0, 0)
    a, b = min(1037, n), min(2291, n)  # offsets that are no multiple of 512 or of 4
    if kind == "burst":
        x[:n] = noise()
        x[a:b] += _tone(b - a, seed)
    elif kind == "from 0":
        x[:min(1501, n)] = _tone(min(1501, n), seed)
        top_db, keep = 60.0, (100, 100)
    elif kind == "to the end":
        x[:n] = noise()
        x[max(n - 1203, 0):n] += _tone(n - max(n - 1203, 0), seed)
        keep = (5000, 5000)  # larger than the silence: the pads hit 0 and n
    elif kind == "zero":
        keep = (7, 7)
    elif kind == "whole":  # speech from the first sample to the last: nothing is cut
        x[:n] = _tone(n, seed)
    elif kind == "non-finite":
        x[:n] = noise()
        x[min(777, n):min(3001, n)] += _tone(min(3001, n) - min(777, n), seed)
        top_db = 60.0
    elif kind == "nan top_db":
        x[a:b] = _tone(b - a, seed)
        top_db = float("nan")
    elif kind == "top_db 0":
        x[a:b] = _tone(b - a, seed)
        top_db = 0.0
    elif kind == "negative keep":
        x[:n] = noise()
        x[a:b] += _tone(b - a, seed)
        keep = (-5, -9)
    elif kind == "keep":
        x[:n] = noise()
        x[a:b] += _tone(b - a, seed)
        top_db, keep = 60.0, (241, 723)
    elif kind == "tile edge":  # a burst across the 2048-sample tile of the sums' launch
        c, d = min(2047, n), min(2050, n)
        x[c:d] = 0.9
        keep = (1, 2)
    elif kind == "two bursts":
        x[:n] = noise()
        for c, d in ((min(601, n), min(1103, n)), (min(2803, n), min(3307, n))):
            x[c:d] += _tone(d - c, seed)
        top_db = 60.0
    else:
        raise KeyError(kind)
    out = x.astype(F32)
    if kind == "non-finite" and n > 1700:
        out[1500] = np.array([NAN_PAYLOAD], dtype=np.uint32).view(F32)[0]
        out[1600], out[1601] = np.inf, -np.inf
    out[n:] = np.nan  # nothing at or past n_b is read
    return out, top_db, keep


KINDS = ["burst", "from 0", "to the end", "zero", "frames 0", "short", "non-finite", "nan top_db", "top_db 0", "negative keep", "keep",
         "tile edge", "two bursts", "whole", "burst", "to the end", "from 0"]


@functools.lru_cache(maxsize=None)
def batch(B, spf, T_cap, trim):
    """-> dict(wave fp32 [B, spf T_cap], frames, top_db, keep, names): row b is KINDS[b]; rows differ in their frame counts."""
    L = spf * T_cap
    wave, frames, top_db, keep = np.zeros((B, L), dtype=F32), [], [], []
    for b in range(B):
        kind = KINDS[b]
        fr = {"frames 0": 0, "short": max(1, 500 // spf)}.get(kind, T_cap - (b % 3) * max(1, T_cap // 9))
        n = row_samples(fr, T_cap, spf, trim)
        wave[b], td, kp = _row(L, n, "whole" if kind in ("frames 0", "short") else kind, 1000 * spf + 10 * b + trim)
        frames.append(fr), top_db.append(td), keep.append(kp)
    return dict(wave=wave, frames=np.array(frames, dtype=np.int32), top_db=np.array(top_db, dtype=F32),
                keep=np.array(keep, dtype=np.int32), names=KINDS[:B], spf=spf, T_cap=T_cap, trim=trim)


SIZES = [300, 511, 512, 513, 2047, 2048]


@functools.lru_cache(maxsize=None)
def sizes_batch():
    """Rows of exactly SIZES valid samples, as rows of one-sample frames (the geometry the hand-over runs the later steps in):
    a burst at the row's end behind silence -- the two long rows are cut in front, the others are shorter than the two frames a
    cut needs.  What differs from size to size is the number of blocks and of frames: (1, 1), (1, 1), (1, 2), (2, 2), (4, 4), (4, 5)."""
    T_cap = 2100
    wave = np.zeros((len(SIZES), T_cap), dtype=F32)
    for b, n in enumerate(SIZES):
        wave[b, max(n - 150, 0):n] = _tone(n - max(n - 150, 0), 50 + b).astype(F32)
        wave[b, n:] = np.nan
    return dict(wave=wave, frames=np.array(SIZES, dtype=np.int32), top_db=np.full(len(SIZES), 30.0, dtype=F32),
                keep=np.tile(np.array([[3, 0]], dtype=np.int32), (len(SIZES), 1)), names=["n = %d" % n for n in SIZES], spf=1,
                T_cap=T_cap, trim=0)


@functools.lru_cache(maxsize=None)
def reference(B, spf, T_cap, trim, F):
    """The rows' reference for a batch of `batch` (B > 0) or `sizes_batch` (B = 0), computed once and shared."""
    from styletts2_amd import resample
    c = batch(B, spf, T_cap, trim) if B else sizes_batch()
    ramp = resample.edge_ramp_design(F) if F else None
    return edges_batch(c["wave"], c["frames"], c["T_cap"], c["spf"], c["trim"], c["top_db"], c["keep"], ramp)
