"""numpy contract of the counter-based noise (styletts2_amd/csrc/st2_rng.h): integers exact, normals in
fp64.  Element i of noise stream s of a row with seed k is output (i mod 4) of the four values made from
Philox4x32-10(counter = (i div 4, 0, s, 0), key = (lo32(k), hi32(k))), k the int64 seed read as uint64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
SAMPLER, STEP, SINE = 0, 1, 0x10000  # st2.h ST2_NOISE_*
MASK = np.uint64(0xFFFFFFFF)

# Random123's known answers (kat_vectors: philox4x32 10): (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

# The seeds of the statistical tests (CPU and GPU): fixed here, and the fp64 contract itself meets every bound under them.
STAT_SEEDS = (20240229, -7)
STAT_N = 1 << 20


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) of one shape, key: two -> the four output words, uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def bits(seed, stream, n):
    """The first n 32-bit words of noise stream `stream` under the int64 `seed` -> uint32 [n]."""
    if not 0 <= n < 1 << 34:
        raise ValueError("a row holds fewer than 2^34 elements")
    k = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(q)
    w = philox4x32_10((q, zero, zero + np.uint64(int(stream) & 0xFFFFFFFF), zero), (k & 0xFFFFFFFF, k >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def normals_from_bits(w):
    """uint32 [4 m] -> fp64 [4 m]: Box-Muller pairs from the words (x0, x1) and (x2, x3) of every counter."""
    w = np.asarray(w, dtype=np.uint32).reshape(-1, 2).astype(np.int64)
    u1 = ((w[:, 0] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * ((w[:, 1] >> 8).astype(np.float64) * 2.0 ** -24)  # in [0, 2): cos(pi a), sin(pi a)
    return np.stack([r * np.cos(np.pi * a), r * np.sin(np.pi * a)], axis=1).reshape(-1)


def normals(seed, stream, n):
    """The first n normals of noise stream `stream` under `seed` -> fp64 [n]."""
    return normals_from_bits(bits(seed, stream, (n + 3) // 4 * 4))[:n]


def fill(seeds, stream0, S, n, counts=None, per_count=None, kind="normal"):
    """What st2_noise_fill writes: [S][B][n] (uint32 or fp64) and the mask of the elements it writes at all."""
    B = len(seeds)
    out = np.zeros((S, B, n), dtype=np.uint32 if kind == "bits" else np.float64)
    written = np.zeros((S, B, n), dtype=bool)
    for s in range(S):
        for b in range(B):
            m = n if counts is None else min(n, max(int(counts[b]), 0) * int(per_count))
            out[s, b, :m] = (bits if kind == "bits" else normals)(seeds[b], stream0 + s, m)
            written[s, b, :m] = True
    return out, written


def stats(z, other=None):
    """The figures the statistical bounds are about, of fp64 draws z (and their correlation with `other`)."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])
    return dict(n=n, mean=float(z.mean()), var=float(z.var()), tail=float((np.abs(z) > 3.0).mean()),
                lag1=corr(z[:-1], z[1:]), cross=None if other is None else corr(z, np.asarray(other, dtype=np.float64)))


TAIL_P = 0.0026997960632601866  # P(|z| > 3) of a standard normal


def check_stats(st, what=""):
    """The bounds of the issue, each at five sigmas of its own sampling distribution."""
    n = st["n"]
    assert abs(st["mean"]) < 5.0 / np.sqrt(n), (what, st)
    assert abs(st["var"] - 1.0) < 5.0 * np.sqrt(2.0 / n), (what, st)
    assert abs(st["tail"] - TAIL_P) < 5.0 * np.sqrt(TAIL_P * (1.0 - TAIL_P) / n), (what, st)
    assert abs(st["lag1"]) < 5.0 / np.sqrt(n), (what, st)
    assert st["cross"] is None or abs(st["cross"]) < 5.0 / np.sqrt(n), (what, st)
