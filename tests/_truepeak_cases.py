"""The rows tests/test_truepeak_gpu.py measures, made once, K-weighted once and interpolated once by the contracts of
tests/_level_ref.py and tests/_truepeak_ref.py, and what those contracts say of them per geometry, per row and per group.
tests/test_truepeak_cpu.py checks, from the contract alone, that no case sits on a tie of the gain's three terms or within
`_level_cases.GUARD_LU` of a gate.  Not product code."""
import functools
import math

import numpy as np

import _level_cases as Cs
import _level_ref as R
import _truepeak_ref as TP

FS, ROW, H = Cs.FS, Cs.ROW, Cs.H
CEILING, MAX_GAIN_DB = Cs.CEILING, Cs.MAX_GAIN_DB
TILE = H  # the true-peak launch works hop by hop: its tile boundary is the hop's
PASS = 256 * 5  # and within a hop a lane's second pass begins here
# name: (valid samples, target).  The C entry takes any target; +10 puts the ceiling in charge of the sine rows (their samples
# reach 0.3536 of a crest of 0.5, so the ceiling term is 2.52 by the sample peak and 1.78 by the true peak)
ROWS = {"empty": (0, -16.0), "zero": (ROW, -16.0), "s17": (17, -16.0), "s11999": (11999, -16.0), "sine": (24000, 10.0),
        "const": (7000, -16.0), "burst_hop": (24000, -16.0), "burst_tile": (24000, -16.0), "impulse": (ROW, -16.0),
        "nan_sample": (24000, 10.0), "nan_target": (ROW, float("nan"))}
MAIN = ("empty", "zero", "s17", "s11999", "sine", "const", "burst_hop", "burst_tile")
OTHER = ("impulse", "sine", "nan_sample", "nan_target", "burst_tile", "s17", "const", "s11999")
GEOMETRIES = [(1, 0), (600, 50)]  # (samples per frame, trim): 1 gives the sample counts above exactly
# passage scope: rows of different loudness, one of them empty, one group led by a NaN target
GROUP_ROWS = ("s11999", "burst_hop", "empty", "nan_target", "sine", "impulse", "const", "s17")
GROUP_START = (1, 0, 0, 1, 0, 1, 0, 0)
SINGLE_START = (1, 1, 1, 1, 1, 1, 1, 1)


def faded_sine(n=24000, fade=2400, amplitude=0.5):
    """A sine at fs / 4 whose samples fall 45 degrees off the crests (BS.1770-4 Annex 2's case), raised-cosine fades at both ends."""
    i = np.arange(n)
    env = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    env[:fade], env[n - fade:] = ramp, ramp[::-1]
    return amplitude * env * np.sin(2.0 * np.pi * i / 4.0 + np.pi / 4.0)


def _burst(x, centre):
    """40 samples of the 45-degree fs / 4 sine at 0.8 under a Hann window, centred on `centre`, added to x."""
    i = np.arange(centre - 20, centre + 20)
    x[i] += 0.8 * np.hanning(40) * np.sin(2.0 * np.pi * i / 4.0 + np.pi / 4.0)
    return x


@functools.lru_cache(maxsize=None)
def content():
    """name -> (x fp32 [ROW], y2 fp64 [ROW]): every row at capacity and its squared K-weighted samples; read-only."""
    g = np.random.default_rng(4242)
    noise = lambda rms, n=ROW: g.standard_normal(n) * rms
    rows = {"empty": np.zeros(ROW), "zero": np.zeros(ROW), "s17": noise(0.1), "s11999": noise(10.0 ** (-30.0 / 20.0))}
    pad = lambda x: np.concatenate([x, noise(0.05, ROW - len(x))])  # behind the issue's count: what a longer geometry reads
    rows["sine"] = pad(faded_sine())
    rows["const"] = np.full(ROW, 0.5)
    rows["burst_hop"] = _burst(noise(0.01), 3 * H)
    rows["burst_tile"] = _burst(_burst(noise(0.01), 7 * TILE), 5 * H + PASS)
    out = {}
    for name, x in rows.items():
        x = x.astype(np.float32)
        out[name] = (x, R.k_weight(R.clean(x), FS) ** 2)
    x = out["sine"][0].copy()
    x[12001] = np.nan  # the sample before a crest pair: the measurement reads 0 there
    out["nan_sample"] = (x, R.k_weight(R.clean(x), FS) ** 2)
    for name in ("impulse", "nan_target"):
        out[name] = Cs.content()[name]
    for x, y2 in out.values():
        x.setflags(write=False)
        y2.setflags(write=False)
    return out


def frames_of(name, spf, trim):
    """The frame count that gives the row its sample count, or the nearest count above it that `spf` and `trim` allow."""
    n = ROWS[name][0]
    return 0 if n == 0 else min(-(-(n + trim) // spf), ROW // spf)


def samples_of(name, spf, trim):
    return R.row_samples([frames_of(name, spf, trim)], ROW // spf, spf, trim)[0]


@functools.lru_cache(maxsize=None)
def measured(name, spf, trim):
    """-> dict(n, z, peak, tp, tp_lo, tp_hi): the row's blocks, its sample peak (fp32, exact), its true peak in fp64 and the
    interval an fp32 evaluation may report."""
    x, y2 = content()[name]
    n = samples_of(name, spf, trim)
    tp, lo, hi = TP.true_peak(x[:n], TP.table()[2])
    return dict(n=n, z=R.blocks_of(y2[:n], FS), peak=R.peak(x[:n]), tp=tp, tp_lo=lo, tp_hi=hi)


def expect_group(names, spf, trim, true_peak, target=None):
    """The rows `names` as ONE group -> (level fp32 [4], (z, passed, l, rel, L)); the peak is the contract's fp64 true peak
    rounded to fp32, or the exact sample peak.  target: the first row's by default."""
    m = [measured(n, spf, trim) for n in names]
    peaks = [np.float32(d["tp"]) if true_peak else d["peak"] for d in m]
    return TP.level_group([d["z"] for d in m], peaks, ROWS[names[0]][1] if target is None else target, CEILING, MAX_GAIN_DB)


def gate_distance(detail):
    """The least distance in LU of any block of a (z, passed, l, rel, L) from the absolute gate and from the relative one."""
    _, _, l, rel, _ = detail
    l = l[np.isfinite(l)]
    dist = [math.inf] + list(np.abs(l - R.ABS_GATE))
    if rel > -math.inf:
        dist += list(np.abs(l[l > R.ABS_GATE] - rel))
    return min(dist)


def loudness_bound_db(detail, peak):
    """`_level_cases.loudness_bound_db` for a block list that is a group's: the same error model over the group's passing blocks
    and the group's largest SAMPLE peak."""
    z, passed, _, _, L = detail
    if not passed.any():
        return 0.0
    eps = sum(Cs.error_model()) * float(peak)
    zmin = z[passed].min()
    delta = 2.0 * eps / math.sqrt(zmin) + eps * eps / zmin + 8 * H * 2.0 ** -53
    return 4.343 * delta + abs(L) * (2.0 ** -24 + 8 * 2.0 ** -53)
