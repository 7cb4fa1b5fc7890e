"""Filter tables of `st2_wave_resample_pack` and of `st2_clip_ingest` (section 16): the polyphase taps
that take the model's 24 kHz to an output rate, and a client's rate to the model's 24 kHz, designed on the host in numpy fp64
-- once per rate and direction -- and kept on the device, one copy per (direction, rate, device).

A table is never built under stream capture (the upload waits): whoever captures the step that reads it makes it first
(`GraphedSynthesis.__init__` does), and `table()` / `input_table()` refuse to build one while a capture is running."""
import math

import numpy as np
import torch

MODEL_RATE = 24000
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
ATTENUATION_DB = 96.0  # Kaiser's design attenuation; the acceptance condition on a table is 90 dB from f_N upward
PASSBAND = 0.85  # the transition band runs from 0.85 f_N to f_N (f_N: the lower of the two Nyquist frequencies)
CUTOFF = (1.0 + PASSBAND) / 2  # 0.925: the cutoff sits at the band's centre
BETA = 0.1102 * (ATTENUATION_DB - 8.7)


def taps_per_phase(up, down):
    """K, even, from Kaiser's formula N = (A - 7.95) / (2.285 dw) for the prototype at `up` times the input rate: its
    transition band is dw = 2 pi * 0.15 * (f_N / input rate) / up wide there and K = N / up.  The formula is empirical; every
    supported rate meets both acceptance conditions with it (tests/test_resample_cpu.py computes them), so nothing is added."""
    width = (1.0 - PASSBAND) * 0.5 * min(1.0, up / down)  # in cycles per input sample
    K = int(math.ceil((ATTENUATION_DB - 7.95) / (2.285 * 2.0 * math.pi * width)))
    return K + (K & 1)


def ratio(rate):
    """-> (U, D): the reduced fraction rate / MODEL_RATE of an output rate of RATES, without designing its table."""
    if rate not in RATES:
        raise ValueError("output rate %r is not supported: one of %s at a model rate of %d" % (rate, list(RATES), MODEL_RATE))
    g = math.gcd(int(rate), MODEL_RATE)
    return int(rate) // g, MODEL_RATE // g


def design(rate, model_rate=MODEL_RATE):
    """-> (U, D, taps float32 [U, K]): U / D is the reduced fraction rate / model_rate and
    taps[p][k] = g(k - (K - 1) // 2 - p / U) with g(t) = r sinc(r t) kaiser(2 t / K; beta), r = 0.925 min(1, U / D)."""
    if model_rate != MODEL_RATE or rate not in RATES:
        raise ValueError("output rate %r is not supported: one of %s at a model rate of %d" % (rate, list(RATES), MODEL_RATE))
    g = math.gcd(int(rate), int(model_rate))
    return _kaiser_table(int(rate) // g, int(model_rate) // g)


def design_input(rate, model_rate=MODEL_RATE):
    """-> (U, D, taps float32 [U, K]) of the way in: U / D is the reduced fraction model_rate / rate, the taps are `design`'s
    formula at that ratio.  K by `taps_per_phase`: 82 / 82 / 82 / 110 / 152 / 164 at 8 / 16 / 22.05 / 32 / 44.1 / 48 kHz; every
    rate meets both acceptance conditions with it (tests/test_ingest_cpu.py computes them), so nothing is added."""
    if model_rate != MODEL_RATE or rate not in RATES:
        raise ValueError("input rate %r is not supported: one of %s at a model rate of %d" % (rate, list(RATES), MODEL_RATE))
    g = math.gcd(int(rate), int(model_rate))
    return _kaiser_table(int(model_rate) // g, int(rate) // g)


def _kaiser_table(U, D):
    """The table of the ratio U / D (reduced): what `design` and `design_input` share."""
    if U == D:
        return 1, 1, np.ones((1, 1), dtype=np.float32)
    K = taps_per_phase(U, D)
    r = CUTOFF * min(1.0, U / D)
    t = np.arange(K, dtype=np.float64)[None, :] - (K - 1) // 2 - np.arange(U, dtype=np.float64)[:, None] / U
    x = 2.0 * t / K
    window = np.where(np.abs(x) <= 1.0, np.i0(BETA * np.sqrt(np.clip(1.0 - x * x, 0.0, None))) / np.i0(BETA), 0.0)
    return U, D, (r * np.sinc(r * t) * window).astype(np.float32)


def prototype(taps):
    """The table flattened to the one low-pass it samples, at U times the input rate: taps[p][k] is its sample k U - p."""
    U, K = taps.shape
    proto = np.zeros(U * K, dtype=np.float64)
    for p in range(U):
        proto[U - 1 - p::U] = taps[p]
    return proto


def output_samples(n, up, down):
    """m = ceil(n U / D): the output samples of a row of n input samples."""
    return (int(n) * up + down - 1) // down


_TABLES = {}


def _device_table(key, rate, device, make, name, call=None):
    dev = torch.device(device)
    key = key + (int(rate), dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    hit = _TABLES.get(key)
    if hit is None:
        U, D, taps = make(rate)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the %d Hz filter table must exist before a stream capture: call resample.%s first"
                               % (rate, call or "%s(%d, device)" % (name, rate)))
        hit = _TABLES[key] = (U, D, taps.shape[1], torch.from_numpy(taps).to(dev))
    return hit


def table(rate, device):
    """-> (U, D, K, taps fp32 [U, K] on `device`), designed and uploaded on first use."""
    return _device_table((), rate, device, design, "table")


def input_table(rate, device):
    """`table` of the way in (`design_input`), under cache keys of its own."""
    return _device_table(("in",), rate, device, design_input, "input_table")


TRUE_PEAK_UP = 8  # ITU-R BS.1770-4 Annex 2 reads the peak at 192 kHz or above: 8 x the model's 24 kHz


def true_peak_table(device):
    """-> (8, K, taps fp32 [8, K] on `device`): the interpolation table of the true-peak measurement (`ops.wave_level(true_peak=)`;
    DESIGN.md section 23) -- the design of every other table here at the ratio 8 / 1 (K = 82), under a cache key of its own,
    designed and uploaded on first use and, like `table`, never under stream capture."""
    U, _, K, taps = _device_table(("tp",), MODEL_RATE * TRUE_PEAK_UP, device, lambda rate: _kaiser_table(TRUE_PEAK_UP, 1),
                                  "true_peak_table", call="true_peak_table(device)")
    return U, K, taps


LIMIT_MAX_W = 1024  # st2_wave_limit's largest half window


def limit_window_design(W):
    """-> fp32 [2 W + 1]: the smoother of the look-ahead limiter (`ops.wave_limit`) -- a Hann window over
    2 W + 1 points without its two zero end points, normalised to sum 1 in fp64 and then rounded: every weight positive."""
    W = int(W)
    if not 1 <= W <= LIMIT_MAX_W:
        raise ValueError("the limiter's half window must be 1..%d samples, got %r" % (LIMIT_MAX_W, W))
    k = np.arange(1, 2 * W + 2, dtype=np.float64)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (2 * W + 2))
    return (h / h.sum()).astype(np.float32)


def limit_window(W, device):
    """-> win fp32 [2 W + 1] on `device`: `limit_window_design(W)`, one copy per (W, device), designed and uploaded on first use and,
    like `table`, never under stream capture."""
    _, _, _, win = _device_table(("lim",), int(W), device, lambda w: (1, 1, limit_window_design(w)[None, :]), "limit_window")
    return win[0]


EDGE_MAX_F = 4096  # st2_wave_edges's longest fade


def edge_ramp_design(F):
    """-> fp32 [F]: the fade of a cut edge (`ops.wave_edges`) -- the rising half of a raised cosine sampled
    at the half points, ramp[i] = 0.5 - 0.5 cos(pi (i + 0.5) / F): strictly inside (0, 1), rising, and ramp[i] + ramp[F - 1 - i] = 1."""
    F = int(F)
    if not 1 <= F <= EDGE_MAX_F:
        raise ValueError("the edge fade must be 1..%d samples, got %r" % (EDGE_MAX_F, F))
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / F)).astype(np.float32)


def edge_ramp(F, device):
    """-> ramp fp32 [F] on `device`: `edge_ramp_design(F)`, one copy per (F, device), designed and uploaded on first use and, like
    `table`, never under stream capture."""
    _, _, _, ramp = _device_table(("edge",), int(F), device, lambda f: (1, 1, edge_ramp_design(f)[None, :]), "edge_ramp")
    return ramp[0]
