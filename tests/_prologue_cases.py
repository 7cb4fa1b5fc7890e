"""Hard inputs of the split-f16 prologue tests, built PER CHANNEL: one channel row holds one magnitude class, so a bar normalised
per (b, channel) row judges every class by its own scale.  Fixed seed; no GPU needed (tests/test_prologue_ref_cpu.py proves that
every list covers what its comments claim).  Every case has B <= 3, C <= 72, L <= 600."""
import math

import numpy as np
import torch

from oracle import ops_ref as R

SEED = 20261
F16_MAX = 65504.0
NAN, INF = float("nan"), float("inf")


def _gen(*salt):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(s) for i, s in enumerate(salt)))


def f32(v):
    return float(np.float32(v))


# ---- section 2: special values of the split -----------------------------------------------------------------------------------
def _f16_midpoints(parity):
    """Midpoints between adjacent f16 values m and m + ulp whose LOWER neighbour has mantissa parity `parity` (0: the tie rounds
    down to it, 1: up to the next): binades 2^-14 (the lowest normal one), 2^-3, 1, 2^7 and 2^15, and the subnormal grid."""
    out = []
    for k in (-14, -3, 0, 7, 15):
        for m in (0, 2, 510, 1022) if parity == 0 else (1, 3, 511, 1021):  # 1023 at 2^15 would be 65520: not a finite f16 pair
            out.append(math.ldexp(1.0 + m / 1024.0 + 1.0 / 2048.0, k))
    for n in (0, 2, 4) if parity == 0 else (1, 3, 1023):
        out.append((n + 0.5) * 2.0 ** -24)
    return out


def _lo_subnormal():
    """hi + r with 0 < |f16(r)| < 2^-14: r on and off the 2^-24 grid of the subnormal lo half, one of them on a tie of that grid."""
    out = []
    for h in (0.25, 0.0625, 0.125, 0.0999755859375):
        for r in (2.0 ** -15 + 3 * 2.0 ** -26, -(2.0 ** -16 + 2.0 ** -26), 1.5 * 2.0 ** -24, 2.0 ** -23 + 2.0 ** -26):
            out.append(h + r)
    return out


SPLIT_ROWS = {
    "zeros": [0.0, -0.0],
    "f32_subnormal": [1e-40, 2.0 ** -149, 2.0 ** -127, 3e-39],
    "tiny_pow2": [2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 3 * 2.0 ** -26],
    "ties_even": _f16_midpoints(0),
    "ties_odd": _f16_midpoints(1),
    "lo_subnormal": _lo_subnormal(),
    "top": [F16_MAX, float(np.nextafter(np.float32(F16_MAX), np.float32(0))), 65472.0, 65488.0],  # the last: tie of 65472 / 65504
    "ordinary": [1.0, 0.333333343267, 1234.5677490234375, 3.0e-3, 17.0, 0.7071067690849304],
    # ---- out of range from here: every element clamps and raises the status bit
    "above_top": [float(np.nextafter(np.float32(F16_MAX), np.float32(INF))), f32(65519.9), 65520.0, 65536.0],
    "huge": [1.0e6, 3.0e38],
    "inf": [INF],
    "nan": [NAN],
}
_IN_RANGE = ["zeros", "f32_subnormal", "tiny_pow2", "ties_even", "ties_odd", "lo_subnormal", "top", "ordinary", "ordinary"]
SPLIT_CASES = {  # case -> the rows of its channels; "in_range" must leave the status word at 0, every other one raises F16_RANGE
    "in_range": _IN_RANGE,
    "above_top": _IN_RANGE + ["above_top"],
    "huge": _IN_RANGE + ["huge"],
    "inf": _IN_RANGE + ["inf"],
    "nan": _IN_RANGE + ["nan"],
}
SPLIT_L = 77


def split_tensor(case, C=None, L=SPLIT_L):
    """x [2, C, L] float32: channel c tiles SPLIT_ROWS[rows[c % len(rows)]] along L; batch item 1 is the negated row, one column on.
    C defaults to one channel per row (10 or 9: no multiple of 8, so the last slot has channel padding)."""
    rows = SPLIT_CASES[case]
    C = C or len(rows)
    x = torch.empty(2, C, L, dtype=torch.float32)
    for c in range(C):
        vals = torch.tensor([f32(v) for v in SPLIT_ROWS[rows[c % len(rows)]]], dtype=torch.float32)
        idx = torch.arange(L) % len(vals)
        x[0, c] = vals[idx]
        x[1, c] = -vals[(idx + 1) % len(vals)]
    return x


# ---- section 3: benign data at edge shapes --------------------------------------------------------------------------------------
SHAPE_L = (1, 255, 256, 257, 513)  # the 256-position blocks of act_split_kernel, after the plan's halo
SHAPE_C = (1, 7, 8, 9, 33, 72)     # the 8-channel slots and the 32-channel padding
ALL_PROS = (R.PRO_NONE, R.PRO_LEAKY, R.PRO_ADAIN_LEAKY, R.PRO_ADAIN_SNAKE, R.PRO_SNAKE, R.PRO_COLNORM)


def benign_case(pro, B, C, L):
    """dict(x, kw): randn data, prologue operands as tests/_util.py make_conv_case draws them (statistics come from the device)."""
    g = _gen(1, pro, B, C, L)
    x = torch.randn(B, C, L, generator=g)
    kw = dict(pro=pro)
    if pro in (R.PRO_LEAKY, R.PRO_ADAIN_LEAKY):
        kw["slope"] = 0.2
    if pro in (R.PRO_ADAIN_LEAKY, R.PRO_ADAIN_SNAKE, R.PRO_COLNORM):
        kw["gamma"], kw["beta"] = torch.randn(B, C, generator=g) * 0.3, torch.randn(B, C, generator=g) * 0.3
    if pro in (R.PRO_ADAIN_SNAKE, R.PRO_SNAKE):
        kw["alpha"] = torch.rand(C, generator=g) + 0.5
    return dict(x=x, kw=kw)


def length_batches(L):
    """Per-row lengths 0, 1, L and L + 5 in two ragged launches of B = 3 (four in one would need B = 4)."""
    return ((0, 1, L + 5), (L, L + 5, 0))


# ---- section 3: hard rows ---------------------------------------------------------------------------------------------------
# AdaIN: (name, gamma, beta, claim on |mean| / std of the row, or None where the row's point is another)
# Measured on an MI355X, st2_act_split at L = 257, max over the rows of the class (kernel error, fp32-contract error):
#                      AdaIN + LeakyReLU(0.2)     AdaIN + Snake (alpha 1, 30, 0.1, 0.01, -2)
#   offset             4.8e-7 / 4.5e-7            7.8e-7 / 7.2e-7
#   constant           0 / 0                      1.6e-8 / 1.4e-8
#   g_zero             0 / 0                      3.3e-8 / 2.6e-8
#   offset_small_std   2.8e-7 / 1.8e-7            4.4e-7 / 3.0e-7
#   benign             4.2e-7 / 5.2e-7            7.6e-7 / 7.1e-7
#   gain_30            1.3e-5 / 8.2e-6            2.3e-5 / 1.5e-5
ADAIN_ROWS = [
    ("offset", 0.3, -0.2, (500.0, 2000.0)),         # 1e3 + randn: |mean| / std ~ 1e3, x - mean cancels three digits
    ("constant", 0.5, 0.25, (1e30, INF)),           # std = 0: rstd = 1 / sqrt(eps) = 316.2
    ("g_zero", -1.0, 0.625, None),                  # gamma = -1: g = 0 and the output is exactly beta
    ("offset_small_std", -0.4, 0.1, (2500.0, 1e4)),  # 50 + 0.01 randn: |mean| / std ~ 5e3, rstd ~ 95
    ("benign", 0.2, 0.3, (0.0, 0.5)),
    ("gain_30", 29.0, 0.0, (0.0, 0.5)),             # g = 30: |u| reaches ~ 100; with alpha = 30, |alpha u| reaches 1e3
]
ADAIN_ALPHAS = [1.0, 30.0, 0.1, 0.01, -2.0]  # channel c: row c % 6, alpha (c // 6) % 5
ADAIN_C = len(ADAIN_ROWS) * len(ADAIN_ALPHAS)


def adain_case(snake, C=ADAIN_C, L=257, B=2, slope=0.2):
    g = _gen(2, snake, C, L)
    x = torch.empty(B, C, L)
    gamma, beta = torch.empty(B, C), torch.empty(B, C)
    for c in range(C):
        name, ga, be, _ = ADAIN_ROWS[c % len(ADAIN_ROWS)]
        r = torch.randn(B, L, generator=g)
        x[:, c] = {"offset": 1e3 + r, "constant": torch.full((B, L), 3.7), "offset_small_std": 50.0 + 0.01 * r}.get(name, r)
        gamma[:, c], beta[:, c] = ga, be
    kw = dict(pro=R.PRO_ADAIN_SNAKE if snake else R.PRO_ADAIN_LEAKY, gamma=gamma, beta=beta)
    if snake:
        kw["alpha"] = torch.tensor([ADAIN_ALPHAS[(c // len(ADAIN_ROWS)) % len(ADAIN_ALPHAS)] for c in range(C)])
    else:
        kw["slope"] = slope
    return dict(x=x, kw=kw)


# Snake (PRO_SNAKE, u = x): (alpha, kind, reach) -- "range": u random in [-reach / |alpha|, reach / |alpha|] with both ends present,
# so max |alpha u| = reach; "pi": u = k pi / alpha, "half": u = (k + 1/2) pi / alpha for the L consecutive k centred on 0
# Measured on an MI355X, st2_act_split at L = 257 (kernel error / fp32-contract error) beside each row; the kernel's share above
# the contract's is the split: 2^-22 |u| = 2.4e-3 at |u| = 1e4.
SNAKE_ROWS = [
    # |alpha u| up to 1e2, 1e3, 1e4: the two-term range reduction
    (1.0, "range", 1e2),    # 1.1e-5 / 3.8e-6
    (1.0, "range", 1e3),    # 9.1e-5 / 3.0e-5
    (1.0, "range", 1e4),    # 1.4e-3 / 4.7e-4
    (30.0, "range", 1e2),   # 3.5e-7 / 1.2e-7
    (30.0, "range", 1e3),   # 3.7e-6 / 1.9e-6
    (30.0, "range", 1e4),   # 4.5e-5 / 1.5e-5
    (0.1, "range", 1e2),    # 9.1e-5 / 3.1e-5
    (0.1, "range", 1e3),    # 1.5e-3 / 4.8e-4
    # small alpha: 1 / alpha = 100 multiplies sin_sq's error
    (0.01, "range", 1e2),   # 1.5e-3 / 4.9e-4
    (0.01, "range", 1.0),   # 2.1e-5 / 1.7e-5
    (0.01, "range", 0.01),  # 1.3e-7 / 4.4e-8
    # negative alpha
    (-2.0, "range", 1e3),   # 4.5e-5 / 1.5e-5
    (-0.1, "range", 1e2),   # 9.0e-5 / 3.1e-5
    # on and halfway between the multiples of pi / alpha
    (1.0, "pi", None),      # 3.1e-5 / 2.2e-10
    (1.0, "half", None),    # 3.1e-5 / 7.6e-6
    (30.0, "pi", None),     # 9.5e-7 / 2.5e-11
    (30.0, "half", None),   # 1.4e-6 / 4.5e-7
    (0.1, "pi", None),      # 2.4e-4 / 9.0e-9
    (0.1, "half", None),    # 2.4e-4 / 6.1e-5
]
SNAKE_C = len(SNAKE_ROWS)


def snake_case(C=SNAKE_C, L=257, B=2):
    g = _gen(3, C, L)
    x = torch.empty(B, C, L)
    alpha = torch.empty(C)
    for c in range(C):
        a, kind, reach = SNAKE_ROWS[c % len(SNAKE_ROWS)]
        alpha[c] = a
        if kind == "range":
            u = (torch.rand(B, L, generator=g) * 2 - 1) * (reach / abs(a))
            u[:, 0], u[:, -1] = reach / abs(a), -reach / abs(a)
        else:
            k = torch.arange(L, dtype=torch.float64) - L // 2 + (0.5 if kind == "half" else 0.0)
            u = (k * math.pi / a).float().expand(B, L).clone()
            u[1] = -u[1].flip(0)
        x[:, c] = u
    return dict(x=x, kw=dict(pro=R.PRO_SNAKE, alpha=alpha))


LEAKY_SLOPES = (0.0, 0.01, 0.2)
LEAKY_ROWS = ["large_negative", "large_mixed", "tiny", "benign", "negative"]  # [-6e4, -1e3]; +-6e4; 1e-6 randn; randn; -|randn|
# Measured on an MI355X, st2_act_split at L = 257 (kernel error / fp32-contract error; the kernel's share is the split, the
# contract's the fp32 rounding of x * slope):
#                    slope 0            slope 0.01           slope 0.2
#   large_negative   0 / 0              7.8e-5 / 4.2e-5      1.6e-3 / 5.9e-4
#   large_mixed      3.9e-3 / 0         3.9e-3 / 3.9e-5      3.9e-3 / 5.9e-4
#   tiny             3.0e-8 / 0         3.0e-8 / 1.1e-15     3.0e-8 / 3.4e-14
#   benign           2.4e-7 / 0         2.4e-7 / 1.3e-9      2.4e-7 / 3.6e-8
#   negative         0 / 0              3.1e-8 / 1.4e-9      9.5e-8 / 3.6e-8
LEAKY_C = len(LEAKY_ROWS)


def leaky_case(slope, C=LEAKY_C, L=257, B=2):
    g = _gen(4, C, L)
    x = torch.empty(B, C, L)
    for c in range(C):
        name = LEAKY_ROWS[c % len(LEAKY_ROWS)]
        r, q = torch.randn(B, L, generator=g), torch.rand(B, L, generator=g)
        x[:, c] = {"large_negative": -1e3 - 5.9e4 * q, "large_mixed": 6e4 * (2 * q - 1), "tiny": 1e-6 * r, "negative": -r.abs()}.get(name, r)
        if name.startswith("large"):
            x[:, c, 0] = -6e4
    return dict(x=x, kw=dict(pro=R.PRO_LEAKY, slope=slope))


# Column norm: statistics per POSITION.  Columns l % 17 == 3 sit on an offset of 1e3 (|mean| / std ~ 1e3 across the channels),
# columns l % 29 == 5 are constant across the channels (rstd = 316.2).  Affine rows alternate in sign, so the rows either side of
# every segment boundary differ by more than 1 in every channel: a column served by its neighbour's row misses every bar.
def colnorm_segs(L):
    return (1, 61, L)


def colnorm_case(C=33, L=257, B=1, gb_seg=0, gamma_plus_one=False):
    g = _gen(5, C, L, gb_seg)
    x = torch.randn(B, C, L, generator=g)
    cols = torch.arange(L)
    x[:, :, cols % 17 == 3] += 1e3
    x[:, :, cols % 29 == 5] = 2.5
    G = (L + gb_seg - 1) // gb_seg if gb_seg else B
    sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).view(G, 1)
    gamma = sign * (0.6 + 0.3 * torch.rand(G, C, generator=g))
    beta = -sign * (0.6 + 0.3 * torch.rand(G, C, generator=g))
    return dict(x=x, kw=dict(pro=R.PRO_COLNORM, gamma=gamma, beta=beta, gamma_plus_one=gamma_plus_one, gb_seg=gb_seg))


def hard_cases(C=None, L=257):
    """name -> case for every hard tensor of section 3 (C = None: one channel per row class; the fused routes pass 24 / 40 / 72)."""
    out = {"adain_leaky": adain_case(False, C or ADAIN_C, L), "adain_snake": adain_case(True, C or ADAIN_C, L),
           "snake": snake_case(C or SNAKE_C, L), "colnorm": colnorm_case(C or 33, L, B=2)}
    for s in LEAKY_SLOPES:
        out["leaky_%g" % s] = leaky_case(s, C or LEAKY_C, L)
    return out


# ---- section 5: arguments of the epilogue activations -------------------------------------------------------------------------
EPI_L = 130  # four full 32-column blocks (the straight-line build where rows_ok holds) and one that straddles the row end
EPI_MAGS = {
    R.ACT_GELU: (1e-4, 1.0, 6.0, 10.0), R.ACT_GELU_TANH: (1e-4, 1.0, 6.0, 10.0), R.ACT_TANH: (1e-4, 9.0, 20.0),
    R.ACT_LEAKY: (1e-3, 1.0, 1e3, 6e4),
}
EPI_EXP = ((-80.0, -60.0), (-1.0, 1.0), (60.0, 80.0), (-80.0, 80.0))  # exp rows: the range of each channel, ends present
EPI_SIN = (1e1, 1e2, 1e3, 1e4)  # sin rows: on (even channels) and halfway between (odd) multiples of pi, up to this many rad


def epilogue_split(C):
    """act_split of ACT_EXP_SIN: strictly inside the channel range and in neither 8-channel nor 32-channel step with it."""
    return C // 2 - 3


def epilogue_args(act, C, L=EPI_L, B=2):
    """x [B, C, L]: channel c holds one magnitude of the activation's list -- the value itself in column 0, then signs alternating
    along L (ACT_LEAKY: all negative) under a +-5 % jitter."""
    g = _gen(6, act, C, L)
    x = torch.empty(B, C, L)
    if act == R.ACT_EXP_SIN:
        sp = epilogue_split(C)
        for c in range(C):
            if c < sp:
                lo, hi = EPI_EXP[c % len(EPI_EXP)]
                x[:, c] = lo + (hi - lo) * torch.rand(B, L, generator=g)
                x[:, c, 0], x[:, c, -1] = lo, hi
            else:
                reach = EPI_SIN[(c // 2) % len(EPI_SIN)]
                kmax = int(reach / math.pi - (0.5 if c % 2 else 0.0))
                k = torch.round(torch.linspace(-kmax, kmax, L, dtype=torch.float64)) + (0.5 if c % 2 else 0.0)
                x[:, c] = (k * math.pi).float()
                x[1, c] = -x[1, c].flip(0)
        return x
    mags = EPI_MAGS[act]
    sign = torch.where(torch.arange(L) % 2 == 0, 1.0, -1.0)
    if act == R.ACT_LEAKY:
        sign = -torch.ones(L)
    for c in range(C):
        m = mags[c % len(mags)]
        x[:, c] = m * sign * (1.0 + 0.05 * (2 * torch.rand(B, L, generator=g) - 1))
        x[:, c, 0], x[:, c, 1] = m * sign[0], m * sign[1]
    return x
