"""References for the split-f16 prologue (csrc/st2_act.h): an fp64 evaluation of the contract and a numpy model of the hi/lo split.
Proved on the CPU by tests/test_prologue_ref_cpu.py, used on the device by tests/test_prologue_edges_gpu.py.

`activate64` is `oracle.ops_ref.activate` evaluated on `.double()` copies of its inputs, with ONE deliberate difference: for the
Snake prologues the sine is taken of the FP32-ROUNDED product alpha * u.  The kernels and the fp32 contract both form that product
in fp32 before the sine, so its rounding (half an ulp of the argument: 5e-4 rad at |alpha u| = 1e4) is part of the operation's
definition, not an error of the code under test; with the fp64 product a test at |alpha u| = 1e4 would measure the ulp of the
argument instead of the kernel.  For PRO_SNAKE (u = x, an fp32 number) the rounded product is bit for bit the kernels' argument.
For PRO_ADAIN_SNAKE u itself is the fp64 affine, so the rounding only removes the part of the argument's error that no fp32
evaluation can avoid; what the affine's own fp32 round-off does to the sine is measured by the fp32 contract on the same inputs.

`split_f16` is the split as st2_split_f16 states it: clamp to the finite f16 range (one median, a NaN becomes -65504), hi = f16(vc),
lo = f16(vc - hi), both round-to-nearest-even, and sat = (vc != w)."""
import numpy as np
import torch

from oracle import ops_ref as R

F16_MAX = 65504.0
SNAKE_PROS = (R.PRO_ADAIN_SNAKE, R.PRO_SNAKE)
NORM_PROS = (R.PRO_ADAIN_LEAKY, R.PRO_ADAIN_SNAKE, R.PRO_COLNORM)
SIN_SQ_ERR = 2.4e-7  # st2_act.h: "sin(x)^2 to ~2.4e-7 absolute"
PLAIN = 3e-6         # the bar of test_activate_planes_match_contract and of the conv contract tests


def x_scale_for(pro):
    """ops.x_scale_for without a library (oracle/ops_ref.py _conv1d states the same rule)."""
    return 8.0 if pro in NORM_PROS else 1.0


def _d(t):
    return t.double() if torch.is_tensor(t) else t


def activate64(x, *, pro=R.PRO_NONE, slope=0.0, stats=None, gamma=None, beta=None, gamma_plus_one=False, alpha=None, gb_seg=0,
               lengths=None):
    """fp64 prologue of x [B, C, L] (see the module docstring for the Snake argument).  `lengths` (a list of ints): row b is zero
    from column min(max(lengths[b], 0), L) on, the conv's zero padding AFTER the activation."""
    xd = x.double()
    if pro in SNAKE_PROS:
        u = xd
        if pro == R.PRO_ADAIN_SNAKE:  # the affine alone: LeakyReLU of slope 1 is the identity
            u = R.activate(xd, pro=R.PRO_ADAIN_LEAKY, slope=1.0, stats=_d(stats), gamma=_d(gamma), beta=_d(beta))
        a = alpha.double().view(1, -1, 1)
        arg = (a * u).float().double()
        y = u + (1.0 / a) * torch.sin(arg) ** 2
    else:
        y = R.activate(xd, pro=pro, slope=slope, stats=_d(stats), gamma=_d(gamma), beta=_d(beta), gamma_plus_one=gamma_plus_one,
                       gb_seg=gb_seg)
    return zero_past(y, lengths)


def activate32(x, *, lengths=None, **kw):
    """The fp32 contract itself on the same inputs (what the bar is taken from)."""
    return zero_past(R.activate(x, **kw), lengths)


def zero_past(y, lengths):
    if lengths is None:
        return y
    y = y.clone()
    L = y.shape[-1]
    for b, n in enumerate(lengths):
        y[b, :, min(max(int(n), 0), L):] = 0
    return y


def split_f16(w):
    """w: float32 array -> (hi, lo, sat): float16, float16, bool arrays of its shape."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        vc = np.where(np.isnan(w), np.float32(-F16_MAX), np.minimum(np.maximum(w, np.float32(-F16_MAX)), np.float32(F16_MAX)))
    vc = vc.astype(np.float32)
    hi = vc.astype(np.float16)
    lo = (vc - hi.astype(np.float32)).astype(np.float16)
    with np.errstate(invalid="ignore"):
        sat = vc != w
    return hi, lo, sat


def ulp_f16(h):
    """Spacing of the f16 grid at h (float array): 2^(e - 10) for a normal h = m * 2^e with m in [1, 2), 2^-24 at and below 2^-14."""
    a = np.abs(np.asarray(h, dtype=np.float64))
    _, e = np.frexp(np.maximum(a, 2.0 ** -14))  # a = f * 2^e, f in [0.5, 1)
    return np.ldexp(1.0, e - 1 - 10)


def split_bound(w):
    """|w - (hi + lo)| <= max(2^-22 |w|, 2^-25) for |w| <= 65504: hi and lo are one f16 rounding each, 2^-11 relative -- lo rounds
    a remainder of at most 2^-11 |w| -- and below 2^-14 the (subnormal) spacing of lo is 2^-24, half of which is 2^-25."""
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(w, dtype=np.float64)), 2.0 ** -25)


def planes_value(data):
    """XsTensor.data [B, 2, cg, Lp, 8] (a CPU tensor) -> (hi, lo) as [B, cg * 8, Lp] float16 tensors."""
    B, _, cg, Lp, _ = data.shape
    hi = data[:, 0].permute(0, 1, 3, 2).reshape(B, cg * 8, Lp)
    lo = data[:, 1].permute(0, 1, 3, 2).reshape(B, cg * 8, Lp)
    return hi, lo


def row_max(t):
    """max |t| over the columns of each (b, channel) row, kept as [B, C, 1]."""
    return t.abs().amax(dim=-1, keepdim=True)


def element_bar(ref, c32, *, x_scale, alpha=None, split=True):
    """(bar [B, C, L], fp32-contract row error [B, C, 1]) in units of u.  ref: the fp64 reference, c32: the fp32 contract on the
    same inputs.  Per element: the derived split bound max(2^-22 |ref|, 2^-25 / x_scale) (`split`; the exact-fp32 conv has none)
    + the arithmetic term of its (b, channel) row, max(3e-6 * max(1, row max |ref|), 4 x the fp32 contract's own error on that
    row) -- the `hard_bar` rule of tests/test_kernel_edges_gpu.py, normalised per row so that a large row cannot hide a small one
    -- + for a Snake channel 2.4e-7 / |alpha|, the stated error of sin_sq times the 1 / alpha that multiplies it.  Nothing the
    kernel computed enters."""
    e32 = row_max(c32.double() - ref)
    bar = torch.maximum(PLAIN * torch.clamp(row_max(ref), min=1.0), 4.0 * e32).expand_as(ref).clone()
    if split:
        bar = bar + torch.clamp(2.0 ** -22 * ref.abs(), min=2.0 ** -25 / x_scale)
    if alpha is not None:
        bar = bar + SIN_SQ_ERR / alpha.double().abs().view(1, -1, 1)
    return bar, e32
