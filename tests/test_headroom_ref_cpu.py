"""tests/_headroom_ref.py on planes small enough to work out by hand: the reference the device's telemetry rows are held to
(tests/test_headroom_edges_gpu.py) must itself be right at both ends of the f16 range and on an empty operand."""
import math

import numpy as np
import pytest

import _headroom_ref as H

F16 = np.float16


def planes(pairs, shape=(1, 1, 4, 8)):
    """hi / lo planes of `shape`, zero except element i = pairs[i] (hi, lo) in storage order."""
    hi, lo = np.zeros(shape, F16), np.zeros(shape, F16)
    for i, (h, l) in enumerate(pairs):
        hi.flat[i], lo.flat[i] = h, l
    return hi, lo


def test_ulp_of_the_lo_half():
    got = H.ulp_lo(np.array([0.0, 2.0 ** -24, 2.0 ** -15, -(2.0 ** -14), 1.5 * 2.0 ** -14, 1.0, -1.999, 2.0, 16.0]))
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -6]
    assert got.tolist() == want  # 2^-14 is the lowest normal: its spacing is 2^(-14 - 10), the subnormal grid's


@pytest.mark.parametrize("hi,lo,ulp,sub", [
    (65504.0, 0.0, 2.0 ** -24, True),            # the top of the range: lo = 0 counts as "subnormal or zero"
    (-65504.0, 16.0, 2.0 ** -6, False),          # lo at half an ulp of hi = 32 / 2
    (1.0, 2.0 ** -14, 2.0 ** -24, False),        # the lowest normal lo
    (1.0, -(2.0 ** -15), 2.0 ** -24, True),      # the first binade below it
    (2.0 ** -14, 2.0 ** -24, 2.0 ** -24, True),  # the smallest lo there is
    (0.0, 2.0 ** -15, 2.0 ** -24, True),         # hi = 0 alone does not make padding
])
def test_one_element_at_each_end(hi, lo, ulp, sub):
    r = H.row(*planes([(hi, lo)]))
    u = hi + lo
    assert r["max_abs"] == abs(hi) and r["frac"] == abs(hi) / 65504.0
    assert r["rel_err"] == math.sqrt(ulp * ulp * (1.0 / 12.0) / (u * u))
    assert r["sub_share"] == (1.0 if sub else 0.0)


def test_frac_is_one_exactly_at_the_clamp():
    assert H.row(*planes([(65504.0, 0.0), (3.0, 0.0)]))["frac"] == 1.0


def test_all_zero_planes_give_a_finite_row():
    """No element enters a sum: [8] and [9] are 0 by definition (the kernel's `su2 > 0 ? ... : 0`), not 0 / 0."""
    with np.errstate(all="raise"):
        r = H.row(*planes([]))
    assert r == {"max_abs": 0.0, "frac": 0.0, "rel_err": 0.0, "sub_share": 0.0}
    r = H.row(*planes([(0.0, -0.0), (-0.0, 0.0)]))  # signed zeros are zeros
    assert r == {"max_abs": 0.0, "frac": 0.0, "rel_err": 0.0, "sub_share": 0.0}


def test_mixed_plane_by_hand():
    """Four elements, one per class; zeros elsewhere are skipped whatever the plane's size."""
    pairs = [(65504.0, 0.0), (1.0, 2.0 ** -14), (1.0, 2.0 ** -15), (0.0, 0.0), (-8.0, 2.0 ** -9)]
    for shape in ((1, 1, 4, 8), (2, 3, 5, 8)):
        r = H.row(*planes(pairs, shape))
        us = [65504.0, 1.0 + 2.0 ** -14, 1.0 + 2.0 ** -15, -8.0 + 2.0 ** -9]
        ulps = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -19]
        su2 = math.fsum(u * u for u in us)
        se2 = math.fsum(q * q * (1.0 / 12.0) for q in ulps)
        assert r["max_abs"] == 65504.0 and r["frac"] == 1.0
        assert r["rel_err"] == math.sqrt(se2 / su2)
        assert r["sub_share"] == (us[0] ** 2 + us[2] ** 2) / su2


def test_expected_planes_of_the_reproducible_prologues():
    x = np.zeros((2, 9, 5), np.float32)
    x[0, 0] = [1.0, -2.0, 65504.0, 70000.0, float("nan")]
    x[0, 8] = [0.1, -0.1, 1e-3, -1e-3, 3.0]
    x[1] = 7.0
    hi, lo = H.expected_planes(x, 1.0, halo=2, lengths=[5, 3], cg=4, Lp=16)
    assert hi.shape == lo.shape == (2, 4, 16, 8) and hi.dtype == F16
    assert hi[0, 0, 2:7, 0].tolist() == [1.0, -2.0, 65504.0, 65504.0, -65504.0] and not lo[0, 0, 2:7, 0].any()
    f = np.float32
    assert hi[0, 1, 2, 0] == F16(f(0.1)) and lo[0, 1, 2, 0] == F16(f(0.1) - f(F16(f(0.1))))
    assert not hi[:, :, :2].any() and not hi[:, :, 7:].any() and not hi[:, 2:].any() and not hi[:, 1, :, 1:].any()
    assert (hi[1, 0, 2:5] == 7.0).all() and not hi[1, :, 5:].any(), "row 1 ends at its length"
    # LeakyReLU, then the scale; a NaN past a row's end is padding
    x[1, :, 3:] = float("nan")
    hi, lo = H.expected_planes(x, 4.0, lengths=[5, 3], pro=H.PRO_LEAKY, slope=0.2)
    assert hi.shape == (2, 2, 5, 8)
    u = f(f(-2.0) * f(0.2)) * f(4.0)
    assert hi[0, 0, 1, 0] == F16(u) and lo[0, 0, 1, 0] == F16(u - f(F16(u))) and lo[0, 0, 1, 0] != 0
    assert hi[0, 0, 0, 0] == 4.0 and np.isfinite(hi.astype(np.float64)).all() and not hi[1, :, 3:].any()
    r = H.row(hi, lo)
    assert r["max_abs"] == 65504.0 and 0.0 < r["rel_err"] < 1e-6 and 0.0 <= r["sub_share"] <= 1.0
    # padding adds nothing: the same tensor in wider planes gives the same row
    assert H.row(*H.expected_planes(x, 4.0, halo=3, lengths=[5, 3], pro=H.PRO_LEAKY, slope=0.2, cg=8, Lp=40)) == r
