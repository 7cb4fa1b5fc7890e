"""Edge shapes for the map and frame kernels of the reference-audio path (csrc/st2_style.hip, plain entries): dwconv3x3s2,
avgpool2x2, stft_frames, power_spectrum, log_norm_.  One thread per output column, 256 to a block: widths that give 256 and 257
output columns, maps of one row and of one column.

Maps are interior views of larger buffers: NaN fills the rows above and below the view and the columns right of W (which are
also what lies left of column 0 of the next channel row), so a finite result proves that the zero padding -- and the replicated
last column of the pool -- comes from a select and not from whatever memory sits beside the map.  Outputs are views of
sentinel-filled buffers, checked afterwards.  References are the contracts of oracle/ops_ref.py on float64 copies at the bars
of test_style_kernels_match_contracts (1e-5 / 1e-6 absolute on unit-scale data), bit equality for the two pure gathers /
one-rounding-per-op kernels."""
import math

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from styletts2_amd import ops
from styletts2_amd._lib import St2Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
NAN = float("nan")


@pytest.fixture(autouse=True)
def _own_status():
    """Each case is judged by the status bits of its own launches only (the word is sticky)."""
    torch.cuda.synchronize()
    ops.status(clear=True)


def g(t):
    return None if t is None else t.to(DEV)


def map_view(x):
    """x [B, H, C, W] on the host -> the same values as the interior of a NaN-filled [B, H + 2, C, W + 3] device buffer."""
    B, H, C, W = x.shape
    big = torch.full((B, H + 2, C, W + 3), NAN, device=DEV)
    v = big[:, 1:H + 1, :, :W]
    v.copy_(g(x))
    return v


def guarded(shape, extra=2):
    """(flat sentinel buffer, a view of `shape` whose rows are `extra` floats longer in memory)."""
    big = torch.full(tuple(shape[:-1]) + (shape[-1] + extra,), SENT, device=DEV)
    return big.view(-1), big[..., :shape[-1]]


def assert_untouched(flat, view, what):
    inside = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    assert int(inside.sum()) == view.numel()
    assert bool((flat[~inside] == SENT).all()), "%s: stored outside the view" % what


# ---- dwconv3x3s2 ----------------------------------------------------------------------------------------------------------------
# W 511 / 512 -> 256 output columns (one block), 513 -> 257 (a second block of one thread); H = 1: both neighbour rows are padding
@pytest.mark.parametrize("H", [1, 2, 3, 8])
@pytest.mark.parametrize("W", [1, 2, 3, 511, 512, 513])
def test_dwconv3x3s2_edges(H, W):
    B, C = 2, 3
    has_bias = (H + W) % 2 == 0
    gen = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(B, H, C, W, generator=gen)
    w = torch.randn(C, 3, 3, generator=gen) * 0.5
    bias = torch.randn(C, generator=gen) if has_bias else None
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert Wo == {1: 1, 2: 1, 3: 2, 511: 256, 512: 256, 513: 257}[W]
    ref = R.dwconv3x3s2(x.double(), w.double(), None if bias is None else bias.double(), torch.empty(B, Ho, C, Wo, dtype=torch.float64))
    flat, out = guarded((B, Ho, C, Wo))
    ops.dwconv3x3s2(map_view(x), g(w), g(bias), out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "padding read from memory beside the map"
    e = (out.cpu().double() - ref).abs().max().item()
    print("dwconv3x3s2 H=%d W=%d bias=%d: %.3e" % (H, W, has_bias, e))
    assert e < 1e-5
    assert_untouched(flat, out, "dwconv3x3s2")
    assert ops.status() == 0


# ---- avgpool2x2 -----------------------------------------------------------------------------------------------------------------
# odd widths replicate their own last column (W = 1: the only one); 513 / 514 -> 257 output columns
@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("W", [1, 2, 3, 511, 512, 513, 514])
def test_avgpool2x2_edges(H, W):
    B, C = 2, 3
    gen = torch.Generator().manual_seed(10 * W + H)
    x = torch.randn(B, H, C, W, generator=gen)
    Wo = (W + 1) // 2
    ref = R.avgpool2x2(x.double(), torch.empty(B, H // 2, C, Wo, dtype=torch.float64))
    flat, out = guarded((B, H // 2, C, Wo))
    ops.avgpool2x2(map_view(x), out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "the replicated column read from memory beside the map"
    e = (out.cpu().double() - ref).abs().max().item()
    print("avgpool2x2 H=%d W=%d: %.3e" % (H, W, e))
    assert e < 1e-6
    assert_untouched(flat, out, "avgpool2x2")
    assert ops.status() == 0


@pytest.mark.parametrize("H", [1, 3, 5])
def test_avgpool2x2_refuses_an_odd_height(H):
    x = torch.randn(2, H, 3, 8, device=DEV)
    out = torch.full((2, H // 2, 3, 4), SENT, device=DEV)
    with pytest.raises(St2Error):
        ops.avgpool2x2(x, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- stft_frames ----------------------------------------------------------------------------------------------------------------
def admitted(L, n_win, hop, shift):
    """st2_stft_frames' own condition: 0 <= shift < L (the left reflection shift - 0 stays inside) and the last frame's last tap
    (L / hop) * hop + n_win - 1 - shift reflects once, to an index >= 0."""
    return L > 1 and 0 <= shift < L and (L // hop) * hop + n_win - 1 - shift <= 2 * (L - 1)


# (n_win, hop, shift): the smallest admitted L.
#   product (1200, 300, 600): shift < L needs L >= 601; at L = 601 the last frame starts at 600 and reaches 600 + 1199 - 600 = 1199
#                             <= 2 * 600.  So 601, and 600 fails on the shift.
#   toy (8, 4, 4):            shift < L needs L >= 5; at L = 5 the last frame starts at 4 and reaches 4 + 7 - 4 = 7 <= 2 * 4.  So 5.
GEOMETRIES = {(1200, 300, 600): 601, (8, 4, 4): 5}


def _frame_lengths(geom):
    n_win, hop, shift = geom
    # the smallest; then 256 frames (the last one a partial hop into the signal), 257 and 513
    return [GEOMETRIES[geom], 255 * hop + hop - 1, 256 * hop, 512 * hop + 1]


@pytest.mark.parametrize("geom,L", [(geom, L) for geom in GEOMETRIES for L in _frame_lengths(geom)])
def test_stft_frames_is_bitwise_the_contract(geom, L):
    n_win, hop, shift = geom
    assert admitted(L, n_win, hop, shift)
    B = 2
    gen = torch.Generator().manual_seed(L)
    wave = torch.randn(B, L, generator=gen)
    ref = R.stft_frames(wave, n_win, hop, shift)
    big = torch.full((B, L + 5), NAN, device=DEV)  # nothing at or past L is a sample
    big[:, :L] = g(wave)
    fr = ops.stft_frames(big[:, :L], n_win, hop, shift)
    torch.cuda.synchronize()
    assert fr.shape == (B, n_win, L // hop + 1)
    assert torch.equal(fr.cpu(), ref)
    assert ops.status() == 0


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_stft_frames_smallest_length_is_the_entry_points_own(geom):
    n_win, hop, shift = geom
    L = GEOMETRIES[geom]
    assert L == next(n for n in range(2, 4 * n_win) if admitted(n, n_win, hop, shift)) and not admitted(L - 1, n_win, hop, shift)
    with pytest.raises(St2Error):
        ops.stft_frames(torch.randn(2, L - 1, device=DEV), n_win, hop, shift)
    assert ops.status() == 0


# ---- power_spectrum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_power_spectrum_is_bitwise_the_contract(K, M):
    B = 2
    gen = torch.Generator().manual_seed(10 * M + K)
    y = torch.randn(B, 2 * K, M, generator=gen) * 3.0
    big = torch.full((B, 2 * K + 3, (M + 3) | 1), NAN, device=DEV)  # rows 1 .. 2K + 1 of a wider buffer, odd row pitch
    yv = big[:, 1:2 * K + 1, :M]
    yv.copy_(g(y))
    p = ops.power_spectrum(yv)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), R.power_spectrum(y))  # one rounding per op, contraction off
    assert ops.status() == 0


# ---- log_norm_ (flat entry) -----------------------------------------------------------------------------------------------------
EPS, MEAN, STD = 1e-5, -4.0, 4.0


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_log_norm_flat_edges(n):
    gen = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=gen) * 10.0
    x[::3] = 0.0  # silence: log(eps) and nothing else
    buf = torch.full((n + 8,), SENT, device=DEV)
    buf[:n] = g(x)
    got = ops.log_norm_(buf[:n], EPS, MEAN, STD)
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT).all())
    got = got.cpu()
    ref = (torch.log(EPS + x.double()) - MEAN) / STD
    assert (got.double() - ref).abs().max().item() < 1e-6
    # x = 0: (log(eps) - mean) / std to fp32 round-off.  eps reaches the kernel through fp32 (2^-24 relative: that much absolute in
    # the log); logf is held to the 3 ulp of the OpenCL full profile (the device library documents 1); the subtraction and the
    # division round once each.
    zero = got[::3]
    exact = (math.log(EPS) - MEAN) / STD
    bar = (2.0 ** -24 + 3 * _ulp32(math.log(EPS)) + 0.5 * _ulp32(math.log(EPS) - MEAN)) / STD + 0.5 * _ulp32(exact)
    assert bar < 1e-6
    assert bool((zero == zero[0]).all())
    assert abs(zero[0].item() - exact) <= bar, (zero[0].item(), exact, bar)
    assert ops.status() == 0
