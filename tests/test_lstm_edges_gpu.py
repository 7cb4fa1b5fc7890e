"""Both BiLSTM recurrence kernels (st2_lstm_bidir: one CU per row and direction; st2_lstm_bidir_coop: W_hh register resident
over 8 workgroups per group of U rows) against a float64 reference, on every build of the cooperative kernel, over long
chains, on hard gates and with the operands the C++ plans hand them (strided views, ragged rows, padding that is never read).

Every test calls ops.lstm_bidir directly with a G made on the host: the same fp32 G goes to the kernel and, converted, to the
reference (tests/_lstm_ref.py, held to nn.LSTM in float64 by tests/test_lstm_ref_cpu.py); the input-projection conv is not under
test here.  H = 256, W_hh drawn as nn.LSTM draws it (uniform +- 1/16) unless a case says otherwise.  Outputs go into a slice of
a larger sentinel-filled buffer and the sentinels are checked afterwards.

Bars.  Errors are absolute (|h| < 1).  Benign data: the 2e-5 of test_lstm_bidir_matches_torch_lstm.  Long and hard cases:
max(2e-5, 4 x e32) with e32 the error of the float32 run of the same reference code against its float64 run on the same inputs
-- 4 for a different but legitimate summation order; the kernel's own output never enters a bar.  Those cases print their
(kernel error, fp32-contract error) pair before they assert (pytest -s); the pairs measured on an MI355X are written beside them.

The cooperative kernel's per-row arithmetic does not depend on U (part[u][gate][k slice][unit], the 8 k slices summed ascending;
each row's mat-vec reads only its own hs[u]): a row's result is bitwise the same alone and inside any block, which
test_a_row_does_not_know_its_neighbours holds it to."""
import numpy as np
import pytest
import torch

import _lstm_cases as K
import _lstm_ref as L
from styletts2_amd import _hooks, _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
NAN = float("nan")
H = K.H
PLAIN = 2e-5  # test_lstm_bidir_matches_torch_lstm's bar


@pytest.fixture(autouse=True)
def _own_status():
    """Each case is judged by the status bits of its own launches only (the word is sticky)."""
    torch.cuda.synchronize()
    ops.status(clear=True)


def hard_bar(what, e_kernel, e_fp32, plain):
    """max(plain bar, 4 x the fp32 contract's own error on these inputs); prints the measured pair."""
    bar = max(plain, 4.0 * e_fp32)
    print("HARD %s: kernel %.3e  fp32-contract %.3e  bar %.3e" % (what, e_kernel, e_fp32, bar))
    return bar


def _lens_dev(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _frame(B, N, col0=0):
    """A [B, 2H, N] output view two channel rows and `col0` columns inside a sentinel-filled buffer of its own."""
    big = torch.full((B, 2 * H + 4, col0 + N + 3), SENT, device=DEV)
    return big, big[:, 2:2 + 2 * H, col0:col0 + N]


def _frame_untouched(big, N, col0=0):
    chk = big.clone()
    chk[:, 2:2 + 2 * H, col0:col0 + N] = SENT
    return bool((chk == SENT).all())


def _run(G, whh, lens, mode=None):
    """ops.lstm_bidir into a sentinel frame; G, whh on the device, lens a list or None.  Returns the output view (checked: the
    frame is untouched, no status bit, no cooperative time-out)."""
    B, _, N = G.shape
    big, view = _frame(B, N)
    out = ops.lstm_bidir(G, whh, _lens_dev(lens), out=view)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    assert ops.lstm_coop_status() == 0, "a cooperative LSTM group timed out"
    assert ops.status() == 0, hex(ops.status())
    assert _frame_untouched(big, N), "the kernel wrote outside its output view"
    return out


def _err(out, ref):
    return float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())


def _tail_is_zero(out, valid):
    """Exact zeros at t >= len[b]."""
    o = out.cpu().numpy()
    return not o[~np.broadcast_to(valid, o.shape)].any()


class _forced_block:
    """st2_lstm_coop_set_block(U) for the duration of a `with`; 0 = the library's rule."""

    def __init__(self, U):
        self.U = U

    def __enter__(self):
        if self.U:
            _lib.load().st2_lstm_coop_set_block(self.U)

    def __exit__(self, *exc):
        _lib.load().st2_lstm_coop_set_block(0)


def _coop_bytes(B, U):
    """st2_lstm_coop_scratch_bytes for B rows in blocks of U: head (status + one counter per group, to 256 bytes) + two
    buffers of U x H 8-byte granules per group -- the size tells which build the library picked."""
    groups = 2 * ((B + U - 1) // U)
    return ((1 + groups) * 4 + 255) // 256 * 256 + groups * 2 * U * H * 8


# ---- 1. every build ---------------------------------------------------------------------------------------------------------
# block_size(B): U = 1 for B = 1, 4 up to B = 32, 8 for B = 33 .. 48, no cooperative launch above (0 scratch bytes: the
# single-CU kernel).  (B, forced block, U that runs): partial last blocks at B = 5 (4 + 1), 33 (4 x 8 + 1), 41 (5 x 8 + 1),
# 3 forced to 2 (2 + 1) and 9 forced to 8 (8 + 1).
BUILDS = [(1, 0, 1), (5, 0, 4), (32, 0, 4), (33, 0, 8), (41, 0, 8), (48, 0, 8), (49, 0, 0), (3, 2, 2), (3, 1, 1), (9, 8, 8)]
BUILD_CASES = [("coop",) + b for b in BUILDS] + [("single",) + b for b in BUILDS if b[1] == 0]


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("mode,B,forced,U", BUILD_CASES, ids=["%s_B%d_f%d_U%d" % c for c in BUILD_CASES])
def test_every_build_matches_fp64(mode, B, forced, U, ragged, monkeypatch):
    """N = 40; ragged rows follow _lstm_cases.block_lengths: len = 1, N and N - 1 inside one block, the longest row never first."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    case = K.build_case(B, ragged)
    G, whh = case.G.to(DEV), case.whh_t.to(DEV)
    with _forced_block(forced):
        if mode == "coop":  # the build that is about to run is the one this case is for
            assert _lib.load().st2_lstm_coop_scratch_bytes(B) == (_coop_bytes(B, U) if U else 0)
        out = _run(G, whh, case.lens)
        again = _run(G, whh, case.lens) if not ragged else None
    e = _err(out, case.ref)
    print("lstm %s B=%d U=%d %s: %.3e" % (mode, B, U, "ragged" if ragged else "uniform", e))
    assert e < PLAIN
    assert _tail_is_zero(out, case.valid)
    if again is not None:
        assert torch.equal(out, again), "bitwise reproducible"


# ---- 2. a row does not know its neighbours ----------------------------------------------------------------------------------
ROW_N, ROW_LEN = 40, 29
# (mode, B, forced block): the fixed row first, fourth and last in the batch
NEIGHBOUR_CASES = [("coop", 5, 0), ("coop", 33, 0), ("coop", 48, 0), ("coop", 5, 2), ("coop", 9, 8),
                   ("single", 5, 0), ("single", 33, 0), ("single", 49, 0)]


@pytest.mark.parametrize("mode,B,forced", NEIGHBOUR_CASES, ids=["%s_B%d_f%d" % c for c in NEIGHBOUR_CASES])
def test_a_row_does_not_know_its_neighbours(mode, B, forced, monkeypatch):
    """One fixed row (length 29 of N = 40) alone at B = 1 and as row 0, row 3 and the last row of a batch whose other rows are
    shorter, longer and full: bitwise equal (and both at the fp64 bar)."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    whh = K.whh(1).to(DEV)
    row = K.randn(4242, 1, 8 * H, ROW_N)
    ref = L.lstm_bidir(row.numpy(), K.whh(1).numpy(), [ROW_LEN])
    alone = _run(row.to(DEV), whh, [ROW_LEN])
    assert _err(alone, ref) < PLAIN
    others = K.randn(4300 + B, B, 8 * H, ROW_N)
    for pos in (0, 3, B - 1):
        G = others.clone()
        G[pos] = row[0]
        lens = K.block_lengths(B, ROW_N)
        lens[pos] = ROW_LEN
        with _forced_block(forced):
            out = _run(G.to(DEV), whh, lens)
        assert torch.equal(out[pos], alone[0]), "row %d of %d differs from its solo run by %.3e" % (
            pos, B, (out[pos] - alone[0]).abs().max().item())


# ---- 3. long chains ---------------------------------------------------------------------------------------------------------
# over a thousand hand-offs through the two granule buffers (tags s + 1, buffer s & 1), exchange form 2 (the default)
# measured on an MI355X (kernel error, fp32-contract error), bar 2e-5 in all four:
#   N = 400:  coop 1.6e-7, 1.6e-7   single 1.7e-7, 1.6e-7        N = 1201: coop 2.3e-7, 2.0e-7   single 2.3e-7, 2.0e-7
# (no growth with the chain length: the recurrence at +- 1/16 forgets its round-off; 0.4 s for the 1201-step cooperative case,
# most of it the host's reference)
@pytest.mark.parametrize("mode", ["coop", "single"])
@pytest.mark.parametrize("N", K.LONG_N)
def test_long_chains(N, mode, monkeypatch):
    monkeypatch.setattr(_hooks, "lstm", mode)
    case = K.long_case(N)
    out = _run(case.G.to(DEV), case.whh_t.to(DEV), case.lens)
    e = _err(out, case.ref)
    assert e <= hard_bar("lstm %s N=%d" % (mode, N), e, case.e32, PLAIN)
    assert _tail_is_zero(out, case.valid)


# ---- 4. hard gates ----------------------------------------------------------------------------------------------------------
# measured on an MI355X (kernel error, fp32-contract error):
#   saturated   (8.9 % of |a| > 20, a in -181 .. 174): coop 4.7e-7, 4.6e-7   single 4.7e-7, 4.6e-7   -> bar 2e-5
#   long_memory (max |c| = 67):                        coop 8.9e-5, 8.7e-5   single 1.05e-4, 8.7e-5  -> bar 3.5e-4
#   large_whh   (e32 5.0 x the benign 1.6e-7):         coop 2.6e-7, 8.2e-7   single 6.3e-7, 8.2e-7   -> bar 2e-5
@pytest.mark.parametrize("mode", ["coop", "single"])
@pytest.mark.parametrize("kind", K.HARD_KINDS)
def test_hard_gates(kind, mode, monkeypatch):
    """N = 300, B = 4 (_lstm_cases.hard_case): saturated gates with exp(-a) over- and underflowing, a cell state that grows for
    hundreds of steps, recurrent weights four times nn.LSTM's.  Each case's condition is checked on the float64 run alone."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    print("%s: %s" % (kind, K.hard_condition(kind)))
    case = K.hard_case(kind)
    out = _run(case.G.to(DEV), case.whh_t.to(DEV), case.lens)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    e = _err(out, case.ref)
    assert e <= hard_bar("lstm %s %s" % (mode, kind), e, case.e32, PLAIN)
    assert _tail_is_zero(out, case.valid)


# ---- 5. padding is never read -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coop", "single"])
def test_padding_is_never_read(mode, monkeypatch):
    """G[b, :, len[b]:] = NaN: bit for bit the run with finite padding, exact zeros past the lengths, no status bit."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    case = K.build_case(9, True)
    pad = torch.from_numpy(~np.broadcast_to(case.valid, tuple(case.G.shape)))
    Gn = case.G.masked_fill(pad, NAN)
    assert bool(torch.isnan(Gn).any())
    whh = case.whh_t.to(DEV)
    plain = _run(case.G.to(DEV), whh, case.lens)
    nan = _run(Gn.to(DEV), whh, case.lens)
    assert bool(torch.isfinite(nan).all())
    assert torch.equal(plain, nan)
    assert _tail_is_zero(nan, case.valid)
    assert _err(nan, case.ref) < PLAIN


# ---- 6. strided operands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coop", "single"])
def test_strided_operands(mode, monkeypatch):
    """What the C++ plans hand the kernels: G a channel slice [:, 3:3 + 8H] of a wider buffer with a row pitch of N + 5 (NaN all
    around it), out a slice [:, 2:2 + 2H] of a sentinel-filled buffer with a pitch of N + 3: bitwise the contiguous call."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    case = K.build_case(5, True)
    B, N = case.B, case.N
    whh = case.whh_t.to(DEV)
    flat = _run(case.G.to(DEV), whh, case.lens).contiguous()
    wide = torch.full((B, 8 * H + 7, N + 5), NAN, device=DEV)
    Gv = wide[:, 3:3 + 8 * H, :N]
    Gv.copy_(case.G)
    assert Gv.stride() == ((8 * H + 7) * (N + 5), N + 5, 1)
    big, view = _frame(B, N)
    assert view.stride() == ((2 * H + 4) * (N + 3), N + 3, 1)
    out = ops.lstm_bidir(Gv, whh, _lens_dev(case.lens), out=view)
    torch.cuda.synchronize()
    assert ops.lstm_coop_status() == 0 and ops.status() == 0
    assert torch.equal(out, flat)
    assert _frame_untouched(big, N)
    assert _err(out, case.ref) < PLAIN


# ---- 7. length values at the boundary of the contract -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["coop", "single"])
def test_lengths_zero_and_past_the_end(mode, monkeypatch):
    """The wrapper checks the lengths tensor's type, shape and device, not its values (they live on the device): 0 gives an
    all-zero row, N + 7 is clamped to N."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    N = 40
    G, W = K.randn(77, 5, 8 * H, N), K.whh(1)
    lens = [0, N + 7, 13, 0, N]
    ref = L.lstm_bidir(G.numpy(), W.numpy(), lens)
    assert np.array_equal(ref, L.lstm_bidir(G.numpy(), W.numpy(), [0, N, 13, 0, N])) and not ref[0].any()
    out = _run(G.to(DEV), W.to(DEV), lens)
    assert _err(out, ref) < PLAIN
    assert float(out[0].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0
    assert _tail_is_zero(out, L.valid_mask(lens, 5, N))
    zeros = _run(G.to(DEV), W.to(DEV), [0] * 5)  # a batch of empty rows: no step runs at all
    assert float(zeros.abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["coop", "single"])
def test_negative_length_is_clamped_to_zero(mode, monkeypatch):
    """A device length of -3 is an empty row: all zeros, nothing written in front of it.  The tail-zeroing loop of both kernels
    used to start at the unclamped value, i.e. three floats in front of every channel row.  The output view starts four columns
    and two channel rows inside the test's own buffer, so that even such a kernel stays within this allocation; the columns in
    front are sentinels like the rest of the frame."""
    monkeypatch.setattr(_hooks, "lstm", mode)
    N, COL0 = 40, 4
    G, W = K.randn(78, 4, 8 * H, N), K.whh(1)
    lens = [N, -3, 7, -3]
    ref = L.lstm_bidir(G.numpy(), W.numpy(), lens)
    assert not ref[1].any() and not ref[3].any()
    big, view = _frame(4, N, col0=COL0)
    out = ops.lstm_bidir(G.to(DEV), W.to(DEV), _lens_dev(lens), out=view)
    torch.cuda.synchronize()
    assert ops.lstm_coop_status() == 0 and ops.status() == 0
    assert _frame_untouched(big, N, col0=COL0), "a negative length wrote in front of its row"
    assert float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0
    assert _err(out, ref) < PLAIN
