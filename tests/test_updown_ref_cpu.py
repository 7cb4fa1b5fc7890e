"""The references of tests/test_updown_kernels_edges_gpu.py (tests/_updown_ref.py) against independent statements of the same
operations, and the bars of those tests against wrong references: a bar that lets a wrong index through proves nothing.

convt_ref      against F.conv_transpose1d (+ ReflectionPad1d((1, 0)) + add) through weights.polyphase_convt, in float64.
finalize_ref   of make_part(y) against the direct float64 mean / rstd of y.
Wrong references (no mutated kernel is run anywhere): pad off by one, the reflected sample from column 0, phase rows ordered
co * stride + r, one slot dropped, a last slot counted at full width."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _updown_ref as U
from oracle import ops_ref as R
from styletts2_amd import weights


# ---- convt_ref ------------------------------------------------------------------------------------------------------------------
# stride 6 and 10: compile-time builds of the kernel; 1, 4, 7: generic.  (C_in, C_out, stride, pad, output_padding, L, reflect)
@pytest.mark.parametrize("C_in,C_out,s,p,op,L,reflect", [(5, 3, 6, 3, 0, 37, True), (4, 3, 10, 5, 0, 9, False),
                                                        (3, 4, 4, 2, 0, 21, False), (4, 2, 7, 3, 1, 13, True),
                                                        (3, 3, 1, 0, 0, 30, True), (2, 3, 3, 2, 1, 1, False)])
def test_convt_ref_is_conv_transpose1d_in_float64(C_in, C_out, s, p, op, L, reflect):
    gen = torch.Generator().manual_seed(10 * s + L)
    x = torch.randn(2, C_in, L, generator=gen, dtype=torch.float64)
    w = torch.randn(C_in, C_out, 2 * s, generator=gen, dtype=torch.float64) * 0.3
    b = torch.randn(C_out, generator=gen, dtype=torch.float64)
    want = F.conv_transpose1d(x, w, b, stride=s, padding=p, output_padding=op)
    L_raw = want.shape[2]
    if reflect:
        want = F.pad(want, (1, 0), mode="reflect")
    add = torch.randn(want.shape, generator=gen, dtype=torch.float64)
    want = want + add
    # the polyphase GEMM of the product: a k = 2 conv, pad_left = 1, L + 1 columns
    Y = F.conv1d(F.pad(x, (1, 1)), weights.polyphase_convt(w, s))
    assert Y.shape == (2, s * C_out, L + 1)
    got = U.convt_ref(Y, C_out, s, p, L_raw, bias=b, add=add, reflect_left=reflect)
    assert got.dtype == torch.float64 and got.shape == want.shape
    e = (got - want).abs().max().item()
    print("convt_ref vs conv_transpose1d: %.3e" % e)
    assert e < 1e-12
    # a column the GEMM did not produce is the transposed conv's zero padding: the same as that column holding zeros
    Yz = Y.clone()
    Yz[:, :, L:] = 0.0
    assert torch.equal(U.convt_ref(Y[:, :, :L], C_out, s, p, L_raw, bias=b, add=add, reflect_left=reflect),
                       U.convt_ref(Yz, C_out, s, p, L_raw, bias=b, add=add, reflect_left=reflect))


def _convt_case(s=6, pad=3, L_raw=1029, C=3, extra=2):
    gen = torch.Generator().manual_seed(77)
    Lq = U.convt_cols(s, pad, L_raw) + extra
    ph = torch.randn(2, s * C, Lq, generator=gen)
    bias = torch.randn(C, generator=gen)
    add = torch.randn(2, C, L_raw + 1, generator=gen)
    return ph, bias, add, dict(C_out=C, stride=s, pad=pad, L_raw=L_raw)


def test_convt_ref_in_float32_is_the_contract_where_the_columns_suffice():
    ph, bias, add, k = _convt_case()
    got = U.convt_ref(ph, k["C_out"], k["stride"], k["pad"], k["L_raw"], bias=bias, add=add, reflect_left=True)
    assert got.dtype == torch.float32
    U.assert_bitwise(got, R._convt_interleave(ph, k["C_out"], k["stride"], k["pad"], k["L_raw"], bias=bias, add=add,
                                              reflect_left=True), "fp32 contract")
    # and the float64 run of the same contract is the float32 one to float32 round-off of two adds
    g64 = U.convt_ref(ph.double(), k["C_out"], k["stride"], k["pad"], k["L_raw"], bias=bias.double(), add=add.double(),
                      reflect_left=True)
    assert (got.double() - g64).abs().max().item() < 4 * 2.0 ** -24 * g64.abs().max().item()


def test_addressed_mask_is_what_the_contract_reads():
    """NaN in every (phase, column) the mask leaves out does not reach the reference; NaN in any one it names does."""
    for (s, pad, L_raw) in [(6, 13, 40), (4, 0, 5), (7, 6, 1), (2, 5, 9)]:
        Lq = U.convt_cols(s, pad, L_raw) + 3
        m = U.convt_addressed(s, pad, L_raw, Lq)
        assert int(m.sum()) == L_raw
        assert not m[:, :pad // s].any() and not m[:, U.convt_cols(s, pad, L_raw):].any()
        ph = torch.randn(1, s * 2, Lq)
        phn = U.convt_poison(ph, 2, s, pad, L_raw)
        assert int(torch.isnan(phn).sum()) == 2 * (s * Lq - L_raw)
        out = U.convt_ref(phn, 2, s, pad, L_raw)
        U.assert_bitwise(out, U.convt_ref(ph, 2, s, pad, L_raw), "s=%d pad=%d" % (s, pad))
        r, q = (int(v) for v in m.nonzero()[L_raw // 2])
        one = ph.clone()
        one[0, r * 2 + 1, q] = float("nan")
        assert bool(torch.isnan(U.convt_ref(one, 2, s, pad, L_raw)).any())


def test_bitwise_bar_rejects_wrong_convt_references():
    ph, bias, add, k = _convt_case()
    C, s, pad, L_raw = k["C_out"], k["stride"], k["pad"], k["L_raw"]
    good = U.convt_ref(ph, C, s, pad, L_raw, bias=bias, add=add, reflect_left=True)
    U.assert_bitwise(good.clone(), good, "the reference itself")
    # pad off by one (either way)
    for dp in (-1, 1):
        with pytest.raises(AssertionError):
            U.assert_bitwise(U.convt_ref(ph, C, s, pad + dp, L_raw, bias=bias, add=add, reflect_left=True), good, "pad %+d" % dp)
    # the reflected sample from column 0 instead of column 1: one element of each row is wrong
    raw = U.convt_ref(ph, C, s, pad, L_raw, bias=bias)
    col0 = torch.cat([raw[:, :, 0:1], raw], dim=2) + add
    assert int((col0 != good).sum()) == 2 * C
    with pytest.raises(AssertionError):
        U.assert_bitwise(col0, good, "reflect from column 0")
    # phase rows ordered co * stride + r instead of r * C + co
    swapped = ph.reshape(2, C, s, -1).permute(0, 2, 1, 3).reshape(ph.shape)
    with pytest.raises(AssertionError):
        U.assert_bitwise(U.convt_ref(swapped, C, s, pad, L_raw, bias=bias, add=add, reflect_left=True), good, "row order")
    # one fp32 ulp in one element
    ulp = good.clone()
    ulp[1, 2, 1024] = torch.nextafter(ulp[1, 2, 1024], torch.tensor(10.0))
    with pytest.raises(AssertionError):
        U.assert_bitwise(ulp, good, "one ulp")


# ---- make_part / finalize_ref -----------------------------------------------------------------------------------------------------
def _rows(seed, rows, L):
    """Unit-scale rows with their own offsets of 1 .. 4 (either sign), float32."""
    gen = torch.Generator().manual_seed(seed)
    off = (1.0 + 3.0 * torch.rand(rows, 1, generator=gen)) * torch.where(torch.rand(rows, 1, generator=gen) < 0.5, -1.0, 1.0)
    return (torch.randn(rows, L, generator=gen) * 0.5 + off).float()


def _direct(y, eps=1e-5):
    y = y.double()
    return y.mean(-1).numpy(), (1.0 / torch.sqrt(y.var(-1, unbiased=False) + eps)).numpy()


@pytest.mark.parametrize("cols,L,extra", [(32, 1, 0), (32, 62 * 32 + 5, 2), (32, 64 * 32, 0), (32, 64 * 32 + 1, 3), (64, 129 * 64 - 7, 1),
                                          (128, 100, 0), (128, 5 * 128 + 1, 4), (1024, 1025, 0), (1024, 2 * 1024 + 3, 2)])
def test_finalize_ref_of_make_part_is_the_direct_statistics(cols, L, extra):
    rows = 5
    y = _rows(L + cols, rows, L)
    nt = -(-L // cols) + extra
    part = U.make_part(y, cols, nt)
    assert part.dtype == torch.float32 and part.numel() == rows * nt * 3
    assert int(torch.isnan(part).sum()) == rows * extra * 3  # unused slots, and only they, hold NaN
    st = U.finalize_ref(part, rows, nt, L, cols)
    mean, rstd = _direct(y)
    em, er = np.abs(st[:, 0] - mean) / np.abs(mean), np.abs(st[:, 1] - rstd) / rstd
    print("finalize_ref cols=%d L=%d: mean %.3e rstd %.3e" % (cols, L, em.max(), er.max()))
    assert em.max() < 1e-6 and er.max() < 1e-6
    U.assert_stats(st, y, "the reference at the secondary bar")


def test_finalize_ref_with_lengths_clamps_and_shares_them():
    B, C, L, cols = 3, 2, 300, 64
    y = _rows(5, B * C, L)
    raw = [0, 130, L + 9]  # clamped to 1 and L; 130 ends mid-slot
    lens = U.row_lengths(B * C, L, raw, C)
    assert lens == [1, 1, 130, 130, 300, 300]
    nt = 6
    st = U.finalize_ref(U.make_part(y, cols, nt, lengths=lens), B * C, nt, L, cols, lengths=raw, len_div=C)
    for r, n in enumerate(lens):
        mean, rstd = _direct(y[r:r + 1, :n])
        assert abs(st[r, 0] - mean[0]) < 1e-6 * abs(mean[0]) and abs(st[r, 1] - rstd[0]) < 1e-6 * rstd[0]
    # len_div = 1: one entry per row
    raw1 = [64, 65, 1, 299, 128, 300]
    st1 = U.finalize_ref(U.make_part(y, cols, nt, lengths=raw1), B * C, nt, L, cols, lengths=raw1, len_div=1)
    for r, n in enumerate(raw1):
        mean, rstd = _direct(y[r:r + 1, :n])
        assert abs(st1[r, 0] - mean[0]) < 1e-6 * abs(mean[0]) and abs(st1[r, 1] - rstd[0]) < 1e-6 * rstd[0]
    # a row of one column: variance 0, rstd = 1 / sqrt(eps) with eps through float32
    assert st[0, 0] == float(y[0, 0]) and st[0, 1] == 1.0 / np.sqrt(np.float64(np.float32(1e-5)))


def _mutants(cols, L, seed):
    """(reference, {name: wrong reference}, y) for one row set: the slots of `finalize_ref`, combined wrongly."""
    rows = 4
    y = _rows(seed, rows, L)
    ns = -(-L // cols)
    part = U.make_part(y, cols, ns).numpy()
    sums = part[:rows * ns * 2].reshape(rows, ns, 2).astype(np.float64)
    sh = part[rows * ns * 2:].reshape(rows, ns).astype(np.float64)
    eps = np.float64(np.float32(1e-5))
    n = U.slot_counts(L, cols, ns)
    full = n.copy()
    full[-1] = cols
    comb = lambda keep, cnt: np.array([U.chan_combine(cnt[keep], sums[r, keep, 0], sums[r, keep, 1], sh[r, keep], L, eps)
                                       for r in range(rows)])
    everything = np.arange(ns)
    wrong = {"last slot dropped": comb(everything[:-1], n), "a middle slot dropped": comb(np.delete(everything, ns // 2), n),
             "last slot at full width": comb(everything, full)}
    return U.finalize_ref(part, rows, ns, L, cols), wrong, y


# 200 slots of 32 with a last slot of one column, 65 slots of 64 with a last slot of one, 3 slots of 1024 with a last slot of 3
@pytest.mark.parametrize("cols,L", [(32, 199 * 32 + 1), (64, 64 * 64 + 1), (1024, 2 * 1024 + 3), (128, 128 + 60)])
def test_both_bars_reject_a_dropped_slot_and_a_full_width_last_slot(cols, L):
    ref, wrong, y = _mutants(cols, L, cols + L)
    ymax = y.abs().max(-1).values.numpy()
    U.assert_finalize(ref.astype(np.float32), ref, ymax, "the reference, rounded")
    U.assert_stats(ref.astype(np.float32), y, "the reference, rounded")
    for name, st in wrong.items():
        with pytest.raises(AssertionError):
            U.assert_finalize(st.astype(np.float32), ref, ymax, name)
        with pytest.raises(AssertionError):
            U.assert_stats(st.astype(np.float32), y, name)


def test_primary_bar_is_one_ulp():
    ref = np.array([[3.0, 2.0], [1e-9, 316.0]])
    ymax = np.array([4.0, 2.0])
    up = lambda v, k: np.float32(v) + k * np.spacing(np.float32(v))
    U.assert_finalize(np.array([[up(3.0, 1), up(2.0, -1)], [1e-9 + 1e-12, up(316.0, 1)]], dtype=np.float32), ref, ymax, "one ulp")
    for bad in ([[up(3.0, 2), 2.0], [1e-9, 316.0]], [[3.0, up(2.0, 2)], [1e-9, 316.0]], [[3.0, 2.0], [1e-9 + 1e-11, 316.0]]):
        with pytest.raises(AssertionError):
            U.assert_finalize(np.array(bad, dtype=np.float32), ref, ymax, "two ulp")
