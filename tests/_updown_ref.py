"""References and comparison helpers of tests/test_updown_kernels_edges_gpu.py; tests/test_updown_ref_cpu.py proves them first.

convt_ref      the contract of oracle/ops_ref._convt_interleave on phases zero-padded to the columns the outputs address: the
               kernel reads columns q >= Lq as the transposed conv's zero padding, where the contract's slice would come up short.
make_part      a producer's partial-sum buffer (layout of ops.new_part) from the tensor itself: sums in float64, rounded once.
finalize_ref   st2_stats_finalize's own formula (Chan et al. over shifted slot sums) in numpy float64 on those float32 partials.
assert_*       the bars of the GPU tests, as functions, so that the CPU test can show them rejecting wrong references.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops_ref as R


# ---- convt_interleave ---------------------------------------------------------------------------------------------------------
def convt_cols(stride, pad, L_raw):
    """Phase columns the raw outputs l in [0, L_raw) address: q = (l + pad) // stride <= this - 1."""
    return (L_raw - 1 + pad) // stride + 1


def convt_addressed(stride, pad, L_raw, Lq):
    """bool [stride, Lq]: the (phase r, column q) pairs some output reads (the reflected sample is raw index 1: one of them)."""
    lp = torch.arange(pad, pad + L_raw)
    q, r = lp // stride, lp % stride
    m = torch.zeros(stride, Lq, dtype=torch.bool)
    keep = q < Lq
    m[r[keep], q[keep]] = True
    return m


def convt_poison(phases, C_out, stride, pad, L_raw):
    """A copy of phases [B, stride * C_out, Lq] with NaN in every element no output addresses."""
    B, _, Lq = phases.shape
    p = phases.clone().reshape(B, stride, C_out, Lq).permute(0, 2, 1, 3).contiguous()  # [B, C_out, stride, Lq]
    p[:, :, ~convt_addressed(stride, pad, L_raw, Lq)] = float("nan")
    return p.permute(0, 2, 1, 3).reshape(B, stride * C_out, Lq).contiguous()


def convt_ref(phases, C_out, stride, pad, L_raw, bias=None, add=None, reflect_left=False):
    """phases [B, stride * C_out, Lq] (float32 or float64, row r * C_out + co) -> [B, C_out, L_raw + reflect_left] in the dtype
    of `phases`, by the contract's own operations in the contract's order (gather, + bias, reflect, + add)."""
    need = convt_cols(stride, pad, L_raw)
    if phases.shape[2] < need:
        phases = F.pad(phases, (0, need - phases.shape[2]))
    return R._convt_interleave(phases, C_out, stride, pad, L_raw, bias=bias, add=add, reflect_left=reflect_left)


def assert_bitwise(got, want, what):
    """The bar of every gather kernel: same shape, same dtype, every element equal (NaN equals nothing)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.dtype, tuple(got.shape),
                                                                                      want.dtype, tuple(want.shape))
    if not torch.equal(got, want):
        bad = ~(got == want)
        first = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r vs %r" % (
            what, int(bad.sum()), bad.numel(), first, got[first].item(), want[first].item()))


# ---- stats_finalize -----------------------------------------------------------------------------------------------------------
def slot_counts(L, cols, ns):
    """Columns of slot 0 .. ns - 1 of a row of L columns: `cols` each, the last one what is left."""
    return np.minimum(cols, L - np.arange(ns) * cols).astype(np.float64)


def row_lengths(rows, L, lengths, len_div):
    """The kernel's clamp: row r covers min(max(lengths[r // len_div], 1), L) columns (L without lengths)."""
    if lengths is None:
        return [L] * rows
    lengths = [int(v) for v in lengths]
    assert len(lengths) * len_div == rows
    return [min(max(lengths[r // len_div], 1), L) for r in range(rows)]


def make_part(y, cols, nt, lengths=None):
    """What a producer leaves for st2_stats_finalize: float2 [rows][nt] of (sum, sum of squares) of (y - shift) over each slot of
    `cols` columns, then float [rows][nt] of the shifts, shift = the slot's first value; one flat float32 tensor.  y is [..., L]
    (rows = the product of the leading extents).  Sums in float64, rounded once; slots without columns hold NaN.  `lengths`: one
    column count per row (already clamped to 1 .. L): the row's sums stop there, as a ragged producer's do."""
    y64 = np.asarray(y.detach().cpu().double().numpy() if torch.is_tensor(y) else y, dtype=np.float64)
    L = y64.shape[-1]
    y64 = y64.reshape(-1, L)
    rows = y64.shape[0]
    assert nt * cols >= L
    sums = np.full((rows, nt, 2), np.nan, dtype=np.float32)
    shifts = np.full((rows, nt), np.nan, dtype=np.float32)
    for r in range(rows):
        Lr = L if lengths is None else int(lengths[r])
        assert 1 <= Lr <= L
        for i in range(-(-Lr // cols)):
            seg = y64[r, i * cols:min((i + 1) * cols, Lr)]
            sh = np.float32(seg[0])
            dv = seg - np.float64(sh)
            sums[r, i, 0], sums[r, i, 1], shifts[r, i] = np.float32(dv.sum()), np.float32((dv * dv).sum()), sh
    return torch.from_numpy(np.concatenate([sums.reshape(-1), shifts.reshape(-1)]))


def chan_combine(n, s1, s2, sh, L, eps):
    """(mean, rstd) of a row of L columns from its slots (n_i columns, shifted sums s1_i / s2_i, shifts sh_i), all float64:
    slot mean = sh + s1 / n, slot M2 = s2 - s1^2 / n, row M2 = sum of slot M2 + sum n_i (mean_i - mean)^2, biased variance."""
    mean = (n * sh + s1).sum() / L
    mi = sh + s1 / n
    m2 = ((s2 - s1 * s1 / n) + n * (mi - mean) * (mi - mean)).sum()
    var = max(m2 / L, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def finalize_ref(part, rows, nt, L, cols, lengths=None, len_div=1, eps=1e-5):
    """stats [rows, 2] (mean, rstd) in float64 from a `make_part` buffer: the kernel's formula on the kernel's inputs.  eps is
    taken through float32, as the C entry takes it."""
    p = np.asarray(part.detach().cpu().numpy() if torch.is_tensor(part) else part)
    assert p.dtype == np.float32 and p.size >= rows * nt * 3
    sums = p[:rows * nt * 2].reshape(rows, nt, 2).astype(np.float64)
    shifts = p[rows * nt * 2:rows * nt * 3].reshape(rows, nt).astype(np.float64)
    eps = np.float64(np.float32(eps))
    out = np.empty((rows, 2), dtype=np.float64)
    for r, Lr in enumerate(row_lengths(rows, L, lengths, len_div)):
        ns = min(nt, -(-Lr // cols))
        out[r] = chan_combine(slot_counts(Lr, cols, ns), sums[r, :ns, 0], sums[r, :ns, 1], shifts[r, :ns], Lr, eps)
    return out


def ulp32(v):
    """One float32 unit in the last place at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def assert_finalize(st, ref, ymax, what):
    """Primary bar.  Kernel and `finalize_ref` evaluate one formula in float64 on identical float32 inputs and differ in the order
    of two float64 sums, so the float32 results differ by the final rounding at most: rstd within one float32 ulp of the
    reference; the mean within one ulp, or within 1e-12 x the row's largest |value| where it cancels to next to nothing (float64
    round-off of the weighted sum, 2^-53 x a few hundred terms, with room)."""
    st = np.asarray(st.detach().cpu().numpy() if torch.is_tensor(st) else st, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 2)
    ymax = np.broadcast_to(np.asarray(ymax, dtype=np.float64), (ref.shape[0],))
    assert st.shape == ref.shape, (st.shape, ref.shape)
    assert np.isfinite(st).all(), "%s: statistics not finite: %r" % (what, st)
    dm, dr = np.abs(st[:, 0] - ref[:, 0]), np.abs(st[:, 1] - ref[:, 1])
    bm, br = np.maximum(ulp32(ref[:, 0]), 1e-12 * ymax), ulp32(ref[:, 1])
    for r in range(ref.shape[0]):
        assert dm[r] <= bm[r], "%s: row %d mean %.9g vs %.17g (|d| %.3g > %.3g)" % (what, r, st[r, 0], ref[r, 0], dm[r], bm[r])
        assert dr[r] <= br[r], "%s: row %d rstd %.9g vs %.17g (|d| %.3g > %.3g)" % (what, r, st[r, 1], ref[r, 1], dr[r], br[r])


def assert_stats(st, y, what, eps=1e-5):
    """Secondary bar: statistics [C, 2] against the float64 reduction of the tensor y [C, n] itself, at the bars of `check_stats`
    in tests/test_ragged_kernels_gpu.py (2e-6 x max(1, max |mean|) on the mean, 5e-6 relative on rstd)."""
    y = (y if torch.is_tensor(y) else torch.as_tensor(y)).detach().cpu().double()
    mean, var = y.mean(-1), y.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    st = (st if torch.is_tensor(st) else torch.as_tensor(st)).detach().cpu().double()
    dm = (st[:, 0] - mean).abs().max().item()
    dr = ((st[:, 1] - rstd).abs() / rstd).max().item()
    assert dm < 2e-6 * max(1.0, mean.abs().max().item()), "%s: |d mean| %g" % (what, dm)
    assert dr < 5e-6, "%s: |d rstd| / rstd %g" % (what, dr)
