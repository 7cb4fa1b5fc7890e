"""Edge shapes and hard inputs for the small kernels of the front's token path (st2_glue.hip, st2_norm.hip, st2_misc.hip):
duration_head, expand_by_durations, colnorm_apply, embed_tokens, tokens_to_channels, mask_tail, broadcast_cols, copy_ncl,
add_chanvec, axpbypcz and time_features.

References are the contracts of oracle/ops_ref.py evaluated on float64 copies of the inputs, or numpy where a kernel is a
pure move; moves are compared bit for bit.  Shapes sit on, one before and one past every edge named in the kernel (beside each
list).  Operands are the strided views the C++ plans hand these kernels; outputs go into a slice of a sentinel-filled buffer
and the sentinels are checked afterwards.

Bars are those the plain tests of tests/test_ops_gpu.py assert.  Hard inputs use the rule of tests/test_kernel_edges_gpu.py:
max(plain bar, 4 x the error of the fp32 evaluation of the same contract against float64 on the same inputs), printed as a
(kernel error, fp32-contract error) pair before the assertion; the pairs measured on an MI355X are written beside the cases."""
import math

import numpy as np
import pytest
import torch

from _util import rel_err
from oracle import ops_ref as R
from styletts2_amd import _lib, ops
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


def d(t):
    return None if t is None else t.double()


def hard_bar(what, e_kernel, e_fp32, plain):
    """max(plain bar, 4 x the fp32 contract's own error on these inputs); prints the measured pair."""
    bar = max(plain, 4.0 * e_fp32)
    print("HARD %s: kernel %.3e  fp32-contract %.3e  bar %.3e" % (what, e_kernel, e_fp32, bar))
    return bar


def bits_equal(a, b):
    """Same shape and the same 32-bit patterns (a move: -0.0 and NaN payloads included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def strided_src(t, front=1, back=2, cols=2, fill=NAN):
    """`t` [B, C, L] on the device as a channel slice of a wider buffer with a longer row pitch; everything around it is `fill`."""
    B, C, L = t.shape
    wide = torch.full((B, C + front + back, L + cols), fill, device=DEV)
    view = wide[:, front:front + C, :L]
    view.copy_(t)
    return view


def framed_out(B, C, L, front=2, back=2, cols=3):
    big = torch.full((B, C + front + back, L + cols), SENT, device=DEV)
    return big, big[:, front:front + C, :L]


def frame_untouched(big, view_shape, front=2):
    _, C, L = view_shape
    chk = big.clone()
    chk[:, front:front + C, :L] = SENT
    return bool((chk == SENT).all())


def lens_dev(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- duration_head ----------------------------------------------------------------------------------------------------------
# duration_head_kernel: one wave per token, lanes stride 64 over K (K = 1: one live lane; 63 / 64 / 65: the wave's edge; 512 the
# model's; 640 = ten sweeps), J sigmoids summed in a loop, N tokens = N workgroups
DUR_CASES = [(K, 50, 83) for K in (1, 63, 64, 65, 512, 640)] + [(1, 1, 1), (65, 1, 83), (64, 50, 1), (640, 1, 1)]


def _dur_inputs(seed, B, K, J, N, w_gain=1.0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, N, generator=gen) * 0.5
    w = torch.randn(J, K, generator=gen) / math.sqrt(K) * w_gain
    bias = torch.randn(J, generator=gen) * 0.1
    return x, w, bias


def _dur_check(what, x, w, bias, lens, tail, hard=False):
    B, K, N = x.shape
    clamped = None if lens is None else torch.tensor([min(max(n, 1), N) for n in lens], dtype=torch.int32)
    rd, rs = R.duration_head(d(x), d(w), d(bias), lengths=clamped, tail=tail, want_sums=True)
    _, s32 = R.duration_head(x, w, bias, lengths=clamped, tail=tail, want_sums=True)
    e32 = (s32.double() - rs).abs().max().item()
    # a duration is decided where the fp64 sum is further from a rounding tie (k + 1/2) than 4 x the fp32 contract's error
    safe = (rs - rs.floor() - 0.5).abs() > 4.0 * e32
    assert int((~safe).sum()) <= 0.01 * B * N, "more than 1 %% of the tokens sit on a rounding tie (%d)" % int((~safe).sum())
    xv = strided_src(g(x), front=2, back=3, cols=0)  # the BiLSTM's output arrives as a channel slice
    dur, sums = ops.duration_head(xv, g(w), g(bias), lengths=lens_dev(lens), tail=tail, want_sums=True)
    assert dur.dtype == torch.int64 and bool(torch.isfinite(sums).all())
    e = (sums.cpu().double() - rs).abs().max().item()
    if hard:
        assert e <= hard_bar(what, e, e32, 2e-5)
    else:
        print("%s: sums %.3e (fp32 contract %.3e)" % (what, e, e32))
        assert e < 2e-5
    assert torch.equal(dur.cpu()[safe], rd[safe])
    assert ops.status() == 0
    return dur.cpu()


@pytest.mark.parametrize("K,J,N", DUR_CASES)
def test_duration_head_edges(K, J, N):
    """Lengths 0 (the kernel clamps to 1: token 0 carries the duration and the tail) and N + 4 (clamped to N) beside a full and
    a one-short row; tail 0 and 5; without lengths."""
    B = 4
    x, w, bias = _dur_inputs(500 + K + J + N, B, K, J, N)
    lens = [N, 0, N + 4, max(N - 1, 1)]
    for lengths, tail in ((None, 0), (None, 5), (lens, 0), (lens, 5)):
        dur = _dur_check("duration_head K=%d J=%d N=%d tail=%d%s" % (K, J, N, tail, "" if lengths is None else " ragged"),
                         x, w, bias, lengths, tail)
        if lengths is not None:
            assert int(dur[1, 1:].sum()) == 0 and int(dur[1, 0]) >= 1 + tail  # the row of length 0 is a row of length 1
            assert int(dur[2].min()) >= 1                                       # N + 4 is N
            if N > 1:
                assert int(dur[3, N - 1]) == 0 and int(dur[3, N - 2]) >= 1 + tail


# measured on an MI355X (kernel error, fp32-contract error) of the un-rounded sums: 7.1e-6, 1.4e-5 -> bar 5.7e-5 (|logit| <= 389);
# the benign K = 512 / J = 50 case beside it: 7.4e-6, 4.0e-6 under its plain 2e-5
def test_duration_head_saturated_logits():
    """Logits of +- 100 and beyond: exp(-a) overflows for the negative ones and the sigmoid is 0 or 1 to the last bit, the few
    unsaturated logits carry the dot product's round-off at |a| ~ 100 into the sum."""
    B, K, J, N = 4, 512, 50, 83
    x, w, bias = _dur_inputs(555, B, K, J, N, w_gain=200.0)
    logits = torch.einsum("bkn,jk->bjn", d(x), d(w)) + d(bias).view(1, J, 1)
    assert logits.max().item() > 100 and logits.min().item() < -100 and (logits.abs() > 20).double().mean().item() > 0.5
    _dur_check("duration_head saturated (|logit| <= %.0f)" % logits.abs().max().item(), x, w, bias, [N, 0, N + 4, N - 1], 5,
               hard=True)


# ---- expand_by_durations ----------------------------------------------------------------------------------------------------
# expand_by_durations_kernel: the prefix sum runs in chunks of 64 tokens (N <= 512), a workgroup covers 256 frames x 64 channels
#   (N, T, C): every N, T and C edge at least once
EXPAND_CASES = [(1, 1, 1), (1, 700, 65), (63, 255, 63), (64, 256, 64), (65, 257, 65), (128, 700, 130), (129, 257, 1),
                (511, 700, 64), (512, 255, 130), (512, 700, 63)]


def _durations(seed, N, T):
    """B = 4 rows summing to T: row 0 starts with a zero and (N > 70) has a run of zeros across the first chunk boundary, in
    row 1 the middle token owns every frame, row 2 is random with many zeros, in row 3 the last token owns all but its
    neighbours' single frames."""
    gen = torch.Generator().manual_seed(seed)

    def scatter(allowed):
        allowed = torch.tensor(allowed)
        idx = allowed[torch.randint(len(allowed), (T,), generator=gen)]
        return torch.bincount(idx, minlength=N)
    r0 = [n for n in range(N) if n != 0 and not 58 <= n < 70] or [0]
    r2 = [n for n in range(N) if n % 3 == 1] or [0]
    dur = torch.zeros(4, N, dtype=torch.int64)
    dur[0] = scatter(r0)
    dur[1, N // 2] = T
    dur[2] = scatter(r2)
    k = min(N - 1, T - 1, 3)
    dur[3, N - 1 - k:N - 1] = 1
    dur[3, N - 1] = T - k
    assert bool((dur.sum(dim=1) == T).all()) and bool((dur >= 0).all())
    return dur


def _expand_ref(x, dur, T, shift):
    y = np.stack([np.repeat(x[b].numpy(), dur[b].numpy(), axis=1) for b in range(x.shape[0])])
    if shift:
        y = np.concatenate([y[:, :, :1], y[:, :, :-1]], axis=2)
    assert y.shape[2] == T
    return torch.from_numpy(y)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("N,T,C", EXPAND_CASES)
def test_expand_by_durations_edges(N, T, C, shift):
    gen = torch.Generator().manual_seed(600 + N + T + C)
    x = torch.randn(4, C, N, generator=gen)
    dur = _durations(601 + N + T + C, N, T)
    if N > 1:
        assert int(dur[0, 0]) == 0
    if N > 70:
        assert int(dur[0, 58:70].sum()) == 0
    big, view = framed_out(4, C, T)
    out = ops.expand_by_durations(strided_src(g(x)), g(dur), T, shift=shift, out=view)
    torch.cuda.synchronize()
    assert bits_equal(out, _expand_ref(x, dur, T, shift))
    assert frame_untouched(big, view.shape)
    assert ops.status() == 0, "rows that sum to T raise nothing"


@pytest.mark.parametrize("N,T,C", [(65, 257, 65), (512, 700, 63), (1, 1, 1)])
@pytest.mark.parametrize("row,delta", [(0, 1), (3, -1), (2, 5)])
def test_expand_by_durations_reports_a_wrong_row_sum(N, T, C, row, delta):
    """STATUS_DURATION_SUM is raised exactly when a row's durations do not sum to T (one row of four, one frame too many or too
    few), reported by check_status and cleared by it; the other rows are what they were."""
    gen = torch.Generator().manual_seed(650 + N)
    x = torch.randn(4, C, N, generator=gen)
    dur = _durations(651 + N, N, T)
    good = ops.expand_by_durations(g(x), g(dur), T)
    torch.cuda.synchronize()
    assert ops.status() == 0
    bad = dur.clone()
    col = int(bad[row].argmax())
    if bad[row, col] + delta < 0:
        delta = 1
    bad[row, col] += delta
    out = ops.expand_by_durations(g(x), g(bad), T)
    torch.cuda.synchronize()
    assert ops.status() == _lib.STATUS_DURATION_SUM
    with pytest.raises(St2Error, match="durations does not sum"):
        ops.check_status()
    assert ops.status() == 0  # cleared by the check
    keep = [b for b in range(4) if b != row]
    assert bits_equal(out[keep], good[keep])


def test_expand_by_durations_refuses_more_than_512_tokens():
    x = torch.zeros(1, 2, 513, device=DEV)
    dur = torch.ones(1, 513, dtype=torch.int64, device=DEV)
    with pytest.raises(St2Error, match="N=513 tokens exceed the 512"):
        ops.expand_by_durations(x, dur, 513)
    assert ops.status() == 0


# ---- colnorm_apply ----------------------------------------------------------------------------------------------------------
# colnorm_apply_kernel: 4 channels per workgroup row (C = 1, 3, 4, 5: a partial, a full and a full + partial row), 256 columns
COLNORM_SHAPES = [(C, 257) for C in (1, 3, 4, 5, 70)] + [(5, L) for L in (1, 255, 256)] + [(70, 1)]
# (gamma / beta per batch row, gamma_plus_one, act)
COLNORM_VARIANTS = [(False, False, R.ACT_NONE), (True, True, R.ACT_NONE), (True, False, R.ACT_LEAKY), (False, True, R.ACT_LEAKY)]


def _colnorm_run(x, st, gamma, beta, plus_one, act, lens):
    """x, stats with NaN in the padded columns go to the kernel; the reference sees the finite copies and the clamped lengths."""
    B, C, L = x.shape
    clamped = torch.tensor([min(max(n, 0), L) for n in lens], dtype=torch.int32)
    pad = torch.arange(L).view(1, 1, L) >= clamped.view(B, 1, 1)
    xn = x.masked_fill(pad, NAN)
    stn = st.masked_fill(pad.view(B, L, 1), NAN)
    ref = R.colnorm_apply(d(x), d(st), d(gamma), d(beta), gamma_plus_one=plus_one, act=act, slope=0.2, lengths=clamped)
    r32 = R.colnorm_apply(x, st, gamma, beta, gamma_plus_one=plus_one, act=act, slope=0.2, lengths=clamped)
    big, view = framed_out(B, C, L)
    out = ops.colnorm_apply(strided_src(g(xn)), g(stn).contiguous(), g(gamma), g(beta), gamma_plus_one=plus_one, act=act,
                            slope=0.2, lengths=lens_dev(lens), out=view)
    torch.cuda.synchronize()
    assert frame_untouched(big, view.shape)
    assert bool(torch.isfinite(out).all())
    assert bool(pad.any()) and float(out.cpu().masked_select(pad.expand(B, C, L)).abs().max()) == 0.0
    assert ops.status() == 0
    return rel_err(out, ref), rel_err(r32, ref)


@pytest.mark.parametrize("C,L", COLNORM_SHAPES)
def test_colnorm_apply_edges(C, L):
    """Lengths L, 0 and L + 3 (the last two clamp to an all-zero and a full row); NaN in the padded columns of x and of the
    statistics gives exact zeros there."""
    gen = torch.Generator().manual_seed(700 + C + L)
    B = 3
    x = torch.randn(B, C, L, generator=gen) * 2 + 0.5
    st = R.colnorm_stats(x, eps=1e-5)
    for per_row, plus_one, act in COLNORM_VARIANTS:
        gamma = torch.randn(B if per_row else 1, C, generator=gen)
        beta = torch.randn(B if per_row else 1, C, generator=gen)
        e, e32 = _colnorm_run(x, st, gamma, beta, plus_one, act, [max(L - 2, 1), 0, L + 3])
        print("colnorm_apply C=%d L=%d rows=%d +1=%d act=%d: %.3e (fp32 contract %.3e)" % (C, L, per_row, plus_one, act, e, e32))
        assert e < 1e-5


# measured on an MI355X (kernel error, fp32-contract error), relative to the largest output: 8.8e-8, 8.8e-8 -> bar 1e-5 (the
# statistics are a shared fp32 input and the kernel's operation order is the contract's, so the two agree to the last bit)
def test_colnorm_apply_offset_dominated_columns():
    """Columns whose mean is 1e3 x their spread: x - mean cancels ten bits and what is left carries the fp32 rounding of x
    itself; the fp32 contract on the same inputs sets the bar."""
    gen = torch.Generator().manual_seed(790)
    B, C, L = 3, 70, 257
    x = torch.randn(B, C, L, generator=gen) + 1e3 * (1.0 + 0.05 * torch.randn(B, 1, L, generator=gen))
    st = R.colnorm_stats(x, eps=1e-5)
    assert float((st[:, :, 0].abs() * st[:, :, 1]).min()) > 500  # |mean| / std
    gamma, beta = torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen)
    e, e32 = _colnorm_run(x, st, gamma, beta, True, R.ACT_LEAKY, [L, 0, L + 3])
    assert e <= hard_bar("colnorm_apply offset-dominated", e, e32, 1e-5)


# ---- embed_tokens -----------------------------------------------------------------------------------------------------------
# embed_tokens_kernel / tokens_to_channels_kernel: 32 tokens x 32 features per tile through LDS
TILE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (65, 65), (1, 65), (65, 1)]  # (N, E)
V = 11


def _embed(tokens, table, add, pos, lens, out):
    B, N = tokens.shape
    Vv, E = table.shape
    p = lambda t: 0 if t is None else t.data_ptr()
    _lib.check(_lib.load().st2_embed_tokens(tokens.data_ptr(), B, N, table.data_ptr(), Vv, E, p(add), p(pos), p(lens),
                                            out.data_ptr(), out.stride(0), out.stride(1), ops._stream()), "st2_embed_tokens")


@pytest.mark.parametrize("N,E", TILE_SHAPES)
def test_embed_tokens_edges(N, E):
    """y[b, e, n] = (table[tok] + add[e]) + pos[n, e] in float32, zeros at n >= len[b]; ids -1 and V read no table row (their
    table term is 0), V - 1 is the last row.  `add` and `pos` each absent and present; lengths N, 0, N - 1 and absent."""
    gen = torch.Generator().manual_seed(800 + N + E)
    B = 4
    tokens = torch.randint(0, V, (B, N), generator=gen)
    tokens[0, 0], tokens[1, N - 1], tokens[2, N // 2], tokens[3, 0] = -1, V, V - 1, V
    table = torch.randn(V, E, generator=gen)
    # a guard row on either side of the table: an id of -1 or V that was read would fetch a NaN
    guarded = torch.full((V + 2, E), NAN)
    guarded[1:V + 1] = table
    tab = g(guarded)[1:V + 1]
    assert tab.is_contiguous()
    add_, pos_ = torch.randn(E, generator=gen), torch.randn(N, E, generator=gen)
    ok = ((tokens >= 0) & (tokens < V)).unsqueeze(-1)
    base = torch.where(ok, table[tokens.clamp(0, V - 1)], torch.zeros(()))  # [B, N, E]
    for add in (None, add_):
        for pos in (None, pos_):
            for lens in (None, [N, 0, N, N - 1]):
                v = base
                if add is not None:
                    v = v + add
                if pos is not None:
                    v = v + pos
                if lens is not None:
                    v = v.masked_fill(torch.arange(N).view(1, N, 1) >= torch.tensor(lens).view(B, 1, 1), 0.0)
                big, view = framed_out(B, E, N, front=3)
                _embed(g(tokens), tab, g(add), g(pos), lens_dev(lens), view)
                torch.cuda.synchronize()
                assert bits_equal(view, v.transpose(1, 2)), (add is not None, pos is not None, lens)
                assert frame_untouched(big, view.shape, front=3)
    assert ops.status() == 0


@pytest.mark.parametrize("N,E", TILE_SHAPES)
def test_tokens_to_channels_edges(N, E):
    """[B, N, E] and the batch-broadcast [N, E] form (e_bs = 0) into a sliced destination: a transpose, bit for bit."""
    gen = torch.Generator().manual_seed(850 + N + E)
    B = 3
    e = torch.randn(B, N, E, generator=gen)
    big, view = framed_out(B, E, N)
    ops.tokens_to_channels(g(e), view)
    assert bits_equal(view, e.transpose(1, 2)) and frame_untouched(big, view.shape)
    big, view = framed_out(B, E, N)
    ops.tokens_to_channels(g(e[1].contiguous()), view, B=B)
    assert bits_equal(view, e[1].t().unsqueeze(0).expand(B, E, N)) and frame_untouched(big, view.shape)
    assert ops.status() == 0


# ---- the 256-column moves ---------------------------------------------------------------------------------------------------
# mask_tail / broadcast_cols / copy_ncl / add_chanvec kernels: one thread per column, 256 columns per workgroup
COLS = [1, 255, 256, 257]


@pytest.mark.parametrize("L", COLS)
def test_mask_tail_edges(L):
    """In place on a strided view: columns >= len[b] become zero (NaN included: a store, not a product), the others and
    everything around the view keep their bits.  Lengths L, 0, L + 1 and L // 2."""
    gen = torch.Generator().manual_seed(900 + L)
    B, C = 4, 3
    x = torch.randn(B, C, L, generator=gen)
    lens = [L, 0, L + 1, L // 2]
    pad = torch.arange(L).view(1, 1, L) >= torch.tensor(lens).view(B, 1, 1)
    big, view = framed_out(B, C, L)
    view.copy_(x.masked_fill(pad, NAN))
    ld = lens_dev(lens)
    _lib.check(_lib.load().st2_mask_tail(view.data_ptr(), view.stride(0), view.stride(1), B, C, L, ld.data_ptr(), ops._stream()),
               "st2_mask_tail")
    torch.cuda.synchronize()
    assert bits_equal(view, x.masked_fill(pad, 0.0))
    assert frame_untouched(big, view.shape)
    assert ops.status() == 0


@pytest.mark.parametrize("L", COLS)
def test_broadcast_cols_and_copy_ncl_edges(L):
    gen = torch.Generator().manual_seed(910 + L)
    B, C = 3, 5
    x = torch.randn(B, C, generator=gen)
    xv = g(torch.cat([torch.full((B, 2), NAN), x, torch.full((B, 1), NAN)], dim=1))[:, 2:2 + C]  # row pitch C + 3
    big, view = framed_out(B, C, L)
    ops.broadcast_cols(xv, view)
    assert bits_equal(view, x.unsqueeze(-1).expand(B, C, L)) and frame_untouched(big, view.shape)
    y = torch.randn(B, C, L, generator=gen)
    big, view = framed_out(B, C, L)
    ops.copy_ncl(strided_src(g(y)), view)
    assert bits_equal(view, y) and frame_untouched(big, view.shape)
    assert ops.status() == 0


@pytest.mark.parametrize("L", COLS)
def test_add_chanvec_and_axpbypcz_edges(L):
    gen = torch.Generator().manual_seed(920 + L)
    B, C = 3, 5
    x, v = torch.randn(B, C, L, generator=gen), torch.randn(B, C, generator=gen)
    vv = g(torch.cat([torch.full((B, 1), NAN), v, torch.full((B, 2), NAN)], dim=1))[:, 1:1 + C]
    big, view = framed_out(B, C, L)
    ops.add_chanvec(strided_src(g(x)), vv, out=view)
    assert rel_err(view, R.add_chanvec(d(x), d(v))) < 1e-6 and frame_untouched(big, view.shape)
    # axpbypcz is flat: L and 3 L elements, each operand absent and present
    for n in (L, 3 * L):
        a, y, z = (torch.randn(n, generator=gen) for _ in range(3))
        for yy, zz in ((None, None), (y, None), (y, z)):
            out = torch.full((n + 4,), SENT, device=DEV)
            ops.axpbypcz(g(a), 0.3, g(yy), -1.2, g(zz), 2.0, out=out[:n])
            assert rel_err(out[:n], R.axpbypcz(d(a), 0.3, d(yy), -1.2, d(zz), 2.0)) < 1e-6
            assert bool((out[n:] == SENT).all())
    assert ops.status() == 0


# ---- time_features ----------------------------------------------------------------------------------------------------------
# time_features_kernel: 256 outputs per workgroup, 1 + 2 H2 outputs per row (3, 129, 257: across the workgroup edge)
@pytest.mark.parametrize("H2", [1, 64, 128])
@pytest.mark.parametrize("t", [1e-4, 1.0, 80.0, 1e3])
def test_time_features_over_the_sigma_range(t, H2):
    """The contract fixes the argument's operation order, ((t * w) * 2) * pi in float32, so the reference is sin / cos in
    float64 OF THAT float32 argument (at t = 1e3 it reaches thousands of radians: the range reduction is what is tested)."""
    gen = torch.Generator().manual_seed(950 + H2)
    B = 3
    w = torch.randn(H2, generator=gen)
    t32 = torch.tensor(t, dtype=torch.float32)
    arg = ((t32 * w) * 2.0) * torch.tensor(math.pi, dtype=torch.float32)
    assert arg.dtype == torch.float32
    ref = torch.cat([t32.double().view(1), arg.double().sin(), arg.double().cos()]).unsqueeze(0).expand(B, -1)
    out = torch.full((B + 1, 1 + 2 * H2), SENT, device=DEV)
    ops.time_features(t, g(w), B, out=out[:B])
    e = (out[:B].cpu().double() - ref).abs().max().item()
    print("time_features t=%g H2=%d (|arg| <= %.0f): %.3e" % (t, H2, arg.abs().max().item(), e))
    assert e < 1e-6
    assert bool((out[:B, 0].cpu() == t32).all()) and bool((out[B] == SENT).all())
    assert ops.status() == 0
