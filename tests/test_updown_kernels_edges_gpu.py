"""Edge shapes for the kernels that move the vocoder between sample rates -- convt_interleave (six builds), phase_split,
conv1d_direct -- and for stats_finalize called on its own, against the references of tests/_updown_ref.py (proved on the CPU by
tests/test_updown_ref_cpu.py).

Bars.  convt_interleave and phase_split gather and (convt) add twice in the contract's own order: bit equality with the fp32
contract.  conv1d_direct: the plain test's 1e-5 against the fp64 contract; its hard cases by the `hard_bar` rule of
tests/test_kernel_edges_gpu.py, max(1e-5, 4 x the fp32 contract's own error on the same inputs), each printing its (kernel error,
fp32-contract error) pair before it asserts -- the pairs measured on an MI355X stand beside the cases.  stats_finalize: one fp32
ulp from `finalize_ref` (derived in _updown_ref.assert_finalize), then the `check_stats` bars against the tensor itself.

Outputs are views of sentinel-filled buffers where the entry takes one: every float outside the view is checked afterwards."""
import pytest
import torch

import _updown_ref as U
from _util import rel_err
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


def lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def hard_bar(what, e_kernel, e_fp32, plain):
    """max(plain bar, 4 x the fp32 contract's own error on these inputs); prints the measured pair."""
    bar = max(plain, 4.0 * e_fp32)
    print("HARD %s: kernel %.3e  fp32-contract %.3e  bar %.3e" % (what, e_kernel, e_fp32, bar))
    return bar


# ---- views ----------------------------------------------------------------------------------------------------------------------
def make_view(kind, B, C, L, fill):
    """(flat buffer filled with `fill`, a [B, C, L] view of it).  kind:
    "a"          every row on a 16-byte boundary (row pitch a multiple of 4 floats)
    "m1".."m3"   every row 1 / 2 / 3 floats past one
    "r0".."r3"   batch item b starts (k + b) % 4 floats past one: the construction of test_instnorm_stats_len_is_address_independent
    "c"          channels 2 .. 2 + C of a [B, C + 4, pitch] concat buffer (aligned rows)
    "o"          channels 1 .. 1 + C of a [B, C + 3, pitch] buffer whose row pitch is odd"""
    if kind in ("c", "o"):
        lead, wide = (2, C + 4) if kind == "c" else (1, C + 3)
        pitch = (L + 7) // 4 * 4 if kind == "c" else (L + 3) | 1
        big = torch.full((B, wide, pitch), fill, device=DEV)
        return big.view(-1), big[:, lead:lead + C, :L]
    base, step = (int(kind[1]), 0) if kind[0] == "m" else (int(kind[1]), 1) if kind[0] == "r" else (0, 0)
    pitch = (L + 7) // 4 * 4
    bs = C * pitch + step
    flat = torch.full((base + B * bs + pitch,), fill, device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = flat.as_strided((B, C, L), (bs, pitch, 1), base)
    assert [(v[b].data_ptr() // 4) % 4 for b in range(B)] == [(base + b * step) % 4 for b in range(B)]
    return flat, v


def assert_untouched(flat, view, fill, what):
    """Every float of `flat` outside `view` still holds `fill`."""
    inside = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    assert int(inside.sum()) == view.numel()
    outside = flat[~inside]
    assert bool((outside == fill).all()), "%s: %d floats outside the view were written" % (what, int((outside != fill).sum()))


def aligned(kind):
    return kind in ("a", "c")


# ---- convt_interleave -----------------------------------------------------------------------------------------------------------
# (stride, pad, L_out, reflect_left, Lq, out view, add view, bias, want_stats)
#   pad   "0": 0   "h": stride // 2   "m": stride - 1   "x": 2 * stride + 1 (columns below pad // stride are never addressed)
#   Lq    "=": exactly the columns the last output needs   "-": one fewer (the last outputs fall in the zero padding)
#         "+": three more.  Every phase ELEMENT no output addresses holds NaN in all three.
#   views see make_view; None = no add.  B = 4, C = 3: the "r" views need four batch items.
# Tiles of 1024 outputs, four per thread: L_out 1..5 (a row shorter than, equal to and one past one quad), 1021..1027 and
# 2047..2049 (a row end in the last quad of a tile, on the tile edge, 1..3 outputs into the next tile).
CONVT_CASES = [
    (2, "0", 1, 0, "=", "a", None, True, True),
    (64, "x", 1, 0, "+", "m1", "m1", False, True),
    (3, "h", 2, 0, "=", "m2", "a", True, False),
    (7, "m", 2, 0, "-", "a", "m3", True, True),
    (5, "x", 3, 0, "+", "m3", "m2", True, False),
    (1, "0", 3, 0, "-", "r0", "r0", True, True),
    (6, "m", 4, 0, "=", "a", "a", True, True),
    (10, "h", 4, 0, "+", "m1", None, False, False),
    (4, "x", 5, 0, "-", "r1", "r3", True, False),
    (2, "m", 5, 0, "=", "c", "a", True, True),
    (2, "h", 1021, 0, "=", "a", "a", True, False),
    (3, "m", 1022, 0, "-", "m1", "a", True, True),
    (5, "0", 1023, 0, "+", "a", "m2", False, False),
    (6, "h", 1024, 0, "=", "r0", "r0", True, True),
    (10, "x", 1025, 0, "-", "a", "a", True, True),
    (1, "0", 1026, 0, "+", "m3", "m3", True, True),
    (4, "h", 1027, 0, "=", "r2", "a", True, True),
    (7, "x", 2047, 0, "-", "a", "r1", False, False),
    (64, "m", 2048, 0, "=", "c", "c", True, True),
    (64, "h", 2049, 0, "-", "r3", "r2", True, True),
    (6, "x", 1023, 0, "+", "m2", None, True, True),
    (10, "0", 2049, 0, "=", "a", "m1", True, False),
    (6, "h", 3, 1, "=", "a", "a", True, True),
    (2, "x", 4, 1, "-", "m1", "m3", True, False),
    (7, "0", 5, 1, "+", "r0", None, False, True),
    (3, "x", 1021, 1, "=", "m3", "a", True, True),
    (10, "m", 1022, 1, "+", "a", "a", True, False),
    (5, "h", 1023, 1, "-", "r1", "r1", True, True),
    (6, "h", 1024, 1, "=", "a", "m2", True, False),
    (2, "0", 1025, 1, "-", "c", "a", False, True),
    (64, "0", 1026, 1, "=", "m2", "m2", True, False),
    (1, "x", 1027, 1, "-", "a", "r0", True, True),
    (4, "m", 2047, 1, "+", "r3", "a", True, False),
    (5, "m", 2048, 1, "=", "a", None, True, True),
    (6, "x", 2049, 1, "+", "m1", "m1", True, True),
    (10, "h", 2049, 1, "-", "r2", "r0", True, False),
    (3, "0", 1025, 1, "+", "a", "c", True, True),
    (7, "h", 1024, 1, "=", "m3", "m1", True, True),
]
CVT_B, CVT_C = 4, 3


def _pad(s, kind):
    return {"0": 0, "h": s // 2, "m": s - 1, "x": 2 * s + 1}[kind]


def test_convt_case_list_covers_what_it_claims():
    """The list above is curated by hand; this keeps an edit from quietly dropping an edge."""
    edges = [1, 2, 3, 4, 5, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049]
    assert {c[0] for c in CONVT_CASES} == {2, 3, 5, 6, 10, 1, 4, 7, 64}
    assert {c[2] for c in CONVT_CASES if not c[3]} == set(edges)
    assert {c[2] for c in CONVT_CASES if c[3]} == set(edges) - {1, 2}  # reflect needs L_raw = L_out - 1 >= 2
    for s in (2, 3, 5, 6, 10):  # every compile-time build with and without the reflected sample
        assert {c[3] for c in CONVT_CASES if c[0] == s} == {0, 1}
    assert {c[1] for c in CONVT_CASES} == {"0", "h", "m", "x"} and {c[4] for c in CONVT_CASES} == {"=", "-", "+"}
    assert any(c[1] == "x" and c[4] == "+" for c in CONVT_CASES)  # NaN columns below pad // stride
    combos = {(aligned(c[5]), aligned(c[6])) for c in CONVT_CASES if c[6] is not None}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    starts = set()
    for c in CONVT_CASES:
        starts |= {int(c[5][1])} if c[5][0] == "m" else set(range(4)) if c[5][0] == "r" else {0}
    assert starts == {0, 1, 2, 3}
    assert any(c[6] is None for c in CONVT_CASES) and any(not c[7] for c in CONVT_CASES)
    assert any(c[5] == "c" for c in CONVT_CASES)
    with_stats = [c for c in CONVT_CASES if c[8]]
    assert 2 * len(with_stats) >= len(CONVT_CASES)
    assert {1, 1025, 1026, 1027, 2049} <= {c[2] for c in with_stats}  # variance 0; a last slot of 1, 2, 3 columns
    for s, pk, L_out, refl, lq, *_ in CONVT_CASES:
        if lq == "-":
            assert U.convt_cols(s, _pad(s, pk), L_out - refl) >= 2


def _convt_inputs(s, pk, L_out, refl, lq, has_add, has_bias):
    pad, L_raw = _pad(s, pk), L_out - refl
    Lq = U.convt_cols(s, pad, L_raw) + {"=": 0, "-": -1, "+": 3}[lq]
    gen = torch.Generator().manual_seed(1000 * s + 7 * L_out + 3 * pad + refl)
    ph = torch.randn(CVT_B, s * CVT_C, Lq, generator=gen)
    bias = torch.randn(CVT_C, generator=gen) if has_bias else None
    add = torch.randn(CVT_B, CVT_C, L_out, generator=gen) if has_add else None
    return pad, L_raw, ph, bias, add


@pytest.mark.parametrize("case", CONVT_CASES, ids=["s%d_p%s_L%d_r%d_q%s_%s_%s_b%d_st%d" % (c[:6] + (c[6] or "none",) + c[7:])
                                                   for c in CONVT_CASES])
def test_convt_interleave_is_bitwise_the_contract(case, monkeypatch):
    s, pk, L_out, refl, lq, ov, av, has_bias, stats = case
    pad, L_raw, ph, bias, add = _convt_inputs(s, pk, L_out, refl, lq, av is not None, has_bias)
    ref = U.convt_ref(ph, CVT_C, s, pad, L_raw, bias=bias, add=add, reflect_left=bool(refl))
    assert ref.dtype == torch.float32 and bool(torch.isfinite(ref).all())
    phd = g(U.convt_poison(ph, CVT_C, s, pad, L_raw))
    addv = None
    if av is not None:
        _, addv = make_view(av, CVT_B, CVT_C, L_out, NAN)
        addv.copy_(g(add))

    def run(want_stats):
        flat, out = make_view(ov, CVT_B, CVT_C, L_out, SENT)
        r = ops.convt_interleave(phd, CVT_C, s, pad, L_raw, bias=g(bias), add=addv, reflect_left=bool(refl), out=out,
                                 want_stats=want_stats)
        torch.cuda.synchronize()
        assert_untouched(flat, out, SENT, "out")
        return r

    out = run(False)
    U.assert_bitwise(out, ref, "convt_interleave")
    if stats:
        # the partial sums start as NaN: a slot the launch did not write would show
        monkeypatch.setattr(ops, "new_part", lambda B, C, nt, device: torch.full((B * C * nt * 3,), NAN, device=device))
        out2, st = run(True)
        U.assert_bitwise(out2, out, "the output with statistics")
        assert st.shape == (CVT_B, CVT_C, 2)
        for b in range(CVT_B):
            U.assert_stats(st[b], out[b], "item %d" % b)
        if L_out == 1:  # one column: the mean is the value, the variance exactly 0
            assert torch.equal(st[..., 0], out[..., 0])
            assert bool((st[..., 1] == st[0, 0, 1]).all()) and abs(st[0, 0, 1].item() - 1e-5 ** -0.5) < 1e-4
    assert ops.status() == 0


def test_convt_interleave_refuses_what_it_cannot_index():
    """stride 65 (the staged window is sized for <= 64), a negative pad ((l + pad) / stride would truncate toward zero and index the
    window from the wrong column), reflect_left with fewer than two raw outputs, no raw output at all: St2Error, nothing launched."""
    C = 3
    out = torch.full((2, C, 16), SENT, device=DEV)

    def call(s, pad, L_raw, refl):
        ph = torch.randn(2, s * C, 8, device=DEV)
        return ops.convt_interleave(ph, C, s, pad, L_raw, reflect_left=refl, out=out[:, :, :L_raw + (1 if refl else 0)])

    for s, pad, L_raw, refl in [(65, 0, 8, False), (6, -1, 8, False), (6, -6, 8, True), (7, -1, 8, False), (64, -3, 8, False),
                                (1, -1, 4, False), (6, 3, 1, True), (7, 3, 1, True), (6, 3, 0, False)]:
        with pytest.raises(St2Error):
            call(s, pad, L_raw, refl)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    call(64, 0, 8, False)  # the largest stride admitted
    torch.cuda.synchronize()
    assert ops.status() == 0


# ---- phase_split ----------------------------------------------------------------------------------------------------------------
# (stride, Lu, L_in, pad, sliced).  One thread per shifted position, 256 to a block: Lu * stride at 255 / 256 / 257 / 513 where the
# stride divides them, else the nearest multiples either side of the block edge.
#   pad  "0": 0   "h": (stride + 1) // 2 (the noise convs)   "b": L_in + 3, the whole first window in the padding
#   sliced: x = channels 1 .. 1 + C of a wider NaN-filled buffer whose row pitch is odd
PS_CASES = [
    (1, 255, 255, "0", False),
    (1, 256, 250, "h", True),    # zero tail: Lu reaches past the input
    (1, 257, 300, "0", False),   # truncation: the input reaches past Lu
    (1, 513, 513, "h", True),
    (2, 128, 256, "h", False),
    (2, 129, 1, "0", True),      # L_in = 1
    (2, 128, 7, "b", False),
    (2, 257, 600, "0", True),
    (5, 51, 255, "h", True),
    (5, 52, 1, "b", False),
    (5, 103, 400, "0", False),
    (6, 42, 300, "0", False),
    (6, 43, 240, "h", True),
    (7, 36, 5, "b", True),
    (7, 37, 259, "h", False),
    (30, 8, 1, "0", False),
    (30, 9, 270, "h", True),
    (30, 18, 100, "b", False),
]


def test_phase_split_case_list_covers_what_it_claims():
    assert {c[0] for c in PS_CASES} == {1, 2, 5, 6, 7, 30}
    assert {255, 256, 257, 513} <= {c[0] * c[1] for c in PS_CASES}
    for s in (2, 5, 6, 7, 30):  # either side of (or on) the 256-thread block edge
        n = {c[0] * c[1] for c in PS_CASES if c[0] == s}
        assert min(n) <= 256 < max(n)
    assert {c[3] for c in PS_CASES} == {"0", "h", "b"} and any(c[2] == 1 for c in PS_CASES) and any(c[4] for c in PS_CASES)


@pytest.mark.parametrize("s,Lu,L_in,pk,sliced", PS_CASES)
def test_phase_split_is_bitwise_the_contract(s, Lu, L_in, pk, sliced):
    B, C = 2, 3
    pad = {"0": 0, "h": (s + 1) // 2, "b": L_in + 3}[pk]
    gen = torch.Generator().manual_seed(100 * s + Lu)
    x = torch.randn(B, C, L_in, generator=gen)
    ref = R.phase_split(x, s, pad, Lu)
    if pk != "b" or Lu * s > pad:
        assert bool((ref != 0).any())
    if sliced:
        _, xv = make_view("o", B, C, L_in, NAN)
        xv.copy_(g(x))
    else:
        xv = g(x)
    out = ops.phase_split(xv, s, pad, Lu)
    torch.cuda.synchronize()
    U.assert_bitwise(out, ref, "phase_split")
    assert ops.status() == 0


# ---- conv1d_direct --------------------------------------------------------------------------------------------------------------
# name: (C_in, C_out, ks, stride, pad, L_in, L_out (None: the natural one), bias, views).  One thread per output, 256 to a block.
# views: x = channels of a NaN-filled buffer with an odd row pitch, out = a view ("r0": rows at every offset) of a sentinel buffer.
CD_CASES = {
    "L_out255": (3, 4, 3, 1, 1, 255, None, True, False),
    "L_out256_stride2": (4, 3, 4, 2, 1, 513, None, True, True),
    "L_out257_ks1_pad0": (3, 5, 1, 1, 0, 257, None, True, False),
    "L_out513_Cin1": (1, 3, 5, 3, 2, 1537, None, True, True),
    "ks_past_input_and_pad": (3, 4, 6, 1, 2, 3, None, True, False),   # ks = 6 > L_in + pad = 5: every window holds both paddings
    "stride_past_ks_pad0": (5, 3, 2, 5, 0, 101, None, True, True),
    "pad_past_ks": (4, 3, 3, 1, 5, 40, None, True, True),             # outputs 0..2 and 45..47 see padding only
    "pad_past_ks_no_bias": (4, 3, 3, 2, 7, 40, None, False, False),   # outputs 0..2 and 24..25 see padding only
    "no_bias": (6, 4, 3, 2, 1, 77, None, False, True),
    "short_L_out": (3, 4, 5, 2, 2, 300, 100, True, True),             # the natural L_out is 150
    "short_L_out_256": (2, 3, 3, 1, 1, 400, 256, False, True),
}


def _cd_run(x, w, bias, stride, pad, L_out, views):
    B, C_in, L_in = x.shape
    C_out = w.shape[0]
    n = L_out if L_out is not None else (L_in + 2 * pad - w.shape[2]) // stride + 1
    if not views:
        out = ops.conv1d_direct(g(x), g(w), g(bias), stride, pad, L_out=L_out)
        torch.cuda.synchronize()
        return out
    _, xv = make_view("o", B, C_in, L_in, NAN)
    xv.copy_(g(x))
    flat, out = make_view("r0", B, C_out, n, SENT)
    ops.conv1d_direct(xv, g(w), g(bias), stride, pad, L_out=L_out, out=out)
    torch.cuda.synchronize()
    assert_untouched(flat, out, SENT, "out")
    return out


@pytest.mark.parametrize("name", list(CD_CASES))
def test_conv1d_direct_edges_match_fp64(name):
    C_in, C_out, ks, stride, pad, L_in, L_out, has_bias, views = CD_CASES[name]
    B = 4 if views else 2
    gen = torch.Generator().manual_seed(len(name) + L_in)
    x = torch.randn(B, C_in, L_in, generator=gen)
    w = torch.randn(C_out, C_in, ks, generator=gen) * 0.2
    bias = torch.randn(C_out, generator=gen) if has_bias else None
    ref = R.conv1d_direct(x.double(), w.double(), None if bias is None else bias.double(), stride, pad, L_out=L_out)
    out = _cd_run(x, w, bias, stride, pad, L_out, views)
    assert out.shape == ref.shape
    e = rel_err(out, ref)
    print("conv1d_direct %s: L_out %d, %.3e" % (name, ref.shape[2], e))
    assert e < 1e-5
    # an output whose window lies wholly in the padding is the bias and nothing else, exactly
    base = torch.arange(ref.shape[2]) * stride - pad
    void = (base + ks - 1 < 0) | (base >= L_in)
    if name.startswith("pad_past_ks"):
        assert int(void.sum()) >= 5 and bool(void[0]) and bool(void[-1])
    want = torch.zeros(C_out) if bias is None else bias
    assert torch.equal(out.cpu()[:, :, void], want.view(1, C_out, 1).expand(B, C_out, int(void.sum())))
    assert ops.status() == 0


# Hard inputs: measured (kernel error, fp32-contract error) on an MI355X beside each.
CD_HARD = {
    # C_in * ks = 4096 products per output, summed in one fp32 chain
    "reduction4096": (512, 3, 8, 4, 4, 64, 0.0),       # kernel 9.440e-07, fp32 contract 2.101e-07
    # an offset 100 x the signal: every product is dominated by the part that cancels in the sum
    "offset_dominated": (22, 4, 12, 6, 3, 200, 100.0),  # kernel 6.695e-07, fp32 contract 8.355e-07
}


@pytest.mark.parametrize("name", list(CD_HARD))
def test_conv1d_direct_hard_inputs(name):
    C_in, C_out, ks, stride, pad, L_in, offset = CD_HARD[name]
    assert name != "reduction4096" or C_in * ks >= 4096
    gen = torch.Generator().manual_seed(C_in)
    x = torch.randn(2, C_in, L_in, generator=gen) + offset
    w = torch.randn(C_out, C_in, ks, generator=gen) * 0.2
    bias = torch.randn(C_out, generator=gen)
    ref = R.conv1d_direct(x.double(), w.double(), bias.double(), stride, pad)
    e32 = rel_err(R.conv1d_direct(x, w, bias, stride, pad), ref)
    out = ops.conv1d_direct(g(x), g(w), g(bias), stride, pad)
    torch.cuda.synchronize()
    e = rel_err(out, ref)
    assert e < hard_bar("conv1d_direct " + name, e, e32, 1e-5)
    assert ops.status() == 0


# ---- stats_finalize on make_part buffers ------------------------------------------------------------------------------------------
# One wave per row, four rows per workgroup, lanes stride the slots by 64.  Slots in use = ceil(L / cols); `extra` slots beyond them
# hold NaN (part_nt larger than the slots in use).  rows: "const" makes row 0 constant, "offset" gives the last row a mean of 1000 x
# its standard deviation.  lengths: raw values (0 and L + 9 clamp to 1 and L), one per B * C / len_div rows.
SF_CASES = {
    "c32_1slot_1col": dict(cols=32, L=1, extra=0, B=1, C=1),
    "c32_63slots": dict(cols=32, L=62 * 32 + 5, extra=2, B=1, C=5, rows=("const", "offset")),
    "c32_64slots": dict(cols=32, L=64 * 32, extra=0, B=7, C=1),
    "c32_65slots_last1": dict(cols=32, L=64 * 32 + 1, extra=3, B=2, C=4, rows=("offset",)),
    "c32_129slots": dict(cols=32, L=128 * 32 + 17, extra=0, B=1, C=5),
    "c32_200slots_last1": dict(cols=32, L=199 * 32 + 1, extra=1, B=2, C=4, rows=("const", "offset")),
    "c64_63slots_const": dict(cols=64, L=63 * 64, extra=2, B=1, C=1, rows=("const",)),
    "c64_65slots_last1": dict(cols=64, L=64 * 64 + 1, extra=0, B=1, C=7),
    "c128_1slot": dict(cols=128, L=100, extra=0, B=1, C=5),
    "c128_129slots": dict(cols=128, L=129 * 128, extra=0, B=2, C=4, rows=("const", "offset")),
    "c1024_2slots_last1": dict(cols=1024, L=1025, extra=2, B=1, C=7),
    "c1024_1col_offset": dict(cols=1024, L=1, extra=1, B=1, C=1, rows=("offset",)),
    "c1024_65slots_offset": dict(cols=1024, L=64 * 1024 + 5, extra=0, B=1, C=1, rows=("offset",)),
    # lengths shared by the C rows of an item: 0, L + 9, mid-slot, on a slot edge
    "c32_len_div_C": dict(cols=32, L=65 * 32, extra=1, B=4, C=2, lengths=[0, 65 * 32 + 9, 40 * 32 + 7, 64 * 32], len_div=2,
                          rows=("offset",)),
    # one length per row: a slot edge, one past it, one before it
    "c128_len_div_1": dict(cols=128, L=3 * 128 + 5, extra=2, B=7, C=1, lengths=[0, 3 * 128 + 14, 128, 129, 127, 256, 300], len_div=1),
    "c1024_len_div_1": dict(cols=1024, L=2 * 1024 + 3, extra=0, B=5, C=1, lengths=[1024, 1025, 1, 2 * 1024 + 12, 2000], len_div=1,
                            rows=("const",)),
    "c64_len_129slots": dict(cols=64, L=129 * 64, extra=0, B=2, C=4, lengths=[65 * 64 + 1, 129 * 64], len_div=4, rows=("const", "offset")),
}


def test_stats_finalize_case_list_covers_what_it_claims():
    c = SF_CASES.values()
    assert {k["cols"] for k in c} == {32, 64, 128, 1024}
    assert {1, 63, 64, 65, 129, 200} <= {-(-k["L"] // k["cols"]) for k in c}
    assert {k["B"] * k["C"] for k in c} == {1, 5, 7, 8}
    assert any(k["extra"] for k in c) and any(k["L"] % k["cols"] == 1 for k in c)
    assert {k["len_div"] == 1 for k in c if "lengths" in k} == {True, False}


@pytest.mark.parametrize("name", list(SF_CASES))
def test_stats_finalize_on_its_own(name):
    k = SF_CASES[name]
    cols, L, B, C = k["cols"], k["L"], k["B"], k["C"]
    rows, kinds = B * C, k.get("rows", ())
    nt = -(-L // cols) + k["extra"]
    gen = torch.Generator().manual_seed(cols + L)
    y = torch.randn(rows, L, generator=gen) * 0.5 + torch.randn(rows, 1, generator=gen) * 3.0
    if "const" in kinds:
        y[0] = 3.25
    if "offset" in kinds:
        y[-1] = 500.0 + 0.5 * torch.randn(L, generator=gen)
    raw, len_div = k.get("lengths"), k.get("len_div", 1)
    n = U.row_lengths(rows, L, raw, len_div)
    part = U.make_part(y, cols, nt, lengths=None if raw is None else n)
    assert bool(torch.isnan(part).any()) == any(-(-v // cols) < nt for v in n)  # NaN in every slot without columns
    ref = U.finalize_ref(part, rows, nt, L, cols, lengths=raw, len_div=len_div)
    st = ops.stats_finalize(g(part), B, C, nt, L, cols=cols, lengths=None if raw is None else lens(raw), len_div=len_div)
    torch.cuda.synchronize()
    assert st.shape == (B, C, 2)
    st = st.cpu().reshape(rows, 2)
    ymax = [y[r, :n[r]].abs().max().item() for r in range(rows)]
    U.assert_finalize(st, ref, ymax, name)
    for r in range(rows):  # and against the tensor itself
        U.assert_stats(st[r:r + 1], y[r:r + 1, :n[r]], "%s row %d (%d columns)" % (name, r, n[r]))
    if "const" in kinds:
        assert st[0, 0].item() == 3.25
    assert ops.status() == 0
