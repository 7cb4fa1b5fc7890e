"""The split-f16 prologue (csrc/st2_act.h: affine, activation, operand scale, f16 clamp, hi/lo split) at its edges and on hard
inputs, on every route that runs it: st2_act_split, the one-role fused conv in its three row layouts (the 32-row one runs the
packed-f32 instantiation), the warp-specialised build -- and the exact-fp32 conv's own prologue and the activations of the conv
epilogue.  References and case lists: tests/_prologue_ref.py and tests/_prologue_cases.py, proved on the CPU by
tests/test_prologue_ref_cpu.py.

Bars.  The split planes of PRO_NONE / PRO_LEAKY are predictable bit for bit (one exact fp32 product per element) and compared as
values with the numpy model.  Prologue values are held per element to `_prologue_ref.element_bar`: the derived split bound
max(2^-22 |u|, 2^-25 / x_scale) + the `hard_bar` rule of tests/test_kernel_edges_gpu.py normalised per (b, channel) row,
max(3e-6 * max(1, row max |ref|), 4 x the fp32 contract's own error against the same fp64 reference on the same row) + for Snake
channels 2.4e-7 / |alpha| (st2_act.h's stated error of sin_sq times the 1 / alpha that multiplies it).  The kernel's output never
enters a bar.  Every value test prints its (kernel error, fp32-contract error) pairs before it asserts (pytest -s), per row class
on the hard cases; the pairs measured on an MI355X stand beside the cases."""
import numpy as np
import pytest
import torch

import _prologue_cases as K
import _prologue_ref as P
from oracle import ops_ref as R
from styletts2_amd import _hooks, _lib, ops, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
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


def dev_kw(xg, kw):
    """The prologue operands on the device; the statistics come from the library's own reductions of x."""
    out = {k: (g(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if kw["pro"] in P.NORM_PROS:
        out["stats"] = ops.colnorm_stats(xg) if kw["pro"] == R.PRO_COLNORM else ops.instnorm_stats(xg)
    return out


def cpu_kw(kw, dkw):
    out = dict(kw)
    if "stats" in dkw:
        out["stats"] = dkw["stats"].cpu()
    return out


def check_planes(xs, B, C, L, lengths=None):
    """Everything that holds for ANY planes st2_act_split writes: every stored half finite, |lo| <= half an ulp of hi, exact zeros
    in the halo, from each row's end up to Lp and in the channel padding up to cg * 8.  Returns (hi, lo) [B, C, L] float16 and
    the reconstruction (hi + lo) / x_scale [B, C, L] (exact in fp32: at most 22 significant bits, a power-of-two scale)."""
    data = xs.data.cpu()
    assert data.shape == (B, 2, xs.cg, xs.Lp, 8) and xs.cg * 8 >= C and xs.Lp >= xs.halo + L and (xs.C, xs.L) == (C, L)
    assert bool(torch.isfinite(data).all()), "a stored half is not finite"
    hi, lo = P.planes_value(data)
    assert bool((np.abs(lo.numpy().astype(np.float64)) <= P.ulp_f16(hi.numpy()) / 2).all()), "|lo| > ulp(hi) / 2"
    h = xs.halo
    for plane in (hi, lo):
        assert bool((plane[:, :, :h] == 0).all()), "halo"
        assert bool((plane[:, C:] == 0).all()), "channel padding"
        for b in range(B):
            end = L if lengths is None else min(max(int(lengths[b]), 0), L)
            assert bool((plane[b, :, h + end:] == 0).all()), "row %d past its end" % b
    hi, lo = hi[:, :C, h:h + L], lo[:, :C, h:h + L]
    return hi, lo, (hi.float() + lo.float()) / xs.x_scale


def hold_to_fp64(what, got, x, kw, *, x_scale, split=True, lengths=None, classes=None):
    """got [B, C, L] (fp32, CPU) against the fp64 prologue of x per element (`_prologue_ref.element_bar`).  Prints the (kernel
    error, fp32-contract error) pair -- per row class where `classes` names them (channel c is of class c % len) -- then asserts."""
    ref = P.activate64(x, lengths=lengths, **kw)
    c32 = P.activate32(x, lengths=lengths, **kw)
    bar, e32 = P.element_bar(ref, c32, x_scale=x_scale, alpha=kw.get("alpha"), split=split)
    err = (got.double() - ref).abs()
    ek = P.row_max(err)
    n = len(classes) if classes else 1
    for i in range(n):
        sel = torch.arange(ref.shape[1]) % n == i
        if bool(sel.any()):
            print("HARD %s%s: kernel %.3e  fp32-contract %.3e  worst err / bar %.3f" % (
                what, " [%s]" % (classes[i],) if classes else "", ek[:, sel].max().item(), e32[:, sel].max().item(),
                (err[:, sel] / bar[:, sel]).max().item()))
    bad = err > bar
    assert not bool(bad.any()), "%s: %d elements over their bar, worst err / bar %.3f at %s" % (
        what, int(bad.sum()), (err / bar).max().item(), tuple(int(i) for i in np.unravel_index(int((err / bar).argmax()), err.shape)))
    return ref


# ---- 2. split planes, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(K.SPLIT_CASES))
@pytest.mark.parametrize("pro,slope", [(R.PRO_NONE, 0.0), (R.PRO_LEAKY, 0.2), (R.PRO_LEAKY, 0.0)],
                         ids=["none", "leaky_0.2", "leaky_0"])
def test_split_planes_bit_for_bit(case, pro, slope):
    """No affine: the device value is ONE exact fp32 product, x * 1 or (x * slope) * 1, so both planes are what the numpy model
    of st2_split_f16 says -- ties to even, subnormal lo halves, the clamp at 65504, +-inf and NaN (-> -65504) included -- and
    ST2_STATUS_F16_RANGE is raised exactly when an element was clamped."""
    x = K.split_tensor(case)
    B, C, L = x.shape
    xn = x.numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        w = xn if pro == R.PRO_NONE else np.where(xn >= 0, xn, (xn * np.float32(slope)).astype(np.float32))
    hi_m, lo_m, sat = P.split_f16(w)
    xs = ops.activate(g(x), pro=pro, slope=slope)
    torch.cuda.synchronize()
    assert xs.x_scale == 1.0
    hi, lo, _ = check_planes(xs, B, C, L)
    assert torch.equal(hi, torch.from_numpy(hi_m)), "hi: %d differ" % int((hi != torch.from_numpy(hi_m)).sum())
    assert torch.equal(lo, torch.from_numpy(lo_m)), "lo: %d differ" % int((lo != torch.from_numpy(lo_m)).sum())
    assert ops.status() == (_lib.STATUS_F16_RANGE if bool(sat.any()) else 0)
    assert pro != R.PRO_NONE or bool(sat.any()) == (case != "in_range")


# ---- 3. prologue values against fp64 (st2_act_split) ----------------------------------------------------------------------------
def run_act_split(what, x, kw, *, xg=None, lengths=None, classes=None):
    xg = g(x) if xg is None else xg
    dkw = dev_kw(xg, kw)
    xs = ops.activate(xg, lengths=None if lengths is None else lens(lengths), **dkw)
    torch.cuda.synchronize()
    B, C, L = x.shape
    assert xs.x_scale == ops.x_scale_for(kw["pro"]) == P.x_scale_for(kw["pro"])
    _, _, got = check_planes(xs, B, C, L, lengths)
    hold_to_fp64(what, got, x, cpu_kw(kw, dkw), x_scale=xs.x_scale, lengths=lengths, classes=classes)
    assert ops.status() == 0
    return got


@pytest.mark.parametrize("C", K.SHAPE_C)
@pytest.mark.parametrize("pro", K.ALL_PROS)
def test_act_split_edge_shapes(pro, C):
    """L on, one before and one past the 256-position blocks (and one column, and two blocks and one), C around the 8-channel
    slots and the 32-channel padding: every element, and every zero the planes owe the conv."""
    for L in K.SHAPE_L:
        case = K.benign_case(pro, 2, C, L)
        run_act_split("p%d C=%d L=%d" % (pro, C, L), case["x"], case["kw"])


@pytest.mark.parametrize("view", ["channel_slice", "batch_stride"])
@pytest.mark.parametrize("pro", K.ALL_PROS)
def test_act_split_reads_strided_views(pro, view):
    """x as channels 2 .. 2 + C of a wider buffer whose row pitch is L + 3 (x_cs != L), and x with a batch stride of C * L + 7; every
    float outside the view is NaN, so a read through the wrong stride shows in the value or in the status word."""
    B, C, L = 2, 9, 257
    case = K.benign_case(pro, B, C, L)
    if view == "channel_slice":
        big = torch.full((B, C + 5, L + 3), NAN, device=DEV)
        xg = big[:, 2:2 + C, :L]
    else:
        flat = torch.full((B * (C * L + 7),), NAN, device=DEV)
        xg = flat.as_strided((B, C, L), (C * L + 7, L, 1))
    xg.copy_(g(case["x"]))
    assert xg.stride() == ((C + 5) * (L + 3), L + 3, 1) if view == "channel_slice" else xg.stride(0) != C * L
    run_act_split("p%d %s" % (pro, view), case["x"], case["kw"], xg=xg)


@pytest.mark.parametrize("pro", [p for p in K.ALL_PROS if p != R.PRO_COLNORM])
def test_act_split_ragged_rows(pro):
    """lengths 0, 1, L and L + 5 (clamped to L): each row's own end is its zero padding, written AFTER the activation -- under an
    affine prologue pro(0) is not 0."""
    C, L = 9, 257
    for batch in K.length_batches(L):
        case = K.benign_case(pro, 3, C, L)
        run_act_split("p%d lengths %s" % (pro, batch), case["x"], case["kw"], lengths=batch)
    with pytest.raises(_lib.St2Error):
        ops.activate(g(case["x"]), pro=R.PRO_COLNORM, lengths=lens(batch))


@pytest.mark.parametrize("gamma_plus_one", [False, True])
@pytest.mark.parametrize("seg", K.colnorm_segs(257))
def test_act_split_colnorm_segments(seg, gamma_plus_one):
    """gb_seg 1 (an affine row per column), 61 (boundaries inside both 256-position blocks) and L (one row): row l // gb_seg at
    column l.  Adjacent rows differ by more than 1 in every channel, so the columns either side of every boundary -- all columns
    are compared -- miss their bar if they take a neighbour's row.  Columns on an offset of 1e3 and constant columns included.
    Measured on an MI355X (kernel, fp32 contract): seg 1: 4.8e-7 / 2.5e-7, with gamma + 1: 9.1e-7 / 6.7e-7; seg 61: 4.3e-7 / 3.3e-7 and
    1.1e-6 / 8.4e-7; seg 257: 4.7e-7 / 2.7e-7 and 1.0e-6 / 7.4e-7."""
    C, L = 33, 257
    case = K.colnorm_case(C, L, gb_seg=seg, gamma_plus_one=gamma_plus_one)
    got = run_act_split("colnorm seg=%d +1=%d" % (seg, gamma_plus_one), case["x"], case["kw"])
    edges = [l for l in range(1, L) if l // seg != (l - 1) // seg]
    assert len(edges) == (L - 1) // seg and got.shape[-1] == L  # ... and they are all inside what was compared


# The (kernel error, fp32-contract error) pairs measured on an MI355X stand beside the row classes in tests/_prologue_cases.py;
# colnorm (B = 2, C = 33, columns on an offset of 1e3 and constant columns): 4.2e-7 / 4.0e-7.
HARD = {
    # AdaIN + LeakyReLU(0.2)
    "adain_leaky": (lambda: K.adain_case(False), [r[0] for r in K.ADAIN_ROWS]),
    # AdaIN + Snake, alphas 1 / 30 / 0.1 / 0.01 / -2 over the same rows
    "adain_snake": (lambda: K.adain_case(True), [r[0] for r in K.ADAIN_ROWS]),
    # Snake alone: the class is (alpha, kind, max |alpha u|)
    "snake": (lambda: K.snake_case(), ["a=%g %s %s" % r for r in K.SNAKE_ROWS]),
    "colnorm": (lambda: K.colnorm_case(33, 257, B=2), None),
    "leaky_0": (lambda: K.leaky_case(0.0), K.LEAKY_ROWS),
    "leaky_0.01": (lambda: K.leaky_case(0.01), K.LEAKY_ROWS),
    "leaky_0.2": (lambda: K.leaky_case(0.2), K.LEAKY_ROWS),
}


@pytest.mark.parametrize("name", sorted(HARD))
def test_act_split_hard_rows(name):
    make, classes = HARD[name]
    case = make()
    got = run_act_split(name, case["x"], case["kw"], classes=classes)
    if name.startswith("adain"):  # gamma = -1: g = 0, the affine is exactly beta whatever the statistics
        gz = [c for c in range(got.shape[1]) if K.ADAIN_ROWS[c % len(K.ADAIN_ROWS)][0] == "g_zero"]
        assert len(gz) > 0 and bool((got[:, gz] == got[:, gz][:, :, :1]).all()), "g = 0 rows must be constant"


# ---- 4. the same hard inputs on the fused routes ------------------------------------------------------------------------------
def _fused_inputs(name, C, L):
    if name.startswith("split_"):
        pro, slope = (R.PRO_LEAKY, 0.2) if name.endswith("_leaky") else (R.PRO_NONE, 0.0)
        case = name[len("split_"):].replace("_leaky", "")
        return K.split_tensor(case, C, L), dict(pro=pro, slope=slope), case != "in_range"
    case = K.hard_cases(C, L)[name]
    return case["x"], case["kw"], False


FUSED_NAMES = (["split_%s" % c for c in sorted(K.SPLIT_CASES)] + ["split_in_range_leaky", "split_nan_leaky", "split_inf_leaky"]
               + sorted(K.hard_cases(24, 8)))


@pytest.mark.parametrize("C", [24, 40, 72])  # the 32-row (packed st2_f2 prologue), 64-row and 128-row layouts
@pytest.mark.parametrize("name", FUSED_NAMES)
def test_hard_inputs_agree_on_every_route(name, C):
    """The hard tensors of sections 2 and 3 through an identity weight on tap ks // 2 (tests/test_ops_gpu.py
    test_prologues_agree_bitwise: every output is exactly (hi + lo) / x_scale of the operand under the tap): act_split + xs conv,
    the one-role fused kernel and, where it exists (AdaIN + Snake at k = 3, C_out <= 64), the warp-specialised build are
    torch.equal, equal the reconstruction from st2_act_split's planes -- so the fp64 verdict of section 3, repeated here at this
    C, carries over to every route -- and raise the same status bit.  Then the exact-fp32 conv (its own prologue, libm sinf)
    against the same fp64 reference at the same bar without the split term.
    Measured on an MI355X at C = 24 / 40 / 72, max over the tensor (split routes; exact-fp32 conv; fp32 contract): adain_leaky
    1.7e-5; 9.7e-6; 9.7e-6 -- adain_snake 2.3e-5; 2.3e-5; 2.3e-5 -- snake 1.5e-3; 4.9e-4; 4.9e-4 (rows of |u| = 1e4: the split's
    2^-22 |u| and half an fp32 ulp) -- colnorm 5.6e-7; 4.2e-7; 4.2e-7 -- leaky 3.9e-3; 5.9e-4; 5.9e-4 (rows of 6e4) -- the in-range
    special values 1.2e-4; 0; 0."""
    lib = _lib.load()
    L = 600
    ks = 3 if name == "adain_snake" else 1
    x, kw, saturates = _fused_inputs(name, C, L)
    B = x.shape[0]
    xg = g(x)
    dkw = dev_kw(xg, kw)
    w = torch.zeros(C, C, ks)
    w[torch.arange(C), torch.arange(C), ks // 2] = 1.0
    wt = weights.pack_conv_f16s(w).to(DEV)
    outs, status = {}, {}

    def done(route, out):
        torch.cuda.synchronize()
        outs[route] = out.cpu()
        status[route] = ops.status(clear=True)

    xs = ops.activate(xg, **dkw)
    done("act_split", ops.conv1d_xs(xs, wt, C, ks, pad_left=ks // 2))
    try:
        for route, variant in (("one_role", 1), ("ws", 2)):
            if variant == 2 and not (kw["pro"] == R.PRO_ADAIN_SNAKE and ks == 3 and C <= 64):
                continue
            lib.st2_conv1d_f16s_set_variant(variant)
            with _hooks.override(conv_path="fused"):
                done(route, ops.conv1d(xg, wt, C, ks, pad_left=ks // 2, **dkw))
    finally:
        lib.st2_conv1d_f16s_set_variant(0)
    assert ("ws" in outs) == (name == "adain_snake" and C <= 64)
    _, _, recon = check_planes(xs, B, C, L)
    assert torch.equal(outs["act_split"], recon), "xs conv vs planes: %d differ" % int((outs["act_split"] != recon).sum())
    for route, out in outs.items():
        assert torch.equal(out, outs["act_split"]), (route, int((out != outs["act_split"]).sum()))
        assert status[route] == (_lib.STATUS_F16_RANGE if saturates else 0), (route, status)
    assert bool(torch.isfinite(recon).all()) and float(recon.min()) < float(recon.max())
    if name.startswith("split_"):  # predictable bit for bit here too: the clamp's +-65504 and a NaN's -65504 on every route
        with np.errstate(invalid="ignore", over="ignore"):
            xn = x.numpy()
            wv = xn if kw["pro"] == R.PRO_NONE else np.where(xn >= 0, xn, (xn * np.float32(kw["slope"])).astype(np.float32))
        hi_m, lo_m, sat = P.split_f16(wv)
        assert bool(sat.any()) == saturates
        assert torch.equal(recon, torch.from_numpy(hi_m.astype(np.float32) + lo_m.astype(np.float32)))
    if saturates:
        return  # inf * 0 in the exact-fp32 conv's other rows is a NaN by IEEE, not by the prologue; the clamp is the split's alone
    ckw = cpu_kw(kw, dkw)
    hold_to_fp64("%s C=%d split routes" % (name, C), recon, x, ckw, x_scale=xs.x_scale)
    out32 = ops.conv1d(xg, g(weights.pack_conv(w)), C, ks, pad_left=ks // 2, **dkw)
    torch.cuda.synchronize()
    hold_to_fp64("%s C=%d exact-fp32 conv" % (name, C), out32.cpu(), x, ckw, x_scale=xs.x_scale, split=False)
    assert ops.status() == 0


# ---- 5. epilogue activations at hard arguments --------------------------------------------------------------------------------
EPI_PLAIN = 3e-6  # the bar of the conv contract tests (tests/test_ops_gpu.py test_conv1d_matches_contract)
# measured on an MI355X, xs and fused alike, C = 32 / 40 (kernel, fp32 contract), in units of the row's scale:
#   gelu 8.9e-8 / 9.0e-8   gelu_tanh 8.5e-8 / 9.6e-8   tanh 3.0e-8 / 3.0e-8   leaky 4.7e-8 / 4.7e-8 (the slope is an fp32 number)
#   exp rows (relative) 7.5e-8 / 6.0e-8   sin rows, up to 1e4 rad, 1.2e-7 / 3.6e-8 (sin_acc's stated 1.2e-7)
EPI_NAMES = {R.ACT_GELU: "gelu", R.ACT_GELU_TANH: "gelu_tanh", R.ACT_TANH: "tanh", R.ACT_LEAKY: "leaky", R.ACT_EXP_SIN: "exp_sin"}


def _act64(v, act, split, slope):
    F = torch.nn.functional
    if act == R.ACT_GELU:
        return F.gelu(v)
    if act == R.ACT_GELU_TANH:
        return F.gelu(v, approximate="tanh")
    if act == R.ACT_TANH:
        return torch.tanh(v)
    if act == R.ACT_LEAKY:
        return F.leaky_relu(v, slope)
    return torch.cat([torch.exp(v[:, :split]), torch.sin(v[:, split:])], dim=1)


@pytest.mark.parametrize("route", ["xs", "fused"])
@pytest.mark.parametrize("C", [32, 40])  # 32: rows_ok holds, the straight-line build on full blocks; 40: the generic build throughout
@pytest.mark.parametrize("act", [R.ACT_GELU, R.ACT_GELU_TANH, R.ACT_TANH, R.ACT_LEAKY, R.ACT_EXP_SIN],
                         ids=["gelu", "gelu_tanh", "tanh", "leaky", "exp_sin"])
def test_epilogue_activations_at_hard_arguments(act, C, route):
    """st2_conv_epilogue.h `finish` (sin_acc, gelu_erf, gelu_tanh, tanhf, expf) through an identity k = 1 conv with PRO_NONE: the
    activation's argument is the reconstructed operand, which the same conv with ACT_NONE returns exactly, and the reference is the
    fp64 activation of THAT operand.  L = 130: four full 32-column blocks and the one that straddles the row end.  Bar: the
    `hard_bar` rule per (b, channel) row -- absolute for gelu, tanh, leaky and the sin rows, relative for the exp rows."""
    x = K.epilogue_args(act, C)
    B, _, L = x.shape
    sp = K.epilogue_split(C) if act == R.ACT_EXP_SIN else 0
    slope = 0.1
    w = torch.zeros(C, C, 1)
    w[torch.arange(C), torch.arange(C), 0] = 1.0
    wt = weights.pack_conv_f16s(w).to(DEV)
    xg = g(x)

    def conv(**kw):
        if route == "xs":
            return ops.conv1d_xs(ops.activate(xg), wt, C, 1, **kw)
        with _hooks.override(conv_path="fused"):
            return ops.conv1d(xg, wt, C, 1, **kw)

    arg = conv().cpu()
    out = conv(act=act, act_split=sp, act_slope=slope).cpu()
    torch.cuda.synchronize()
    assert (arg - x).abs().max().item() <= (2.0 ** -22 * x.abs()).clamp(min=2.0 ** -25).max().item() and ops.status() == 0
    assert bool(((arg - x).abs() <= (2.0 ** -22 * x.abs()).clamp(min=2.0 ** -25)).all())
    ref = _act64(arg.double(), act, sp, slope)
    c32 = _act64(arg, act, sp, slope).double()
    # both errors in units of the row's scale: max(1, row max |ref|), or |ref| itself on the exp rows (relative, per element)
    scale = torch.clamp(P.row_max(ref), min=1.0).expand_as(ref).clone()
    if act == R.ACT_EXP_SIN:
        scale[:, :sp] = ref[:, :sp].abs()
    err, e32 = (out.double() - ref).abs() / scale, P.row_max((c32 - ref).abs() / scale)
    bar = torch.clamp(4.0 * e32, min=EPI_PLAIN).expand_as(err)
    for nm in (["exp", "sin"] if act == R.ACT_EXP_SIN else ["all"]):
        sel = slice(0, sp) if nm == "exp" else slice(sp, C)
        print("HARD epilogue %s C=%d %s [%s]: kernel %.3e  fp32-contract %.3e  bar %.3e" % (
            EPI_NAMES[act], C, route, nm, err[:, sel].max().item(), e32[:, sel].max().item(), bar[:, sel].max().item()))
    bad = err > bar
    assert not bool(bad.any()), "%d elements over their bar, worst err / bar %.3f at %s" % (
        int(bad.sum()), (err / bar).max().item(), tuple(int(i) for i in np.unravel_index(int((err / bar).argmax()), err.shape)))
