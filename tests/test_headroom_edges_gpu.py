"""The operand-range telemetry (include/st2.h `st2_debug_headroom`) held to an fp64 reference row, on both routes that record it:
st2_act_split (kind 0) and the fused conv's prologue probe (kind 1).  `pipeline.calibrate` turns these rows into every conv
site's operand scale, so a row that is wrong -- measured past a ragged row's end, over channel padding, in the wrong order -- is
a wrong scale on a real checkpoint and nothing else in the suite would say so.

Reference: tests/_headroom_ref.py (proved by tests/test_headroom_ref_cpu.py) on the planes of the launch.  PRO_NONE / PRO_LEAKY:
planes built in numpy from x.  AdaIN / Snake / COLNORM (the sine polynomial is not reproducible in numpy): the planes the
device's own `ops.activate` returns for the same input and lengths -- for the act_split route those ARE the measured launch's;
for the fused route the three prologue implementations are held bitwise equal by tests/test_ops_gpu.py
test_prologues_agree_bitwise and tests/test_prologue_edges_gpu.py.

Bars.  max_abs ([6]) and frac ([7]) are a maximum over exact f16 values and its quotient by 65504 in fp64: EQUAL.  rel_err ([8])
and sub_share ([9]) are quotients of fp64 sums of non-negative terms, each term exact or rounded once, added by atomics in no
fixed order: n terms carry at most n 2^-53 relative error whatever the order.  The largest case here has n = 3 x 72 x 600 =
129 600 elements, n 2^-53 = 1.4e-11; the bar is REL = 1e-9 (it would cover 9e6 terms)."""
import numpy as np
import pytest
import torch

import _headroom_ref as H
import _prologue_cases as K
import _prologue_ref as P
from oracle import ops_ref as R
from styletts2_amd import _hooks, _lib, ops, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-9
ROUTES = ["act_split", "fused"]
KIND = {"act_split": "act_split", "fused": "fused conv"}
SHAPE_C = (24, 40, 72)  # channel tails of the fused conv's 32-, 64- and 128-row layouts; none a multiple of the 32-channel padding
SHAPE_L = (1, 7, 255, 256, 257, 600)  # around the 256-position blocks of the activation pass and the probe's grid stride
RAGGED_PROS = [p for p in K.ALL_PROS if p != R.PRO_COLNORM]
C_OUT = 8


@pytest.fixture(autouse=True)
def _own_status():
    torch.cuda.synchronize()
    ops.status(clear=True)


def g(t):
    return None if t is None else t.to(DEV)


def lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


_W = {}


def weight(C, ks):
    """One packed weight per (C, ks), shared by every case: its values never enter a telemetry row."""
    if (C, ks) not in _W:
        _W[C, ks] = weights.pack_conv_f16s(torch.randn(C_OUT, C, ks, generator=torch.Generator().manual_seed(C + ks)) / 8).to(DEV)
    return _W[C, ks]


def dev_kw(xg, kw, lengths=None):
    """The prologue operands on the device; the statistics are the library's own, over each row's valid columns."""
    out = {k: (g(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if kw["pro"] == R.PRO_COLNORM:
        out["stats"] = ops.colnorm_stats(xg)
    elif kw["pro"] in P.NORM_PROS:
        out["stats"] = ops.instnorm_stats(xg, lengths=None if lengths is None else lens(lengths))
    return out


def measure(route, xg, dkw, lengths=None, x_scale=None, ks=3):
    """One launch on `route` under a recording of its own -> (its row, the XsTensor the act_split route wrote or None)."""
    B, C, L = xg.shape
    ld = None if lengths is None else lens(lengths)
    xs = None
    with ops.headroom() as h:
        if route == "act_split":
            xs = ops.activate(xg, x_scale=x_scale, lengths=ld, **dkw)
        else:
            with _hooks.override(conv_path="fused"):
                ops.conv1d(xg, weight(C, ks), C_OUT, ks, pad_left=ks // 2, x_scale=x_scale, x_len=ld, **dkw)
    assert len(h.rows) == 1, h.rows
    r = h.rows[0]
    assert (r["kind"], r["B"], r["C"], r["L"], r["site"]) == (KIND[route], B, C, L, -1), r
    return r, xs


def reference(x, kw, xg, dkw, lengths=None, x_scale=None, xs=None):
    """The fp64 row of the launch.  `xs`: the planes the measured launch itself returned (act_split route)."""
    pro = kw["pro"]
    if pro in (R.PRO_NONE, R.PRO_LEAKY):
        return H.row(*H.expected_planes(x.numpy(), x_scale or P.x_scale_for(pro), lengths=lengths, pro=pro,
                                        slope=kw.get("slope", 0.0)))
    if xs is None:
        with _hooks.override(conv_path="xs"):
            xs = ops.activate(xg, x_scale=x_scale, lengths=None if lengths is None else lens(lengths), **dkw)
    torch.cuda.synchronize()
    return H.row(*H.planes_of(xs.data.cpu()))


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def hold(what, r, ref):
    print("HEADROOM %s: max_abs %r / %r  rel_err %.17g / %.17g  sub_share %.17g / %.17g" % (
        what, r["max_abs"], ref["max_abs"], r["rel_err"], ref["rel_err"], r["sub_share"], ref["sub_share"]))
    assert r["max_abs"] == ref["max_abs"], (what, r["max_abs"], ref["max_abs"])
    assert r["frac"] == ref["frac"], (what, r["frac"], ref["frac"])
    assert close(r["rel_err"], ref["rel_err"]), (what, r["rel_err"], ref["rel_err"])
    assert close(r["sub_share"], ref["sub_share"]), (what, r["sub_share"], ref["sub_share"])
    assert np.isfinite([r["max_abs"], r["frac"], r["rel_err"], r["sub_share"]]).all()


# ---- 1. dense launches: every prologue, channel tail and block edge -------------------------------------------------------------
@pytest.mark.parametrize("C", SHAPE_C)
@pytest.mark.parametrize("pro", K.ALL_PROS)
@pytest.mark.parametrize("route", ROUTES)
def test_dense_row_matches_reference(route, pro, C):
    """B = 2, randn data at the scale by rule (x_scale 1: a third of the elements have a subnormal lo half, so [8] and [9] are far
    from both of their ends).  The planes are padded to 32 channels and to Lp columns: padding must add nothing."""
    for L in SHAPE_L:
        case = K.benign_case(pro, 2, C, L)
        xg = g(case["x"])
        dkw = dev_kw(xg, case["kw"])
        r, xs = measure(route, xg, dkw, ks=1 if pro == R.PRO_COLNORM else 3)
        assert r["x_scale"] == P.x_scale_for(pro) and r["pro"] == ["none", "leaky", "adain+leaky", "adain+snake", "snake",
                                                                    "layernorm"][pro]
        ref = reference(case["x"], case["kw"], xg, dkw, xs=xs)
        hold("%s p%d C=%d L=%d" % (route, pro, C, L), r, ref)
        assert 0.0 < ref["max_abs"] < 65504.0 and ref["rel_err"] > 0.0
        assert ops.status() == 0
    if pro == R.PRO_COLNORM:  # per-row lengths are undefined for it: refused, not measured over something else
        with pytest.raises(_lib.St2Error):
            ops.activate(xg, lengths=lens([L, 1]), **dkw)


# ---- 2. ragged launches: a row ends at x_len[b], whatever memory holds past it -------------------------------------------------
@pytest.mark.parametrize("sentinel", [3.0e5, -7777.0, float("nan")], ids=["3e5", "-7777", "nan"])
@pytest.mark.parametrize("pro", RAGGED_PROS)
@pytest.mark.parametrize("route", ROUTES)
def test_ragged_row_is_measured_over_its_valid_columns(route, pro, sentinel):
    """B = 3 with lengths [L, 1, L // 2 + 1]; every column at and past x_len[b] of the short rows holds the sentinel -- a longer
    earlier batch, a fill value, a NaN.  The row must be the reference's over the valid columns, raise no status bit (a NaN or
    3e5 that reached the split would clamp and say so) and equal the row of the same call with zeroed tails."""
    for C in SHAPE_C:
        for L in SHAPE_L:
            lengths = [L, 1, L // 2 + 1]
            case = K.benign_case(pro, 3, C, L)
            x = case["x"]
            dirty = x.clone()
            clean = x.clone()
            for b, n in enumerate(lengths):
                dirty[b, :, n:] = sentinel
                clean[b, :, n:] = 0.0
            what = "%s p%d C=%d L=%d" % (route, pro, C, L)
            dg, cg_ = g(dirty), g(clean)
            dkw = dev_kw(dg, case["kw"], lengths)
            r, _ = measure(route, dg, dkw, lengths)
            torch.cuda.synchronize()
            assert ops.status() == 0, what
            ref = reference(clean, case["kw"], cg_, dev_kw(cg_, case["kw"], lengths), lengths)  # from the valid columns alone
            hold(what, r, ref)
            rz, _ = measure(route, cg_, dev_kw(cg_, case["kw"], lengths), lengths)
            hold(what + " zeroed tails", rz, ref)
            assert (rz["max_abs"], rz["frac"]) == (r["max_abs"], r["frac"])
            assert close(rz["rel_err"], r["rel_err"]) and close(rz["sub_share"], r["sub_share"])
            assert ops.status() == 0, what


# ---- 3. extremes ------------------------------------------------------------------------------------------------------------
def _plain(C=24, L=257, B=2, seed=5):
    return torch.randn(B, C, L, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("k", [-3, 0, 2])
@pytest.mark.parametrize("route", ROUTES)
def test_operand_at_and_one_ulp_above_the_clamp(route, k):
    """x_scale = 2^k and one element at 65504 / 2^k (exact in fp32): u = 65504, frac == 1.0 and nothing was clamped, so no status
    bit.  The next fp32 above it scales to 65504 (1 + 2^-23): clamped to the same 65504, frac == 1.0, ST2_STATUS_F16_RANGE."""
    xsc = 2.0 ** k
    top = np.float32(65504.0 / xsc)
    assert float(top) * xsc == 65504.0
    for above in (False, True):
        x = _plain() * (0.01 / xsc)
        x[1, 23, 200] = -float(np.nextafter(top, np.float32(np.inf))) if above else -float(top)
        r, _ = measure(route, g(x), dict(pro=R.PRO_NONE), x_scale=xsc)
        torch.cuda.synchronize()
        assert r["x_scale"] == xsc and r["max_abs"] == 65504.0 and r["frac"] == 1.0, r
        hold("%s 2^%d above=%d" % (route, k, above), r, reference(x, dict(pro=R.PRO_NONE), None, None, x_scale=xsc))
        assert ops.status(clear=True) == (_lib.STATUS_F16_RANGE if above else 0)


@pytest.mark.parametrize("route", ROUTES)
def test_all_zero_input_gives_a_finite_row(route):
    r, _ = measure(route, torch.zeros(2, 24, 257, device=DEV), dict(pro=R.PRO_NONE))
    assert (r["max_abs"], r["frac"], r["rel_err"], r["sub_share"]) == (0.0, 0.0, 0.0, 0.0), r
    assert ops.status() == 0


@pytest.mark.parametrize("route", ROUTES)
def test_small_operand_by_rule_equals_the_reference(route):
    """An input at 1e-3 with x_scale = 1: every lo half is subnormal.  Not merely "large": the reference's figures."""
    x = _plain(C=40, L=600) * 1e-3
    r, _ = measure(route, g(x), dict(pro=R.PRO_NONE), x_scale=1.0)
    ref = reference(x, dict(pro=R.PRO_NONE), None, None, x_scale=1.0)
    hold("%s 1e-3" % route, r, ref)
    assert ref["sub_share"] > 0.99 and 3e-6 < ref["rel_err"] < 1e-4  # what test_headroom_reports_both_ends asks of the device


# ---- 4. several launches in one recording -----------------------------------------------------------------------------------
def test_rows_come_back_in_launch_order_with_site_minus_one():
    shapes = [("act_split", R.PRO_NONE, 24, 7), ("fused", R.PRO_LEAKY, 40, 255), ("act_split", R.PRO_SNAKE, 72, 257),
              ("fused", R.PRO_NONE, 24, 600), ("fused", R.PRO_ADAIN_LEAKY, 72, 256)]
    calls = []
    for route, pro, C, L in shapes:
        case = K.benign_case(pro, 2, C, L)
        xg = g(case["x"])
        calls.append((route, case, xg, dev_kw(xg, case["kw"])))
    kept = []
    with ops.headroom() as h:
        for route, case, xg, dkw in calls:
            if route == "act_split":
                kept.append(ops.activate(xg, **dkw))
            else:
                kept.append(None)
                with _hooks.override(conv_path="fused"):
                    ops.conv1d(xg, weight(xg.shape[1], 3), C_OUT, 3, pad_left=1, **dkw)
    assert len(h.rows) == len(shapes)
    for i, ((route, pro, C, L), (_, case, xg, dkw), xs, r) in enumerate(zip(shapes, calls, kept, h.rows)):
        assert (r["index"], r["kind"], r["B"], r["C"], r["L"]) == (i, KIND[route], 2, C, L), r
        assert r["site"] == -1, "a per-kernel call belongs to no engine site"
        hold("launch %d" % i, r, reference(case["x"], case["kw"], xg, dkw, xs=xs))
    with ops.headroom() as h2:  # a new recording starts empty
        pass
    assert h2.rows == []


def test_launches_under_stream_capture_add_no_row():
    """A recorded probe would re-run at every replay and, for the fused conv, read scratch planes the recording has freed: the
    hook promises to skip captured launches.  One eager launch after the capture shows the recording was live."""
    case = K.benign_case(R.PRO_LEAKY, 2, 24, 257)
    xg = g(case["x"])
    dkw = dev_kw(xg, case["kw"])

    def both():
        ops.activate(xg, **dkw)
        with _hooks.override(conv_path="fused"):
            return ops.conv1d(xg, weight(24, 3), C_OUT, 3, pad_left=1, **dkw)

    both()  # packs the weight and loads the kernels outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.headroom() as h:
        with torch.cuda.graph(graph):
            both()
        r_xs = ops.activate(xg, **dkw)
    assert [r["kind"] for r in h.rows] == ["act_split"], h.rows
    hold("after capture", h.rows[0], reference(case["x"], case["kw"], xg, dkw, xs=r_xs))
    assert ops.status() == 0


# ---- 5. the warp-specialised build --------------------------------------------------------------------------------------------
def test_warp_specialised_build_records_the_same_row():
    """AdaIN + Snake at k = 3, C = 24, C_out <= 64 is where the warp-specialised build exists (variant 2); its probe is the one-role
    build's (variant 1).  Dense and ragged."""
    lib = _lib.load()
    C, L = 24, 600
    for lengths in (None, [L, 1, L // 2 + 1]):
        B = 3 if lengths else 2
        case = K.benign_case(R.PRO_ADAIN_SNAKE, B, C, L)
        xg = g(case["x"])
        dkw = dev_kw(xg, case["kw"], lengths)
        rows = {}
        try:
            for variant in (1, 2):
                lib.st2_conv1d_f16s_set_variant(variant)
                rows[variant], _ = measure("fused", xg, dkw, lengths)
        finally:
            lib.st2_conv1d_f16s_set_variant(0)
        ref = reference(case["x"], case["kw"], xg, dkw, lengths)
        for variant in (1, 2):
            hold("variant %d lengths %s" % (variant, lengths), rows[variant], ref)
        assert (rows[1]["max_abs"], rows[1]["frac"]) == (rows[2]["max_abs"], rows[2]["frac"])
        assert ops.status() == 0
