"""Per-kernel parity of the length-aware (ragged) entry points (include/st2.h, ABI v23), one kernel at a time.

Every case runs a batch of rows with lengths of their own, chosen where length handling goes wrong: one column either side of a
32 / 64 / 128 / 256 / 512 tile edge, of a 1024-position interleave tile or of a partial-sum slot, a reflection at the row's own
end, a value above the padded length (clamped).  Inputs past each row's end hold NaN (the header promises selects: nothing
there may reach a stored value) and outputs start as a sentinel, so the tail is checked against what the header promises --
left as the memory held it (conv y_len, adain_leaky_pool, convt_interleave) or exact zeros (conv1d_direct, har_source, stft,
istft, expand).  Row b is compared with the oracle/ops_ref contract applied to the row cut to its own length, evaluated in
float64 where the op allows (har_source: the fp32 bit-faithful contract), at the bar of the plain test of the same kernel in
tests/test_ops_gpu.py.  Per-element and per-frame kernels must also give row b bit for bit as their plain launch on that row
alone."""
import math

import pytest
import torch

from _util import make_conv_case, rel_err
from oracle import ops_ref as R
from styletts2_amd import _hooks, _lib, ops, weights

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


def nan_part(monkeypatch):
    """Partial-sum buffers start as NaN: statistics that match prove the slots past a row's end are never read."""
    monkeypatch.setattr(ops, "new_part", lambda B, C, nt, device: torch.full((B * C * nt * 3,), NAN, device=device))


def check_stats(st, y, what):
    """Epilogue statistics against the fp64 reduction of the stored row y [C, n] (bars of test_conv1d_xs_epilogue_stats)."""
    y = y.detach().cpu().double()
    mean, var = y.mean(-1), y.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    st = st.detach().cpu().double()
    dm = (st[:, 0] - mean).abs().max().item()
    dr = ((st[:, 1] - rstd).abs() / rstd).max().item()
    assert dm < 2e-6 * max(1.0, mean.abs().max().item()), "%s: |d mean| %g" % (what, dm)
    assert dr < 5e-6, "%s: |d rstd| / rstd %g" % (what, dr)


# ---- split-f16 convs: st2_conv1d_f16s (fused prologue) and st2_act_split_len + st2_conv1d_xs ------------------------------
PRO_KEYS = ("pro", "slope", "stats", "gamma", "beta", "alpha")

CONV_CASES = [
    # path, geometry, lengths (x_len = y_len unless y_len is given; values above L are clamped), extras
    # fused: the three wave layouts (C_out > 64, 33..64, <= 32), k = 3 / 7 / 11, dilation > 1, every prologue
    dict(path="fused", B=5, C_in=128, C_out=128, L=600, ks=11, dil=5, pro=R.PRO_ADAIN_SNAKE, res=True, res2=True, div=3.0,
         x_len=[1, 129, 599, 600, 700]),
    dict(path="fused", B=5, C_in=64, C_out=64, L=520, ks=7, dil=3, pro=R.PRO_ADAIN_LEAKY, res=True, res_shift=1,
         x_len=[31, 32, 33, 513, 520], want_stats=True),
    dict(path="fused", B=5, C_in=128, C_out=22, L=530, ks=7, dil=2, pro=R.PRO_LEAKY, act=R.ACT_EXP_SIN,
         x_len=[127, 128, 255, 257, 511]),
    dict(path="fused", B=5, C_in=48, C_out=40, L=300, ks=3, dil=2, pro=R.PRO_NONE, res=True,
         x_len=[1, 128, 129, 299, 300], want_stats=True),
    # the ConvTranspose polyphase GEMM: k = 2, pad_left = 1, one output more than the input (x_len != y_len)
    dict(path="fused", B=5, C_in=64, C_out=120, L=300, ks=2, dil=1, pro=R.PRO_LEAKY, pad_left=1, L_out=301,
         x_len=[1, 33, 150, 299, 300], y_len=[2, 34, 151, 300, 301]),
    # xs: 32-column slots (small grid), 64-column slots, 128-column tiles with row ends in a quarter body (17 of 128 columns)
    dict(path="xs", B=3, C_in=256, C_out=256, L=1900, ks=3, dil=1, pro=R.PRO_ADAIN_SNAKE, res=True, x_len=[33, 1025, 1899],
         want_stats=True, cols=32),
    dict(path="xs", B=3, C_in=128, C_out=128, L=9000, ks=3, dil=1, pro=R.PRO_ADAIN_SNAKE, res=True, x_len=[65, 4097, 9000],
         want_stats=True, cols=64),
    dict(path="xs", B=4, C_in=512, C_out=512, L=400, ks=3, dil=1, pro=R.PRO_ADAIN_LEAKY, res=True, x_len=[257, 273, 400, 450],
         want_stats=True, cols=128),
    dict(path="xs", B=4, C_in=128, C_out=128, L=1300, ks=7, dil=3, pro=R.PRO_NONE, res2=True, div=2.0,
         x_len=[1, 511, 513, 1299]),
    dict(path="xs", B=3, C_in=128, C_out=128, L=777, ks=11, dil=5, pro=R.PRO_ADAIN_SNAKE, x_len=[255, 777, 1000]),
]


def _row(kw, b, xl, yl):
    """make_conv_case keyword arguments restricted to row b at input length xl / output length yl, in float64."""
    out = {}
    for k, v in kw.items():
        if k in ("stats", "gamma", "beta") and torch.is_tensor(v):
            v = v[b:b + 1]
        elif k == "res" and v is not None:
            v = v[b:b + 1, :, :(yl + (1 << kw.get("res_shift", 0)) - 1) >> kw.get("res_shift", 0)]
        elif k == "res2" and v is not None:
            v = v[b:b + 1, :, :yl]
        out[k] = v.double() if torch.is_tensor(v) else v
    out["L_out"] = yl
    return out


def run_conv(case, monkeypatch):
    c = dict(case)
    path, cols, want_stats = c.pop("path"), c.pop("cols", None), c.pop("want_stats", False)
    x_len = c.pop("x_len")
    y_len = c.pop("y_len", None) or x_len
    monkeypatch.setattr(_hooks, "conv_path", "xs" if path == "xs" else "fused")
    x, w, kw = make_conv_case(seed=4242 + c["L"], **c)
    B, L, C_out, ks = c["B"], c["L"], c["C_out"], c["ks"]
    L_out = kw["L_out"] or L
    xl = [min(n, L) for n in x_len]
    yl = [min(n, L_out) for n in y_len]
    xn = x.clone()
    for b in range(B):
        xn[b, :, xl[b]:] = NAN
        if kw.get("res") is not None:
            kw["res"][b, :, (yl[b] + (1 << kw["res_shift"]) - 1) >> kw["res_shift"]:] = NAN
        if kw.get("res2") is not None:
            kw["res2"][b, :, yl[b]:] = NAN
    wt = weights.pack_conv_f16s(w)
    wtg = wt.to(DEV)
    kwg = {k: (g(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if want_stats:
        nan_part(monkeypatch)
    out = torch.full((B, C_out, L_out), SENT, device=DEV)
    if path == "xs":
        xs = ops.activate(g(xn), lengths=lens(x_len), **{k: v for k, v in kwg.items() if k in PRO_KEYS})
        ckw = {k: v for k, v in kwg.items() if k not in PRO_KEYS}
        if cols is not None:
            d = _lib.ConvDesc()
            d.B, d.C_in, d.C_out, d.L_in, d.L_out, d.ks = B, c["C_in"], C_out, L, L_out, ks
            assert _lib.load().st2_conv1d_xs_part_cols(d) == cols, "the case is meant to run %d-column slots" % cols
        r = ops.conv1d_xs(xs, wtg, C_out, ks, out=out, y_len=lens(y_len), want_stats=want_stats, **ckw)
    else:
        r = ops.conv1d(g(xn), wtg, C_out, ks, out=out, x_len=lens(x_len), y_len=lens(y_len), want_stats=want_stats, **kwg)
    out, st = r if want_stats else (r, None)
    torch.cuda.synchronize()
    exact = weights.pack_conv(w).double()
    for b in range(B):
        ref = R.conv1d(x[b:b + 1, :, :xl[b]].double(), exact, C_out, ks, **_row(kw, b, xl[b], yl[b]))
        e = rel_err(out[b:b + 1, :, :yl[b]], ref)
        assert e < 3e-6, "row %d (x_len %d, y_len %d): rel err vs fp64 %g" % (b, x_len[b], y_len[b], e)
        assert bool((out[b, :, yl[b]:] == SENT).all()), "row %d: stored past y_len = %d" % (b, yl[b])
        if st is not None:
            check_stats(st[b], out[b, :, :yl[b]], "row %d (y_len %d)" % (b, yl[b]))
    assert ops.status() == 0
    return x, xl, yl, wtg, kwg, out


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "%s_ci%d_co%d_L%d_k%d_d%d_p%d" % (
    c["path"], c["C_in"], c["C_out"], c["L"], c["ks"], c["dil"], c["pro"]))
def test_split_f16_conv_ragged_rows_match_fp64(case, monkeypatch):
    x, xl, yl, wtg, kwg, out = run_conv(case, monkeypatch)
    if case["path"] != "xs":
        return
    # the xs conv computes every output element with the same products in the same order whatever the tile width or the
    # batch (bitwise across part_cols): row b is its plain launch on the row alone, at its own length
    ckw = {k: v for k, v in kwg.items() if k not in PRO_KEYS}
    for b in range(case["B"]):
        row = {k: (v.float() if torch.is_tensor(v) else v) for k, v in _row(kwg, b, xl[b], yl[b]).items()}
        xs = ops.activate(g(x[b:b + 1, :, :xl[b]]), **{k: v for k, v in row.items() if k in PRO_KEYS})
        solo = ops.conv1d_xs(xs, wtg, case["C_out"], case["ks"], **{k: v for k, v in row.items() if k in ckw or k == "L_out"})
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :yl[b]]), "row %d (y_len %d) differs from its solo launch" % (b, yl[b])
    assert ops.status() == 0


def test_split_k_conv_with_y_len(monkeypatch):
    """A split-K geometry of st2_conv1d_f16s (few workgroups, long k loop): the slices' reduction applies the row ends."""
    d = _lib.ConvDesc()
    d.B, d.C_in, d.C_out, d.L_in, d.L_out, d.ks, d.dil = 3, 2048, 1024, 100, 100, 1, 1
    d.wq_co_pad, d.wq_cin_pad = 1024, 2048
    assert _lib.load().st2_conv1d_f16s_splitk_bytes(d) > 0, "the case is meant to run split-K"
    run_conv(dict(path="fused", B=3, C_in=2048, C_out=1024, L=100, ks=1, dil=1, pro=R.PRO_NONE, res=True, res2=True, div=2.0,
                  x_len=[1, 33, 99]), monkeypatch)


def test_warp_specialised_variant_with_lengths_is_the_one_role_result(monkeypatch):
    """st2_conv1d_f16s_set_variant(2) asks for the warp-specialised build, which does not carry row ends (ws_eligible): with
    lengths set the launch must still give the one-role result bit for bit."""
    lib = _lib.load()
    case = dict(path="fused", B=3, C_in=40, C_out=64, L=9001, ks=7, dil=1, pro=R.PRO_ADAIN_SNAKE, res=True,
                x_len=[4097, 8999, 9001], want_stats=True)
    outs = []
    try:
        for variant in (1, 2):
            lib.st2_conv1d_f16s_set_variant(variant)
            outs.append(run_conv(case, monkeypatch)[-1].clone())
    finally:
        lib.st2_conv1d_f16s_set_variant(0)
    assert torch.equal(outs[0], outs[1])


def test_activate_len_planes_are_selects_and_clamp():
    """st2_act_split_len: position l of row b is x_scale * pro(x) for l < len[b], exactly 0 from there (NaN past the end never
    reaches a plane), lengths above L clamp to L; each row's planes are those of its plain launch on the row alone."""
    B, C, L = 4, 70, 333
    x, _, kw = make_conv_case(seed=8, B=B, C_in=C, C_out=8, L=L, ks=1, dil=1, pro=R.PRO_ADAIN_SNAKE)
    n = [1, 32, 257, 400]
    xn = x.clone()
    for b in range(B):
        xn[b, :, min(n[b], L):] = NAN
    akw = {k: (g(v) if torch.is_tensor(v) else v) for k, v in kw.items() if k in PRO_KEYS}
    xs = ops.activate(g(xn), lengths=lens(n), **akw)
    torch.cuda.synchronize()
    d = xs.data.cpu()
    for b in range(B):
        m = min(n[b], L)
        solo = ops.activate(g(x[b:b + 1, :, :m]), **{k: (v[b:b + 1] if k in ("stats", "gamma", "beta") else v)
                                                     for k, v in akw.items()})
        torch.cuda.synchronize()
        s = solo.data.cpu()
        assert torch.equal(d[b, :, :, :xs.halo + m], s[0, :, :, :xs.halo + m]), "row %d" % b
        assert d[b, :, :, xs.halo + m:].float().abs().max().item() == 0.0, "row %d: plane tail past len = %d" % (b, m)
    assert ops.status() == 0
    with pytest.raises(_lib.St2Error):
        ops.activate(g(x), pro=R.PRO_COLNORM, stats=g(R.colnorm_stats(x)), gamma=g(torch.ones(1, C)), beta=g(torch.zeros(1, C)),
                     lengths=lens([L] * B))


def test_packed_fp32_weight_rejects_lengths():
    x = torch.randn(2, 8, 40, device=DEV)
    wt = weights.pack_conv(torch.randn(8, 8, 3)).to(DEV)
    with pytest.raises(_lib.St2Error):
        ops.conv1d(x, wt, 8, 3, pad_left=1, y_len=lens([40, 20]))
    torch.cuda.synchronize()
    assert ops.status() == 0


# ---- st2_stats_finalize_len on its own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [32, 64, 128, 1024])
def test_stats_finalize_len_counts_only_valid_columns(cols):
    """Synthetic shifted partial sums (what the producers write: slot i = (sum, sum of squares) of y - y[first column of the
    slot] over its columns) for rows that end one column either side of a slot boundary; the slots past each end hold NaN."""
    B, Cc = 5, 3
    L = 4 * cols + 7
    nt = -(-L // cols)
    n = [cols - 1, cols, cols + 1, 3 * cols + 1, L + 5]  # the last clamps to L
    gen = torch.Generator().manual_seed(cols)
    y = (torch.randn(B, Cc, L, generator=gen) * 0.5 + torch.randn(1, Cc, 1, generator=gen) * 3.0).float()
    part = torch.full((B * Cc, nt, 2), NAN)
    shift = torch.full((B * Cc, nt), NAN)
    for b in range(B):
        m = min(n[b], L)
        for c in range(Cc):
            r = b * Cc + c
            for i in range(-(-m // cols)):
                seg = y[b, c, i * cols:min((i + 1) * cols, m)].double()
                dv = seg - seg[0]
                part[r, i, 0], part[r, i, 1], shift[r, i] = dv.sum().float(), (dv * dv).sum().float(), seg[0].float()
    buf = g(torch.cat([part.reshape(-1), shift.reshape(-1)]))
    st = ops.stats_finalize(buf, B, Cc, nt, L, cols=cols, lengths=lens(n), len_div=Cc)
    torch.cuda.synchronize()
    for b in range(B):
        check_stats(st[b], y[b, :, :min(n[b], L)], "row %d (len %d, %d-column slots)" % (b, n[b], cols))
    assert ops.status() == 0


# ---- st2_instnorm_stats_len -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n", [(2100, [1, 2047, 2048, 2049, 2100]), (1500, [3, 700, 1499, 1500, 9999]),
                                 (48001, [2048, 2049, 30001, 48000, 48001])])
def test_instnorm_stats_len(L, n):
    """Row b over its first n[b] columns against the fp64 reduction (bars of test_instnorm_stats); NaN past the end; lengths
    above L clamp.  The launch picks 64 or 256 threads from the PADDED L, so a row of <= 2048 columns in a batch padded past
    2048 may reduce in another order than alone: bitwise equality with the solo launch is reported, not asserted."""
    B, C = len(n), 6
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(B, C, L, generator=gen) * 2.0 + 5.0
    xn = x.clone()
    for b in range(B):
        xn[b, :, min(n[b], L):] = NAN
    st = ops.instnorm_stats(g(xn), lengths=lens(n)).cpu()
    solo_equal = []
    for b in range(B):
        m = min(n[b], L)
        ref = R.instnorm_stats(x[b:b + 1, :, :m].double())[0]
        assert rel_err(st[b, :, 0], ref[:, 0]) < 1e-6, "row %d (len %d): mean" % (b, n[b])
        assert rel_err(st[b, :, 1], ref[:, 1]) < 1e-5, "row %d (len %d): rstd" % (b, n[b])
        solo = ops.instnorm_stats(g(x[b:b + 1, :, :m]), lengths=lens([m])).cpu()
        solo_equal.append(bool(torch.equal(solo[0], st[b])))
    print("instnorm_stats_len L=%d: row == solo launch bitwise: %s" % (L, solo_equal))
    assert ops.status() == 0


@pytest.mark.parametrize("L,n", [(1000, 999), (3001, 2999)])
def test_instnorm_stats_len_is_address_independent(L, n):
    """The same row stored at float offsets 0, 1, 2, 3 (16-byte aligned or not) gives bitwise the same statistics."""
    B, C = 4, 5
    pitch = (L + 7) // 4 * 4
    bs = C * pitch + 1  # batch item b starts b floats past a 16-byte boundary
    gen = torch.Generator().manual_seed(n)
    row = torch.randn(C, L, generator=gen) * 3.0 - 1.0
    flat = torch.full((B * bs + pitch,), NAN, device=DEV)
    x = flat.as_strided((B, C, L), (bs, pitch, 1))
    x.copy_(g(row).unsqueeze(0).expand(B, C, L))
    assert [(x[b].data_ptr() // 4) % 4 for b in range(B)] == [0, 1, 2, 3]
    st = ops.instnorm_stats(x, lengths=lens([n] * B)).cpu()
    for b in range(1, B):
        assert torch.equal(st[b], st[0]), "offset %d" % b
    ref = R.instnorm_stats(row[None, :, :n].double())[0]
    assert rel_err(st[0, :, 0], ref[:, 0]) < 1e-6 and rel_err(st[0, :, 1], ref[:, 1]) < 1e-5
    assert ops.status() == 0


# ---- st2_convt_interleave_stats_len -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_out,s,p,L_raw,reflect", [(6, 6, 3, 1320, True), (3, 2, 1, 3400, False), (8, 10, 5, 1200, False)])
@pytest.mark.parametrize("want_stats", [False, True])
def test_convt_interleave_len(C_out, s, p, L_raw, reflect, want_stats, monkeypatch):
    """Rows of out_len 1023 / 1024 / 1025 (either side of a 1024-position tile) and a short one; the phase columns past q_len
    hold NaN (the transposed conv's zero padding), outputs past out_len keep the sentinel, the statistics cover only the row."""
    B = 4
    L_out = L_raw + (1 if reflect else 0)
    Lq = (L_raw + p) // s + 2
    out_len = [1023, 1024, 1025, 7]
    q_len = [(o - (1 if reflect else 0) + p) // s + 1 for o in out_len]  # enough columns for the row's last output
    q_len[1] -= 1  # one row whose last output falls in the zero padding
    gen = torch.Generator().manual_seed(s * 100 + L_raw)
    ph = torch.randn(B, s * C_out, Lq, generator=gen)
    add = torch.randn(B, C_out, L_out, generator=gen)
    bias = torch.randn(C_out, generator=gen)
    phn, addn = ph.clone(), add.clone()
    for b in range(B):
        phn[b, :, q_len[b]:] = NAN
        addn[b, :, out_len[b]:] = NAN
    if want_stats:
        nan_part(monkeypatch)
    out = torch.full((B, C_out, L_out), SENT, device=DEV)
    r = ops.convt_interleave(g(phn), C_out, s, p, L_raw, bias=g(bias), add=g(addn), reflect_left=reflect, out=out,
                             want_stats=want_stats, q_len=lens(q_len), out_len=lens(out_len))
    out, st = r if want_stats else (r, None)
    torch.cuda.synchronize()
    for b in range(B):
        o = out_len[b]
        phr = torch.zeros(1, s * C_out, Lq, dtype=torch.float64)
        phr[..., :q_len[b]] = ph[b:b + 1, :, :q_len[b]].double()
        ref = R._convt_interleave(phr, C_out, s, p, o - (1 if reflect else 0), bias=bias.double(), add=add[b:b + 1, :, :o].double(),
                                  reflect_left=reflect)
        assert rel_err(out[b:b + 1, :, :o], ref) < 2e-5, "row %d (out_len %d)" % (b, o)
        assert bool((out[b, :, o:] == SENT).all()), "row %d: stored past out_len = %d" % (b, o)
        if st is not None:
            check_stats(st[b], out[b, :, :o], "row %d (out_len %d)" % (b, o))
    assert ops.status() == 0


# ---- st2_conv1d_direct_len --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in,C_out,ks,stride,pad,L", [(22, 16, 12, 6, 3, 481), (1, 8, 60, 30, 15, 3000), (256, 1, 1, 1, 0, 300)])
def test_conv1d_direct_len(C_in, C_out, ks, stride, pad, L):
    B = 4
    L_out = (L + 2 * pad - ks) // stride + 1
    x_len = [1, L // 2 + 1, L - 1, L]
    y_len = [1, (x_len[1] + 2 * pad - ks) // stride + 1, L_out - 1, L_out + 3]
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(B, C_in, L, generator=gen)
    w = torch.randn(C_out, C_in, ks, generator=gen) * 0.2
    bias = torch.randn(C_out, generator=gen)
    xn = x.clone()
    for b in range(B):
        xn[b, :, x_len[b]:] = NAN
    out = torch.full((B, C_out, L_out), SENT, device=DEV)
    ops.conv1d_direct(g(xn), g(w), g(bias), stride, pad, out=out, x_len=lens(x_len), y_len=lens(y_len))
    torch.cuda.synchronize()
    for b in range(B):
        yl = min(y_len[b], L_out)
        xr = torch.zeros(1, C_in, L, dtype=torch.float64)
        xr[..., :x_len[b]] = x[b:b + 1, :, :x_len[b]].double()
        ref = R.conv1d_direct(xr, w.double(), bias.double(), stride, pad)[:, :, :yl]
        assert rel_err(out[b:b + 1, :, :yl], ref) < 1e-5, "row %d" % b
        if yl < L_out:
            assert out[b, :, yl:].abs().max().item() == 0.0, "row %d: tail not exactly 0" % b
        # per-element kernel: bitwise its plain launch on the row alone (input cut to x_len, L_out = y_len)
        solo = ops.conv1d_direct(g(x[b:b + 1, :, :x_len[b]]), g(w), g(bias), stride, pad, L_out=yl)
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :yl]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


# ---- st2_adain_leaky_pool_len -----------------------------------------------------------------------------------------------
def test_adain_leaky_pool_len():
    B, C, L = 4, 70, 300
    n = [1, 2, 129, 300]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(B, C, L, generator=gen) + 1.0
    st = R.instnorm_stats(x)
    h = torch.randn(B, 2 * C, generator=gen) * 0.3
    w = torch.randn(C, 3, generator=gen)
    bias = torch.randn(C, generator=gen)
    xn = x.clone()
    for b in range(B):
        xn[b, :, n[b]:] = NAN
    hg = g(h)
    out = torch.full((B, C, 2 * L), SENT, device=DEV)
    ops.adain_leaky_pool(g(xn), g(st), hg[:, :C], hg[:, C:], 0.2, g(w), g(bias), out=out, lengths=lens(n))
    torch.cuda.synchronize()
    for b in range(B):
        m = n[b]
        ref = R.adain_leaky_pool(x[b:b + 1, :, :m].double(), st[b:b + 1].double(), h[b:b + 1, :C].double(),
                                 h[b:b + 1, C:].double(), 0.2, w.double(), bias.double())
        assert rel_err(out[b:b + 1, :, :2 * m], ref) < 1e-5, "row %d" % b
        assert bool((out[b, :, 2 * m:] == SENT).all()), "row %d: stored past 2 len = %d" % (b, 2 * m)
        solo = ops.adain_leaky_pool(g(x[b:b + 1, :, :m]), g(st[b:b + 1]), hg[b:b + 1, :C], hg[b:b + 1, C:], 0.2, g(w), g(bias))
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :2 * m]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


# ---- st2_har_source_len -----------------------------------------------------------------------------------------------------
def test_har_source_len():
    """f_len = 1, a voiced -> unvoiced switch in a row's last frame, an unvoiced -> voiced one, f_len = F; f0 and noise past
    f_len * U hold NaN; the output is exactly 0 from f_len * U on."""
    B, F, U, H = 4, 40, 300, 9
    f_len = [1, 23, 17, 40]
    gen = torch.Generator().manual_seed(23)
    f0 = torch.rand(B, F, generator=gen) * 300.0 + 80.0
    f0[1, 22] = 0.0                     # voiced -> unvoiced in the last frame of row 1
    f0[2, :16] = 0.0                    # unvoiced -> voiced in the last frame of row 2
    f0[3, F // 2: F // 2 + 3] = -40.0
    noise = torch.randn(B, F * U, H, generator=gen)
    lw = torch.randn(H, generator=gen) * 0.5
    lb = torch.randn(1, generator=gen) * 0.1
    f0n, noisen = f0.clone(), noise.clone()
    for b in range(B):
        f0n[b, f_len[b]:] = NAN
        noisen[b, f_len[b] * U:] = NAN
    out = torch.full((B, F * U), SENT, device=DEV)
    ops.har_source(g(f0n), U, g(noisen), g(lw), g(lb), f_len=lens(f_len), out=out)
    torch.cuda.synchronize()
    for b in range(B):
        m = f_len[b] * U
        ref = R.har_source(f0[b:b + 1, :f_len[b]], U, noise[b:b + 1, :m], lw, lb)
        diff = (out[b:b + 1, :m].cpu() - ref).abs().max().item()
        assert diff < 2e-5, "row %d (f_len %d): max %g" % (b, f_len[b], diff)
        if m < F * U:
            assert out[b, m:].abs().max().item() == 0.0, "row %d: tail not exactly 0" % b
        solo = ops.har_source(g(f0[b:b + 1, :f_len[b]]), U, g(noise[b:b + 1, :m]), g(lw), g(lb))
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :m]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


# ---- st2_stft_mag_phase_len / st2_istft_len ---------------------------------------------------------------------------------
def _stft64(x, n_fft, hop):
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    X = torch.stft(x.double(), n_fft, hop, n_fft, window=win, return_complex=True)
    return torch.cat([X.abs(), X.angle()], dim=1)


def _istft64(sp, n_fft, hop):
    nb = n_fft // 2 + 1
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    sp = sp.double()
    return torch.istft(sp[:, :nb] * torch.exp(sp[:, nb:] * 1j), n_fft, hop, n_fft, window=win).unsqueeze(-2)


def test_stft_mag_phase_len():
    """Rows not a multiple of hop long, n_fft / 2 + 1 samples (the shortest row the reflection allows) and L, each reflected at
    its own end; frames past len // hop are exactly 0.  Rows of <= n_fft / 2 samples clamp to n_fft / 2 + 1 (include/st2.h)."""
    n_fft, hop, L = 20, 5, 4000
    n = [11, 1237, 2003, 3999, 4000, 10, 1, 0]
    B = len(n)
    M = L // hop + 1
    gen = torch.Generator().manual_seed(29)
    x = torch.tanh(torch.randn(B, L, generator=gen))
    xn = x.clone()
    for b in range(B):
        xn[b, max(n[b], n_fft // 2 + 1):] = NAN
    out = torch.full((B, n_fft + 2, M), SENT, device=DEV)
    ops.stft_mag_phase(g(xn), n_fft, hop, lengths=lens(n), out=out)
    torch.cuda.synchronize()
    nb = n_fft // 2 + 1
    for b in range(B):
        m = max(n[b], nb)
        Mb = m // hop + 1
        got = out[b:b + 1, :, :Mb].cpu()
        ref = _stft64(x[b:b + 1, :m], n_fft, hop)
        assert (got[:, :nb] - ref[:, :nb]).abs().max().item() < 2e-5, "row %d (len %d): magnitude" % (b, n[b])
        d = torch.remainder(got[:, nb:].double() - ref[:, nb:] + math.pi, 2 * math.pi) - math.pi
        assert (d.abs() * ref[:, :nb]).max().item() < 5e-5, "row %d (len %d): phase" % (b, n[b])
        if Mb < M:
            assert out[b, :, Mb:].abs().max().item() == 0.0, "row %d: frames past len // hop not 0" % b
        solo = ops.stft_mag_phase(g(x[b:b + 1, :m]), n_fft, hop)
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :Mb]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


def test_istft_len():
    n_fft, hop, M = 20, 5, 201
    m_len = [2, 3, 200, 201]
    B = len(m_len)
    gen = torch.Generator().manual_seed(31)
    sp = torch.cat([torch.exp(torch.randn(B, 11, M, generator=gen)), torch.sin(torch.randn(B, 11, M, generator=gen) * 3)], 1)
    spn = sp.clone()
    for b in range(B):
        spn[b, :, m_len[b]:] = NAN
    out = torch.full((B, 1, hop * (M - 1)), SENT, device=DEV)
    ops.istft(g(spn), n_fft, hop, m_len=lens(m_len), out=out)
    torch.cuda.synchronize()
    for b in range(B):
        m = m_len[b]
        Lw = hop * (m - 1)
        ref = _istft64(sp[b:b + 1, :, :m], n_fft, hop)
        got = out[b:b + 1, :, :Lw].cpu().double()
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 2e-5 * ref.abs().max().item() + 1e-6, "row %d (m_len %d)" % (b, m)
        if m < M:
            assert out[b, :, Lw:].abs().max().item() == 0.0, "row %d: tail not exactly 0" % b
        solo = ops.istft(g(sp[b:b + 1, :, :m]), n_fft, hop)
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :Lw]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


# ---- st2_expand_by_durations_len --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True])
def test_expand_by_durations_len(shift):
    B, C, N, T = 4, 70, 20, 300
    n = [1, 37, 256, 300]
    gen = torch.Generator().manual_seed(37)
    x = torch.randn(B, C, N, generator=gen)
    dur = torch.zeros(B, N, dtype=torch.int64)
    for b in range(B):
        cuts = torch.sort(torch.randint(0, n[b] + 1, (N - 1,), generator=gen)).values
        edges = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([n[b]])])
        dur[b] = edges[1:] - edges[:-1]
        assert int(dur[b].sum()) == n[b]
    out = torch.full((B, C, T), SENT, device=DEV)
    ops.expand_by_durations(g(x), g(dur), T, shift=shift, out=out, lengths=lens(n))
    torch.cuda.synchronize()
    for b in range(B):
        ref = R.expand_by_durations(x[b:b + 1].double(), dur[b:b + 1], n[b], shift=shift)
        assert torch.equal(out[b:b + 1, :, :n[b]].cpu().double(), ref), "row %d (len %d)" % (b, n[b])
        if n[b] < T:
            assert out[b, :, n[b]:].abs().max().item() == 0.0, "row %d: tail not exactly 0" % b
        solo = ops.expand_by_durations(g(x[b:b + 1]), g(dur[b:b + 1]), n[b], shift=shift)
        torch.cuda.synchronize()
        assert torch.equal(solo, out[b:b + 1, :, :n[b]]), "row %d differs from its solo launch" % b
    assert ops.status() == 0


# ---- st2_ragged_lengths -----------------------------------------------------------------------------------------------------
def test_ragged_lengths_is_floor_division():
    T_max = 90
    frames = [-3, 0, 1, 45, T_max, T_max + 7]
    coef = [(600, 0, 1), (2, 1, 1), (1, -5, 3), (-2, 3, 4), (3, -200, 7), (1, 0, 2), (5, -91, 6)]
    out = ops.ragged_lengths(lens(frames), T_max, coef).cpu()
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(coef), len(frames))
    for i, (mul, add, div) in enumerate(coef):
        for b, f in enumerate(frames):
            fc = min(max(f, 1), T_max)
            assert int(out[i, b]) == (mul * fc + add) // div, (mul, add, div, f)
    assert ops.status() == 0
