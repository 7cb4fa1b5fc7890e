"""The references and case lists of tests/test_prologue_edges_gpu.py, proved without a GPU: the numpy split meets its derived bound,
the fp64 prologue is the fp32 contract to fp32 round-off on benign data, and every hand-curated case list covers what it claims."""
import math

import numpy as np
import pytest
import torch

import _prologue_cases as K
import _prologue_ref as P
from oracle import ops_ref as R


def _sweep():
    """fp32 values across the f16 range: every power of two from 2^-30 to 2^16 under random mantissas, the f16 grid around each
    binade edge, fp32 subnormals, the top of the range and the specials."""
    rng = np.random.default_rng(K.SEED)
    e = np.arange(-30, 17, dtype=np.float64)
    v = (np.ldexp(1.0, e.astype(int))[:, None] * (1.0 + rng.random((e.size, 400)))).ravel()
    edges = np.ldexp(1.0, np.arange(-25, 16))[:, None] * (1.0 + np.array([-2.0 ** -11, -2.0 ** -12, -2.0 ** -24, 0.0, 2.0 ** -23,
                                                                           2.0 ** -12, 2.0 ** -11, 2.0 ** -10]))[None, :]
    named = [x for row in K.SPLIT_ROWS.values() for x in row]
    w = np.concatenate([v, edges.ravel(), np.array(named, dtype=np.float64), [1e-45, 1e-38, 65503.0, 65505.0, 1e30]])
    w = np.concatenate([w, -w]).astype(np.float32)
    return w


def test_split_model_meets_the_derived_bound():
    w = _sweep()
    hi, lo, sat = P.split_f16(w)
    assert hi.dtype == lo.dtype == np.float16 and bool(np.isfinite(hi).all()) and bool(np.isfinite(lo).all())
    inr = np.abs(w) <= K.F16_MAX  # false for NaN
    assert bool((sat == ~inr).all()), "sat exactly on the out-of-range values and the NaN"
    assert int(sat.sum()) > 20 and int(inr.sum()) > 30000
    rec = hi.astype(np.float64) + lo.astype(np.float64)
    err = np.abs(w[inr].astype(np.float64) - rec[inr])
    assert bool((err <= P.split_bound(w[inr])).all()), float((err / P.split_bound(w[inr])).max())
    assert bool((np.abs(lo.astype(np.float64)) <= P.ulp_f16(hi) / 2).all())
    # out of range: the clamp, and a NaN at the negative end
    assert bool((rec[~inr & (w > 0)] == K.F16_MAX).all()) and bool((rec[~inr & ~(w > 0)] == -K.F16_MAX).all())
    # the bound is not slack by a binade: somewhere the error comes within a factor 2 of it in both regimes
    ratio = err / P.split_bound(w[inr])
    big = np.abs(w[inr]) > 2.0 ** -3
    assert ratio[big].max() > 0.5 and ratio[~big].max() > 0.5


def test_ulp_f16_is_the_grid_spacing():
    for v, u in ((1.0, 2.0 ** -10), (1.999, 2.0 ** -10), (2.0, 2.0 ** -9), (65504.0, 32.0), (2.0 ** -14, 2.0 ** -24),
                 (2.0 ** -15, 2.0 ** -24), (0.0, 2.0 ** -24), (-0.75, 2.0 ** -11)):
        assert float(P.ulp_f16(np.array([v]))[0]) == u, v
        h = np.float16(v)
        assert v == 65504.0 or float(np.nextafter(h, np.float16(np.inf))) - float(h) == u


@pytest.mark.parametrize("pro", K.ALL_PROS)
def test_fp64_reference_is_the_fp32_contract_on_benign_data(pro):
    B, C, L = 2, 9, 257
    case = K.benign_case(pro, B, C, L)
    x, kw = case["x"], dict(case["kw"])
    if pro in P.NORM_PROS:
        kw["stats"] = R.colnorm_stats(x) if pro == R.PRO_COLNORM else R.instnorm_stats(x)
    ref = P.activate64(x, **kw)
    c32 = P.activate32(x, **kw)
    assert ref.dtype == torch.float64 and c32.dtype == torch.float32 and ref.shape == c32.shape == (B, C, L)
    e = (c32.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    assert e < 1e-6, e  # a handful of fp32 roundings of O(1) values
    if pro in P.SNAKE_PROS:  # the one deliberate difference: the sine's argument is the fp32 product
        a = kw["alpha"].double().view(1, -1, 1)
        u = x.double() if pro == R.PRO_SNAKE else R.activate(x.double(), pro=R.PRO_ADAIN_LEAKY, slope=1.0, stats=kw["stats"].double(),
                                                             gamma=kw["gamma"].double(), beta=kw["beta"].double())
        plain64 = u + (1.0 / a) * torch.sin(a * u) ** 2
        assert 0.0 < (plain64 - ref).abs().max().item() < 1e-6
    lens = (0, 1) if B == 2 else None
    z = P.activate64(x, lengths=lens, **kw)
    assert bool((z[0] == 0).all()) and bool((z[1, :, 1:] == 0).all()) and torch.equal(z[1, :, :1], ref[1, :, :1])


def test_split_case_list_covers_what_it_claims():
    """The lists of _prologue_cases.py are curated by hand; this keeps an edit from quietly dropping an edge."""
    rows = {k: np.array([K.f32(v) for v in vals], dtype=np.float32) for k, vals in K.SPLIT_ROWS.items()}
    for k, vals in K.SPLIT_ROWS.items():  # the named values ARE fp32 numbers (the other rows are rounded to fp32 by split_tensor)
        if k not in ("above_top", "ordinary", "f32_subnormal", "huge", "lo_subnormal"):
            assert all(float(np.float32(v)) == v or v != v for v in vals), k
    assert set(rows["zeros"].tolist()) == {0.0} and bool(np.signbit(rows["zeros"]).any()) and not bool(np.signbit(rows["zeros"]).all())
    assert bool(((rows["f32_subnormal"] > 0) & (rows["f32_subnormal"] < 2.0 ** -126)).all())
    assert {2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14} <= set(rows["tiny_pow2"].astype(np.float64).tolist())
    for name, up in (("ties_even", False), ("ties_odd", True)):
        v = rows[name].astype(np.float64)
        h = v.astype(np.float16)
        below = np.where(h.astype(np.float64) > v, np.nextafter(h, np.float16(0)), h).astype(np.float16)
        above = np.nextafter(below, np.float16(np.inf)).astype(np.float64)
        assert bool((v - below.astype(np.float64) == above - v).all()) and bool((above > v).all()), name  # exactly midway
        assert bool(((h.astype(np.float64) > v) == up).all()), name                  # parity of the lower neighbour
        assert bool((h.view(np.uint16) & 1 == 0).all())                              # round-to-nearest-EVEN
        assert bool((v < 2.0 ** -14).any()) and bool((v > 2.0 ** 15).any()) and bool((v == v.astype(np.float32)).all())
    hi, lo, sat = P.split_f16(rows["lo_subnormal"])
    assert bool(((np.abs(lo.astype(np.float64)) < 2.0 ** -14) & (lo != 0)).all()) and not bool(sat.any())
    frac = rows["lo_subnormal"].astype(np.float64) - hi.astype(np.float64)
    assert bool((np.mod(np.abs(frac) * 2.0 ** 24, 1.0) == 0.5).any()), "a tie on the subnormal grid of lo"
    top = rows["top"].astype(np.float64).tolist()
    assert 65504.0 in top and 65488.0 in top and any(65503.9 < t < 65504.0 for t in top)
    above = rows["above_top"].astype(np.float64).tolist()
    assert min(above) == float(np.nextafter(np.float32(65504.0), np.float32(np.inf))) and 65520.0 in above
    assert any(65519.0 < t < 65520.0 for t in above)
    assert 1.0e6 in rows["huge"].tolist() and bool(np.isinf(rows["inf"]).all()) and bool(np.isnan(rows["nan"]).all())
    # cases: status expected exactly where a case holds an out-of-range element or a NaN (PRO_NONE: the device value is x itself)
    for case in K.SPLIT_CASES:
        x = K.split_tensor(case)
        assert x.shape[0] == 2 and x.shape[1] % 8 != 0 and x.shape[1] <= 72 and x.shape[2] <= 600
        sat = P.split_f16(x.numpy())[2]
        assert bool(sat.any()) == (case != "in_range"), case
        if case == "inf":
            assert bool((x == K.INF).any()) and bool((x == -K.INF).any())
        for C in (24, 40, 72):  # the fused routes' copies hold every row
            assert len(K.SPLIT_CASES[case]) <= C and K.split_tensor(case, C, 600).shape == (2, C, 600)
    both = K.split_tensor("in_range")
    assert bool((both[0] > 0).any()) and bool((both[1] < 0).any()) and bool((both == -65504.0).any())


def _ratio(row):
    """|mean| / std of a row in fp64 (inf for a constant one)."""
    r = row.double()
    s = r.std(unbiased=False).item()
    return math.inf if s == 0 else abs(r.mean().item()) / s


def test_hard_rows_are_what_their_comments_say():
    case = K.adain_case(True)
    x, kw = case["x"], case["kw"]
    assert x.shape == (2, K.ADAIN_C, 257)
    st = R.instnorm_stats(x)
    for c in range(K.ADAIN_C):
        name, ga, be, claim = K.ADAIN_ROWS[c % len(K.ADAIN_ROWS)]
        assert float(kw["gamma"][0, c]) == np.float32(ga) and float(kw["beta"][1, c]) == np.float32(be)
        if claim is not None:
            for b in range(2):
                assert claim[0] <= _ratio(x[b, c]) <= claim[1], (name, _ratio(x[b, c]))
        if name == "constant":
            assert abs(st[0, c, 1].item() - 1.0 / math.sqrt(1e-5)) < 1e-2
    assert {n for n, *_ in K.ADAIN_ROWS} >= {"offset", "constant", "g_zero"}
    assert dict((n, g) for n, g, *_ in K.ADAIN_ROWS)["g_zero"] == -1.0
    # every (row, alpha) pair is a channel; g = 30 under alpha = 30 reaches |alpha u| = 1e3
    pairs = {(c % len(K.ADAIN_ROWS), float(kw["alpha"][c])) for c in range(K.ADAIN_C)}
    assert len(pairs) == K.ADAIN_C
    aff = R.activate(x.double(), pro=R.PRO_ADAIN_LEAKY, slope=1.0, stats=st.double(), gamma=kw["gamma"].double(), beta=kw["beta"].double())
    au = (aff * kw["alpha"].double().view(1, -1, 1)).abs().amax(dim=(0, 2))
    c = [i for i in range(K.ADAIN_C) if K.ADAIN_ROWS[i % 6][0] == "gain_30" and float(kw["alpha"][i]) == 30.0][0]
    assert 1e3 < au[c].item() < 1e4
    gz = [i for i in range(K.ADAIN_C) if K.ADAIN_ROWS[i % 6][0] == "g_zero"]
    assert bool((aff[:, gz] == 0.625).all())

    case = K.snake_case()
    x, alpha = case["x"], case["kw"]["alpha"]
    reaches, alphas = set(), set()
    for c, (a, kind, reach) in enumerate(K.SNAKE_ROWS):
        assert float(alpha[c]) == np.float32(a)
        au = (x[:, c] * alpha[c]).abs()  # the fp32 product the kernels form
        if kind == "range":
            assert 0.999 * reach <= au.max().item() <= 1.001 * reach, (a, reach, au.max().item())
            reaches.add(reach)
            alphas.add(a)
        else:  # on / halfway between multiples of pi, to the rounding of u and of the product
            ph = (x[:, c].double() * float(alpha[c]) / math.pi) - (0.5 if kind == "half" else 0.0)
            assert (ph - ph.round()).abs().max().item() < 1e-4 and ph[0].round().unique().numel() == 257
    assert {1e2, 1e3, 1e4} <= reaches and {0.01, 0.1, 1.0, 30.0} <= alphas and min(alphas) < 0
    for a in (1.0, 30.0, 0.1):
        assert {k for aa, k, _ in K.SNAKE_ROWS if aa == a} == {"range", "pi", "half"}

    assert set(K.LEAKY_SLOPES) == {0.0, 0.01, 0.2}
    x = K.leaky_case(0.2)["x"]
    assert x[:, 0].max().item() <= -1e3 and x[:, 0].min().item() == -6e4 and x[:, 1].min().item() == -6e4
    assert x[:, 2].abs().max().item() < 1e-5 and x[:, 4].max().item() <= 0

    for seg in K.colnorm_segs(257):
        case = K.colnorm_case(gb_seg=seg)
        x, kw = case["x"], case["kw"]
        G = kw["gamma"].shape[0]
        assert x.shape[0] == 1 and G == -(-257 // seg) and kw["beta"].shape == kw["gamma"].shape
        if G > 1:  # a neighbour's row is a different affine in every channel
            assert (kw["gamma"][1:] - kw["gamma"][:-1]).abs().min().item() > 1.0
            assert (kw["beta"][1:] - kw["beta"][:-1]).abs().min().item() > 1.0
        cols = x[0].double()
        r = cols.mean(0).abs() / cols.std(0, unbiased=False)
        assert 500 < r[3].item() < 2000 and 500 < r[20].item() < 2000 and cols.std(0, unbiased=False)[5].item() == 0
    assert set(K.colnorm_segs(257)) == {1, 61, 257}
    assert set(K.SHAPE_L) == {1, 255, 256, 257, 513} and set(K.SHAPE_C) == {1, 7, 8, 9, 33, 72}
    assert sorted({n for bt in K.length_batches(257) for n in bt}) == [0, 1, 257, 262] and all(len(bt) == 3 for bt in K.length_batches(257))


def _all_cases():
    out = []
    for C in (None, 24, 40, 72):
        L = 257 if C is None else 600
        out += [("%s_C%s" % (n, C), c) for n, c in K.hard_cases(C, L).items()]
    for seg in K.colnorm_segs(257):
        out.append(("colnorm_seg%d" % seg, K.colnorm_case(gb_seg=seg, gamma_plus_one=True)))
    for pro in K.ALL_PROS:
        for C, L in ((1, 1), (72, 513), (9, 257)):
            out.append(("benign_p%d_%d_%d" % (pro, C, L), K.benign_case(pro, 2, C, L)))
    return out


def test_no_case_sits_at_the_clamp_and_none_uses_alpha_zero():
    """Only the deliberately saturating rows of section 2 may clamp: every other reference value stays 1e-3 (relative) clear of
    65504 / x_scale, so no case's verdict hangs on which side of the clamp a rounding fell.  alpha = 0 is 0 * inf = NaN in the
    reference model too: out of scope, and no case uses it."""
    for name, case in _all_cases():
        x, kw = case["x"], dict(case["kw"])
        assert x.shape[0] <= 3 and x.shape[1] <= 72 and x.shape[2] <= 600, name
        if kw["pro"] in P.NORM_PROS:
            kw["stats"] = R.colnorm_stats(x) if kw["pro"] == R.PRO_COLNORM else R.instnorm_stats(x)
        if "alpha" in kw:
            assert bool((kw["alpha"] != 0).all()) and bool(torch.isfinite(1.0 / kw["alpha"]).all()), name
        ref = P.activate64(x, **kw)
        assert bool(torch.isfinite(ref).all()), name
        assert ref.abs().max().item() < (1.0 - 1e-3) * K.F16_MAX / P.x_scale_for(kw["pro"]), (name, ref.abs().max().item())
    x = K.split_tensor("in_range")
    assert x.abs().max().item() == K.F16_MAX  # the one in-range case AT the top, on purpose: 65504 itself must not raise the bit
    for act in (R.ACT_GELU, R.ACT_GELU_TANH, R.ACT_TANH, R.ACT_LEAKY, R.ACT_EXP_SIN):
        for C in (32, 40):
            assert K.epilogue_args(act, C).abs().max().item() < (1.0 - 1e-3) * K.F16_MAX


def test_epilogue_arguments_cover_what_they_claim():
    for C in (32, 40):
        sp = K.epilogue_split(C)
        assert 0 < sp < C - 8 and sp % 8 != 0
        for act, mags in K.EPI_MAGS.items():
            x = K.epilogue_args(act, C)
            assert x.shape == (2, C, K.EPI_L) and K.EPI_L % 32 not in (0,) and K.EPI_L > 128
            for c in range(C):
                m = mags[c % len(mags)]
                assert abs(x[0, c, 0].item()) == np.float32(m) and 0.94 * m < x[:, c].abs().min().item() and x[:, c].abs().max().item() < 1.06 * m
                assert bool((x[:, c] < 0).any()) and (act == R.ACT_LEAKY) == (not bool((x[:, c] > 0).any()))
        assert set(K.EPI_MAGS[R.ACT_GELU]) == set(K.EPI_MAGS[R.ACT_GELU_TANH]) == {1e-4, 1.0, 6.0, 10.0}
        assert set(K.EPI_MAGS[R.ACT_TANH]) == {1e-4, 9.0, 20.0}
        x = K.epilogue_args(R.ACT_EXP_SIN, C)
        assert x[:, :sp].min().item() == -80.0 and x[:, :sp].max().item() == 80.0
        seen = set()
        for c in range(sp, C):
            reach = K.EPI_SIN[(c // 2) % len(K.EPI_SIN)]
            ph = x[:, c].double() / math.pi - (0.5 if c % 2 else 0.0)
            assert (ph - ph.round()).abs().max().item() < 2e-4  # half an fp32 ulp of 1e4 rad, in units of pi
            assert 0.6 * reach < x[:, c].abs().max().item() <= reach, (c, reach, x[:, c].abs().max().item())
            seen.add((reach, c % 2))
        assert seen == {(r, p) for r in K.EPI_SIN for p in (0, 1)}
