"""The look-ahead limiter of the hand-over on the device: `st2_wave_limit` against the fp64 contract of
tests/_limit_ref.py.

Rows.  `_rows(W)` states them by sample count and by where their over-ceiling samples sit, in units of W and of the kernel's
tile (`ops.LIMIT_TILE`).  The counts are met exactly at one sample per frame; at 5 and 600 samples per frame with a trim of 0 or
3 only spf f - trim can be had, so there every row takes the nearest count at or above its own that the capacity allows and
keeps the events that still fall inside it -- the tile edges 2047 / 2048 / 2049 and 4095 / 4096 / 4097 are inside a row of 4 800.

Bounds, all derived here from the reference: limit[b][0] to one fp32 ulp of rule 1; everything behind it is the contract over the
REPORTED g' (the check of each stage is about that stage).  r (read from the head of the workspace) to one fp32 ulp; m bit for
bit through a window that is 1 at its centre (then q = fl32(1 - fl32(1 - m)), no sum); out to (2 W + 6) 2^-24 |x g'|.  With the
table the fp32 interpolation may be off by (K + 1) 2^-24 sum |taps x| per value: r, m, s and q are monotone in the envelope, so
the device's q lies between the contract's q of the two extreme envelopes, and out between their products, plus the bound."""
import functools

import numpy as np
import pytest
import torch

import _level_ref as R
import _limit_ref as LR
import _truepeak_ref as TP
from styletts2_amd import ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = ops.LIMIT_TILE
CEILING, MAX_GAIN_DB, DRIVE_DB = 10.0 ** (-1.0 / 20.0), 60.0, 6.0
GEOMETRIES = [(5, 8, 0), (5, 8, 3), (600, 8, 0), (600, 8, 3), (1, 4800, 0)]  # (samples per frame, T_cap, trim)
SENTINEL = 7.25
NAN_PAYLOAD = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)


def _rows(W):
    """[(name, n, [over-ceiling positions], target)] -- 17 rows; a position of -1 is the row's last sample."""
    big = 4800
    return [("empty", 0, [], 0.0), ("short", max(1, W - 1), [0], 0.0), ("n=2W", 2 * W, [W], 0.0), ("n=2W+1", 2 * W + 1, [0, -1], 0.0),
            ("n=T-1", T - 1, [0, -1], 0.0), ("n=T", T, [0, T - 1], 0.0), ("n=T+1", T + 1, [T - 1, T], 0.0),
            ("edges", big, [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1], 0.0),
            ("pairs", big, [1000, 1000 + 2 * W, 3000, 3000 + 2 * W + 1], 0.0), ("all over", 2500, "all", 0.0),
            ("under", 2500, [700], -60.0), ("non-finite", 2100, [100], 0.0), ("nan target", 2100, [50], float("nan")),
            ("group a", 2300, [2047], -10.0), ("group b", 900, [5], float("nan")), ("group c", big, [4096], -60.0),
            ("speech", big, "speech", 0.0)]


GROUP_START = [1] * 13 + [1, 0, 0, 1]
SUBSET = [7, 0, 12, 3, 9]  # B = 5: rows of the 17 in another order


def _content(name, n, over, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 0.02).astype(np.float32)
    if isinstance(over, str) and over == "all":
        # a 1 kHz square: at the target of 0 LUFS its flat tops stand at about 1.0, over the ceiling of 0.89 from end to end
        x = (0.5 * np.where(np.arange(n) % 24 < 12, 1.0, -1.0) * (1.0 - 0.01 * g.random(n))).astype(np.float32)
        x[n // 3] = 0.5
    elif isinstance(over, str):  # bursts of a decaying 180 Hz pulse train: a crest factor like a voice's
        t = np.arange(n)
        x += (0.5 * np.exp(-(t % 133) / 20.0) * np.sin(2 * np.pi * 700.0 * t / 24000.0) * (t % 1600 < 1100)).astype(np.float32)
    else:
        for k, i in enumerate(i for i in over if -n <= i < n):
            x[i] = (0.5 if k == 0 else 0.35 + 0.02 * k) * (-1.0 if k % 2 else 1.0)
    if name == "non-finite" and n > 6:
        x[5], x[n // 2], x[n - 2] = np.nan, np.inf, -np.inf
        if n > T:
            x[T - 1], x[T] = np.inf, np.nan
    if name == "nan target":
        x[:min(4, n)] = NAN_PAYLOAD[:min(4, n)]
    return x


@functools.lru_cache(maxsize=None)
def _case(geo, W, rows=None):
    """The batch of a geometry and a W on the host: (wave fp32 [B, stride] with the sentinel behind every n_b, n, frames, targets)."""
    spf, T_cap, trim = geo
    spec = _rows(W)
    spec = spec if rows is None else [spec[i] for i in rows]
    cap = spf * T_cap
    host = np.full((len(spec), cap + 24), np.float32(SENTINEL))
    n, frames = [], []
    for b, (name, want, over, _) in enumerate(spec):
        f = 0 if want == 0 else min(T_cap, -(-(want + trim) // spf))
        n_b = max(0, spf * f - trim)
        host[b, :n_b] = _content(name, n_b, over, 1000 + sum(map(ord, name)))
        n.append(n_b)
        frames.append(f)
    host.setflags(write=False)
    return host, tuple(n), tuple(frames), tuple(np.float32(s[3]) for s in spec)


@functools.lru_cache(maxsize=None)
def _envelope(geo, W, b, true_peak):
    host, n, _, _ = _case(geo, W)
    return LR.envelope(host[b, :n[b]], TP.table()[2] if true_peak else None)


def _run(geo, W, true_peak, rows=None, starts=None, win=None):
    """One measurement and one limiter call -> dict of host arrays: level, out (with its sentinel margin), limit, r."""
    spf, T_cap, trim = geo
    host, n, frames, targets = _case(geo, W, rows)
    B, cap = len(n), spf * T_cap
    wave = torch.from_numpy(np.array(host)).to(DEV)[:, :cap]
    fr = torch.tensor(frames, dtype=torch.int32, device=DEV)
    tg = torch.tensor(targets, dtype=torch.float32, device=DEV)
    more = {}
    if true_peak:
        more["true_peak"] = resample.true_peak_table(DEV)
    if starts is not None:
        more["starts"] = torch.tensor(starts, dtype=torch.int32, device=DEV)
    level = ops.wave_level(wave, fr, tg, ceiling=CEILING, max_gain_db=MAX_GAIN_DB, trim=trim, samples_per_frame=spf, **more)
    before = level.clone()
    out = torch.full((B, cap + 24), SENTINEL, device=DEV)
    work = torch.zeros((ops.wave_limit_workspace_bytes(B, T_cap, spf),), dtype=torch.uint8, device=DEV)
    win = resample.limit_window(W, DEV) if win is None else win
    o, lim = ops.wave_limit(wave, fr, level, tg, win, ceiling=CEILING, max_gain_db=MAX_GAIN_DB, drive_db=DRIVE_DB, trim=trim,
                            samples_per_frame=spf, out=out[:, :cap], workspace=work, **more)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and torch.equal(level, before), "the level table is not modified"
    return dict(level=level.cpu().numpy(), out=out.cpu().numpy(), limit=lim.cpu().numpy(),
                r=work.view(torch.float32)[:B * cap].view(B, cap).cpu().numpy(), host=host, n=n, targets=targets)


@functools.lru_cache(maxsize=None)
def _cached(geo, W, true_peak):
    return _run(geo, W, true_peak, starts=tuple(GROUP_START))


def _check(got, geo, W, true_peak, win, starts, idx=None):
    """Every row of a run against the contract."""
    host, n, targets = got["host"], got["n"], got["targets"]
    tg = LR.groups_target(list(targets), starts)
    cap = geo[0] * geo[1]
    for b, n_b in enumerate(n):
        x, out = host[b, :n_b], got["out"][b]
        assert (out[n_b:] == np.float32(SENTINEL)).all(), (b, "nothing at or past n_b is written")
        g_ref = LR.drive_gain(got["level"][b, 0], got["level"][b, 1], tg[b], CEILING, MAX_GAIN_DB, DRIVE_DB)
        if g_ref is None:
            assert out[:n_b].tobytes() == x.tobytes() and got["limit"][b].tolist() == [1.0, 1.0], (b, "left alone: a bit copy")
            continue
        g = got["limit"][b, 0]
        assert abs(float(g) - float(g_ref)) <= float(np.spacing(g_ref)), (b, g, g_ref)
        if n_b == 0:
            assert got["limit"][b, 1] == 1.0
            continue
        e, e_bound = _envelope(geo, W, b if idx is None else idx[b], true_peak)
        r = LR.required(e, CEILING, g)
        m = LR.hold(r, W)
        s = LR.smooth(m, win, W, n_b)
        ref = dict(r=r, e=e, e_bound=e_bound, q=np.minimum(s, r.astype(np.float64)), xg=TP.clean32(x) * g)
        bound = LR.bound(ref, W)
        axg = np.abs(ref["xg"].astype(np.float64))
        q_lo, q_hi = LR.q_interval(ref, g, CEILING, W, win) if true_peak else (ref["q"], ref["q"])
        r_lo = LR.required(e + e_bound, CEILING, g)
        r_hi = LR.required(np.maximum(e - e_bound, 0.0), CEILING, g)
        dev_r = got["r"][b, :n_b]
        assert (dev_r >= r_lo - np.spacing(r_lo)).all() and (dev_r <= r_hi + np.spacing(r_hi)).all(), (b, "r")
        dev = out[:n_b].astype(np.float64)
        assert ((np.abs(dev) <= bound) | (np.sign(dev) == np.sign(ref["xg"]))).all(), (b, "sign")
        lo, hi = axg * q_lo - bound, axg * q_hi + bound
        worst = float(np.max(np.maximum(lo - np.abs(dev), np.abs(dev) - hi)))
        print("spf %d trim %d W %3d tp %d row %2d n %5d: g' %.6f min q %.6f  out past its interval by %.3e (bound up to %.3e)" % (
            geo[0], geo[2], W, true_peak, b, n_b, g, got["limit"][b, 1], worst, float(bound.max())))
        assert worst <= 0.0, (b, worst)
        assert (np.abs(dev) <= CEILING * (1 + 2.0 ** -21)).all(), (b, float(np.abs(dev).max()))
        slack = (2 * W + 4) * 2.0 ** -24
        assert q_lo.min() - slack <= float(got["limit"][b, 1]) <= q_hi.min() + slack, (b, got["limit"][b], q_lo.min(), q_hi.min())


@pytest.mark.parametrize("W", [1, 7, 192])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "spf%d-trim%d" % (g[0], g[2]))
def test_sample_peak_rows_against_the_contract(geo, W):
    got = _cached(geo, W, False)
    _check(got, geo, W, False, LR.window(W), GROUP_START)
    spec = [s[0] for s in _rows(W)]
    a = spec.index("group a")
    assert got["limit"][a + 1, 0] == got["limit"][a, 0] == got["limit"][a + 2, 0] != 1.0, "the group's first target decides"
    assert got["limit"][spec.index("under"), 1] == 1.0, "a row under the ceiling is multiplied by g' alone"
    if geo[0] * geo[1] >= 2500:
        b = spec.index("all over")
        assert (got["r"][b, :got["n"][b]] < 1.0).all() and got["limit"][b, 1] < 0.99,"a whole row over the ceiling is turned down as a whole"
    assert ops.status() == 0


@pytest.mark.parametrize("W", [1, 7, 192])
@pytest.mark.parametrize("geo", [GEOMETRIES[0], GEOMETRIES[3], GEOMETRIES[4]], ids=lambda g: "spf%d-trim%d" % (g[0], g[2]))
def test_true_peak_rows_against_the_contract(geo, W):
    got = _cached(geo, W, True)
    _check(got, geo, W, True, LR.window(W), GROUP_START)
    plain = _cached(geo, W, False)
    assert (got["r"] <= plain["r"])[[b for b, n_b in enumerate(got["n"]) if n_b and got["limit"][b, 0] == plain["limit"][b, 0]]].all()
    assert ops.status() == 0


@pytest.mark.parametrize("W", [1, 7, 192])
def test_the_hold_bit_for_bit_through_a_window_of_one_weight(W):
    geo = GEOMETRIES[4]
    delta = np.zeros(2 * W + 1, dtype=np.float32)
    delta[W] = 1.0
    got = _run(geo, W, False, starts=GROUP_START, win=torch.from_numpy(delta).to(DEV))
    host, n = got["host"], got["n"]
    for b, n_b in enumerate(n):
        if n_b == 0 or got["limit"][b].tolist() == [1.0, 1.0] and np.isnan(got["targets"][b]):
            continue
        g = got["limit"][b, 0]
        r = got["r"][b, :n_b]
        assert r.tobytes() == LR.required(_envelope(geo, W, b, False)[0], CEILING, g).tobytes(), (b, "r is rule 3's one rounding")
        m = LR.hold(r, W)[W:W + n_b]
        q = np.minimum(np.float32(1.0) - (np.float32(1.0) - m), r)
        want = (TP.clean32(host[b, :n_b]) * g) * q
        assert got["out"][b, :n_b].tobytes() == want.astype(np.float32).tobytes(), b
        assert got["limit"][b, 1].tobytes() == q.min().tobytes(), b


@pytest.mark.parametrize("true_peak", [False, True], ids=["sample", "true"])
@pytest.mark.parametrize("W", [7, 192])
def test_a_row_does_not_depend_on_its_place_in_the_batch(W, true_peak):
    geo = GEOMETRIES[3]
    full = _cached(geo, W, true_peak)
    for rows in (tuple(SUBSET), (7,)):
        got = _run(geo, W, true_peak, rows=rows)
        for b, i in enumerate(rows):
            n_b = got["n"][b]
            assert n_b == full["n"][i] and got["out"][b].tobytes() == full["out"][i].tobytes(), (rows, b)
            assert got["limit"][b].tobytes() == full["limit"][i].tobytes() and got["r"][b, :n_b].tobytes() == full["r"][i, :n_b].tobytes()
        _check(got, geo, W, true_peak, LR.window(W), None, idx=rows)
    assert ops.status() == 0


def test_a_row_that_needed_the_ceiling_reaches_its_target_within_the_drive():
    """The rows' targets are set 4 dB above what the ceiling lets a plain `Level` reach (less than the drive of 6 dB, so rule 1's
    target term decides): the limiter's q is never below c / (peak g') = -4 dB, so the limited row is at least as loud as the
    plain one, and it misses the target by what the limiter took, at most those 4 dB."""
    geo, W = GEOMETRIES[2], 192
    spf, T_cap, trim = geo
    host, n, frames, _ = _case(geo, W, (16, 8))  # the speech-like row and the row of lone peaks
    B, cap = len(n), spf * T_cap
    wave = torch.from_numpy(np.array(host)).to(DEV)[:, :cap]
    fr = torch.tensor(frames, dtype=torch.int32, device=DEV)
    leave = torch.full((B,), float("nan"), device=DEV)
    first = ops.wave_level(wave, fr, leave, trim=trim, samples_per_frame=spf).cpu().numpy()
    target = (first[:, 0] + 20.0 * np.log10(CEILING / first[:, 1]) + 4.0).astype(np.float32)
    tg = torch.from_numpy(target).to(DEV)
    level = ops.wave_level(wave, fr, tg, ceiling=CEILING, max_gain_db=MAX_GAIN_DB, trim=trim, samples_per_frame=spf)
    lv = level.cpu().numpy()
    assert (lv[:, 2] == np.float32(CEILING / lv[:, 1].astype(np.float64))).all(), "the ceiling decided under the plain Level"
    limited, lim = ops.wave_limit(wave, fr, level, tg, resample.limit_window(W, DEV), ceiling=CEILING, max_gain_db=MAX_GAIN_DB,
                                  drive_db=DRIVE_DB, trim=trim, samples_per_frame=spf)
    plain = wave * level[:, 2:3]
    L_plain = ops.wave_level(plain.contiguous(), fr, leave, trim=trim, samples_per_frame=spf).cpu().numpy()[:, 0]
    L_lim = ops.wave_level(limited, fr, leave, trim=trim, samples_per_frame=spf).cpu().numpy()[:, 0]
    for b in range(B):
        print("row %d: L %.2f as measured, %.2f under the plain Level, %.2f behind the limiter (target %.1f, drive %.1f dB), min q %.4f"
              % (b, lv[b, 0], L_plain[b], L_lim[b], target[b], DRIVE_DB, lim[b, 1].item()))
        assert L_lim[b] >= L_plain[b] and abs(L_lim[b] - target[b]) <= DRIVE_DB
    assert ops.status() == 0


# ---- the true peak of the limited output -----------------------------------------------------------------------------------------
def clips(n=4800):
    """The three clips of DESIGN.md section 27's overshoot figure, each peaking 6 dB over the ceiling before the limiter."""
    t = np.arange(n)
    g = np.random.default_rng(27)
    sine = np.sin(2 * np.pi * t / 4.0 + np.pi / 4.0)  # fs / 4, sampled 45 degrees off its crests
    burst = np.exp(-(t % 133) / 20.0) * np.sin(2 * np.pi * 700.0 * t / 24000.0) * (t % 1600 < 1100) + 0.01 * g.standard_normal(n)
    noise = g.standard_normal(n)
    return {k: (v / np.abs(v).max()).astype(np.float32) for k, v in (("sine", sine), ("burst", burst), ("noise", noise))}


def overshoot(x, W, out32):
    """The true peak of a limited row over the ceiling, as a ratio."""
    return TP.true_peak(out32, TP.table()[2])[0] / CEILING


def test_true_peak_of_the_limited_output_stays_within_the_contracts_overshoot():
    W, spf, T_cap = 192, 600, 8
    U, K, taps = TP.table()
    win = LR.window(W)
    names = sorted(clips())
    host = np.stack([clips()[k] for k in names])
    wave = torch.from_numpy(host).to(DEV)
    fr = torch.full((3,), T_cap, dtype=torch.int32, device=DEV)
    tg = torch.zeros((3,), device=DEV)  # 0 LUFS and 60 dB: the noise and the burst go in 6 dB over the ceiling, the sine 3 dB
    tp = resample.true_peak_table(DEV)
    level = ops.wave_level(wave, fr, tg, ceiling=CEILING, max_gain_db=MAX_GAIN_DB, samples_per_frame=spf, true_peak=tp)
    out, lim = ops.wave_limit(wave, fr, level, tg, resample.limit_window(W, DEV), ceiling=CEILING, max_gain_db=MAX_GAIN_DB,
                              drive_db=DRIVE_DB, samples_per_frame=spf, true_peak=tp)
    out, lim = out.cpu().numpy(), lim.cpu().numpy()
    gain = float(np.abs(taps.astype(np.float64)).sum(axis=1).max())  # what the interpolation can make of a per-sample error
    for b, name in enumerate(names):
        ref = LR.limit_row(host[b], lim[b, 0], CEILING, W, win, taps)
        q_lo, q_hi = LR.q_interval(ref, lim[b, 0], CEILING, W, win)
        err = float((np.abs(ref["xg"]) * (q_hi - q_lo) + LR.bound(ref, W)).max())
        over_ref, over_dev = overshoot(host[b], W, ref["out"].astype(np.float32)), overshoot(host[b], W, out[b])
        print("%-5s: true peak / ceiling - 1: contract %+.3e, device %+.3e; allowed on top %.2e; min q %.4f" % (
            name, over_ref - 1.0, over_dev - 1.0, gain * err / CEILING, lim[b, 1]))
        assert over_dev <= over_ref + gain * err / CEILING, name
        assert np.abs(out[b]).max() <= CEILING * (1 + 2.0 ** -21)
    assert ops.status() == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_end_to_end_packed_bytes_and_one_graph_for_any_targets():
    """The packed bytes of a limiting call are the parent's pack entry over the limited rows, where the limited rows are
    `ops.wave_limit`'s (held to the contract above) -- a 16-bit code of two values one fp32 rounding apart may differ, so the bytes
    are compared through the device's rows, and the 24 kHz codes are also held to one code of the contract's rows."""
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    Tf, N = P["T"], b["tokens"].shape[1]
    ld = b["lengths"].to(torch.int32).to(DEV)
    feed = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    W = 192
    win = resample.limit_window(W, DEV)
    for pack, rate, gaps in (("s16", None, None), ("ulaw", 8000, [80, 0, 160, 40])):
        lvl = pipeline.Level(K, target=-14.0, limiter=True, true_peak=pack == "ulaw")
        build = dict(ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, pack=pack, sample_rate=rate)
        if gaps is not None:
            build.update(passage=True, max_gap=200)
        gs = pipeline.GraphedSynthesis(model, sampler, K, N, Tf, STEPS, level=lvl, **build)
        for targets in (None, [-20.0, -12.0, None, -16.0]):
            call = dict(feed) if targets is None else dict(level=targets)
            if gaps is not None:
                call["gaps"] = gaps
            res = gs(**call)
            rows, lv, lim = res.to_host(level=True, limit=True)
            rows, lv, lim = [r.copy() for r in rows], lv.copy(), lim.copy()
            spf = res.wave.shape[-1] // Tf
            st = gs.static["level"]
            more = dict(true_peak=resample.true_peak_table(DEV)) if st.true_peak else {}
            level = ops.wave_level(res.wave, res.frames, st.target, ceiling=st.ceiling, max_gain_db=st.max_gain_db, trim=P["trim"],
                                   samples_per_frame=spf, **more)
            limited, limit = ops.wave_limit(res.wave, res.frames, level, st.target, win, ceiling=st.ceiling, max_gain_db=st.max_gain_db,
                                            drive_db=st.drive_db, trim=P["trim"], samples_per_frame=spf, **more)
            assert level.cpu().numpy().tobytes() == lv.tobytes() and limit.cpu().numpy().tobytes() == lim.tobytes()
            if gaps is None:
                packed, offs = ops.wave_pack(limited, res.frames, trim=P["trim"], fmt=pack, samples_per_frame=spf)
            else:
                packed, offs = ops.wave_pack_gaps(limited, res.frames, torch.tensor(gaps, dtype=torch.int32, device=DEV), 200, rate=rate,
                                                  fmt=pack, trim=P["trim"], samples_per_frame=spf)
            o = offs.cpu().tolist()
            assert o == res.offsets.cpu().tolist()
            assert packed[:o[-1]].cpu().numpy().tobytes() == res.packed[:o[-1]].cpu().numpy().tobytes(), (pack, targets)
            if targets is not None:
                assert np.isnan(st.target.cpu().numpy()[2]) and lim[2].tolist() == [1.0, 1.0]
            if gaps is None:  # against the contract's rows, to one 16-bit code
                w = res.wave[:, 0].cpu().numpy()
                fr = res.frames.cpu().tolist()
                refs, _ = LR.wave_limit(w, [max(0, spf * f - P["trim"]) for f in fr], lv, st.target.cpu().numpy(), st.ceiling,
                                        st.max_gain_db, st.drive_db, W, LR.window(W))
                for k, ref in enumerate(refs):
                    if ref is not None:
                        want = np.rint(np.clip(ref["out"], -1, 1) * 32767.0)
                        assert np.abs(rows[k].astype(np.float64) - want).max() <= 1.0, k
    torch.cuda.synchronize()
    ops.check_status()
