"""The true-peak ceiling and the passage scope of the level measurement on the device: `st2_wave_level_ex`
against the fp64 contracts of tests/_truepeak_ref.py and tests/_level_ref.py on the rows of tests/_truepeak_cases.py.

The reported peak is held to the interval the fp32 chain's derived bound allows (`_resample_ref.polyphase`'s (K + 1) 2^-24 sum
|taps x| per output) joined with the exact sample peak; L and the block count are, bit for bit, what `st2_wave_level` gives for
the same rows; the gain is the contract's formula over the REPORTED fp32 peak, to one fp32 ulp and section 23's loudness bound,
and where the ceiling binds it is fl32(ceiling / reported peak) itself -- the formula's one rounding to fp32, the format of g_b,
is to nearest, so that is the reading of "g_b <= ceiling / level[b][1] exactly" the test holds the kernel to: equality with the
quotient in fp32.  Geometry: 24 kHz, rows of 72 000 samples, B = 8, a row stride larger than the row, NaN bit patterns behind every
n_b.  The true-peak launch tiles a row by hops (2 400 samples) and a lane passes twice over a hop (1 280 positions a pass): the
two burst rows sit on a hop boundary, and on a hop boundary and a pass boundary."""
import functools

import numpy as np
import pytest
import torch

import _level_ref as R
import _resample_ref as RR
import _truepeak_cases as TC
import _truepeak_ref as TP
from styletts2_amd import ops, pipeline, resample
from test_truepeak_cpu import ripple

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIDE = TC.ROW + 608


def _batch(names, spf, trim, targets=None):
    B = len(names)
    host = np.full((B, STRIDE), np.nan, dtype=np.float32)
    for b, name in enumerate(names):
        n_b = TC.samples_of(name, spf, trim)
        host[b, :n_b] = TC.content()[name][0][:n_b]
    wave = torch.from_numpy(host).to(DEV)[:, :TC.ROW]
    target = torch.tensor([TC.ROWS[n][1] for n in names] if targets is None else targets, dtype=torch.float32, device=DEV)
    frames = torch.tensor([TC.frames_of(n, spf, trim) for n in names], dtype=torch.int32, device=DEV)
    return wave, frames, target, host[:, :TC.ROW]


def _level(names, spf, trim, true_peak=False, starts=None, targets=None):
    wave, frames, target, _ = _batch(names, spf, trim, targets)
    more = {}
    if true_peak:
        more["true_peak"] = resample.true_peak_table(DEV)
    if starts is not None:
        more["starts"] = torch.tensor(starts, dtype=torch.int32, device=DEV)
    lv = ops.wave_level(wave, frames, target, ceiling=TC.CEILING, max_gain_db=TC.MAX_GAIN_DB, trim=trim, samples_per_frame=spf,
                        sample_rate=TC.FS, **more)
    torch.cuda.synchronize()
    assert lv.dtype == torch.float32 and tuple(lv.shape) == (len(names), 4)
    got = lv.cpu().numpy()
    got.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def _cached(names, spf, trim, true_peak):
    return _level(names, spf, trim, true_peak)


def _check_gain(got, detail, target, bound_db, what):
    """(c): the contract's gain from the reported peak and the contract's L; the target term may move by the loudness bound."""
    want = R.gain(detail[4], got[1], target, TC.CEILING, TC.MAX_GAIN_DB)
    terms = TP.binding_terms(detail[4], got[1], target, TC.CEILING, TC.MAX_GAIN_DB)
    slack = float(want) * (10.0 ** (bound_db / 20.0) - 1.0) if terms[0] == min(terms) and terms[0] < np.inf else 0.0
    assert abs(float(got[2]) - float(want)) <= float(np.spacing(want)) + slack, (what, got, want)
    if terms[2] == min(terms) and terms[2] < np.inf:  # the ceiling binds: no L in it
        assert got[2].tobytes() == np.float32(TC.CEILING / float(got[1])).tobytes(), (what, got)
    if min(terms) == np.inf:
        assert got[2].tobytes() == np.float32(1.0).tobytes(), (what, got)


@pytest.mark.parametrize("spf,trim", TC.GEOMETRIES)
@pytest.mark.parametrize("names", [TC.MAIN, TC.OTHER], ids=["main", "variants"])
def test_true_peak_rows_against_the_contract(names, spf, trim):
    got, plain = _cached(names, spf, trim, True), _cached(names, spf, trim, False)
    for b, name in enumerate(names):
        d = TC.measured(name, spf, trim)
        _, detail = TC.expect_group((name,), spf, trim, True)
        print("spf %d trim %d row %-10s n %5d: peak %.8g in [%.8g, %.8g] (sample peak %.8g) L %.6f gain %.8g blocks %d" % (
            spf, trim, name, d["n"], got[b, 1], d["tp_lo"], d["tp_hi"], d["peak"], got[b, 0], got[b, 2], got[b, 3]))
        assert d["tp_lo"] <= float(got[b, 1]) <= d["tp_hi"], (name, got[b], d)  # (a)
        assert got[b, 1] >= d["peak"] and plain[b, 1].tobytes() == d["peak"].tobytes()
        assert got[b, [0, 3]].tobytes() == plain[b, [0, 3]].tobytes(), (name, got[b], plain[b])  # (b)
        _check_gain(got[b], detail, TC.ROWS[name][1], TC.loudness_bound_db(detail, d["peak"]), name)  # (c)
    for name in ("empty", "zero"):
        if name in names:
            assert got[names.index(name)].tolist() == [-np.inf, 0.0, 1.0, 0.0]
    if "sine" in names:
        s, r = got[names.index("sine")], ripple()
        assert 0.5 * np.cos(np.pi / 32) * (1 - r) - 1e-5 <= s[1] <= 0.5 * (1 + r) + 1e-5 and plain[names.index("sine"), 1] < 0.3536
        assert s[2] < plain[names.index("sine"), 2] * 0.72, "3 dB less gain than the sample-peak ceiling allowed"
    if "impulse" in names:
        assert got[names.index("impulse"), 1] == 1.0, "the sample peak wins: phase 0 reads 0.925 of a lone sample"
    assert ops.status() == 0


@pytest.mark.parametrize("spf,trim", TC.GEOMETRIES)
def test_a_row_does_not_depend_on_its_place_and_neither_argument_is_the_plain_entry(spf, trim):
    main, other = _cached(TC.MAIN, spf, trim, True), _cached(TC.OTHER, spf, trim, True)
    for name in set(TC.MAIN) & set(TC.OTHER):  # (d)
        assert main[TC.MAIN.index(name)].tobytes() == other[TC.OTHER.index(name)].tobytes(), name
    for name in ("sine", "burst_tile"):
        assert _level((name,), spf, trim, True)[0].tobytes() == main[TC.MAIN.index(name)].tobytes(), name
    # (e) taps = start = NULL through the _ex entry: st2_wave_level's bytes
    from styletts2_amd import _lib
    wave, frames, target, _ = _batch(TC.OTHER, spf, trim)
    B = len(TC.OTHER)
    work = torch.empty((ops.wave_level_workspace_bytes(B, TC.ROW // spf, spf),), dtype=torch.uint8, device=DEV)
    out = torch.full((B, 4), 7.0, device=DEV)
    _lib.check(_lib.load().st2_wave_level_ex(wave.data_ptr(), wave.stride(0), frames.data_ptr(), B, TC.ROW // spf, spf, trim, TC.FS,
                                            target.data_ptr(), TC.CEILING, TC.MAX_GAIN_DB, out.data_ptr(), work.data_ptr(),
                                            work.numel(), torch.cuda.current_stream().cuda_stream, 0, 0, 0, 0), "st2_wave_level_ex")
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == _cached(TC.OTHER, spf, trim, False).tobytes()
    # and all-ones start flags are the row scope, bit for bit, with and without the table
    for tp in (False, True):
        assert _level(TC.OTHER, spf, trim, tp, starts=TC.SINGLE_START).tobytes() == _cached(TC.OTHER, spf, trim, tp).tobytes()
    assert ops.status() == 0


@pytest.mark.parametrize("spf,trim", TC.GEOMETRIES)
@pytest.mark.parametrize("true_peak", [False, True], ids=["sample", "true"])
def test_groups_get_one_level(true_peak, spf, trim):
    names = TC.GROUP_ROWS
    got = _level(names, spf, trim, true_peak, starts=TC.GROUP_START)
    rows = _cached(names, spf, trim, true_peak)  # the same rows in the row scope
    for a, e in TP.groups(TC.GROUP_START, len(names)):
        grp = names[a:e]
        want, detail = TC.expect_group(grp, spf, trim, true_peak)
        pk = max(TC.measured(n, spf, trim)["peak"] for n in grp)
        bound = TC.loudness_bound_db(detail, pk)
        print("spf %d trim %d group %-28s: L %.6f (contract %.9f, bound %.2e) peak %.8g gain %.8g blocks %d" % (
            spf, trim, "+".join(grp), got[a, 0], detail[4], bound, got[a, 1], got[a, 2], got[a, 3]))
        for b in range(a, e):
            assert got[b].tobytes() == got[a].tobytes(), (grp, got[a:e])  # identical bits in every row of the group
        assert got[a, 3] == want[3] and abs(float(got[a, 0]) - detail[4]) <= bound, (grp, got[a], want)
        assert got[a, 1].tobytes() == rows[a:e, 1].max().tobytes(), "the peak is the group's"
        _check_gain(got[a], detail, TC.ROWS[grp[0]][1], bound, grp)
    assert np.isnan(TC.ROWS[names[3]][1]) and got[3, 2] == 1.0 and got[4, 2] == 1.0, "a NaN first target leaves the whole group alone"
    assert got[0, 0] != rows[0, 0] and got[1, 2] == got[0, 2] and rows[1, 2] != rows[0, 2]
    # a group of one row equals the row scope, bitwise
    one = _level(names, spf, trim, true_peak, starts=(1, 1, 0, 1, 1, 1, 0, 0))
    for b in (0, 3, 4):
        assert one[b].tobytes() == rows[b].tobytes(), b
    assert ops.status() == 0


def test_packed_sine_row_holds_its_ceiling_at_48_khz_only_with_the_true_peak():
    spf, trim, names = 600, 50, TC.MAIN
    wave, frames, target, _ = _batch(names, spf, trim)
    b = names.index("sine")
    limit = 32767.0 * TC.CEILING * (1.0 + ripple()) + 0.5
    U, D, taps = resample.design(48000)
    n = TC.samples_of("sine", spf, trim)
    seen = {}
    for tp in (False, True):
        lv = torch.from_numpy(np.array(_cached(names, spf, trim, tp))).to(DEV)
        packed, offs = ops.wave_pack_level(wave, frames, lv, rate=48000, fmt="s16", trim=trim, samples_per_frame=spf)
        o = offs.cpu().tolist()
        row = packed[o[b]:o[b + 1]].cpu().numpy().astype(np.int64)
        _, bound = RR.polyphase(TC.content()["sine"][0][:n] * lv[b, 2].item(), n, taps, U, D)
        seen[tp] = (int(np.abs(row).max()), limit + 32767.0 * float(bound.max()))
        print("true_peak %d: gain %.6f, largest packed magnitude %d, limit %.2f" % (tp, lv[b, 2].item(), *seen[tp]))
    assert seen[True][0] <= seen[True][1], "with the true peak every output sample is at or below the ceiling"
    assert seen[False][0] == 32767 and seen[False][0] > seen[False][1] + 1000, "the sample-peak run clamps: the test tells the two apart"
    assert ops.status() == 0


def test_one_graph_serves_targets_and_start_flags_and_a_plain_level_records_what_it_did(monkeypatch):
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T, N = P["T"], b["tokens"].shape[1]
    ld = b["lengths"].to(torch.int32).to(DEV)
    feed = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    build = dict(ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, pack="s16", sample_rate=48000, marks=True, passage=True)
    calls = []
    real = ops.wave_level
    monkeypatch.setattr(ops, "wave_level", lambda *a, **kw: calls.append(sorted(k for k in ("true_peak", "starts") if k in kw)) or real(*a, **kw))
    plain = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, level=pipeline.Level(K, target=-23.0), **build)
    res = plain(**feed)
    rows0, marks0, lv0 = res.to_host(marks=True, level=True)
    rows0, marks0, lv0 = [r.copy() for r in rows0], marks0.copy(), lv0.copy()
    assert calls and all(c == [] for c in calls), "a plain Level records the plain entry (the warm-up run and the capture)"
    again = real(res.wave, res.frames, plain.static["level"].target, ceiling=plain.static["level"].ceiling, max_gain_db=20.0,
                 trim=P["trim"], samples_per_frame=res.wave.shape[-1] // T)
    assert again.cpu().numpy().tobytes() == lv0.tobytes(), "and its table is st2_wave_level's, bit for bit"
    with pytest.raises(ValueError, match="pass passage"):
        pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, level=pipeline.Level(K, scope="passage"),
                                  **dict(build, passage=False))
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, level=pipeline.Level(K, target=-23.0, true_peak=True, scope="passage"),
                                   **build)
    assert gs.static["level"].true_peak and gs.static["level"].scope == "passage"
    res = gs(**feed)
    graph = gs._g["graph"]
    assert calls[-1] == ["starts", "true_peak"]
    rows1, marks1, lv1 = res.to_host(marks=True, level=True)
    lv1 = lv1.copy()
    assert np.array_equal(marks1, marks0) and [len(r) for r in rows1] == [len(r) for r in rows0], "marks and counts do not move"
    assert all(lv1[k].tobytes() == lv1[0].tobytes() for k in range(K)), "one passage, one level"
    assert lv1[0, 1] >= lv0[:, 1].max(), "the passage's true peak is no less than any row's sample peak"
    # changed start flags and changed targets: the same graph
    res = gs(starts=[1, 0, 1, 0], level=[-20.0, -30.0, -26.0, None])
    assert gs._g["graph"] is graph, "no re-record"
    rows2, marks2, lv2 = res.to_host(marks=True, level=True)
    lv2 = lv2.copy()
    # (the start flags also reset the style carry, so the synthesis itself differs: the plain graph under the same flags)
    rows3, marks3 = plain(starts=[1, 0, 1, 0]).to_host(marks=True)
    assert np.array_equal(marks2, marks3) and [len(r) for r in rows2] == [len(r) for r in rows3], "marks and counts do not move"
    res = gs()
    assert lv2[0].tobytes() == lv2[1].tobytes() and lv2[2].tobytes() == lv2[3].tobytes() and lv2[0].tobytes() != lv2[2].tobytes()
    eager = real(res.wave, res.frames, gs.static["level"].target, ceiling=gs.static["level"].ceiling, max_gain_db=20.0, trim=P["trim"],
                 samples_per_frame=res.wave.shape[-1] // T, true_peak=resample.true_peak_table(DEV),
                 starts=torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=DEV))
    assert eager.cpu().numpy().tobytes() == lv2.tobytes()
    torch.cuda.synchronize()
    ops.check_status()
