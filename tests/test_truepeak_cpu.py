"""Host side and contract of the true-peak ceiling and the passage scope of the level measurement:
`st2_wave_level_ex` and its size helper are declared, exported and bound under ABI 23 and refuse bad arguments before any launch,
in their own name -- and in `st2_wave_level`'s, byte for byte, when neither new argument is given; the 8 / 1 table meets the
section 15 acceptance conditions; the numpy contract of tests/_truepeak_ref.py reads the standard's fs / 4 case and a lone sample
as it must, and groups rows as a brute-force restatement does; `pipeline` carries and refuses the two `Level` options; and none
of the rows tests/test_truepeak_gpu.py measures sits on a tie of the gain's terms or next to a gate.  No GPU needed."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest
import torch

import _level_cases as Cs
import _level_ref as R
import _resample_ref as RR
import _truepeak_cases as TC
import _truepeak_ref as TP
from styletts2_amd import _lib, ops, pipeline, resample
from test_level_cpu import HEADER, LEVEL_ORDER, D, _err

EX_ORDER = LEVEL_ORDER + ("stream", "taps", "up", "K", "start")


# ---- the C entry -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in ("st2_wave_level_ex", "st2_wave_level_ex_workspace_bytes"):
        assert re.search(r"\b(int|int64_t) %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    for args in ((2, 10, 600, 24000), (8, 120, 600, 24000), (0, 10, 600, 24000), (2, 10, 600, 24005)):
        assert lib.st2_wave_level_ex_workspace_bytes(*args) == lib.st2_wave_level_workspace_bytes(*args), args
    assert ops.wave_level_workspace_bytes(8, 120) == 8 * 30 * 12


def _base(lib):
    need = lib.st2_wave_level_workspace_bytes(2, 10, 600, 24000)
    return dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, rate=24000, target=D, ceiling=0.89, max_gain_db=20.0,
                level=D, work=D, work_bytes=need, stream=None, taps=D, up=8, K=82, start=D)


OLD_REFUSALS = ((dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
                (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"),
                (dict(wave=C.c_void_p(258)), "aligned"), (dict(target=None), "NULL"), (dict(level=None), "NULL"),
                (dict(work=None), "NULL"), (dict(work_bytes=15), "too small"), (dict(rate=0), "sample_rate"),
                (dict(rate=22055), "sample_rate"), (dict(rate=2000000), "LDS"), (dict(ceiling=0.0), "ceiling"),
                (dict(ceiling=float("nan")), "ceiling"), (dict(max_gain_db=60.5), "max_gain_db"), (dict(level=C.c_void_p(258)), "aligned"),
                (dict(work=C.c_void_p(260)), "aligned"))


def _sized(lib, a):
    if a["rate"] > 0 and a["rate"] % 10 == 0 and a["work_bytes"] > 15:  # sized for that rate: the refusal is the rate's own
        a["work_bytes"] = max(lib.st2_wave_level_workspace_bytes(2, 10, 600, a["rate"]), 16)
    return a


def test_ex_entry_refuses_everything_before_any_launch_in_its_own_name():
    lib = _lib.load()
    for given in (dict(), dict(start=None), dict(taps=None, up=0, K=0)):  # both, the table alone, the flags alone
        for change, word in OLD_REFUSALS:
            a = _sized(lib, dict(_base(lib), **given, **change))
            assert lib.st2_wave_level_ex(*[a[k] for k in EX_ORDER]) != 0, (given, change)
            assert _err(lib).startswith("st2_wave_level_ex:") and word in _err(lib), (given, change, _err(lib))
    for change, text in ((dict(up=0), "st2_wave_level_ex: bad ratio 0 / 1 (each 1..1024)"),
                         (dict(up=1025), "st2_wave_level_ex: bad ratio 1025 / 1 (each 1..1024)"),
                         (dict(K=0), "st2_wave_level_ex: taps_per_phase=0 is outside 1..512"),
                         (dict(K=513), "st2_wave_level_ex: taps_per_phase=513 is outside 1..512"),
                         (dict(up=64, K=512), "st2_wave_level_ex: the table (up=64, taps_per_phase=512) does not fit the 61440 bytes of "
                                              "LDS beside one hop of 2400 samples"),
                         (dict(up=24, K=512, rate=48000), "st2_wave_level_ex: the table (up=24, taps_per_phase=512) does not fit the 61440 "
                                                          "bytes of LDS beside one hop of 4800 samples"),
                         (dict(taps=C.c_void_p(258)), "st2_wave_level_ex: taps is not aligned to float"),
                         (dict(start=C.c_void_p(258)), "st2_wave_level_ex: start is not aligned to int32"),
                         (dict(taps=None, start=C.c_void_p(258)), "st2_wave_level_ex: start is not aligned to int32")):
        a = _sized(lib, dict(_base(lib), **change))
        assert lib.st2_wave_level_ex(*[a[k] for k in EX_ORDER]) != 0, change
        assert _err(lib) == text, (change, _err(lib))
    # without a table, up and taps_per_phase are not looked at: the first refusal is then some later one (here: none but start's)
    a = dict(_base(lib), taps=None, up=-5, K=9999, start=C.c_void_p(258))
    assert lib.st2_wave_level_ex(*[a[k] for k in EX_ORDER]) != 0 and "start is not aligned" in _err(lib)


def test_with_neither_argument_the_ex_entry_is_the_plain_entry_refusal_for_refusal():
    lib = _lib.load()
    for change, _ in OLD_REFUSALS:
        a = _sized(lib, dict(_base(lib), taps=None, up=8, K=82, start=None, **change))
        assert lib.st2_wave_level(*[a[k] for k in LEVEL_ORDER], None) != 0
        plain = _err(lib)
        assert lib.st2_wave_level_ex(*[a[k] for k in EX_ORDER]) != 0
        assert _err(lib) == plain and plain.startswith("st2_wave_level:"), (change, plain, _err(lib))


def test_wrapper_has_no_cpu_path_and_routes_by_its_arguments(monkeypatch):
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_level(w, f, torch.zeros(2), true_peak=(8, 82, torch.zeros(8, 82)))
    with pytest.raises(_lib.St2Error):
        ops.wave_level(w, f, torch.zeros(2), starts=torch.ones(2, dtype=torch.int32))
    sig = inspect.signature(ops.wave_level).parameters
    assert sig["true_peak"].default is None and sig["starts"].default is None and list(sig)[-2:] == ["true_peak", "starts"]


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_table_is_the_section_15_design_at_8_over_1_and_meets_its_acceptance_conditions():
    U, K, taps = TP.table()
    assert (U, K) == (8, 82) and taps.shape == (8, 82) and taps.dtype == np.float32 and resample.TRUE_PEAK_UP == 8
    assert K == resample.taps_per_phase(8, 1)
    # phases 0 and 4 are the 48 kHz hand-over's two phases: what that resampler interpolates is among what the measurement reads
    U2, D2, taps2 = resample.design(48000)
    assert (U2, D2) == (2, 1) and np.array_equal(taps2, taps[[0, 4]])
    # test_resample_cpu.py's two conditions, as it computes them: the response of the flattened prototype by a zero-padded FFT
    proto = resample.prototype(taps.astype(np.float64)) / U
    nfft = 1 << int(math.ceil(math.log2(len(proto) * 64)))
    H = np.abs(np.fft.rfft(proto, nfft))
    f = np.arange(len(H)) / nfft * U  # cycles per INPUT sample
    dev = np.abs(20 * np.log10(H[f <= 0.85 * 0.5])).max()
    att = -20 * np.log10(np.maximum(H[f >= 0.5], 1e-300)).max()
    print("8 / 1: K %d, passband deviation %.5f dB, stopband attenuation %.2f dB" % (K, dev, att))
    assert dev <= 0.05 and att >= 90.0
    assert np.abs(taps.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-4


def test_true_peak_table_has_a_cache_key_of_its_own_and_is_not_built_under_capture(monkeypatch):
    monkeypatch.setattr(resample, "_TABLES", {})
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)  # the cache key of a device without an index, without a device
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    U, K, taps = resample.true_peak_table("cpu")
    assert (U, K) == (8, 82) and taps.dtype == torch.float32 and tuple(taps.shape) == (8, 82)
    assert np.array_equal(taps.numpy(), TP.table()[2]) and resample.true_peak_table("cpu")[2] is taps
    assert list(resample._TABLES) == [("tp", 192000, "cpu", 0)]
    monkeypatch.setattr(resample, "_TABLES", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match=r"before a stream capture: call resample.true_peak_table\(device\) first"):
        resample.true_peak_table("cpu")
    with pytest.raises(RuntimeError, match=r"call resample.table\(8000, device\) first"):
        resample.table(8000, "cpu")


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def ripple():
    """The passband figure the sine cases use: computed from the table, over [0, 0.85] of Nyquist."""
    return TP.deviation(TP.table()[2])


def test_ripple_figure_is_computed_from_the_table():
    r = ripple()
    at_quarter = TP.deviation(TP.table()[2], 0.5, 0.5, 1)
    print("passband deviation of the 8 / 1 table over [0, 0.85 f_N]: %.3e; at fs / 4 alone: %.3e" % (r, at_quarter))
    assert 0.0 < at_quarter <= r < 1e-3  # 0.01 dB is 1.15e-3: the acceptance condition, in its complex form
    assert TP.deviation(TP.table()[2], 0.0, 1.0) > 0.4  # and the transition band is under-read: -6 dB at the cutoff, more above


def test_contract_on_hand_computed_rows():
    _, K, taps = TP.table()
    lone = np.zeros(200, dtype=np.float32)
    lone[100] = 1.0
    tp, lo, hi = TP.true_peak(lone, taps)
    y, _ = TP.interpolate(lone, taps)
    assert abs(np.abs(y).max() - resample.CUTOFF) < 1e-6 and tp == 1.0 and lo == hi == 1.0  # phase 0 is not the identity
    assert TP.true_peak(np.zeros(0, np.float32), taps) == (0.0, 0.0, 0.0) and TP.true_peak(np.zeros(50, np.float32), taps)[0] == 0.0
    x = TC.faded_sine().astype(np.float32)
    r = ripple()
    tp, lo, hi = TP.true_peak(x, taps)
    print("faded fs/4 sine: sample peak %.6f, true peak %.6f in [%.6f, %.6f]; fp32 interval [%.7f, %.7f]" % (
        R.peak(x), tp, 0.5 * math.cos(math.pi / 32) * (1 - r), 0.5 * (1 + r), lo, hi))
    assert abs(float(R.peak(x)) - 0.5 * math.sqrt(0.5)) < 1e-6
    assert 0.5 * math.cos(math.pi / 32) * (1 - r) <= tp <= 0.5 * (1 + r)
    assert hi - lo <= 2 * (K + 1) * 2.0 ** -24 * 2.0 * 0.5  # sum_k |taps| of a phase stays below 2: some 1e-5 of the crest either way
    # a NaN counts as 0 for the interpolation too, and chunking does not show
    xn = x.copy()
    xn[5000] = np.nan
    x0 = x.copy()
    x0[5000] = 0.0
    assert TP.true_peak(xn, taps) == TP.true_peak(x0, taps)
    whole, _ = RR.polyphase(TP.clean32(x), len(x), taps, 8, 1)
    assert np.array_equal(TP.interpolate(x, taps, chunk=1000)[0], whole)


def test_groups_against_a_brute_force_restatement():
    assert TP.groups(None, 3) == [(0, 1), (1, 2), (2, 3)]
    assert TP.groups([1, 0, 0, 1, 0, 1, 0, 0], 8) == [(0, 3), (3, 5), (5, 8)]
    assert TP.groups([0, 0, 1], 3) == [(0, 2), (2, 3)] and TP.groups([0, 5, -1], 3) == [(0, 1), (1, 2), (2, 3)]
    g = np.random.default_rng(11)
    rows = [(g.standard_normal(n) * rms).astype(np.float32) for n, rms in ((12000, 0.1), (0, 1.0), (5000, 0.003), (30000, 0.02))]
    zs = [R.blocks(x, 24000) for x in rows]
    peaks = [R.peak(x) for x in rows]
    got, (z, passed, l, rel, L) = TP.level_group(zs, peaks, -20.0, 0.89, 20.0)
    # brute force: one list of every row's blocks, gated once
    every = [v for x in rows for v in R.blocks(x, 24000)]
    lk = [-0.691 + 10.0 * math.log10(v) for v in every]
    above = [v for v, q in zip(every, lk) if q > -70.0]
    rel_thr = -0.691 + 10.0 * math.log10(sum(above) / len(above)) - 10.0
    kept = [v for v, q in zip(every, lk) if q > -70.0 and q > rel_thr]
    L_bf = -0.691 + 10.0 * math.log10(sum(kept) / len(kept))
    assert len(every) == 2 + 0 + 1 + 9 and got[3] == len(kept) and abs(L - L_bf) < 1e-12 and 0 < len(kept) < len(every)
    assert got[1] == max(peaks) and got[2] == R.gain(L, max(peaks), -20.0, 0.89, 20.0)
    # the quiet aside is not pulled up: on its own it would get the limit, in the group it gets the group's gain
    alone = R.level_row(rows[2], 24000, -20.0, 0.89, 20.0)[0]
    assert alone[2] == np.float32(10.0) and got[2] < 3.0
    # a group of one row is the row
    one, _ = TP.level_group([zs[0]], [peaks[0]], -20.0, 0.89, 20.0)
    assert one.tobytes() == R.level_row(rows[0], 24000, -20.0, 0.89, 20.0)[0].tobytes()
    nan, _ = TP.level_group(zs, peaks, float("nan"), 0.89, 20.0)
    assert nan[2] == 1.0 and nan[0] == got[0]


# ---- Level and the refusals ------------------------------------------------------------------------------------------------------
def test_level_carries_both_options_and_refuses_a_bad_scope():
    lv = pipeline.Level(3, device="cpu")
    assert lv.true_peak is False and lv.scope == "row"
    lv = pipeline.Level(4, target=[-10.0, -20.0, -30.0, -40.0], device="cpu", true_peak=True, scope="passage")
    assert lv.true_peak is True and lv.scope == "passage" and lv.target.tolist() == [-10.0, -20.0, -30.0, -40.0]
    part = lv.slice(1, 3)
    assert part.true_peak is True and part.scope == "passage" and part.B == 2
    for bad in ("sentence", None, True):
        with pytest.raises(ValueError, match="Level: scope must be one of"):
            pipeline.Level(3, device="cpu", scope=bad)
    with pytest.raises(ValueError, match="Level"):
        pipeline.Level(0, device="cpu", true_peak=True)


def test_output_spec_refuses_a_passage_scope_without_a_passage_and_across_front_groups():
    tokens = torch.zeros(2, 5, dtype=torch.long)
    lv = pipeline.Level(2, device="cpu", scope="passage")
    text = "level of scope 'passage' is one gain for the rows of a passage: pass passage"
    for more in (dict(), dict(passage=False)):
        with pytest.raises(ValueError) as e:
            pipeline.inference(None, None, tokens, max_frames=10, pack="s16", level=lv, **more)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        pipeline._output_spec(2, True, pack="s16", level=lv, graph=True, passage=False)
    assert str(e.value) == text
    pipeline._output_spec(2, True, pack="s16", level=lv, passage=True)
    pipeline._output_spec(2, True, pack="s16", level=lv, passage=[1, 0])
    pipeline._output_spec(2, True, pack="s16", level=pipeline.Level(2, device="cpu", true_peak=True))  # a row scope needs none
    sentences = [torch.zeros(5, dtype=torch.long), torch.zeros(3, dtype=torch.long), torch.zeros(4, dtype=torch.long)]
    lv3 = pipeline.Level(3, device="cpu", scope="passage")
    with pytest.raises(ValueError) as e:
        pipeline.synthesize_long(None, None, sentences, max_frames=10, pack="s16", level=lv3, front_batch=2)
    assert str(e.value) == ("level of scope 'passage' is one gain for the rows of ONE call, and front_batch cuts this passage into 2: "
                            "pass front_batch=0")
    # the refusals live where section 24 keeps the level refusals
    src = inspect.getsource(pipeline._output_spec)
    assert "scope 'passage'" in src and "pipeline.Level of %d rows" in src
    assert sum(inspect.getsource(f).count("scope 'passage'") for f in (pipeline.inference, pipeline.synthesize_long,
                                                                       pipeline._synthesize_long_capacity, pipeline._hand_over)) == 0


@pytest.fixture
def spied(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "wave_pack_level", lambda wave, frames, *a, **kw: (kw["out"], kw["offsets"]))
    monkeypatch.setattr(ops, "wave_level", lambda wave, frames, target, **kw: seen.append(kw) or kw["out"])
    monkeypatch.setattr(pipeline.resample, "true_peak_table", lambda dev: (8, 82, "taps on %s" % dev))
    return seen


def test_hand_over_passes_the_table_and_the_start_flags_on_and_neither_for_a_plain_level(spied):
    B, L, spf = 3, 1200, 600
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    pipeline._hand_over(wave, frames, 50, "s16", spf, level=pipeline.Level(B, device="cpu"), starts=[1, 0, 1])
    assert "true_peak" not in spied[0] and "starts" not in spied[0]
    pipeline._hand_over(wave, frames, 50, "s16", spf, level=pipeline.Level(B, device="cpu", true_peak=True))
    assert spied[1]["true_peak"] == (8, 82, "taps on cpu") and "starts" not in spied[1]
    lv = pipeline.Level(B, device="cpu", true_peak=True, scope="passage")
    for passage, want in ((None, [1, 0, 0]), (True, [1, 0, 0]), ([0, 1, 1], [0, 1, 1]), (torch.tensor([1, 0, 7]), [1, 0, 1])):
        del spied[:]
        pipeline._hand_over(wave, frames, 50, "s16", spf, level=lv, starts=passage)
        st = spied[0]["starts"]
        assert st.dtype == torch.int32 and st.tolist() == want and spied[0]["true_peak"][0] == 8
    sig = inspect.signature(pipeline._hand_over).parameters
    assert list(sig)[-2:] == ["level", "starts"] and sig["starts"].default is None


# ---- the GPU test's cases, from the contract alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("spf,trim", TC.GEOMETRIES)
def test_no_gpu_case_sits_on_a_tie_or_next_to_a_gate(spf, trim):
    cases = []
    for names in (TC.MAIN, TC.OTHER):
        for name in names:
            for tp in (False, True):
                cases.append(((name,), tp, None))
    for a, e in TP.groups(TC.GROUP_START, 8):
        for tp in (False, True):
            cases.append((TC.GROUP_ROWS[a:e], tp, None))
    for names, tp, _ in cases:
        want, detail = TC.expect_group(names, spf, trim, tp)
        assert TC.gate_distance(detail) >= Cs.GUARD_LU, (names, tp, TC.gate_distance(detail))
        terms = sorted(TP.binding_terms(detail[4], want[1], TC.ROWS[names[0]][1], TC.CEILING, TC.MAX_GAIN_DB))
        print("spf %d trim %d %-40s true_peak %d: L %9.4f peak %.6f terms %s gain %.6f" % (spf, trim, "+".join(names), tp, detail[4],
                                                                                            want[1], ["%.4g" % t for t in terms], want[2]))
        if terms[0] < math.inf:
            assert terms[1] >= terms[0] * (1 + 1e-3), (names, tp, terms)
    if spf == 1:
        assert [TC.samples_of(n, spf, trim) for n in ("empty", "s17", "s11999")] == [0, 17, 11999]
    # the sine rows: the ceiling binds under either peak, and the two readings are 3 dB apart
    for tp, pk in ((False, 0.5 * math.sqrt(0.5)), (True, 0.5)):
        want, detail = TC.expect_group(("sine",), spf, trim, tp)
        assert abs(float(want[1]) - pk) < 2e-3 * pk and want[2] == np.float32(TC.CEILING / float(want[1]))


def test_packed_sine_row_tells_a_sample_peak_ceiling_from_a_true_peak_one():
    """What tests/test_truepeak_gpu.py's packing case asserts, computed from the contract: at 48 kHz s16 the sine row packed with
    the sample-peak gain has samples far above its ceiling, with the true-peak gain none above 32767 ceiling (1 + ripple) + 0.5 +
    the fp32 bound."""
    spf, trim = 600, 50
    n = TC.samples_of("sine", spf, trim)
    x = TC.content()["sine"][0][:n]
    U, D, taps = resample.design(48000)
    limit = 32767.0 * TC.CEILING * (1.0 + ripple()) + 0.5
    seen = {}
    for tp in (False, True):
        g = TC.expect_group(("sine",), spf, trim, tp)[0][2]
        y, bound = RR.polyphase(x * g, n, taps, U, D)
        seen[tp] = np.abs(32767.0 * y).max() + 32767.0 * bound.max() * tp - 32767.0 * bound.max() * (not tp)
        print("true_peak %d: gain %.5f, largest packed magnitude %.1f against the limit %.1f" % (tp, g, seen[tp], limit))
    assert seen[True] <= limit and min(seen[False], 32767.0) > limit + 1000.0
