"""Intonation without a GPU: the numpy contract of tests/_intonation_ref.py against its plain loop and the
properties the design states; `pipeline.Intonation` validating, slicing and staying neutral; the refusals of every entry point,
which come before anything needs a model; `st2_pitch_shape` declared, exported, bound under ABI 23 and refusing bad arguments
before any launch."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _intonation_ref as R
from styletts2_amd import _build, _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


def curve(L, seed=0, unvoiced=0.3):
    """A speech-like F0 row: 80..400 Hz with unvoiced stretches of exact zeros."""
    g = np.random.default_rng(seed)
    x = (80.0 * np.exp2(2.3 * g.random(L))).astype(F32)
    x[g.random(L) < unvoiced] = 0
    return x


# ---- the contract --------------------------------------------------------------------------------------------------------------
CASES = [dict(), dict(r_b=0.0), dict(r_b=2.5), dict(r_b=NAN), dict(r_b=7.0), dict(points=[(0, 0), (1, 12)]),
         dict(points=[(0.2, -3), (0.5, 4), (0.5, -4), (0.9, 2)], r_b=1.5), dict(points=[(0.7, 5), (0.3, -5), (NAN, 1), (1.0, NAN)]),
         dict(points=[(-1, -30), (2, 30)]), dict(points=[(0.5, 6)]), dict(tok="tok", shift=False), dict(tok="tok", shift=True, r_b=3.0),
         dict(tok="tok", shift=True, r_b=0.5, points=[(0, 2), (0.5, -2), (1, 7)], lo_hz=120.0, hi_hz=260.0)]


@pytest.mark.parametrize("L,T_b", [(2, 1), (40, 20), (40, 13), (600, 129), (16, 0)])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_contract_agrees_with_a_plain_loop(L, T_b, case):
    g = np.random.default_rng(L + T_b)
    x = curve(L, seed=L)
    x[1::7] = [NAN, INF, -INF, -120.0, 10.0, 9.5][L % 6]
    kw = dict(case)
    if kw.get("tok") is not None:
        N = 7
        kw["tok"] = np.array([0.0, 0.5, 1.0, 2.0, NAN, 9.0, -1.0], dtype=F32)
        kw["dur"] = g.integers(0, max(L // 8, 2), N)
        kw["dur"][-1] = 0
    a, pa = R.reference_row(x, T_b, **kw)
    b, pb = R.brute_row(x, T_b, **kw)
    assert np.array_equal(R.bits(a), R.bits(b)) and np.array_equal(R.bits(pa), R.bits(pb))
    assert np.array_equal(R.bits(a[2 * T_b:]), R.bits(x[2 * T_b:]))


def test_range_one_without_points_is_the_identity_and_unvoiced_columns_keep_their_bits():
    x = curve(200)
    x[3], x[10], x[11], x[50], x[51], x[60] = NAN, INF, -INF, -200.0, 10.0, F32(-0.0)
    for kw in (dict(), dict(r_b=1.0), dict(r_b=1.0, points=[(NAN, 3)]), dict(r_b=1.0, points=[(0.0, 0.0), (1.0, 0.0)]),
               dict(r_b=1.0, tok=np.ones(4, dtype=F32), dur=[10, 20, 30, 40])):
        out, p = R.reference_row(x, 100, **kw)
        assert np.array_equal(R.bits(out), R.bits(x))
    un = ~R.is_voiced(x, 10.0)
    assert un[[3, 10, 11, 50, 51, 60]].all()
    out, _ = R.reference_row(x, 100, r_b=2.0, points=[(0, 5), (1, -5)])
    assert np.array_equal(R.bits(out[un]), R.bits(x[un])) and not np.array_equal(out[~un], x[~un])
    # a row without a voiced column is left alone and reports {NaN, 0, NaN, NaN}
    out, p = R.reference_row(np.where(un, x, F32(0)), 100, r_b=0.0, points=[(0, 5)])
    assert np.array_equal(R.bits(out), R.bits(np.where(un, x, F32(0)))) and p[1] == 0 and np.isnan(p[[0, 2, 3]]).all()


def test_range_zero_is_the_geometric_mean_and_the_mean_of_log2_is_kept():
    x = curve(400, seed=3)
    vo = R.is_voiced(x, 10.0)
    m = np.log2(x[vo].astype(F64)).mean()
    out, p = R.reference_row(x, 200, r_b=0.0)
    assert (out[vo] == F32(np.exp2(m))).all() and p[0] == p[2] == p[3] == F32(np.exp2(m)) and p[1] == vo.sum()
    for r in (0.25, 0.5, 2.0):  # exp2(m +- 2.3 * 2) stays inside [1e-3, 1e5]: no clamp at these bounds
        out, p = R.reference_row(x, 200, r_b=r, lo_hz=10.5, hi_hz=20000.0)
        assert abs(np.log2(out[vo].astype(F64)).mean() - m) <= 1e-6
        # the deviations are the input's times r, to fp32 rounding of the output (2^-24 relative = 9e-8 in log2)
        assert np.abs((np.log2(out[vo].astype(F64)) - m) - r * (np.log2(x[vo].astype(F64)) - m)).max() <= 2e-7


def test_a_rising_contour_doubles_the_last_frame_against_the_first_to_the_half_frame_offset():
    T = 50
    x = np.full(2 * T, 200.0, dtype=F32)
    out, _ = R.reference_row(x, T, points=[(0, 0), (1, 12)], hi_hz=20000.0)
    # frame t sits at x = (t + 0.5) / T: the first at 0.5 / T, the last at 1 - 0.5 / T -> 12 (1 - 1 / T) semitones between them
    want = np.exp2((12.0 * (1.0 - 1.0 / T)) / 12.0)
    assert abs(float(out[-1]) / float(out[0]) - want) <= 4 * 2.0 ** -24 * want
    assert out[0] == out[1] and out[-1] == out[-2] and (np.diff(out[::2]) > 0).all()
    assert abs(float(out[0]) - 200.0 * np.exp2(0.5 / T)) <= 2 * 2.0 ** -24 * 200.0 * 2


def test_coincident_points_step_and_positions_outside_the_points_are_flat():
    T = 40
    x = np.full(2 * T, 150.0, dtype=F32)
    out, _ = R.reference_row(x, T, points=[(0.25, 0), (0.5, 0), (0.5, 12), (0.75, 12)])
    assert (out[:2 * 20] == F32(150.0)).all() and np.array_equal(R.bits(out[:40]), R.bits(x[:40]))  # c == 0: the input's bits
    assert (out[2 * 20:] == F32(300.0)).all()  # frame 20 sits at 0.5125 > 0.5: both points passed, c = 12
    ps, vs = R.clean_contour([(0.7, 5), (0.3, -5), (NAN, 1), (1.0, NAN), (2.0, 30), (-1, -30)])
    assert ps.tolist() == [F32(0.7), F32(0.7), 1.0, 1.0] and vs.tolist() == [5.0, -5.0, 24.0, -24.0]


def test_a_clamped_column_stays_voiced_and_pitch_reports_the_output():
    x = curve(300, seed=5)
    vo = R.is_voiced(x, 10.0)
    out, p = R.reference_row(x, 150, r_b=4.0, points=[(0, -24), (1, 24)], lo_hz=40.0, hi_hz=1100.0)
    assert (out[vo] >= 40.0).all() and (out[vo] <= 1100.0).all() and (out[vo] == 40.0).any() and (out[vo] == 1100.0).any()
    assert np.array_equal(R.is_voiced(out, 10.0), vo)
    assert p.dtype == F32 and p[1] == vo.sum() and p[2] == out[vo].min() == 40.0 and p[3] == out[vo].max() == 1100.0
    assert p[0] == F32(np.exp2(np.float64(np.log2(x[vo].astype(F64)).mean()))) or abs(p[0] - np.exp2(np.log2(x[vo].astype(F64)).mean())) < 1e-4
    # the batch form: rows, frames and tables line up
    f0 = np.stack([curve(40, seed=b) for b in range(3)])
    outs, ps = R.reference(f0, frames=[0, 7, 99], range=[0.0, 0.0, 0.0])
    assert np.array_equal(R.bits(outs[0]), R.bits(f0[0])) and ps[0, 1] == 0 and np.array_equal(R.bits(outs[1, 14:]), R.bits(f0[1, 14:]))
    assert ps[2, 1] == R.is_voiced(f0[2], 10.0).sum() and len(np.unique(outs[2][R.is_voiced(f0[2], 10.0)])) == 1


def test_token_ranges_follow_the_expansions_index():
    import _marks_ref as M
    dur = [3, 0, 4, 2, 0]
    for shift in (False, True):
        assert R.token_index(dur, 9, 12, shift).tolist() == M.brute_index(dur, 9, shift)
    x = np.full(24, 100.0, dtype=F32)
    x[::2] = 200.0  # log2 deviations of +-0.5 around m = log2(141.4)
    out, _ = R.reference_row(x, 9, r_b=2.0, tok=[0.0, 1.0, 0.5, 3.0, 1.0], dur=dur, shift=False, lo_hz=20.0, hi_hz=20000.0)
    gm = F32(np.exp2(F64(0.5) * (np.log2(F64(100)) + np.log2(F64(200)))))
    assert (out[:6] == gm).all()  # token 0: r = 2 * 0 = 0
    assert np.array_equal(R.bits(out[6:14]), R.bits(x[6:14]))  # token 2: r = 2 * 0.5 = 1.0f -> the input's bits
    assert np.allclose(out[14:18:2], 141.42135 * 4.0) and np.allclose(out[15:18:2], 141.42135 / 4.0)  # token 3: min(2 * 3, 4) = 4
    assert np.array_equal(R.bits(out[18:]), R.bits(x[18:]))  # past the row's 9 frames


# ---- Intonation ----------------------------------------------------------------------------------------------------------------
def test_intonation_validates_keeps_one_table_each_and_slices_over_the_same_memory():
    it = pipeline.Intonation(3, range=[0, 1, 4], contour=[[(0, 0), (1, 12)], [], [(0.5, -24), (0.5, 24), (1.0, 0)]], tok_range=0.5, N=6,
                             device="cpu")
    assert it.range.tolist() == [0.0, 1.0, 4.0] and tuple(it.contour.shape) == (3, 8, 2) and tuple(it.tok_range.shape) == (3, 6)
    assert it.contour[0, :2].tolist() == [[0.0, 0.0], [1.0, 12.0]] and it.contour[0, 2:].isnan().all() and it.contour[1].isnan().all()
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in (it.range, it.contour, it.tok_range))
    assert (it.B, it.K, it.N, it.voiced_hz) == (3, 8, 6, 10.0) and it.device == torch.device("cpu")
    part = it.slice(1, 3)
    assert part.B == 2 and (part.K, part.N, part.voiced_hz) == (8, 6, 10.0)
    assert part.range.data_ptr() == it.range[1:].data_ptr() and part.contour.data_ptr() == it.contour[1].data_ptr()
    assert part.tok_range.data_ptr() == it.tok_range[1].data_ptr()
    one = pipeline.Intonation(2, contour=[(0, 1), (1, 2)], K=2, device="cpu")  # one list for every row
    assert one.range is None and one.tok_range is None and one.N is None and torch.equal(one.contour[0], one.contour[1])
    assert pipeline.Intonation(2, tok_range=torch.ones(2, 9), device="cpu").N == 9
    assert pipeline.Intonation(2, device="cpu").contour is None
    bad = [(dict(range=-0.1), "range must lie in"), (dict(range=4.5), "range must lie in"), (dict(range=NAN), "range must lie in"),
           (dict(range=[1, 2]), "range must be one value or 3 values"), (dict(tok_range=5.0, N=4), "tok_range must lie in"),
           (dict(tok_range=INF, N=4), "tok_range must lie in"), (dict(tok_range=1.0), "tok_range needs N"),
           (dict(tok_range=torch.ones(3, 4), N=5), r"tok_range must be one value or \[3, 5\] values"), (dict(N=0), "N must lie in 1..512"),
           (dict(N=513), "N must lie in 1..512"), (dict(K=9), "K must lie in 0..8"), (dict(K=-1), "K must lie in 0..8"),
           (dict(voiced_hz=0.0), "voiced_hz must lie in"), (dict(voiced_hz=40.0), "voiced_hz must lie in"), (dict(voiced_hz=NAN), "voiced_hz"),
           (dict(contour=[(0.5, 1), (0.4, 1)]), "must ascend"), (dict(contour=[(1.5, 0)]), "must lie in"),
           (dict(contour=[(-0.1, 0)]), "must lie in"), (dict(contour=[(0.5, 25)]), "must lie in"), (dict(contour=[(0.5, NAN)]), "must lie in"),
           (dict(contour=[(NAN, 0)]), "must lie in"), (dict(contour=[[(0, 0)], [(1, 1)]]), "or 3 of them"),
           (dict(contour=[(0.1, 0), (0.2, 0), (0.3, 0)], K=2), "at most K = 2"), (dict(contour=[[(0, 0, 0)], [], []]), "pairs")]
    for kw, text in bad:
        with pytest.raises(ValueError, match="Intonation: .*" + text):
            pipeline.Intonation(3, device="cpu", **kw)
    with pytest.raises(ValueError, match="Intonation: B must be positive"):
        pipeline.Intonation(0, device="cpu")
    sig = list(inspect.signature(pipeline.Intonation.__init__).parameters)[1:]
    assert sig == ["B", "range", "contour", "tok_range", "N", "K", "voiced_hz", "device"]


def test_neutral_holds_every_table_and_the_contract_makes_it_the_identity():
    it = pipeline.Intonation.neutral(2, N=5, K=4, device="cpu")
    assert it.range.tolist() == [1.0, 1.0] and it.tok_range.eq(1).all() and tuple(it.contour.shape) == (2, 4, 2) and it.contour.isnan().all()
    assert pipeline.Intonation.neutral(2, device="cpu").tok_range is None
    f0 = np.stack([curve(40, seed=b) for b in range(2)])
    out, _ = R.reference(f0, range=it.range.numpy(), tok_range=it.tok_range.numpy(), dur=np.full((2, 5), 4), contour=it.contour.numpy())
    assert np.array_equal(R.bits(out), R.bits(f0))


# ---- refusals, with no model ---------------------------------------------------------------------------------------------------
TOKENS = torch.zeros(2, 5, dtype=torch.long)
SENTENCES = [torch.zeros(5, dtype=torch.long), torch.zeros(3, dtype=torch.long)]


@pytest.mark.parametrize("entry", ["prepare", "inference", "inference_capacity", "synthesize_long", "synthesize_long_capacity"])
def test_entry_points_refuse_before_anything_needs_a_model(entry, monkeypatch):
    it = pipeline.Intonation(2, range=2.0, device="cpu")

    def call(intonation, **kw):
        if entry == "prepare":
            return pipeline.prepare(None, None, TOKENS, intonation=intonation, **kw)
        if entry.startswith("inference"):
            return pipeline.inference(None, None, TOKENS, intonation=intonation, **kw, **({"max_frames": 20} if "capacity" in entry else {}))
        kw.pop("taps", None)
        return pipeline.synthesize_long(None, None, SENTENCES, intonation=intonation, **kw, **({"max_frames": 20} if "capacity" in entry else {}))

    with pytest.raises(ValueError, match="intonation must be a pipeline.Intonation"):
        call(dict(range=2.0))
    with pytest.raises(ValueError, match="intonation needs the C\\+\\+ engine path \\(HIP device, no taps\\)"):
        call(it)  # a CPU batch
    if not entry.endswith("long_capacity"):  # (that path refuses any front= on its own)
        with pytest.raises(ValueError, match="intonation cannot be combined with front="):
            call(it, front=object())
    monkeypatch.setattr(pipeline._hooks, "plan", "python")
    with pytest.raises(ValueError, match="intonation needs the C\\+\\+ engine plans"):
        call(it)
    monkeypatch.undo()
    if entry.startswith("synthesize_long"):
        with pytest.raises(ValueError, match="one row per sentence \\(2\\)"):
            call(pipeline.Intonation(3, device="cpu"))
        if entry == "synthesize_long":
            with pytest.raises(ValueError, match="per-token ranges are not served on the long-form path"):
                call(pipeline.Intonation(2, tok_range=1.0, N=5, device="cpu"))


def test_the_one_check_judges_rows_width_device_and_taps_of_a_device_batch():
    """What a CPU batch cannot reach: `_check_intonation` as the entry points call it for a batch on cuda:0."""
    dev = torch.device("cuda", 0)

    def on(it, d=dev):
        it.device = d  # as if its tables lived there
        return it
    ok = on(pipeline.Intonation(2, tok_range=1.0, N=5, device="cpu"))
    pipeline._check_intonation(ok, dev, 2, None, None, 5)
    pipeline._check_intonation(ok, dev, 2, None, None, None)
    with pytest.raises(ValueError, match="per-token rows of 5 tokens, the batch is 4 wide"):
        pipeline._check_intonation(ok, dev, 2, None, None, 4)
    with pytest.raises(ValueError, match="intonation describes 2 rows on cuda:0, the batch has 3 on cuda:0"):
        pipeline._check_intonation(ok, dev, 3, None, None, 5)
    with pytest.raises(ValueError, match="intonation describes 2 rows on cuda:1, the batch has 2 on cuda:0"):
        pipeline._check_intonation(on(pipeline.Intonation(2, device="cpu"), torch.device("cuda", 1)), dev, 2, None, None, 5)
    with pytest.raises(ValueError, match="HIP device, no taps"):
        pipeline._check_intonation(ok, dev, 2, {}, None, 5)


def test_graphed_synthesis_refuses_a_wrong_intonation_before_it_looks_at_the_model():
    with pytest.raises(ValueError, match="intonation must be True or a pipeline.Intonation, got dict"):
        pipeline.GraphedSynthesis(None, None, 2, 5, 20, 3, intonation={})
    with pytest.raises(ValueError, match="intonation must be a pipeline.Intonation of 2 rows"):
        pipeline.GraphedSynthesis(None, None, 2, 5, 20, 3, intonation=pipeline.Intonation(3, device="cpu"))
    g = object.__new__(pipeline.GraphedSynthesis)  # a graph built without it refuses the argument at the call
    g.static = {}
    with pytest.raises(ValueError, match="this graph was built without intonation: pass intonation=True"):
        g(intonation=pipeline.Intonation(2, device="cpu"))
    g.static = {"intonation": pipeline.Intonation.neutral(2, device="cpu")}
    for given, text in ((pipeline.Intonation(3, device="cpu"), "of 2 rows"), (pipeline.Intonation(2, K=4, device="cpu"), "the graph's own"),
                        (pipeline.Intonation(2, voiced_hz=5.0, device="cpu"), "the graph's own"),
                        (pipeline.Intonation(2, tok_range=1.0, N=5, device="cpu"), "token_controls=True")):
        with pytest.raises(ValueError, match=text):
            g(intonation=given)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
D = C.c_void_p(4096)
BASE = dict(f0=D, bs=600, B=3, L=600, frames=D, range=D, tok_range=D, dur=D, N=70, shift=1, contour=D, K=8, voiced_hz=10.0, lo_hz=40.0,
            hi_hz=1100.0, pitch=D)


def _call(lib, a):
    return lib.st2_pitch_shape(a["f0"], a["bs"], a["B"], a["L"], a["frames"], a["range"], a["tok_range"], a["dur"], a["N"], a["shift"],
                               a["contour"], a["K"], a["voiced_hz"], a["lo_hz"], a["hi_hz"], a["pitch"], None)


def test_pitch_shape_is_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "st2.h")).read()
    assert re.search(r"\bint st2_pitch_shape\(float\* f0, int64_t bs, int32_t B, int32_t L, const int32_t\* frames", text)
    assert hasattr(lib, "st2_pitch_shape") and "st2_pitch_shape" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert "st2_intonation.hip" in _build.SOURCES and _build.EXTRA_FLAGS["st2_intonation.hip"] == ["-fno-slp-vectorize"]
    assert ops.PITCH_POINTS == R.MAX_POINTS == 8
    # the scan is stated once, in the header both units include
    csrc = os.path.join(ROOT, "styletts2_amd", "csrc")
    where = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and "void scan_durations" in open(os.path.join(csrc, f)).read()]
    assert where == ["st2_tokens.h"]
    for unit in ("st2_marks.hip", "st2_intonation.hip"):
        assert '#include "st2_tokens.h"' in open(os.path.join(csrc, unit)).read()


def test_pitch_shape_validates_before_any_launch():
    lib = _lib.load()
    cases = [(dict(f0=None), "f0 is NULL"), (dict(B=0), "B=0 must lie in 1..65535"), (dict(B=65536), "must lie in 1..65535"),
             (dict(L=0), "L=0 must be positive and even"), (dict(L=-2), "positive and even"), (dict(L=601), "positive and even"),
             (dict(bs=599), "bs=599 is less than L=600"), (dict(dur=None), "tok_range needs dur"), (dict(N=0), "N=0 tokens must lie in 1..512"),
             (dict(N=513), "N=513 tokens must lie in 1..512"), (dict(K=-1), "K=-1 contour points must lie in 0..8"),
             (dict(K=9), "K=9 contour points must lie in 0..8"), (dict(contour=None), "contour is NULL with K=8"),
             (dict(voiced_hz=0.0), "must lie in (0, 1000]"), (dict(voiced_hz=-1.0), "must lie in (0, 1000]"),
             (dict(voiced_hz=1000.5, lo_hz=2000.0, hi_hz=3000.0), "must lie in (0, 1000]"), (dict(voiced_hz=NAN), "must lie in (0, 1000]"),
             (dict(lo_hz=10.0), "need voiced_hz=10 < lo_hz=10 < hi_hz=1100 <= 20000"), (dict(lo_hz=1100.0), "need voiced_hz"),
             (dict(hi_hz=20000.5), "need voiced_hz"), (dict(lo_hz=NAN), "need voiced_hz"), (dict(hi_hz=NAN), "need voiced_hz")]
    for change, word in cases:
        assert _call(lib, dict(BASE, **change)) != 0, change
        msg = lib.st2_last_error().decode()
        assert msg.startswith("st2_pitch_shape:") and word in msg, (change, msg)
        with pytest.raises(_lib.St2Error, match=re.escape(word)):  # as `ops.pitch_shape` reports it
            _lib.check(_call(lib, dict(BASE, **change)), "st2_pitch_shape")
    # nothing to apply and nothing to report: 0 without a launch (a launch would fail here: there is no device)
    quiet = dict(BASE, range=None, tok_range=None, contour=None, K=0, pitch=None)
    assert _call(lib, quiet) == 0 and _call(lib, dict(quiet, dur=None, N=0, frames=None, B=1, bs=0)) == 0
    assert _call(lib, dict(quiet, contour=D)) == 0  # K = 0: no point
    assert _call(lib, dict(quiet, K=8)) != 0  # the refusals stay


def test_wrapper_has_no_cpu_path_and_checks_its_tables_first():
    f0 = torch.zeros(2, 40)
    with pytest.raises(_lib.St2Error, match="HIP device"):
        ops.pitch_shape(f0)
    with pytest.raises(_lib.St2Error, match="range must live on the device"):
        ops.pitch_shape(f0, range=torch.ones(2))
    with pytest.raises(_lib.St2Error, match="range must be a contiguous 1-D tensor of 2 entries"):
        ops.pitch_shape(f0, range=torch.ones(3))
    with pytest.raises(_lib.St2Error, match=r"tok_range must be a contiguous \[2, 5\] tensor"):
        ops.pitch_shape(f0, tok_range=torch.ones(2, 4), dur=torch.ones(2, 5, dtype=torch.long))
    with pytest.raises(_lib.St2Error, match=r"contour must be a contiguous \[2, K, 2\] tensor"):
        ops.pitch_shape(f0, contour=torch.ones(2, 8))
    with pytest.raises(_lib.St2Error, match="contour must be a float32 tensor"):
        ops.pitch_shape(f0, contour=[[0, 0]])
    with pytest.raises(_lib.St2Error, match="frames must be an int32 tensor"):
        ops.pitch_shape(f0, frames=torch.ones(2))
    sig = list(inspect.signature(ops.pitch_shape).parameters)
    assert sig == ["f0", "range", "tok_range", "dur", "contour", "frames", "shift", "voiced_hz", "lo_hz", "hi_hz", "pitch"]
