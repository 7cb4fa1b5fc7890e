"""C ABI and host-side contract of the compressor of the hand-over: `st2_wave_dynamics` and its helpers are
declared, exported and bound under ABI 23 and refuse bad arguments before any launch; `Dynamics` validates its settings, keeps
them as one table and slices over the same memory; the hand-over layout gains its ninth part without moving the other eight;
`_output_spec` refuses the option in the one place; `_hand_over_edges` runs the stage behind the breaks and in front of the level
and calls nothing new without it; the numpy contract of tests/_dynamics_ref.py agrees with a plain loop and has the properties
the design states.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _dynamics_ref as R
from styletts2_amd import _build, _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_wave_dynamics", "st2_wave_dynamics_workspace_bytes", "st2_wave_dynamics_tile")
INF, NAN = float("inf"), float("nan")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW + ("st2_wave_dynamics_chunk",):
        assert re.search(r"\b(int|int32_t|int64_t) %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert lib.st2_wave_dynamics_tile() == ops.DYNAMICS_TILE and lib.st2_wave_dynamics_chunk() == ops.DYNAMICS_CHUNK
    assert ops.DYNAMICS_BLOCK == 64 and ops.DYNAMICS_TILE % 64 == 0
    assert "st2_dynamics.hip" in _build.SOURCES and _build.EXTRA_FLAGS["st2_dynamics.hip"] == ["-fno-slp-vectorize"]
    # the block sums are stated once, in the header both units include
    csrc = os.path.join(ROOT, "styletts2_amd", "csrc")
    where = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and "void breaks_sums_kernel" in open(os.path.join(csrc, f)).read()]
    assert where == ["st2_blocksums.h"]
    for unit in ("st2_breaks.hip", "st2_dynamics.hip"):
        assert '#include "st2_blocksums.h"' in open(os.path.join(csrc, unit)).read()


D = C.c_void_p(4096)
ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "params", "A", "win", "rho", "out", "o_bs", "dyn", "work", "work_bytes")


def _call(lib, a):
    return lib.st2_wave_dynamics(a["wave"], a["w_bs"], a["frames"], a["B"], a["T_cap"], a["spf"], a["trim"], a["params"], a["A"],
                                 a["win"], C.c_double(a["rho"]), a["out"], a["o_bs"], a["dyn"], a["work"], a["work_bytes"], None)


def test_wave_dynamics_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_dynamics_workspace_bytes(2, 10, 600)
    assert need == (4 * 2 * 2 * 94 + 15) // 16 * 16  # lin and s, ceil(6000 / 64) = 94 blocks a row
    assert ops.wave_dynamics_workspace_bytes(2, 10, 600) == need
    for bad in ((0, 10, 600), (2, 0, 600), (2, 10, 0), (-1, 10, 600)):
        assert lib.st2_wave_dynamics_workspace_bytes(*bad) == 0
    far = C.c_void_p(4096 + (1 << 20))
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, params=D, A=3, win=D, rho=0.2, out=far, o_bs=6000, dyn=D,
                work=D, work_bytes=need)
    cases = [(dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
             (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"),
             (dict(o_bs=5999), "o_bs"), (dict(T_cap=1 << 22, spf=600), "too long"), (dict(A=-1), "A=-1"), (dict(A=65), "A=65"),
             (dict(win=None), "win is NULL"), (dict(rho=0.0), "rho"), (dict(rho=-0.2), "rho"), (dict(rho=INF), "rho"), (dict(rho=NAN), "rho"),
             (dict(work_bytes=need - 1), "too small"), (dict(out=D), "aliases"), (dict(out=C.c_void_p(4096 + 4 * 11000)), "aliases"),
             (dict(out=C.c_void_p(4096 - 4 * 11000 + (1 << 20)), wave=far), "aliases"),
             (dict(frames=C.c_void_p(4098)), "frames is not aligned")]
    cases += [({k: None}, "NULL") for k in ("params", "out", "dyn", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to float") for k in ("wave", "params", "win", "dyn", "work")]
    cases += [(dict(out=C.c_void_p(4098 + (1 << 20))), "not aligned to float")]
    for change, word in cases:
        assert _call(lib, dict(base, **change)) != 0, change
        assert _err(lib).startswith("st2_wave_dynamics:") and word in _err(lib), (change, _err(lib))
    # A = 0 needs no window; its refusals stay
    assert _call(lib, dict(base, A=0, win=None, rho=NAN)) != 0 and "rho" in _err(lib)


def test_wrapper_has_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_dynamics(w, f, torch.zeros(2, 4), None, A=0, rho=0.2)
    sig = inspect.signature(ops.wave_dynamics).parameters
    assert list(sig)[:4] == ["wave", "frames", "params", "win"] and {"A", "rho", "trim", "samples_per_frame", "dynamics"} <= set(sig)
    assert sig["A"].kind is inspect.Parameter.KEYWORD_ONLY and sig["rho"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- Dynamics ------------------------------------------------------------------------------------------------------------------
def test_dynamics_validates_and_keeps_one_table():
    d = pipeline.Dynamics(3, device="cpu")
    assert d.params.dtype == torch.float32 and tuple(d.params.shape) == (3, 4) and d.params.is_contiguous()
    assert torch.equal(d.params, torch.tensor([[-24.0, 1.0 - 1.0 / 3.0, 6.0, 0.0]] * 3))
    assert (d.A, d.rho) == (3, 80.0 * 64 / 24000) and d.options() == dict(attack_ms=8.0, release_db_per_s=80.0)
    d = pipeline.Dynamics(3, threshold_db=[-20, None, NAN], ratio=[1, INF, 4], knee_db=0, makeup_db=[-24, 0, 24], attack_ms=0,
                          release_db_per_s=2000, device="cpu")
    assert d.params[:, 1].tolist() == [0.0, 1.0, 0.75] and d.params[:, 2].tolist() == [0.0] * 3 and d.params[:, 3].tolist() == [-24.0, 0.0, 24.0]
    assert d.params[0, 0] == -20 and torch.isnan(d.params[1:, 0]).all() and d.A == 0 and d.rho == 2000 * 64 / 24000
    assert pipeline.Dynamics(1, attack_ms=170, device="cpu").A == 64
    part = d.slice(1, 3)
    assert part.B == 2 and part.params.data_ptr() == d.params[1].data_ptr() and (part.A, part.rho) == (d.A, d.rho)
    assert pipeline.Dynamics(1, threshold_db=None, device="cpu").params[0, 0].isnan()
    for bad in (dict(threshold_db=-70.5), dict(threshold_db=0.5), dict(threshold_db=INF), dict(ratio=0.99), dict(ratio=NAN),
                dict(ratio=None), dict(ratio=[3, None, 3]), dict(knee_db=-1), dict(knee_db=41), dict(knee_db=NAN), dict(makeup_db=-25),
                dict(makeup_db=25), dict(makeup_db=None), dict(attack_ms=-1), dict(attack_ms=171), dict(attack_ms=NAN),
                dict(release_db_per_s=0.5), dict(release_db_per_s=2001), dict(release_db_per_s=NAN), dict(threshold_db=[-20, -30]),
                dict(ratio=[2, 3, 4, 5])):
        with pytest.raises(ValueError, match="Dynamics"):
            pipeline.Dynamics(3, device="cpu", **bad)
    with pytest.raises(ValueError, match="Dynamics"):
        pipeline.Dynamics(0, device="cpu")
    sig = list(inspect.signature(pipeline.Dynamics.__init__).parameters)[1:]
    assert sig == ["B", "threshold_db", "ratio", "knee_db", "makeup_db", "attack_ms", "release_db_per_s", "device"]


# ---- the hand-over layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,fmt,more", list(itertools.product((1, 3), (False, True), (False, True), ("f32", "ulaw"),
                                                                         ({}, dict(with_level=True, with_limit=True, with_edges=True, with_breaks=True)))))
def test_layout_with_the_dynamics_part_and_without(B, marks, gaps, fmt, more):
    n_marks = B * 6 if marks else 0
    old = pipeline._HandOver(B, fmt, n_marks, gaps, **more)
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_dynamics=True, **more)
    names = ("offsets_at", "marks_at", "gaps_at", "level_at", "limit_at", "edges_at", "breaks_at", "dynamics_at")
    assert [getattr(lay, n) for n in names] == [getattr(old, n) for n in names]
    assert old.dynamics_at == old.breaks_at + (8 * B if more else 0) and old.samples_at == (old.dynamics_at + 15) // 16 * 16  # today's
    assert lay.samples_at == (lay.dynamics_at + 8 * B + 15) // 16 * 16
    ho = lay.allocate(10, "cpu")
    assert len(lay.views(ho.buf)) == 5 and ho.dynamics.dtype == torch.float32 and ho.dynamics.numel() == 2 * B
    assert ho.dynamics.data_ptr() - ho.buf.data_ptr() == lay.dynamics_at and ho.packed.data_ptr() - ho.buf.data_ptr() == lay.samples_at
    old.allocate(10, "cpu")
    assert old.dynamics is None and old.dynamics_view(old.buf) is None and old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize
    res = pipeline.SynthesisResult(torch.zeros(B, 1, 600), torch.ones(B, dtype=torch.int32), 1, pipeline._Output(fmt, 0), ho)
    assert tuple(res.dynamics.shape) == (B, 2) and res.dynamics.data_ptr() == ho.dynamics.data_ptr()
    plain = pipeline.SynthesisResult(torch.zeros(B, 1, 600), torch.ones(B, dtype=torch.int32), 1, pipeline._Output(fmt, 0), old)
    assert plain.dynamics is None
    with pytest.raises(ValueError, match="dynamics"):
        plain.to_host(dynamics=True)
    assert inspect.signature(pipeline.SynthesisResult.to_host).parameters["dynamics"].default is False


def test_output_spec_refuses_dynamics_in_the_one_place():
    d = pipeline.Dynamics(3, device="cpu")
    for kw, word in ((dict(capacity=True, pack=None), "pass max_frames and pack"), (dict(capacity=False, pack="s16"), "pass max_frames and pack"),
                     (dict(capacity=True, pack="s16", dynamics=pipeline.Dynamics(2, device="cpu")), "Dynamics of 3 rows"),
                     (dict(capacity=True, pack="s16", dynamics=True), "Dynamics of 3 rows")):
        with pytest.raises(ValueError, match=word):
            pipeline._output_spec(3, **dict(dict(dynamics=d), **kw))
    spec, _ = pipeline._output_spec(3, True, "s16", dynamics=d)
    assert spec == pipeline._output_spec(3, True, "s16")[0], "the spec does not carry it"
    for f in (pipeline.inference, pipeline.synthesize_long, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__):
        assert inspect.signature(f).parameters["dynamics"].default is None, f
    with pytest.raises(ValueError, match="max_frames"):
        pipeline.synthesize_long(None, None, [torch.zeros(3, dtype=torch.int64)], dynamics=d)


# ---- routing ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def spied(monkeypatch):
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append((name, wave, frames, kw))
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps", "wave_pack_level"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(ops, "wave_level", lambda wave, frames, target, **kw: seen.append(("wave_level", wave, frames, kw)) or kw["out"])

    def limit(wave, frames, level, target, win, **kw):
        seen.append(("wave_limit", wave, frames, kw))
        return torch.full_like(wave, 5.0), kw["limit"]

    def breaks(wave, frames, pos, brk, max_break, ramp=None, **kw):
        seen.append(("wave_breaks", wave, frames, kw))
        kw["breaks"].copy_(10 + torch.arange(kw["breaks"].numel(), dtype=torch.int32))
        return torch.full((wave.shape[0], wave.shape[-1] + max_break), 4.0), "ins", None, kw["breaks"]

    def dynamics(wave, frames, params, win, **kw):
        seen.append(("wave_dynamics", wave, frames, dict(kw, params=params, win=win)))
        return torch.full((wave.shape[0], wave.shape[-1]), 6.0), kw["dynamics"]
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_breaks", breaks)
    monkeypatch.setattr(ops, "wave_dynamics", dynamics)
    monkeypatch.setattr(ops, "token_marks", lambda dur, frames, T_cap, **kw: seen.append(("token_marks", dur, frames, kw)) or "pos")
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    monkeypatch.setattr(pipeline.resample, "limit_window", lambda W, dev: torch.from_numpy(resample.limit_window_design(W)))
    monkeypatch.setattr(pipeline.resample, "edge_ramp", lambda F, dev: torch.from_numpy(resample.edge_ramp_design(F)))
    return seen


@pytest.mark.parametrize("with_breaks,gaps,fmt,rate,level", list(itertools.product((False, True), (False, True), ("s16", "ulaw"), (None, 8000),
                                                                                   (None, "plain", "limiter"))))
def test_hand_over_compresses_behind_the_breaks_and_in_front_of_the_level(spied, with_breaks, gaps, fmt, rate, level):
    B, N, L, spf, max_gap = 3, 4, 1200, 600, 7
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = None if level is None else pipeline.Level(B, device="cpu", limiter=level == "limiter")
    more = {}
    if with_breaks:
        more = dict(breaks=pipeline.Breaks(B, N, ms=[[0, 10, 0, 0]] * B, max_ms=100, device="cpu"),
                    tokens=dict(dur="dur", frames=frames, T_cap=2, lengths="lens", shift=True, trim=50, samples_per_frame=spf))
    dy = pipeline.Dynamics(B, threshold_db=[-20, None, -30], attack_ms=16.0, release_db_per_s=120.0, device="cpu")
    args = (wave, frames, 50, fmt, spf, rate)
    kw = dict(n_marks=B * (N + 1), gaps=g, max_gap=max_gap if gaps else 0, level=lv, **more)
    old = pipeline._hand_over_edges(*args, **kw)
    before = [s[0] for s in spied]
    assert "wave_dynamics" not in before and old.dynamics is None, "nothing new is called without the option"
    del spied[:]
    ho = pipeline._hand_over_edges(*args, dynamics=dy, **kw)
    at = 2 if with_breaks else 0
    assert [s[0] for s in spied] == before[:at] + ["wave_dynamics"] + before[at:], "behind the breaks, in front of the level and the rest"
    _, w, f, k = spied[at]
    if with_breaks:
        assert bool((w == 4.0).all()) and f.tolist() == [10, 12, 14] and k["trim"] == 0 and k["samples_per_frame"] == 1
    else:
        assert w is wave and f is frames and k["trim"] == 50 and k["samples_per_frame"] == spf
    assert k["params"] is dy.params and k["A"] == 6 and k["win"].numel() == 13 and k["rho"] == 120.0 * 64 / 24000
    assert k["dynamics"].data_ptr() == ho.dynamics.data_ptr() and ho.dynamics.numel() == 2 * B
    for name, w, f, k2 in spied[at + 1:]:
        limited = level == "limiter" and name not in ("wave_level", "wave_limit")  # the packers read the limiter's rows
        assert bool((w == (5.0 if limited else 6.0)).all()), (name, "everything behind reads the compressed rows")
        assert k2["trim"] == k["trim"] and k2["samples_per_frame"] == k["samples_per_frame"] and (f is spied[at][2] or f.tolist() == spied[at][2].tolist())
    assert ho.packed.numel() == old.packed.numel() and ho.samples_at >= old.samples_at, "sample counts do not change"
    # no attack: no window
    del spied[:]
    pipeline._hand_over_edges(*args, dynamics=pipeline.Dynamics(B, attack_ms=0, device="cpu"), **kw)
    assert spied[at][3]["win"] is None and spied[at][3]["A"] == 0


# ---- the contract ------------------------------------------------------------------------------------------------------------------
RHO = 80.0 * 64 / 24000


def _noise(n, seed, amp=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def _win(A):
    return None if A == 0 else resample.limit_window_design(A)


@pytest.mark.parametrize("n,A,p", [(1, 0, (-24, 0.66, 6, 0)), (63, 1, (-30, 1.0, 0, 2)), (64, 2, (-30, 0.5, 12, -3)), (200, 3, (-24, 0.66, 6, 0)),
                                   (700, 5, (-40, 0.9, 40, 1)), (333, 0, (-26, 0.75, 3, 0)), (450, 64, (-30, 0.5, 6, 0))])
def test_contract_agrees_with_a_plain_loop(n, A, p):
    x = _noise(n, n + A) * np.float32(10.0) ** (np.linspace(-2, 0.5, n).astype(np.float32))
    if n > 100:
        x[n // 2] = np.nan
        x[5] = np.inf
    out, dyn, st = R.reference_row(x, p, A, _win(A), RHO)
    b_out, b_dyn = R.brute_row(x, p, A, _win(A), RHO)
    assert np.array_equal(out.view(np.uint32), b_out.view(np.uint32)) and np.array_equal(dyn, b_dyn)
    assert st["lin"].dtype == np.float32 and len(st["lin"]) == (n + 63) // 64 and (n == 1 or dyn[1] > 0)
    assert np.array_equal(np.isnan(out), np.isnan(x))


def test_a_row_under_the_threshold_is_bit_identical_and_ratio_one_is_the_makeup_gain():
    x = _noise(5000, 1, 0.01)  # -40 dBFS against a threshold of -24 with a knee of 6
    x[17] = np.nan
    out, dyn, st = R.reference_row(x, (-24.0, 0.9, 6.0, 0.0), 3, _win(3), RHO)
    assert (st["lin"] == 1.0).all() and np.array_equal(out.view(np.uint32), x.view(np.uint32)) and dyn.tolist() == [0.0, 0.0]
    loud = _noise(5000, 2, 0.5)
    out, dyn, st = R.reference_row(loud, (-24.0, 0.0, 6.0, 4.0), 3, _win(3), RHO)
    g = np.float32(10.0 ** (4.0 / 20.0))
    assert (st["lin"] == g).all() and np.array_equal(out, loud * g) and dyn.tolist() == [0.0, 0.0]
    # left alone: a NaN anywhere, a threshold that is not finite, an empty row
    for p in ((NAN, 0.5, 6, 0), (-24, NAN, 6, 0), (-24, 0.5, NAN, 0), (-24, 0.5, 6, NAN), (INF, 0.5, 6, 0), (-INF, 0.5, 6, 0)):
        out, dyn, st = R.reference_row(loud, p, 3, _win(3), RHO)
        assert st is None and np.array_equal(out, loud) and dyn.tolist() == [0.0, 0.0]
    assert R.reference_row(loud[:0], (-24, 0.5, 6, 0), 3, _win(3), RHO)[2] is None
    # the clamps
    assert R.row_params((-24, 1.5, 90, -30))[2:] == (1.0, 40.0, -24.0) and R.row_params((-24, -0.5, -1, 30))[2:] == (0.0, 0.0, 24.0)


@pytest.mark.parametrize("A", [0, 1, 3, 64])
def test_no_block_is_reduced_by_less_than_the_curve_asks(A):
    """d' >= g holds exactly (it is a maximum with g); g >= c up to the two roundings of rule 5, z = fl(c + k rho) and g = fl(P -
    k rho), each half an ulp of a number no larger than c + k rho."""
    x = _noise(64 * 600, 3) * np.repeat(10.0 ** (np.random.default_rng(4).uniform(-3, 0.3, 600) / 1.0), 64).astype(np.float32)
    st = R.row_stages(x, (-30.0, 0.8, 6.0, 0.0), A, _win(A), RHO)
    assert (st["c"] >= 0).all() and (st["dp"] >= st["g"]).all() and (st["c"] > 0).sum() > 50
    slack = np.spacing(st["c"] + np.arange(600) * RHO)
    assert (st["dp"] >= st["c"] - slack).all()
    assert (st["lin"] <= 1.0).all() and (st["lin"] > 0).all()


def test_after_a_burst_the_reduction_falls_by_rho_per_block_until_it_meets_the_curve():
    rho = 0.25  # exact in binary, so that P - k rho falls by exactly rho
    x = np.concatenate([_noise(64 * 20, 5, 0.5), _noise(64 * 200, 6, 0.0005), _noise(64 * 30, 7, 0.02)])
    st = R.row_stages(x, (-40.0, 1.0, 0.0, 0.0), 0, None, rho)  # A = 0: d' = g
    c, g = st["c"], st["dp"]
    assert (c[22:218] == 0).all() and c[:20].min() > 20 and 3 < c[225] < 12
    top = int(np.argmax(c[:22] + np.arange(22) * rho))
    k = np.arange(top, 218)
    assert np.array_equal(g[top:218], np.maximum(g[top] - (k - top) * rho, 0.0)), "a straight line in dB down to the curve, which is 0 here"
    assert (np.diff(g[top:top + 100]) == -rho).all() and g[top] > 100 * rho and (g[180:218] == 0).all()
    slack = np.spacing(c + np.arange(250) * rho)  # the two roundings of rule 5
    assert (g[218:] >= c[218:] - slack[218:]).all() and abs(g[220] - c[220]) <= slack[220] and c[220] > c[219] + 2, "and the attack is instant"


@pytest.mark.parametrize("over,slope", [(6.0, 0.5), (12.0, 2.0 / 3.0), (20.0, 1.0)])
def test_a_steady_sine_over_the_threshold_is_reduced_by_slope_times_the_excess(over, slope):
    """A sine of amplitude a at f = 1 kHz, fs = 24 kHz: its mean square over a window of N = 192 samples is a^2 / 2 (1 - r) with
    |r| <= |sin(N w)| / (N sin w) <= 1 / (N sin w), w = 2 pi f / fs -- the ripple of the 192-sample RMS.  In dB the level is off by
    at most 10 log10(1 + 1 / (N sin w)) = 0.087 dB either way, and the reduction, slope times the level past the knee, by no more
    than that times the slope; the fp32 sums add less than 1e-5 dB.  (192 samples are exactly 8 periods here, so the ripple
    itself nearly vanishes; the bound does not rely on that.)"""
    T, fs, f, N = -30.0, 24000.0, 1000.0, 192
    w = 2 * np.pi * f / fs
    a = np.sqrt(2.0) * 10.0 ** ((T + over) / 20.0)  # RMS = T + over dB
    x = (a * np.sin(w * np.arange(64 * 400) + 0.3)).astype(np.float32)
    st = R.row_stages(x, (T, slope, 4.0, 0.0), 3, _win(3), RHO)
    tol = slope * 10.0 * np.log10(1.0 + 1.0 / (N * np.sin(w))) + 1e-4
    inner = slice(8, 392)  # away from the row's edges, whose windows are part zeros
    assert np.abs(st["dp"][inner] - slope * over).max() <= tol, (np.abs(st["dp"][inner] - slope * over).max(), tol)
    assert np.abs(-20.0 * np.log10(st["lin"][inner].astype(np.float64)) - slope * over).max() <= tol + 1e-5
    assert (st["L"][[0, -1]] < st["L"][10] - 1.5).all(), "the first and the last block are divided by 192 like the others"


@pytest.mark.parametrize("chunk", [1, 2, 7, 64, 255, 256, 1024])
def test_the_release_does_not_depend_on_how_the_scan_is_cut(chunk):
    c = np.maximum(np.random.default_rng(8).normal(0.0, 6.0, 3000), 0.0)
    assert np.array_equal(R.release(c, RHO), R.release(c, RHO, chunk))
    z = c + np.arange(3000) * RHO
    assert np.array_equal(R.release(c, RHO), np.array([z[:k + 1].max() for k in range(3000)]) - np.arange(3000) * RHO)


def test_fma_rounds_once_and_the_gain_is_exact_at_the_block_centres():
    g = np.random.default_rng(9)
    t = (g.integers(0, 64, 4000) * 2 + 1).astype(np.float32) / np.float32(128)
    d = g.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** g.integers(-30, 3, 4000).astype(np.float32)
    a = g.standard_normal(4000).astype(np.float32)
    from fractions import Fraction

    def nearest(q):  # the fp32 value nearest to the exact rational q: the best of the doubly rounded one and its two neighbours
        c = np.float32(float(q))
        return min((c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))), key=lambda v: abs(Fraction(float(v)) - q))
    want = np.array([nearest(Fraction(float(ti)) * Fraction(float(di)) + Fraction(float(ai))) for ti, di, ai in zip(t, d, a)], dtype=np.float32)
    assert np.array_equal(R._fma32(t, d, a), want)
    lin = np.array([1.0, 0.5, 0.25], dtype=np.float32)
    gain = R.sample_gain(lin, 190)
    assert (gain[:32] == 1.0).all() and (gain[160:] == 0.25).all() and gain[63] == np.float32(1.0 - 0.5 * 63 / 128)
    assert gain[32] == np.float32(1.0 - 0.5 / 128) and (np.diff(gain[31:161].astype(np.float64)) < 0).all()
