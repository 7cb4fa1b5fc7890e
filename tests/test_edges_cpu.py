"""C ABI and host-side contract of the edge trim of the hand-over: `st2_wave_edges`, its helpers and
`st2_token_marks_edges` are declared, exported and bound under ABI 23 and refuse bad arguments before any launch; `Edges` and
`_output_spec` refuse what they must; the hand-over layout gains its seventh part without moving the other six; the numpy
contract of tests/_edges_ref.py agrees with a plain loop over samples in exact arithmetic; `_hand_over_edges` runs `ops.wave_edges`
first and everything behind it over rows of one-sample frames, and without `edges` reaches the ops it reached before.  No GPU."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _edges_ref as E
from styletts2_amd import _build, _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_wave_edges", "st2_wave_edges_workspace_bytes", "st2_wave_edges_tile", "st2_token_marks_edges")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b(int|int32_t|int64_t) %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert lib.st2_wave_edges_tile() == ops.EDGES_TILE == 2048
    assert "st2_edges.hip" in _build.SOURCES and _build.EXTRA_FLAGS["st2_edges.hip"] == _build.EXTRA_FLAGS["st2_ingest.hip"]
    # the trim rule is stated once, in the header both directions include
    src = lambda n: open(os.path.join(ROOT, "styletts2_amd", "csrc", n)).read()
    assert '#include "st2_trim.h"' in src("st2_ingest.hip") and '#include "st2_trim.h"' in src("st2_edges.hip")
    assert "1e-10f" in src("st2_trim.h") and "1e-10f" not in src("st2_ingest.hip") and "1e-10f" not in src("st2_edges.hip")


D = C.c_void_p(4096)
ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "top_db", "keep", "ramp", "F", "out", "edges", "work", "work_bytes")


def test_wave_edges_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_edges_workspace_bytes(2, 10, 600)
    assert need == 4 * 2 * 4 * 3  # the block sums of ceil(6000 / 2048) = 3 tiles of four blocks, per row
    assert lib.st2_wave_edges_workspace_bytes(3, 1, 5) == (4 * 3 * 4 + 15) // 16 * 16
    assert lib.st2_wave_edges_workspace_bytes(0, 10, 600) == 0 and lib.st2_wave_edges_workspace_bytes(2, 10, 0) == 0
    far = C.c_void_p(4096 + (1 << 20))
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, top_db=D, keep=D, ramp=D, F=48, out=far, edges=D, work=D,
                work_bytes=need)
    cases = [(dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
             (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"),
             (dict(T_cap=1 << 30, spf=2), "too long"), (dict(F=-1), "F=-1"), (dict(F=4097), "F=4097"), (dict(ramp=None), "ramp is NULL"),
             (dict(work_bytes=need - 1), "too small"), (dict(out=D), "aliases"), (dict(out=C.c_void_p(4096 + 4 * 11000)), "aliases"),
             (dict(out=C.c_void_p(4098 + (1 << 20))), "not aligned to float")]
    cases += [({k: None}, "NULL") for k in ("top_db", "keep", "out", "edges", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to float") for k in ("wave", "top_db", "ramp", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to int32") for k in ("frames", "keep", "edges")]
    for change, word in cases:
        a = dict(base, **change)
        assert lib.st2_wave_edges(*[a[k] for k in ORDER], None) != 0, change
        assert _err(lib).startswith("st2_wave_edges:") and word in _err(lib), (change, _err(lib))


def test_token_marks_edges_validates_before_any_launch():
    lib = _lib.load()
    base = [D, 2, 8, None, None, 10, 0, 600, 0, 1, 1, D, None]
    assert lib.st2_token_marks_edges(*base, None, None) != 0 and "edges is NULL" in _err(lib)
    assert lib.st2_token_marks_edges(*base, C.c_void_p(4098), None) != 0 and "not aligned" in _err(lib)
    for at, value, word in ((0, None, "NULL"), (11, None, "NULL"), (2, 513, "512"), (9, 0, "up=0"), (8, -1, "negative"), (1, 0, "geometry")):
        a = list(base)
        a[at] = value
        assert lib.st2_token_marks_edges(*a, D, None) != 0 and _err(lib).startswith("st2_token_marks_edges:") and word in _err(lib), at
        assert lib.st2_token_marks(*a, None) != 0 and _err(lib).startswith("st2_token_marks:") and word in _err(lib), at


def test_wrappers_have_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_edges(w, f, torch.zeros(2), torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(_lib.St2Error):
        ops.token_marks_edges(torch.zeros(2, 4, dtype=torch.int64), f, 2, torch.zeros(2, 2, dtype=torch.int32))
    sig = list(inspect.signature(ops.wave_edges).parameters)
    assert sig[:5] == ["wave", "frames", "top_db", "keep", "ramp"] and {"trim", "samples_per_frame", "out", "edges", "workspace"} <= set(sig)
    assert list(inspect.signature(ops.token_marks_edges).parameters)[:4] == ["dur", "frames", "T_cap", "edges"]


# ---- Edges and the spec ----------------------------------------------------------------------------------------------------------------
def test_edges_object_validates_on_the_host_and_slices():
    e = pipeline.Edges(3, device="cpu")
    assert e.top_db.tolist() == [40.0] * 3 and e.keep.tolist() == [[240, 720]] * 3 and e.F == 48 and e.keep.dtype == torch.int32
    assert list(inspect.signature(pipeline.Edges.__init__).parameters)[1:] == ["B", "top_db", "lead_ms", "tail_ms", "fade_ms", "device"]
    e = pipeline.Edges(3, top_db=[20.0, None, 120.0], lead_ms=0, tail_ms=500, fade_ms=0, device="cpu")
    t = e.top_db.numpy()
    assert t[0] == 20.0 and np.isnan(t[1]) and t[2] == 120.0 and e.keep.tolist() == [[0, 12000]] * 3 and e.F == 0
    part = e.slice(1, 3)
    assert part.B == 2 and part.F == 0 and part.keep.shape == (2, 2) and part.top_db.data_ptr() == e.top_db.data_ptr() + 4
    assert part.options() == dict(lead_ms=0.0, tail_ms=500.0, fade_ms=0.0)
    assert np.isnan(pipeline.Edges(2, top_db=float("nan"), device="cpu").top_db.numpy()).all()
    for bad in (dict(top_db=0.0), dict(top_db=-3.0), dict(top_db=120.5), dict(top_db=[20.0, 30.0]), dict(lead_ms=-1), dict(lead_ms=501),
                dict(tail_ms=float("nan")), dict(tail_ms=500.5), dict(fade_ms=-0.1), dict(fade_ms=171), dict(fade_ms=501)):
        with pytest.raises(ValueError, match="Edges"):
            pipeline.Edges(3, device="cpu", **bad)
    with pytest.raises(ValueError, match="Edges"):
        pipeline.Edges(0, device="cpu")
    assert pipeline.Edges(1, fade_ms=170, device="cpu").F == 4080 <= resample.EDGE_MAX_F == 4096


def test_edge_ramp_is_rising_positive_and_complementary():
    for F in (1, 2, 48, 4096):
        r = resample.edge_ramp_design(F)
        assert r.dtype == np.float32 and r.shape == (F,) and (r > 0).all() and (r < 1).all() and (np.diff(r) > 0).all()
        assert np.abs(r.astype(np.float64) + r[::-1] - 1.0).max() <= 2.0 ** -23
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            resample.edge_ramp_design(bad)


def test_output_spec_refuses_edges_in_the_one_place():
    e = pipeline.Edges(3, device="cpu")
    for kw, word in ((dict(capacity=True, pack=None), "pass max_frames and pack"), (dict(capacity=False, pack="s16"), "pass max_frames and pack"),
                     (dict(capacity=True, pack="s16", edges=pipeline.Edges(2, device="cpu")), "Edges of 3 rows"),
                     (dict(capacity=True, pack="s16", edges=40.0), "Edges of 3 rows")):
        kw = dict(dict(edges=e), **kw)
        with pytest.raises(ValueError, match=word):
            pipeline._output_spec(3, kw.pop("capacity"), **kw)
    spec, _ = pipeline._output_spec(3, True, pack="s16", trim=0, edges=e)
    assert spec == pipeline._output_spec(3, True, pack="s16", trim=0)[0]
    for f in (pipeline.inference, pipeline.synthesize_long, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__):
        assert inspect.signature(f).parameters["edges"].default is None, f
    assert inspect.signature(pipeline.SynthesisResult.to_host).parameters["edges"].default is False
    with pytest.raises(ValueError, match="max_frames"):
        pipeline.synthesize_long(None, None, [torch.zeros(3, dtype=torch.long)], edges=pipeline.Edges(1, device="cpu"))


# ---- the hand-over layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,level,limit,fmt", [c for c in itertools.product(
    (1, 3), (False, True), (False, True), (False, True), (False, True), ("f32", "ulaw")) if c[3] or not c[4]])  # a limit part has a level part
def test_layout_with_the_edges_part_and_without(B, marks, gaps, level, limit, fmt):
    n_marks = B * 6 if marks else 0
    old = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=level, with_limit=limit)
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=level, with_limit=limit, with_edges=True)
    for name in ("offsets_at", "marks_at", "gaps_at", "level_at", "limit_at", "edges_at"):
        assert getattr(lay, name) == getattr(old, name), name
    assert lay.edges_at == lay.limit_at + (8 * B if limit else 0) and lay.samples_at == (lay.edges_at + 8 * B + 15) // 16 * 16
    assert old.samples_at == (old.edges_at + 15) // 16 * 16  # today's, byte for byte
    ho = lay.allocate(10, "cpu")
    assert len(lay.views(ho.buf)) == 5 and ho.edges.dtype == torch.int32 and ho.edges.numel() == 2 * B
    assert ho.edges.data_ptr() - ho.buf.data_ptr() == lay.edges_at and ho.packed.data_ptr() - ho.buf.data_ptr() == lay.samples_at
    assert (ho.limit is None) == (not limit) and (ho.level is None) == (not level)
    old.allocate(10, "cpu")
    assert old.edges is None and old.edges_view(old.buf) is None and old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize


# ---- the contract against a plain loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,trim,F", [((5, 700), 3, 48), ((600, 8), 0, 1), ((600, 8), 3, 0)])
def test_contract_agrees_with_a_per_sample_loop(geo, trim, F):
    spf, T_cap = geo
    c = E.batch(17, spf, T_cap, trim)
    ref = E.reference(17, spf, T_cap, trim, F)
    ramp = resample.edge_ramp_design(F) if F else None
    x = c["wave"][c["names"].index("tile edge")]
    assert x[ops.EDGES_TILE - 1] != 0 and x[ops.EDGES_TILE] != 0, "that row's burst lies across the tile of the sums' launch"
    for b in (0, 1, 3, 4, 5, 6, 9, 10, 11, 12):
        n = E.row_samples(c["frames"][b], T_cap, spf, trim)
        want = E.brute_row(c["wave"][b, :n], c["top_db"][b], c["keep"][b], ramp)
        got = ref[b]
        assert (got["start"], got["end"], got["head"], got["count"]) == (want["start"], want["end"], want["head"], want["count"]), c["names"][b]
        assert np.array_equal(got["bits"], want["bits"]), c["names"][b]


def test_contract_on_the_sizes_and_its_properties():
    c = E.sizes_batch()
    ramp = resample.edge_ramp_design(700)
    ref = E.reference(0, 1, c["T_cap"], 0, 700)
    for b, n in enumerate(E.SIZES):
        want = E.brute_row(c["wave"][b, :n], c["top_db"][b], c["keep"][b], ramp)
        assert (ref[b]["head"], ref[b]["count"]) == (want["head"], want["count"]) and np.array_equal(ref[b]["bits"], want["bits"]), n
    r = ref[5]  # 2048 samples, cut in front: a fade of count div 2 at the head, none at the tail, the middle copied
    x = c["wave"][5, :2048]
    f = r["count"] // 2
    assert r["head"] == 1024 - 3 and r["head"] + r["count"] == 2048 and f < 700
    assert np.array_equal(r["bits"][f:], x[r["head"] + f:].view(np.uint32))
    assert np.array_equal(r["bits"][:f], (x[r["head"]:r["head"] + f] * ramp[:f]).view(np.uint32))
    # round32 / fma32: one rounding, ties to even
    one, ulp = np.float32(1.0), np.float32(2.0 ** -24)
    a = np.array([1.0 + 2.0 ** -12], dtype=np.float32)  # a^2 = 1 + 2^-11 + 2^-24: a tie broken by the addend
    assert E.fma32(a, a, np.array([ulp * ulp], dtype=np.float32))[0] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert E.fma32(a, a, np.array([0.0], dtype=np.float32))[0] == np.float32(1.0 + 2.0 ** -11)
    import fractions
    assert E.round32(fractions.Fraction(float(a[0])) ** 2 + fractions.Fraction(float(ulp)) ** 2) == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert E.round32(fractions.Fraction(float(a[0])) ** 2) == np.float32(1.0 + 2.0 ** -11) and E.round32(fractions.Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148)
    # a NaN with a payload is copied, the measurement counts it as 0
    c17 = E.batch(17, 600, 8, 0)
    got = E.reference(17, 600, 8, 0, 48)[6]
    assert c17["names"][6] == "non-finite" and E.NAN_PAYLOAD in got["bits"].tolist() and got["count"] < 4800


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
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

    def edges(wave, frames, top_db, keep, ramp=None, **kw):
        seen.append(("wave_edges", wave, frames, dict(kw, top_db=top_db, keep=keep, ramp=ramp)))
        kw["edges"].copy_(torch.arange(kw["edges"].numel(), dtype=torch.int32))
        return torch.full_like(wave[:, 0], 3.0), kw["edges"]
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_edges", edges)
    monkeypatch.setattr(ops, "token_marks", lambda *a, **kw: seen.append(("token_marks", None, None, kw)))
    monkeypatch.setattr(ops, "token_marks_edges", lambda *a, **kw: seen.append(("token_marks_edges", None, None, kw)))
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    monkeypatch.setattr(pipeline.resample, "limit_window", lambda W, dev: torch.from_numpy(resample.limit_window_design(W)))
    monkeypatch.setattr(pipeline.resample, "edge_ramp", lambda F, dev: torch.from_numpy(resample.edge_ramp_design(F)))
    return seen


@pytest.mark.parametrize("gaps,fmt,rate,level", list(itertools.product((False, True), ("s16", "ulaw"), (None, 8000), (None, "plain", "limiter"))))
def test_hand_over_trims_first_and_runs_the_rest_over_one_sample_frames(spied, gaps, fmt, rate, level):
    B, L, spf, max_gap = 3, 1200, 600, 7
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = None if level is None else pipeline.Level(B, device="cpu", limiter=level == "limiter")
    e = pipeline.Edges(B, top_db=[20.0, None, 60.0], device="cpu")
    args = (wave, frames, 50, fmt, spf, rate)
    kw = dict(n_marks=B * 4, gaps=g, max_gap=max_gap if gaps else 0, level=lv)
    old = pipeline._hand_over(*args, **kw)
    before = [s[0] for s in spied]
    assert "wave_edges" not in before and old.edges is None and all(s[3]["trim"] == 50 and s[3]["samples_per_frame"] == spf for s in spied)
    del spied[:]
    ho = pipeline._hand_over_edges(*args, edges=e, **kw)
    assert [s[0] for s in spied] == ["wave_edges"] + before, "the stage runs first, the rest is the call without it"
    _, w, f, k = spied[0]
    assert w is wave and f is frames and k["trim"] == 50 and k["samples_per_frame"] == spf and k["top_db"] is e.top_db and k["keep"] is e.keep
    assert k["ramp"].numel() == 48 and k["edges"].data_ptr() == ho.edges.data_ptr()
    for name, w, f, k in spied[1:]:
        limited = level == "limiter" and name not in ("wave_level", "wave_limit")  # the packers read the limiter's rows
        assert bool((w == (5.0 if limited else 3.0)).all()), name
        assert f.tolist() == [1, 3, 5] and f.is_contiguous() and k["trim"] == 0 and k["samples_per_frame"] == 1, name
    assert ho.buf.numel() == old.buf.numel() + (ho.samples_at - old.samples_at) and ho.packed.numel() == old.packed.numel()
    res = pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output(fmt, 50), ho)
    assert tuple(res.edges.shape) == (B, 2) and res.edges.data_ptr() == ho.edges.data_ptr()
    with pytest.raises(ValueError, match="edges"):
        pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output(fmt, 50), old).to_host(edges=True)
    # an Edges without a fade passes no ramp
    del spied[:]
    pipeline._hand_over_edges(*args, edges=pipeline.Edges(B, fade_ms=0, device="cpu"), **kw)
    assert spied[0][3]["ramp"] is None
