"""C ABI and host-side contract of the pauses inside a row: `st2_wave_breaks`, its helper and
`st2_token_marks_breaks` are declared, exported and bound under ABI 23 and refuse bad arguments before any launch; `Breaks`,
`break_samples` and `_output_spec` refuse what they must; the hand-over layout gains its eighth part without moving the other
seven; the numpy contract of tests/_breaks_ref.py agrees with a plain loop over samples; `_hand_over_edges` runs `ops.wave_breaks`
behind `ops.wave_edges` and everything else over rows of one-sample frames, and without `breaks` reaches the ops it reached
before.  No GPU."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _breaks_ref as R
from styletts2_amd import _build, _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_wave_breaks", "st2_wave_breaks_workspace_bytes", "st2_token_marks_breaks")


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
    assert "st2_breaks.hip" in _build.SOURCES and _build.EXTRA_FLAGS["st2_breaks.hip"] == _build.EXTRA_FLAGS["st2_edges.hip"]


D = C.c_void_p(4096)
ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "pos", "brk", "N", "max_break", "ramp", "F", "out", "o_bs", "ins", "cuts",
         "breaks", "work", "work_bytes")


def test_wave_breaks_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_breaks_workspace_bytes(2, 10, 600, 7)
    assert need == 4 * 2 * (32 * 3 + 1032)  # the block sums of ceil(6000 / 2048) = 3 tiles of 32 blocks and one table, per row
    assert lib.st2_wave_breaks_workspace_bytes(3, 1, 5, 1) == (4 * 3 * (32 + 1032) + 15) // 16 * 16
    for bad in ((0, 10, 600, 7), (2, 0, 600, 7), (2, 10, 0, 7), (2, 10, 600, 0), (2, 10, 600, 513)):
        assert lib.st2_wave_breaks_workspace_bytes(*bad) == 0, bad
    far = C.c_void_p(4096 + (1 << 20))
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, pos=D, brk=D, N=7, max_break=100, ramp=D, F=48, out=far,
                o_bs=6100, ins=D, cuts=D, breaks=D, work=D, work_bytes=need)
    cases = [(dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
             (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"),
             (dict(T_cap=1 << 30, spf=2), "too long"), (dict(F=-1), "F=-1"), (dict(F=4097), "F=4097"), (dict(ramp=None), "ramp is NULL"),
             (dict(work_bytes=need - 1), "too small"), (dict(out=D), "aliases"), (dict(out=C.c_void_p(4096 + 4 * 11000)), "aliases"),
             (dict(out=C.c_void_p(4098 + (1 << 20))), "not aligned to float"),
             # what this entry adds
             (dict(N=0), "N=0"), (dict(N=513), "N=513"), (dict(max_break=-1), "max_break=-1"), (dict(o_bs=6099), "o_bs"),
             (dict(max_break=2 ** 31 - 6001), "too long"), (dict(T_cap=3000000, max_break=2 ** 31 - 3000000 * 600 - 4000), "too long")]
    cases += [({k: None}, "NULL") for k in ("pos", "brk", "ins", "cuts", "breaks", "out", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to float") for k in ("wave", "ramp", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to int32") for k in ("frames", "pos", "brk", "ins", "cuts", "breaks")]
    for change, word in cases:
        a = dict(base, **change)
        if "T_cap" in change:
            a.update(w_bs=a["T_cap"] * a["spf"], o_bs=2 ** 31)
        assert lib.st2_wave_breaks(*[a[k] for k in ORDER], None) != 0, change
        assert _err(lib).startswith("st2_wave_breaks:") and word in _err(lib), (change, _err(lib))


def test_token_marks_breaks_validates_before_any_launch():
    lib = _lib.load()
    base = [D, D, 2, 8, 1, 1, D]
    for at, value, word in ((0, None, "NULL"), (1, None, "NULL"), (6, None, "NULL"), (0, C.c_void_p(4098), "not aligned"),
                            (1, C.c_void_p(4098), "not aligned"), (6, C.c_void_p(4098), "not aligned"), (2, 0, "geometry"),
                            (3, 0, "geometry"), (3, 513, "geometry"), (4, 0, "up=0"), (4, 1025, "up=1025"), (5, 0, "down=0"),
                            (5, 1025, "down=1025")):
        a = list(base)
        a[at] = value
        assert lib.st2_token_marks_breaks(*a, None) != 0 and _err(lib).startswith("st2_token_marks_breaks:") and word in _err(lib), at


def test_wrappers_have_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    pos, brk = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_breaks(w, f, pos, brk, 100)
    with pytest.raises(_lib.St2Error):
        ops.token_marks_breaks(pos, brk)
    sig = list(inspect.signature(ops.wave_breaks).parameters)
    assert sig[:6] == ["wave", "frames", "pos", "brk", "max_break", "ramp"]
    assert {"trim", "samples_per_frame", "out", "ins", "cuts", "breaks", "workspace"} <= set(sig)
    assert list(inspect.signature(ops.token_marks_breaks).parameters) == ["pos", "ins", "rate", "out"]


# ---- Breaks and the spec ----------------------------------------------------------------------------------------------------------
def test_breaks_object_validates_on_the_host_and_slices():
    assert list(inspect.signature(pipeline.Breaks.__init__).parameters)[1:] == ["B", "N", "ms", "samples", "fade_ms", "max_ms", "device"]
    b = pipeline.Breaks(3, 4, device="cpu")
    assert b.samples.dtype == torch.int32 and b.samples.tolist() == [[0] * 4] * 3 and b.F == 48 and b.max_break == 48000
    b = pipeline.Breaks(2, 3, ms=[[0, 300, 0.02], [12.5, -1, 0]], fade_ms=0, max_ms=500, device="cpu")
    assert b.samples.tolist() == [[0, 7200, 0], [300, -24, 0]] and b.F == 0 and b.max_break == 12000
    assert isinstance(b.max_break, int) and b.options() == dict(fade_ms=0.0, max_ms=500.0)
    b = pipeline.Breaks(3, 2, samples=[[1, 2], [3, 4], [5, 6]], device="cpu")
    part = b.slice(1, 3)
    assert (part.B, part.N, part.F, part.max_break) == (2, 2, 48, 48000) and part.samples.data_ptr() == b.samples.data_ptr() + 8
    assert pipeline.break_samples(300) == 7200 and pipeline.break_samples([[300, 0.02], [12.5]]) == [[7200, 0], [300]]
    assert pipeline.break_samples(0.0625) == 2 and pipeline.break_samples(0.1875) == 4  # 1.5 and 4.5 samples: half to even
    for bad in (dict(B=0), dict(N=0), dict(N=513), dict(ms=[[1.0]] * 3), dict(ms=[[float("nan")] * 4] * 3), dict(samples=[[0.5] * 4] * 3),
                dict(samples=[[2 ** 31] * 4] * 3), dict(ms=[[0] * 4] * 3, samples=[[0] * 4] * 3), dict(fade_ms=-1), dict(fade_ms=171),
                dict(max_ms=-1), dict(max_ms=60001), dict(max_ms=float("nan"))):
        with pytest.raises(ValueError, match="Breaks"):
            pipeline.Breaks(**dict(dict(B=3, N=4, device="cpu"), **bad))


def test_output_spec_refuses_breaks_in_the_one_place():
    b = pipeline.Breaks(3, 4, device="cpu")
    for kw, word in ((dict(capacity=True, pack=None), "pass max_frames and pack"), (dict(capacity=False, pack="s16"), "pass max_frames and pack"),
                     (dict(capacity=True, pack="s16", breaks=pipeline.Breaks(2, 4, device="cpu")), "Breaks of 3 rows"),
                     (dict(capacity=True, pack="s16", N=5), "Breaks of 3 rows of 5 tokens"),
                     (dict(capacity=True, pack="s16", breaks=[[0] * 4] * 3), "Breaks of 3 rows")):
        kw = dict(dict(breaks=b), **kw)
        with pytest.raises(ValueError, match=word):
            pipeline._output_spec(3, kw.pop("capacity"), **kw)
    spec, _ = pipeline._output_spec(3, True, pack="s16", trim=0, breaks=b, N=4)
    assert spec == pipeline._output_spec(3, True, pack="s16", trim=0)[0]
    for f in (pipeline.inference, pipeline.synthesize_long, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__):
        assert inspect.signature(f).parameters["breaks"].default is None, f
    assert inspect.signature(pipeline.GraphedSynthesis.__init__).parameters["max_break_ms"].default is None
    assert inspect.signature(pipeline.SynthesisResult.to_host).parameters["breaks"].default is False
    with pytest.raises(ValueError, match="max_frames"):
        pipeline.synthesize_long(None, None, [torch.zeros(3, dtype=torch.long)], breaks=pipeline.Breaks(1, 3, device="cpu"))


# ---- the hand-over layout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,level,limit,edges,fmt", [c for c in itertools.product(
    (1, 3), (False, True), (False, True), (False, True), (False, True), (False, True), ("f32", "ulaw")) if c[3] or not c[4]])
def test_layout_with_the_breaks_part_and_without(B, marks, gaps, level, limit, edges, fmt):
    n_marks = B * 6 if marks else 0
    old = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=level, with_limit=limit, with_edges=edges)
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=level, with_limit=limit, with_edges=edges, with_breaks=True)
    for name in ("offsets_at", "marks_at", "gaps_at", "level_at", "limit_at", "edges_at", "breaks_at"):
        assert getattr(lay, name) == getattr(old, name), name
    assert lay.breaks_at == lay.edges_at + (8 * B if edges else 0) and lay.samples_at == (lay.breaks_at + 8 * B + 15) // 16 * 16
    assert old.samples_at == (old.breaks_at + 15) // 16 * 16  # today's, byte for byte
    ho = lay.allocate(10, "cpu")
    assert len(lay.views(ho.buf)) == 5 and ho.breaks.dtype == torch.int32 and ho.breaks.numel() == 2 * B
    assert ho.breaks.data_ptr() - ho.buf.data_ptr() == lay.breaks_at and ho.packed.data_ptr() - ho.buf.data_ptr() == lay.samples_at
    assert (ho.edges is None) == (not edges)
    old.allocate(10, "cpu")
    assert old.breaks is None and old.breaks_view(old.buf) is None and old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize


# ---- the contract against a plain loop --------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got["ins"].tolist() == want["ins"].tolist() and got["cuts"].tolist() == want["cuts"].tolist(), what
    assert (got["count"], got["total"]) == (want["count"], want["total"]) and np.array_equal(got["bits"], want["bits"]), what


@pytest.mark.parametrize("B,N,F,rows", [(17, 7, 48, range(17)), (17, 7, 700, (0, 1, 6, 7, 8, 9)), (5, 1, 1, range(5)), (5, 512, 48, (0, 3)),
                                        (0, 7, 48, range(9)), (0, 7, 0, (3, 5, 8))])
def test_contract_agrees_with_a_per_sample_loop(B, N, F, rows):
    c, ref = R.case(B, N), R.reference(B, N, F)
    ramp = resample.edge_ramp_design(F) if F else None
    for b in rows:
        n = R.row_samples(c["frames"][b], c["T_cap"], c["spf"], c["trim"])
        _same(ref[b], R.brute_row(c["wave"][b, :n], c["pos"][b], c["brk"][b], c["max_break"], ramp), (c["names"][b], b))


def test_the_constructed_rows_are_what_they_are_named():
    c, ref = R.batch(17, 7), R.reference(17, 7, 48)
    row = {name: (b, ref[b]) for b, name in reversed(list(enumerate(c["names"])))}  # the first row of every kind
    n = lambda b: R.row_samples(c["frames"][b], c["T_cap"], c["spf"], c["trim"])
    assert row["empty spans"][1]["cuts"].tolist() == [-1, 500, 500, -1, 1200, -1, -1]
    assert row["short spans"][1]["cuts"].tolist() == [-1, 127, -1, 363, -1, 1050, -1], "no aligned window: the middle"
    assert row["128 samples"][1]["cuts"].tolist() == [64, 192, -1, 1064, -1, 2064, -1], "aligned: the one candidate; unaligned: the middle"
    b, r = row["whole row"]
    assert r["cuts"][3] % 64 == 0 and 64 <= r["cuts"][3] <= n(b) - 64 and r["count"] == n(b) + 300
    for name in ("none asked", "no break"):
        b, r = row[name]
        assert r["total"] == 0 and (r["cuts"] == -1).all() and np.array_equal(r["bits"], c["wave"][b, :n(b)].view(np.uint32)), "a bit copy"
    r = row["adjacent"][1]
    assert 900 <= r["cuts"][2] <= 1000 <= r["cuts"][3] <= 1800 and r["ins"].tolist() == [0, 0, 100, 120, 0, 0, 0]
    r = row["close cuts"][1]
    assert r["cuts"][[1, 3]].tolist() == [1015, 1075] and r["cuts"][3] - r["cuts"][1] < 2 * 48
    r = row["cap"][1]
    assert r["ins"].tolist() == [0, 100, 0, 0, 350, 0, 0] and r["cuts"][6] == -1 and r["total"] == R.MAX_BREAK
    assert row["zero span"][1]["cuts"][3] == 1088, "equal windows: the smallest k with 64 (k - 1) >= 1000"
    b, r = row["non-finite"]
    assert R.NAN_PAYLOAD in r["bits"].tolist() and r["cuts"][3] not in range(1024, 1217), "the window over 3e30 is +inf, not the minimum"
    assert row["frames 0"][1]["bits"].tolist() == [0] * 30 and row["frames 0"][1]["cuts"].tolist() == [-1, 0, -1, -1, -1, -1, 0]
    b, r = row["bad pos"]
    assert 64 <= r["cuts"][0] <= 900 - 64 and r["cuts"][2] == 900 and r["cuts"][5] == n(b)
    assert ref[15]["total"] == R.MAX_BREAK and ref[15]["ins"].tolist() == [90, 0, 0, 0, 110, 0, 250], "the cap met exactly"
    assert ref[16]["ins"].tolist() == [0, 0, 0, 0, R.MAX_BREAK, 0, 0]
    # silence is +0.0f and follows its cut; the samples around it are the faded ends of the two segments
    r, x = row["plain"][1], c["wave"][0]
    cut, ramp = int(r["cuts"][2]), resample.edge_ramp_design(48)
    assert (r["bits"][cut:cut + 240] == 0).all() and np.array_equal(r["bits"][:cut - 48], x[:cut - 48].view(np.uint32))
    assert np.array_equal(r["bits"][cut - 48:cut], (x[cut - 48:cut] * ramp[::-1]).view(np.uint32))
    assert np.array_equal(r["bits"][cut + 240:cut + 288], (x[cut:cut + 48] * ramp).view(np.uint32))
    # N = 512: seeded rows meet the cap and take pos out of order
    big = R.reference(17, 512, 48)
    assert max(r["total"] for r in big) == R.MAX_BREAK and sum(r["total"] > 0 for r in big) >= 12
    assert all((np.diff(r["cuts"][r["cuts"] >= 0]) >= 0).all() for r in big), "the cuts of a row do not decrease"


def test_marks_reference():
    pos, ins = np.array([[0, 10, 10, 50]]), np.array([[5, 0, 7]])
    assert R.marks(pos, ins).tolist() == [[0, 15, 15, 62]] and R.marks(pos, ins, 1, 3).tolist() == [[0, 5, 5, 21]]
    assert R.marks(pos, ins, 147, 80).tolist() == [[0, 28, 28, 114]]


# ---- routing ------------------------------------------------------------------------------------------------------------------------
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
        seen.append(("wave_edges", wave, frames, kw))
        kw["edges"].copy_(torch.arange(kw["edges"].numel(), dtype=torch.int32))
        return torch.full_like(wave[:, 0], 3.0), kw["edges"]

    def breaks(wave, frames, pos, brk, max_break, ramp=None, **kw):
        seen.append(("wave_breaks", wave, frames, dict(kw, pos=pos, brk=brk, max_break=max_break, ramp=ramp)))
        kw["breaks"].copy_(10 + torch.arange(kw["breaks"].numel(), dtype=torch.int32))
        return torch.full((wave.shape[0], wave.shape[-1] + max_break), 4.0), "ins", None, kw["breaks"]

    def marks(name):
        def f(dur, frames, T_cap, **kw):
            seen.append((name, dur, frames, dict(kw, T_cap=T_cap)))
            return name + " pos"
        return f
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_edges", edges)
    monkeypatch.setattr(ops, "wave_breaks", breaks)
    monkeypatch.setattr(ops, "token_marks", marks("token_marks"))
    monkeypatch.setattr(ops, "token_marks_edges", marks("token_marks_edges"))
    monkeypatch.setattr(ops, "token_marks_breaks", lambda pos, ins, **kw: seen.append(("token_marks_breaks", pos, ins, kw)))
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    monkeypatch.setattr(pipeline.resample, "limit_window", lambda W, dev: torch.from_numpy(resample.limit_window_design(W)))
    monkeypatch.setattr(pipeline.resample, "edge_ramp", lambda F, dev: torch.from_numpy(resample.edge_ramp_design(F)))
    return seen


@pytest.mark.parametrize("edges,gaps,fmt,rate,level", list(itertools.product((False, True), (False, True), ("s16", "ulaw"), (None, 8000),
                                                                             (None, "plain", "limiter"))))
def test_hand_over_splices_behind_the_trim_and_runs_the_rest_over_one_sample_frames(spied, edges, gaps, fmt, rate, level):
    B, N, L, spf, max_gap = 3, 4, 1200, 600, 7
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = None if level is None else pipeline.Level(B, device="cpu", limiter=level == "limiter")
    e = pipeline.Edges(B, device="cpu") if edges else None
    br = pipeline.Breaks(B, N, ms=[[0, 10, 0, 0]] * B, max_ms=100, device="cpu")
    tokens = dict(dur="dur", frames=frames, T_cap=2, lengths="lens", shift=True, trim=50, samples_per_frame=spf)
    args = (wave, frames, 50, fmt, spf, rate)
    kw = dict(n_marks=B * (N + 1), gaps=g, max_gap=max_gap if gaps else 0, level=lv, edges=e)
    old = pipeline._hand_over_edges(*args, **kw)
    before = [s[0] for s in spied]
    assert "wave_breaks" not in before and not any(n.startswith("token_marks") for n in before) and old.breaks is None
    del spied[:]
    ho = pipeline._hand_over_edges(*args, breaks=br, tokens=tokens, **kw)
    pos_by = "token_marks_edges" if edges else "token_marks"
    stage = [pos_by, "wave_breaks"]
    assert [s[0] for s in spied] == before[:edges] + stage + before[edges:], "behind the trim, in front of the rest, which is the call without it"
    _, d, f, k = spied[edges]  # the boundaries: the decoder's geometry, no rate
    assert d == "dur" and f is frames and k["T_cap"] == 2 and k["lengths"] == "lens" and k["shift"] is True and k["trim"] == 50
    assert k["samples_per_frame"] == spf and "rate" not in k and "out" not in k and (k["edges"].data_ptr() == ho.edges.data_ptr() if edges else "edges" not in k)
    _, w, f, k = spied[edges + 1]
    if edges:
        assert bool((w == 3.0).all()) and f.tolist() == [1, 3, 5] and k["trim"] == 0 and k["samples_per_frame"] == 1
    else:
        assert w is wave and f is frames and k["trim"] == 50 and k["samples_per_frame"] == spf
    assert k["pos"] == pos_by + " pos" and k["brk"] is br.samples and k["max_break"] == 2400 and k["ramp"].numel() == 48
    assert k["breaks"].data_ptr() == ho.breaks.data_ptr() and ho.pos == pos_by + " pos" and ho.ins == "ins"
    for name, w, f, k in spied[edges + 2:]:
        limited = level == "limiter" and name not in ("wave_level", "wave_limit")  # the packers read the limiter's rows
        assert bool((w == (5.0 if limited else 4.0)).all()) and w.shape[-1] == L + 2400, name
        assert f.tolist() == [10, 12, 14] and f.is_contiguous() and k["trim"] == 0 and k["samples_per_frame"] == 1, name
    U, Dn = resample.ratio(rate or resample.MODEL_RATE)
    assert ho.packed.numel() == old.packed.numel() + B * resample.output_samples(2400, U, Dn), "room grows by the cap at the output rate"
    res = pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output(fmt, 50), ho)
    assert tuple(res.breaks.shape) == (B, 2) and res.breaks.data_ptr() == ho.breaks.data_ptr()
    with pytest.raises(ValueError, match="breaks"):
        pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output(fmt, 50), old).to_host(breaks=True)
    # a Breaks without a fade passes no ramp
    del spied[:]
    pipeline._hand_over_edges(*args, breaks=pipeline.Breaks(B, N, fade_ms=0, device="cpu"), tokens=tokens, **kw)
    assert spied[edges + 1][3]["ramp"] is None

