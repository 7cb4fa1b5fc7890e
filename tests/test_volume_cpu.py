"""C ABI and host-side contract of the volume stage of the hand-over: `st2_wave_volume` and its helper are
declared, exported and bound under ABI 23 and refuse bad arguments before any launch; `Volume` validates its settings, keeps one
table per kind and slices over the same memory; the hand-over layout gains its tenth part without moving the other nine;
`_output_spec` refuses the option in the one place; `_hand_over_edges` runs the stage behind the compressor and in front of the
level, over the boundaries of the rows as they are by then, and calls nothing new without it; the numpy contract of
tests/_volume_ref.py agrees with a plain loop and has the properties the design states; `emphasis_tables`.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _volume_ref as R
from styletts2_amd import _build, _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_wave_volume", "st2_wave_volume_workspace_bytes")
INF, NAN = float("inf"), float("nan")


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
    assert ops.VOLUME_BLOCK == 64 and ops.VOLUME_TILE == 4096 and ops.VOLUME_DB == (-60.0, 20.0)
    assert "st2_volume.hip" in _build.SOURCES and _build.EXTRA_FLAGS["st2_volume.hip"] == ["-fno-slp-vectorize"]


D = C.c_void_p(4096)


def _call(lib, a):
    return lib.st2_wave_volume(a["wave"], a["w_bs"], a["frames"], a["B"], a["T_cap"], a["spf"], a["trim"], a["pos"], a["lengths"], a["N"],
                               a["db"], a["tok_db"], a["A"], a["win"], a["out"], a["o_bs"], a["vol"], a["work"], a["work_bytes"], None)


def test_wave_volume_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_volume_workspace_bytes(2, 10, 600)
    assert need == (4 * 2 * (94 + 1 + 2) + 15) // 16 * 16  # lin: ceil(6000 / 64) = 94 blocks a row; one chunk of them; two tiles
    assert ops.wave_volume_workspace_bytes(2, 10, 600) == need
    for bad in ((0, 10, 600), (2, 0, 600), (2, 10, 0), (-1, 10, 600)):
        assert lib.st2_wave_volume_workspace_bytes(*bad) == 0
    far = C.c_void_p(4096 + (1 << 20))
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, pos=D, lengths=D, N=8, db=D, tok_db=D, A=3, win=D, out=far,
                o_bs=6000, vol=D, work=D, work_bytes=need)
    cases = [(dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=-2), "bad geometry"),
             (dict(B=70000), "bad geometry"), (dict(T_cap=0), "bad geometry"), (dict(T_cap=-5), "bad geometry"), (dict(spf=0), "bad geometry"),
             (dict(spf=-1), "bad geometry"), (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"), (dict(o_bs=5999), "o_bs"),
             (dict(T_cap=1 << 22, spf=600), "too long"), (dict(N=0), "N=0"), (dict(N=-1), "N=-1"), (dict(N=513), "N=513"),
             (dict(A=-1), "A=-1"), (dict(A=65), "A=65"), (dict(win=None), "win is NULL"), (dict(A=0), "win must be NULL"),
             (dict(work_bytes=need - 1), "too small"), (dict(work_bytes=-1), "too small"), (dict(out=D), "aliases"),
             (dict(out=C.c_void_p(4096 + 4 * 11000)), "aliases"), (dict(out=C.c_void_p(4096 - 4 * 11000 + (1 << 20)), wave=far), "aliases")]
    cases += [({k: None}, "NULL") for k in ("pos", "out", "vol", "work")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to float") for k in ("wave", "db", "tok_db", "win", "vol", "work")]
    cases += [(dict(out=C.c_void_p(4098 + (1 << 20))), "not aligned to float")]
    cases += [({k: C.c_void_p(4098)}, "not aligned to int32") for k in ("frames", "pos", "lengths")]
    for change, word in cases:
        assert _call(lib, dict(base, **change)) != 0, change
        assert _err(lib).startswith("st2_wave_volume:") and word in _err(lib), (change, _err(lib))
    # the tables and the lengths may be missing; the refusals behind them stay
    assert _call(lib, dict(base, db=None, tok_db=None, lengths=None, A=0, win=None, work_bytes=0)) != 0 and "too small" in _err(lib)


def test_wrapper_has_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_volume(w, f, torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2), torch.zeros(2, 4), None, A=0)
    with pytest.raises(_lib.St2Error):
        ops.wave_volume(w, None, torch.zeros(2, 5, dtype=torch.int32), None, None, None, A=0)
    sig = inspect.signature(ops.wave_volume).parameters
    assert list(sig) == ["wave", "frames", "pos", "db", "tok_db", "win", "A", "lengths", "trim", "samples_per_frame", "out", "volume", "workspace"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[6:])
    assert (sig["lengths"].default, sig["trim"].default, sig["samples_per_frame"].default) == (None, 0, 600)


# ---- Volume --------------------------------------------------------------------------------------------------------------------
def test_volume_validates_and_keeps_one_table_per_kind():
    v = pipeline.Volume(3, device="cpu")
    assert v.db is None and v.tok_db is None and v.N is None and (v.A, v.ramp_ms) == (3, 8.0) and v.options() == dict(ramp_ms=8.0)
    v = pipeline.Volume(3, N=4, db=[0, -6.5, -INF], tok_db=[[0, 3, 0, 0], [0, 0, -60, 20], [1, 1, 1, 1]], ramp_ms=0, device="cpu")
    assert v.db.dtype == torch.float32 and v.db.tolist() == [0.0, -6.5, -INF] and tuple(v.tok_db.shape) == (3, 4) and v.tok_db.is_contiguous()
    assert v.tok_db[1].tolist() == [0.0, 0.0, -60.0, 20.0] and v.A == 0 and v.device == torch.device("cpu")
    assert pipeline.Volume(2, tok_db=np.zeros((2, 7), dtype=np.float32), device="cpu").N == 7, "N from the table"
    only_n = pipeline.Volume(2, N=5, device="cpu")
    assert only_n.db is None and only_n.tok_db.tolist() == [[0.0] * 5] * 2, "with N the per-token table is there, 0 dB"
    assert pipeline.Volume(2, db=-3, tok_db=1.5, N=3, device="cpu").tok_db.tolist() == [[1.5] * 3] * 2
    assert pipeline.Volume(1, ramp_ms=170, device="cpu").A == 64 and pipeline.Volume(1, ramp_ms=1.0, device="cpu").A == 0
    part = v.slice(1, 3)
    assert part.B == 2 and part.N == 4 and part.db.data_ptr() == v.db[1:].data_ptr() and part.tok_db.data_ptr() == v.tok_db[1].data_ptr()
    assert part.options() == v.options() and part.A == v.A and part.device == v.device
    assert pipeline.Volume(2, db=-3.0, device="cpu").slice(0, 1).tok_db is None
    nt = pipeline.Volume.neutral(3, 4, device="cpu")
    assert nt.db.tolist() == [0.0] * 3 and nt.tok_db.tolist() == [[0.0] * 4] * 3 and nt.A == 3
    assert pipeline.Volume.neutral(3, device="cpu").tok_db is None
    for bad in (dict(db=-60.5), dict(db=20.5), dict(db=INF), dict(db=NAN), dict(db=[0, 0]), dict(db=[0, 0, 0, 0]), dict(db="loud"),
                dict(tok_db=[0, 1, 2]), dict(tok_db=[[0, 1], [0, 1]]), dict(tok_db=[[0, 1]] * 3, N=3), dict(tok_db=[[0, NAN]] * 3),
                dict(tok_db=[[0, 21]] * 3), dict(N=0), dict(N=513), dict(ramp_ms=-1), dict(ramp_ms=171), dict(ramp_ms=NAN)):
        with pytest.raises(ValueError, match="Volume"):
            pipeline.Volume(3, device="cpu", **bad)
    with pytest.raises(ValueError, match="Volume"):
        pipeline.Volume(0, device="cpu")
    sig = list(inspect.signature(pipeline.Volume.__init__).parameters)[1:]
    assert sig == ["B", "N", "db", "tok_db", "ramp_ms", "device"]


# ---- the hand-over layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,fmt,more", list(itertools.product((1, 3), (False, True), (False, True), ("f32", "ulaw"),
                                                                         ({}, dict(with_level=True, with_limit=True, with_edges=True, with_breaks=True,
                                                                                   with_dynamics=True)))))
def test_layout_with_the_volume_part_and_without(B, marks, gaps, fmt, more):
    n_marks = B * 6 if marks else 0
    old = pipeline._HandOver(B, fmt, n_marks, gaps, **more)
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_volume=True, **more)
    names = ("offsets_at", "marks_at", "gaps_at", "level_at", "limit_at", "edges_at", "breaks_at", "dynamics_at", "volume_at")
    assert [getattr(lay, n) for n in names] == [getattr(old, n) for n in names]
    assert old.volume_at == old.dynamics_at + (8 * B if more else 0) and old.samples_at == (old.volume_at + 15) // 16 * 16  # today's
    assert lay.samples_at == (lay.volume_at + 8 * B + 15) // 16 * 16
    ho = lay.allocate(10, "cpu")
    assert len(lay.views(ho.buf)) == 5 and ho.volume.dtype == torch.float32 and ho.volume.numel() == 2 * B
    assert ho.volume.data_ptr() - ho.buf.data_ptr() == lay.volume_at and ho.packed.data_ptr() - ho.buf.data_ptr() == lay.samples_at
    old.allocate(10, "cpu")
    assert old.volume is None and old.volume_view(old.buf) is None and old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize
    res = pipeline.SynthesisResult(torch.zeros(B, 1, 600), torch.ones(B, dtype=torch.int32), 1, pipeline._Output(fmt, 0), ho)
    assert tuple(res.volume.shape) == (B, 2) and res.volume.data_ptr() == ho.volume.data_ptr()
    plain = pipeline.SynthesisResult(torch.zeros(B, 1, 600), torch.ones(B, dtype=torch.int32), 1, pipeline._Output(fmt, 0), old)
    assert plain.volume is None
    with pytest.raises(ValueError, match="volume"):
        plain.to_host(volume=True)
    assert inspect.signature(pipeline.SynthesisResult.to_host).parameters["volume"].default is False


def test_output_spec_refuses_volume_in_the_one_place():
    v = pipeline.Volume(3, N=5, device="cpu")
    for kw, word in ((dict(capacity=True, pack=None), "pass max_frames and pack"), (dict(capacity=False, pack="s16"), "pass max_frames and pack"),
                     (dict(capacity=True, pack="s16", volume=pipeline.Volume(2, device="cpu")), "Volume of 3 rows"),
                     (dict(capacity=True, pack="s16", volume=True), "Volume of 3 rows"),
                     (dict(capacity=True, pack="s16", N=6), "Volume of 3 rows of 6 tokens"),
                     (dict(capacity=True, pack="s16", N=5, device="meta"), "holds its tables on cpu")):
        with pytest.raises(ValueError, match=word):
            pipeline._output_spec(3, **dict(dict(volume=v), **kw))
    spec, _ = pipeline._output_spec(3, True, "s16", volume=v, N=5, device="cpu")
    assert spec == pipeline._output_spec(3, True, "s16")[0], "the spec does not carry it"
    pipeline._output_spec(3, True, "s16", volume=pipeline.Volume(3, db=-3.0, device="cpu"), N=9)  # no per-token table: any width
    for f in (pipeline.inference, pipeline.synthesize_long, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__):
        assert inspect.signature(f).parameters["volume"].default is None, f
    with pytest.raises(ValueError, match="max_frames"):
        pipeline.synthesize_long(None, None, [torch.zeros(3, dtype=torch.int64)], volume=v)


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

    def edges(wave, frames, top_db, keep, ramp=None, **kw):
        seen.append(("wave_edges", wave, frames, kw))
        kw["edges"].copy_(torch.tensor([[3, 20 + b] for b in range(wave.shape[0])], dtype=torch.int32).reshape(-1))
        return torch.full((wave.shape[0], wave.shape[-1]), 3.0), kw["edges"]

    def breaks(wave, frames, pos, brk, max_break, ramp=None, **kw):
        seen.append(("wave_breaks", wave, frames, dict(kw, pos=pos)))
        kw["breaks"].copy_(10 + torch.arange(kw["breaks"].numel(), dtype=torch.int32))
        return torch.full((wave.shape[0], wave.shape[-1] + max_break), 4.0), "ins", None, kw["breaks"]

    def dynamics(wave, frames, params, win, **kw):
        seen.append(("wave_dynamics", wave, frames, kw))
        return torch.full((wave.shape[0], wave.shape[-1]), 6.0), kw["dynamics"]

    def volume(wave, frames, pos, db, tok_db, win, **kw):
        seen.append(("wave_volume", wave, frames, dict(kw, pos=pos, db=db, tok_db=tok_db, win=win)))
        return torch.full((wave.shape[0], wave.shape[-1]), 7.0), kw["volume"]
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(ops, "wave_edges", edges)
    monkeypatch.setattr(ops, "wave_breaks", breaks)
    monkeypatch.setattr(ops, "wave_dynamics", dynamics)
    monkeypatch.setattr(ops, "wave_volume", volume)
    monkeypatch.setattr(ops, "token_marks", lambda dur, frames, T_cap, **kw: seen.append(("token_marks", dur, frames, kw)) or "pos")
    monkeypatch.setattr(ops, "token_marks_edges", lambda dur, frames, T_cap, **kw: seen.append(("token_marks_edges", dur, frames, kw)) or "pos_e")
    monkeypatch.setattr(ops, "token_marks_breaks", lambda pos, ins, **kw: seen.append(("token_marks_breaks", pos, ins, kw)) or "pos_b")
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    monkeypatch.setattr(pipeline.resample, "limit_window", lambda W, dev: torch.from_numpy(resample.limit_window_design(W)))
    monkeypatch.setattr(pipeline.resample, "edge_ramp", lambda F, dev: torch.from_numpy(resample.edge_ramp_design(F)))
    return seen


@pytest.mark.parametrize("with_edges,with_breaks,with_dyn,gaps,fmt_rate,level", list(itertools.product(
    (False, True), (False, True), (False, True), (False, True), (("s16", None), ("ulaw", 8000)), (None, "plain", "limiter"))))
def test_hand_over_sets_the_volume_behind_the_compressor_and_in_front_of_the_level(spied, with_edges, with_breaks, with_dyn, gaps, fmt_rate, level):
    B, N, L, spf, max_gap = 3, 4, 1200, 600, 7
    fmt, rate = fmt_rate
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = None if level is None else pipeline.Level(B, device="cpu", limiter=level == "limiter")
    tokens = dict(dur="dur", frames=frames, T_cap=2, lengths="lens", shift=True, trim=50, samples_per_frame=spf)
    more = {}
    if with_edges:
        more.update(edges=pipeline.Edges(B, device="cpu"))
    if with_breaks:
        more.update(breaks=pipeline.Breaks(B, N, ms=[[0, 10, 0, 0]] * B, max_ms=100, device="cpu"))
    if with_dyn:
        more.update(dynamics=pipeline.Dynamics(B, device="cpu"))
    vo = pipeline.Volume(B, N, db=[0, -6, 3], tok_db=[[0, 6, 0, 0]] * B, ramp_ms=16.0, device="cpu")
    args = (wave, frames, 50, fmt, spf, rate)
    kw = dict(n_marks=B * (N + 1), gaps=g, max_gap=max_gap if gaps else 0, level=lv, **more)
    old = pipeline._hand_over_edges(*args, **dict(kw, **({"tokens": tokens} if with_breaks else {})))
    before = [s[0] for s in spied]
    assert "wave_volume" not in before and old.volume is None, "nothing new is called without the option"
    assert ("token_marks_breaks" not in before) and (("token_marks" in before or "token_marks_edges" in before) == with_breaks)
    del spied[:]
    ho = pipeline._hand_over_edges(*args, volume=vo, tokens=tokens, **kw)
    at = with_edges + 2 * with_breaks + with_dyn  # the stages in front: the trim; the boundaries and the breaks; the compressor
    source = "token_marks_breaks" if with_breaks else "token_marks_edges" if with_edges else "token_marks"
    names = [s[0] for s in spied]
    assert names == before[:at] + [source, "wave_volume"] + before[at:], "behind the compressor, in front of the level and the rest"
    assert at == 0 or names[at - 1] == ("wave_dynamics" if with_dyn else "wave_breaks" if with_breaks else "wave_edges")
    assert names.count("token_marks") + names.count("token_marks_edges") + names.count("token_marks_breaks") == 1 + with_breaks, "one launch more"
    marks = spied[at]
    if with_breaks:
        assert marks[1] == "pos_e" if with_edges else marks[1] == "pos"
        assert marks[2] == "ins" and "rate" not in marks[3], "the boundaries the breaks read, moved by what they inserted"
        assert ho.pos == ("pos_e" if with_edges else "pos")
    else:
        assert marks[1] == "dur" and marks[2] is frames and "rate" not in marks[3], "without a rate"
        assert marks[3]["lengths"] == "lens" and marks[3]["shift"] is True and marks[3]["trim"] == 50 and marks[3]["samples_per_frame"] == spf
        if with_edges:
            assert marks[3]["edges"].data_ptr() == ho.edges.data_ptr()
    _, w, f, k = spied[at + 1]
    assert k["pos"] == {"token_marks": "pos", "token_marks_edges": "pos_e", "token_marks_breaks": "pos_b"}[source]
    stage = 6.0 if with_dyn else 4.0 if with_breaks else 3.0 if with_edges else None
    assert w is wave if stage is None else bool((w == stage).all()), "the rows of the stage in front"
    if with_edges or with_breaks:  # rows of one-sample frames, nothing trimmed
        assert k["trim"] == 0 and k["samples_per_frame"] == 1 and f.tolist() == ([10, 12, 14] if with_breaks else [20, 21, 22])
    else:
        assert f is frames and k["trim"] == 50 and k["samples_per_frame"] == spf
    assert k["db"] is vo.db and k["tok_db"] is vo.tok_db and k["A"] == 6 and k["win"].numel() == 13 and k["lengths"] == "lens"
    assert k["volume"].data_ptr() == ho.volume.data_ptr() and ho.volume.numel() == 2 * B
    for name, w2, f2, k2 in spied[at + 2:]:
        limited = level == "limiter" and name not in ("wave_level", "wave_limit")  # the packers read the limiter's rows
        assert bool((w2 == (5.0 if limited else 7.0)).all()), (name, "everything behind reads the rows with their gains")
        assert k2["trim"] == k["trim"] and k2["samples_per_frame"] == k["samples_per_frame"] and (f2 is f or f2.tolist() == f.tolist())
    assert ho.packed.numel() == old.packed.numel() and ho.samples_at >= old.samples_at, "sample counts do not change"
    # no ramp: no window; no per-token table: none handed on
    del spied[:]
    pipeline._hand_over_edges(*args, volume=pipeline.Volume(B, db=-3.0, ramp_ms=0, device="cpu"), tokens=tokens, **kw)
    k = spied[at + 1][3]
    assert k["win"] is None and k["A"] == 0 and k["tok_db"] is None and k["db"].tolist() == [-3.0] * B


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def _noise(n, seed, amp=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def _win(A):
    return None if A == 0 else resample.limit_window_design(A)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    """Bit-equal, with any NaN equal to any NaN where neither side kept a word (a NaN made by inf * 0 has no payload to keep)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("n,A,Nb,db", [(1, 0, 3, -3.0), (63, 1, 5, None), (64, 2, 5, 2.0), (65, 0, 0, -7.0), (200, 3, 5, NAN), (700, 5, 4, 6.0),
                                       (333, 0, 5, -INF), (450, 64, 5, 19.0), (4097, 3, 1, -1.0)])
def test_contract_agrees_with_a_plain_loop(n, A, Nb, db):
    x = _noise(n, n + A)
    if n > 100:
        x[n // 2], x[5], x[40] = np.nan, np.inf, 1e-42
    pos = np.array([0, 0, n // 3, n // 3, (2 * n) // 3, n], dtype=np.int32)
    tok = np.array([20.0, -4.0, NAN, 6.0, -60.0], dtype=np.float32)
    out, vol, st = R.reference_row(x, pos, Nb, db, tok, A, _win(A))
    b_out, b_vol, b_lin = R.brute_row(x, pos, Nb, db, tok, A, _win(A))
    assert np.array_equal(bits(st["lin"]), bits(b_lin)) and _same(out, b_out) and np.array_equal(bits(vol), bits(b_vol))
    assert st["lin"].dtype == np.float32 and len(st["lin"]) == (n + 63) // 64 and vol[1] <= len(st["lin"])
    assert np.array_equal(np.isnan(out[np.isfinite(x)]), np.zeros(np.isfinite(x).sum(), dtype=bool))
    no_tab, _, st0 = R.reference_row(x, pos, Nb, None, None, A, _win(A))
    assert (st0["lin"] == 1).all() and np.array_equal(bits(no_tab), bits(x)), "no table: a bit copy"


def test_cleaning_maps_nan_to_zero_and_clamps():
    got = R.clean([NAN, -INF, INF, -60.0, 20.0, -60.5, 20.5, 0.0, -3.25])
    assert got.dtype == np.float32 and got.tolist() == [0.0, -60.0, 20.0, -60.0, 20.0, -60.0, 20.0, 0.0, -3.25]
    pos = np.array([0, 100], dtype=np.int32)
    assert R.wanted(100, pos, 1, 15.0, np.array([15.0], dtype=np.float32)).tolist() == [20.0, 20.0], "the sum is clamped again"
    assert R.wanted(100, pos, 1, -40.0, np.array([-40.0], dtype=np.float32)).tolist() == [-60.0, -60.0]
    assert R.wanted(100, pos, 0, -40.0, np.array([-40.0], dtype=np.float32)).tolist() == [-40.0, -40.0], "no token: the term is 0"


@pytest.mark.parametrize("A", [0, 1, 3, 64])
def test_zero_db_keeps_the_bits_and_a_constant_gain_is_one_product(A):
    n = 64 * 300 + 17
    x = _noise(n, 11)
    x[7], x[9000] = np.nan, np.inf
    x[8:12].view(np.uint32)[:] = [0x7fc12345, 0x7f812345, 0xffc00001, 0x00000007]  # NaN payloads, quiet and signalling; a denormal
    pos = np.array([0, 64 * 100, 64 * 200, n], dtype=np.int32)
    out, vol, st = R.reference_row(x, pos, 3, 0.0, np.zeros(3, dtype=np.float32), A, _win(A))
    assert (st["e"] == 0).all() and (st["lin"] == 1).all() and np.array_equal(bits(out), bits(x)) and vol[1] == 0
    assert vol[0] == np.inf
    # one row gain: x * fl32(10^(d / 20)) everywhere
    for d in (-6.0, 3.5, 20.0):
        out, vol, st = R.reference_row(x, pos, 3, d, None, A, _win(A))
        g = np.float32(np.power(10.0, np.float64(d) / 20.0))
        assert (st["e"] == d).all() and (st["lin"] == g).all() and vol[1] == len(st["lin"])
        with np.errstate(invalid="ignore", over="ignore"):
            assert _same(out, x * g)
    # one token at +6 dB: its gain away from the edges of the change, the others' bits kept away from them
    tok = np.array([0.0, 6.0, 0.0], dtype=np.float32)
    out, vol, st = R.reference_row(x, pos, 3, None, tok, A, _win(A))
    g = np.float32(np.power(10.0, 6.0 / 20.0))
    inside = slice(64 * (100 + A + 1), 64 * (200 - A - 1))
    if A < 49:
        assert (st["lin"][100 + A:200 - A] == g).all()
        with np.errstate(invalid="ignore"):
            assert _same(out[inside], x[inside] * g)
    keep = np.r_[0:64 * (100 - A - 1), 64 * (200 + A + 1):n]
    assert np.array_equal(bits(out[keep]), bits(x[keep])) and (st["lin"][:100 - A] == 1).all() and (st["lin"][200 + A:] == 1).all()
    assert vol[1] == np.count_nonzero(st["lin"] != 1) and 100 <= vol[1] <= 100 + 2 * A
    mid = st["lin"][100 - A:100 + A]
    assert ((mid >= 1) & (mid <= g)).all()
    if A < 49:  # the window sees one edge of the token at a time
        assert (np.diff(st["e"][100 - A - 1:100 + A + 1]) >= 0).all(), "a monotone ramp between the two"


def test_at_or_under_minus_sixty_the_samples_are_exact_zeros():
    n = 64 * 120
    x = _noise(n, 12) + np.float32(0.5)
    pos = np.array([0, 64 * 40, 64 * 80, n], dtype=np.int32)
    for tok in ([0.0, -60.0, 0.0], [0.0, -INF, 0.0], [0.0, -75.0, 0.0]):
        out, vol, st = R.reference_row(x, pos, 3, None, np.array(tok, dtype=np.float32), 3, _win(3))
        assert (st["lin"][43:77] == 0).all() and (out[64 * 44:64 * 76] == 0).all() and not np.signbit(out[64 * 44:64 * 76]).any()
        assert (st["lin"][:37] == 1).all() and (st["lin"][37:43] > 0).all(), "only the ramp lies between"
    out, vol, st = R.reference_row(x, pos, 3, -60.0, None, 3, _win(3))
    assert (st["lin"] == 0).all() and (out == 0).all() and vol.tolist() == [0.0, 120.0]
    out, vol, st = R.reference_row(x, pos, 3, -59.0, None, 3, _win(3))
    assert (st["lin"] > 0).all() and (out != 0).all()


def test_two_tokens_at_one_boundary_and_tokens_of_no_samples():
    n = 64 * 10
    # tokens 0 and 1 collapsed to 0 as after an edge trim; tokens 3 and 4 begin at one sample (token 3 has none); pad tokens at n
    pos = np.array([0, 0, 0, 200, 200, 400, n, n, n], dtype=np.int32)
    idx = R.token_of_block(pos, 6, n)
    assert idx.tolist() == [2, 2, 2, 4, 4, 4, 5, 5, 5, 5], "the last of several tokens at one boundary owns what follows"
    assert R.token_of_block(pos, 8, n).tolist() == idx.tolist(), "pad tokens at the row's end own nothing: no centre reaches n"
    assert R.token_of_block(pos, 2, n).tolist() == [1] * 10 and R.token_of_block(pos, 0, n).tolist() == [0] * 10
    assert R.token_of_block(np.array([50, 100, n], dtype=np.int32), 2, n).tolist() == [0, 0] + [1] * 8, "nothing at or under c: token 0"
    assert R.token_of_block(np.array([0, 70], dtype=np.int32), 2, 71).tolist() == [0, 1], "the last block's centre is clamped to n - 1"
    # the centre rule at a boundary of 64 k + 31 / 32 / 33
    for at, want in ((64 * 3 + 31, 1), (64 * 3 + 32, 1), (64 * 3 + 33, 0)):
        assert R.token_of_block(np.array([0, at, n], dtype=np.int32), 2, n)[3] == want
    tok = np.array([-20.0, -20.0, 0.0, 9.0, 6.0, -6.0, 0.0, 0.0], dtype=np.float32)
    st = R.row_stages(n, pos, 6, None, tok, 0, None)
    assert st["d"].tolist() == [0.0] * 3 + [6.0] * 3 + [-6.0] * 4, "a token of no samples colours nothing"
    # a short row: one sample, one block, whichever window
    for A in (0, 3, 64):
        out, vol, st = R.reference_row(np.array([0.5], dtype=np.float32), np.array([0, 1], dtype=np.int32), 1, -6.0, None, A, _win(A))
        assert len(st["lin"]) == 1 and out[0] == np.float32(0.5) * st["lin"][0] and vol[1] == 1


def test_smoothing_is_exact_on_flat_stretches_and_a_weighted_mean_between():
    d = np.r_[np.zeros(200), np.full(200, -12.0), np.zeros(100)]
    for A in (1, 3, 64):
        e = R.smooth(d, A, _win(A))
        assert (e[:200 - A] == 0).all() and (e[200 + A:400 - A] == -12.0).all() and (e[400 + A:] == 0).all()
        assert ((e >= -12.0) & (e <= 0)).all() and (np.diff(e[190 - A:210 + A]) <= 0).all()
        w = resample.limit_window_design(A).astype(np.float64)
        k = 200
        mean = sum(w[j + A] * d[k + j] for j in range(-A, A + 1))
        assert abs(e[k] - mean) <= 1e-5, "the window's weighted mean (its fp32 weights sum to 1 within rounding)"
    assert np.array_equal(R.smooth(d, 0, None), d)


# ---- <emphasis> --------------------------------------------------------------------------------------------------------------------
def test_emphasis_tables_presets_overlaps_and_neutrality():
    t = pipeline.emphasis_tables(2, 6, [])
    assert sorted(t) == ["tok_db", "tok_f0_scale", "tok_range", "tok_speed"]
    for name, neutral in (("tok_speed", 1.0), ("tok_f0_scale", 1.0), ("tok_range", 1.0), ("tok_db", 0.0)):
        assert t[name].dtype == np.float32 and t[name].shape == (2, 6) and (t[name] == neutral).all()
    t = pipeline.emphasis_tables(2, 6, [(0, 1, 3, "strong"), (1, 0, 0, "reduced"), (0, 3, 4, "moderate"), (1, 5, 5, "strong"), (1, 5, 5, "none")])
    f = np.float32
    assert t["tok_db"].tolist() == [[0, 3, 3, 1.5, 1.5, 0], [-3, 0, 0, 0, 0, 0]], "the later span wins; `none` puts back to neutral"
    assert t["tok_speed"][0].tolist() == [1, f(0.9), f(0.9), f(0.95), f(0.95), 1] and t["tok_speed"][1, 0] == f(1.05)
    assert t["tok_f0_scale"][0].tolist() == [1, f(1.06), f(1.06), f(1.03), f(1.03), 1] and t["tok_f0_scale"][1, 0] == f(0.98)
    assert t["tok_range"][0].tolist() == [1, f(1.3), f(1.3), f(1.15), f(1.15), 1] and t["tok_range"][1].tolist() == [f(0.8), 1, 1, 1, 1, 1]
    assert set(pipeline.EMPHASIS_PRESETS) == {"strong", "moderate", "none", "reduced"} and pipeline.EMPHASIS_PRESETS["none"] == (1.0, 1.0, 1.0, 0.0)
    mine = dict(pipeline.EMPHASIS_PRESETS, strong=(0.8, 1.1, 1.5, 6.0))
    assert pipeline.emphasis_tables(1, 3, [(0, 0, 1, "strong")], presets=mine)["tok_db"].tolist() == [[6.0, 6.0, 0.0]]
    assert pipeline.EMPHASIS_PRESETS["strong"] == (0.90, 1.06, 1.3, 3.0), "the defaults are not written to"
    for bad in ([(2, 0, 1, "strong")], [(0, 3, 2, "strong")], [(0, 0, 6, "strong")], [(0, -1, 2, "strong")], [(0, 0, 1, "loud")], [(0, 0, 1)]):
        with pytest.raises(ValueError, match="emphasis_tables"):
            pipeline.emphasis_tables(2, 6, bad)
    # the arrays are what the three classes take
    v = pipeline.Volume(2, tok_db=t["tok_db"], device="cpu")
    assert v.N == 6 and v.tok_db.tolist() == t["tok_db"].tolist()
    it = pipeline.Intonation(2, tok_range=t["tok_range"], device="cpu")
    assert it.tok_range.tolist() == t["tok_range"].tolist()
