"""C ABI and host-side contract of the look-ahead limiter of the hand-over: `st2_wave_limit` and its helpers
are declared, exported and bound under ABI 23 and refuse bad arguments before any launch; `Level` takes and validates the three
limiter options and is today's object without them; the hand-over layout gains its sixth part without moving the other five; the
numpy contract of tests/_limit_ref.py agrees with a per-sample loop and has the properties the design states; `_hand_over`
routes a limiting `Level` to `ops.wave_limit` and the un-levelled pack, a plain one to `ops.wave_pack_level`.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import re
import os

import numpy as np
import pytest
import torch

import _limit_ref as LR
from styletts2_amd import _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_wave_limit", "st2_wave_limit_workspace_bytes", "st2_wave_limit_tile")


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
    assert lib.st2_wave_limit_tile() == ops.LIMIT_TILE == 2048
    assert "st2_limit.hip" in __import__("styletts2_amd._build", fromlist=["x"]).SOURCES
    assert __import__("styletts2_amd._build", fromlist=["x"]).EXTRA_FLAGS["st2_limit.hip"] == ["-fno-slp-vectorize"]


D = C.c_void_p(4096)
ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "target", "ceiling", "max_gain_db", "level", "taps", "up", "K", "start",
         "drive_db", "W", "win", "out", "limit", "work", "work_bytes")


def test_wave_limit_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_limit_workspace_bytes(2, 10, 600)
    assert need == (4 * 2 * (6000 + 3 + 2) + 15) // 16 * 16  # r, the minima of ceil(6000 / 2048) tiles, {g', alone} per row
    assert lib.st2_wave_limit_workspace_bytes(0, 10, 600) == 0 and lib.st2_wave_limit_workspace_bytes(2, 10, 0) == 0
    far = C.c_void_p(4096 + (1 << 20))
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, target=D, ceiling=0.89, max_gain_db=20.0, level=D,
                taps=None, up=0, K=0, start=None, drive_db=6.0, W=192, win=D, out=far, limit=D, work=D, work_bytes=need)
    tp = dict(base, taps=D, up=8, K=82)
    cases = [(base, dict(wave=None), "NULL"), (base, dict(frames=None), "NULL"), (base, dict(B=0), "bad geometry"),
             (base, dict(B=70000), "bad geometry"), (base, dict(T_cap=0), "bad geometry"), (base, dict(spf=0), "bad geometry"),
             (base, dict(trim=-1), "negative"), (base, dict(w_bs=5999), "w_bs"), (base, dict(ceiling=0.0), "ceiling"),
             (base, dict(ceiling=1.0001), "ceiling"), (base, dict(ceiling=float("nan")), "ceiling"),
             (base, dict(max_gain_db=-0.1), "max_gain_db"), (base, dict(max_gain_db=60.5), "max_gain_db"),
             (base, dict(drive_db=-0.1), "drive_db"), (base, dict(drive_db=24.5), "drive_db"), (base, dict(drive_db=float("nan")), "drive_db"),
             (base, dict(W=0), "W=0"), (base, dict(W=1025), "W=1025"), (base, dict(work_bytes=need - 1), "too small"),
             (base, dict(out=D), "aliases"), (base, dict(out=C.c_void_p(4096 + 4 * 11000)), "aliases"),
             (base, dict(start=C.c_void_p(4098)), "start is not aligned"),
             (tp, dict(up=0), "ratio"), (tp, dict(K=513), "taps_per_phase"), (tp, dict(up=1024, K=512), "LDS"),
             (tp, dict(taps=C.c_void_p(4098)), "aligned")]
    cases += [(base, {k: None}, "NULL") for k in ("level", "target", "out", "limit", "win", "work")]
    cases += [(base, {k: C.c_void_p(4098)}, "not aligned to float") for k in ("wave", "level", "target", "limit", "win", "work")]
    cases += [(base, dict(out=C.c_void_p(4098 + (1 << 20))), "not aligned to float")]
    for b, change, word in cases:
        a = dict(b, **change)
        assert lib.st2_wave_limit(*[a[k] for k in ORDER], None) != 0, change
        assert _err(lib).startswith("st2_wave_limit:") and word in _err(lib), (change, _err(lib))


def test_wrapper_has_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_limit(w, f, torch.zeros(2, 4), torch.zeros(2), torch.ones(3) / 3)
    sig = list(inspect.signature(ops.wave_limit).parameters)
    assert sig[:5] == ["wave", "frames", "level", "target", "win"] and {"drive_db", "true_peak", "starts", "out", "limit"} <= set(sig)


# ---- Level ---------------------------------------------------------------------------------------------------------------------
def test_level_takes_and_validates_the_limiter_options_and_is_todays_object_without_them():
    plain = pipeline.Level(3, device="cpu")
    assert set(vars(plain)) == {"B", "ceiling_db", "max_gain_db", "ceiling", "target", "true_peak", "scope"}
    assert (plain.limiter, plain.drive_db, plain.window_ms, plain.W) == (False, 6.0, 8.0, 192)
    same = pipeline.Level(3, device="cpu", limiter=False, drive_db=6.0, window_ms=8.0)
    assert set(vars(same)) == set(vars(plain)) and all(
        torch.equal(vars(same)[k], v) if torch.is_tensor(v) else vars(same)[k] == v for k, v in vars(plain).items())
    lv = pipeline.Level(3, target=[-16.0, None, -20.0], device="cpu", limiter=True, drive_db=9, window_ms=0.5, true_peak=True)
    assert (lv.limiter, lv.drive_db, lv.window_ms, lv.W, lv.true_peak) == (True, 9.0, 0.5, 12, True)
    assert pipeline.Level(1, device="cpu", limiter=True, window_ms=40).W == 960
    part = lv.slice(1, 3)
    assert (part.limiter, part.drive_db, part.W, part.true_peak, part.B) == (True, 9.0, 12, True, 2)
    assert plain.slice(0, 2).limiter is False and set(vars(plain.slice(0, 2))) == set(vars(plain))
    assert lv.options() == dict(true_peak=True, scope="row", limiter=True, drive_db=9.0, window_ms=0.5)
    for bad in (dict(drive_db=-1), dict(drive_db=24.5), dict(drive_db=float("nan")), dict(window_ms=0.4), dict(window_ms=41),
                dict(window_ms=float("nan"))):
        with pytest.raises(ValueError, match="Level"):
            pipeline.Level(3, device="cpu", limiter=True, **bad)
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(pipeline.Level.__init__))[1:] == ["B", "target", "ceiling_db", "max_gain_db", "device"]
    assert sig(pipeline.SynthesisResult.to_host)["limit"].default is False


# ---- the hand-over layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,fmt", list(itertools.product((1, 3), (False, True), (False, True), ("f32", "ulaw"))))
def test_layout_with_the_limit_part_and_without(B, marks, gaps, fmt):
    n_marks = B * 6 if marks else 0
    old = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=True)
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=True, with_limit=True)
    assert (lay.offsets_at, lay.marks_at, lay.gaps_at, lay.level_at) == (old.offsets_at, old.marks_at, old.gaps_at, old.level_at)
    assert lay.limit_at == lay.level_at + 16 * B and lay.samples_at == (lay.limit_at + 8 * B + 15) // 16 * 16
    assert old.limit_at == lay.limit_at and old.samples_at == (old.level_at + 16 * B + 15) // 16 * 16  # today's, byte for byte
    ho = lay.allocate(10, "cpu")
    assert len(lay.views(ho.buf)) == 5 and ho.limit.dtype == torch.float32 and ho.limit.numel() == 2 * B
    assert ho.limit.data_ptr() - ho.buf.data_ptr() == lay.limit_at and ho.packed.data_ptr() - ho.buf.data_ptr() == lay.samples_at
    assert ho.level.data_ptr() - ho.buf.data_ptr() == lay.level_at and ho.level.numel() == 4 * B
    old.allocate(10, "cpu")
    assert old.limit is None and old.limit_view(old.buf) is None and old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize


# ---- the window and the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 7, 12, 192, 960, 1024])
def test_limit_window_is_non_negative_symmetric_and_sums_to_one(W):
    win = resample.limit_window_design(W)
    assert win.dtype == np.float32 and win.shape == (2 * W + 1,) and (win > 0).all()
    assert np.array_equal(win, win[::-1]) and abs(float(win.astype(np.float64).sum()) - 1.0) <= 2.0 ** -20
    assert np.array_equal(win, LR.window(W)) and win.argmax() == W
    with pytest.raises(ValueError):
        resample.limit_window_design(0)
    with pytest.raises(ValueError):
        resample.limit_window_design(1025)


def _row(n, seed, over=()):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 0.1).astype(np.float32)
    for i, v in over:
        x[i] = v
    return x


@pytest.mark.parametrize("W,n", [(1, 9), (3, 2), (3, 6), (3, 7), (5, 40)])
def test_contract_agrees_with_a_per_sample_loop(W, n):
    x = _row(n, W * 100 + n, over=[(0, 0.9), (n - 1, -1.4), (n // 2, np.nan)])
    win, c, g = LR.window(W), 0.7, np.float32(1.3)
    ref = LR.limit_row(x, g, c, W, win)
    out, q = LR.brute(x, g, c, W, win)
    assert np.allclose(ref["out"], out, rtol=0, atol=1e-15) and np.allclose(ref["q"], q, rtol=0, atol=1e-15)
    assert ref["r"].dtype == np.float32 and ref["m"].shape == (n + 2 * W,) and ref["r"][n // 2] == 1.0


def test_contract_properties():
    W, c, g = 7, 0.5, np.float32(2.0)
    win = LR.window(W)
    n = 400
    x = _row(n, 3)
    x[np.abs(x) * 2.0 > c] = 0.2  # everything under the ceiling after the gain, but for the three set below
    x[100], x[101], x[300] = 0.9, -0.7, 0.3
    ref = LR.limit_row(x, g, c, W, win)
    assert (ref["q"] <= ref["r"]).all() and (ref["q"] > 0).all()
    assert (np.abs(ref["out"]) <= c * (1 + 2.0 ** -21)).all()
    over = np.flatnonzero(ref["r"] < 1.0)
    assert over.tolist() == [100, 101, 300]
    far = np.ones(n, bool)
    for i in over:
        far[max(0, i - 2 * W):i + 2 * W + 1] = False
    assert far.sum() > 200 and np.array_equal(ref["out"][far], ref["xg"][far].astype(np.float64)), "x g' farther than 2 W from a peak"
    assert (ref["q"][~far] <= 1.0).all() and ref["q"][100] <= c / (0.9 * 2.0) * (1 + 1e-6)
    # a row under the ceiling: q is 1 everywhere
    under = LR.limit_row(np.clip(x, -0.2, 0.2), g, c, W, win)
    assert (under["q"] == 1.0).all() and np.array_equal(under["out"], under["xg"].astype(np.float64))
    # rule 1
    assert LR.drive_gain(-30.0, 0.5, -20.0, 0.5, 20.0, 6.0) == np.float32(min(10 ** 0.5, 10 ** 0.3 * 0.5 / 0.5))
    assert LR.drive_gain(-30.0, 0.01, -20.0, 0.5, 20.0, 0.0) == np.float32(10 ** 0.5)
    assert LR.drive_gain(-30.0, 0.5, -20.0, 0.5, 20.0, 0.0) == np.float32(1.0)
    for L, pk, t in ((-30.0, 0.1, float("nan")), (-np.inf, 0.1, -20.0), (-30.0, 0.0, -20.0)):
        assert LR.drive_gain(L, pk, t, 0.5, 20.0, 6.0) is None
    # with drive 0 and the row's own sample peak the limiter has nothing to do but rounding
    g0 = LR.drive_gain(-30.0, np.abs(x).max(), 0.0, c, 60.0, 0.0)
    assert LR.limit_row(x, g0, c, W, win)["q"].min() >= 1 - 2.0 ** -22


# ---- routing -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def spied(monkeypatch):
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append((name, wave, a, kw))
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps", "wave_pack_level"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(ops, "wave_level", lambda wave, frames, target, **kw: seen.append(("wave_level", wave, (target,), kw)) or kw["out"])

    def limit(wave, frames, level, target, win, **kw):
        seen.append(("wave_limit", wave, (level, target, win), kw))
        return torch.full_like(wave[:, 0], 5.0), kw["limit"]
    monkeypatch.setattr(ops, "wave_limit", limit)
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    monkeypatch.setattr(pipeline.resample, "limit_window", lambda W, dev: torch.from_numpy(resample.limit_window_design(W)))
    monkeypatch.setattr(pipeline.resample, "true_peak_table", lambda dev: (8, 82, None))
    return seen


@pytest.mark.parametrize("gaps,fmt,rate", list(itertools.product((False, True), ("s16", "ulaw"), (None, 8000))))
def test_hand_over_limits_then_packs_without_a_level_and_a_plain_level_packs_as_it_did(spied, gaps, fmt, rate):
    B, L, spf, max_gap = 3, 1200, 600, 7
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = pipeline.Level(B, target=[-16.0, None, -23.0], ceiling_db=-2.0, max_gain_db=12.0, device="cpu", limiter=True, drive_db=4.0,
                        window_ms=1.0, true_peak=True)
    ho = pipeline._hand_over(wave, frames, 50, fmt, spf, rate, n_marks=B * 4, gaps=g, max_gap=max_gap if gaps else 0, level=lv)
    want = "wave_pack_gaps" if gaps else ("wave_resample_pack" if pipeline._resamples(fmt, rate) else "wave_pack")
    assert [s[0] for s in spied] == ["wave_level", "wave_limit", want]
    _, w, (table, target, win), kw = spied[1]
    assert w is wave and table.data_ptr() == ho.level.data_ptr() and target is lv.target and win.numel() == 2 * 24 + 1
    assert kw["limit"].data_ptr() == ho.limit.data_ptr() and kw["drive_db"] == 4.0 and kw["ceiling"] == lv.ceiling
    assert kw["max_gain_db"] == 12.0 and kw["trim"] == 50 and kw["samples_per_frame"] == spf and kw["true_peak"] == (8, 82, None)
    assert spied[0][3]["true_peak"] == (8, 82, None) and "starts" not in kw
    _, w, a, kw = spied[2]
    assert bool((w == 5.0).all()), "the pack reads the limited rows"
    assert "level" not in kw and kw["out"].data_ptr() == ho.packed.data_ptr() and kw["trim"] == 50
    assert ho.limit.numel() == 2 * B and ho.limit_at == ho.level_at + 16 * B
    # a plain Level: the parent's two calls and the parent's buffer
    del spied[:]
    plain = pipeline.Level(B, target=[-16.0, None, -23.0], ceiling_db=-2.0, max_gain_db=12.0, device="cpu")
    old = pipeline._hand_over(wave, frames, 50, fmt, spf, rate, n_marks=B * 4, gaps=g, max_gap=max_gap if gaps else 0, level=plain)
    assert [s[0] for s in spied] == ["wave_level", "wave_pack_level"] and old.limit is None
    assert old.buf.numel() == ho.buf.numel() - (ho.samples_at - old.samples_at)
    res = pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output("s16", 0), ho)
    assert tuple(res.limit.shape) == (B, 2) and res.limit.data_ptr() == ho.limit.data_ptr()
    with pytest.raises(ValueError, match="limit"):
        pipeline.SynthesisResult(torch.zeros(B, 1, L), frames, 2, pipeline._Output("s16", 0), old).to_host(limit=True)
