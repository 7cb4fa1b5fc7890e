"""C ABI and host-side contract of the loudness-normalised hand-over: `st2_wave_level`, its size helper
and `st2_wave_pack_level` are declared, exported and bound under ABI 23 and validate their arguments before any launch; the
numpy contract of tests/_level_ref.py reproduces the BS.1770-4 coefficient table and the standard's conformance figure; the
hand-over layout gains its fifth part without moving the other four; `pipeline` validates `Level` and leaves the calls without
it on the wrappers they always used.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _level_ref as R
from styletts2_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
LIBDIR = os.path.join(ROOT, "styletts2_amd")
NEW = ("st2_wave_level_workspace_bytes", "st2_wave_level", "st2_wave_pack_level")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b(int|int64_t) %s\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert not any("level" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)


def test_plain_c_translation_unit_calls_the_level_entry_points(tmp_path):
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers are not installed")
    src = tmp_path / "level.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "st2.h"
int main(void) {
  const char* m;
  if (st2_wave_level_workspace_bytes(8, 120, 600, 24000) != 8 * 30 * 12) return 1;
  if (st2_wave_level_workspace_bytes(8, 120, 600, 24001) != 0) return 2;
  if (st2_wave_level(NULL, 0, NULL, 2, 10, 600, 0, 24000, NULL, 0.9, 20.0, NULL, NULL, 0, NULL) == 0) return 3;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_wave_level")) return 4;
  if (st2_wave_pack_level(NULL, 0, NULL, 2, 10, 600, 0, 1, 1, NULL, 0, ST2_PCM_S16, NULL, 0, NULL, 0, NULL, NULL, NULL) == 0) return 5;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_wave_pack_level")) return 6;
  printf("ok %d\n", ST2_ABI_VERSION);
  return 0;
}
''')
    exe = str(tmp_path / "level")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + LIBDIR, "-lst2_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 23", (r.returncode, r.stdout, r.stderr)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------
D = C.c_void_p(256)
LEVEL_ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "rate", "target", "ceiling", "max_gain_db", "level", "work",
               "work_bytes")
PACK_ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "up", "down", "taps", "K", "fmt", "gaps", "gap_cap", "out", "cap",
              "offsets")


def test_wave_level_validates_before_any_launch():
    lib = _lib.load()
    need = lib.st2_wave_level_workspace_bytes(2, 10, 600, 24000)
    assert need == (2 * 3 * 12 + 15) // 16 * 16  # fp64 energies and fp32 peaks of ceil(6000 / 2400) hops per row
    assert lib.st2_wave_level_workspace_bytes(0, 10, 600, 24000) == 0 and lib.st2_wave_level_workspace_bytes(2, 10, 600, 24005) == 0
    base = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, rate=24000, target=D, ceiling=0.89, max_gain_db=20.0,
                level=D, work=D, work_bytes=need)
    for change, word in ((dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(B=70000), "bad geometry"), (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"),
                         (dict(trim=-1), "negative"), (dict(w_bs=5999), "w_bs"), (dict(wave=C.c_void_p(258)), "aligned"),
                         (dict(target=None), "NULL"), (dict(level=None), "NULL"), (dict(work=None), "NULL"),
                         (dict(work_bytes=need - 1), "too small"), (dict(rate=0), "sample_rate"), (dict(rate=-24000), "sample_rate"),
                         (dict(rate=22055), "sample_rate"), (dict(rate=2000000), "LDS"), (dict(ceiling=0.0), "ceiling"),
                         (dict(ceiling=1.0001), "ceiling"), (dict(ceiling=float("nan")), "ceiling"), (dict(max_gain_db=-0.1), "max_gain_db"),
                         (dict(max_gain_db=60.5), "max_gain_db"), (dict(max_gain_db=float("nan")), "max_gain_db"),
                         (dict(level=C.c_void_p(258)), "aligned"), (dict(work=C.c_void_p(260)), "aligned")):
        a = dict(base, **change)
        if "rate" in change and change["rate"] > 0 and change["rate"] % 10 == 0:  # sized for that rate: the refusal is the rate's own
            a["work_bytes"] = max(lib.st2_wave_level_workspace_bytes(2, 10, 600, change["rate"]), 16)
        assert lib.st2_wave_level(*[a[k] for k in LEVEL_ORDER], None) != 0, change
        assert "st2_wave_level:" in _err(lib) and word in _err(lib), (change, _err(lib))


def test_wave_pack_level_refuses_what_the_gaps_entry_refuses_in_its_own_name():
    lib = _lib.load()
    move = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, up=1, down=1, taps=None, K=0, fmt=_lib.PCM_S16, gaps=D,
                gap_cap=100, out=D, cap=12200, offsets=D)
    rs = dict(move, up=1, down=3, taps=D, K=16, fmt=_lib.PCM_ULAW)
    call = lambda a, level: lib.st2_wave_pack_level(*[a[k] for k in PACK_ORDER], None, level)
    for level in (None, D):
        for base, change, word in ((move, dict(wave=None), "NULL"), (move, dict(B=0), "bad geometry"), (move, dict(trim=-1), "negative"),
                                   (move, dict(fmt=7), "format"), (move, dict(w_bs=5999), "w_bs"), (move, dict(gap_cap=-1), "gap_cap"),
                                   (move, dict(up=2), "up="), (move, dict(fmt=_lib.PCM_ULAW), "taps"),
                                   (move, dict(gaps=C.c_void_p(258)), "aligned"), (rs, dict(up=0), ""), (rs, dict(K=513), ""),
                                   (rs, dict(fmt=4), ""), (rs, dict(up=1024, K=512), "LDS"), (rs, dict(taps=C.c_void_p(258)), "aligned")):
            assert call(dict(base, **change), level) != 0, change
            assert "st2_wave_pack_level" in _err(lib) and word in _err(lib), (change, _err(lib))
    for base in (move, rs):  # its one refusal of its own
        assert call(base, C.c_void_p(258)) != 0
        assert "st2_wave_pack_level: level is not aligned" in _err(lib), _err(lib)


def test_wrappers_have_no_cpu_path():
    w, f = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_level(w, f, torch.zeros(2))
    with pytest.raises(_lib.St2Error):
        ops.wave_pack_level(w, f, torch.zeros(2, 4))
    with pytest.raises(_lib.St2Error):
        ops.wave_pack_level(w, f, None)
    with pytest.raises(ValueError):
        ops.wave_pack_level(w, f, None, fmt="ulaw")  # G.711 needs the resampling move: a rate


# ---- the contract against the standard -----------------------------------------------------------------------------------------
def test_coefficients_at_48_khz_are_the_table_of_the_standard():
    (b1, a1), (b2, a2) = R.coefficients(48000)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             -1.99004745483398, 0.99007225036621]
    got = b1 + a1[1:] + a2[1:]
    assert max(abs(g - t) for g, t in zip(got, table)) <= 1e-12, got
    assert a1[0] == 1.0 and a2[0] == 1.0 and b2 == [1.0, -2.0, 1.0]
    assert abs(R.pole_radius(24000) - 0.990072) < 1e-6


def _sine(fs, seconds=3.0, f=997.0):
    t = np.arange(int(fs * seconds), dtype=np.float64) / fs
    return np.sin(2.0 * np.pi * f * t).astype(np.float32)


def test_full_scale_997_hz_sine_reads_the_conformance_figure():
    L48 = R.gate(R.blocks(_sine(48000), 48000))[0]
    assert abs(L48 - (-3.01)) <= 0.01, L48
    L24 = R.gate(R.blocks(_sine(24000), 24000))[0]  # the shelf is warped at the model rate
    assert abs(L24 - (-2.98)) <= 0.01, L24
    with pytest.raises(ValueError):
        R.blocks(_sine(22055, 0.1), 22055)


def test_contract_blocks_gates_and_gain_rules():
    fs, h = 24000, 2400
    g = np.random.default_rng(5)
    x = (g.standard_normal(5 * h + 77) * 0.05).astype(np.float32)
    y2 = R.k_weight(R.clean(x), fs) ** 2
    z = R.blocks(x, fs)
    assert len(z) == 2 and abs(z[1] - y2[h:5 * h].sum() / (4 * h)) <= 1e-15 * z[1] * 10
    assert len(R.blocks(x[:4 * h], fs)) == 1 and len(R.blocks(x[:4 * h - 1], fs)) == 1 and len(R.blocks(x[:0], fs)) == 0
    short = R.blocks(x[:5000], fs)
    assert abs(short[0] - y2[:5000].sum() / 5000) <= 1e-14 * short[0]  # the filter is causal: a prefix's output is a prefix
    # a NaN sample counts as 0 and is no peak
    xn = x.copy()
    xn[100] = np.nan
    x0 = x.copy()
    x0[100] = 0.0
    assert np.array_equal(R.blocks(xn, fs), R.blocks(x0, fs)) and R.peak(xn) == R.peak(x0)
    # the gates: silence in front is dropped by the absolute gate, a part 25 dB down by the relative one
    quiet = np.concatenate([np.zeros(10 * h, np.float32), x])
    L, passed, l, rel = R.gate(R.blocks(quiet, fs))
    assert not passed[:6].any() and passed[-1]
    L_all, passed_all, _, _ = R.gate(np.array([1e-2, 1e-2, 1e-2 * 10 ** -2.5]))
    assert passed_all.tolist() == [True, True, False] and abs(L_all - (-0.691 - 20.0)) < 1e-12
    assert R.gate(np.array([1e-8]))[0] == -math.inf and R.gate(np.zeros(0))[0] == -math.inf
    # the gain
    assert R.gain(-30.0, 0.1, -20.0, 0.5, 20.0) == np.float32(10 ** 0.5)  # the target
    assert R.gain(-30.0, 0.4, -20.0, 0.5, 20.0) == np.float32(0.5 / float(np.float32(0.4)))  # the ceiling
    assert R.gain(-60.0, 0.001, -20.0, 0.5, 20.0) == np.float32(10.0)  # the limit
    for L_, pk, tg in ((-30.0, 0.1, float("nan")), (-math.inf, 0.1, -20.0), (-30.0, 0.0, -20.0)):
        one = R.gain(L_, pk, tg, 0.5, 20.0)
        assert one.dtype == np.float32 and one == np.float32(1.0)


def test_warm_up_bound_of_the_kernel_meets_the_design_condition():
    """W = 4 ceil(0.032 fs): a chain from zero state W samples early is off by at most T(W) peak per sample; on a block above the
    absolute gate (sqrt(z) >= 3.4e-4) of a row that peaks at full scale that is 2 T / 3.4e-4 relative, which must stay below 1e-6."""
    for fs in (24000, 48000):
        W = 4 * ((32 * fs + 999) // 1000)
        T = R.tail_sum(fs, W)
        root_z = math.sqrt(10.0 ** ((R.ABS_GATE - R.OFFSET) / 10.0))
        rel = 2.0 * T / root_z + (T / root_z) ** 2
        print("fs %d: W = %d, T(W) = %.3g, relative block energy bound %.3g" % (fs, W, T, rel))
        assert W == {24000: 3072, 48000: 6144}[fs] and T <= 1.3e-12 and rel <= 1e-6
    assert abs(R.pole_radius(24000) ** 3072 - 4.9e-14) < 0.1e-14


# ---- the hand-over layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,marks,gaps,fmt", list(itertools.product((1, 3), (False, True), (False, True), ("f32", "s16", "ulaw"))))
def test_layout_with_the_level_part_and_without(B, marks, gaps, fmt):
    n_marks = B * 6 if marks else 0
    lay = pipeline._HandOver(B, fmt, n_marks, gaps, with_level=True)
    assert lay.offsets_at == 0 and lay.marks_at == 8 * (B + 1) and lay.gaps_at == 8 * (B + 1) + 4 * n_marks
    assert lay.level_at == lay.gaps_at + (4 * B if gaps else 0) and lay.level_at % 4 == 0
    assert lay.samples_at == (lay.level_at + 16 * B + 15) // 16 * 16
    ho = lay.allocate(10, "cpu")
    views = lay.views(ho.buf)
    assert len(views) == 5 and views[4].dtype == torch.float32 and views[4].numel() == 4 * B
    assert views[4].data_ptr() - ho.buf.data_ptr() == lay.level_at and ho.level.data_ptr() == views[4].data_ptr()
    assert views[3].data_ptr() - ho.buf.data_ptr() == lay.samples_at and views[3].numel() == 10
    assert (views[1] is None) == (not marks) and (views[2] is None) == (not gaps)
    # without the level part: the parent's layout, byte for byte, and a fifth view of None
    old = pipeline._HandOver(B, fmt, n_marks, gaps)
    assert old.samples_at == (8 * (B + 1) + 4 * n_marks + (4 * B if gaps else 0) + 15) // 16 * 16 and old.level_at == old.gaps_at + (
        4 * B if gaps else 0)
    old.allocate(10, "cpu")
    assert old.buf.numel() == old.samples_at + 10 * old.dtype.itemsize and old.views(old.buf)[4] is None and old.level is None


# ---- Level and the signatures ----------------------------------------------------------------------------------------------------
def test_level_validation():
    lv = pipeline.Level(3, device="cpu")
    assert lv.target.dtype == torch.float32 and lv.target.tolist() == [-16.0] * 3 and lv.max_gain_db == 20.0
    assert abs(lv.ceiling - 10 ** (-1 / 20)) < 1e-15 and lv.ceiling_db == -1.0
    lv = pipeline.Level(3, target=[-23.0, None, float("nan")], ceiling_db=0.0, max_gain_db=0, device="cpu")
    t = lv.target.tolist()
    assert t[0] == -23.0 and math.isnan(t[1]) and math.isnan(t[2]) and lv.ceiling == 1.0
    assert all(math.isnan(v) for v in pipeline.Level(2, target=None, device="cpu").target.tolist())
    assert pipeline.Level(4, target=[-10.0, -20.0, -30.0, -40.0], device="cpu").slice(1, 3).target.tolist() == [-20.0, -30.0]
    for bad in (dict(target=0.5), dict(target=-70.5), dict(target=[-16.0, -16.0]), dict(target=float("inf")), dict(ceiling_db=0.1),
                dict(ceiling_db=-20.5), dict(max_gain_db=-1), dict(max_gain_db=61), dict(ceiling_db=float("nan"))):
        with pytest.raises(ValueError, match="Level"):
            pipeline.Level(3, device="cpu", **bad)
    with pytest.raises(ValueError, match="Level"):
        pipeline.Level(0, device="cpu")


def test_signature_additions_and_refusals():
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(pipeline.Level.__init__))[1:] == ["B", "target", "ceiling_db", "max_gain_db", "device"]
    assert [sig(pipeline.Level.__init__)[k].default for k in ("target", "ceiling_db", "max_gain_db", "device")] == [-16.0, -1.0, 20.0, None]
    for f in (pipeline.inference, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__, pipeline.synthesize_long,
              pipeline._hand_over, pipeline.SynthesisResult.to_host):
        assert "level" in sig(f), f
    assert list(sig(pipeline._hand_over))[:9] == ["wave", "frames", "trim", "fmt", "samples_per_frame", "sample_rate", "n_marks", "gaps",
                                                  "max_gap"] and sig(pipeline._hand_over)["level"].default is None
    assert sig(pipeline.SynthesisResult.to_host)["level"].default is False
    tokens = torch.zeros(2, 5, dtype=torch.long)
    lv = pipeline.Level(2, device="cpu")
    with pytest.raises(ValueError, match="max_frames and pack"):
        pipeline.inference(None, None, tokens, level=lv)
    with pytest.raises(ValueError, match="max_frames and pack"):
        pipeline.inference(None, None, tokens, max_frames=10, level=lv)
    with pytest.raises(ValueError, match="Level of 2 rows"):
        pipeline.inference(None, None, tokens, max_frames=10, pack="s16", level=pipeline.Level(3, device="cpu"))
    with pytest.raises(ValueError, match="Level of 2 rows"):
        pipeline.inference(None, None, tokens, max_frames=10, pack="s16", level=-16.0)
    with pytest.raises(ValueError, match="capacity-bound"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], level=lv)
    res = pipeline.SynthesisResult(torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32), 2)
    assert res.level is None
    with pytest.raises(ValueError, match="level"):
        res.to_host(level=True)


# ---- _hand_over ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def spied(monkeypatch):
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append((name, a, kw))
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps", "wave_pack_level"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(ops, "wave_level", lambda wave, frames, target, **kw: seen.append(("wave_level", (target,), kw)) or kw["out"])
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    return seen


@pytest.mark.parametrize("gaps,fmt,rate", list(itertools.product((False, True), ("f32", "s16", "ulaw"), (None, 8000))))
def test_hand_over_measures_once_and_packs_once_with_a_level_and_calls_what_it_always_did_without(spied, gaps, fmt, rate):
    B, L, spf, max_gap = 3, 1200, 600, 7
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    lv = pipeline.Level(B, target=[-16.0, None, -23.0], ceiling_db=-2.0, max_gain_db=12.0, device="cpu")
    ho = pipeline._hand_over(wave, frames, 50, fmt, spf, rate, n_marks=B * 4, gaps=g, max_gap=max_gap if gaps else 0, level=lv)
    assert [s[0] for s in spied] == ["wave_level", "wave_pack_level"]
    _, (target,), kw = spied[0]
    assert target is lv.target and kw["out"].data_ptr() == ho.level.data_ptr() and kw["trim"] == 50 and kw["sample_rate"] == 24000
    assert kw["ceiling"] == lv.ceiling and kw["max_gain_db"] == 12.0 and kw["samples_per_frame"] == spf
    _, (table,), kw = spied[1]
    assert table.data_ptr() == ho.level.data_ptr() and kw["out"].data_ptr() == ho.packed.data_ptr() and kw["trim"] == 50
    assert (kw["gaps"] is None) == (not gaps) and kw["max_gap"] == (max_gap if gaps else 0)
    assert kw["rate"] == (rate if rate is not None else (24000 if fmt == "ulaw" else None))
    assert ho.level.numel() == 4 * B and ho.level.data_ptr() - ho.buf.data_ptr() == ho.level_at
    U, D = (1, 1) if kw["rate"] is None else pipeline.resample.ratio(kw["rate"])
    assert ho.packed.numel() == B * ((L * U + D - 1) // D + (max_gap if gaps else 0))
    # without a level: the parent's one call and the parent's buffer
    del spied[:]
    old = pipeline._hand_over(wave, frames, 50, fmt, spf, rate, n_marks=B * 4, gaps=g, max_gap=max_gap if gaps else 0)
    want = "wave_pack_gaps" if gaps else ("wave_resample_pack" if pipeline._resamples(fmt, rate) else "wave_pack")
    assert [s[0] for s in spied] == [want] and old.level is None and old.buf.numel() == ho.buf.numel() - (ho.samples_at - old.samples_at)
