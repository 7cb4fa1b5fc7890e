"""C ABI and host-side contract of fit-to-duration: the numpy contract of tests/_fit_ref.py equals a
brute-force apportionment and has the five stated properties over committed seeds, every flag is reached; `st2_durations_fit`
is declared, exported and bound under ABI 23 without a backend slot and refuses bad arguments before any launch; `pipeline`
takes `fit_frames` / `fit_hold` on its entry points, refuses what does not go with them and, without them, never reaches the
new launch.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _fit_ref as R
from styletts2_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
LIBDIR = os.path.join(ROOT, "styletts2_amd")
SEEDS = (20261, 20262, 20263, 20264)
ROWS_PER_SEED = 1500


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_contract_by_hand():
    # 3 + 1 + 4 = 8 frames to 12: lo = 3, R = 9, m = (2, 0, 3), M = 5: q = (3, 0, 5), r = (3, 0, 2), K = 1 -> token 0
    assert R.fit_row([3, 1, 4], 3, 12, None, 100) == ([5, 1, 6], (8, 12, R.OK, 2))
    # the same to 3 frames: everything to one frame; to 2: infeasible, the nearest total is lo = 3
    assert R.fit_row([3, 1, 4], 3, 3, None, 100) == ([1, 1, 1], (8, 3, R.OK, 2))
    assert R.fit_row([3, 1, 4], 3, 2, None, 100) == ([1, 1, 1], (8, 3, R.NEAREST, 2))
    # the target S is the identity; a zero duration counts as one frame and is written as one
    assert R.fit_row([3, 1, 4], 3, 8, None, 100) == ([3, 1, 4], (8, 8, R.OK, 0))
    assert R.fit_row([3, 0, 4], 3, 8, None, 100) == ([3, 1, 4], (8, 8, R.OK, 1))
    # all equal: every remainder ties, the lower indices take the K frames; all ones: the fallback shares R the same way
    assert R.fit_row([2, 2, 2, 2], 4, 10, None, 100) == ([3, 3, 2, 2], (8, 10, R.OK, 2))
    assert R.fit_row([1, 1, 1, 1], 4, 10, None, 100) == ([3, 3, 2, 2], (4, 10, R.OK, 4))
    # a held token keeps its frames, the free ones take the rest; a short row's tail is zeros; the capacity bounds T'
    assert R.fit_row([3, 5, 4, 9], 3, 20, [0, 1, 0, 0], 100) == ([6, 5, 9, 0], (12, 20, R.OK, 2))
    assert R.fit_row([3, 5, 4], 3, 50, None, 30)[1] == (12, 30, R.NEAREST, 3)
    # rows that are not apportioned come back whole, tail included
    assert R.fit_row([3, 5, 4, 9], 3, 0, None, 100) == ([3, 5, 4, 9], (12, 12, R.OK, 0))
    assert R.fit_row([3, 5, 4, 9], 0, 7, None, 100) == ([0, 0, 0, 0], (0, 0, R.NOTHING_FREE, 0))
    assert R.fit_row([3, 5, 4, 9], 3, 7, [1, 1, 1, 0], 100) == ([3, 5, 4, 9], (12, 12, R.NOTHING_FREE, 0))
    assert R.fit_row([3, 5, 4, 9], 3, 7, [0, 1, 1, 0], 9) == ([3, 5, 4, 9], (12, 12, R.REFUSED, 0))
    big = 2 ** 31 - 1
    assert R.fit_row([big, big, 1], 3, 7, None, 100) == ([big, big, 1], (big, big, R.REFUSED, 0))
    assert R.fit_row([2 ** 62, 2 ** 62], 2, 0, None, 100)[1] == (big, big, R.OK, 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_contract_equals_brute_force_and_has_the_five_properties(seed):
    rng = np.random.default_rng(seed)
    flags = set()
    for _ in range(ROWS_PER_SEED):
        dur, n_b, target, hold, T_cap = R.random_row(rng)
        out, rep = R.fit_row(dur, n_b, target, hold, T_cap)
        assert (out, rep) == R.fit_row_brute(dur, n_b, target, hold, T_cap), (dur, n_b, target, hold, T_cap)
        S, T, flag, changed = rep
        flags.add(flag)
        v = [max(d, 1) for d in dur[:n_b]]
        held = [hold is not None and bool(hold[n]) for n in range(n_b)]
        assert S == sum(v)
        if flag in (R.NOTHING_FREE, R.REFUSED):
            assert out == (dur if n_b else [0] * len(dur)) and T == S and changed == 0
            continue
        lo = sum(x if h else 1 for x, h in zip(v, held))
        assert sum(out) == T and out[n_b:] == [0] * (len(dur) - n_b)                              # 1. the sum is T' exactly
        assert (T == target) == (lo <= target <= T_cap) == (flag == R.OK)                         # 2. feasible targets are met
        assert T == min(max(target, lo), T_cap)
        assert T != S or out[:n_b] == v                                                           # 3. S is the identity
        assert all(out[n] == v[n] for n in range(n_b) if held[n])                                 # 4. held tokens stay
        free = sorted((v[n], out[n]) for n in range(n_b) if not held[n])                          # 5. monotone among free tokens
        assert all(a[1] <= b[1] for a, b in zip(free, free[1:]) if a[0] < b[0])
        assert all(o >= 1 for o in out[:n_b]) and changed == sum(out[n] != dur[n] for n in range(n_b))
    assert flags == {R.OK, R.NEAREST, R.NOTHING_FREE, R.REFUSED}, flags


def test_batch_form_rows_depend_on_themselves_alone():
    rng = np.random.default_rng(SEEDS[0])
    N = 9
    rows = [R.random_row(rng, N=N) for _ in range(3)]
    hold = [[0] * N if r[3] is None else r[3] for r in rows]
    pick = lambda idx: R.fit([rows[i][0] for i in idx], [rows[i][1] for i in idx], [rows[i][2] for i in idx], [hold[i] for i in idx], 64)
    o3, r3 = pick([0, 1, 2])
    o2, r2 = pick([2, 0])
    assert o3.dtype == np.int64 and r3.dtype == np.int32 and o3.shape == (3, N) and r3.shape == (3, 4)
    assert np.array_equal(o2, o3[[2, 0]]) and np.array_equal(r2, r3[[2, 0]])
    assert np.array_equal(R.fit([rows[0][0]], None, [5], None, 64, row=R.fit_row_brute)[0], R.fit([rows[0][0]], [N], [5], [[0] * N], 64)[0])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    assert re.search(r"\bint st2_durations_fit\(", text)
    assert hasattr(lib, "st2_durations_fit") and "st2_durations_fit" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert not any("fit" in s.split("_") for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)
    assert (ops.FIT_OK, ops.FIT_NEAREST, ops.FIT_NOTHING_FREE, ops.FIT_REFUSED) == (R.OK, R.NEAREST, R.NOTHING_FREE, R.REFUSED) == (0, 1, 2, 3)
    assert _lib.STATUS_FRAME_CAPACITY == 16 and "ST2_STATUS_FIT" not in text  # no new sticky status bit


def test_plain_c_translation_unit_calls_the_fit_entry_point(tmp_path):
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers are not installed")
    src = tmp_path / "fit.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "st2.h"
int main(void) {
  const char* m;
  if (st2_durations_fit(NULL, 2, 16, NULL, NULL, NULL, 96, NULL, NULL, NULL) == 0) return 1;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_durations_fit:") || !strstr(m, "NULL")) return 2;
  printf("ok %d\n", ST2_ABI_VERSION);
  return 0;
}
''')
    exe = str(tmp_path / "fit")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + LIBDIR, "-lst2_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 23", (r.returncode, r.stdout, r.stderr)


D = C.c_void_p(256)
ORDER = ("dur", "B", "N", "len", "target", "hold", "T_cap", "out", "report")


def test_durations_fit_validates_before_any_launch():
    lib = _lib.load()
    base = dict(dur=D, B=3, N=16, len=None, target=D, hold=None, T_cap=96, out=D, report=None)
    for change, word in ((dict(dur=None), "NULL"), (dict(target=None), "NULL"), (dict(out=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(B=-1), "bad geometry"), (dict(B=65536), "bad geometry"), (dict(N=0), "bad geometry"),
                         (dict(N=-3), "bad geometry"), (dict(N=513), "bad geometry"), (dict(T_cap=0), "T_cap"), (dict(T_cap=-5), "T_cap"),
                         (dict(dur=C.c_void_p(260)), "aligned"), (dict(out=C.c_void_p(260)), "aligned"),
                         (dict(len=C.c_void_p(258)), "aligned"), (dict(target=C.c_void_p(258)), "aligned"),
                         (dict(report=C.c_void_p(257)), "aligned")):
        a = dict(base, **change)
        assert lib.st2_durations_fit(*[a[k] for k in ORDER], None) != 0, change  # (a launch would read the made-up pointers)
        assert "st2_durations_fit:" in _err(lib) and word in _err(lib), (change, _err(lib))


def test_wrapper_has_no_cpu_path_and_checks_its_operands():
    dur, target = torch.ones(3, 8, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.durations_fit(dur, target, 96)
    with pytest.raises(_lib.St2Error):
        ops.durations_fit([[1, 2]], target, 96)
    with pytest.raises(_lib.St2Error):
        ops.durations_fit(dur.to(torch.int32), target, 96)
    assert list(inspect.signature(ops.durations_fit).parameters) == ["dur", "target", "T_cap", "lengths", "hold", "out", "report"]


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------
def test_fit_frames_converts_seconds_to_frames():
    assert pipeline.fit_frames(3.2) == 128 and pipeline.fit_frames(3.2, trim=50) == 128  # 76 800 samples; 76 850 / 600 = 128.08
    assert pipeline.fit_frames(1.0) == 40 and pipeline.fit_frames(0.0) == 1 and pipeline.fit_frames(0.001) == 1
    assert pipeline.fit_frames(1.0, trim=300) == round(24300 / 600) == 40 and pipeline.fit_frames(1.0, trim=301) == 41
    assert pipeline.fit_frames([0.5, 2, 3.2]) == [20, 80, 128] and pipeline.fit_frames((1,)) == [40]
    for text in ("600 samples", "25 ms", "tail frames", "durations="):
        assert text in pipeline.fit_frames.__doc__, text


def test_signature_additions_and_refusals():
    sig = lambda f: inspect.signature(f).parameters
    for f in (pipeline.inference, pipeline.GraphedSynthesis.__call__, pipeline.synthesize_long):
        assert "fit_frames" in sig(f) and sig(f)["fit_frames"].default is None, f
    for f in (pipeline.inference, pipeline.GraphedSynthesis.__call__):
        assert "fit_hold" in sig(f) and sig(f)["fit_hold"].default is None, f
    assert sig(pipeline.GraphedSynthesis.__init__)["fit"].default is False and sig(pipeline.prepare)["fit"].default is None
    assert sig(pipeline.SynthesisResult.__init__)["fit"].default is None
    for f in (pipeline._hand_over, pipeline._output_spec):  # inputs, not output options
        assert "fit_frames" not in sig(f) and "fit_hold" not in sig(f) and "fit" not in sig(f)
    assert "fit" not in pipeline._Output._fields and "fit" not in sig(pipeline._HandOver.__init__)
    res = pipeline.SynthesisResult(torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32), 2)
    assert res.fit is None
    tokens = torch.zeros(2, 5, dtype=torch.long)
    for kw in (dict(fit_frames=[10, 0]), dict(fit_hold=torch.zeros(2, 5, dtype=torch.bool)),
               dict(fit_frames=[10, 0], fit_hold=torch.zeros(2, 5, dtype=torch.bool))):
        with pytest.raises(ValueError, match="fit_frames / fit_hold belong to the capacity-bound path: pass max_frames"):
            pipeline.inference(None, None, tokens, **kw)
    with pytest.raises(ValueError, match="pass fit_frames"):
        pipeline.inference(None, None, tokens, max_frames=20, fit_hold=torch.zeros(2, 5, dtype=torch.bool))
    for bad in ([10], [10, 0, 3], [1.5, 2], [True, 2], 7, "ab", torch.zeros(2, 1, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                [-1, 4], [4, 21], torch.tensor([0, 21])):
        with pytest.raises(ValueError, match="fit_frames must"):
            pipeline.inference(None, None, tokens, max_frames=20, fit_frames=bad)
    for bad in (torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2, 5), [[0] * 5] * 2):  # not on the device / no flags / no tensor
        with pytest.raises(ValueError, match="fit_hold must be"):
            pipeline.inference(None, None, tokens, max_frames=20, fit_frames=[20, 0], fit_hold=bad)
    with pytest.raises(ValueError, match="fit_frames / fit_hold belong to the capacity-bound path: pass max_frames"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], fit_frames=[7, 0])
    for bad in ([7], [7, 21], [7, -2], torch.zeros(2, dtype=torch.int64).tolist() + [1]):
        with pytest.raises(ValueError, match="fit_frames must"):
            pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], max_frames=20, fit_frames=bad)
    with pytest.raises(ValueError, match="capacity-bound path"):
        pipeline.prepare(None, None, tokens, fit=(torch.zeros(2, dtype=torch.int32), None))


def test_check_fit_passes_what_it_accepts_through():
    assert pipeline._check_fit([3, 0], None, 2, 5, 20) == ([3, 0], None)
    assert pipeline._check_fit((20, 0), None, 2, 5, 20) == ([20, 0], None)
    assert pipeline._check_fit(torch.tensor([3, 0]), None, 2, 5, 20) == ([3, 0], None)  # a host tensor is a host sequence


class _Reached(Exception):
    pass


def test_without_the_arguments_the_new_launch_is_never_reached(monkeypatch):
    """`inference` hands `prepare` a `fit` only when the caller gave the arguments, and `prepare` is the one caller of
    `ops.durations_fit`: a call without them takes the path it always took."""
    seen = []

    def stub(model, sampler, tokens, **kw):
        seen.append(kw)
        raise _Reached()

    calls, real_prepare = [], inspect.getsource(pipeline.prepare)
    monkeypatch.setattr(pipeline, "prepare", stub)
    monkeypatch.setattr(ops, "durations_fit", lambda *a, **k: calls.append(a))
    monkeypatch.setattr(pipeline, "_fit_on", lambda fit, dev: fit)  # (the upload needs a device)
    tokens = torch.zeros(2, 5, dtype=torch.long)
    for more in (dict(), dict(max_frames=20), dict(max_frames=20, pack="s16")):
        with pytest.raises(_Reached):
            pipeline.inference(None, None, tokens, **more)
        assert "fit" not in seen[-1], more
    with pytest.raises(_Reached):
        pipeline.inference(None, None, tokens, max_frames=20, fit_frames=[7, 0])
    assert seen[-1]["fit"] == ([7, 0], None) and calls == []
    src = inspect.getsource(pipeline)
    assert src.count("ops.durations_fit(") == 1 and "ops.durations_fit(" in real_prepare
    assert re.search(r"if fit is not None:[^\n]*\n\s+durations, fitted\[\"fit\"\] = ops\.durations_fit\(", real_prepare)
