"""C ABI and host-side contract of the per-request controls: the new entry points are declared, exported
and bound under ABI 23 without a version bump or a backend-table slot, their arguments are validated before any launch,
`pipeline.Controls` validates host values, the pipeline refuses what it cannot serve, and the numpy contract is pinned on its
tie cases.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _controls_ref as R
from styletts2_amd import _hooks, _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
LIBDIR = os.path.join(ROOT, "styletts2_amd")
NEW = ("st2_duration_head_rate", "st2_style_mix_rows", "st2_prosody_controls", "st2_front_forward_ctl", "st2_sizeof_controls")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_abi_stays_23_and_the_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in st2.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in _lib.EXPORTS
    # additive: no struct grew, no backend-table slot was added
    assert lib.st2_sizeof_front_args() == C.sizeof(_lib.FrontArgs)
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3


def test_sizeof_controls_matches_the_ctypes_struct():
    lib = _lib.load()
    assert lib.st2_sizeof_controls() == C.sizeof(_lib.ControlRows) == 4 * C.sizeof(C.c_void_p)
    assert [f[0] for f in _lib.ControlRows._fields_] == ["speed", "alpha", "beta", "t"]
    assert re.search(r"const float \*speed, \*alpha, \*beta, \*t;", open(HEADER).read())


def test_plain_c_translation_unit_calls_the_control_entry_points(tmp_path):
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers are not installed")
    src = tmp_path / "controls.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "st2.h"
int main(void) {
  st2_controls ctl = {NULL, NULL, NULL, NULL};
  const char* m;
  if (st2_sizeof_controls() != (int)sizeof(st2_controls)) return 1;
  if (st2_duration_head_rate(NULL, 0, 0, NULL, NULL, 2, 512, 50, 4, NULL, 0, NULL, NULL, NULL, NULL) == 0) return 2;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_duration_head_rate")) return 3;
  if (st2_style_mix_rows(NULL, NULL, NULL, NULL, NULL, NULL, 0.7, 0.3, 0.7, 2, 128, 0, NULL, NULL, NULL, NULL) == 0) return 4;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_style_mix_rows")) return 5;
  if (st2_prosody_controls(NULL, NULL, 0, 2, 8, NULL, NULL, NULL, NULL) == 0) return 6;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_prosody_controls")) return 7;
  if (st2_front_forward_ctl(NULL, NULL, &ctl, NULL, 0, NULL) == 0) return 8;
  printf("ok %d\n", ST2_ABI_VERSION);
  return 0;
}
''')
    exe = str(tmp_path / "controls")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + LIBDIR, "-lst2_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 23", (r.returncode, r.stdout, r.stderr)


def test_kernel_entry_points_validate_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    f = lib.st2_duration_head_rate
    ok = dict(x=d, x_bs=2048, x_cs=4, w=d, bias=d, B=2, K=512, J=50, N=4, len=None, tail=0, speed=d, dur=d, dsum=None)
    for change, word in ((dict(x=None), "NULL"), (dict(speed=None), "NULL"), (dict(dur=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(N=-1), "bad geometry"), (dict(tail=-1), "bad geometry"), (dict(B=70000), "grid")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_duration_head_rate" in _err(lib) and word in _err(lib), (change, _err(lib))
    f = lib.st2_style_mix_rows
    ok = dict(sp=d, prev=None, ref_s=None, t=None, alpha=None, beta=None, t0=0.7, a0=0.3, b0=0.7, B=2, sty=128, carry=0, ref=d,
              s=d, out=None)
    for change, word in ((dict(sp=None), "NULL"), (dict(ref=None), "NULL"), (dict(s=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(sty=0), "bad geometry"), (dict(t0=1.5), "[0, 1]"), (dict(a0=-0.1), "[0, 1]"),
                         (dict(b0=float("nan")), "[0, 1]")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_style_mix_rows" in _err(lib) and word in _err(lib), (change, _err(lib))
    f = lib.st2_prosody_controls
    ok = dict(f0=d, n=d, bs=16, B=2, L=16, sc=d, sh=d, frames=None)
    for change, word in ((dict(f0=None), "NULL"), (dict(n=None), "NULL"), (dict(B=0), "bad geometry"), (dict(L=0), "bad geometry"),
                         (dict(bs=15), "bad geometry")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_prosody_controls" in _err(lib) and word in _err(lib), (change, _err(lib))
    assert f(d, d, 16, 2, 16, None, None, None, None) == 0  # nothing to apply: no launch, no error


def test_wrappers_have_no_cpu_path_and_check_their_rows_first():
    x, w, b = torch.zeros(2, 8, 4), torch.zeros(5, 8), torch.zeros(5)
    with pytest.raises(_lib.St2Error, match="speed"):
        ops.duration_head(x, w, b, speed=torch.ones(2))  # a host row never reaches a launch
    with pytest.raises(_lib.St2Error, match="speed"):
        ops.duration_head(x, w, b, speed=[1.0, 1.0])
    with pytest.raises(_lib.St2Error):
        ops.style_mix_rows(torch.zeros(2, 256))
    with pytest.raises(_lib.St2Error, match="alpha"):
        ops.style_mix_rows(torch.zeros(2, 256), alpha=torch.ones(2, dtype=torch.float64))
    with pytest.raises(_lib.St2Error):
        ops.prosody_controls(torch.zeros(2, 8), torch.zeros(2, 8), f0_scale=None, n_shift=None)
    with pytest.raises(_lib.St2Error, match="f0_scale"):
        ops.prosody_controls(torch.zeros(2, 8), torch.zeros(2, 8), f0_scale=torch.ones(3))


BAD = {"speed": (0.2, 4.5, 0.0, -1.0), "alpha": (-0.01, 1.01), "beta": (-1.0, 2.0), "t": (-0.5, 1.5), "f0_scale": (0.49, 2.1, 0.0),
       "n_shift": (-2.5, 2.01)}


@pytest.mark.parametrize("name", pipeline.Controls.NAMES)
def test_controls_validates_every_host_value(name):
    lo, hi = pipeline.Controls.RANGES[name]
    assert (lo, hi) == R.RANGES[name]
    for bad in BAD[name] + (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(3, device="cpu", **{name: bad})
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(3, device="cpu", **{name: [lo, bad, hi]})  # one bad value in a sequence
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(3, device="cpu", **{name: torch.tensor([lo, hi, bad])})  # ... or in a host tensor
    with pytest.raises(ValueError, match=name):
        pipeline.Controls(3, device="cpu", **{name: [lo, hi]})  # two values for three rows
    c = pipeline.Controls(3, device="cpu", **{name: [lo, hi, (lo + hi) / 2]})  # the ends of the range are legal
    assert c.present == (name,) and c.row(name).tolist() == [np.float32(lo), np.float32(hi), np.float32((lo + hi) / 2)]
    assert all(c.row(n) is None for n in c.NAMES if n != name)


def test_controls_layout_neutral_and_slices():
    c = pipeline.Controls(4, speed=[1, 0.5, 2, 4], t=0.25, device="cpu")
    assert c.buf.shape == (6, 4) and c.buf.dtype == torch.float32 and c.B == 4
    assert set(c.front_rows()) == {"speed", "t"} and c.row("t").tolist() == [0.25] * 4
    # an absent row holds what the device clamp turns into "no control": 1 / NaN (the call's scalar) / 0
    assert c.buf[4].tolist() == [1.0] * 4 and c.buf[5].tolist() == [0.0] * 4 and bool(torch.isnan(c.buf[1:3]).all())
    s = c.slice(1, 3)
    assert s.B == 2 and s.row("speed").tolist() == [0.5, 2.0] and s.row("speed").data_ptr() == c.buf[0, 1:].data_ptr()
    n = pipeline.Controls.neutral(2, alpha=0.3, beta=0.7, t=0.7, device="cpu")
    assert n.present == n.NAMES and n.row("speed").tolist() == [1.0, 1.0] and n.row("n_shift").tolist() == [0.0, 0.0]
    assert n.row("alpha").tolist() == [np.float32(0.3)] * 2
    assert bool(torch.isnan(pipeline.Controls.neutral(2, device="cpu").row("beta")).all())
    with pytest.raises(ValueError):
        pipeline.Controls(0, device="cpu")


def test_refused_combinations_raise_a_clear_value_error():
    tokens = torch.zeros(2, 5, dtype=torch.long)
    c = pipeline.Controls(2, speed=1.25, device="cpu")
    with pytest.raises(ValueError, match="engine path"):
        pipeline.prepare(None, None, tokens, controls=c)  # a CPU batch: the controls are engine-only
    with pytest.raises(ValueError, match="front="):
        pipeline.prepare(None, None, tokens, controls=c, front=object())
    with _hooks.override(plan="python"):
        with pytest.raises(ValueError, match="python"):
            pipeline.prepare(None, None, tokens, controls=c)
    with pytest.raises(ValueError, match="Controls"):
        pipeline.prepare(None, None, tokens, controls={"speed": 1.0})
    with pytest.raises(ValueError):
        pipeline.inference(None, None, tokens, controls=c, taps={})
    with pytest.raises(ValueError, match="one row per sentence"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1], tokens[0]], controls=c)


def test_speed_with_forced_durations_raises(monkeypatch):
    """Checked behind the device checks, so the test stands in a HIP device for the batch's."""
    tokens = torch.zeros(2, 5, dtype=torch.long)
    dur = torch.full((2, 5), 3)
    c = pipeline.Controls(2, speed=1.25, device="cpu")
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(pipeline.Controls, "device", property(lambda self: dev))
    with pytest.raises(ValueError, match="nothing to scale"):
        pipeline._check_controls(c, dev, 2, None, None, dur)
    pipeline._check_controls(pipeline.Controls(2, f0_scale=1.5, device="cpu"), dev, 2, None, None, dur)  # pitch alone is fine
    with pytest.raises(ValueError, match="rows"):
        pipeline._check_controls(c, dev, 3, None, None, None)


def test_numpy_contract_tie_cases():
    f = lambda v: np.array([v], dtype=np.float32)
    dur = lambda total, speed, **kw: R.durations(f(total), None if speed is None else [speed], **kw)[0].tolist()
    assert dur([2.5, 3.5], 1.0) == [2, 4] and dur([2.5, 3.5], None) == [2, 4]  # round half to even
    assert dur([25.0], 2.0) == [12]  # 12.5 -> 12
    assert dur([0.4, 0.2], 1.0) == [1, 1] and dur([0.4], 4.0) == [1]  # never below one frame
    assert dur([1.25, 1.75], 1.0) == [1, 2]
    assert dur([3.0, 3.0, 3.0, 3.0], 1.0, lengths=[2], tail=5) == [3, 8, 0, 0]  # pad -> 0, tail on the row's last token
    assert dur([3.0, 3.0, 3.0], 0.5, lengths=[3], tail=5) == [6, 6, 11]  # the tail is not scaled
    # the device clamp: 0 -> 0.25, 100 -> 4, NaN -> 1
    assert dur([10.0], 0.0) == [40] and dur([10.0], 100.0) == [2] and dur([10.0], float("nan")) == [10]
    assert R.clamp("alpha", [1.5, -1.0, float("nan")], scalar=0.3).tolist() == [1.0, 0.0, np.float32(0.3)]
    assert R.clamp("n_shift", [float("nan"), 9.0]).tolist() == [0.0, 2.0]
    # a row weight equal to the scalar gives the scalar's pair when the scalar is an fp32 value
    w = float(np.float32(0.3))
    assert R._weight("alpha", np.array([w], np.float32), 0, 0.9) == R._weight("alpha", None, 0, w)
    # -0.0 survives a zero shift; a neutral scale keeps the bits
    F0, N = R.prosody(f([3.0, -0.0]), f([-0.0, 1.0]), [1.0], [0.0])
    assert np.signbit(N[0, 0]) and np.signbit(F0[0, 1]) and F0[0, 0] == 3.0
    F0, N = R.prosody(f([1.0, 2.0, 3.0, 4.0]), f([1.0, 2.0, 3.0, 4.0]), [2.0], [0.5], frames=[1])
    assert F0[0].tolist() == [2.0, 4.0, 3.0, 4.0] and N[0].tolist() == [1.5, 2.5, 3.0, 4.0]
