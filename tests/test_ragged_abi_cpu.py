"""C ABI of the length-aware (ragged) decoder and prosody entry points (ABI v23): declared, exported, callable from plain C,
argument validation before any launch, and the two backend-table sizes st2_debug_set_backend accepts.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from styletts2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
LIBDIR = os.path.join(ROOT, "styletts2_amd")
NEW = ("st2_decoder_forward_ragged", "st2_prosody_forward_ragged")


def test_abi_version_23():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23
    assert "#define ST2_ABI_VERSION 23" in open(HEADER).read()
    assert lib.st2_sizeof_conv_desc() == C.sizeof(_lib.ConvDesc)


def test_ragged_symbols_exported_and_declared():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW + ("st2_ragged_lengths",):
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in st2.h" % name


def test_plain_c_translation_unit_calls_the_ragged_entry_points(tmp_path):
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers are not installed")
    src = tmp_path / "ragged.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "st2.h"
int main(void) {
  int rc = st2_decoder_forward_ragged(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 2, 10, NULL, NULL, 0, NULL, NULL);
  const char* m = st2_last_error();
  if (rc == 0 || !m || !strstr(m, "frames")) return 1;
  rc = st2_prosody_forward_ragged(NULL, NULL, NULL, NULL, NULL, NULL, 2, 4, 10, 0, NULL, NULL, NULL, NULL, 0, NULL);
  m = st2_last_error();
  if (rc == 0 || !m || !strstr(m, "frames")) return 2;
  printf("ok %d\n", ST2_ABI_VERSION);
  return 0;
}
''')
    exe = str(tmp_path / "ragged")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + LIBDIR, "-lst2_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 23", (r.returncode, r.stdout, r.stderr)


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_argument_validation_before_any_launch():
    lib = _lib.load()
    frames = (C.c_int32 * 2)(3, 4)
    fp = C.cast(frames, C.c_void_p)
    dummy = C.c_void_p(256)
    # frames NULL
    assert lib.st2_decoder_forward_ragged(dummy, dummy, dummy, dummy, dummy, dummy, None, None, 2, 4, dummy, dummy,
                                          1 << 20, None, None) != 0
    assert "frames" in _err(lib)
    assert lib.st2_prosody_forward_ragged(dummy, dummy, dummy, dummy, dummy, None, 2, 3, 4, 0, dummy, dummy, dummy,
                                          dummy, 1 << 20, None) != 0
    assert "frames" in _err(lib)
    # B <= 0, T_max <= 0
    for B, T in ((0, 4), (-1, 4), (2, 0), (2, -3)):
        assert lib.st2_decoder_forward_ragged(dummy, dummy, dummy, dummy, dummy, dummy, None, fp, B, T, dummy, dummy,
                                              1 << 20, None, None) != 0
        assert "bad geometry" in _err(lib)
        assert lib.st2_prosody_forward_ragged(dummy, dummy, dummy, dummy, dummy, fp, B, 3, T, 0, dummy, dummy, dummy,
                                              dummy, 1 << 20, None) != 0
        assert "bad geometry" in _err(lib)


def test_debug_set_backend_accepts_both_slot_counts():
    lib = _lib.load()
    buf = C.create_string_buffer(8)
    ptr = C.cast(buf, C.c_void_p).value
    old, full = len(_lib.BACKEND_SLOTS), len(_lib.BACKEND_SLOTS) + len(_lib.BACKEND_SLOTS_RAGGED)
    try:
        for n in (old, full):
            table = (C.c_void_p * n)(*([ptr] * n))  # never called: only the table's shape is checked here
            assert lib.st2_debug_set_backend(table, n) == 0, _err(lib)
        table = (C.c_void_p * (full + 1))(*([ptr] * (full + 1)))
        assert lib.st2_debug_set_backend(table, full + 1) != 0
        assert "entries" in _err(lib)
    finally:
        assert lib.st2_debug_set_backend(None, 0) == 0
