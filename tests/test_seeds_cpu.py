"""C ABI and host-side contract of the per-request seeds: the numpy contract of tests/_rng_ref.py gives
Random123's known answers for Philox4x32-10 and, under the committed seeds, meets the statistical bounds the GPU test holds the
kernel to; `st2_noise_fill` is declared, exported and bound under ABI 23 without a backend slot and refuses bad arguments before
any launch; `pipeline` takes `seeds` on its three entry points and refuses what does not go with them.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _rng_ref as R
from styletts2_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
LIBDIR = os.path.join(ROOT, "styletts2_amd")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def test_contract_gives_the_published_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
        assert [int(v[0]) for v in got] == list(want), (counter, key, [hex(int(v[0])) for v in got])
    # and through the element rule: counter (i div 4, 0, s, 0), key (lo32, hi32) of the seed read as uint64
    assert R.bits(0, 0, 4).tolist() == list(R.KNOWN_ANSWERS[0][2])
    k = (0x299f31d0 << 32) | 0xa4093822
    one = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in (5, 0, 7, 0)], (0xa4093822, 0x299f31d0))
    assert R.bits(k, 7, 24)[20:24].tolist() == [int(v[0]) for v in one]
    assert R.bits(-1, 3, 8).tolist() == R.bits((1 << 64) - 1, 3, 8).tolist()  # int64 -1 is uint64 2^64 - 1
    assert R.bits(9, 3, 7).tolist() == R.bits(9, 3, 1027)[:7].tolist()  # a prefix is a prefix: n does not enter
    with pytest.raises(ValueError):
        R.bits(0, 0, 1 << 34)


def test_contract_normals_are_the_stated_box_muller_pairs():
    w = np.array([0x00000000, 0x00000000, 0xFFFFFFFF, 0x40000000], dtype=np.uint32)
    z = R.normals_from_bits(w)
    r_max = np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -24))
    assert abs(z[0] - r_max) < 1e-12 and abs(z[1]) < 1e-12 and r_max < 5.9  # the largest |z| there is
    r_min = np.sqrt(-2.0 * np.log(1.0 - 2.0 ** -25))  # u1 next to 1: not 0
    assert 2.4e-4 < r_min < 2.5e-4 and abs(z[2]) < 1e-15 and abs(z[3] - r_min) < 1e-15  # the angle is pi / 2
    assert R.normals(5, 1, 6).tolist() == R.normals(5, 1, 8)[:6].tolist()


@pytest.fixture(scope="module")
def stat_draws():
    return {(k, s): R.normals(k, s, R.STAT_N) for k in R.STAT_SEEDS for s in (R.SAMPLER, R.STEP, R.SINE)}


def test_contract_meets_the_statistical_bounds_under_the_committed_seeds(stat_draws):
    for k in R.STAT_SEEDS:
        for s in (R.SAMPLER, R.STEP, R.SINE):
            st = R.stats(stat_draws[k, s], stat_draws[k, R.STEP] if s == R.SAMPLER else None)  # streams 0 and 1 of one seed
            print("seed %d stream %#x: %s" % (k, s, st))
            R.check_stats(st, (k, s))
        st = R.stats(stat_draws[k, R.SAMPLER], R.normals(k + 1, R.SAMPLER, R.STAT_N))  # seeds k and k + 1
        R.check_stats(st, (k, "k+1"))
        assert np.abs(stat_draws[k, R.SAMPLER]).max() <= 5.9


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    assert re.search(r"\bint st2_noise_fill\(", text)
    assert hasattr(lib, "st2_noise_fill") and "st2_noise_fill" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert not any("noise" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)
    for name, value in (("SAMPLER", 0), ("STEP", 1), ("SINE", 0x10000)):
        m = re.search(r"#define ST2_NOISE_%s (\w+)" % name, text)
        assert m and int(m.group(1).rstrip("u"), 0) == value == getattr(_lib, "NOISE_" + name) == getattr(R, name) == getattr(
            ops, "NOISE_" + name)
    assert "ST2_NOISE_NORMAL = 0, ST2_NOISE_BITS = 1" in text and (_lib.NOISE_NORMAL, _lib.NOISE_BITS) == (0, 1)


def test_plain_c_translation_unit_calls_the_noise_entry_point(tmp_path):
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers are not installed")
    src = tmp_path / "noise.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "st2.h"
int main(void) {
  const char* m;
  if (st2_noise_fill(NULL, 2, ST2_NOISE_SINE, 1, ST2_NOISE_NORMAL, NULL, 0, 5400, 5400, NULL, 0, NULL) == 0) return 1;
  m = st2_last_error();
  if (!m || !strstr(m, "st2_noise_fill") || !strstr(m, "NULL")) return 2;
  if (ST2_NOISE_SAMPLER != 0 || ST2_NOISE_STEP != 1 || ST2_NOISE_SINE != 65536 || ST2_NOISE_BITS != 1) return 3;
  printf("ok %d\n", ST2_ABI_VERSION);
  return 0;
}
''')
    exe = str(tmp_path / "noise")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + LIBDIR, "-lst2_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 23", (r.returncode, r.stdout, r.stderr)


D = C.c_void_p(256)
ORDER = ("seeds", "B", "stream0", "S", "kind", "out", "s_stride", "b_stride", "n", "counts", "per_count")


def test_noise_fill_validates_before_any_launch():
    lib = _lib.load()
    base = dict(seeds=D, B=3, stream0=1, S=4, kind=_lib.NOISE_NORMAL, out=D, s_stride=3 * 256, b_stride=256, n=256, counts=None,
                per_count=0)
    for change, word in ((dict(seeds=None), "NULL"), (dict(out=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=-1), "bad geometry"),
                         (dict(S=0), "bad geometry"), (dict(S=-2), "bad geometry"), (dict(B=65536), "bad geometry"),
                         (dict(n=-1), "negative"), (dict(n=1 << 34, b_stride=1 << 34, s_stride=1 << 36), "2^34"),
                         (dict(kind=2), "unknown kind"), (dict(kind=-1), "unknown kind"), (dict(b_stride=255), "b_stride"),
                         (dict(b_stride=-256), "b_stride"), (dict(s_stride=3 * 256 - 1), "s_stride"), (dict(s_stride=0), "s_stride"),
                         (dict(counts=D, per_count=0), "per_count"), (dict(counts=D, per_count=-5), "per_count"),
                         (dict(stream0=0xFFFFFFFD), "2^32"), (dict(seeds=C.c_void_p(260)), "aligned"),
                         (dict(out=C.c_void_p(258)), "aligned"), (dict(counts=C.c_void_p(258), per_count=1), "aligned")):
        a = dict(base, **change)
        assert lib.st2_noise_fill(*[a[k] for k in ORDER], None) != 0, change
        assert "st2_noise_fill:" in _err(lib) and word in _err(lib), (change, _err(lib))
    # n = 0 is a successful no-op -- after the checks: nothing is launched, so the made-up pointers are never read
    assert lib.st2_noise_fill(*[dict(base, n=0)[k] for k in ORDER], None) == 0
    assert lib.st2_noise_fill(*[dict(base, n=0, kind=5)[k] for k in ORDER], None) != 0
    # one row / one stream: the stride it does not use is not looked at
    assert lib.st2_noise_fill(*[dict(base, n=0, B=1, b_stride=0, s_stride=0, S=1)[k] for k in ORDER], None) == 0


def test_wrapper_has_no_cpu_path_and_checks_its_operands():
    seeds, out = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 8)
    with pytest.raises(_lib.St2Error):
        ops.noise_fill(seeds, out, 0)
    with pytest.raises(_lib.St2Error):
        ops.noise_fill([1, 2, 3], out, 0)
    with pytest.raises(_lib.St2Error):
        ops.noise_fill(seeds.to(torch.int32), out, 0)


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------
def test_signature_additions_and_refusals():
    sig = lambda f: inspect.signature(f).parameters
    for f in (pipeline.inference, pipeline.GraphedSynthesis.__init__, pipeline.GraphedSynthesis.__call__, pipeline.synthesize_long):
        assert "seeds" in sig(f), f
    assert sig(pipeline.inference)["seeds"].default is None and sig(pipeline.synthesize_long)["seeds"].default is None
    assert sig(pipeline.GraphedSynthesis.__init__)["seeds"].default is False
    assert sig(pipeline.GraphedSynthesis.__call__)["seeds"].default is None
    assert "seeds" not in sig(pipeline._hand_over) and "seeds" not in sig(pipeline._output_spec)  # an input, not an output option
    assert list(sig(ops.noise_fill))[:6] == ["seeds", "out", "stream0", "counts", "per_count", "bits"]
    tokens = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="capacity-bound path: pass max_frames"):
        pipeline.inference(None, None, tokens, seeds=[1, 2])
    for explicit in ("noise", "step_noise", "sine_noise"):
        with pytest.raises(ValueError, match="one or the other"):
            pipeline.inference(None, None, tokens, max_frames=10, seeds=[1, 2], **{explicit: torch.zeros(2, 1, 256)})
    for bad in ([1, 2, 3], [1], torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), [1.5, 2], [1, 2 ** 63],
                torch.zeros(2, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="seeds must be"):
            pipeline.inference(None, None, tokens, max_frames=10, seeds=bad)
    with pytest.raises(ValueError, match="capacity-bound path: pass max_frames"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], seeds=7)
    with pytest.raises(ValueError, match="one or the other"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], max_frames=10, seeds=7, noises=[torch.zeros(1, 1, 256)] * 2)
    with pytest.raises(ValueError, match="seeds must be"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], max_frames=10, seeds=[7])


def test_one_seed_expands_to_consecutive_seeds_and_wraps_in_int64():
    assert pipeline.seed_rows(7, 3) == [7, 8, 9] and pipeline.seed_rows(-1, 3) == [-1, 0, 1]
    assert pipeline.seed_rows(2 ** 63 - 2, 4) == [2 ** 63 - 2, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 1]
    assert pipeline.seed_rows([5, -2 ** 63, 2 ** 63 - 1], 3) == [5, -2 ** 63, 2 ** 63 - 1]
    assert pipeline.seed_rows(torch.tensor([3, 4]), 2) == [3, 4]
    t = torch.tensor(pipeline.seed_rows(2 ** 63 - 1, 2), dtype=torch.int64)
    assert t.tolist() == [2 ** 63 - 1, -2 ** 63]
    # consecutive int64 seeds, read as uint64, are consecutive keys: the wrap is the generator's own
    assert R.bits(-2 ** 63, 0, 4).tolist() == R.bits(2 ** 63, 0, 4).tolist()
