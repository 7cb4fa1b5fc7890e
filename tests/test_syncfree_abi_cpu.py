"""C ABI and host-side contract of the sync-free path: `st2_frames_from_durations` and `st2_wave_pack`
are declared, exported and bound, added under ABI 23 without a version bump; their arguments are validated before any launch;
`pipeline.prepare(max_frames=)` refuses what it cannot serve.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _syncfree_ref as R
from styletts2_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_frames_from_durations", "st2_wave_pack")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_syncfree_symbols_declared_exported_and_bound():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in st2.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in _lib.EXPORTS
    m = re.search(r"#define ST2_STATUS_FRAME_CAPACITY (\d+)", text)
    assert m and int(m.group(1)) == _lib.STATUS_FRAME_CAPACITY == 16  # the next free bit after LSTM_RECOVERED = 8
    taken = (_lib.STATUS_F16_RANGE, _lib.STATUS_LSTM_TIMEOUT, _lib.STATUS_DURATION_SUM, _lib.STATUS_LSTM_RECOVERED)
    assert all(_lib.STATUS_FRAME_CAPACITY & b == 0 for b in taken)
    assert re.search(r"ST2_PACK_F32 = 0, ST2_PACK_S16 = 1", text) and (_lib.PACK_F32, _lib.PACK_S16) == (0, 1)
    assert "added under ABI 23, additive" in text


def test_abi_is_still_23_and_no_backend_slot_was_added():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23
    assert "#define ST2_ABI_VERSION 23" in open(HEADER).read()
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11
    assert not any("frames_from" in s or "wave_pack" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED)


def test_frames_from_durations_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    f = lib.st2_frames_from_durations
    for args, word in (((None, 2, 4, None, 10, d, None), "NULL"), ((d, 2, 4, None, 10, None, None), "NULL"),
                       ((d, 0, 4, None, 10, d, None), "bad geometry"), ((d, -1, 4, None, 10, d, None), "bad geometry"),
                       ((d, 2, 0, None, 10, d, None), "bad geometry"), ((d, 2, 4, None, 0, d, None), "bad geometry"),
                       ((d, 2, 4, None, -5, d, None), "bad geometry"), ((d, 2, 513, None, 10, d, None), "512")):
        assert f(*args) != 0, args
        assert "st2_frames_from_durations" in _err(lib) and word in _err(lib), (args, _err(lib))


def test_wave_pack_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    f = lib.st2_wave_pack
    ok = dict(wave=d, w_bs=6000, frames=d, B=2, T_cap=10, spf=600, trim=0, fmt=_lib.PACK_S16, out=d, cap=12000, offsets=d)
    order = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "fmt", "out", "cap", "offsets")
    for change, word in ((dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(out=None), "NULL"),
                         (dict(offsets=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
                         (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"),
                         (dict(cap=-1), "negative"), (dict(fmt=2), "unknown format"), (dict(w_bs=5999), "w_bs"),
                         (dict(out=C.c_void_p(257)), "aligned")):
        a = dict(ok, **change)
        assert f(*[a[k] for k in order], None) != 0, change
        assert "st2_wave_pack" in _err(lib) and word in _err(lib), (change, _err(lib))


def test_wrappers_have_no_cpu_path():
    with pytest.raises(_lib.St2Error):
        ops.frames_from_durations(torch.ones(2, 4, dtype=torch.long), None, 10)
    with pytest.raises(_lib.St2Error):
        ops.wave_pack(torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.wave_pack(torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32), fmt="u8")


def test_prepare_max_frames_refuses_taps_and_host_tensors():
    tokens = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises((ValueError, _lib.St2Error)):
        pipeline.prepare(None, None, tokens, max_frames=64)  # a CPU tensor: the capacity-bound path is engine-only
    with pytest.raises((ValueError, _lib.St2Error)):
        pipeline.prepare(None, None, tokens, max_frames=64, taps={})
    with pytest.raises((ValueError, _lib.St2Error)):
        pipeline.prepare(None, None, tokens, max_frames=0)
    with pytest.raises(ValueError):
        pipeline.inference(None, None, tokens, pack="s16")  # packing belongs to the capacity-bound path


def test_reference_contract_of_the_pcm_conversion():
    """The numpy contract the GPU test compares against, pinned on the cases that matter: clamp, ties to even, NaN -> 0."""
    x = np.array([0.0, 1.0, -1.0, 2.5, -7.0, np.nan, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, np.inf, -np.inf],
                 dtype=np.float32)
    got = R.pcm16(x)
    want = np.rint(np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0), -1, 1).astype(np.float32) * np.float32(32767))
    assert got.dtype == np.int16 and got.tolist() == want.astype(np.int16).tolist()
    assert got[:6].tolist() == [0, 32767, -32767, 32767, -32767, 0]
    packed, offs = R.wave_pack(np.ones((3, 1800), np.float32), [1, 3, 9], T_cap=3, samples_per_frame=600, trim=700, fmt="f32")
    assert offs.tolist() == [0, 0, 1100, 2200] and packed.shape == (2200,)
    fr, over = R.frames_from_durations(torch.tensor([[3, 4, 5], [0, 0, 0], [9, 9, 9]]), torch.tensor([2, 3, 3]), 20)
    assert fr.tolist() == [7, 1, 20] and over.tolist() == [False, False, True]
