"""The three packing entries share one plan (csrc/st2_passage.hip `pack_plan`); each still refuses in its own name and words.
The expected messages were recorded from the build before the entries were merged.  No GPU needed: every call is refused
before any launch."""
import ctypes as C

import pytest

from styletts2_amd import _lib

D = C.c_void_p(256)
ORDER = {"st2_wave_pack": ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "fmt", "out", "cap", "offsets"),
         "st2_wave_resample_pack": ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "up", "down", "taps", "K", "fmt", "out",
                                    "cap", "offsets"),
         "st2_wave_pack_gaps": ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "up", "down", "taps", "K", "fmt", "gaps",
                                "gap_cap", "out", "cap", "offsets")}
PLAIN = dict(wave=D, w_bs=6000, frames=D, B=2, T_cap=10, spf=600, trim=0, up=1, down=1, taps=None, K=0, fmt=_lib.PCM_S16, gaps=D,
             gap_cap=100, out=D, cap=12200, offsets=D)
RESAMPLE = dict(PLAIN, up=1, down=3, taps=D, K=16, fmt=_lib.PCM_ULAW)
NULL = {False: "%s: wave / frames / out / offsets is NULL", True: "%s: wave / frames / taps / out / offsets is NULL"}
CASES = [  # entry, its arguments, a format outside its set, the words it refuses that format with
    ("st2_wave_pack", PLAIN, 2, "%s: unknown format 2"),
    ("st2_wave_resample_pack", RESAMPLE, 4, "%s: unknown format 4"),
    ("st2_wave_pack_gaps", PLAIN, 2, "%s: format 2 needs the resampling move (taps); without taps fp32 and 16-bit PCM only"),
    ("st2_wave_pack_gaps", RESAMPLE, 4, "%s: unknown format 4"),
]


@pytest.mark.parametrize("entry,base,bad_fmt,fmt_words", CASES)
def test_every_entry_refuses_in_its_own_name(entry, base, bad_fmt, fmt_words):
    lib = _lib.load()
    for change, words in ((dict(out=None), NULL[base["taps"] is not None]),
                          (dict(B=0), "%s: bad geometry (B=0, T_cap=10, samples_per_frame=600)"),
                          (dict(trim=-1), "%s: trim=-1 / out_capacity=12200 must not be negative"),
                          (dict(fmt=bad_fmt), fmt_words)):
        a = dict(base, **change)
        assert getattr(lib, entry)(*[a[k] for k in ORDER[entry]], None) != 0, (entry, change)
        assert lib.st2_last_error().decode() == words % entry, (entry, change)


def test_the_resampling_entry_does_not_become_the_plain_move_without_taps():
    lib = _lib.load()
    a = dict(RESAMPLE, taps=None)
    assert lib.st2_wave_resample_pack(*[a[k] for k in ORDER["st2_wave_resample_pack"]], None) != 0
    assert lib.st2_last_error().decode() == NULL[True] % "st2_wave_resample_pack"
