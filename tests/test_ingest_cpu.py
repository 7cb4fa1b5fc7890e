"""Reference clips at a client's rate and in G.711, the part that needs no GPU: the C ABI of
`st2_clip_ingest` (declared, exported, bound, additive under ABI 23, validated before any launch), the input filter tables
against the output side's design requirements, `resample.design` unchanged, the fp64 reference of tests/_ingest_ref.py against
hand-computed cases, what the Python surface refuses, and the margin condition of every clip tests/test_ingest_gpu.py trims."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest
import torch

import _ingest_ref as I
import _resample_ref as R
from styletts2_amd import _lib, ops, resample, style

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_clip_ingest", "st2_clip_ingest_work_bytes")
RATIOS = {8000: (3, 1), 16000: (3, 2), 22050: (160, 147), 24000: (1, 1), 32000: (3, 4), 44100: (80, 147), 48000: (1, 2)}
TAPS = {8000: 82, 16000: 82, 22050: 82, 24000: 1, 32000: 110, 44100: 152, 48000: 164}
# sha256 over (rate, U, D, shape, dtype, bytes) of resample.design(r) for every rate, taken before design_input existed
DESIGN_SHA256 = "8ab075918a03fc15bc244d91bfa8709b9c87882bf0ff8d23ae60e0dde43a3f2f"


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound_additively():
    lib = _lib.load()
    text = open(HEADER).read()
    assert re.search(r"\bint st2_clip_ingest\(", text) and re.search(r"\bint64_t st2_clip_ingest_work_bytes\(", text)
    for name in NEW:
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11
    assert not any("ingest" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)
    assert "enum st2_pcm_format { ST2_PCM_F32 = 0, ST2_PCM_S16 = 1, ST2_PCM_ULAW = 2, ST2_PCM_ALAW = 3 };" in text
    assert (_lib.STATUS_F16_RANGE, _lib.STATUS_LSTM_TIMEOUT, _lib.STATUS_DURATION_SUM, _lib.STATUS_LSTM_RECOVERED,
            _lib.STATUS_FRAME_CAPACITY) == (1, 2, 4, 8, 16) and "ST2_STATUS_" + "CLIP" not in text  # no new sticky bit


def test_work_bytes():
    lib = _lib.load()
    f = lib.st2_clip_ingest_work_bytes
    assert f(0, 100) == 0 and f(3, 0) == 0 and f(-1, -1) == 0
    for B, L in ((1, 1), (6, 9000), (32, 240000), (5, 1024), (5, 1025)):
        stride = (L + 1023) // 1024 * 1024
        need = B * (4 * stride + 4 * stride // 512 + 4)  # the 24 kHz rows, their 512-sample block sums, the cuts
        assert need <= f(B, L) < need + 16 and f(B, L) % 16 == 0


def test_clip_ingest_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(4096)
    f = lib.st2_clip_ingest
    order = ("src", "src_bs", "n", "B", "N_cap", "fmt", "up", "down", "taps", "K", "top_db", "L_min", "wave", "w_bs", "L_cap",
             "len", "start", "flags", "work", "work_bytes", "stream")
    ok = dict(src=d, src_bs=1000, n=d, B=2, N_cap=1000, fmt=_lib.PCM_ULAW, up=3, down=1, taps=d, K=82, top_db=30.0, L_min=0,
              wave=d, w_bs=3000, L_cap=3000, len=d, start=None, flags=None, work=d,
              work_bytes=lib.st2_clip_ingest_work_bytes(2, 3000), stream=None)
    cases = [
        (dict(src=None), "NULL"), (dict(n=None), "NULL"), (dict(taps=None), "NULL"), (dict(wave=None), "NULL"),
        (dict(len=None), "NULL"), (dict(work=None), "NULL"),
        (dict(B=0), "bad geometry"), (dict(B=65536), "bad geometry"), (dict(N_cap=0), "bad geometry"),
        (dict(L_cap=0), "bad geometry"), (dict(L_cap=-5), "bad geometry"),
        (dict(w_bs=2996), "w_bs"), (dict(w_bs=3002), "w_bs"), (dict(src_bs=999), "src_bs"),
        (dict(up=0), "ratio"), (dict(up=1025), "ratio"), (dict(down=0), "ratio"), (dict(down=1025), "ratio"),
        (dict(K=0), "taps_per_phase"), (dict(K=513), "taps_per_phase"),
        (dict(fmt=4), "unknown format"), (dict(fmt=-1), "unknown format"),
        (dict(L_min=-1), "L_min"), (dict(L_min=3001), "L_min"),
        (dict(work_bytes=lib.st2_clip_ingest_work_bytes(2, 3000) - 1), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
        (dict(fmt=_lib.PCM_S16, src=C.c_void_p(4097)), "aligned"), (dict(fmt=_lib.PCM_F32, src=C.c_void_p(4098)), "aligned"),
        (dict(wave=C.c_void_p(4104)), "aligned"), (dict(work=C.c_void_p(4100)), "aligned"),
        (dict(up=1000, K=512), "LDS"),  # a table no tile fits beside
    ]
    for change, word in cases:
        a = dict(ok, **change)
        assert f(*[a[k] for k in order]) != 0, change
        assert "st2_clip_ingest" in _err(lib) and word in _err(lib), (change, _err(lib))


# ---- filter tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(RATIOS))
def test_input_table_meets_the_output_side_requirements(rate):
    U, D, taps = resample.design_input(rate)
    K = taps.shape[1]
    assert (U, D) == RATIOS[rate] and math.gcd(U, D) == 1 and U * rate == D * 24000
    assert taps.dtype == np.float32 and taps.shape == (U, K) and K == TAPS[rate] == (resample.taps_per_phase(U, D) if U != D else 1)
    assert 4 * (U * K + 1024 * D // U + K + 8 + 1024 + 8) <= 63 * 1024, "table, a 1024-sample tile and its span fit the kernel's LDS"
    if rate == 24000:
        assert taps.tolist() == [[1.0]]
        return
    proto = resample.prototype(taps.astype(np.float64)) / U
    nfft = 1 << int(math.ceil(math.log2(len(proto) * 64)))
    H = np.abs(np.fft.rfft(proto, nfft))
    f = np.arange(len(H)) / nfft * U  # cycles per INPUT sample
    f_n = 0.5 * min(1.0, U / D)  # the lower of the two Nyquist frequencies
    dev = np.abs(20 * np.log10(H[f <= 0.85 * f_n])).max()
    att = -20 * np.log10(np.maximum(H[f >= f_n], 1e-300)).max()
    print("rate %d: U/D %d/%d, K %d, table %d B, passband deviation %.5f dB, stopband attenuation %.2f dB"
          % (rate, U, D, K, taps.nbytes, dev, att))
    assert dev <= 0.05, "passband deviation %.4f dB" % dev
    assert att >= 90.0, "stopband attenuation %.2f dB" % att


def test_output_tables_are_byte_identical_to_before():
    h = hashlib.sha256()
    for r in resample.RATES:
        U, D, t = resample.design(r)
        h.update(("%d %d %d %s %s;" % (r, U, D, t.shape, t.dtype)).encode())
        h.update(t.tobytes())
    assert h.hexdigest() == DESIGN_SHA256
    for rate in (0, 11025, 96000, None):
        with pytest.raises(ValueError):
            resample.design_input(rate)


# ---- G.711 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_expansion_all_256_codes(law):
    """The reference's expansion (the bit formula of G.191) is `_resample_ref`'s for every code, and encode(decode(c)) == c for
    every code but ONE: mu-law 0x7F, the negative zero, decodes to 0 and 0 encodes to 0xFF.  A-law has no such code: its
    negative zero 0x55 decodes to -8, which encodes to 0x55 again."""
    codes = np.arange(256)
    v = I.EXPAND[law](codes)
    assert np.array_equal(v, R.DECODE[law](codes))
    assert v.min() >= -32768 and v.max() <= 32767 and np.array_equal(I.decode(codes.astype(np.uint8), law), (v / 32768.0).astype(np.float32))
    assert np.array_equal(I.decode(codes.astype(np.uint8), law).astype(np.float64) * 32768.0, v.astype(np.float64)), "exact in fp32"
    again = R.ENCODE[law](v)
    excepted = {0x7F} if law == "ulaw" else set()
    assert set(codes[again != codes].tolist()) == excepted
    if law == "ulaw":
        assert v[0x7F] == 0 and again[0x7F] == 0xFF
    else:
        assert v[0x55] == -8 and v[0xD5] == 8


# ---- the trim reference -------------------------------------------------------------------------------------------------------
def test_trim_reference_on_hand_computed_clips():
    one = np.ones
    # 1. 5000 samples, ones on [2048, 3072): frames 0..9; frame f covers [512 f - 1024, 512 f + 1024) and meets the ones for
    #    f = 3 (512 of them) .. 7 ([2560, 4608): 512 of them); 2 and 8 meet none.  start = 1536, end = 4096.
    x = np.zeros(5000)
    x[2048:3072] = 1.0
    e = I.frame_energies(x)
    assert len(e) == 10 and e[[2, 8]].tolist() == [1e-10, 1e-10]
    assert e[3:8].tolist() == [0.25, 0.5, 0.5, 0.5, 0.25]
    assert I.trim_bounds(x, 30.0)[:2] == (1536, 4096)
    # 2. ones from 4000 to the end of a 5000-sample clip: frame 6 = [2048, 4096) holds 96 of them (e = 96 / 2048 = 0.047 >
    #    e_ref 1e-3), frame 5 none; last frame 9 -> end = min(5000, 5120) = 5000.
    x = np.zeros(5000)
    x[4000:] = 1.0
    assert I.trim_bounds(x, 30.0)[:2] == (3072, 5000)
    # 3. 1000 samples of 0.5 (shorter than a frame): frames 0, 1; both hold the clip -> the whole of it.  At 20 dB the same.
    assert I.trim_bounds(0.5 * one(1000), 30.0)[:2] == (0, 1000) and I.trim_bounds(0.5 * one(1000), 20.0)[:2] == (0, 1000)
    # a loud block and one 25 dB below it: kept at top_db 30, dropped at top_db 20
    x = np.zeros(8192)
    x[:2048], x[6144:] = 1.0, 10.0 ** (-25 / 20)
    assert I.trim_bounds(x, 30.0)[:2] == (0, 8192) and I.trim_bounds(x, 20.0)[:2] == (0, 3072)
    # all zero: every frame sits on the floor 1e-10 = e_ref, above e_ref / 1000 -> the whole clip, as librosa gives
    assert I.trim_bounds(np.zeros(3000), 30.0)[:2] == (0, 3000) and I.trim_bounds(np.zeros(0), 30.0)[:2] == (0, 0)
    assert I.trim_bounds(x, 0.0)[:2] == (0, 8192)
    # the minimum-length rule
    assert I.min_length(1536, 4096, 5000, 2000) == (1536, 4096, False)
    assert I.min_length(1536, 4096, 5000, 3000) == (1536, 4536, True)
    assert I.min_length(3072, 5000, 5000, 3000) == (2000, 5000, True)
    assert I.min_length(0, 1000, 1000, 3000) == (0, 1000, True)


def test_reference_row_end_to_end_on_a_tiny_case():
    """U / D = 1 / 1: the decode alone; capacity and flags."""
    taps = np.ones((1, 1), dtype=np.float32)
    raw = np.array([0, 16384, -32768, 32767, 5], dtype=np.int16)
    row = I.ingest_row(raw, 4, "s16", taps, 1, 1, 0.0, 0, 10)
    assert row["wave"].tolist() == [0.0, 0.5, -1.0, 32767 / 32768] and row["len"] == 4 and row["flags"] == 0
    row = I.ingest_row(raw, 9, "s16", taps, 1, 1, 0.0, 4, 3)
    assert row["len"] == 3 and row["start"] == 0 and row["flags"] == 3  # cut to capacity, and still below L_min


# ---- the GPU test's clips -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt", I.TRIM_RATES)
def test_every_trimmed_clip_keeps_3_db_from_the_threshold(rate, fmt):
    """What makes `start` / `len` exact on the device: in the fp64 reference every frame's energy is at least 2 x above or
    2 x below the threshold, orders beyond the ~1e-4 relative error of a 2048-term fp32 mean square plus the resampler's."""
    for kind, L_min in (("trim", 0), ("short", I.L_MIN)):
        names, rows, L_cap = I.reference(kind, rate, fmt, L_min)
        for name, row in zip(names, rows):
            print("%s %d %s: m %d start %d len %d flags %d margin %.3g" % (name, rate, fmt, row["m"], row["start"], row["len"],
                                                                          row["flags"], row["margin"]))
            assert row["margin"] >= 2.0, (name, row["margin"])
    names, rows, L_cap = I.reference("trim", rate, fmt, 0)
    by = dict(zip(names, rows))
    r = by["burst at the very start"]
    assert r["start"] == 0 and 2816 < r["len"] < r["m"]
    r = by["burst at the very end"]
    assert r["start"] > 0 and r["start"] + r["len"] == r["m"] and r["m"] % 512 != 0
    r = by["two bursts, silence between"]
    assert 0 < r["start"] < 1792 and 7424 < r["start"] + r["len"] < r["m"], "the silence inside is kept"
    r = by["all zero"]
    assert r["start"] == 0 and r["len"] == r["m"] > 0
    r = by["shorter than one frame"]
    assert r["m"] < 2048 and r["start"] == 0 and r["len"] == r["m"]
    assert all(r["flags"] == 0 for r in rows)
    names, rows, L_cap = I.reference("short", rate, fmt, I.L_MIN)
    mid, first, last, tiny = rows
    assert all(r["flags"] == 2 for r in rows) and [r["len"] for r in rows[:3]] == [I.L_MIN] * 3
    assert mid["start"] > 0 and mid["start"] + mid["len"] < mid["m"]
    assert first["start"] == 0 and last["start"] + last["len"] == last["m"] and last["start"] == last["m"] - I.L_MIN
    assert tiny["start"] == 0 and tiny["len"] == tiny["m"] < I.L_MIN


# ---- wrappers -----------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_bad_combinations():
    u8 = torch.zeros(2, 8000, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sample_rate"):
        style.compute_style(None, u8, sample_rate=11025, encoding="ulaw")
    with pytest.raises(ValueError, match="encoding"):
        style.compute_style(None, u8, sample_rate=8000, encoding="u8")
    with pytest.raises(_lib.St2Error, match="encoding"):
        style.compute_style(None, u8, sample_rate=8000, encoding="s16")  # uint8 bytes are not 16-bit samples
    with pytest.raises(_lib.St2Error, match="encoding"):
        style.ingest_clips([torch.zeros(8000), torch.zeros(8000, dtype=torch.int16)], sample_rate=8000, encoding="f32")
    with pytest.raises(_lib.St2Error, match="23700"):
        style.compute_style(None, u8, lengths=[8000, 7899], sample_rate=8000, encoding="ulaw")  # 3 x 7899 = 23 697 < MIN_CLIP
    with pytest.raises(_lib.St2Error, match="23700"):
        style.ingest_clips([torch.zeros(8000, dtype=torch.uint8), torch.zeros(100, dtype=torch.uint8)], sample_rate=8000,
                           encoding="alaw")
    with pytest.raises(_lib.St2Error):
        style.ingest_clips(u8, lengths=[8000, 8001], sample_rate=8000, encoding="ulaw")  # past the buffer's row
    with pytest.raises(_lib.St2Error):
        style.ingest_clips(u8, lengths=[8000], sample_rate=8000, encoding="ulaw")
    with pytest.raises(_lib.St2Error, match="HIP device"):
        style.ingest_clips(u8, lengths=[8000, 7900], sample_rate=8000, encoding="ulaw")  # valid, but there is no CPU path
    with pytest.raises(_lib.St2Error, match="carries its own lengths"):
        style.ingest_clips([u8[0]], lengths=[8000], sample_rate=8000, encoding="ulaw")
    n = torch.tensor([8000, 8000], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.clip_ingest(u8, n, 11025, "ulaw")
    with pytest.raises(ValueError):
        ops.clip_ingest(u8, n, 8000, "u8")
    with pytest.raises(_lib.St2Error):
        ops.clip_ingest(u8, n, 8000, "ulaw")  # CPU tensors
    assert style.MIN_CLIP == 23700 and resample.output_samples(7900, 3, 1) == 23700
