"""Output sample rates and G.711 in the packed hand-over, the part that needs no GPU: the filter tables
of `styletts2_amd/resample.py` against their design requirements, the G.711 reference of tests/_resample_ref.py against the
standard, the C ABI of `st2_wave_resample_pack` (declared, exported, bound, additive under ABI 23, validated before any launch)
and what the Python surface refuses."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _resample_ref as R
from styletts2_amd import _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NAME = "st2_wave_resample_pack"
STATIC_LDS = 64 * 1024  # what a gfx950 kernel may declare statically
RATIOS = {8000: (1, 3), 16000: (2, 3), 22050: (147, 160), 24000: (1, 1), 32000: (4, 3), 44100: (147, 80), 48000: (2, 1)}


# ---- filter tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(RATIOS))
def test_table_shape_and_frequency_response(rate):
    U, D, taps = resample.design(rate)
    K = taps.shape[1]
    assert (U, D) == RATIOS[rate] and math.gcd(U, D) == 1 and U * 24000 == D * rate
    assert taps.dtype == np.float32 and taps.shape == (U, K)
    assert taps.nbytes < STATIC_LDS, "the table alone must fit static LDS"
    if rate == 24000:
        assert K == 1 and taps.tolist() == [[1.0]]
        return
    assert K % 2 == 0 and K <= 512
    # the tap definition, spot-checked against the formula in fp64
    r, beta, h = 0.925 * min(1.0, U / D), 0.1102 * (96 - 8.7), (K - 1) // 2
    for p, k in ((0, h), (U - 1, 0), (U // 2, K - 1)):
        t = k - h - p / U
        want = r * np.sinc(r * t) * np.i0(beta * math.sqrt(max(0.0, 1 - (2 * t / K) ** 2))) / np.i0(beta)
        assert abs(float(taps[p, k]) - want) <= 2.0 ** -24 * max(abs(want), 1e-30) * 1.01 + 1e-45, (p, k)
    # the response of the flattened prototype (sampled at U times the input rate; DC gain U), by a zero-padded FFT
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


def test_unsupported_rates_raise():
    for rate in (0, 11025, 12000, 24001, 96000, -8000, None, "8000"):
        with pytest.raises(ValueError):
            resample.design(rate)
    with pytest.raises(ValueError):
        resample.design(8000, model_rate=22050)
    assert resample.output_samples(550, 1, 3) == 184 and resample.output_samples(0, 147, 160) == 0


# ---- G.711 reference -----------------------------------------------------------------------------------------------------------
ALL16 = np.arange(-32768, 32768, dtype=np.int64)


def test_g711_anchors():
    """The issue's anchors; the standard's reference code (ITU-T G.191) gives every one of them, so none had to yield."""
    v = np.array([0, 32767, -32768, -1])
    assert R.ulaw_encode(v).tolist() == [0xFF, 0x80, 0x00, 0x7F]
    assert R.alaw_encode(v[:3]).tolist() == [0xD5, 0xAA, 0x2A]
    assert int(R.alaw_encode(np.array([-1]))[0]) == 0x55  # the one's-complement magnitude of -1 is 0: A-law's negative zero


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_round_trip_is_monotone_and_within_half_a_step(law):
    """All 65 536 inputs.  mu-law clips: its largest code is centred on 32124 and reaches to +-32635, beyond which the standard
    itself overloads -- there the code must be the extreme one and the error is what clipping leaves."""
    code = R.ENCODE[law](ALL16)
    assert code.dtype == np.uint8
    back = R.DECODE[law](code)
    assert (np.diff(back) >= 0).all(), "decoding is monotone in the input"
    assert (np.diff(R.rank(code, law)) >= 0).all() and len(np.unique(code)) == 256
    err = np.abs(back - ALL16)
    inside = np.abs(ALL16 + (ALL16 < 0)) <= (32635 if law == "ulaw" else 32767)  # one's-complement magnitude
    assert (err[inside] <= R.half_step(code, law)[inside]).all(), int((err - R.half_step(code, law))[inside].max())
    if law == "ulaw":
        assert set(code[~inside & (ALL16 > 0)].tolist()) == {0x80} and set(code[~inside & (ALL16 < 0)].tolist()) == {0x00}
        assert err[~inside].max() <= 32768 - 32124
    again = R.ENCODE[law](back)  # a decoded value encodes to its own code, except mu-law's negative zero (it decodes to 0)
    assert ((again == code) | ((code == 0x7F) & (again == 0xFF) & (law == "ulaw"))).all()


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_symbol_declared_exported_and_bound_additively():
    lib = _lib.load()
    text = open(HEADER).read()
    assert re.search(r"\bint %s\(" % NAME, text), "%s is not declared in st2.h" % NAME
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    assert "enum st2_pcm_format { ST2_PCM_F32 = 0, ST2_PCM_S16 = 1, ST2_PCM_ULAW = 2, ST2_PCM_ALAW = 3 };" in text
    assert (_lib.PCM_F32, _lib.PCM_S16, _lib.PCM_ULAW, _lib.PCM_ALAW) == (0, 1, 2, 3)
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11
    assert not any("resample" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)
    # st2_wave_pack is untouched: its enum line and its two formats
    assert "enum st2_pack_format { ST2_PACK_F32 = 0, ST2_PACK_S16 = 1 };" in text
    assert set(ops.PACK_FORMATS) == {"f32", "s16"}
    assert {k: v[1] for k, v in ops.OUTPUT_FORMATS.items()} == {"f32": torch.float32, "s16": torch.int16,
                                                                "ulaw": torch.uint8, "alaw": torch.uint8}


def test_resample_pack_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    f = lib.st2_wave_resample_pack
    ok = dict(wave=d, w_bs=6000, frames=d, B=2, T_cap=10, spf=600, trim=0, up=1, down=3, taps=d, K=246, fmt=_lib.PCM_S16,
              out=d, cap=4000, offsets=d)
    order = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "up", "down", "taps", "K", "fmt", "out", "cap", "offsets")
    cases = [  # every st2_wave_pack condition ...
        (dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(out=None), "NULL"), (dict(offsets=None), "NULL"),
        (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"), (dict(T_cap=0), "bad geometry"),
        (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"), (dict(cap=-1), "negative"), (dict(w_bs=5999), "w_bs"),
        (dict(out=C.c_void_p(257)), "aligned"), (dict(fmt=_lib.PCM_F32, out=C.c_void_p(258)), "aligned"),
        # ... and the entry's own
        (dict(taps=None), "NULL"), (dict(up=0), "ratio"), (dict(up=1025), "ratio"), (dict(down=0), "ratio"),
        (dict(down=1025), "ratio"), (dict(K=0), "taps_per_phase"), (dict(K=513), "taps_per_phase"),
        (dict(fmt=4), "unknown format"), (dict(fmt=-1), "unknown format"),
        (dict(up=1000, K=512), "LDS"),  # a table no tile fits beside
    ]
    for change, word in cases:
        a = dict(ok, **change)
        assert f(*[a[k] for k in order], None) != 0, change
        assert NAME in _err(lib) and word in _err(lib), (change, _err(lib))
    # the format code st2_wave_pack refuses stays refused there
    assert lib.st2_wave_pack(d, 6000, d, 2, 10, 600, 0, 2, d, 12000, d, None) != 0 and "unknown format" in _err(lib)


# ---- wrappers --------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_they_cannot_serve():
    wave, frames = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_resample_pack(wave, frames, 8000, fmt="ulaw")  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        ops.wave_resample_pack(wave, frames, 8000, fmt="u8")
    with pytest.raises(ValueError):
        ops.wave_resample_pack(wave, frames, 11025)
    tokens = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="sample_rate"):
        pipeline.inference(None, None, tokens, max_frames=64, sample_rate=8000)  # the rate of WHAT: it needs pack
    with pytest.raises(ValueError, match="max_frames"):
        pipeline.inference(None, None, tokens, pack="ulaw")
    with pytest.raises(ValueError, match="sample_rate"):
        pipeline.inference(None, None, tokens, max_frames=64, pack="s16", sample_rate=11025)
    with pytest.raises(ValueError, match="pack"):
        pipeline.inference(None, None, tokens, max_frames=64, pack="u8")


def test_reference_contract_on_a_hand_computed_row():
    """tests/_resample_ref.py on a case small enough to write out: U / D = 2 / 3, K = 2, n = 4 -> m = 3."""
    taps = np.array([[1.0, 0.5], [0.25, 2.0]], dtype=np.float32)
    x = np.array([1.0, -2.0, 4.0, 8.0, np.nan], dtype=np.float32)  # the NaN sits at n: never looked at
    y, bound = R.polyphase(x, 4, taps, 2, 3)
    # j = 0: c 0, p 0 -> x[0] + .5 x[1];  j = 1: c 1, p 1 -> .25 x[1] + 2 x[2];  j = 2: c 3, p 0 -> x[3] + .5 * 0
    assert y.tolist() == [0.0, 7.5, 8.0]
    assert np.allclose(bound, 3 * 2.0 ** -24 * np.array([2.0, 8.5, 8.0]), rtol=0, atol=0)
    n, m = R.row_counts([0, 1, 3, 9], 3, 600, 50, 1, 3)
    assert n == [0, 550, 1750, 1750] and m == [0, 184, 584, 584]
    lo, hi = R.pcm_interval(np.array([0.0, 2.0, -2.0, 0.5]), np.array([0.0, 0.0, 0.0, 1e-4]))
    assert lo.tolist() == [0, 32767, -32767, 16380] and hi.tolist() == [0, 32767, -32767, 16387]
