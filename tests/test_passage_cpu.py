"""C ABI and host-side contract of the passage path: `st2_wave_pack_gaps` is declared, exported and bound
under ABI 23; its arguments are validated before any launch; the numpy contract of tests/_passage_ref.py equals a brute-force
per-sample loop; `pipeline` refuses what it cannot serve and leaves the calls without the new arguments on the wrappers they
always used.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _passage_ref as R
from styletts2_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_symbol_is_declared_exported_and_bound_and_the_abi_is_still_23():
    lib = _lib.load()
    text = open(HEADER).read()
    assert re.search(r"\bint st2_wave_pack_gaps\(", text)
    assert hasattr(lib, "st2_wave_pack_gaps") and "st2_wave_pack_gaps" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3
    assert not any("gaps" in s for s in _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE)


ORDER = ("wave", "w_bs", "frames", "B", "T_cap", "spf", "trim", "up", "down", "taps", "K", "fmt", "gaps", "gap_cap", "out", "cap",
         "offsets")


def _call(lib, a):
    return lib.st2_wave_pack_gaps(*[a[k] for k in ORDER], None)


def test_wave_pack_gaps_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    move = dict(wave=d, w_bs=6000, frames=d, B=2, T_cap=10, spf=600, trim=0, up=1, down=1, taps=None, K=0, fmt=_lib.PCM_S16, gaps=d,
                gap_cap=100, out=d, cap=12200, offsets=d)
    rs = dict(move, up=1, down=3, taps=d, K=16, fmt=_lib.PCM_ULAW)
    # every refusal of st2_wave_pack
    for change, word in ((dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(out=None), "NULL"),
                         (dict(offsets=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
                         (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"),
                         (dict(cap=-1), "negative"), (dict(fmt=7), "format"), (dict(w_bs=5999), "w_bs"),
                         (dict(out=C.c_void_p(257)), "aligned"),
                         # its own
                         (dict(gap_cap=-1), "gap_cap"), (dict(up=2), "up="), (dict(down=3), "down="),
                         (dict(fmt=_lib.PCM_ULAW), "taps"), (dict(fmt=_lib.PCM_ALAW), "taps"), (dict(gaps=C.c_void_p(258)), "aligned")):
        assert _call(lib, dict(move, **change)) != 0, change
        assert "st2_wave_pack_gaps" in _err(lib) and word in _err(lib), (change, _err(lib))
    # every refusal of st2_wave_resample_pack
    for change, word in ((dict(wave=None), "NULL"), (dict(frames=None), "NULL"), (dict(out=None), "NULL"),
                         (dict(offsets=None), "NULL"), (dict(B=0), "bad geometry"), (dict(B=70000), "bad geometry"),
                         (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"), (dict(trim=-1), "negative"),
                         (dict(cap=-1), "negative"), (dict(w_bs=5999), "w_bs"), (dict(up=0), ""), (dict(up=1025), ""),
                         (dict(down=0), ""), (dict(down=1025), ""), (dict(K=0), ""), (dict(K=513), ""), (dict(fmt=4), ""),
                         (dict(fmt=-1), ""), (dict(fmt=_lib.PCM_S16, out=C.c_void_p(257)), "aligned"),
                         (dict(taps=C.c_void_p(258)), "aligned"), (dict(up=1024, K=512), "LDS"), (dict(gap_cap=-5), "gap_cap")):
        assert _call(lib, dict(rs, **change)) != 0, change
        assert "st2_wave_pack_gaps" in _err(lib) and word in _err(lib), (change, _err(lib))
    # the same refusals with gaps == NULL or gap_cap == 0: the checks come before the hand-over to the wrapped entry
    for more in (dict(gaps=None), dict(gap_cap=0)):
        assert _call(lib, dict(move, B=0, **more)) != 0 and _call(lib, dict(rs, T_cap=0, **more)) != 0
        assert _call(lib, dict(move, fmt=_lib.PCM_ULAW, **more)) != 0 and _call(lib, dict(move, up=2, **more)) != 0


def test_wrapper_has_no_cpu_path_and_checks_its_format():
    w, f, g = torch.zeros(2, 1, 1200), torch.ones(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_lib.St2Error):
        ops.wave_pack_gaps(w, f, g, 10)
    with pytest.raises(ValueError):
        ops.wave_pack_gaps(w, f, g, 10, fmt="ulaw")  # G.711 needs the resampling move: a rate
    with pytest.raises(ValueError):
        ops.wave_pack_gaps(w, f, g, 10, rate=11025)


# ---- the numpy contract against a per-sample loop -----------------------------------------------------------------------------
def _brute(rows, gaps, gap_cap, fmt, cap):
    """Element by element, from the sentences of the contract: which row or gap owns position p, if any."""
    z = R.silence(fmt)
    m = [len(r) for r in rows]
    g = [0 if gaps is None else min(max(int(v), 0), gap_cap) for v in gaps] if gaps is not None else [0] * len(rows)
    off = [0]
    for b in range(len(rows)):
        off.append(off[-1] + m[b] + g[b])
    limit = min(off[-1], cap)
    out = []
    for p in range(limit):
        for b in range(len(rows)):
            if off[b] <= p < off[b] + m[b]:
                out.append(rows[b][p - off[b]])
                break
            if off[b] + m[b] <= p < off[b + 1]:
                out.append(z)
                break
        else:
            raise AssertionError("position %d below the limit belongs to nothing" % p)
    return np.asarray(out, dtype=R.DTYPES[fmt]), off, limit


@pytest.mark.parametrize("fmt", ["f32", "s16", "ulaw", "alaw"])
def test_reference_equals_a_per_sample_loop(fmt):
    g = np.random.default_rng(19)
    dt = R.DTYPES[fmt]
    mk = lambda n: (g.standard_normal(n).astype(np.float32) if fmt == "f32" else g.integers(1, 100, n).astype(dt))
    rows = [mk(7), mk(0), mk(12), mk(3), mk(5)]  # row 1: no samples, followed by a gap
    gaps, cap = [4, 6, 0, -9, 50], 10  # 0, negative, above gap_cap
    total = 7 + 4 + 0 + 6 + 12 + 0 + 3 + 0 + 5 + 10
    for limit_at in (None, 20, 9, 7 + 4 + 3, total - 4, total + 5, 0):  # whole; inside row 2; inside gap 0 / gap 1 / the last gap
        out, off, limit = R.pack_gaps(rows, gaps, cap, fmt, limit_at)
        want, woff, wlimit = _brute(rows, gaps, cap, fmt, total + 99 if limit_at is None else limit_at)
        assert off.dtype == np.int64 and off.tolist() == woff and limit == wlimit
        assert out.dtype == dt and out.tobytes() == want.tobytes()
    assert off.tolist() == [0, 11, 17, 29, 32, 47]
    out, off, _ = R.pack_gaps(rows, None, cap, fmt)
    assert out.tobytes() == np.concatenate(rows).tobytes() and off.tolist() == [0, 7, 7, 19, 22, 27]
    assert R.pack_gaps(rows, gaps, 0, fmt)[1].tolist() == off.tolist()  # gap_cap == 0: no gaps
    big = R.offsets([2 ** 31 - 1] * 3, [2 ** 31 - 1] * 3, 2 ** 31 - 1)
    assert big[-1] == 6 * (2 ** 31 - 1)  # 64-bit sums


def test_silence_is_the_encoders_zero_not_byte_zero():
    assert R.silence("f32") == 0.0 and R.silence("f32").dtype == np.float32 and R.silence("s16") == 0
    assert int(R.silence("ulaw")) == 0xFF and int(R.silence("alaw")) == 0xD5


def test_gap_samples_rounding():
    assert pipeline.gap_samples(250) == 6000 and pipeline.gap_samples(250, 8000) == 2000
    assert pipeline.gap_samples(0.0625, 8000) == 0 and pipeline.gap_samples(0.1875, 8000) == 2  # 0.5 -> 0, 1.5 -> 2: ties to even
    assert pipeline.gap_samples(0.3125, 8000) == 2 and pipeline.gap_samples(1, 44100) == 44  # 2.5 -> 2; 44.1 -> 44
    assert pipeline.gap_samples([10, 0, 33.4], 22050) == [220, 0, 736]  # 220.5 -> 220; 736.47 -> 736
    for ms, rate in ((250, 24000), (0.0625, 8000), (0.1875, 8000), (0.3125, 8000), (33.4, 22050), (1, 44100), (999.99, 48000)):
        assert pipeline.gap_samples(ms, rate) == R.gap_samples(ms, rate)


def test_pipeline_refuses_what_it_cannot_serve():
    tokens = torch.zeros(2, 5, dtype=torch.long)
    for kw in (dict(passage=True), dict(passage=[1, 0]), dict(gaps=[10, 20]), dict(gaps=[10, 20], pack="s16"),
               dict(s_prev=torch.zeros(1, 256)), dict(max_gap=5)):
        with pytest.raises(ValueError, match="max_frames"):
            pipeline.inference(None, None, tokens, **kw)
    with pytest.raises(ValueError, match="pack"):
        pipeline.inference(None, None, tokens, max_frames=64, gaps=[10, 20])
    with pytest.raises(ValueError, match="passage"):
        pipeline.inference(None, None, tokens, max_frames=64, s_prev=torch.zeros(1, 256))
    with pytest.raises(ValueError, match="gaps"):
        pipeline.inference(None, None, tokens, max_frames=64, pack="s16", gaps=[10, 20, 30])
    with pytest.raises(ValueError, match="gaps"):
        pipeline.inference(None, None, tokens, max_frames=64, pack="s16", gaps=[0.5, 2.0])
    with pytest.raises(ValueError, match="max_gap"):
        pipeline.inference(None, None, tokens, max_frames=64, pack="s16", gaps=[1, 2], max_gap=-1)
    with pytest.raises(ValueError, match="start flags"):
        pipeline.inference(None, None, tokens, max_frames=64, passage=[1, 0, 0])
    sentences = [torch.zeros(5, dtype=torch.long), torch.zeros(3, dtype=torch.long)]
    for kw in (dict(pack="s16"), dict(sample_rate=8000), dict(marks=True), dict(gaps=[1, 2])):
        with pytest.raises(ValueError, match="max_frames"):
            pipeline.synthesize_long(None, None, sentences, **kw)
    with pytest.raises(ValueError, match="decode_streams"):
        pipeline.synthesize_long(None, None, sentences, max_frames=64, decode_streams=2)
    with pytest.raises(ValueError, match="per-token"):  # without max_frames the function is untouched
        pipeline.synthesize_long(None, None, sentences, controls=pipeline.Controls(2, tok_speed=1.0, N=5, device="cpu"))


class _Result:
    def __init__(self, B):
        self.style = torch.zeros(B, 256)


def test_synthesize_long_max_frames_accepts_token_controls_and_chains_the_style(monkeypatch):
    calls = []

    def fake(model, sampler, tokens, **kw):
        calls.append(dict(kw, tokens=tokens))
        r = _Result(tokens.shape[0])
        r.style[-1] = len(calls)
        return r
    monkeypatch.setattr(pipeline, "inference", fake)
    sentences = [torch.arange(n, dtype=torch.long) + 1 for n in (5, 3, 7, 2)]
    tok = torch.ones(4, 7)
    tok[2, 1] = 0.5
    ctl = pipeline.Controls(4, tok_speed=tok, device="cpu")
    seen = []
    res, s_last = pipeline.synthesize_long(None, None, sentences, max_frames=64, pack="s16", marks=True, front_batch=2,
                                           gaps=[10, 20, 30, 40], controls=ctl, on_chunk=lambda k, r: seen.append((k, r)))
    assert len(calls) == 2 and len(res) == 2 and [k for k, _ in seen] == [0, 1] and seen[1][1] is res[1]
    a, b = calls
    assert tuple(a["tokens"].shape) == (2, 7) and tuple(b["tokens"].shape) == (2, 7)  # right-padded to the controls' width
    assert a["tokens"][1].tolist() == [1, 2, 3, 0, 0, 0, 0] and a["lengths_dev"].tolist() == [5, 3] and b["lengths_dev"].tolist() == [7, 2]
    assert a["passage"] is True and b["passage"] is True and a["s_prev"] is None
    assert b["s_prev"] is res[0].style[-1:] or torch.equal(b["s_prev"], res[0].style[-1:])
    assert torch.equal(s_last, res[1].style[-1:]) and float(s_last[0, 0]) == 2.0
    assert a["gaps"].tolist() == [10, 20] and b["gaps"].tolist() == [30, 40] and a["max_gap"] == b["max_gap"] == 40
    assert a["max_frames"] == 64 and a["pack"] == "s16" and a["marks"] is True and a["trim"] == 0
    assert b["controls"].B == 2 and torch.equal(b["controls"].tok_row("tok_speed"), tok[2:4])
    with pytest.raises(ValueError, match="longest sentence"):
        pipeline.synthesize_long(None, None, sentences, max_frames=64, controls=pipeline.Controls(4, tok_speed=1.0, N=9, device="cpu"))


def test_calls_without_the_new_arguments_stay_on_the_old_wrappers(monkeypatch):
    """`_hand_over` without gaps goes through ops.wave_pack / ops.wave_resample_pack with the layout it always had; with gaps
    through ops.wave_pack_gaps, B * max_gap samples and B int32 larger."""
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append((name, a, {k: v for k, v in kw.items() if k not in ("out", "offsets")}, kw["out"].numel()))
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    B, L = 3, 1200
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    ho = pipeline._hand_over(wave, frames, 0, "s16", 600)
    assert seen[-1][0] == "wave_pack" and ho.buf.numel() == 32 + 2 * B * L and ho.packed.numel() == B * L and ho.gaps is None
    ho = pipeline._hand_over(wave, frames, 0, "ulaw", 600, 8000, n_marks=B * 6)
    assert seen[-1][0] == "wave_resample_pack" and seen[-1][1] == (8000,)
    assert ho.buf.numel() == (32 + 4 * B * 6 + 15) // 16 * 16 + B * 400 and ho.gaps is None
    assert not any(n == "wave_pack_gaps" for n, *_ in seen)
    gaps = torch.tensor([5, 0, 70], dtype=torch.int32)
    ho = pipeline._hand_over(wave, frames, 0, "s16", 600, gaps=gaps, max_gap=64)
    assert seen[-1][0] == "wave_pack_gaps" and seen[-1][2]["rate"] is None and seen[-1][1][1] == 64
    assert ho.packed.numel() == B * (L + 64) and ho.buf.numel() == (32 + 4 * B + 15) // 16 * 16 + 2 * B * (L + 64)
    g = ho.gaps
    assert g.tolist() == [5, 0, 70] and g.data_ptr() == ho.buf.data_ptr() + 32  # the kernel reads them from the hand-over's header
    assert seen[-1][1][0].data_ptr() == g.data_ptr()
    ho = pipeline._hand_over(wave, frames, 0, "alaw", 600, 8000, n_marks=B * 6, gaps=gaps, max_gap=8)
    assert seen[-1][0] == "wave_pack_gaps" and seen[-1][2]["rate"] == 8000 and ho.packed.numel() == B * (400 + 8)
    assert ho.gaps.data_ptr() == ho.buf.data_ptr() + 32 + 4 * B * 6
    ho = pipeline._hand_over(wave, frames, 0, "ulaw", 600, None, gaps=gaps, max_gap=8)
    assert seen[-1][2]["rate"] == 24000  # G.711 at the model rate: the resampling move with U = D = 1


def test_public_signatures_carry_the_new_arguments():
    import inspect
    assert {"marks", "passage"} <= set(inspect.signature(pipeline.SynthesisResult.to_host).parameters)
    assert {"passage", "gaps", "max_gap", "s_prev", "t"} <= set(inspect.signature(pipeline.inference).parameters)
    assert {"passage", "max_gap", "t"} <= set(inspect.signature(pipeline.GraphedSynthesis.__init__).parameters)
    assert {"starts", "s_prev", "gaps"} <= set(inspect.signature(pipeline.GraphedSynthesis.__call__).parameters)
    assert {"max_frames", "pack", "sample_rate", "marks", "gaps"} <= set(inspect.signature(pipeline.synthesize_long).parameters)
