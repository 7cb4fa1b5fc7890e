"""C ABI and host-side contract of the timing marks and per-token controls, the part that needs no GPU:
the five new entry points are declared, exported and bound under ABI 23 without a version bump, a struct change or a
backend-table slot; `st2_token_marks` validates its arguments before any launch; `pipeline.Controls` validates the token
rows; `marks=` is refused where it has no meaning; and the numpy contract of tests/_marks_ref.py is checked against a
brute-force per-frame expansion."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _marks_ref as R
from styletts2_amd import _lib, ops, pipeline, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "st2.h")
NEW = ("st2_token_marks", "st2_prosody_controls_tok", "st2_duration_head_rate_tok", "st2_front_forward_tok",
       "st2_sizeof_token_controls")


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_abi_stays_23_and_the_five_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 23 and lib.st2_abi_version() == 23 and "#define ST2_ABI_VERSION 23" in text
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in st2.h" % name
        assert hasattr(lib, name), "%s is not exported" % name
        assert name in _lib.EXPORTS
    # additive: no struct grew, no backend-table slot was added
    assert lib.st2_sizeof_front_args() == C.sizeof(_lib.FrontArgs)
    assert lib.st2_sizeof_controls() == C.sizeof(_lib.ControlRows) == 4 * C.sizeof(C.c_void_p)
    assert lib.st2_sizeof_token_controls() == C.sizeof(_lib.TokenControlRows) == C.sizeof(C.c_void_p)
    assert [f[0] for f in _lib.TokenControlRows._fields_] == ["speed"]
    assert len(_lib.BACKEND_SLOTS) == 33 and len(_lib.BACKEND_SLOTS_RAGGED) == 11 and len(_lib.BACKEND_SLOTS_STYLE) == 3


def test_token_marks_validates_before_any_launch():
    lib = _lib.load()
    d = C.c_void_p(256)
    f = lib.st2_token_marks
    ok = dict(dur=d, B=2, N=8, len=None, frames=None, T_cap=100, shift=0, spf=600, trim=0, up=1, down=1, marks=d, bound=None)
    for change, word in ((dict(dur=None), "NULL"), (dict(marks=None), "NULL"), (dict(N=513), "512"), (dict(up=0), "1..1024"),
                         (dict(up=1025), "1..1024"), (dict(down=0), "1..1024"), (dict(down=1025), "1..1024"),
                         (dict(trim=-1), "negative"), (dict(B=0), "bad geometry"), (dict(N=0), "bad geometry"),
                         (dict(T_cap=0), "bad geometry"), (dict(spf=0), "bad geometry"),
                         (dict(T_cap=4_000_000), "int32"),  # 600 * 4e6 = 2.4e9 samples
                         (dict(T_cap=1_000_000, up=4, down=1), "int32"),  # fits at 24 kHz, not at four times the rate
                         (dict(T_cap=30_000, up=1024, down=1), "int32")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_token_marks" in _err(lib) and word in _err(lib), (change, _err(lib))
    f = lib.st2_prosody_controls_tok
    ok = dict(f0=d, n=d, bs=16, B=2, L=16, dur=d, N=4, shift=0, sc=d, sh=d, frames=None)
    for change, word in ((dict(f0=None), "NULL"), (dict(n=None), "NULL"), (dict(dur=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(L=15), "bad geometry"), (dict(bs=15), "bad geometry"), (dict(N=0), "bad geometry"), (dict(N=513), "512")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_prosody_controls_tok" in _err(lib) and word in _err(lib), (change, _err(lib))
    assert f(d, d, 16, 2, 16, d, 4, 0, None, None, None, None) == 0  # nothing to apply: no launch, no error
    f = lib.st2_duration_head_rate_tok
    ok = dict(x=d, x_bs=2048, x_cs=4, w=d, bias=d, B=2, K=512, J=50, N=4, len=None, tail=0, speed=None, tok=d, dur=d, dsum=None)
    for change, word in ((dict(x=None), "NULL"), (dict(tok=None), "NULL"), (dict(dur=None), "NULL"), (dict(B=0), "bad geometry"),
                         (dict(tail=-1), "bad geometry"), (dict(B=70000), "grid")):
        a = dict(ok, **change)
        assert f(*a.values(), None) != 0, change
        assert "st2_duration_head_rate_tok" in _err(lib) and word in _err(lib), (change, _err(lib))
    assert lib.st2_front_forward_tok(None, None, None, None, None, 0, None) != 0


def test_wrappers_have_no_cpu_path_and_check_their_rows_first():
    dur = torch.ones(2, 4, dtype=torch.int64)
    with pytest.raises(_lib.St2Error):
        ops.token_marks(dur, None, 16)
    with pytest.raises(_lib.St2Error):
        ops.prosody_controls_tok(torch.zeros(2, 8), torch.zeros(2, 8), dur, tok_f0_scale=None, tok_n_shift=None)
    with pytest.raises(_lib.St2Error, match="tok_f0_scale"):
        ops.prosody_controls_tok(torch.zeros(2, 8), torch.zeros(2, 8), dur, tok_f0_scale=torch.ones(2, 3))
    with pytest.raises(_lib.St2Error, match="tok_speed"):
        ops.duration_head(torch.zeros(2, 8, 4), torch.zeros(5, 8), torch.zeros(5), tok_speed=torch.ones(2, 4))  # a host row


BAD = {"tok_speed": (0.2, 4.5, 0.0, -1.0), "tok_f0_scale": (0.49, 2.1, 0.0), "tok_n_shift": (-2.5, 2.01)}


@pytest.mark.parametrize("name", pipeline.Controls.TOK_NAMES)
def test_controls_validates_every_host_token_value(name):
    lo, hi = pipeline.Controls.TOK_RANGES[name]
    assert (lo, hi) == R.TOK_RANGES[name] and pipeline.Controls.TOK_ABSENT[name] == R.TOK_NEUTRAL[name]
    B, N = 2, 3
    good = [[lo, hi, (lo + hi) / 2], [hi, lo, lo]]
    for bad in BAD[name] + (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(B, device="cpu", N=N, **{name: bad})
        rows = [list(r) for r in good]
        rows[1][2] = bad
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(B, device="cpu", **{name: rows})  # one bad value in a nested sequence
        with pytest.raises(ValueError, match=name):
            pipeline.Controls(B, device="cpu", **{name: torch.tensor(rows)})  # ... or in a host tensor
    with pytest.raises(ValueError, match=name):
        pipeline.Controls(B, device="cpu", N=N, **{name: [[lo, hi], [lo, hi]]})  # two tokens for three
    with pytest.raises(ValueError, match=name):
        pipeline.Controls(B, device="cpu", N=N, **{name: [lo, hi, lo]})  # one row for two
    with pytest.raises(ValueError, match="N"):
        pipeline.Controls(B, device="cpu", **{name: lo})  # a scalar says nothing about the width
    with pytest.raises(ValueError):
        pipeline.Controls(B, device="cpu", N=513, **{name: lo})
    c = pipeline.Controls(B, device="cpu", **{name: good})  # the ends of the range are legal; N from the array
    assert c.N == N and c.tok_present == (name,) and c.present == ()
    assert c.tok_row(name).tolist() == [[float(np.float32(v)) for v in r] for r in good]
    assert all(c.tok_row(n) is None for n in c.TOK_NAMES if n != name)


def test_token_controls_layout_neutral_and_slices():
    c = pipeline.Controls(4, speed=[1, 0.5, 2, 4], tok_speed=2.0, N=5, device="cpu")
    assert c.buf.shape == (6, 4) and c.tok_buf.shape == (3, 4, 5) and c.tok_buf.dtype == torch.float32
    assert set(c.front_rows()) == {"speed", "tok_speed"} and c.front_rows()["tok_speed"].tolist() == [[2.0] * 5] * 4
    # an absent token row holds the device clamp's neutral value
    assert c.tok_buf[1].tolist() == [[1.0] * 5] * 4 and c.tok_buf[2].tolist() == [[0.0] * 5] * 4
    s = c.slice(1, 3)
    assert s.B == 2 and s.N == 5 and s.tok_present == ("tok_speed",) and s.tok_row("tok_speed").shape == (2, 5)
    assert s.tok_buf.data_ptr() == c.tok_buf[:, 1:].data_ptr()
    plain = pipeline.Controls(4, speed=1.5, device="cpu")  # no token argument: no second tensor, nothing new for the front
    assert plain.tok_buf is None and plain.N is None and plain.tok_present == () and set(plain.front_rows()) == {"speed"}
    assert plain.slice(0, 2).tok_buf is None
    n = pipeline.Controls.neutral(2, device="cpu", N=7)
    assert n.tok_present == n.TOK_NAMES and n.tok_row("tok_speed").tolist() == [[1.0] * 7] * 2
    assert n.tok_row("tok_n_shift").tolist() == [[0.0] * 7] * 2
    assert pipeline.Controls.neutral(2, device="cpu").tok_buf is None


def test_refused_combinations(monkeypatch):
    tokens = torch.zeros(2, 5, dtype=torch.long)
    for kw in (dict(), dict(max_frames=64), dict(pack="s16")):
        with pytest.raises(ValueError, match="marks"):
            pipeline.inference(None, None, tokens, marks=True, **kw)
    # tok_speed with forced durations raises, as speed does; checked behind the device checks (a stand-in HIP device)
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(pipeline.Controls, "device", property(lambda self: dev))
    dur = torch.full((2, 5), 3)
    c = pipeline.Controls(2, tok_speed=1.25, N=5, device="cpu")
    with pytest.raises(ValueError, match="nothing to scale"):
        pipeline._check_controls(c, dev, 2, None, None, dur, 5)
    pipeline._check_controls(pipeline.Controls(2, tok_f0_scale=1.5, N=5, device="cpu"), dev, 2, None, None, dur, 5)  # pitch alone is fine
    with pytest.raises(ValueError, match="tokens"):
        pipeline._check_controls(c, dev, 2, None, None, None, 6)  # rows of another width
    with pytest.raises(ValueError, match="long-form"):
        pipeline.synthesize_long(None, None, [tokens[0], tokens[1]], controls=c)
    r = pipeline.SynthesisResult(torch.zeros(1, 1, 600), torch.ones(1, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="marks"):
        r.to_host(marks=True)


def test_rate_ratio_is_the_resampler_table_ratio():
    for rate in resample.RATES:
        assert resample.ratio(rate) == resample.design(rate)[:2]
    with pytest.raises(ValueError):
        resample.ratio(11025)


# ---- the numpy contract against a brute-force per-frame expansion ------------------------------------------------------------
def _cases():
    """(dur [B, N], lengths or None, frames, T_cap): random durations with zeros, len = 0 / 1 / N, rows over capacity, rows whose
    durations fall short of their frames."""
    g = np.random.default_rng(18)
    out = []
    for N in (1, 2, 7, 20):
        B = 6
        dur = g.integers(0, 6, size=(B, N)).astype(np.int64)
        dur[g.random((B, N)) < 0.3] = 0
        dur[4] = 0  # an all-zero row
        lens = np.array([0, 1, N, N, N, max(N // 2, 1)], dtype=np.int64)
        for b in range(B):
            dur[b, lens[b]:] = 0  # what the duration head writes at pad tokens
        T_cap = max(int(dur.sum(axis=1).max()) - 3, 4)  # the longest row is over capacity
        frames = np.clip(dur.sum(axis=1), 1, T_cap)  # st2_frames_from_durations
        out.append((dur, lens, frames, T_cap))
        out.append((dur, None, frames + np.array([0, 2, 0, 1, 0, 0]), T_cap + 2))  # forced durations, short of `frames`
    return out


@pytest.mark.parametrize("shift", [0, 1])
def test_bounds_are_the_first_frame_of_the_brute_force_expansion(shift):
    checked = 0
    for dur, lens, frames, T_cap in _cases():
        bd = R.bounds(dur, lens, frames, T_cap, shift)
        B, N = dur.shape
        for b in range(B):
            T_b = int(min(max(frames[b], 0), T_cap))
            idx = R.brute_index(dur[b], T_b, shift)
            for n in range(N + 1):
                want = T_b if n == N else R.first_frame_at_or_past(idx, n, T_b)
                assert bd[b, n] == want, (N, b, n, dur[b].tolist(), T_b, bd[b].tolist())
                checked += 1
            assert bd[b, 0] == 0 and bd[b, N] == T_b and np.all(np.diff(bd[b]) >= 0)
            total = int(dur[b].sum())
            if lens is not None and total >= 1:  # pad tokens sit at the row's end (a row of no frames at all has no end to sit at)
                assert np.all(bd[b, max(int(lens[b]), 1):] == T_b), (b, bd[b].tolist())
            if total > T_cap:  # a truncated row: every token that starts at or past the capacity gets T_b
                c = np.cumsum(dur[b])
                assert all(bd[b, n] == T_b for n in range(1, N + 1) if c[n - 1] >= T_cap)
    assert checked > 300


@pytest.mark.parametrize("rate", resample.RATES)
def test_marks_are_monotone_and_end_at_the_packed_row_length(rate):
    U, D = resample.ratio(rate)
    for dur, lens, frames, T_cap in _cases():
        for shift, trim in ((0, 0), (1, 50), (0, 10 ** 7)):
            m = R.marks(dur, lens, frames, T_cap, shift, 600, trim, U, D)
            bd = R.bounds(dur, lens, frames, T_cap, shift)
            for b in range(dur.shape[0]):
                T_b = int(min(max(frames[b], 0), T_cap))
                n_smp = max(0, 600 * T_b - trim)
                assert m[b, 0] == 0 and np.all(np.diff(m[b]) >= 0)
                assert m[b, -1] == resample.output_samples(n_smp, U, D)
                for n in range(dur.shape[1] + 1):  # the first output sample j whose input position (j D) div U is at or past s
                    s = min(600 * int(bd[b, n]), n_smp)
                    j = int(m[b, n])
                    assert (j * D) // U >= s and (j == 0 or ((j - 1) * D) // U < s)


def test_numpy_contract_of_the_token_rate():
    f = lambda v: np.array([v], dtype=np.float32)
    d = lambda total, speed, tok, **kw: R.durations(f(total), None if speed is None else [speed], f(tok), **kw)[0].tolist()
    assert d([2.5, 3.5, 25.0], None, [1.0, 1.0, 2.0]) == [2, 4, 12]  # round half to even, 12.5 -> 12
    assert d([10.0, 10.0, 10.0], None, [0.0, 100.0, float("nan")]) == [40, 2, 10]  # the device clamp
    assert d([10.0, 10.0], 4.0, [4.0, 0.25]) == [2, 10]  # the PRODUCT is clamped to [0.25, 4] too
    assert d([10.0, 10.0], 0.25, [0.25, 4.0]) == [40, 10]
    assert d([3.0, 3.0, 3.0, 3.0], None, [0.5, 1.0, 1.0, 1.0], lengths=[2], tail=5) == [6, 8, 0, 0]  # the tail is not scaled
    assert d([0.4], 2.0, [2.0]) == [1]  # never below one frame
    F0, N = R.prosody_tok(f([1, 2, 3, 4, 5, 6, 7, 8]), f([1, 2, 3, 4, 5, 6, 7, -0.0]), np.array([[1, 2, 5]]), 0,
                          f([2.0, 0.5, 9.0]), f([0.5, float("nan"), 0.0]), frames=[4])
    assert F0[0].tolist() == [2.0, 4.0, 1.5, 2.0, 2.5, 3.0, 14.0, 16.0] and N[0].tolist()[:6] == [1.5, 2.5, 3.0, 4.0, 5.0, 6.0]
    assert np.signbit(N[0, 7]) and N[0, 6] == 7.0  # a zero shift selects x
    F0s, _ = R.prosody_tok(f([1, 1, 1, 1, 1, 1, 1, 1]), f([0] * 8), np.array([[1, 2, 5]]), 1, f([2.0, 0.5, 1.0]), None, frames=[3])
    assert F0s[0].tolist() == [2.0, 2.0, 2.0, 2.0, 0.5, 0.5, 1.0, 1.0]  # the shift repeats frame 0's token
