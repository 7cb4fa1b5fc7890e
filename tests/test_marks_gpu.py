"""Timing marks and per-token prosody controls on the device: `st2_token_marks`, `st2_prosody_controls_tok`
and the token-rate duration head against the numpy contract of tests/_marks_ref.py AND against the expansion kernel they must
agree with, then the `marks=` / token-control paths of the pipeline against the paths without them.  Every comparison is
integer-exact or one fp32 operation: bit equality throughout.  Shapes are the smallest at which the kernels can still go wrong
(token counts across the 64-lane scan chunks, more than one 1024-column workgroup per row); the pipeline cases reuse the tiny
seeded models and the B = 3 batch of tests/test_controls_gpu.py."""
import warnings

import numpy as np
import pytest
import torch

import _marks_ref as R
from styletts2_amd import _lib, ops, pipeline, resample
from test_controls_gpu import CAPACITY_BITS, LENS, STEPS, T_SINE, _batch, _kw, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = (24000, 8000, 44100, 48000)


def _dev(v, dtype=torch.float32):
    return torch.tensor(v, dtype=dtype, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. st2_token_marks against the numpy contract --------------------------------------------------------------------------
def _marks_rows(N, seed):
    """B = 5: random durations with zeros; row 3 runs over the capacity; row 4 is all zero (its frame count clamps to 1)."""
    g = np.random.default_rng(seed)
    dur = g.integers(0, 7, size=(5, N)).astype(np.int64)
    dur[g.random((5, N)) < 0.25] = 0
    dur[4] = 0
    T_cap = max(int(dur[:3].sum(axis=1).max()), 2)
    dur[3, N // 2] += T_cap + 3
    return dur, T_cap


@pytest.mark.parametrize("N", [1, 7, 64, 65, 130, 512])
def test_token_marks_equal_the_numpy_contract(N):
    dur, T_cap = _marks_rows(N, 100 + N)
    d = _dev(dur, torch.int64)
    torch.cuda.synchronize()
    ops.status(clear=True)
    checked = 0
    for lens in ([0, 1, N, N, N], None):
        ld = None if lens is None else _dev(lens, torch.int32)
        frames = ops.frames_from_durations(d, ld, T_cap)
        fh = frames.cpu().numpy()
        assert fh[3] == T_cap and fh[4] == 1 and (lens is None or fh[0] == 1)
        for shift in (0, 1):
            want_b = R.bounds(dur, lens, fh, T_cap, shift)
            for trim in (0, 50, 600 * T_cap + 7):
                for rate in RATES:
                    U, D = resample.ratio(rate)
                    m, bd = ops.token_marks(d, frames, T_cap, lengths=ld, shift=bool(shift), trim=trim, rate=rate, want_bound=True)
                    assert m.dtype == torch.int32 and tuple(m.shape) == (5, N + 1)
                    want = R.marks(dur, lens, fh, T_cap, shift, 600, trim, U, D)
                    assert np.array_equal(m.cpu().numpy(), want), (lens, shift, trim, rate)
                    assert np.array_equal(bd.cpu().numpy(), want_b), (lens, shift, trim, rate)
                    n_smp = np.maximum(0, 600 * fh.astype(np.int64) - trim)
                    assert m[:, N].cpu().tolist() == [resample.output_samples(int(v), U, D) for v in n_smp]
                    checked += 1
    assert checked == 48
    # frames = None: every row has T_cap frames; rate None is 24 kHz
    m = ops.token_marks(d, None, T_cap, trim=50)
    assert np.array_equal(m.cpu().numpy(), R.marks(dur, None, None, T_cap, 0, 600, 50))
    torch.cuda.synchronize()
    assert ops.status() & ~_lib.STATUS_FRAME_CAPACITY == 0  # frames_from_durations reports row 3; the marks kernel raises nothing
    ops.status(clear=True)


def test_token_marks_pass_2_to_the_31_inside_and_stay_exact():
    """T_cap = 30 000 and one duration of 30 000 at 44.1 kHz: 600 * 30 000 * 147 = 2.646e9 > 2^31 inside, 33 075 000 samples out."""
    B, N, T_cap = 5, 7, 30000
    dur = np.zeros((B, N), dtype=np.int64)
    dur[0, 0] = 30000
    dur[1] = [4000, 0, 9000, 1, 8000, 8999, 0]
    dur[2, 3] = 2 ** 40  # saturates, never wraps
    dur[3] = 5
    frames = [30000, 30000, 30000, 35, 1]
    d, f = _dev(dur, torch.int64), _dev(frames, torch.int32)
    U, D = resample.ratio(44100)
    for shift in (0, 1):
        m, bd = ops.token_marks(d, f, T_cap, shift=bool(shift), trim=50, rate=44100, want_bound=True)
        want = R.marks(dur, None, frames, T_cap, shift, 600, 50, U, D)
        assert want.max() == resample.output_samples(600 * 30000 - 50, U, D) > 2 ** 24 and 600 * 30000 * U > 2 ** 31
        assert np.array_equal(m.cpu().numpy(), want) and np.array_equal(bd.cpu().numpy(), R.bounds(dur, None, frames, T_cap, shift))


# ---- 2. the boundaries against the expansion kernel itself ------------------------------------------------------------------
@pytest.mark.parametrize("N", [9, 70])
@pytest.mark.parametrize("shift", [0, 1])
def test_bounds_are_where_the_expansion_kernel_changes_token(N, shift):
    g = np.random.default_rng(7 * N + shift)
    B, T = 4, 96
    dur = g.integers(0, 4, size=(B, N)).astype(np.int64)
    dur[0] = 0
    dur[0, :6] = [3, 0, 0, 5, 1, 7]  # short of its frames: the last token owns the rest
    dur[1, N - 1] += 400  # truncated
    dur[2, 0] = 0  # a leading zero duration
    sums = dur.sum(axis=1)
    frames = [40, T, int(max(min(sums[2], T), 1)), int(min(sums[3] + 9, T))]  # rows 0 and 3 fall short of `frames`
    d, f = _dev(dur, torch.int64), _dev(frames, torch.int32)
    x = torch.arange(N, dtype=torch.float32, device=DEV).reshape(1, 1, N).expand(B, 1, N).contiguous()  # the ramp x[b][0][n] = n
    y = ops.expand_by_durations(x, d, T, shift=bool(shift), lengths=f)[:, 0].cpu().numpy()
    _, bd = ops.token_marks(d, f, T, shift=bool(shift), want_bound=True)
    bd = bd.cpu().numpy()
    for b in range(B):
        T_b = frames[b]
        for n in range(N + 1):
            hit = np.nonzero(y[b, :T_b] >= n)[0]
            want = T_b if n == N or hit.size == 0 else int(hit[0])
            assert bd[b, n] == want, (b, n, dur[b].tolist(), T_b, bd[b].tolist())
    assert np.array_equal(bd, R.bounds(dur, None, frames, T, shift))
    torch.cuda.synchronize()
    ops.status(clear=True)  # the expansion reports the rows whose durations do not sum to their frames: expected here


# ---- 3. st2_prosody_controls_tok ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_prosody_controls_tok_is_one_operation_per_element_and_stops_at_the_row(shift):
    B, T, N = 3, 700, 70  # L = 1400: two workgroups of 1024 columns per row, the second partial; N crosses one scan chunk
    L = 2 * T
    frames = [700, 513, 1]
    g = torch.Generator().manual_seed(18 + shift)
    dur = torch.randint(0, 16, (B, N), generator=g)
    dur[0, N - 1] += 700  # runs over: truncated at T
    dur[1, 40:] = 0  # falls short of 513: token N - 1 owns the rest
    dur[:, 0] = 9  # columns 0 .. 17 of every row belong to token 0, whose shift is 0
    F0, Nc = torch.randn(B, L, generator=g) * 100 + 200, torch.randn(B, L, generator=g)
    Nc[0, 5], Nc[1, 0] = -0.0, -0.0
    for b, f in enumerate(frames):  # poisoned tails: nothing of them may be read into a result or overwritten
        F0[b, 2 * f:] = float("nan")
        Nc[b, 2 * f:] = float("nan")
    sc = torch.rand(B, N, generator=g) * 1.5 + 0.5
    sh = torch.rand(B, N, generator=g) * 4 - 2
    sh[:, ::3] = 0.0
    d, fd = dur.to(DEV), _dev(frames, torch.int32)
    torch.cuda.synchronize()
    ops.status(clear=True)

    def expanded(row):  # the token row as the EXPANSION kernel lays it over the frames, twice per frame
        e = ops.expand_by_durations(row.to(DEV).reshape(B, 1, N).contiguous(), d, T, shift=bool(shift), lengths=fd)[:, 0]
        return e.repeat_interleave(2, dim=1)
    torch.cuda.synchronize()
    e_sc, e_sh = expanded(sc), expanded(sh)
    torch.cuda.synchronize()
    ops.status(clear=True)  # the expansion's DURATION_SUM for the rows made to run over / fall short
    f0, n = ops.prosody_controls_tok(F0.to(DEV), Nc.to(DEV), d, sc.to(DEV), sh.to(DEV), frames=fd, shift=bool(shift))
    F0d, Nd = F0.to(DEV), Nc.to(DEV)
    for b in range(B):
        e = 2 * frames[b]
        assert torch.equal(_bits(f0[b, :e]), _bits(F0d[b, :e] * e_sc[b, :e])), "row %d F0" % b
        want_n = torch.where(e_sh[b, :e] == 0, Nd[b, :e], Nd[b, :e] + e_sh[b, :e])
        assert torch.equal(_bits(n[b, :e]), _bits(want_n)), "row %d N" % b
        assert torch.equal(_bits(f0[b, e:]), _bits(F0d[b, e:])) and torch.equal(_bits(n[b, e:]), _bits(Nd[b, e:])), "row %d tail" % b
    assert bool(torch.signbit(n[0, 5])) and float(n[0, 5]) == 0.0, "-0.0 survives a zero shift"
    wf, wn = R.prosody_tok(F0.numpy(), Nc.numpy(), dur.numpy(), shift, sc.numpy(), sh.numpy(), frames)
    assert np.array_equal(f0.cpu().numpy().view(np.uint32), wf.view(np.uint32)), "the numpy contract, bit for bit"
    assert np.array_equal(n.cpu().numpy().view(np.uint32), wn.view(np.uint32))
    # neutral rows leave every bit; one curve alone leaves the other
    f1, n1 = ops.prosody_controls_tok(F0.to(DEV), Nc.to(DEV), d, torch.ones(B, N, device=DEV), torch.zeros(B, N, device=DEV),
                                      frames=fd, shift=bool(shift))
    assert torch.equal(_bits(f1), _bits(F0d)) and torch.equal(_bits(n1), _bits(Nd))
    f2, n2 = ops.prosody_controls_tok(F0.to(DEV), Nc.to(DEV), d, None, sh.to(DEV), frames=fd, shift=bool(shift))
    assert torch.equal(_bits(f2), _bits(F0d)) and torch.equal(_bits(n2), _bits(n))
    # a constant token row is the per-row control with that scalar
    cs, ch = [2.0, 0.7, 1.0], [0.0, -1.25, 0.3]
    f3, n3 = ops.prosody_controls_tok(F0.to(DEV), Nc.to(DEV), d, _dev(cs)[:, None].expand(B, N).contiguous(),
                                      _dev(ch)[:, None].expand(B, N).contiguous(), frames=fd, shift=bool(shift))
    f4, n4 = ops.prosody_controls(F0.to(DEV), Nc.to(DEV), _dev(cs), _dev(ch), frames=fd)
    assert torch.equal(_bits(f3), _bits(f4)) and torch.equal(_bits(n3), _bits(n4))
    # device values out of range or NaN: clamped where they are read, no fault, no status bit
    bad = torch.tensor([0.0, 100.0, float("nan")]).repeat(B, (N + 2) // 3)[:, :N].contiguous()
    f5, n5 = ops.prosody_controls_tok(F0.to(DEV), Nc.to(DEV), d, bad.to(DEV), (bad - 50.0).to(DEV), frames=fd, shift=bool(shift))
    wf, wn = R.prosody_tok(F0.numpy(), Nc.numpy(), dur.numpy(), shift, R.clamp("tok_f0_scale", bad.numpy()),
                           R.clamp("tok_n_shift", (bad - 50.0).numpy()), frames)
    assert R.clamp("tok_f0_scale", bad.numpy())[0, :3].tolist() == [0.5, 2.0, 1.0]
    assert R.clamp("tok_n_shift", (bad - 50.0).numpy())[0, :3].tolist() == [-2.0, 2.0, 0.0]
    assert np.array_equal(f5.cpu().numpy().view(np.uint32), wf.view(np.uint32))
    assert np.array_equal(n5.cpu().numpy().view(np.uint32), wn.view(np.uint32))
    # without `frames` every row is T frames long
    F0f, Nf = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    f6, n6 = ops.prosody_controls_tok(F0f.to(DEV), Nf.to(DEV), d, sc.to(DEV), sh.to(DEV), shift=bool(shift))
    wf, wn = R.prosody_tok(F0f.numpy(), Nf.numpy(), dur.numpy(), shift, sc.numpy(), sh.numpy(), None)
    assert np.array_equal(f6.cpu().numpy().view(np.uint32), wf.view(np.uint32))
    assert np.array_equal(n6.cpu().numpy().view(np.uint32), wn.view(np.uint32))
    torch.cuda.synchronize()
    assert ops.status() == 0


# ---- 4. the duration head with a per-token rate --------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 5])
def test_duration_head_token_rate_is_the_numpy_contract_bit_for_bit(tail):
    B, K, N, J = 3, 512, 24, 50
    lens = [24, 17, 1]
    g = torch.Generator().manual_seed(41)
    x = (torch.randn(B, K, N, generator=g) * 0.5).to(DEV)
    w = (torch.randn(J, K, generator=g) / K ** 0.5).to(DEV)
    bias = (torch.randn(J, generator=g) * 0.5).to(DEV)
    ld = _dev(lens, torch.int32)
    tok = torch.rand(B, N, generator=g) * 3.75 + 0.25
    speeds = [1.0, 0.8, 1.5]
    torch.cuda.synchronize()
    ops.status(clear=True)
    dur0, sums = ops.duration_head(x, w, bias, lengths=ld, tail=tail, want_sums=True)
    total = sums.cpu().numpy()
    dur, sums_t = ops.duration_head(x, w, bias, lengths=ld, tail=tail, want_sums=True, tok_speed=tok.to(DEV))
    assert torch.equal(sums_t, sums), "the sums are formed before the division: unchanged"
    assert dur.dtype == torch.int64 and np.array_equal(dur.cpu().numpy(), R.durations(total, None, tok.numpy(), lens, tail))
    both = ops.duration_head(x, w, bias, lengths=ld, tail=tail, speed=_dev(speeds), tok_speed=tok.to(DEV))
    assert np.array_equal(both.cpu().numpy(), R.durations(total, speeds, tok.numpy(), lens, tail)), "row rate times token rate"
    assert not torch.equal(dur, dur0) and not torch.equal(both, dur)
    # neutral keeps the bits; a constant token rate is the per-row rate, bit for bit
    one = torch.ones(B, N, device=DEV)
    assert torch.equal(ops.duration_head(x, w, bias, lengths=ld, tail=tail, tok_speed=one), dur0)
    assert torch.equal(ops.duration_head(x, w, bias, lengths=ld, tail=tail, speed=_dev([1.0] * B), tok_speed=one), dur0)
    for c in (0.8, 1.5, 3.0):
        a = ops.duration_head(x, w, bias, lengths=ld, tail=tail, tok_speed=torch.full((B, N), c, device=DEV))
        assert torch.equal(a, ops.duration_head(x, w, bias, lengths=ld, tail=tail, speed=_dev([c] * B))), c
    # one token's rate changes that token's duration alone
    t1 = torch.ones(B, N)
    t1[0, 3] = 0.5
    d1 = ops.duration_head(x, w, bias, lengths=ld, tail=tail, tok_speed=t1.to(DEV))
    keep = torch.ones(B, N, dtype=torch.bool)
    keep[0, 3] = False
    assert torch.equal(d1.cpu()[keep], dur0.cpu()[keep]) and int(d1[0, 3]) > int(dur0[0, 3])
    # device values out of range or NaN: the clamped / neutral token, no fault, no status bit
    bad = torch.tensor([0.0, 100.0, float("nan")]).repeat(B, N // 3).contiguous()
    got = ops.duration_head(x, w, bias, lengths=ld, tail=tail, tok_speed=bad.to(DEV))
    assert np.array_equal(got.cpu().numpy(), R.durations(total, None, bad.numpy(), lens, tail))
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("J,speed,tok,want", [(5, None, 1.0, 2), (7, None, 1.0, 4), (50, None, 2.0, 12), (5, 2.0, 1.0, 1),
                                              (7, 1.0, 2.0, 2), (50, 2.0, 2.0, 6), (50, 4.0, 4.0, 6), (7, 0.5, 0.5, 14)])
def test_duration_head_token_rate_rounds_ties_to_even(J, speed, tok, want):
    """w = 0, bias = 0: every sigmoid is exactly 0.5, the sum J / 2 exactly: 2.5 -> 2, 3.5 -> 4, 12.5 -> 12, 1.25 -> 1, 1.75 -> 2,
    6.25 -> 6; 4 * 4 clamps to 4 (6.25 -> 6); 0.5 * 0.5 = 0.25 (14)."""
    B, K, N = 2, 64, 3
    x = torch.randn(B, K, N, generator=torch.Generator().manual_seed(J)).to(DEV)
    w, bias = torch.zeros(J, K, device=DEV), torch.zeros(J, device=DEV)
    sp = None if speed is None else _dev([speed] * B)
    dur, sums = ops.duration_head(x, w, bias, want_sums=True, speed=sp, tok_speed=torch.full((B, N), tok, device=DEV))
    assert sums.cpu().tolist() == [[J / 2.0] * N] * B
    assert dur.cpu().tolist() == [[want] * N] * B
    assert np.array_equal(dur.cpu().numpy(), R.durations(sums.cpu().numpy(), None if speed is None else [speed] * B,
                                                         np.full((B, N), tok, dtype=np.float32)))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def _tok_controls(B, N):
    """Token controls that differ from token to token and from row to row (host values, in range)."""
    g = torch.Generator().manual_seed(5)
    tok_speed = torch.ones(B, N)
    tok_speed[0, 2:5] = 0.5  # "slow this word down"
    tok_speed[1, 1] = 2.0
    tok_f0 = torch.ones(B, N)
    tok_f0[2, :4] = 1.25  # "raise the pitch on this phrase"
    tok_n = (torch.rand(B, N, generator=g) - 0.5).round(decimals=2)
    tok_n[:, ::2] = 0.0
    return dict(tok_speed=tok_speed, tok_f0_scale=tok_f0, tok_n_shift=tok_n)


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
@pytest.mark.parametrize("pack,rate", [("s16", None), ("ulaw", 8000)])
def test_marks_end_to_end(tag, pack, rate):
    man, model, sampler = _model(tag)
    b = _batch(bool(man["config"]["multispeaker"]))
    B, N = b["tokens"].shape
    hifigan = model.decoder.kind == "hifigan"
    trim = 50 if hifigan else 0
    U, D = resample.ratio(24000 if rate is None else rate)
    ctl = pipeline.Controls(B, speed=[1.0, 0.9, 1.0], **_tok_controls(B, N))
    need = [pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, controls=c, **_kw(b))["frames_host"]
            for c in (None, ctl)]
    assert need[0] != need[1]
    T_cap = (max(max(n) for n in need) + 63) // 64 * 64
    assert T_cap <= T_SINE
    torch.cuda.synchronize()
    ops.status(clear=True)
    kw = _kw(b, sine_noise=b["sine"], max_frames=T_cap, pack=pack, sample_rate=rate)
    base = pipeline.inference(model, sampler, b["tokens"], **kw)
    assert base.marks is None
    base_rows = [r.copy() for r in base.to_host()]
    for c, frames_host in ((None, need[0]), (pipeline.Controls.neutral(B, N=N), need[0]), (ctl, need[1])):
        plain = pipeline.inference(model, sampler, b["tokens"], controls=c, **kw)
        plain_rows = [r.copy() for r in plain.to_host()]
        res = pipeline.inference(model, sampler, b["tokens"], controls=c, marks=True, **kw)
        assert res.marks.dtype == torch.int32 and tuple(res.marks.shape) == (B, N + 1) and res.marks.is_cuda
        rows, m = res.to_host(marks=True)
        assert res.frames.cpu().tolist() == frames_host
        # samples are bitwise those of the call without marks; neutral token controls are the call without them
        assert torch.equal(res.wave, plain.wave) and torch.equal(res.offsets, plain.offsets)
        assert all(np.array_equal(x, y) for x, y in zip(rows, plain_rows))
        if c is None or c.tok_present == c.TOK_NAMES and c is not ctl:
            assert torch.equal(res.wave, base.wave) and all(np.array_equal(x, y) for x, y in zip(rows, base_rows))
        assert np.array_equal(m, res.marks.cpu().numpy())
        p = pipeline.prepare(model, sampler, b["tokens"], max_frames=T_cap, controls=c, **_kw(b))
        dur = p["durations"].cpu().numpy()
        want = R.marks(dur, list(LENS), p["frames"].cpu().numpy(), T_cap, 1 if hifigan else 0, 600, trim, U, D)
        assert np.array_equal(m, want), (m.tolist(), want.tolist())
        assert [int(m[r, N]) for r in range(B)] == [len(x) for x in rows]
        assert [len(x) for x in rows] == [resample.output_samples(600 * f - trim, U, D) for f in frames_host]
        assert np.all(np.diff(m, axis=1) >= 0) and np.all(m[:, 0] == 0)
        for r, n_r in enumerate(LENS):  # every real token owns samples (the last may lose its only frame to the shift); pads own none
            assert np.all(np.diff(m[r, :n_r]) > 0) and np.all(m[r, n_r:] == m[r, N])
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_token_controls_move_what_they_say_and_nothing_else():
    man, model, sampler = _model("ljspeech")
    b = _batch(False)
    B, N = b["tokens"].shape
    tc = _tok_controls(B, N)
    p0 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))
    T_cap = (max(p0["frames_host"]) * 2 + 63) // 64 * 64
    q0 = pipeline.prepare(model, sampler, b["tokens"], max_frames=T_cap, **_kw(b))
    q1 = pipeline.prepare(model, sampler, b["tokens"], max_frames=T_cap, controls=pipeline.Controls(B, **tc), **_kw(b))
    d0, d1 = q0["durations"].cpu(), q1["durations"].cpu()
    changed = tc["tok_speed"] != 1.0
    for r, n_r in enumerate(LENS):
        changed[r, n_r:] = False
    assert torch.equal(d1[~changed], d0[~changed]) and bool((d1[0, 2:5] > d0[0, 2:5]).all()) and int(d1[1, 1]) <= int(d0[1, 1])
    assert torch.equal(q1["s_pred"], q0["s_pred"])
    # pitch and energy alone: the durations, the frames and asr keep their bits; F0 / N are the expansion of the token rows
    q2 = pipeline.prepare(model, sampler, b["tokens"], max_frames=T_cap,
                          controls=pipeline.Controls(B, tok_f0_scale=tc["tok_f0_scale"], tok_n_shift=tc["tok_n_shift"]), **_kw(b))
    assert torch.equal(q2["durations"], q0["durations"]) and torch.equal(q2["frames"], q0["frames"]) and torch.equal(q2["asr"], q0["asr"])
    shift = 1 if model.decoder.kind == "hifigan" else 0
    wf, wn = R.prosody_tok(q0["F0"].cpu().numpy(), q0["N"].cpu().numpy(), d0.numpy(), shift, tc["tok_f0_scale"].numpy(),
                           tc["tok_n_shift"].numpy(), q0["frames"].cpu().tolist())
    assert np.array_equal(q2["F0"].cpu().numpy().view(np.uint32), wf.view(np.uint32))
    assert np.array_equal(q2["N"].cpu().numpy().view(np.uint32), wn.view(np.uint32))
    assert not torch.equal(q2["F0"], q0["F0"]) and not torch.equal(q2["N"], q0["N"])
    with pytest.raises(ValueError, match="nothing to scale"):
        pipeline.inference(model, sampler, b["tokens"], max_frames=T_cap, durations=q0["durations"],
                           controls=pipeline.Controls(B, tok_speed=tc["tok_speed"]), **_kw(b))
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_with_marks_serves_any_lengths_and_token_controls():
    man, model, sampler = _model("ljspeech")
    b = _batch(False)
    B, N = b["tokens"].shape
    ld = b["lengths"].to(torch.int32).to(DEV)
    tc = _tok_controls(B, N)
    other = dict(tok_speed=tc["tok_speed"].flip(0).contiguous(), tok_n_shift=tc["tok_n_shift"].flip(1).contiguous())
    lens2 = torch.tensor([10, 9, 5], dtype=torch.int32, device=DEV)
    p0 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))
    T_cap = (max(p0["frames_host"]) * 2 + 63) // 64 * 64
    assert T_cap <= T_SINE
    out = dict(pack="ulaw", sample_rate=8000)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS, marks=True, **out)
    assert gs.static["controls"].tok_present == pipeline.Controls.TOK_NAMES
    records = []
    orig = gs._record
    gs._record = lambda: records.append(1) or orig()
    torch.cuda.synchronize()
    ops.status(clear=True)
    first = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    eager_kw = dict(noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"], diffusion_steps=STEPS, max_frames=T_cap,
                    marks=True, **out)
    cases = [(None, ld), (pipeline.Controls(B, speed=[1.0, 0.9, 1.1], **tc), ld), (pipeline.Controls(B, **other), lens2),
             (pipeline.Controls(B, f0_scale=1.25), lens2), (None, ld)]
    seen = []
    for i, (ctl, lens) in enumerate(cases):
        res = gs(controls=ctl, **dict(first if i == 0 else {}, lengths=lens))
        torch.cuda.synchronize()
        eager = pipeline.inference(model, sampler, b["tokens"], controls=ctl, lengths_dev=lens, **eager_kw)
        torch.cuda.synchronize()
        assert torch.equal(res.frames, eager.frames) and torch.equal(res.wave, eager.wave), "replay %d" % i
        assert torch.equal(res.marks, eager.marks) and torch.equal(res.offsets, eager.offsets), "replay %d" % i
        n_tot = int(eager.offsets[-1])
        assert torch.equal(res.packed[:n_tot], eager.packed[:n_tot])
        rows, m = res.to_host(marks=True)
        assert [int(m[r, N]) for r in range(B)] == [len(x) for x in rows]
        seen.append(m.copy())
    assert len(records) == 1, "other lengths and other token controls never re-record"
    assert np.array_equal(seen[0], seen[4]) and not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert ops.status() & CAPACITY_BITS == 0
    # a row slowed past the capacity: truncated and reported; the other rows keep their bits and their marks
    fit_ctl = dict(tok_speed=torch.ones(B, N), tok_f0_scale=tc["tok_f0_scale"])
    fit = gs(controls=pipeline.Controls(B, **fit_ctl), lengths=ld)
    torch.cuda.synchronize()
    fit_wave, fit_marks, fit_frames = fit.wave.clone(), fit.marks.clone(), fit.frames.cpu().tolist()
    assert ops.status() & CAPACITY_BITS == 0 and 4 * fit_frames[0] > T_cap + 4 * 5  # the unscaled +5 tail counts once
    slow = torch.ones(B, N)
    slow[0] = 0.25
    over = gs(controls=pipeline.Controls(B, tok_speed=slow, tok_f0_scale=tc["tok_f0_scale"]), lengths=ld)
    torch.cuda.synchronize()
    assert ops.status() & _lib.STATUS_FRAME_CAPACITY, hex(ops.status())
    assert over.frames.cpu().tolist() == [T_cap] + fit_frames[1:]
    for r in (1, 2):
        assert torch.equal(over.wave[r], fit_wave[r]) and torch.equal(over.marks[r], fit_marks[r]), "row %d" % r
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows, m = over.to_host(marks=True)
    assert any("FRAME_CAPACITY" in str(w.message) for w in caught)
    hifigan = model.decoder.kind == "hifigan"
    trim = 50 if hifigan else 0
    n0 = resample.output_samples(600 * T_cap - trim, *resample.ratio(8000))
    assert len(rows[0]) == n0 == m[0, N] and np.all(np.diff(m[0]) >= 0)
    p = pipeline.prepare(model, sampler, b["tokens"], max_frames=T_cap, lengths_dev=ld,
                         controls=pipeline.Controls(B, tok_speed=slow, tok_f0_scale=tc["tok_f0_scale"]), noise=b["noise"],
                         step_noise=b["step_noise"], diffusion_steps=STEPS)
    torch.cuda.synchronize()
    want = R.marks(p["durations"].cpu().numpy(), list(LENS), p["frames"].cpu().numpy(), T_cap, 1 if hifigan else 0, 600, trim,
                   *resample.ratio(8000))
    assert np.array_equal(m, want)
    with pytest.raises(ValueError, match="token_controls"):
        pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS)(controls=pipeline.Controls(B, **tc))
    with pytest.raises(ValueError, match="wide"):
        gs(controls=pipeline.Controls(B, N=N + 1))  # token rows of another width, even with none of them set
    ops.status(clear=True)
    assert len(records) == 1
