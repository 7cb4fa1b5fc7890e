"""`st2_wave_resample_pack` on the device against the fp64 contract of tests/_resample_ref.py, and its
place in the pipeline: `inference(pack=, sample_rate=)` and `GraphedSynthesis` from tokens to telephony bytes in one graph.

The tolerance is derived, not tuned: fp32 fmaf accumulation of K terms differs from the exact sum by at most
(K + 1) 2^-24 sum_k |taps x|, which the reference computes per sample; 16-bit samples may differ by that times 32767 plus the
half unit of the rounding; a G.711 byte must be the code of some 16-bit value in that interval.  No sample is excluded."""
import functools

import numpy as np
import pytest
import torch

import _resample_ref as R
import _syncfree_ref as S
from styletts2_amd import models, ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPF, T_CAP, FRAMES = 600, 8, [0, 1, 3, 8, 8, 2]  # n_b = 0, one frame, several output tiles, two rows at capacity
NP_DTYPE = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8, "alaw": np.uint8}
SENTINEL = {"f32": -77.25, "s16": 12345, "ulaw": 0x5A, "alaw": 0x5A}
CASES = [(r, f) for r in (8000, 16000, 22050, 44100, 48000) for f in ("f32", "s16")] + [(8000, "ulaw"), (8000, "alaw")]


@functools.lru_cache(maxsize=None)
def _batch(trim):
    """The batch of the issue.  At trim = 0 everything at and past a row's n_b is NaN (no valid sample sits there: the output
    must come out finite); at trim = 50 the NaNs start behind the row's frames and the kernel is held to the reference of the
    same input.  ~5 % of the samples lie beyond +-1: the 16-bit clamp is in play."""
    g = torch.Generator().manual_seed(31 + trim)
    wave = torch.randn(len(FRAMES), SPF * T_CAP, generator=g) * 0.5
    for b, f in enumerate(FRAMES):
        wave[b, SPF * f:] = float("nan")
    return wave


@functools.lru_cache(maxsize=None)
def _reference(rate, trim):
    U, D, taps = resample.design(rate)
    y, bound, offsets = R.wave_resample(_batch(trim).numpy(), FRAMES, T_CAP, taps, U, D, SPF, trim)
    for a in (y, bound, offsets):
        a.setflags(write=False)  # shared among the tests: left unchanged
    return y, bound, offsets


def _check(got, y, bound, fmt, what):
    """got: what the kernel wrote for the samples whose reference is (y, bound)."""
    if fmt == "f32":
        err = np.abs(got.astype(np.float64) - y)
        assert (err <= bound).all(), "%s: %d samples beyond the fp32 bound, worst %g x" % (what, (err > bound).sum(),
                                                                                            (err / np.maximum(bound, 1e-300)).max())
        return
    lo, hi = R.pcm_interval(y, bound)
    if fmt == "s16":
        bad = (got < lo) | (got > hi)
    else:  # the byte is the code of some int16 in [lo, hi]: encoding is monotone, so its rank lies between the ends' ranks
        r = R.rank(got, fmt)
        bad = (r < R.rank(R.ENCODE[fmt](lo), fmt)) | (r > R.rank(R.ENCODE[fmt](hi), fmt))
    assert not bad.any(), "%s: %d samples outside their interval, first at %d" % (what, bad.sum(), int(np.argmax(bad)))


def _run(wave, frames, rate, fmt, trim, room, shift=0, cap=None):
    """The kernel into room[shift:shift + cap] (a sentinel-filled device buffer) -> (the whole buffer on the host, offsets)."""
    out = room[shift:] if cap is None else room[shift:shift + cap]
    packed, offs = ops.wave_resample_pack(wave, frames, rate, fmt=fmt, trim=trim, out=out, samples_per_frame=SPF)
    torch.cuda.synchronize()
    assert packed.data_ptr() == out.data_ptr() and offs.dtype == torch.int64
    return room.cpu().numpy(), offs.cpu().numpy()


def _room(total, fmt, extra=64):
    return torch.full((total + extra,), SENTINEL[fmt], dtype=ops.OUTPUT_FORMATS[fmt][1], device=DEV)


@pytest.mark.parametrize("trim", [0, 50])
@pytest.mark.parametrize("rate,fmt", CASES)
def test_every_rate_and_format_within_the_derived_bound(rate, fmt, trim):
    U, D, K, _ = resample.table(rate, DEV)
    y, bound, want_off = _reference(rate, trim)
    n, m = R.row_counts(FRAMES, T_CAP, SPF, trim, U, D)
    total = int(want_off[-1])
    assert n[0] == 0 and m[0] == 0 and total == sum(m)
    if trim == 0:
        assert n[1] == 600
    if rate == 8000:
        assert m[1] < K, "row 1 (%d output samples) is shorter than the table's K = %d" % (m[1], K)
    fd = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    got, offs = _run(_batch(trim).to(DEV), fd, rate, fmt, trim, _room(total, fmt))
    assert offs.tolist() == want_off.tolist()
    assert got.dtype == NP_DTYPE[fmt] and (got[total:] == NP_DTYPE[fmt](SENTINEL[fmt])).all(), "written past offsets[B]"
    if trim == 0 and fmt == "f32":
        assert np.isfinite(got[:total]).all(), "a NaN from at or past n_b reached the sum"
    _check(got[:total], y, bound, fmt, "rate %d %s trim %d" % (rate, fmt, trim))


def test_out_capacity_cuts_inside_row_3_and_offsets_stay_whole():
    rate, fmt, trim = 16000, "s16", 0
    y, bound, want_off = _reference(rate, trim)
    total = int(want_off[-1])
    cap = int(want_off[3]) + int(want_off[4] - want_off[3]) // 2 + 3  # inside row 3, on no vector boundary
    assert want_off[3] < cap < want_off[4]
    fd = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    got, offs = _run(_batch(trim).to(DEV), fd, rate, fmt, trim, _room(total, fmt), cap=cap)
    assert offs.tolist() == want_off.tolist(), "offsets describe the untruncated layout"
    assert (got[cap:] == SENTINEL[fmt]).all(), "something at or past min(offsets[B], out_capacity) changed"
    _check(got[:cap], y[:cap], bound[:cap], fmt, "truncated at %d" % cap)


@pytest.mark.parametrize("rate,fmt,shift", [(8000, "ulaw", 5), (48000, "s16", 3), (22050, "f32", 1)])
def test_an_offset_out_pointer_peels_a_head(rate, fmt, shift):
    trim = 50
    y, bound, want_off = _reference(rate, trim)
    total = int(want_off[-1])
    room = _room(total + shift, fmt)
    assert (room.data_ptr() + shift * room.element_size()) % 16 != 0, "the first row's head peel is non-empty"
    fd = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    got, offs = _run(_batch(trim).to(DEV), fd, rate, fmt, trim, room, shift=shift)
    assert offs.tolist() == want_off.tolist()
    assert (got[:shift] == NP_DTYPE[fmt](SENTINEL[fmt])).all() and (got[shift + total:] == NP_DTYPE[fmt](SENTINEL[fmt])).all()
    _check(got[shift:shift + total], y, bound, fmt, "rate %d %s shift %d" % (rate, fmt, shift))


@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_24000_is_bitwise_wave_pack(fmt):
    trim = 50
    wave = _batch(trim).to(DEV)
    fd = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    want, want_off = ops.wave_pack(wave, fd, trim=trim, fmt=fmt, samples_per_frame=SPF)
    got, offs = ops.wave_resample_pack(wave, fd, 24000, fmt=fmt, trim=trim, samples_per_frame=SPF)
    torch.cuda.synchronize()
    total = int(want_off[-1])
    assert total > 0 and torch.equal(offs, want_off) and got.dtype == want.dtype
    bits = torch.int32 if fmt == "f32" else torch.int16
    assert torch.equal(got[:total].view(bits), want[:total].view(bits))


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_24000_g711_is_exact_for_all_65536_codes(law):
    T_cap = 110  # one row of 66 000 samples: all 65 536 16-bit values, v / 32767, then zeros; 17 output tiles
    v = np.arange(-32768, 32768, dtype=np.int64)
    x = np.zeros(SPF * T_cap, dtype=np.float32)
    x[:v.size] = (v / 32767.0).astype(np.float32)
    want = R.ENCODE[law](S.pcm16(x).astype(np.int64))
    assert (S.pcm16(x)[:v.size] == np.maximum(v, -32767)).all()  # every value is met (-32768 clamps to -32767)
    fd = torch.tensor([T_cap], dtype=torch.int32, device=DEV)
    got, offs = ops.wave_resample_pack(torch.from_numpy(x).to(DEV).unsqueeze(0), fd, 24000, fmt=law, samples_per_frame=SPF)
    torch.cuda.synchronize()
    assert offs.tolist() == [0, x.size] and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("rate,fmt", [(22050, "s16"), (16000, "ulaw"), (44100, "f32")])
def test_two_calls_agree_bitwise_and_a_row_does_not_depend_on_its_place(rate, fmt):
    trim = 50
    frames = [8, 1, 3, 8, 2, 8]
    wave = _batch(trim).clone()
    wave[0], wave[5] = wave[3], wave[3]  # the same 8-frame row at b = 0 and at b = 5: other offsets, other alignment
    wave, fd = wave.to(DEV), torch.tensor(frames, dtype=torch.int32, device=DEV)
    a, offs = ops.wave_resample_pack(wave, fd, rate, fmt=fmt, trim=trim, samples_per_frame=SPF)
    b, offs_b = ops.wave_resample_pack(wave, fd, rate, fmt=fmt, trim=trim, samples_per_frame=SPF)
    torch.cuda.synchronize()
    o = offs.tolist()
    bits = {"f32": torch.int32, "s16": torch.int16}.get(fmt, torch.uint8)
    assert torch.equal(offs, offs_b) and torch.equal(a[:o[-1]].view(bits), b[:o[-1]].view(bits))
    assert o[1] - o[0] == o[6] - o[5] > 0 and (o[5] * a.element_size()) % 16 != 0
    assert torch.equal(a[o[0]:o[1]].view(bits), a[o[5]:o[6]].view(bits)), "row 0 and row 5 hold the same samples"


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthesis():
    """The small seeded LJSpeech model of tests/test_syncfree_gpu.py on the device, two right-padded two-row batches of
    validation text and a frame capacity above everything they need (from one host-read run each)."""
    from test_syncfree_gpu import KEYS, STEPS, _model, _val_rows
    man, model, sds = _model("ljspeech")
    for k in KEYS:
        model[k].to(DEV)
    sampler = models.make_sampler(model)
    sets = [_val_rows([3, 4], False, seed=11), _val_rows([6, 3], False, seed=12)]
    N = max(t.shape[1] for t, *_ in sets)
    need = []
    for tokens, lengths, noise, lens, step_noise, _ in sets:
        p = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), diffusion_steps=STEPS,
                             step_noise=step_noise.to(DEV), allow_ragged=True)
        need.append(p["durations"].sum(dim=1).tolist())
    T_cap = (max(max(n) for n in need) + 64) // 64 * 64
    return model, sampler, sets, N, T_cap, need, STEPS


def _replays(gs, sets, N, T_cap, need, steps, model, sampler):
    """Every batch of `sets` through the graph -> (result, the eager `inference(max_frames=)` run on the same static buffers)."""
    g = torch.Generator().manual_seed(5)
    for i, (tokens, lengths, noise, lens, step_noise, _) in enumerate(sets):
        tk = torch.zeros(2, N, dtype=torch.long)
        tk[:, :tokens.shape[1]] = tokens
        sine = torch.randn(2, 600 * T_cap, 9, generator=g)
        res = gs(tokens=tk, lengths=lengths.to(torch.int32), noise=noise, step_noise=step_noise, sine_noise=sine)
        torch.cuda.synchronize()
        st = gs.static
        eager = pipeline.inference(model, sampler, st["tokens"], noise=st["noise"], step_noise=st["step_noise"],
                                   sine_noise=st["sine_noise"], lengths_dev=st["lengths_dev"], diffusion_steps=steps,
                                   max_frames=T_cap)
        torch.cuda.synchronize()
        assert eager.frames.cpu().tolist() == need[i] and torch.equal(res.wave, eager.wave), "replay %d" % i
        yield res, eager


def test_one_graph_from_tokens_to_8_khz_mu_law():
    model, sampler, sets, N, T_cap, need, steps = _synthesis()
    gs = pipeline.GraphedSynthesis(model, sampler, 2, N, T_cap, steps, pack="ulaw", sample_rate=8000)
    recorded = None
    for res, eager in _replays(gs, sets, N, T_cap, need, steps, model, sampler):
        assert res.sample_rate == 8000 and res.pack == "ulaw" and res.packed.dtype == torch.uint8
        assert recorded is None or gs._g is recorded, "other tokens and lengths replay the same graph"
        recorded = gs._g
        want, want_off = ops.wave_resample_pack(eager.wave, eager.frames, 8000, fmt="ulaw", trim=res.trim)
        torch.cuda.synchronize()
        assert torch.equal(res.offsets, want_off)
        o = want_off.tolist()
        rows = res.to_host()
        for b, fr in enumerate(eager.frames.cpu().tolist()):
            m_b = resample.output_samples(max(0, 600 * fr - res.trim), 1, 3)
            assert rows[b].dtype == np.uint8 and len(rows[b]) == m_b == o[b + 1] - o[b]
            assert np.array_equal(rows[b], want[o[b]:o[b + 1]].cpu().numpy()), "row %d" % b


def test_the_default_graph_is_still_wave_pack_bit_for_bit():
    model, sampler, sets, N, T_cap, need, steps = _synthesis()
    gs = pipeline.GraphedSynthesis(model, sampler, 2, N, T_cap, steps, pack="s16")
    for res, eager in _replays(gs, sets[:1], N, T_cap, need, steps, model, sampler):
        assert res.sample_rate == 24000 and res.packed.dtype == torch.int16
        want, want_off = ops.wave_pack(eager.wave, eager.frames, trim=res.trim, fmt="s16")
        torch.cuda.synchronize()
        total = int(want_off[-1])
        assert total == sum(600 * f - res.trim for f in need[0])
        assert torch.equal(res.offsets, want_off) and torch.equal(res.packed[:total], want[:total])
        rows = res.to_host()
        assert [len(r) for r in rows] == [600 * f - res.trim for f in need[0]] and rows[0].dtype == np.int16
