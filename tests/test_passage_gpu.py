"""Passages on the sync-free path: `st2_wave_pack_gaps` against the numpy contract of
tests/_passage_ref.py, byte for byte, then the `passage=` / `gaps=` paths of `inference`, `GraphedSynthesis` and
`synthesize_long(max_frames=)` against the paths that existed before them.  Every comparison is integer- or byte-exact except
where a different conv path may be picked (another frame capacity, another B): there the project's bar between conv-path
variants, 1e-6 * max(rms, 1), holds.  Shapes are tiny: rows of at most 8 frames for the kernel, the seeded test models and
four sentences of 7-12 tokens end to end."""
import functools

import numpy as np
import pytest
import torch

import _passage_ref as R
from _util import rms
from styletts2_amd import ops, pipeline, resample
from test_controls_gpu import CAPACITY_BITS, STEPS, T_SINE, _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = {"f32": 7.5, "s16": 0x5A5A, "ulaw": 0x5A, "alaw": 0x5A}  # differs from every format's silence code
TORCH_DT = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}
GAP_CAP = 37


# ---- 1. the kernel against the numpy contract -------------------------------------------------------------------------------------
def _rows_of(packed, offs):
    p, o = packed.cpu().numpy(), offs.cpu().tolist()
    return [p[o[b]:o[b + 1]].copy() for b in range(len(o) - 1)]


def _speech(wave, frames, rate, fmt, trim, spf):
    """Every row's speech as the wrapped entry hands it over (the contract's definition of those bytes), with its offsets."""
    if rate is None:
        packed, offs = ops.wave_pack(wave, frames, trim=trim, fmt=fmt, samples_per_frame=spf)
    else:
        packed, offs = ops.wave_resample_pack(wave, frames, rate, fmt=fmt, trim=trim, samples_per_frame=spf)
    return packed, offs


def _case(B, spf, T_cap, trim, seed):
    g = np.random.default_rng(seed)
    frames = g.integers(0, T_cap + 1, size=B).astype(np.int32)
    frames[0] = T_cap
    if B > 2:
        frames[1], frames[2] = 0, T_cap + 2  # a row of no samples (followed by a gap); a count over the capacity
    wave = (g.standard_normal((B, spf * T_cap)) * 0.6).astype(np.float32)
    for b in range(B):
        wave[b, spf * min(max(int(frames[b]), 0), T_cap):] = np.nan  # the ragged decoder's tails may hold anything
    return torch.from_numpy(wave).to(DEV), torch.from_numpy(frames).to(DEV)


def _run_gaps(wave, frames, gaps, rate, fmt, trim, spf, rows, cap=None, shift=0):
    """One call into a sentinel-filled buffer that starts `shift` elements behind a 16-byte boundary; everything below the limit
    must equal the reference, nothing at or past it may have changed.  -> the destination residues (mod 16 bytes) of the gaps."""
    B = wave.shape[0]
    want, woff, limit = R.pack_gaps(rows, gaps, GAP_CAP, fmt, cap)
    dt = TORCH_DT[fmt]
    room = int(woff[-1]) + 40 if cap is None else cap
    whole = torch.full((shift + room + 64,), SENTINEL[fmt], dtype=dt, device=DEV)
    out = whole[shift:shift + room]
    gd = None if gaps is None else torch.tensor(gaps, dtype=torch.int32, device=DEV)
    packed, offs = ops.wave_pack_gaps(wave, frames, gd, GAP_CAP, rate=rate, fmt=fmt, trim=trim, out=out, samples_per_frame=spf)
    assert packed.data_ptr() == out.data_ptr() and offs.dtype == torch.int64
    assert offs.cpu().tolist() == woff.tolist(), (B, spf, trim, gaps)
    got = whole.cpu().numpy()
    assert got[shift:shift + limit].tobytes() == want.tobytes(), (B, spf, trim, cap, shift)
    rest = np.concatenate([got[:shift], got[shift + limit:]])
    assert rest.tobytes() == np.full(rest.shape, SENTINEL[fmt], dtype=rest.dtype).tobytes(), "written at or past the limit"
    size = dt.itemsize
    g = R.clamp_gaps(gaps, GAP_CAP, B)
    return {(out.data_ptr() + size * (int(woff[b + 1]) - g[b])) % 16 for b in range(B) if g[b] > 0}


@pytest.mark.parametrize("rate", [None, 24000, 8000, 44100])
@pytest.mark.parametrize("fmt", ["f32", "s16", "ulaw", "alaw"])
def test_wave_pack_gaps_equals_the_numpy_contract(fmt, rate):
    if rate is None and fmt not in ops.PACK_FORMATS:
        with pytest.raises(ValueError):  # the plain move serves fp32 and 16-bit PCM; G.711 at 24 kHz is the rate = 24000 case
            ops.wave_pack_gaps(torch.zeros(1, 5, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), None, 0, fmt=fmt,
                               samples_per_frame=5)
        return
    T_cap = 8
    residues, lengths = set(), set()
    for B in (1, 5, 17):
        for spf in (5, 600):
            for trim in (0, 3):
                wave, frames = _case(B, spf, T_cap, trim, 1000 * B + spf + trim)
                packed0, offs0 = _speech(wave, frames, rate, fmt, trim, spf)
                rows = _rows_of(packed0, offs0)
                m = [len(r) for r in rows]
                for rnd in range(3):  # gap lengths 0 .. 50 over the rounds: 0 .. 33, and everything above 37 clamps to gap_cap
                    gaps = [(b + 17 * rnd + 5 * (B == 1)) for b in range(B)]
                    if B == 5:
                        gaps[3] = -4 - rnd  # negative: no gap
                    g = R.clamp_gaps(gaps, GAP_CAP, B)
                    lengths |= set(g)
                    residues |= _run_gaps(wave, frames, gaps, rate, fmt, trim, spf, rows, shift=rnd + (spf == 5))
                    off = R.offsets(m, gaps, GAP_CAP)
                    in_row = [b for b in range(B) if m[b] >= 2]
                    in_gap = [b for b in range(B) if g[b] >= 2]
                    if in_row:  # the limit inside a row
                        b = in_row[len(in_row) // 2]
                        _run_gaps(wave, frames, gaps, rate, fmt, trim, spf, rows, cap=int(off[b]) + m[b] // 2, shift=1)
                    if in_gap:  # the limit inside a gap
                        b = in_gap[len(in_gap) // 2]
                        _run_gaps(wave, frames, gaps, rate, fmt, trim, spf, rows, cap=int(off[b]) + m[b] + g[b] // 2, shift=2)
                # gaps = None: the wrapped entry, byte for byte, out and offsets
                packed1, offs1 = ops.wave_pack_gaps(wave, frames, None, GAP_CAP, rate=rate, fmt=fmt, trim=trim, samples_per_frame=spf)
                total = int(offs0[-1])
                assert torch.equal(offs1, offs0) and torch.equal(packed1[:total], packed0[:total])
                _run_gaps(wave, frames, None, rate, fmt, trim, spf, rows)
    size = TORCH_DT[fmt].itemsize
    assert residues == set(range(0, 16, size)), "gap starts must cover every residue mod 16 bytes: %s" % sorted(residues)
    assert set(range(34)) | {GAP_CAP} <= lengths, sorted(lengths)
    torch.cuda.synchronize()
    assert ops.status() == 0


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------
LENS4 = (12, 9, 7, 10)
K = len(LENS4)


@functools.lru_cache(maxsize=None)
def _passage(tag):
    """The K-sentence passage of a tag once: the model, the pinned draws, the parent's long-form result (one ragged front group)
    and the frame counts read from it."""
    man, model, sampler = _model(tag)
    multi = bool(man["config"]["multispeaker"])
    b = _batch(multi, LENS4)
    sentences = [b["tokens"][k, :LENS4[k]].clone() for k in range(K)]
    ref_s = b["ref_s"][:1] if multi else None
    noises = [b["noise"][k:k + 1] for k in range(K)]
    step_noises = [b["step_noise"][:, k:k + 1].contiguous() for k in range(K)]
    sines = [b["sine"][k:k + 1] for k in range(K)]
    torch.cuda.synchronize()
    ops.status(clear=True)
    waves, s_last = pipeline.synthesize_long(model, sampler, sentences, ref_s=ref_s, diffusion_steps=STEPS, noises=noises,
                                             step_noises=step_noises, sine_noises=sines, front_batch=0, overlap=False,
                                             ragged_decode=True, trim=0)
    torch.cuda.synchronize()
    frames = [w.numel() // 600 for w in waves]
    assert all(w.numel() == 600 * f for w, f in zip(waves, frames)) and len(set(frames)) > 1 and max(frames) <= T_SINE
    trim = 50 if model.decoder.kind == "hifigan" else 0
    kw = dict(input_lengths=b["lengths"], noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"], diffusion_steps=STEPS,
              ref_s=None if ref_s is None else ref_s.expand(K, -1).contiguous(), lj_tail=False, trim=trim)
    return dict(model=model, sampler=sampler, b=b, sentences=sentences, ref_s=ref_s, noises=noises, step_noises=step_noises,
                sines=sines, waves=waves, s_last=s_last, frames=frames, T=max(frames), trim=trim, kw=kw)


def _repack(P, pack, rate):
    """The parent's waveforms through the same packing step."""
    T = P["T"]
    w = torch.zeros((K, 1, 600 * T), device=DEV)
    for k in range(K):
        w[k, 0, :600 * P["frames"][k]] = P["waves"][k]
    f = torch.tensor(P["frames"], dtype=torch.int32, device=DEV)
    if pipeline._resamples(pack, rate):
        return ops.wave_resample_pack(w, f, 24000 if rate is None else rate, fmt=pack, trim=P["trim"])
    return ops.wave_pack(w, f, trim=P["trim"], fmt=pack)


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
@pytest.mark.parametrize("pack,rate", [("s16", None), ("ulaw", 8000)])
def test_passage_equals_the_long_form_path_and_gaps_leave_the_speech_alone(tag, pack, rate):
    P = _passage(tag)
    model, sampler, b = P["model"], P["sampler"], P["b"]
    out = dict(pack=pack, sample_rate=rate)
    res = pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], passage=True, marks=True, **out, **P["kw"])
    torch.cuda.synchronize()
    want_packed, want_offs = _repack(P, pack, rate)
    total = int(want_offs[-1])
    assert res.frames.cpu().tolist() == P["frames"]
    assert torch.equal(res.offsets, want_offs) and torch.equal(res.packed[:total], want_packed[:total]), "bit-equal to the parent"
    assert tuple(res.style.shape) == (K, 256) and torch.equal(res.style[-1:], P["s_last"]) and res.gaps is None
    rows = [r.copy() for r in res.to_host()]
    # the capacity rounded up to the next multiple of 64: another conv geometry, the conv-path bar
    T64 = (P["T"] + 63) // 64 * 64
    r64 = pipeline.inference(model, sampler, b["tokens"], max_frames=T64, passage=True, **P["kw"])
    assert r64.frames.cpu().tolist() == P["frames"] and torch.equal(r64.style, res.style)
    for k in range(K):
        a, ref = r64.wave[k, 0, :600 * P["frames"][k]].cpu(), P["waves"][k].cpu()
        err, bar = rms(a - ref), 1e-6 * max(rms(ref), 1.0)
        print("row %d at max_frames %d: rms error %.3g (bar %.3g)" % (k, T64, err, bar))
        assert err <= bar, (k, err, bar)
    # with gaps: the speech bytes are unchanged, the gap bytes are cvt(0), the offsets add up with the marks
    hz = 24000 if rate is None else rate
    gaps = pipeline.gap_samples([250, 0, 1.0, 33.4], hz)
    assert gaps == [R.gap_samples(v, hz) for v in (250, 0, 1.0, 33.4)] and gaps[1] == 0
    rg = pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], passage=True, marks=True, gaps=gaps, **out, **P["kw"])
    assert rg.max_gap == max(gaps) and rg.gaps.cpu().tolist() == gaps and torch.equal(rg.wave, res.wave)
    whole = rg.to_host(passage=True).copy()
    rows_g, m = rg.to_host(marks=True)
    offs = rg.offsets.cpu().tolist()
    N = b["tokens"].shape[1]
    assert len(whole) == offs[K] == sum(len(r) for r in rows) + sum(gaps)
    z = R.silence(pack)
    for k in range(K):
        assert np.array_equal(rows_g[k], rows[k]), "speech of row %d" % k
        assert offs[k + 1] - offs[k] == int(m[k, N]) + gaps[k] and int(m[k, N]) == len(rows[k])
        assert whole[offs[k]:offs[k] + len(rows[k])].tobytes() == rows[k].tobytes()
        gap = whole[offs[k] + len(rows[k]):offs[k + 1]]
        assert len(gap) == gaps[k] and gap.tobytes() == np.full(gaps[k], z, dtype=gap.dtype).tobytes()
    assert np.array_equal(m, res.marks.cpu().numpy()), "marks stay row-relative"
    want, woff, _ = R.pack_gaps(rows, gaps, max(gaps), pack)
    assert whole.tobytes() == want.tobytes() and offs == woff.tolist()
    # a device tensor of gaps is clamped where it is read, never on the host
    gd = torch.tensor([5, -3, 10 ** 6, 7], dtype=torch.int32, device=DEV)
    rd = pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], passage=True, gaps=gd, max_gap=9, **out, **P["kw"])
    want, woff, _ = R.pack_gaps(rows, [5, -3, 10 ** 6, 7], 9, pack)
    assert rd.to_host(passage=True).tobytes() == want.tobytes() and rd.offsets.cpu().tolist() == woff.tolist()
    assert all(np.array_equal(x, y) for x, y in zip(rd.to_host(), rows))
    with pytest.raises(ValueError, match="max_gap"):
        pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], passage=True, gaps=gd, **out, **P["kw"])
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def _sub(P, i, j, **more):
    """inference() keywords for the rows i .. j-1 of the passage's batch."""
    b = P["b"]
    kw = dict(P["kw"], input_lengths=b["lengths"][i:j], noise=b["noise"][i:j], step_noise=b["step_noise"][:, i:j].contiguous(),
              sine_noise=b["sine"][i:j], ref_s=None if P["kw"]["ref_s"] is None else P["kw"]["ref_s"][i:j])
    kw.update(more)
    return b["tokens"][i:j], kw


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_start_flags_and_continuation(tag):
    P = _passage(tag)
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T = P["T"]
    one = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=True, **P["kw"])
    # two passages of two sentences in one batch == two calls
    both = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=[1, 0, 1, 0], **P["kw"])
    flags_dev = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=DEV)
    both_dev = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=flags_dev, **P["kw"])
    assert torch.equal(both_dev.style, both.style) and torch.equal(both_dev.wave, both.wave)
    for i in (0, 2):
        tk, kw = _sub(P, i, i + 2)
        part = pipeline.inference(model, sampler, tk, max_frames=T, passage=True, **kw)
        assert torch.equal(both.style[i:i + 2], part.style), "rows %d-%d: style" % (i, i + 1)
        assert both.frames[i:i + 2].cpu().tolist() == part.frames.cpu().tolist()
        for r in range(2):
            n = 600 * int(part.frames[r])
            a, ref = both.wave[i + r, 0, :n].cpu(), part.wave[r, 0, :n].cpu()
            err, bar = rms(a - ref), 1e-6 * max(rms(ref), 1.0)
            print("row %d of B = 4 against B = 2: rms error %.3g (bar %.3g)" % (i + r, err, bar))
            assert err <= bar
    assert torch.equal(both.style[:2], one.style[:2]) and not torch.equal(both.style[2:], one.style[2:])
    # continuation: rows 0-1, then rows 2-3 from style[-1:]
    tk, kw = _sub(P, 0, 2)
    first = pipeline.inference(model, sampler, tk, max_frames=T, passage=True, **kw)
    tk, kw = _sub(P, 2, 4)
    second = pipeline.inference(model, sampler, tk, max_frames=T, passage=True, s_prev=first.style[-1:], **kw)
    assert torch.equal(torch.cat([first.style, second.style]), one.style), "the continued passage is the one-call passage"
    # flags all zero with s_prev None: row 0 still has no previous; all ones: no carry at all
    none = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=[0, 0, 0, 0], **P["kw"])
    assert torch.equal(none.style, one.style)
    solo = pipeline.inference(model, sampler, b["tokens"], max_frames=T, **P["kw"])
    ones = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=[1, 1, 1, 1], **P["kw"])
    assert torch.equal(ones.style, solo.style) and not torch.equal(solo.style[1:], one.style[1:])
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_gaps_start_flags_and_s_prev():
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T, N = P["T"], b["tokens"].shape[1]
    out = dict(pack="ulaw", sample_rate=8000)
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, passage=True,
                                   max_gap=300, **out)
    assert gs.static["starts"].cpu().tolist() == [1, 0, 0, 0] and gs.static["gaps"].cpu().tolist() == [0] * K
    ld = b["lengths"].to(torch.int32).to(DEV)
    eager_kw = dict(P["kw"], input_lengths=None, lengths_dev=ld, max_frames=T, **out)
    s_other = (torch.randn(1, 256, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    res = gs(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    graph = gs._g["graph"]
    cases = [(None, None, None, dict(passage=[1, 0, 0, 0], gaps=[0] * K, s_prev=torch.zeros(1, 256, device=DEV))),
             ([120, 0, 300, 7], [0, 0, 1, 0], s_other, None),
             (torch.tensor([1, 2, 400, -5], dtype=torch.int32, device=DEV), torch.tensor([1, 1, 0, 0], device=DEV), None, None)]
    gaps_now, starts_now, prev_now = [0] * K, [1, 0, 0, 0], torch.zeros(1, 256, device=DEV)
    for i, (gaps, starts, s_prev, _) in enumerate(cases):
        if i:
            res = gs(gaps=gaps, starts=starts, s_prev=s_prev)
        torch.cuda.synchronize()
        gaps_now = gaps_now if gaps is None else (gaps.cpu().tolist() if torch.is_tensor(gaps) else gaps)
        starts_now = starts_now if starts is None else (starts.cpu().tolist() if torch.is_tensor(starts) else starts)
        prev_now = prev_now if s_prev is None else s_prev
        eager = pipeline.inference(model, sampler, b["tokens"], passage=starts_now, s_prev=prev_now,
                                   gaps=torch.tensor(gaps_now, dtype=torch.int32, device=DEV), max_gap=300, **eager_kw)
        torch.cuda.synchronize()
        assert torch.equal(res.frames, eager.frames) and torch.equal(res.wave, eager.wave), "replay %d" % i
        assert torch.equal(res.style, eager.style) and torch.equal(res.offsets, eager.offsets), "replay %d" % i
        total = int(eager.offsets[-1])
        assert torch.equal(res.packed[:total], eager.packed[:total]) and torch.equal(res.gaps, eager.gaps), "replay %d" % i
        g = R.clamp_gaps(gaps_now, 300, K)
        rows = res.to_host()
        offs = res.offsets.cpu().tolist()
        assert [offs[k + 1] - offs[k] - len(rows[k]) for k in range(K)] == g
        assert gs._g["graph"] is graph, "no re-record"
    # row 0's start flag set: whatever s_prev holds is not looked at
    a = gs(starts=[1, 0, 0, 0], s_prev=s_other).style.clone()
    c = gs(s_prev=torch.zeros(1, 256, device=DEV)).style.clone()
    assert torch.equal(a, c) and gs._g["graph"] is graph
    # built without passage / max_gap: the graph has no such buffers and refuses them
    plain = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, ref_s=P["ref_s"], **out)
    assert not {"starts", "s_prev", "gaps"} & set(plain.static)
    with pytest.raises(ValueError, match="built without"):
        plain(gaps=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="pack"):
        pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, max_gap=10)
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_synthesize_long_on_the_sync_free_path():
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T = P["T"]
    one = pipeline.inference(model, sampler, b["tokens"], max_frames=T, passage=True, pack="s16", marks=True, **P["kw"])
    one_rows = [r.copy() for r in one.to_host()]
    common = dict(ref_s=P["ref_s"], diffusion_steps=STEPS, noises=P["noises"], step_noises=P["step_noises"], sine_noises=P["sines"],
                  max_frames=T, pack="s16", marks=True, trim=P["trim"])
    seen = []
    results, s_last = pipeline.synthesize_long(model, sampler, P["sentences"], front_batch=2, on_chunk=lambda k, r: seen.append(k),
                                               gaps=[100, 0, 55, 3], **common)
    assert len(results) == 2 and seen == [0, 1] and all(isinstance(r, pipeline.SynthesisResult) for r in results)
    assert torch.equal(torch.cat([r.style for r in results]), one.style), "the groups' styles are the one-call passage's"
    assert torch.equal(s_last, one.style[-1:])
    assert [r.gaps.cpu().tolist() for r in results] == [[100, 0], [55, 3]] and all(r.marks is not None for r in results)
    assert torch.cat([r.frames for r in results]).cpu().tolist() == P["frames"]
    got = [x for r in results for x in r.to_host()]
    assert [len(x) for x in got] == [len(x) for x in one_rows]
    # a per-token rate row of the longest sentence's width: runs, and slows what it says
    N = max(LENS4)
    tok = torch.ones(K, N)
    tok[1, 2:5] = 0.5
    slow, _ = pipeline.synthesize_long(model, sampler, P["sentences"], front_batch=2, controls=pipeline.Controls(K, tok_speed=tok),
                                       **dict(common, max_frames=2 * T))
    f = torch.cat([r.frames for r in slow]).cpu().tolist()
    assert f[0] == P["frames"][0] and f[1] > P["frames"][1]
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()
