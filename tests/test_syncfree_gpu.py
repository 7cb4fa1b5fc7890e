"""The sync-free path on the device: device frame counts, packed PCM, the capacity-bound pipeline and
its one-graph form, against the contracts of tests/_syncfree_ref.py, the parent path `inference(ragged_decode=True)` and the
oracle.  Every test runs once."""
import numpy as np
import pytest
import torch

import _syncfree_ref as R
from _util import WAVE_RMS_TOL, manifest, rms
from oracle import st2_oracle as O
from benchdata import synth  # seeded synthetic weights (test + bench helper, not product code)
from styletts2_amd import _lib, models, ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPACITY_BITS = _lib.STATUS_FRAME_CAPACITY | _lib.STATUS_DURATION_SUM  # what a truncated row raises
KEYS = ["decoder", "diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]
STEPS = 5


# ---- 1. frames kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,with_len", [(1, 512, False), (1, 37, True), (32, 512, True), (32, 183, False)])
def test_frames_from_durations_equals_integer_sums_and_reports_capacity(B, N, with_len):
    torch.cuda.synchronize()
    ops.status(clear=True)
    g = torch.Generator().manual_seed(1000 + B + N)
    dur = torch.randint(0, 51, (B, N), generator=g)
    lengths = torch.randint(1, N + 1, (B,), generator=g).to(torch.int32) if with_len else None
    if with_len:
        lengths[0] = N
    tot = R.frames_from_durations(dur, lengths, 1 << 30)[0]
    T_cap = int(tot.max())  # every row fits
    want, over = R.frames_from_durations(dur, lengths, T_cap)
    assert not bool(over.any())
    ld = None if lengths is None else lengths.to(DEV)
    got = ops.frames_from_durations(dur.to(DEV), ld, T_cap)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    assert ops.status() & _lib.STATUS_FRAME_CAPACITY == 0, "every row fits: the bit stays clear"
    # one row over capacity: clamped to T_cap, the bit is raised, and cleared by st2_status(clear)
    row = int(tot.argmax())
    cap = T_cap - 1 if T_cap > 1 else 1
    if T_cap == 1:
        dur[row, 0] += 5
    want, over = R.frames_from_durations(dur, lengths, cap)
    assert bool(over[row])
    got = ops.frames_from_durations(dur.to(DEV), ld, cap)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want) and int(got[row]) == cap
    assert ops.status(clear=True) & _lib.STATUS_FRAME_CAPACITY
    assert ops.status() == 0
    # an all-zero row (nothing but padding) is one frame, as on every other path
    z = torch.zeros((B, N), dtype=torch.long, device=DEV)
    assert ops.frames_from_durations(z, None, 9).cpu().tolist() == [1] * B
    assert ops.status(clear=True) == 0


# ---- 2. pack kernel -----------------------------------------------------------------------------------------------------
def _pack_case(seed=5):
    T_cap, spf = 7, 600
    frames = [1, T_cap, 0, 3, 5, 1, T_cap, 4]  # 1 and T_cap included; frames 0: spf * T_b <= trim for every trim
    B, L = len(frames), spf * T_cap
    g = torch.Generator().manual_seed(seed)
    wave = torch.randn(B, L, generator=g) * 0.7  # ~15 % of the samples beyond +-1
    wave[1, 17], wave[1, 4000], wave[3, 1799], wave[4, 0] = float("nan"), 3.5, -2.25, float("nan")
    wave[6, 100:108] = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, 32766.5, 1e-9, -1e-9]) / 32767.0  # ties
    for b, f in enumerate(frames):
        wave[b, spf * f:] = float("nan")  # the ragged decoder's tails may hold anything: none of it may appear
    return wave, frames, T_cap, spf


@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("trim", [0, 50, 650])
def test_wave_pack_is_bit_for_bit_the_numpy_contract(fmt, trim):
    wave, frames, T_cap, spf = _pack_case()
    B = len(frames)
    dtype, npd, bits = (torch.int16, np.int16, np.int16) if fmt == "s16" else (torch.float32, np.float32, np.uint32)
    want, want_off = R.wave_pack(wave.numpy(), frames, T_cap, spf, trim, fmt)
    total = int(want_off[-1])
    assert total > 0 and (trim < 600 or want_off[1] == 0)
    fd = torch.tensor(frames, dtype=torch.int32, device=DEV)
    sentinel = 12345 if fmt == "s16" else -77.25
    # (a) a roomy output at an odd element offset: heads, bodies and tails of every alignment; nothing past offsets[B]
    for shift in (0, 1, 3):
        room = torch.full((total + 64 + shift,), sentinel, dtype=dtype, device=DEV)
        packed, offs = ops.wave_pack(wave.to(DEV), fd, trim=trim, fmt=fmt, out=room[shift:], samples_per_frame=spf)
        torch.cuda.synchronize()
        assert offs.dtype == torch.int64 and offs.cpu().numpy().tolist() == want_off.tolist()
        got = room.cpu().numpy()
        assert np.array_equal(got[shift:shift + total].view(bits), want.view(bits)), "fmt %s trim %d shift %d" % (fmt, trim, shift)
        assert (got[:shift] == npd(sentinel)).all() and (got[shift + total:] == npd(sentinel)).all()
    if fmt == "f32":  # the NaNs put INSIDE valid ranges travel; the NaN tails do not
        inside = int(np.isnan(want).sum())
        assert inside == 2 and int(np.isnan(got[3:3 + total]).sum()) == inside
    # (b) a truncating out_capacity: offsets describe the whole layout, nothing at or past the capacity is written
    cap = total - 1234
    room = torch.full((total + 64,), sentinel, dtype=dtype, device=DEV)
    packed, offs = ops.wave_pack(wave.to(DEV), fd, trim=trim, fmt=fmt, out=room[:cap], samples_per_frame=spf)
    torch.cuda.synchronize()
    got = room.cpu().numpy()
    assert offs.cpu().numpy().tolist() == want_off.tolist()
    assert np.array_equal(got[:cap].view(bits), want[:cap].view(bits)) and (got[cap:] == npd(sentinel)).all()
    # (c) default buffers, [B, 1, L] input
    packed, offs = ops.wave_pack(wave.to(DEV).unsqueeze(1), fd, trim=trim, fmt=fmt, samples_per_frame=spf)
    torch.cuda.synchronize()
    assert packed.numel() == B * spf * T_cap and np.array_equal(packed[:total].cpu().numpy().view(bits), want.view(bits))


# ---- 3.-5. pipeline -------------------------------------------------------------------------------------------------------
def _model(tag):
    man = manifest(tag)
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    for i, k in enumerate(KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval()
    sds = {k: {n: t.clone() for n, t in model[k].state_dict().items()} for k in KEYS}
    return man, model, sds


def _val_rows(rows, multi, seed=8):
    """Rows of benchdata/val_phonemes_32.txt as a right-padded batch with pinned draws (no sine noise: it is sized by the
    frame counts, which the test learns from the parent path)."""
    import bench
    tokens, lengths, noise, _, lens = bench.ragged_inputs("cpu")
    lens = [lens[i] for i in rows]
    N = max(lens)
    g = torch.Generator().manual_seed(seed)
    step_noise = torch.randn(STEPS - 1, len(rows), 1, 256, generator=g)
    ref_s = torch.randn(len(rows), 256, generator=g) if multi else None
    return tokens[rows][:, :N].contiguous(), lengths[rows], noise[rows], lens, step_noise, ref_s


class _count_calls:
    """Counts Engine.prosody_forward / Engine.decoder_forward calls."""

    def __enter__(self):
        from styletts2_amd import engine as E
        self.E, self.n = E, {"prosody": 0, "decoder": 0}
        self.orig = (E.Engine.prosody_forward, E.Engine.decoder_forward)
        op, od, n = self.orig[0], self.orig[1], self.n

        def cp(eng, *a, **k):
            n["prosody"] += 1
            return op(eng, *a, **k)

        def cd(eng, *a, **k):
            n["decoder"] += 1
            return od(eng, *a, **k)
        E.Engine.prosody_forward, E.Engine.decoder_forward = cp, cd
        return self.n

    def __exit__(self, *exc):
        self.E.Engine.prosody_forward, self.E.Engine.decoder_forward = self.orig


class _no_device_reads:
    """Any .tolist() / .item() on a device tensor raises while this is active."""

    def __enter__(self):
        self.orig = (torch.Tensor.tolist, torch.Tensor.item)
        ot, oi = self.orig

        def tolist(t):
            assert not t.is_cuda, ".tolist() on a device tensor"
            return ot(t)

        def item(t):
            assert not t.is_cuda, ".item() on a device tensor"
            return oi(t)
        torch.Tensor.tolist, torch.Tensor.item = tolist, item

    def __exit__(self, *exc):
        torch.Tensor.tolist, torch.Tensor.item = self.orig


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_capacity_path_predicted_durations_equals_the_ragged_path(tag):
    """The first 8 validation utterances with PREDICTED durations (2 100 - 4 555 frames with the seeded weights).
    `max_frames == max(tot)`: bitwise the parent path (same geometry); rounded up to the next multiple of 64: within the
    project's conv-path bar, 1e-6 * max(rms, 1), tails exactly zero.  One prosody and one decoder call, no host read in
    `prepare` (it is captured into a hipGraph: a synchronising call would abort the capture).  Row 3 (84 tokens) is held to the
    oracle at WAVE_RMS_TOL: iSTFTNet with the oracle's harmonic features injected, HiFi-GAN end to end."""
    man, model, sds = _model(tag)
    multi = bool(man["config"]["multispeaker"])
    hifigan = man["config"]["decoder"]["type"] == "hifigan"
    rows = list(range(8))
    tokens, lengths, noise, lens, step_noise, ref_s = _val_rows(rows, multi)
    B, b0 = len(rows), 3
    n0 = lens[b0]
    # the oracle's own run of row 3 gives its frame count; the sine noise of every row is sized by the 64-rounded capacity
    to = {}
    with torch.no_grad():
        o_in = O.front(sds, man["config"], man["plbert"], tokens[b0:b0 + 1, :n0], lengths[b0:b0 + 1], noise[b0:b0 + 1],
                       step_noise[:, b0:b0 + 1], diffusion_steps=STEPS, ref_s=None if ref_s is None else ref_s[b0:b0 + 1],
                       taps=to)  # (asr, F0, N, decoder style) of the oracle's own run
    T0 = int(to["durations"].sum())
    for k in KEYS:
        model[k].to(DEV)
    sampler = models.make_sampler(model)
    d = lambda t: None if t is None else t.to(DEV)
    tk, nz, sz, rs = d(tokens), d(noise), d(step_noise), d(ref_s)
    kw = dict(diffusion_steps=STEPS, ref_s=rs, step_noise=sz)
    taps_free = pipeline.prepare(model, sampler, tk, lengths, nz, allow_ragged=True, ragged_decode=True, **kw)
    tot = taps_free["frames_host"]
    T_max = max(tot)
    T_64 = (T_max + 63) // 64 * 64
    assert tot[b0] == T0 and len(set(tot)) > 1 and T_64 > T_max, (tot, T0)
    g = torch.Generator().manual_seed(77)
    sine = torch.randn(B, 600 * T_64, 9, generator=g).to(DEV)  # both paths see the same values in every row's 600 T_b samples
    parent = pipeline.inference(model, sampler, tk, lengths, nz, sine_noise=sine, ragged_decode=True, **kw)
    torch.cuda.synchronize()
    assert [w.shape[-1] for w in parent] == [600 * t for t in tot]
    # -- max_frames == max(tot): the parent's geometry, bit for bit; one call each; no device read in prepare
    with _count_calls() as calls, _no_device_reads():
        res = pipeline.inference(model, sampler, tk, lengths, nz, sine_noise=sine, max_frames=T_max, **kw)
    torch.cuda.synchronize()
    assert calls == {"prosody": 1, "decoder": 1}, calls
    assert isinstance(res, pipeline.SynthesisResult) and res.wave.shape == (B, 1, 600 * T_max)
    assert res.frames.dtype == torch.int32 and res.frames.cpu().tolist() == tot
    for b in range(B):
        assert torch.equal(res.wave[b, :, :600 * tot[b]], parent[b]), "row %d at max_frames == max(tot)" % b
        assert not bool(res.wave[b, :, 600 * tot[b]:].any())
    # -- spare capacity: the next multiple of 64
    res64 = pipeline.inference(model, sampler, tk, lengths, nz, sine_noise=sine, max_frames=T_64, **kw)
    torch.cuda.synchronize()
    assert res64.wave.shape == (B, 1, 600 * T_64) and res64.frames.cpu().tolist() == tot
    for b in range(B):
        pw = parent[b].cpu()
        e, bar = rms(res64.wave[b, :, :600 * tot[b]].cpu() - pw), 1e-6 * max(rms(pw), 1.0)
        print("%s row %d (%d frames) at capacity %d: rms diff %.3e, bar %.3e" % (tag, b, tot[b], T_64, e, bar))
        assert e <= bar, "row %d: %g > %g" % (b, e, bar)
        assert not bool(res64.wave[b, :, 600 * tot[b]:].any()), "row %d: tail not exactly zero" % b
    assert ops.status() & CAPACITY_BITS == 0
    # -- prepare(max_frames=) under stream capture: a synchronising call (a read-back of the durations) would abort it
    ld = lengths.to(torch.int32).to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with _no_device_reads():
                pg = pipeline.prepare(model, sampler, tk, None, nz, lengths_dev=ld, max_frames=T_64, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert "frames_host" not in pg and pg["frames"].cpu().tolist() == tot and pg["asr"].shape == (B, 512, T_64)
    # -- row 3 against the oracle at the 1e-4 bar
    with torch.no_grad():
        ref = O.decoder(sds["decoder"], man["config"]["decoder"], *o_in, noise=sine[b0:b0 + 1, :600 * T0].cpu(), taps=to)
    if hifigan:  # no ill-conditioned STFT-phase input: the true end-to-end bar, nothing injected
        for name, w in (("parent", parent[b0]), ("max_frames", res.wave[b0, :, :600 * T0]), ("max_frames 64", res64.wave[b0, :, :600 * T0])):
            e = rms(w.cpu() - ref[0])
            print("%s row %d vs oracle, %s: rms %.3e (bar %.1e)" % (tag, b0, name, e, WAVE_RMS_TOL))
            assert e < WAVE_RMS_TOL, "%s: %g" % (name, e)
    else:  # the tap-point protocol: the ragged decoder at capacity on the oracle's inputs and harmonic features
        Tc = T0 + 64
        asr, F0, Nn = torch.zeros(2, 512, Tc), torch.zeros(2, 2 * Tc), torch.zeros(2, 2 * Tc)
        hp = torch.zeros(2, to["har"].shape[1], 120 * Tc + 1)
        for r in range(2):
            asr[r, :, :T0], F0[r, :2 * T0], Nn[r, :2 * T0] = o_in[0][0], o_in[1][0], o_in[2][0]
            hp[r, :, :to["har"].shape[-1]] = to["har"][0]
        fr = torch.tensor([T0, T0], dtype=torch.int32, device=DEV)
        s2 = o_in[3].repeat(2, 1)
        w = model.decoder(asr.to(DEV), F0.to(DEV), Nn.to(DEV), s2.to(DEV), noise=sine[b0:b0 + 2, :600 * Tc].contiguous(),
                          har=hp.to(DEV), frames=fr)
        e = rms(w[:1, :, :600 * T0].cpu() - ref)
        print("%s row %d vs oracle (harmonic features injected): rms %.3e (bar %.1e)" % (tag, b0, e, WAVE_RMS_TOL))
        assert e < WAVE_RMS_TOL
    ops.check_status()


def test_graphed_synthesis_replays_the_eager_capacity_call():
    """One hipGraph from tokens to packed PCM: the replay equals the eager `max_frames` call on the same buffers, a second
    replay serves other tokens AND other lengths from the same graph, packed / offsets are `ops.wave_pack` of the eager wave,
    and `to_host()` hands back every row's own samples."""
    man, model, sds = _model("ljspeech")
    for k in KEYS:
        model[k].to(DEV)
    sampler = models.make_sampler(model)
    sets = [_val_rows([3, 4], False, seed=11), _val_rows([6, 3], False, seed=12)]  # 84 / 87 and 108 / 84 tokens
    B, N = 2, max(t.shape[1] for t, *_ in sets)
    need = []  # the capacity comes from a first, host-read run of both batches: no frame count of the seeded weights is assumed
    for tokens, lengths, noise, lens, step_noise, _ in sets:
        p = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), diffusion_steps=STEPS,
                             step_noise=step_noise.to(DEV), allow_ragged=True)
        need.append(p["durations"].sum(dim=1).tolist())
    T_cap = (max(max(n) for n in need) + 64) // 64 * 64  # the next multiple of 64 above the longest row: nothing truncated
    assert need[0] != need[1] and all(max(n) < T_cap for n in need)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS, pack="s16")
    g = torch.Generator().manual_seed(5)
    for i, (tokens, lengths, noise, lens, step_noise, _) in enumerate(sets):
        tk = torch.zeros(B, N, dtype=torch.long)
        tk[:, :tokens.shape[1]] = tokens
        sine = torch.randn(B, 600 * T_cap, 9, generator=g)
        res = gs(tokens=tk, lengths=lengths.to(torch.int32), noise=noise, step_noise=step_noise, sine_noise=sine)
        torch.cuda.synchronize()
        st = gs.static
        eager = pipeline.inference(model, sampler, st["tokens"], noise=st["noise"], step_noise=st["step_noise"],
                                   sine_noise=st["sine_noise"], lengths_dev=st["lengths_dev"], diffusion_steps=STEPS,
                                   max_frames=T_cap, pack="s16")
        torch.cuda.synchronize()
        fr = eager.frames.cpu().tolist()
        assert fr == need[i], (fr, need[i])  # the frame counts of the host-read run: nothing truncated
        assert torch.equal(res.frames, eager.frames) and torch.equal(res.wave, eager.wave), "replay %d" % i
        packed, offs = ops.wave_pack(eager.wave, eager.frames, trim=0, fmt="s16")
        torch.cuda.synchronize()
        total = int(offs[-1])
        assert offs.cpu().tolist() == [0, 600 * fr[0], 600 * (fr[0] + fr[1])]
        assert torch.equal(res.offsets, offs) and torch.equal(res.packed[:total], packed[:total])
        host = res.to_host()
        assert len(host) == B
        for b in range(B):
            want = R.pcm16(eager.wave[b, 0, :600 * fr[b]].cpu().numpy())
            assert host[b].dtype == np.int16 and np.array_equal(host[b], want), "row %d of replay %d" % (b, i)
    assert gs._g is not None and ops.status() & CAPACITY_BITS == 0
    # a result made without `pack` packs as fp32 on the way out
    plain = pipeline.inference(model, sampler, st["tokens"], noise=st["noise"], step_noise=st["step_noise"],
                               sine_noise=st["sine_noise"], lengths_dev=st["lengths_dev"], diffusion_steps=STEPS, max_frames=T_cap)
    rows_h = plain.to_host()
    assert all(np.array_equal(rows_h[b].view(np.uint32), eager.wave[b, 0, :600 * fr[b]].cpu().numpy().view(np.uint32))
               for b in range(B))


def test_a_row_over_capacity_is_truncated_and_reported_and_the_others_are_untouched():
    man, model, sds = _model("ljspeech")
    for k in KEYS:
        model[k].to(DEV)
    sampler = models.make_sampler(model)
    tokens, lengths, noise, lens, step_noise, _ = _val_rows([3, 4, 6], False, seed=21)  # 84, 87, 108 tokens
    base = dict(noise=noise.to(DEV), diffusion_steps=STEPS, step_noise=step_noise.to(DEV))
    # what every row needs, from a host-read run; the capacity is then put between the two short rows and the long one
    need = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, allow_ragged=True, **base)["durations"].sum(dim=1).tolist()
    assert max(need[:2]) + 1 < need[2], need
    T_cap = (max(need[:2]) + need[2]) // 2
    sine = torch.randn(3, 600 * T_cap, 9, generator=torch.Generator().manual_seed(4)).to(DEV)
    kw = dict(sine_noise=sine, max_frames=T_cap, **base)
    torch.cuda.synchronize()
    ops.status(clear=True)
    short = lengths.clone()
    short[2] = min(lens[:2]) - 4  # the fitting run: the same tokens, row 2 cut to fewer phonemes than the rows that fit
    fit = pipeline.inference(model, sampler, tokens.to(DEV), short, **kw)
    torch.cuda.synchronize()
    f_fit = fit.frames.cpu().tolist()
    assert ops.status() & CAPACITY_BITS == 0 and max(f_fit) < T_cap and f_fit[:2] == need[:2], (f_fit, need)
    over = pipeline.inference(model, sampler, tokens.to(DEV), lengths, **kw)  # completes
    torch.cuda.synchronize()
    st = ops.status()
    assert st & _lib.STATUS_FRAME_CAPACITY, hex(st)
    f_over = over.frames.cpu().tolist()
    assert f_over == [f_fit[0], f_fit[1], T_cap] and over.wave.shape[-1] == 600 * T_cap
    for b in range(2):
        assert torch.equal(over.wave[b], fit.wave[b]), "row %d changed because row 2 ran out of capacity" % b
    assert bool(torch.isfinite(over.wave[2]).all()) and bool(over.wave[2, :, -600:].any())  # truncated, not padded
    with pytest.warns(RuntimeWarning, match="FRAME_CAPACITY"):
        rows = over.to_host()  # the one place that waits also looks at the status word: reported as a warning, and the
        #                        DURATION_SUM the expansion raised for the same row goes with it
    assert [len(r) for r in rows] == [600 * f for f in f_over]
    assert ops.status() & CAPACITY_BITS == 0


# ---- 6. the output options together ------------------------------------------------------------------
def test_every_output_option_at_once_equals_the_pieces_composed_by_hand():
    """Three rows of 12, 9 and 7 tokens at a capacity three frames above the longest, 16-bit PCM at 16 kHz with marks, breaks and a
    level: the smallest call whose header has all five parts and a pad that is not zero.  What `to_host` hands back is, byte for
    byte, `ops.wave_level`, `ops.wave_pack_level` and `ops.token_marks` over the result's own `wave` and `frames`."""
    from test_passage_gpu import _passage, _sub
    P = _passage("libritts")
    model, sampler, trim = P["model"], P["sampler"], P["trim"]
    tk, kw = _sub(P, 0, 3)
    B, N = tk.shape
    front = {k: v for k, v in kw.items() if k not in ("sine_noise", "trim")}
    need = pipeline.prepare(model, sampler, tk, allow_ragged=True, ragged_decode=True, **front)["frames_host"]
    T, gaps = max(need) + 3, [0, 5, 3]
    assert len(set(need)) == B
    lv = pipeline.Level(B, target=[-20.0, None, -30.0], max_gain_db=30.0)
    torch.cuda.synchronize()
    ops.status(clear=True)
    res = pipeline.inference(model, sampler, tk, max_frames=T, pack="s16", sample_rate=16000, marks=True, gaps=gaps, level=lv, **kw)
    rows, marks, level = res.to_host(marks=True, level=True)
    rows, marks, level = [r.copy() for r in rows], marks.copy(), level.copy()
    assert res.frames.cpu().tolist() == need and ops.status() & CAPACITY_BITS == 0
    assert (res.pack, res.trim, res.sample_rate, res.max_gap, res.max_frames, res.samples_per_frame) == ("s16", trim, 16000, 5, T, 600)
    header = 8 * (B + 1) + 4 * B * (N + 1) + 4 * B + 16 * B
    assert header % 16 and res.packed.data_ptr() - res.offsets.data_ptr() == (header + 15) // 16 * 16
    assert res.gaps.cpu().tolist() == gaps and tuple(res.marks.shape) == (B, N + 1) and tuple(res.level.shape) == (B, 4)
    # by hand
    p = pipeline.prepare(model, sampler, tk, max_frames=T, **front)
    want_lv = ops.wave_level(res.wave, res.frames, lv.target, ceiling=lv.ceiling, max_gain_db=lv.max_gain_db, trim=trim)
    want, woff = ops.wave_pack_level(res.wave, res.frames, want_lv, gaps=torch.tensor(gaps, dtype=torch.int32, device=DEV), max_gap=5,
                                     rate=16000, fmt="s16", trim=trim)
    want_m = ops.token_marks(p["durations"], res.frames, T, lengths=p["token_lengths"], shift=model.decoder.kind == "hifigan",
                             trim=trim, rate=16000)
    torch.cuda.synchronize()
    want, offs = want.cpu().numpy(), woff.cpu().tolist()
    assert torch.equal(res.offsets, woff) and res.to_host(passage=True).tobytes() == want[:offs[B]].tobytes()
    for b in range(B):
        assert rows[b].dtype == np.int16 and rows[b].tobytes() == want[offs[b]:offs[b + 1] - gaps[b]].tobytes(), "row %d" % b
        assert not want[offs[b + 1] - gaps[b]:offs[b + 1]].any(), "the break behind row %d" % b
    assert marks.dtype == np.int32 and marks.tobytes() == want_m.cpu().numpy().tobytes()
    assert level.dtype == np.float32 and level.tobytes() == want_lv.cpu().numpy().tobytes()
    assert level[1, 2] == 1.0 and level[0, 2] != 1.0, "row 1 is left alone, row 0 is not"
    ops.check_status()


def test_the_constructor_and_a_device_tensor_of_gaps_refuse_what_the_table_says(monkeypatch):
    """The rows of tests/golden/output_refusals.json that need a device: `GraphedSynthesis` refuses in `__init__`, before any
    capture, and `inference` a device tensor of gaps without `max_gap`."""
    import json
    import os
    from test_output_spec_cpu import _arg
    from test_passage_gpu import K, STEPS, _passage, _sub  # the passage's own draws: its number of diffusion steps
    table = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "output_refusals.json")))
    P = _passage("libritts")
    recorded = []
    monkeypatch.setattr(pipeline, "_record_graph", lambda *a, **kw: recorded.append(a))
    cases = [c for c in table if c["entry"] == "graphed"]
    assert {c["fault"] for c in cases} == {"marks without pack", "max_gap without pack", "bad sample_rate", "level without pack"}
    for c in cases:
        with pytest.raises(Exception) as e:
            pipeline.GraphedSynthesis(P["model"], P["sampler"], K, P["b"]["tokens"].shape[1], P["T"], STEPS, ref_s=P["ref_s"], **c["args"])
        assert type(e.value).__name__ == c["raises"] and str(e.value) == c["text"], c["fault"]
    (c,) = [c for c in table if c["entry"] == "inference_device"]
    tk, kw = _sub(P, 0, 2)
    with pytest.raises(Exception) as e:
        pipeline.inference(P["model"], P["sampler"], tk, **kw, **{k: _arg(v, DEV) for k, v in c["args"].items()})
    assert type(e.value).__name__ == c["raises"] and str(e.value) == c["text"]
    assert not recorded


def test_one_graph_with_breaks_and_a_level_equals_the_eager_call_at_every_replay():
    """ONE recorded graph with `pack`, `max_gap` and `level=True`: other breaks and other targets at the second replay, and at
    each what `to_host(level=True)` hands back is the eager `inference` call on the same static inputs, byte for byte."""
    from test_passage_gpu import K, STEPS, _passage  # the passage's own draws: its number of diffusion steps
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T, N = P["T"], b["tokens"].shape[1]
    out = dict(pack="s16", sample_rate=16000)
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, max_gap=40,
                                   level=True, **out)
    ld = b["lengths"].to(torch.int32).to(DEV)
    feed = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    eager_kw = dict(P["kw"], input_lengths=None, lengths_dev=ld, max_frames=T, **out)
    graph = None
    for i, (gaps, targets) in enumerate((([7, 0, 40, 3], [-20.0, -23.0, None, -30.0]), ([0, 55, 1, 9], [-35.0, None, -18.0, -27.0]))):
        res = gs(gaps=gaps, level=targets, **(feed if i == 0 else {}))
        graph = gs._g["graph"] if graph is None else graph
        assert gs._g["graph"] is graph, "no re-record"
        rows, lv = res.to_host(level=True)
        rows, lv, whole = [r.copy() for r in rows], lv.copy(), res.to_host(passage=True).copy()
        eager = pipeline.inference(model, sampler, b["tokens"], gaps=torch.tensor(gaps, dtype=torch.int32, device=DEV), max_gap=40,
                                   level=pipeline.Level(K, target=targets), **eager_kw)
        erows, elv = eager.to_host(level=True)
        assert torch.equal(res.wave, eager.wave) and torch.equal(res.offsets, eager.offsets), "replay %d" % i
        assert all(x.tobytes() == y.tobytes() for x, y in zip(rows, erows)) and lv.tobytes() == elv.tobytes(), "replay %d" % i
        assert whole.tobytes() == eager.to_host(passage=True).tobytes(), "replay %d" % i
        offs = res.offsets.cpu().tolist()
        assert [offs[k + 1] - offs[k] - len(rows[k]) for k in range(K)] == [min(g, 40) for g in gaps]
        assert [bool(v == 1.0) for v in lv[:, 2]] == [t is None for t in targets]
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()
