"""Intonation on the device: `st2_pitch_shape` against the numpy contract of tests/_intonation_ref.py -- by
bits where the contract says bits (unvoiced columns, columns with r == 1 and c == 0, everything at or past a row's end and
between L and the row stride), to one fp32 ulp elsewhere (the last ulp of fp64 log2 / exp2 and the order of the fp64 sum are the
only freedom), the voiced count exact -- then `intonation=` through the pipeline.  Shapes are the smallest at which the kernel
can still go wrong: one frame; rows that end inside a wave, past the workgroup's 256 threads and past 512 columns; an empty row
beside full ones; one, seventy (two scan chunks) and 512 tokens.

The pipeline tests need a voiced F0 curve.  The seeded synthetic weights predict F0 within about [-1.5, 0.3] whatever the seed
(their output head is a 1 x 1 conv of unit-scale weights), which no voiced threshold makes a quarter voiced.  So these tests
build a model of their own with that head mapped to the speech range -- `F0_proj.weight *= 300`, `F0_proj.bias = 150`: the CPU
oracle gives 84 % to 92 % of the columns above the default 10 Hz for the three rows used here -- and assert the share."""
import functools

import numpy as np
import pytest
import torch

import _intonation_ref as R
from styletts2_amd import _lib, models, ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NAN, INF = float("nan"), float("inf")
CANARY = F32(333.25)  # a voiced value: a kernel that read it would move the row's mean
PAD = 8


def curve(B, L, seed, unvoiced=0.3, hard=True):
    g = np.random.default_rng(seed)
    x = (80.0 * np.exp2(2.3 * g.random((B, L)))).astype(F32)
    x[g.random((B, L)) < unvoiced] = 0
    if hard and L >= 40:
        x[:, 5], x[:, 6], x[:, 17], x[:, 18], x[:, 19], x[:, L - 1] = NAN, INF, -INF, -250.0, 10.0, F32(9.999)
    return x


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def run(f0, frames=None, rng=None, tok=None, dur=None, shift=False, contour=None, pitch=True, **hz):
    """One `ops.pitch_shape` call on rows of stride L + PAD, canaries between L and the stride -> (buffer, pitch) as numpy."""
    B, L = f0.shape
    buf = torch.full((B, L + PAD), float(CANARY), device=DEV)
    buf[:, :L] = dev(f0)
    p = ops.pitch_shape(buf[:, :L], range=dev(rng), tok_range=dev(tok), dur=dev(dur, torch.int64), contour=dev(contour),
                        frames=dev(frames, torch.int32), shift=shift, pitch=pitch, **hz)
    return buf.cpu().numpy(), None if p is None else p.cpu().numpy()


def check(f0, frames=None, rng=None, tok=None, dur=None, shift=False, contour=None, tag="", **hz):
    """Every bar of the contract for one call -> the number of columns that differ from the reference at all."""
    B, L = f0.shape
    got, gp = run(f0, frames, rng, tok, dur, shift, contour, **hz)
    want, wp = R.reference(f0, frames=frames, range=rng, tok_range=tok, dur=dur, shift=shift, contour=contour,
                           **dict(dict(voiced_hz=10.0, lo_hz=40.0, hi_hz=1100.0), **hz))
    exact = R.reference.exact
    assert (got[:, L:] == CANARY).all(), (tag, "written between L and the row stride")
    out = got[:, :L]
    assert np.array_equal(R.bits(out[exact]), R.bits(want[exact])), (tag, "a column the contract fixes by bits")
    err = R.ulp_diff(out[~exact], want[~exact])
    assert err.size == 0 or err.max() <= 1, (tag, "a shaped column is more than one fp32 ulp off", err.max())
    assert np.array_equal(gp[:, 1], wp[:, 1]), (tag, "n_v", gp[:, 1], wp[:, 1])
    assert np.array_equal(np.isnan(gp), np.isnan(wp)), (tag, gp, wp)
    fin = ~np.isnan(wp)
    assert R.ulp_diff(gp[fin], wp[fin]).max(initial=0) <= 1, (tag, "pitch", gp, wp)
    differ = int((err > 0).sum())
    print("%s: %d of %d shaped columns differ from the reference by one ulp" % (tag, differ, err.size))
    return differ


def tables(B, N, K, seed, T_cap, wild=False):
    """range [B], tok_range [B, N], durations [B, N] with zeros and an empty last token, contour [B, K, 2]."""
    g = np.random.default_rng(seed)
    rng = g.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0, 3.5], dtype=F32), B)
    tok = g.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0, 4.0], dtype=F32), (B, N))
    dur = g.integers(0, max(2 * T_cap // max(N, 1), 2) + 1, (B, N))
    dur[:, N // 2] = 0
    dur[:, -1] = 0 if N > 1 else T_cap
    con = np.full((B, max(K, 1), 2), NAN, dtype=F32)[:, :K]
    for b in range(B):
        n = g.integers(0, K + 1)
        con[b, :n, 0] = np.sort(g.random(n))
        con[b, :n, 1] = g.uniform(-12, 12, n)
    if wild:  # what a device tensor may hold: out of range, NaN, descending
        rng[0], tok[:, 0], tok[:, 1 % N] = 9.0, -3.0, NAN
        if B > 1:
            rng[1] = NAN
        if K >= 2:
            con[:, 0], con[:, 1] = (0.8, 40.0), (0.2, -40.0)
        if K >= 4:
            con[:, 2], con[:, 3] = (NAN, 3.0), (0.9, NAN)
    return rng, tok, dur, con


# ---- the kernel against the contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True])
def test_rows_that_end_inside_a_wave_past_the_workgroup_and_past_512_columns(shift):
    f0 = curve(3, 600, 1)
    frames = [1, 129, 300]
    rng, tok, dur, con = tables(3, 70, 8, 2, 300)
    for tag, kw in (("range", dict(rng=rng)), ("tok_range", dict(tok=tok, dur=dur)), ("contour", dict(contour=con)),
                    ("all", dict(rng=rng, tok=tok, dur=dur, contour=con)), ("none", dict())):
        check(f0, frames, shift=shift, tag="%s shift=%d" % (tag, shift), **kw)
    rng, tok, dur, con = tables(3, 70, 8, 3, 300, wild=True)
    check(f0, frames, rng, tok, dur, shift, con, tag="clamped tables")
    # nothing at or past a row's end is looked at: canaries there, and they come back by bits
    g = f0.copy()
    for b, t in enumerate(frames):
        g[b, 2 * t:] = CANARY
    check(g, frames, rng, tok, dur, shift, con, tag="canaries past the rows")


def test_one_frame_an_empty_row_beside_full_ones_and_no_frames():
    for B in (1, 2):
        f0 = np.array([[120.0, 180.0], [0.0, 95.0]], dtype=F32)[:B]
        check(f0, None, rng=[0.0, 3.0][:B], contour=np.array([[[0.5, 7.0]]] * B, dtype=F32), tag="L = 2, B = %d" % B)
    f0 = curve(4, 80, 4)
    rng, tok, dur, con = tables(4, 5, 3, 5, 40)
    check(f0, [0, 40, 0, 17], rng, tok, dur, True, con, tag="T_b = 0 beside full rows")
    check(f0, [-3, 99, 1, 40], rng, tok, dur, False, con, tag="frames outside 0..T_cap are clamped")
    check(f0, None, rng, tok, dur, False, con, tag="frames = NULL")
    got, gp = run(f0, [0, 40, 0, 17], rng=rng)
    assert np.isnan(gp[[0, 2]][:, [0, 2, 3]]).all() and (gp[[0, 2], 1] == 0).all()


def test_rows_without_a_voiced_column_with_exactly_one_and_with_nonfinite_columns():
    f0 = np.zeros((4, 64), dtype=F32)
    f0[0, ::3], f0[0, 1::3] = NAN, -INF  # none voiced
    f0[1, 41] = 212.5  # exactly one: it is its own mean, and any range keeps it there
    f0[2] = curve(1, 64, 6, hard=False)[0]
    f0[2, [0, 1, 30, 63]] = [NAN, INF, -INF, NAN]
    f0[3] = 10.0  # at the threshold: not above it
    con = np.array([[[0.0, 5.0], [1.0, -5.0]]] * 4, dtype=F32)
    check(f0, None, rng=[2.0, 0.0, 0.5, 3.0], contour=con, tag="voicing")
    got, gp = run(f0, None, rng=[2.0, 2.0, 2.0, 2.0])
    assert np.array_equal(R.bits(got[[0, 1, 3], :64]), R.bits(f0[[0, 1, 3]])), "no voiced column, or one that is the mean: left alone"
    assert gp[1].tolist() == [212.5, 1.0, 212.5, 212.5] and gp[0, 1] == gp[3, 1] == 0


@pytest.mark.parametrize("N", [1, 70, 512])
@pytest.mark.parametrize("shift", [False, True])
def test_token_ranges_over_one_seventy_and_512_tokens(N, shift):
    f0 = curve(2, 260, 7 + N)
    rng, tok, dur, _ = tables(2, N, 0, 8 + N, 130)
    check(f0, [130, 77], rng, tok, dur, shift, tag="N = %d shift = %d" % (N, shift))
    dur[:] = 0
    dur[0, :1], dur[1, N // 3] = 500, 40  # one token over the capacity; durations that end early: the last token owns the rest
    check(f0, [130, 77], None, tok, dur, shift, tag="N = %d degenerate durations" % N)


@pytest.mark.parametrize("K", [0, 1, 8])
def test_contours_of_no_point_one_point_and_eight(K):
    f0 = curve(3, 120, 11 + K)
    con = np.full((3, K, 2), NAN, dtype=F32)
    if K == 1:
        con[0, 0], con[1, 0] = (0.4, -6.0), (NAN, 2.0)
    if K == 8:
        con[0] = [(0.0, 0.0), (0.25, 3.0), (0.25, -3.0), (0.5, -3.0), (0.5, 9.0), (0.75, 0.0), (1.0, 12.0), (1.0, -12.0)]  # coincident
        con[1] = [(0.9, 1.0), (0.1, 2.0), (NAN, 3.0), (0.5, NAN), (0.95, -4.0), (2.0, 30.0), (-1.0, -30.0), (INF, 1.0)]  # descending, NaN
        con[2, 3] = (0.5, 0.0)  # one used point of value 0: c == 0 everywhere, the input's bits
    check(f0, [60, 33, 60], contour=con, tag="K = %d" % K)
    if K == 8:
        got, _ = run(f0, [60, 33, 60], contour=con, pitch=None)
        assert np.array_equal(R.bits(got[2, :120]), R.bits(f0[2]))


def test_the_clamps_are_reached_and_a_clamped_column_stays_voiced():
    f0 = curve(2, 200, 13)
    con = np.array([[[0.0, -24.0], [1.0, 24.0]]] * 2, dtype=F32)
    check(f0, None, rng=[4.0, 4.0], contour=con, tag="lo and hi", lo_hz=90.0, hi_hz=300.0)
    got, gp = run(f0, None, rng=[4.0, 4.0], contour=con, lo_hz=90.0, hi_hz=300.0)
    vo = R.is_voiced(f0, 10.0)
    out = got[:, :200]
    assert (out[vo] == 90.0).any() and (out[vo] == 300.0).any() and np.array_equal(R.is_voiced(out, 10.0), vo)
    assert (gp[:, 2] == 90.0).all() and (gp[:, 3] == 300.0).all()
    check(f0, None, rng=[0.0, 2.0], tag="voiced_hz = 120", voiced_hz=120.0, lo_hz=121.0, hi_hz=1100.0)


def test_a_call_that_only_measures_writes_no_f0_and_one_without_anything_launches_nothing():
    f0 = curve(2, 90, 17)
    got, gp = run(f0, [45, 20])
    want, wp = R.reference(f0, frames=[45, 20])
    assert np.array_equal(R.bits(got[:, :90]), R.bits(f0)) and np.array_equal(gp[:, 1], wp[:, 1])
    assert R.ulp_diff(gp[:, [0, 2, 3]], wp[:, [0, 2, 3]]).max() <= 1 and np.array_equal(gp[:, 2:], wp[:, 2:])
    x = dev(f0)
    assert ops.pitch_shape(x) is None and ops.pitch_shape(x, contour=torch.empty((2, 0, 2), device=DEV)) is None
    assert np.array_equal(R.bits(x.cpu().numpy()), R.bits(f0))
    mine = torch.empty((2, 4), device=DEV)
    assert ops.pitch_shape(x, range=dev([0.0, 0.0]), pitch=mine) is mine and mine[:, 1].tolist() == wp_full(f0)
    with pytest.raises(_lib.St2Error, match="st2_pitch_shape: L=89 must be positive and even"):
        ops.pitch_shape(x[:, :89].contiguous(), range=dev([1.0, 1.0]))
    with pytest.raises(_lib.St2Error, match="need voiced_hz=10 < lo_hz=5"):
        ops.pitch_shape(x, range=dev([1.0, 1.0]), lo_hz=5.0)
    with pytest.raises(_lib.St2Error, match="tok_range needs dur"):
        ops.pitch_shape(x, tok_range=dev(np.ones((2, 4))))
    torch.cuda.synchronize()


def wp_full(f0):
    return [float(R.is_voiced(r, 10.0).sum()) for r in f0]


# ---- through the pipeline --------------------------------------------------------------------------------------------------------
VOICED_HZ = 10.0  # the default: the harmonic source's threshold


@functools.lru_cache(maxsize=None)
def _voiced():
    """The module's own model (see the module's docstring): the seeded ljspeech weights with the F0 head mapped to the speech range."""
    from test_controls_gpu import KEYS, _batch
    from _util import manifest
    from benchdata import synth
    man = manifest("ljspeech")
    model = models.build_model(models.recursive_munch(man["config"]), None, None, models.load_plbert(man["plbert"]))
    for i, k in enumerate(KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval()
    with torch.no_grad():
        model.predictor.F0_proj.weight.mul_(300.0)
        model.predictor.F0_proj.bias.fill_(150.0)
    for k in KEYS:
        model[k].to(DEV)
    b = _batch(False)
    B, N = b["tokens"].shape
    g = np.random.default_rng(5)
    settings = dict(range=[0.5, 2.0, 1.0], contour=[[(0.0, 0.0), (1.0, 6.0)], [(0.5, -3.0)], []],
                    tok_range=g.choice(np.array([0.0, 0.5, 1.0, 2.0], dtype=F32), (B, N)))
    return model, models.make_sampler(model), b, settings


def _kw(b, **more):
    from test_controls_gpu import STEPS
    return dict(input_lengths=b["lengths"], noise=b["noise"], diffusion_steps=STEPS, step_noise=b["step_noise"], **more)


def _contour_table(rows, K=8):
    con = np.full((len(rows), K, 2), NAN, dtype=F32)
    for b, pts in enumerate(rows):
        con[b, :len(pts)] = np.asarray(pts, dtype=F32).reshape(-1, 2)
    return con


def _hold(f0_plain, f0_shaped, pitch, frames, dur, shift, settings, tag, rows=None):
    """`f0_shaped` and `pitch` against the contract applied to `f0_plain` under the kernel tests' bars; the non-vacuity condition."""
    pick = (lambda v: v) if rows is None else (lambda v: np.asarray(v)[rows])
    x = f0_plain.cpu().numpy()
    want, wp = R.reference(x, frames=frames, range=pick(settings["range"]), tok_range=pick(settings["tok_range"]), dur=dur.cpu().numpy(),
                           shift=shift, contour=pick(_contour_table(settings["contour"])), voiced_hz=VOICED_HZ)
    valid = np.zeros(x.shape, dtype=bool)
    for b in range(x.shape[0]):
        valid[b, :x.shape[1] if frames is None else 2 * frames[b]] = True
    share = (R.is_voiced(x, VOICED_HZ) & valid).sum() / valid.sum()
    assert share >= 0.25, (tag, "the plain curve is not voiced enough to show anything", share)
    exact, got = R.reference.exact, f0_shaped.cpu().numpy()
    assert np.array_equal(R.bits(got[exact]), R.bits(want[exact])), tag
    err = R.ulp_diff(got[~exact], want[~exact])
    assert err.size > 0 and err.max() <= 1, (tag, err.max(initial=0))
    gp = pitch.cpu().numpy()
    assert np.array_equal(gp[:, 1], wp[:, 1]) and R.ulp_diff(gp[:, [0, 2, 3]], wp[:, [0, 2, 3]]).max() <= 1, (tag, gp, wp)
    print("%s: voiced share %.2f, %d of %d shaped columns differ by one ulp" % (tag, share, int((err > 0).sum()), err.size))


def _same_packed(a, b):
    """The packed samples of two results agree up to offsets[B]: the allocation behind them is at capacity and not cleared."""
    total = int(a.offsets[-1])
    return torch.equal(a.offsets, b.offsets) and torch.equal(a.packed[:total], b.packed[:total])


def test_prepare_shapes_the_curve_by_the_contract_and_leaves_the_rest_alone():
    model, sampler, b, settings = _voiced()
    B = b["tokens"].shape[0]
    shift = model.decoder.kind == "hifigan"
    it = pipeline.Intonation(B, voiced_hz=VOICED_HZ, **settings)
    for tag, more in (("ragged", dict(allow_ragged=True, ragged_decode=True)), ("groups", dict(allow_ragged=True)),
                      ("uniform", dict(durations=torch.full(tuple(b["tokens"].shape), 3, dtype=torch.long)))):
        p0 = pipeline.prepare(model, sampler, b["tokens"], **_kw(b, **more))
        p1 = pipeline.prepare(model, sampler, b["tokens"], intonation=it, **_kw(b, **more))
        assert torch.equal(p1["durations"], p0["durations"]) and torch.equal(p1["s_pred"], p0["s_pred"])
        if tag == "groups":
            assert len(p0["groups"]) == B, "three rows of three frame counts"
            for (idx, g0), (_, g1) in zip(p0["groups"], p1["groups"]):
                assert torch.equal(g1["asr"], g0["asr"]) and torch.equal(g1["N"], g0["N"])
                _hold(g0["F0"], g1["F0"], g1["pitch"], None, p0["durations"][idx], shift, settings, "groups row %s" % idx, rows=idx)
            continue
        assert torch.equal(p1["asr"], p0["asr"]) and torch.equal(p1["N"], p0["N"]) and tuple(p1["pitch"].shape) == (B, 4)
        _hold(p0["F0"], p1["F0"], p1["pitch"], p0.get("frames_host"), p0["durations"], shift, settings, tag)
    # shaped first, then the request's flat scale: the controls multiply the shaped curve
    ctl = pipeline.Controls(B, f0_scale=[1.5, 0.75, 1.25])
    more = dict(allow_ragged=True, ragged_decode=True)
    p1 = pipeline.prepare(model, sampler, b["tokens"], intonation=it, **_kw(b, **more))
    p2 = pipeline.prepare(model, sampler, b["tokens"], intonation=it, controls=ctl, **_kw(b, **more))
    assert torch.equal(p2["F0"], p1["F0"] * ctl.row("f0_scale")[:, None]) and torch.equal(p2["pitch"], p1["pitch"])
    torch.cuda.synchronize()
    ops.check_status()


def test_neutral_is_the_plain_call_and_the_capacity_path_decodes_the_shaped_curves():
    from test_controls_gpu import T_SINE
    model, sampler, b, settings = _voiced()
    B, N = b["tokens"].shape
    T_cap = 704
    assert T_cap <= T_SINE
    kw = _kw(b, sine_noise=b["sine"], max_frames=T_cap, pack="s16")
    plain = pipeline.inference(model, sampler, b["tokens"], **kw)
    neutral = pipeline.inference(model, sampler, b["tokens"], intonation=pipeline.Intonation.neutral(B, N=N), **kw)
    assert torch.equal(neutral.wave, plain.wave) and _same_packed(neutral, plain) and torch.equal(neutral.frames, plain.frames)
    assert plain.pitch is None and tuple(neutral.pitch.shape) == (B, 4) and bool((neutral.pitch[:, 1] > 0).all())
    it = pipeline.Intonation(B, voiced_hz=VOICED_HZ, **settings)
    res = pipeline.inference(model, sampler, b["tokens"], intonation=it, **kw)
    p = pipeline.prepare(model, sampler, b["tokens"], intonation=it, **_kw(b, max_frames=T_cap))
    p0 = pipeline.prepare(model, sampler, b["tokens"], **_kw(b, max_frames=T_cap))
    frames = p0["frames"].cpu().tolist()
    assert max(frames) < T_cap, "no row is truncated"
    _hold(p0["F0"], p["F0"], p["pitch"], frames, p0["durations"], model.decoder.kind == "hifigan", settings, "capacity")
    w = pipeline._decode_frames(model, p, b["sine"], strict=True)
    assert torch.equal(res.wave, w) and torch.equal(res.pitch, p["pitch"]) and torch.equal(res.frames, plain.frames)
    assert not torch.equal(res.wave, plain.wave)
    packed, offs = ops.wave_pack(w, p["frames"], trim=res.trim, fmt="s16", samples_per_frame=res.samples_per_frame)
    assert torch.equal(offs, res.offsets) and torch.equal(packed[:int(offs[-1])], res.packed[:int(offs[-1])])
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_intonation_and_its_neutral_replay_is_the_graph_without_it():
    from test_controls_gpu import STEPS
    model, sampler, b, settings = _voiced()
    B, N = b["tokens"].shape
    T_cap = 704
    ld = b["lengths"].to(torch.int32).to(DEV)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS, pack="s16", intonation=True, token_controls=True)
    first = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    other = dict(range=[2.0, 0.0, 3.0], contour=[(0.0, 4.0), (0.5, 4.0), (0.5, -4.0)], tok_range=None)
    eager_kw = dict(noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"], lengths_dev=ld, diffusion_steps=STEPS,
                    max_frames=T_cap, pack="s16")
    graphs, waves = [], []
    for i, s in enumerate((settings, other)):
        res = gs(intonation=pipeline.Intonation(B, **s), **(first if i == 0 else {}))
        graphs.append(gs._g["graph"])
        eager = pipeline.inference(model, sampler, b["tokens"], intonation=pipeline.Intonation(B, **s), **eager_kw)
        assert torch.equal(res.wave, eager.wave) and _same_packed(res, eager) and torch.equal(res.pitch, eager.pitch), i
        waves.append(res.wave.clone())
    assert graphs[0] is graphs[1] and not torch.equal(waves[0], waves[1]), "no second capture, another rendition"
    res = gs()  # left out: the tables go back to neutral
    without = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS, pack="s16", token_controls=True)
    base = without(**first)
    assert gs._g["graph"] is graphs[0] and torch.equal(res.wave, base.wave) and _same_packed(res, base)
    assert base.pitch is None
    with pytest.raises(ValueError, match="built without intonation"):
        without(intonation=pipeline.Intonation(B))
    torch.cuda.synchronize()
    ops.check_status()


def test_long_form_takes_one_row_per_sentence_on_both_paths():
    from test_controls_gpu import LENS, STEPS
    model, sampler, b, settings = _voiced()
    K = len(LENS)
    sentences = [b["tokens"][k, :LENS[k]].clone() for k in range(K)]
    noises = [b["noise"][k:k + 1] for k in range(K)]
    step_noises = [b["step_noise"][:, k:k + 1].contiguous() for k in range(K)]
    per_row = dict(range=settings["range"], contour=settings["contour"])
    it = pipeline.Intonation(K, **per_row)
    one = lambda k: pipeline.Intonation(1, range=[per_row["range"][k]], contour=[per_row["contour"][k]])
    # sentence by sentence, each with an object of its own
    want, sines, s_prev = [], [], None
    for k in range(K):
        p = pipeline.prepare(model, sampler, sentences[k][None], noise=noises[k], step_noise=step_noises[k], diffusion_steps=STEPS,
                             lj_tail=False, s_prev=s_prev, intonation=one(k))
        sines.append(b["sine"][k:k + 1, :600 * p["asr"].shape[-1]].contiguous())
        want.append(model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sines[k]).reshape(-1))
        s_prev = p["s_pred"]
    waves, s_last = pipeline.synthesize_long(model, sampler, sentences, diffusion_steps=STEPS, noises=noises, step_noises=step_noises,
                                             sine_noises=sines, front_batch=0, overlap=False, intonation=it)
    plain, _ = pipeline.synthesize_long(model, sampler, sentences, diffusion_steps=STEPS, noises=noises, step_noises=step_noises,
                                        sine_noises=sines, front_batch=0, overlap=False)
    for k in range(K):
        assert torch.equal(waves[k], want[k]), "sentence %d" % k
    assert torch.equal(s_last, s_prev) and not torch.equal(waves[0], plain[0]) and torch.equal(waves[2], plain[2])  # row 2 is neutral
    # the capacity-bound path: two front groups, each a slice of the rows
    T_cap = 704
    cap = dict(diffusion_steps=STEPS, noises=noises, step_noises=step_noises, sine_noises=[s[0] for s in sines], max_frames=T_cap, pack="s16")
    results, _ = pipeline.synthesize_long(model, sampler, sentences, front_batch=(2, 0), intonation=it, **cap)
    assert [r.frames.numel() for r in results] == [2, 1]
    s_prev = None
    for (i, j), res in zip(((0, 2), (2, 3)), results):
        npad = max(LENS[i:j])
        tk = torch.zeros((j - i, npad), dtype=torch.long, device=DEV)
        for r, k in enumerate(range(i, j)):
            tk[r, :LENS[k]] = sentences[k]
        sine = torch.zeros((j - i, 600 * T_cap, 9), device=DEV)
        for r, k in enumerate(range(i, j)):
            sine[r, :sines[k].shape[1]] = sines[k][0]
        own = pipeline.Intonation(j - i, range=per_row["range"][i:j], contour=per_row["contour"][i:j])
        ref = pipeline.inference(model, sampler, tk, input_lengths=torch.LongTensor(list(LENS[i:j])), noise=torch.cat(noises[i:j]),
                                 step_noise=torch.cat(step_noises[i:j], dim=1), sine_noise=sine, diffusion_steps=STEPS, lj_tail=False,
                                 max_frames=T_cap, pack="s16", trim=0, passage=True, s_prev=s_prev, intonation=own)
        assert torch.equal(res.wave, ref.wave) and torch.equal(res.pitch, ref.pitch) and _same_packed(res, ref), (i, j)
        s_prev = ref.style[-1:]
    torch.cuda.synchronize()
    ops.check_status()
