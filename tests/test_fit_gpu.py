"""Fit to duration on the device: `st2_durations_fit` against the numpy contract of tests/_fit_ref.py, bit
for bit in `out` and `report`, over every path the kernel has -- one and two tokens per thread, short rows, ties, the flat-row
fallback, every flag, in place --, a row's result independent of its place and of the batch, and the wiring:
`inference(fit_frames=)`, `GraphedSynthesis(fit=True)` and `synthesize_long(fit_frames=)` hand over exactly the frames asked for."""
import functools

import numpy as np
import pytest
import torch

import _fit_ref as R
from styletts2_amd import ops, pipeline
from test_controls_gpu import CAPACITY_BITS, LENS, STEPS, _batch, _kw, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -0x5A5A5A5A5A5A5A5A
BIG = 2 ** 31 - 1
T_CAP = 96  # the end-to-end capacity in frames -- more where a row's own prediction is longer: the synthetic weights predict some
#             25 frames per token, and a row that is left alone must not be truncated


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _device_fit(dur, lens, target, hold, T_cap, hold_dtype=torch.uint8, in_place=False):
    d = torch.tensor(np.asarray(dur, dtype=np.int64), device=DEV)
    B, N = d.shape
    out = d if in_place else torch.full((B, N), SENTINEL, dtype=torch.int64, device=DEV)
    rep = torch.full((B, 4), -77, dtype=torch.int32, device=DEV)
    h = None if hold is None else torch.tensor(np.asarray(hold, dtype=np.uint8), device=DEV).to(hold_dtype)
    o, r = ops.durations_fit(d, _i32(target), T_cap, lengths=None if lens is None else _i32(lens), hold=h, out=out, report=rep)
    assert o is out and r is rep
    return out.cpu().numpy(), rep.cpu().numpy()


def _check(dur, lens, target, hold, T_cap, what, flags=None):
    """One batch against the contract, out of place into a sentinel-filled `out`, then in place, then -- without `hold` -- with
    an all-zero one, and -- with it -- as bool."""
    want_o, want_r = R.fit(dur, lens, target, hold, T_cap)
    got_o, got_r = _device_fit(dur, lens, target, hold, T_cap)
    assert np.array_equal(got_r, want_r), (what, got_r.tolist(), want_r.tolist())
    assert np.array_equal(got_o, want_o), (what, np.argwhere(got_o != want_o)[:4].tolist())
    assert (got_o != SENTINEL).all()
    if flags is not None:
        assert want_r[:, 2].tolist() == list(flags), (what, want_r.tolist())
    in_o, in_r = _device_fit(dur, lens, target, hold, T_cap, in_place=True)
    assert np.array_equal(in_o, want_o) and np.array_equal(in_r, want_r), what + ": in place"
    B, N = want_o.shape
    other = _device_fit(dur, lens, target, np.zeros((B, N)), T_cap) if hold is None else _device_fit(dur, lens, target, hold, T_cap, torch.bool)
    assert np.array_equal(other[0], want_o) and np.array_equal(other[1], want_r), what + ": hold as zeros / as bool"
    return want_r


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 64, 65, 511, 512])
def test_kernel_equals_the_contract_bit_for_bit(N, B):
    rng = np.random.default_rng(1000 * N + B)
    rows = lambda v: [list(v) for _ in range(B)]
    dur = rng.integers(0, 20, size=(B, N))  # zeros count as one frame
    S = np.maximum(dur, 1).sum(axis=1)
    cap = int(3 * S.max())
    spread = lambda *v: [v[b % len(v)] for b in range(B)]
    # random rows at full length and at lengths 0, 1 and N; targets from far below lo to far above S
    for lens in (None, spread(N, 0, 1), spread(1, N, 0), spread(0, 1, N)):
        for scale in (0.3, 1.0, 1.7):
            _check(dur, lens, [max(int(scale * s), 1) for s in S], None, cap, "random, lens %s, x %.1f" % (lens, scale))
    hold = (rng.random((B, N)) < 0.3).astype(np.uint8)
    _check(dur, None, [int(1.4 * s) for s in S], hold, cap, "random with held tokens")
    # all durations equal: every remainder ties, the index decides; all ones: the M = 0 fallback
    _check(rows([3] * N), None, [3 * N + N // 2 + 1] * B, None, 4 * N + 8, "all equal", [0] * B)
    _check(rows([3] * N), None, [2 * N + N // 3] * B, None, 4 * N + 8, "all equal, shrinking", [0] * B)
    _check(rows([1] * N), None, [N + N // 3 + 1] * B, None, 4 * N + 8, "all ones", [0] * B)
    # target = len, = S, = T_cap, > T_cap
    eq = R.fit(dur, None, S.tolist(), None, cap)
    assert np.array_equal(eq[0], np.maximum(dur, 1))
    for name, target, flag in (("len", [N] * B, 0), ("S", S.tolist(), 0), ("T_cap", [cap] * B, 0), ("past T_cap", [cap + 5] * B, 1)):
        _check(dur, None, target, None, cap, "target = " + name, [flag] * B)
    # below lo with held tokens: the nearest feasible total; all held; lo > T_cap; a forced total past 2^31 - 1
    lo = np.where(hold != 0, np.maximum(dur, 1), 1).sum(axis=1)
    if (hold == 0).any(axis=1).all():
        _check(dur, None, [max(int(v) - 2, 1) for v in lo], hold, cap, "below lo", [0 if v == 1 else 1 for v in lo])
    _check(dur, None, [int(s) + 4 for s in S], np.ones((B, N)), cap, "all held", [2] * B)
    heavy = np.array(rows([50] * N))
    _check(heavy, None, [60] * B, np.ones((B, N)) if N == 1 else np.tile(np.arange(N) > 0, (B, 1)), 49 if N == 1 else 50 * N - 50,
           "lo > T_cap", [3] * B)  # lo = 50 (N - 1) + 1
    if N >= 2:
        forced = np.array(rows([BIG, BIG] + [1] * (N - 2)), dtype=np.int64)
        r = _check(forced, None, [100] * B, None, BIG, "2^31 - 1 twice", [3] * B)
        assert r[:, :2].tolist() == [[BIG, BIG]] * B
    _check(np.array(rows([BIG] + [0] * (N - 1)), dtype=np.int64), spread(1, N), [BIG] * B, None, BIG, "one token of 2^31 - 1")
    # rows with target 0 between fitted ones: copied whole, tail included, into the sentinel-filled out
    target = [int(1.5 * s) if b % 2 == 0 else 0 for b, s in enumerate(S)] if B > 1 else [0]
    r = _check(dur, spread(N, max(N - 1, 0), N), target, None, cap, "target 0 between fitted rows")
    assert r[:, 3].tolist()[1 if B > 1 else 0] == 0
    torch.cuda.synchronize()
    ops.check_status()


def test_a_rows_result_depends_on_that_row_alone():
    rng = np.random.default_rng(7)
    for N in (5, 300):
        dur = rng.integers(1, 25, size=(3, N))
        hold = (rng.random((3, N)) < 0.2).astype(np.uint8)
        lens, target = [N, N - 1, max(N - 3, 1)], [3 * N, 7 * N, 11 * N]
        o3, r3 = _device_fit(dur, lens, target, hold, 12 * N)
        pick = [2, 0]
        o2, r2 = _device_fit(dur[pick], [lens[k] for k in pick], [target[k] for k in pick], hold[pick], 12 * N)
        assert np.array_equal(o2, o3[pick]) and np.array_equal(r2, r3[pick])
        assert np.array_equal(o3, R.fit(dur, lens, target, hold, 12 * N)[0])


# ---- wiring ------------------------------------------------------------------------------------------------------------------------
def _same_rows(got, want, what):
    assert [len(r) for r in got] == [len(r) for r in want], what
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), "%s: row %d differs in %d of %d samples" % (what, k, int((x != y).sum()), len(x))


@functools.lru_cache(maxsize=None)
def _setup(tag):
    """The three-row batch of a tag once, with the frames its rows have on their own and a capacity that holds them."""
    man, model, sampler = _model(tag)
    b = _batch(bool(man["config"]["multispeaker"]))
    natural = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))["durations"].sum(dim=1).tolist()
    return model, sampler, b, max(T_CAP, (max(natural) + 31) // 32 * 32), natural


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_inference_hands_over_the_frames_asked_for(tag, monkeypatch):
    model, sampler, b, cap, natural = _setup(tag)
    B, N = b["tokens"].shape
    sine = b["sine"][:, :600 * cap]
    kw = _kw(b, sine_noise=sine, max_frames=cap, pack="s16", marks=True)
    torch.cuda.synchronize()
    ops.status(clear=True)
    calls = []
    real = ops.durations_fit
    monkeypatch.setattr(ops, "durations_fit", lambda *a, **k: calls.append(1) or real(*a, **k))
    plain = pipeline.inference(model, sampler, b["tokens"], **kw)
    plain_rows = [r.copy() for r in plain.to_host()]
    assert calls == [] and plain.fit is None  # without the arguments the launch is never issued
    assert plain.frames.cpu().tolist() == natural
    # feasible; leave alone; fewer frames than row 2 has tokens: the nearest feasible total is one each
    targets = [64 if natural[0] != 64 else 63, 0, 5]
    assert LENS[0] <= targets[0] <= cap and LENS[2] > 5
    res = pipeline.inference(model, sampler, b["tokens"], fit_frames=targets, **kw)
    assert calls == [1]
    rows, marks = res.to_host(marks=True)
    rows = [r.copy() for r in rows]
    fit = res.fit.cpu().tolist()
    frames = res.frames.cpu().tolist()
    print(tag, "natural frames", natural, "fit", fit)
    assert [f[2] for f in fit] == [0, 0, 1] and frames == [targets[0], natural[1], LENS[2]] == [f[1] for f in fit]
    assert [f[0] for f in fit][:2] == natural[:2] and fit[1][3] == 0
    offs = res.offsets.cpu().tolist()
    assert [offs[k + 1] - offs[k] for k in range(B)] == [600 * f - res.trim for f in frames]
    assert marks[:, N].tolist() == [600 * f - res.trim for f in frames] and (np.diff(marks.astype(np.int64), axis=1) >= 0).all()
    # the fitted durations forced on a second call, with the same explicit noise: the same bytes
    p = pipeline.prepare(model, sampler, b["tokens"], max_frames=cap, fit=(_i32(targets), None), **_kw(b))
    want_d, want_r = R.fit(pipeline.prepare(model, sampler, b["tokens"], max_frames=cap, **_kw(b))["durations"].cpu().numpy(),
                           list(LENS), targets, None, cap)
    assert np.array_equal(p["durations"].cpu().numpy(), want_d) and np.array_equal(p["fit"].cpu().numpy(), want_r)
    assert p["durations"].sum(dim=1).tolist() == frames
    forced = pipeline.inference(model, sampler, b["tokens"], durations=p["durations"], **kw)
    assert forced.frames.cpu().tolist() == frames
    _same_rows(forced.to_host(), rows, "forced fitted durations")
    # a row with target 0 is the row of the call without fit_frames, within one batch shape
    assert np.array_equal(rows[1], plain_rows[1]) and len(rows[0]) != len(plain_rows[0])
    # a device tensor is never judged on the host: past the capacity the kernel takes the capacity and says so
    far = pipeline.inference(model, sampler, b["tokens"], fit_frames=_i32([cap + 40, 0, 0]), **kw)
    assert far.frames.cpu().tolist()[0] == cap and far.fit.cpu().tolist()[0][1:3] == [cap, 1]
    # held tokens keep their predicted durations
    hold = torch.zeros((B, N), dtype=torch.bool, device=DEV)
    hold[0, :4] = True
    near = natural[0] - 20  # (the four held tokens alone may be longer than targets[0])
    held = pipeline.inference(model, sampler, b["tokens"], fit_frames=[near, 0, 0], fit_hold=hold, **kw)
    assert held.frames.cpu().tolist()[0] == near and held.fit.cpu().tolist()[0][:3] == [natural[0], near, 0]
    assert 0 < held.fit.cpu().tolist()[0][3] <= LENS[0] - 4
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_one_graph_serves_any_targets():
    model, sampler, b, T_CAP, _ = _setup("ljspeech")
    B, N = b["tokens"].shape
    ld = b["lengths"].to(torch.int32).to(DEV)
    sine = b["sine"][:, :600 * T_CAP].contiguous()
    plain = pipeline.GraphedSynthesis(model, sampler, B, N, T_CAP, STEPS, pack="s16")
    assert "fit_frames" not in plain.static and "fit_hold" not in plain.static
    for kw in (dict(fit_frames=[64, 0, 0]), dict(fit_hold=torch.zeros((B, N), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError, match="built without fit"):
            plain(**kw)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_CAP, STEPS, pack="s16", fit=True)
    assert gs.static["fit_frames"].dtype == torch.int32 and gs.static["fit_frames"].tolist() == [0] * B
    assert gs.static["fit_hold"].dtype == torch.uint8 and tuple(gs.static["fit_hold"].shape) == (B, N) and not gs.static["fit_hold"].any()
    with pytest.raises(ValueError, match="fit_frames must"):
        gs(fit_frames=[64, 0])
    with pytest.raises(ValueError, match="fit_frames must"):
        gs(fit_frames=[T_CAP + 1, 0, 0])
    noise = dict(noise=b["noise"], step_noise=b["step_noise"], sine_noise=sine)
    eager = lambda t: pipeline.inference(model, sampler, b["tokens"], lengths_dev=ld, max_frames=T_CAP, pack="s16",
                                         diffusion_steps=STEPS, fit_frames=t, **noise)
    torch.cuda.synchronize()
    ops.status(clear=True)
    graph = None
    for targets in ([64, 0, 30], [20, T_CAP, 0], _i32([50, 40, 3])):
        res = gs(tokens=b["tokens"], lengths=ld, fit_frames=targets, **noise)
        rows, fit, frames = [r.copy() for r in res.to_host()], res.fit.cpu().tolist(), res.frames.cpu().tolist()
        want = eager(targets)
        _same_rows(rows, want.to_host(), "replay under %s" % (targets,))
        assert fit == want.fit.cpu().tolist() and frames == want.frames.cpu().tolist()
        host = targets.tolist() if torch.is_tensor(targets) else targets
        assert all(f == t for f, t, row in zip(frames, host, fit) if t and row[2] == 0) and [row[2] for row in fit].count(0) >= 2
        graph = graph or gs._g["graph"]
        assert gs._g["graph"] is graph, "no re-record"
    again = gs(tokens=b["tokens"], lengths=ld, **noise)  # a call without targets replays the ones the graph holds
    assert again.frames.cpu().tolist() == frames
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_synthesize_long_fits_every_sentence_to_its_own_target():
    model, sampler, b, cap, _ = _setup("ljspeech")
    sentences = [b["tokens"][k, :LENS[k]].clone() for k in range(3)]
    targets = [LENS[0] + 30, 0, LENS[2] + 11]
    common = dict(diffusion_steps=STEPS, max_frames=2 * cap, pack="s16", front_batch=2, seeds=5)  # (the carried style moves row 1)
    torch.cuda.synchronize()
    ops.status(clear=True)
    plain, _ = pipeline.synthesize_long(model, sampler, sentences, **common)
    natural = [f for r in plain for f in r.frames.cpu().tolist()]
    for given in (targets, _i32(targets)):
        got, _ = pipeline.synthesize_long(model, sampler, sentences, fit_frames=given, **common)
        assert len(got) == 2 and all(r.fit is not None for r in got)
        frames = [f for r in got for f in r.frames.cpu().tolist()]
        fit = [row for r in got for row in r.fit.cpu().tolist()]
        assert frames == [targets[0], natural[1], targets[2]] and [row[2] for row in fit] == [0, 0, 0], (frames, natural, fit)
        lens = [len(x) for r in got for x in r.to_host()]
        assert lens == [600 * f - got[0].trim for f in frames]
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()
