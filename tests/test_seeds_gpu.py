"""Per-request seeds on the device: `st2_noise_fill` against the numpy contract of tests/_rng_ref.py -- the
raw words bit for bit, the normals within the budget of the fp32 functions they are made of and within the statistical bounds
the contract itself meets --, nothing written outside a row's limit, a row's draws independent of its place and of the batch,
and the wiring: `inference(seeds=)`, `GraphedSynthesis(seeds=True)` and `synthesize_long(seeds=)` give the bytes of the calls
with explicit noise made by the same fill."""
import functools

import numpy as np
import pytest
import torch

import _rng_ref as R
from styletts2_amd import ops, pipeline
from test_controls_gpu import CAPACITY_BITS, LENS, STEPS, T_SINE, _batch, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEDS3 = (0, -1, 2 ** 63 - 1)
SENTINEL = 0x5A5A5A5A  # as a float 1.5e16: no normal
SIZES = (0, 1, 3, 4, 5, 256, 1027)
NORMAL_BAR = 8.0 * 2.0 ** -24  # logf, sqrtf and sincospif at a few ulp each, two multiplies, on an exact angle


def _seeds(v):
    return torch.tensor(list(v), dtype=torch.int64, device=DEV)


def _filled(seeds, stream0, S, n, pad, shift, bits, counts=None, per_count=None):
    """One fill into a sentinel buffer: rows of n values `pad` apart, the first `shift` floats into the buffer, one row's room
    behind the last -> (the [S, B, n + pad] words of the rows, the words in front of and behind them), as uint32."""
    B, stride = len(seeds), n + pad
    buf = torch.full((shift + (S * B + 1) * stride,), SENTINEL, dtype=torch.int32, device=DEV)
    rows = buf[shift:shift + S * B * stride].view(S, B, stride)[:, :, :n]
    out = rows if bits else rows.view(torch.float32)
    c = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=DEV)
    ops.noise_fill(_seeds(seeds), out if S > 1 else out[0], stream0, counts=c, per_count=per_count, bits=bits,
                   streams=S if S > 1 else None)
    host = buf.cpu().numpy().view(np.uint32)
    body = host[shift:shift + S * B * stride].reshape(S, B, stride)
    return body, np.concatenate([host[:shift], host[shift + S * B * stride:]])


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("stream0", [0, 1, 0x10000])
@pytest.mark.parametrize("pad,shift", [(0, 0), (7, 0), (8, 1)], ids=["dense", "strided", "offset-by-one-float"])
def test_bits_equal_the_contract_word_for_word_and_nothing_else_is_written(S, stream0, pad, shift):
    for n in SIZES:
        got, around = _filled(SEEDS3, stream0, S, n, pad, shift, bits=True)
        want, _ = R.fill(SEEDS3, stream0, S, n, kind="bits")
        assert np.array_equal(got[:, :, :n], want), (n, np.argwhere(got[:, :, :n] != want)[:4])
        assert (got[:, :, n:] == SENTINEL).all() and (around == SENTINEL).all(), "n = %d: padding or a neighbour was written" % n


@pytest.mark.parametrize("bits", [True, False])
@pytest.mark.parametrize("pad,shift", [(4, 0), (3, 1)], ids=["aligned", "unaligned"])
def test_counts_bound_what_a_row_receives(bits, pad, shift):
    counts, per_count, n = [0, 1, 2], 5, 12
    got, around = _filled(SEEDS3, R.SINE, 1, n, pad, shift, bits, counts=counts, per_count=per_count)
    want, written = R.fill(SEEDS3, R.SINE, 1, n, counts=counts, per_count=per_count, kind="bits")
    assert written.sum(axis=2).tolist() == [[0, 5, 10]]
    assert (got[:, :, :n][~written] == SENTINEL).all() and (got[:, :, n:] == SENTINEL).all() and (around == SENTINEL).all()
    assert (got[:, :, :n][written] != SENTINEL).all()
    if bits:
        assert np.array_equal(got[:, :, :n][written], want[written])
    # a count past the row, a negative one and a huge per_count: the row's n values, none, and no overflow
    got, around = _filled(SEEDS3, R.SINE, 1, n, pad, shift, True, counts=[2 ** 31 - 1, -3, 1], per_count=2 ** 62)
    want, written = R.fill(SEEDS3, R.SINE, 1, n, counts=[3, 0, 3], per_count=5, kind="bits")
    assert written.sum(axis=2).tolist() == [[12, 0, 12]] and np.array_equal(got[:, :, :n][written], want[written])
    assert (got[:, :, :n][~written] == SENTINEL).all() and (around == SENTINEL).all()


@pytest.mark.parametrize("S,stream0", [(1, 0), (4, 1), (1, 0x10000)])
@pytest.mark.parametrize("pad,shift", [(0, 0), (8, 1)], ids=["dense", "offset-by-one-float"])
def test_normals_stay_within_the_budget_of_their_fp32_functions(S, stream0, pad, shift):
    worst = 0.0
    for n in SIZES:
        got, around = _filled(SEEDS3, stream0, S, n, pad, shift, bits=False)
        want, _ = R.fill(SEEDS3, stream0, S, n)
        z = got[:, :, :n].view(np.float32).astype(np.float64)
        err = np.abs(z - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, float(err.max()) if n else 0.0)
        assert (err <= NORMAL_BAR).all(), (n, float(err.max()) / 2.0 ** -24)
        assert (got[:, :, n:] == SENTINEL).all() and (around == SENTINEL).all()
    print("normals, S = %d from stream %#x: max |z - z_ref| / max(1, |z_ref|) = %.2f x 2^-24" % (S, stream0, worst / 2.0 ** -24))


@functools.lru_cache(maxsize=None)
def _stat_fill(seed):
    """One 2^20-element device fill per noise stream under `seed` and under seed + 1 -> fp64 rows on the host."""
    seeds = _seeds([seed, seed + 1])
    out = torch.empty((2, 2, R.STAT_N), device=DEV)
    ops.noise_fill(seeds, out, R.SAMPLER, streams=2)  # streams 0 and 1
    sine = ops.noise_fill(seeds[:1], torch.empty((1, R.STAT_N), device=DEV), R.SINE)
    return out.cpu().numpy().astype(np.float64), sine.cpu().numpy().astype(np.float64)[0]


@pytest.mark.parametrize("seed", R.STAT_SEEDS)
def test_device_normals_meet_the_statistical_bounds_of_the_contract(seed):
    z, sine = _stat_fill(seed)
    for s, name in ((0, "sampler"), (1, "step")):
        st = R.stats(z[s, 0], z[1, 0] if s == 0 else None)  # streams 0 and 1 of one seed
        print("seed %d %s: %s" % (seed, name, st))
        R.check_stats(st, (seed, name))
    R.check_stats(R.stats(z[0, 0], z[0, 1]), (seed, "k and k + 1"))
    R.check_stats(R.stats(sine), (seed, "sine"))
    assert np.abs(z).max() <= 5.9 and np.isfinite(z).all()
    # and the whole 2^20 against the fp64 contract: the tails of u1 next to 0 and to 1 are in here
    want = R.normals(seed, R.SAMPLER, R.STAT_N)
    err = np.abs(z[0, 0] - want) / np.maximum(1.0, np.abs(want))
    print("seed %d: 2^20 normals, max error %.2f x 2^-24, smallest |z_ref| %.3g" % (seed, err.max() / 2.0 ** -24, np.abs(want).min()))
    assert (err <= NORMAL_BAR).all()


def test_a_rows_draws_depend_on_its_seed_alone():
    a, b, c = 11, -5, 2 ** 40 + 3
    for stream0, S, n3, n2 in ((R.SAMPLER, 1, 256, 256), (R.STEP, STEPS - 1, 256, 256), (R.SINE, 1, 5400 * 7, 5400 * 12)):
        for bits in (True, False):
            dt = torch.int32 if bits else torch.float32
            o3 = ops.noise_fill(_seeds([a, b, c]), torch.empty((S, 3, n3), dtype=dt, device=DEV), stream0, bits=bits, streams=S)
            o2 = ops.noise_fill(_seeds([c, a]), torch.empty((S, 2, n2), dtype=dt, device=DEV), stream0, bits=bits, streams=S)
            m = min(n2, n3)  # another max_frames is another n: the common prefix is the same
            o3, o2 = o3.view(torch.int32), o2.view(torch.int32)
            assert torch.equal(o2[:, 0, :m], o3[:, 2, :m]) and torch.equal(o2[:, 1, :m], o3[:, 0, :m]), (stream0, bits)
            assert not torch.equal(o3[:, 0, :m], o3[:, 1, :m])


# ---- wiring ------------------------------------------------------------------------------------------------------------------------
WIRE_SEEDS = (3, 2 ** 63 - 1, -17)


@functools.lru_cache(maxsize=None)
def _wired(tag):
    """The three-row batch of a tag under WIRE_SEEDS once: the noise of the header's stream ids made by the fill, the capacity
    read from a front run under it, and the result of the call with that noise given explicitly."""
    man, model, sampler = _model(tag)
    multi = bool(man["config"]["multispeaker"])
    b = _batch(multi)
    B = len(LENS)
    seeds = _seeds(WIRE_SEEDS)
    noise = ops.noise_fill(seeds, torch.empty((B, 1, 256), device=DEV), ops.NOISE_SAMPLER)
    step = ops.noise_fill(seeds, torch.empty((STEPS - 1, B, 1, 256), device=DEV), ops.NOISE_STEP, streams=STEPS - 1)
    kw = dict(input_lengths=b["lengths"], diffusion_steps=STEPS, ref_s=b["ref_s"])
    p = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, noise=noise, step_noise=step, **kw)
    tot = p["frames_host"]
    T_cap = (max(tot) + 63) // 64 * 64
    assert len(set(tot)) > 1 and min(tot) < T_cap <= T_SINE, tot  # a row of fewer frames than the capacity
    sine = ops.noise_fill(seeds, torch.empty((B, 600 * T_cap, 9), device=DEV), ops.NOISE_SINE)
    torch.cuda.synchronize()
    ops.status(clear=True)
    want = pipeline.inference(model, sampler, b["tokens"], max_frames=T_cap, pack="s16", noise=noise, step_noise=step,
                              sine_noise=sine, **kw)
    rows = [r.copy() for r in want.to_host()]
    assert want.frames.cpu().tolist() == tot
    return dict(model=model, sampler=sampler, b=b, seeds=seeds, noise=noise, step=step, sine=sine, T=T_cap, kw=kw, rows=rows,
                frames=tot)


def _same_rows(got, want, what):
    assert [len(r) for r in got] == [len(r) for r in want], what
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), "%s: row %d differs in %d of %d samples" % (what, k, int((x != y).sum()), len(x))


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_inference_with_seeds_is_the_call_with_the_fills_noise(tag):
    W = _wired(tag)
    model, sampler, b, T = W["model"], W["sampler"], W["b"], W["T"]
    for seeds in (W["seeds"], list(WIRE_SEEDS)):  # on the device, or a host sequence
        res = pipeline.inference(model, sampler, b["tokens"], max_frames=T, pack="s16", seeds=seeds, **W["kw"])
        assert res.frames.cpu().tolist() == W["frames"]
        _same_rows(res.to_host(), W["rows"], "B = 3")
    # B = 2, the rows permuted, at another capacity: against explicit rows gathered from the B = 3 fill
    perm = [2, 0]
    T2 = T + 64
    sine2 = torch.zeros((2, 600 * T2, 9), device=DEV)
    sine2[:, :600 * T] = W["sine"][perm]
    kw2 = dict(input_lengths=b["lengths"][perm], diffusion_steps=STEPS, ref_s=None if b["ref_s"] is None else b["ref_s"][perm].contiguous())
    tokens2 = b["tokens"][perm].contiguous()
    want = pipeline.inference(model, sampler, tokens2, max_frames=T2, pack="s16", noise=W["noise"][perm].contiguous(),
                              step_noise=W["step"][:, perm].contiguous(), sine_noise=sine2, **kw2)
    want_rows = [r.copy() for r in want.to_host()]
    got = pipeline.inference(model, sampler, tokens2, max_frames=T2, pack="s16", seeds=[WIRE_SEEDS[k] for k in perm], **kw2)
    _same_rows(got.to_host(), want_rows, "B = 2, permuted")
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_one_graph_serves_any_seeds():
    W = _wired("ljspeech")
    model, sampler, b, T = W["model"], W["sampler"], W["b"], W["T"] + 64  # room for the other seeds' durations
    B, N = b["tokens"].shape
    ld = b["lengths"].to(torch.int32).to(DEV)
    plain = pipeline.GraphedSynthesis(model, sampler, B, N, T, STEPS, pack="s16")
    assert "seeds" not in plain.static and plain.static["sine_noise"].shape == (B, 600 * T, 9)
    with pytest.raises(ValueError, match="built without seeds"):
        plain(seeds=list(WIRE_SEEDS))
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T, STEPS, pack="s16", seeds=True)
    assert gs.static["seeds"].dtype == torch.int64 and gs.static["seeds"].tolist() == [0] * B
    assert all(gs.static[k] is None for k in ("noise", "step_noise", "sine_noise"))
    for name in ("noise", "step_noise", "sine_noise"):
        with pytest.raises(ValueError, match="one or the other"):
            gs(**{name: W[{"noise": "noise", "step_noise": "step", "sine_noise": "sine"}[name]]})
    with pytest.raises(ValueError, match="seeds must be"):
        gs(seeds=[1, 2])
    eager = lambda s: pipeline.inference(model, sampler, b["tokens"], lengths_dev=ld, max_frames=T, pack="s16", diffusion_steps=STEPS,
                                         seeds=s)
    torch.cuda.synchronize()
    ops.status(clear=True)
    seen = {}
    other = [WIRE_SEEDS[0], 1234, WIRE_SEEDS[2]]  # row 1 alone changes
    for s in (list(WIRE_SEEDS), other, [7, 8, 9], _seeds(WIRE_SEEDS)):
        res = gs(tokens=b["tokens"], lengths=ld, seeds=s)
        rows = [r.copy() for r in res.to_host()]
        graph = gs._g["graph"]
        _same_rows(rows, eager(s).to_host(), "replay under %s" % (s,))
        seen[tuple(int(v) for v in (s.tolist() if torch.is_tensor(s) else s))] = rows
    assert gs._g["graph"] is graph, "no re-record"
    again = gs().to_host()  # a call without seeds replays the ones it holds
    _same_rows(again, seen[WIRE_SEEDS], "the same seeds again")
    for k in range(B):
        x, y = seen[WIRE_SEEDS][k], seen[(7, 8, 9)][k]
        assert len(x) != len(y) or not np.array_equal(x, y), "row %d does not depend on its seed" % k
    # a row's bytes do not depend on its neighbour's seed -- as they do not depend on its neighbour's explicit noise
    assert np.array_equal(seen[WIRE_SEEDS][0], seen[tuple(other)][0]) and np.array_equal(seen[WIRE_SEEDS][2], seen[tuple(other)][2])
    assert not np.array_equal(seen[WIRE_SEEDS][1], seen[tuple(other)][1])
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()


def test_with_explicit_noise_a_row_does_not_depend_on_its_neighbours_draws():
    """The property the seeded graph's row check rests on, on the path that takes explicit noise."""
    W = _wired("ljspeech")
    model, sampler, b, T = W["model"], W["sampler"], W["b"], W["T"] + 64
    B = len(LENS)

    def run(seeds):
        seeds = _seeds(seeds)
        noise = ops.noise_fill(seeds, torch.empty((B, 1, 256), device=DEV), ops.NOISE_SAMPLER)
        step = ops.noise_fill(seeds, torch.empty((STEPS - 1, B, 1, 256), device=DEV), ops.NOISE_STEP, streams=STEPS - 1)
        sine = ops.noise_fill(seeds, torch.empty((B, 600 * T, 9), device=DEV), ops.NOISE_SINE)
        res = pipeline.inference(model, sampler, b["tokens"], max_frames=T, pack="s16", noise=noise, step_noise=step, sine_noise=sine,
                                 **W["kw"])
        return [r.copy() for r in res.to_host()]
    one, two = run(WIRE_SEEDS), run([WIRE_SEEDS[0], 1234, WIRE_SEEDS[2]])  # row 1's draws alone change
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2]) and not np.array_equal(one[1], two[1])
    torch.cuda.synchronize()
    ops.check_status()


def test_synthesize_long_with_seeds_is_the_call_with_per_sentence_noise_from_the_fill():
    from test_passage_gpu import _passage
    P = _passage("libritts")
    model, sampler = P["model"], P["sampler"]
    sentences, K, T = P["sentences"][:3], 3, P["T"] + 64
    first = 2 ** 63 - 2  # the expansion wraps inside the passage
    rows = pipeline.seed_rows(first, K)
    assert rows == [2 ** 63 - 2, 2 ** 63 - 1, -2 ** 63]
    one = lambda k, shape, stream0, **kw: ops.noise_fill(_seeds([rows[k]]), torch.empty(shape, device=DEV), stream0, **kw)
    noises = [one(k, (1, 1, 256), ops.NOISE_SAMPLER) for k in range(K)]
    step_noises = [one(k, (STEPS - 1, 1, 1, 256), ops.NOISE_STEP, streams=STEPS - 1) for k in range(K)]
    sines = [one(k, (1, 600 * T, 9), ops.NOISE_SINE) for k in range(K)]
    common = dict(ref_s=P["ref_s"], diffusion_steps=STEPS, max_frames=T, pack="s16", trim=P["trim"], front_batch=2)
    torch.cuda.synchronize()
    ops.status(clear=True)
    want, s_want = pipeline.synthesize_long(model, sampler, sentences, noises=noises, step_noises=step_noises, sine_noises=sines,
                                            **common)
    want_rows = [x.copy() for r in want for x in r.to_host()]
    got, s_got = pipeline.synthesize_long(model, sampler, sentences, seeds=first, **common)
    _same_rows([x for r in got for x in r.to_host()], want_rows, "the passage")
    assert torch.equal(s_got, s_want) and len(got) == 2
    listed, _ = pipeline.synthesize_long(model, sampler, sentences, seeds=_seeds(rows), **common)
    _same_rows([x for r in listed for x in r.to_host()], want_rows, "K seeds on the device")
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == 0
    ops.check_status()
