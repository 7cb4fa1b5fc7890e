"""Per-request controls on the device: the three kernels against the numpy contract of
tests/_controls_ref.py and against the launches they replace, and the `controls=` paths of the pipeline against the paths without
them.  Shapes are the smallest at which the kernels can still go wrong: B = 3 right-padded rows of 12 / 9 / 7 tokens cut from
benchdata/val_phonemes_32.txt (about 25 frames per token with the seeded weights: rows of a few hundred frames), B = 4 and B = 1
for the carry scan.  Models and draws are built once per module."""
import functools
import warnings

import numpy as np
import pytest
import torch

import _controls_ref as R
from _util import manifest, rms
from benchdata import synth  # seeded synthetic weights (test + bench helper, not product code)
from styletts2_amd import _lib, models, ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAPACITY_BITS = _lib.STATUS_FRAME_CAPACITY | _lib.STATUS_DURATION_SUM  # what a truncated row raises
KEYS = ["decoder", "diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]
STEPS = 3
LENS = (12, 9, 7)
SPEEDS = (1.0, 0.8, 1.5)
T_SINE = 1024  # frames of pinned SineGen draws per row: more than any row here needs


@functools.lru_cache(maxsize=None)
def _model(tag):
    man = manifest(tag)
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    for i, k in enumerate(KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval()
        model[k].to(DEV)
    return man, model, models.make_sampler(model)


@functools.lru_cache(maxsize=None)
def _batch(multi, lens=LENS, seed=8):
    """Right-padded rows of `lens` tokens cut from the validation phonemes, with pinned draws, on the device."""
    import bench
    tokens, _, noise, _, _ = bench.ragged_inputs("cpu")
    B, N = len(lens), max(lens)
    tk = torch.zeros((B, N), dtype=torch.long)
    for b, n in enumerate(lens):
        tk[b, :n] = tokens[b, :n]
    g = torch.Generator().manual_seed(seed)
    step_noise = torch.randn(STEPS - 1, B, 1, 256, generator=g)
    ref_s = torch.randn(B, 256, generator=g) if multi else None
    sine = torch.randn(B, 600 * T_SINE, 9, generator=g)
    d = lambda t: None if t is None else t.to(DEV)
    return dict(tokens=d(tk), lengths=torch.LongTensor(list(lens)), noise=d(noise[:B].contiguous()), step_noise=d(step_noise),
                ref_s=d(ref_s), sine=d(sine))


def _kw(b, **more):
    return dict(input_lengths=b["lengths"], noise=b["noise"], diffusion_steps=STEPS, step_noise=b["step_noise"], ref_s=b["ref_s"],
                **more)


def _dev(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


# ---- 1. duration head with a per-row rate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 5])
def test_duration_head_rate_is_the_numpy_contract_bit_for_bit(tail):
    B, K, N, J = 3, 512, 24, 50
    lens = [24, 17, 1]
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(B, K, N, generator=g) * 0.5).to(DEV)
    w = (torch.randn(J, K, generator=g) / K ** 0.5).to(DEV)
    bias = (torch.randn(J, generator=g) * 0.5).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ops.status(clear=True)
    dur0, sums = ops.duration_head(x, w, bias, lengths=ld, tail=tail, want_sums=True)
    dur, sums_r = ops.duration_head(x, w, bias, lengths=ld, tail=tail, want_sums=True, speed=_dev(SPEEDS))
    total = sums.cpu().numpy()
    assert torch.equal(sums_r, sums), "the sums are formed before the division: unchanged"
    assert dur.dtype == torch.int64 and np.array_equal(dur.cpu().numpy(), R.durations(total, SPEEDS, lens, tail))
    assert np.array_equal(dur0.cpu().numpy(), R.durations(total, None, lens, tail))
    assert torch.equal(ops.duration_head(x, w, bias, lengths=ld, tail=tail, speed=_dev([1.0] * B)), dur0), "x / 1 is exact"
    assert not torch.equal(dur, dur0) and int(dur[2, 1:].abs().sum()) == 0 and int(dur[2, 0]) >= 1 + tail
    # device values out of range or NaN: the clamped / neutral row, no fault, no status bit
    bad = [0.0, 100.0, float("nan")]
    got = ops.duration_head(x, w, bias, lengths=ld, tail=tail, speed=_dev(bad))
    assert np.array_equal(got.cpu().numpy(), R.durations(total, bad, lens, tail))
    assert np.array_equal(got.cpu().numpy(), R.durations(total, [0.25, 4.0, 1.0], lens, tail))
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("J,speed,want", [(5, 1.0, 2), (7, 1.0, 4), (50, 1.0, 25), (5, 2.0, 1), (7, 2.0, 2), (50, 2.0, 12)])
def test_duration_head_rate_rounds_ties_to_even(J, speed, want):
    """w = 0, bias = 0: every sigmoid is exactly 0.5, the sum J / 2 exactly: 2.5 -> 2, 3.5 -> 4, 25 / 2 = 12.5 -> 12, 1.25 -> 1."""
    B, K, N = 2, 64, 3
    x = torch.randn(B, K, N, generator=torch.Generator().manual_seed(J)).to(DEV)
    w, bias = torch.zeros(J, K, device=DEV), torch.zeros(J, device=DEV)
    dur, sums = ops.duration_head(x, w, bias, want_sums=True, speed=_dev([speed] * B))
    assert sums.cpu().tolist() == [[J / 2.0] * N] * B
    assert dur.cpu().tolist() == [[want] * N] * B
    assert np.array_equal(dur.cpu().numpy(), R.durations(sums.cpu().numpy(), [speed] * B))


# ---- 2. style mixing as one launch --------------------------------------------------------------------------------------------
W3, W7 = float(np.float32(0.3)), float(np.float32(0.7))  # fp32 values handed to the scalar path as doubles: one value on both sides


def _by_launches(sp, s_prev, ref_s, t, alpha, beta, carry):
    """The st2_axpbypcz launches of the front plan (csrc/st2_plan_front.inc), row by row with row b's weights as the scalars of
    its launches; the plan's st2_copy_ncl launches move bits and are slices here."""
    B, C2 = sp.shape
    sty = C2 // 2
    rows = []
    for b in range(B):
        cur = sp[b:b + 1].contiguous()
        prev = (rows[-1] if b else s_prev) if carry else (None if s_prev is None else s_prev[b:b + 1].contiguous())
        if prev is not None:
            cur = ops.axpbypcz(prev, t[b], cur, 1.0 - t[b])
        if ref_s is not None:
            rs = ref_s[b:b + 1].contiguous()
            ma = ops.axpbypcz(cur, alpha[b], rs, 1.0 - alpha[b])
            mb = ops.axpbypcz(cur, beta[b], rs, 1.0 - beta[b])
            cur = torch.cat([ma[:, :sty], mb[:, sty:]], dim=1)
        rows.append(cur)
    return torch.cat(rows, dim=0)


def _ulp_err(got, exact, *operands):
    """max |got - exact| in fp32 ulps.  The unit is the spacing at the largest magnitude among the element's result and operands:
    a convex mix of values of opposite sign cancels, and its roundings (one per product, one per sum) are committed at the
    operands' scale, not at the result's."""
    scale = np.maximum.reduce([np.abs(exact)] + [np.abs(np.asarray(o, dtype=np.float64)) for o in operands])
    return float((np.abs(got.astype(np.float64) - exact) / np.spacing(scale.astype(np.float32)).astype(np.float64)).max())


@pytest.mark.parametrize("B,carry", [(3, False), (4, True), (1, True)])
@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("with_prev", [False, True])
def test_style_mix_rows_equals_the_launches_it_replaces(B, carry, with_ref, with_prev):
    sty, C2 = 128, 256
    g = torch.Generator().manual_seed(100 + 10 * B + 2 * with_ref + with_prev)
    sp = torch.randn(B, C2, generator=g).to(DEV)
    s_prev = torch.randn(1 if carry else B, C2, generator=g).to(DEV) if with_prev else None
    ref_s = torch.randn(B, C2, generator=g).to(DEV) if with_ref else None
    n = lambda v: None if v is None else v.cpu().numpy()
    # (a) scalar weights, no rows: the call's scalars for every row
    for t0, a0, b0 in ((0.25, 0.5, 0.75), (W7, W3, W7), (0.5, W7, 0.25)):
        ref, s, out = ops.style_mix_rows(sp, s_prev, ref_s, t0=t0, alpha0=a0, beta0=b0, carry=carry)
        want = _by_launches(sp, s_prev, ref_s, [t0] * B, [a0] * B, [b0] * B, carry)
        assert torch.equal(out, want) and torch.equal(ref, want[:, :sty]) and torch.equal(s, want[:, sty:]), (t0, a0, b0)
    # (b) weights that differ between the rows: every row is the scalar launches with that row's weights
    pool = [0.25, W3, 0.5, W7, 0.75]
    t = [pool[(b + 1) % 5] for b in range(B)]
    a = [pool[(2 * b) % 5] for b in range(B)]
    bt = [pool[(3 * b + 2) % 5] for b in range(B)]
    ref, s, out = ops.style_mix_rows(sp, s_prev, ref_s, t=_dev(t), alpha=_dev(a), beta=_dev(bt), t0=0.9, alpha0=0.9, beta0=0.9,
                                     carry=carry)
    want = _by_launches(sp, s_prev, ref_s, t, a, bt, carry)
    assert torch.equal(out, want) and torch.equal(ref, want[:, :sty]) and torch.equal(s, want[:, sty:])
    # ... and within 2 ulp of the same mix in float64
    e_ref, e_s = R.style_mix(n(sp), n(s_prev), n(ref_s), t, a, bt, carry=carry, exact=True)
    operands = [np.abs(n(sp))] + ([np.abs(np.broadcast_to(n(s_prev), (B, C2)))] if with_prev else []) + \
        ([np.abs(n(ref_s))] if with_ref else [])
    scale = np.maximum.reduce(operands)
    if carry:  # a row's previous style is bounded by the largest operand of the rows before it
        scale = np.maximum.accumulate(scale, axis=0)
    err = _ulp_err(out.cpu().numpy(), np.concatenate([e_ref, e_s], axis=1), scale)
    print("style_mix_rows B=%d carry=%d ref_s=%d s_prev=%d: max error %.3f ulp" % (B, carry, with_ref, with_prev, err))
    assert err <= 2.0
    got32 = R.style_mix(n(sp), n(s_prev), n(ref_s), t, a, bt, carry=carry)
    assert np.array_equal(out.cpu().numpy(), np.concatenate(got32, axis=1)), "the numpy statement of the contract, bit for bit"
    # (c) NaN rows are the call's scalars; out-of-range rows are clamped to [0, 1]
    nan = _dev([float("nan")] * B)
    assert torch.equal(ops.style_mix_rows(sp, s_prev, ref_s, t=nan, alpha=nan, beta=nan, t0=W7, alpha0=W3, beta0=0.5,
                                          carry=carry)[2], _by_launches(sp, s_prev, ref_s, [W7] * B, [W3] * B, [0.5] * B, carry))
    assert torch.equal(ops.style_mix_rows(sp, s_prev, ref_s, t=_dev([7.0] * B), alpha=_dev([-3.0] * B), beta=_dev([1.5] * B),
                                          carry=carry)[2], _by_launches(sp, s_prev, ref_s, [1.0] * B, [0.0] * B, [1.0] * B, carry))


# ---- 6a. the prosody-controls kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [True, False])
def test_prosody_controls_kernel_one_operation_per_element_and_nothing_past_the_row(ragged):
    B, T = 3, 700  # L = 1400: more than one workgroup per row (1024 columns each), not a multiple of it
    L = 2 * T
    frames = [700, 513, 1]
    g = torch.Generator().manual_seed(6)
    F0, N = torch.randn(B, L, generator=g) * 100 + 200, torch.randn(B, L, generator=g)
    N[0, 5], N[1, 0] = -0.0, -0.0
    if ragged:
        for b, f in enumerate(frames):  # poisoned tails: nothing of them may be read into a result or overwritten
            F0[b, 2 * f:] = float("nan")
            N[b, 2 * f:] = float("nan")
    sc, sh = [2.0, W7, 1.0], [0.0, -1.25, W3]
    fd = torch.tensor(frames, dtype=torch.int32, device=DEV) if ragged else None
    f0, n = ops.prosody_controls(F0.to(DEV), N.to(DEV), _dev(sc), _dev(sh), frames=fd)
    f0, n = f0.cpu(), n.cpu()
    bits = lambda t: t.contiguous().view(torch.int32)
    for b in range(B):
        e = 2 * frames[b] if ragged else L
        assert torch.equal(bits(f0[b, :e]), bits(F0[b, :e] * torch.tensor(sc[b]))), "row %d F0" % b
        want_n = N[b, :e] if sh[b] == 0 else N[b, :e] + torch.tensor(sh[b])
        assert torch.equal(bits(n[b, :e]), bits(want_n)), "row %d N" % b
        assert torch.equal(bits(f0[b, e:]), bits(F0[b, e:])) and torch.equal(bits(n[b, e:]), bits(N[b, e:])), "row %d tail" % b
    assert bool(torch.signbit(n[0, 5])) and n[0, 5] == 0, "-0.0 survives a zero shift"
    assert np.array_equal(f0.numpy().view(np.uint32), R.prosody(F0.numpy(), N.numpy(), sc, sh, frames if ragged else None)[0].view(np.uint32))
    # one curve alone; device values out of range / NaN are clamped where they are read
    f0b, nb = ops.prosody_controls(F0.to(DEV), N.to(DEV), None, _dev([9.0, float("nan"), -9.0]), frames=fd)
    wf, wn = R.prosody(F0.numpy(), N.numpy(), None, [2.0, 0.0, -2.0], frames if ragged else None)
    assert np.array_equal(f0b.cpu().numpy().view(np.uint32), wf.view(np.uint32))
    assert np.array_equal(nb.cpu().numpy().view(np.uint32), wn.view(np.uint32))
    f0c, _ = ops.prosody_controls(F0.to(DEV), N.to(DEV), _dev([0.0, float("nan"), 50.0]), None, frames=fd)
    assert np.array_equal(f0c.cpu().numpy().view(np.uint32),
                          R.prosody(F0.numpy(), N.numpy(), [0.5, 1.0, 2.0], None, frames if ragged else None)[0].view(np.uint32))


# ---- 3. neutral controls are the call without controls -----------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_neutral_controls_are_the_no_controls_call_bitwise(tag):
    man, model, sampler = _model(tag)
    b = _batch(bool(man["config"]["multispeaker"]))
    B = len(LENS)
    p0 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))
    tot = p0["frames_host"]
    assert len(set(tot)) > 1 and max(tot) < T_SINE, tot
    w0 = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, **_kw(b))
    T_cap = (max(tot) + 63) // 64 * 64
    c0 = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], max_frames=T_cap, **_kw(b))
    for ctl in (pipeline.Controls.neutral(B, alpha=0.3, beta=0.7, t=0.7), pipeline.Controls.neutral(B)):
        p1 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, controls=ctl, **_kw(b))
        for k in ("durations", "s_pred", "ref", "asr", "F0", "N", "frames"):
            assert torch.equal(p1[k], p0[k]), k
        w1 = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, controls=ctl, **_kw(b))
        assert all(torch.equal(x, y) for x, y in zip(w1, w0)) and [w.shape[-1] for w in w1] == [600 * t for t in tot]
        c1 = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], max_frames=T_cap, controls=ctl, **_kw(b))
        assert torch.equal(c1.frames, c0.frames) and torch.equal(c1.wave, c0.wave)
        for r in range(B):
            assert not bool(c1.wave[r, :, 600 * tot[r]:].any()), "row %d: tail not exactly zero" % r
    torch.cuda.synchronize()
    ops.check_status()


# ---- 4. per-row speed end to end -----------------------------------------------------------------------------------------------
def test_per_row_speed_end_to_end():
    man, model, sampler = _model("ljspeech")
    b = _batch(False)
    B = len(LENS)
    ld = b["lengths"].to(torch.int32).to(DEV)
    # the sums the duration head rounds: the duration BiLSTM + head of the front's own d, kernel by kernel
    f = pipeline._front_core(model, sampler, b["tokens"], b["lengths"], ld, b["noise"], b["step_noise"], None, None,
                             diffusion_steps=STEPS, embedding_scale=1.0, alpha=0.3, beta=0.7, t=0.7, predict=True, lj_tail=True)
    x = model.predictor.lstm.forward_cm(f["d"].transpose(1, 2).contiguous().float(), ld)
    lin = model.predictor.duration_proj.linear_layer
    dur1, sums = ops.duration_head(x, lin.weight.detach().float().contiguous(), lin.bias.detach().float().contiguous(), lengths=ld,
                                   tail=5, want_sums=True)
    assert torch.equal(dur1, f["durations"]), "the kernel-by-kernel duration stage is the plan's"
    want = torch.from_numpy(R.durations(sums.cpu().numpy(), SPEEDS, list(LENS), tail=5))
    ctl = pipeline.Controls(B, speed=SPEEDS)
    kw = _kw(b)
    p = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, controls=ctl, **kw)
    assert torch.equal(p["durations"].cpu(), want), "the durations of the numpy contract"
    tot, tot1 = p["frames_host"], dur1.sum(dim=1).tolist()
    assert tot == want.sum(dim=1).tolist() and len(set(tot)) == B and tot != tot1 and tot[0] == tot1[0]
    assert tot[1] > tot1[1] and tot[2] < tot1[2], (tot, tot1)  # 0.8 slows a row down, 1.5 speeds it up
    # the parent's own paths first: predicted durations and the same values forced agree bit for bit at speed 1 ...
    w_pred = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, **kw)
    w_forced = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, durations=dur1, **kw)
    for r in range(B):
        e = rms(w_pred[r] - w_forced[r])
        print("speed 1, row %d: predicted vs forced durations rms diff %.3e" % (r, e))
        assert torch.equal(w_pred[r], w_forced[r]), "row %d at speed 1" % r
    # ... so per-row speed equals the call with its durations forced, bit for bit
    w_ctl = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, controls=ctl, **kw)
    w_want = pipeline.inference(model, sampler, b["tokens"], sine_noise=b["sine"], ragged_decode=True, durations=want.to(DEV), **kw)
    assert [w.shape[-1] for w in w_ctl] == [600 * t for t in tot]
    for r in range(B):
        assert torch.equal(w_ctl[r], w_want[r]), "row %d" % r
    with pytest.raises(ValueError, match="nothing to scale"):
        pipeline.inference(model, sampler, b["tokens"], ragged_decode=True, durations=dur1, controls=ctl, **kw)
    torch.cuda.synchronize()
    ops.check_status()


# ---- 5. per-row alpha / beta ----------------------------------------------------------------------------------------------------
def test_per_row_alpha_beta_rows_equal_the_scalar_runs():
    man, model, sampler = _model("libritts")
    b = _batch(True)
    B = len(LENS)
    pairs = [(0.25, 0.75), (0.75, 0.25)]

    def run(**more):
        p = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b, **more))
        return p, pipeline._decode_ragged(model, p, b["sine"])
    scalar = [run(alpha=a, beta=bt) for a, bt in pairs]
    which = [r % 2 for r in range(B)]
    ctl = pipeline.Controls(B, alpha=[pairs[i][0] for i in which], beta=[pairs[i][1] for i in which])
    p, waves = run(controls=ctl, alpha=0.9, beta=0.1)  # the call's scalars are not what any row uses
    assert not torch.equal(scalar[0][0]["ref"], scalar[1][0]["ref"])
    for r in range(B):
        ps, ws = scalar[which[r]]
        for k in ("ref", "s_pred", "durations"):
            assert torch.equal(p[k][r], ps[k][r]), "row %d %s" % (r, k)
        assert p["frames_host"][r] == ps["frames_host"][r] and torch.equal(waves[r], ws[r]), "row %d waveform" % r
    torch.cuda.synchronize()
    ops.check_status()


# ---- 6b. pitch and energy through the pipeline -----------------------------------------------------------------------------------
def test_f0_scale_and_n_shift_through_prepare():
    man, model, sampler = _model("ljspeech")
    b = _batch(False)
    B = len(LENS)
    sc, sh = [1.5, W7, 1.0], [0.0, -0.75, W3]
    p0 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))
    p1 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True,
                          controls=pipeline.Controls(B, f0_scale=sc, n_shift=sh), **_kw(b))
    tot = p0["frames_host"]
    assert torch.equal(p1["asr"], p0["asr"]) and torch.equal(p1["durations"], p0["durations"]) and p1["frames_host"] == tot
    assert torch.equal(p1["s_pred"], p0["s_pred"])
    bits = lambda t: t.contiguous().view(torch.int32)
    for r in range(B):
        e = 2 * tot[r]
        assert torch.equal(bits(p1["F0"][r, :e]), bits(p0["F0"][r, :e] * _dev(sc[r]))), "row %d F0" % r
        want_n = p0["N"][r, :e] + _dev(sh[r]) if sh[r] else p0["N"][r, :e]
        assert torch.equal(bits(p1["N"][r, :e]), bits(want_n)), "row %d N" % r
        assert not bool(p1["F0"][r, e:].any()) and not bool(p1["N"][r, e:].any()), "row %d: exact zeros from 2 T_b on" % r
    assert not torch.equal(p1["F0"], p0["F0"]) and not torch.equal(p1["N"], p0["N"])
    # the uniform path (one frame count, no `frames`): every column of every row
    dur = torch.full((B, max(LENS)), 3, dtype=torch.long)
    u0 = pipeline.prepare(model, sampler, b["tokens"], durations=dur, **_kw(b))
    u1 = pipeline.prepare(model, sampler, b["tokens"], durations=dur, controls=pipeline.Controls(B, f0_scale=sc, n_shift=sh), **_kw(b))
    assert torch.equal(bits(u1["F0"]), bits(u0["F0"] * _dev(sc)[:, None])) and torch.equal(u1["asr"], u0["asr"])
    assert torch.equal(bits(u1["N"][1:]), bits(u0["N"][1:] + _dev(sh)[1:, None])) and torch.equal(bits(u1["N"][0]), bits(u0["N"][0]))
    # the waveform follows: a scaled pitch curve is another utterance
    w = pipeline._decode_ragged(model, p1, b["sine"])
    w0 = pipeline._decode_ragged(model, p0, b["sine"])
    assert all(bool(torch.isfinite(x).all()) for x in w) and not torch.equal(w[0], w0[0])
    torch.cuda.synchronize()
    ops.check_status()


# ---- 7. one graph, many requests ------------------------------------------------------------------------------------------------
def test_one_graph_serves_any_controls_and_reports_a_row_over_capacity():
    man, model, sampler = _model("ljspeech")
    b = _batch(False)
    B, N = b["tokens"].shape
    ld = b["lengths"].to(torch.int32).to(DEV)
    cases = [pipeline.Controls(B, speed=SPEEDS, f0_scale=[1.0, 1.25, 0.8]), pipeline.Controls.neutral(B), None,
             pipeline.Controls(B, speed=[0.8, 1.0, 2.0], n_shift=[0.5, 0.0, -0.5])]
    need = []  # the capacity: the slowest case's frames, from host-read runs, rounded up to 64
    for ctl in cases:
        p = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, controls=ctl, **_kw(b))
        need.append(p["frames_host"])
    T_cap = (max(max(n) for n in need) + 63) // 64 * 64
    assert len({tuple(n) for n in need}) == 3 and T_cap <= T_SINE, need  # neutral and omitted agree; the others differ
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS)
    records = []
    orig = gs._record
    gs._record = lambda: records.append(1) or orig()
    torch.cuda.synchronize()
    ops.status(clear=True)
    first = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    eager_kw = dict(noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"], lengths_dev=ld, diffusion_steps=STEPS,
                    max_frames=T_cap)
    for i, ctl in enumerate(cases):
        res = gs(controls=ctl, **(first if i == 0 else {}))
        torch.cuda.synchronize()
        eager = pipeline.inference(model, sampler, b["tokens"], controls=ctl, **eager_kw)
        torch.cuda.synchronize()
        assert res.frames.cpu().tolist() == need[i], (i, res.frames.cpu().tolist(), need[i])
        assert torch.equal(res.frames, eager.frames) and torch.equal(res.wave, eager.wave), "replay %d" % i
    assert len(records) == 1, "other controls never re-record"
    assert ops.status() & CAPACITY_BITS == 0
    # a row slowed past the capacity: truncated and reported; the other rows are the run in which every row fits
    fit = gs(controls=pipeline.Controls(B, speed=[1.0, 0.8, 1.5]))
    torch.cuda.synchronize()
    fit_wave, fit_frames = fit.wave.clone(), fit.frames.cpu().tolist()
    assert ops.status() & CAPACITY_BITS == 0 and 4 * need[1][0] > T_cap
    over = gs(controls=pipeline.Controls(B, speed=[0.25, 0.8, 1.5]))
    torch.cuda.synchronize()
    assert ops.status() & CAPACITY_BITS == CAPACITY_BITS, hex(ops.status())
    assert over.frames.cpu().tolist() == [T_cap] + fit_frames[1:]
    for r in (1, 2):
        assert torch.equal(over.wave[r], fit_wave[r]), "row %d changed because row 0 ran out of capacity" % r
    assert bool(torch.isfinite(over.wave[0]).all()) and bool(over.wave[0, :, -600:].any())  # truncated, not padded
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        rows = over.to_host()
    hits = [w for w in caught if issubclass(w.category, RuntimeWarning) and "FRAME_CAPACITY" in str(w.message)]
    assert len(hits) == 1 and [len(r) for r in rows] == [600 * T_cap] + [600 * f for f in fit_frames[1:]]
    assert len(records) == 1 and ops.status() & CAPACITY_BITS == 0


# ---- 8. long-form: per-sentence rate and style ----------------------------------------------------------------------------------
def test_long_form_per_sentence_speed_and_t_one_mix_launch():
    man, model, sampler = _model("libritts")
    b = _batch(True)
    K = len(LENS)
    sentences = [b["tokens"][k, :LENS[k]].clone() for k in range(K)]
    ref_s = b["ref_s"][:1]
    speeds, ts = [1.0, 0.8, 1.5], [0.5, W3, 0.75]
    noises = [b["noise"][k:k + 1] for k in range(K)]
    step_noises = [b["step_noise"][:, k:k + 1].contiguous() for k in range(K)]
    # the sentence-by-sentence schedule with the same values as scalars (and the rate as a one-row control)
    want, sines, s_prev = [], [], None
    for k in range(K):
        p = pipeline.prepare(model, sampler, sentences[k][None], noise=noises[k], step_noise=step_noises[k], ref_s=ref_s,
                             diffusion_steps=STEPS, lj_tail=False, s_prev=s_prev, t=ts[k],
                             controls=pipeline.Controls(1, speed=[speeds[k]]))
        T = p["asr"].shape[-1]
        sines.append(b["sine"][k:k + 1, :600 * T].contiguous())
        want.append(model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sines[k]).reshape(-1)[:-100])
        s_prev = p["s_pred"]
    assert len({w.numel() for w in want}) == K
    n0 = ops.style_mix_launches
    waves, s_last = pipeline.synthesize_long(model, sampler, sentences, ref_s=ref_s, diffusion_steps=STEPS, noises=noises,
                                             step_noises=step_noises, sine_noises=sines, front_batch=0, overlap=False,
                                             controls=pipeline.Controls(K, speed=speeds, t=ts))
    assert ops.style_mix_launches - n0 == 1, "the passage's front issues ONE mix launch"
    for k in range(K):
        assert waves[k].shape == want[k].shape and torch.equal(waves[k], want[k]), "sentence %d" % k
    assert torch.equal(s_last, s_prev)
    torch.cuda.synchronize()
    ops.check_status()
