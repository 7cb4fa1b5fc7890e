"""Length-aware prosody and decoder: one call per ragged batch.  Row b of a ragged call must be the
utterance synthesised alone at its own frame count T_b; everything past a row's end is exactly 0 and never read."""
import pytest
import torch

from _util import MEL_L1_TOL, WAVE_RMS_TOL, decoder_kwargs, manifest, mel_l1, rms
from oracle import st2_oracle as O
from benchdata import synth  # seeded synthetic weights / inputs (test + bench helper, not product code)
from styletts2_amd import models, pipeline
from styletts2_amd.decoder import Decoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_MAX = 400
FRAMES = [T_MAX, T_MAX - 1, 128, 203, 64, 331]  # full row, one short, one 128-column tile, ragged ends


def _decoder(tag):
    dc = manifest(tag)["config"]["decoder"]
    dec = Decoder(**decoder_kwargs(dc)).eval()
    synth.init_synthetic_(dec, 1)
    sd = {k: v.clone() for k, v in dec.state_dict().items()}
    return dc, dec.to(DEV), sd


def _padded_inputs(frames, seed=3):
    """Per-row inputs drawn at each row's own length, zero-padded to T_MAX (the same tensors the solo runs see)."""
    B = len(frames)
    asr = torch.zeros(B, 512, T_MAX)
    F0 = torch.zeros(B, 2 * T_MAX)
    N = torch.zeros(B, 2 * T_MAX)
    noise = torch.zeros(B, 600 * T_MAX, 9)
    s = torch.zeros(B, 128)
    rows = []
    for b, T in enumerate(frames):
        a, f, n, st, nz = synth.decoder_inputs(1, T, seed + b)
        asr[b, :, :T], F0[b, :2 * T], N[b, :2 * T], s[b], noise[b, :600 * T] = a[0], f[0], n[0], st[0], nz[0]
        rows.append((a, f, n, st, nz))
    return asr, F0, N, s, noise, rows


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_ragged_decoder_rows_equal_solo_runs(tag):
    dc, dec, sd = _decoder(tag)
    asr, F0, N, s, noise, rows = _padded_inputs(FRAMES)
    frames = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    args = [t.to(DEV) for t in (asr, F0, N, s)]
    wave = dec(*args, noise=noise.to(DEV), frames=frames)
    torch.cuda.synchronize()
    assert wave.shape == (len(FRAMES), 1, 600 * T_MAX)
    uniform_equal = []
    for b, T in enumerate(FRAMES):
        a, f, n, st, nz = rows[b]
        solo = dec(a.to(DEV), f.to(DEV), n.to(DEV), st.to(DEV), noise=nz.to(DEV))
        row = wave[b:b + 1, :, :600 * T]
        assert solo.shape == row.shape
        err = rms(row.cpu() - solo.cpu())
        assert err < 1e-6, "%s row %d (T=%d) differs from its solo run: RMS %g" % (tag, b, T, err)
        assert bool((wave[b, :, 600 * T:] == 0).all()), "row %d: tail past 600 T_b is not exactly 0" % b
        # a uniform batch of four at T_b picks the same tile widths: report (not assert) bitwise equality
        uni = dec(*(t.repeat(4, *([1] * (t.dim() - 1))).to(DEV) for t in (a, f, n, st)),
                  noise=nz.repeat(4, 1, 1).to(DEV))
        uniform_equal.append(bool(torch.equal(uni[:1], row)))
    print("%s: ragged row bitwise == row of a uniform B=4 batch at T_b: %s" % (tag, uniform_equal))
    # one row against the CPU oracle, harmonic features injected (tap-point protocol)
    b = 3
    T = FRAMES[b]
    a, f, n, st, nz = rows[b]
    to = {}
    ref = O.decoder(sd, dc, a, f, n, st, noise=nz, taps=to)
    har = to["har"]
    if dc["type"] == "istftnet":
        hp = torch.zeros(len(FRAMES), har.shape[1], 120 * T_MAX + 1)
        hp[b, :, :har.shape[-1]] = har[0]
    else:
        hp = torch.zeros(len(FRAMES), 1, 600 * T_MAX)
        hp[b, :, :har.shape[-1]] = har.reshape(1, -1)
    w_inj = dec(*args, noise=noise.to(DEV), har=hp.to(DEV), frames=frames)
    out = w_inj[b:b + 1, :, :600 * T].cpu()
    assert rms(out - ref) < WAVE_RMS_TOL, "oracle RMS %g" % rms(out - ref)
    assert mel_l1(out, ref) < MEL_L1_TOL


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])
def test_ragged_decoder_full_rows_bitwise_plain_and_nan_tails_ignored(tag):
    dc, dec, sd = _decoder(tag)
    B, T = 4, 160
    asr, F0, N, s, noise = synth.decoder_inputs(B, T, 5)
    args = [t.to(DEV) for t in (asr, F0, N, s)]
    plain = dec(*args, noise=noise.to(DEV))
    full = dec(*args, noise=noise.to(DEV), frames=[T] * B)
    torch.cuda.synchronize()
    assert torch.equal(plain, full), "all frames == T_max must be today's st2_decoder_forward bit for bit"
    # NaN past every row's end: the masks are selects, the output is the zero-padded run's
    asr, F0, N, s, noise, _ = _padded_inputs(FRAMES, seed=11)
    frames = torch.tensor(FRAMES, dtype=torch.int32, device=DEV)
    clean = dec(asr.to(DEV), F0.to(DEV), N.to(DEV), s.to(DEV), noise=noise.to(DEV), frames=frames)
    for b, Tb in enumerate(FRAMES):
        asr[b, :, Tb:] = float("nan")
        F0[b, 2 * Tb:] = float("nan")
        N[b, 2 * Tb:] = float("nan")
        noise[b, 600 * Tb:] = float("nan")
    poisoned = dec(asr.to(DEV), F0.to(DEV), N.to(DEV), s.to(DEV), noise=noise.to(DEV), frames=frames)
    torch.cuda.synchronize()
    assert torch.equal(clean, poisoned)


def _model(tag):
    man = manifest(tag)
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    keys = ["decoder", "diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]
    for i, k in enumerate(keys):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval()
    sds = {k: {n: t.clone() for n, t in model[k].state_dict().items()} for k in keys}
    for k in keys:
        model[k].to(DEV)
    return man, model, sds


def _real_batch():
    import bench
    tokens, lengths, noise, dur, lens = bench.ragged_inputs("cpu")
    pick = [21, 29, 3, 9, 0, 5]  # 50, 47, 84, 73, 131, 182 tokens (test_pipeline_gpu's real-text batch)
    tokens, lengths, noise, dur = tokens[pick], lengths[pick], noise[pick], dur[pick]
    lens = [lens[i] for i in pick]
    N = max(lens)
    g = torch.Generator().manual_seed(8)
    steps, B = 5, len(pick)
    step_noise = torch.randn(steps - 1, B, 1, 256, generator=g)
    sine_noise = torch.randn(B, 600 * 4 * N, 9, generator=g)
    return tokens[:, :N], lengths, noise, dur[:, :N], lens, step_noise, sine_noise, steps


def test_ragged_prosody_rows_equal_group_calls():
    man, model, sds = _model("ljspeech")
    tokens, lengths, noise, dur, lens, step_noise, sine_noise, steps = _real_batch()
    sampler = models.make_sampler(model)
    pg = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), diffusion_steps=steps,
                          durations=dur.to(DEV), step_noise=step_noise.to(DEV), allow_ragged=True)
    pr = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), diffusion_steps=steps,
                          durations=dur.to(DEV), step_noise=step_noise.to(DEV), allow_ragged=True, ragged_decode=True)
    torch.cuda.synchronize()
    assert "groups" not in pr and pr["frames_host"] == [4 * n for n in lens]
    for idx, g in pg["groups"]:
        for j, b in enumerate(idx):
            T = pr["frames_host"][b]
            assert g["asr"].shape[-1] == T
            assert torch.equal(pr["asr"][b, :, :T], g["asr"][j])
            for k in ("F0", "N"):
                ref = g[k][j]
                e = (pr[k][b, :2 * T] - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
                assert e < 1e-4, "%s row %d rel err %g" % (k, b, e)
            assert bool((pr["asr"][b, :, T:] == 0).all())
            assert bool((pr["F0"][b, 2 * T:] == 0).all()) and bool((pr["N"][b, 2 * T:] == 0).all())


def test_ragged_pipeline_one_call_each_matches_grouped_path_and_graphs():
    from styletts2_amd import engine as E
    man, model, sds = _model("ljspeech")
    tokens, lengths, noise, dur, lens, step_noise, sine_noise, steps = _real_batch()
    sampler = models.make_sampler(model)
    kw = dict(diffusion_steps=steps, durations=dur.to(DEV), step_noise=step_noise.to(DEV), sine_noise=sine_noise.to(DEV))
    base = pipeline.inference(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), **kw)
    calls = {"prosody": 0, "decoder": 0}
    orig_p, orig_d = E.Engine.prosody_forward, E.Engine.decoder_forward

    def cp(self, *a, **k):
        calls["prosody"] += 1
        return orig_p(self, *a, **k)

    def cd(self, *a, **k):
        calls["decoder"] += 1
        return orig_d(self, *a, **k)
    E.Engine.prosody_forward, E.Engine.decoder_forward = cp, cd
    try:
        rag = pipeline.inference(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), ragged_decode=True, **kw)
        torch.cuda.synchronize()
    finally:
        E.Engine.prosody_forward, E.Engine.decoder_forward = orig_p, orig_d
    assert calls == {"prosody": 1, "decoder": 1}, calls
    assert [w.shape for w in rag] == [w.shape for w in base]
    for a, b in zip(rag, base):
        assert rms(a.cpu() - b.cpu()) <= 1e-6 * max(rms(b.cpu()), 1.0)
    again = pipeline.inference(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), ragged_decode=True, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(rag, again))
    # the ragged decoder inside a captured hipGraph: replay == the eager call
    p = pipeline.prepare(model, sampler, tokens.to(DEV), lengths, noise.to(DEV), diffusion_steps=steps,
                         durations=dur.to(DEV), step_noise=step_noise.to(DEV), allow_ragged=True, ragged_decode=True)
    T_max = p["asr"].shape[-1]
    sn = torch.zeros(len(lens), 600 * T_max, 9, device=DEV)
    for b, T in enumerate(p["frames_host"]):
        sn[b, :600 * T] = sine_noise[b, :600 * T].to(DEV)
    eager = model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sn, frames=p["frames"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            graphed = model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sn, frames=p["frames"])
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed, eager)
    # one utterance against the oracle at the 1e-4 bar (harmonic features injected)
    b0, n0 = 1, lens[1]
    to = {}
    ref = O.inference(sds, man["config"], man["plbert"], tokens[b0:b0 + 1, :n0], lengths[b0:b0 + 1], noise[b0:b0 + 1],
                      step_noise[:, b0:b0 + 1], sine_noise[b0:b0 + 1, :600 * 4 * n0], diffusion_steps=steps,
                      durations=dur[b0:b0 + 1, :n0], taps=to)
    T0 = 4 * n0
    asr = torch.zeros(2, 512, T0 + 7)
    F0 = torch.zeros(2, 2 * (T0 + 7))
    Nn = torch.zeros(2, 2 * (T0 + 7))
    snp = torch.zeros(2, 600 * (T0 + 7), 9)
    hp = torch.zeros(2, to["har"].shape[1], 120 * (T0 + 7) + 1)
    for r in range(2):
        asr[r, :, :T0], F0[r, :2 * T0], Nn[r, :2 * T0] = to["asr"][0], to["F0"][0], to["N"][0]
        snp[r, :600 * T0] = sine_noise[b0, :600 * T0]
        hp[r, :, :to["har"].shape[-1]] = to["har"][0]
    s2 = to["s_pred"][:, :128].repeat(2, 1)
    w = model.decoder(asr.to(DEV), F0.to(DEV), Nn.to(DEV), s2.to(DEV), noise=snp.to(DEV), har=hp.to(DEV),
                      frames=[T0, T0 + 7])
    assert rms(w[:1, :, :600 * T0].cpu() - ref) < WAVE_RMS_TOL


def test_ragged_long_form_matches_default_path():
    man, model, sds = _model("ljspeech")
    tokens, lengths, noise, dur, lens, step_noise, sine_noise, steps = _real_batch()
    sents = [tokens[b, :lens[b]].to(DEV) for b in range(3)]
    durs = [dur[b:b + 1, :lens[b]] for b in range(3)]
    sn = [sine_noise[b:b + 1, :600 * 4 * lens[b]].to(DEV) for b in range(3)]
    nz = [noise[b:b + 1].to(DEV) for b in range(3)]
    stn = [step_noise[:, b:b + 1].to(DEV) for b in range(3)]
    sampler = models.make_sampler(model)
    kw = dict(diffusion_steps=steps, noises=nz, step_noises=stn, sine_noises=sn, durations=durs, front_batch=0)
    w0, s0 = pipeline.synthesize_long(model, sampler, sents, **kw)
    w1, s1 = pipeline.synthesize_long(model, sampler, sents, ragged_decode=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1)
    for a, b in zip(w1, w0):
        assert a.shape == b.shape
        assert rms(a.cpu() - b.cpu()) <= 1e-6 * max(rms(b.cpu()), 1.0)
