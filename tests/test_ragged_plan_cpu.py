"""The ragged decoder and prosody plans (st2_decoder_forward_ragged / st2_prosody_forward_ragged) on HOST memory through the
full backend table of tests/_cpu_backend_ragged.py: every row of a ragged call against the same plan run unpadded at the
row's own frame count, tails exactly 0.  Checks the plans' length bookkeeping (per-row length table, View::len threading,
length-aware statistics) independently of the HIP kernels -- no GPU needed."""
import pytest
import torch

import _cpu_backend_ragged as CBR
from _cpu_backend_ragged import ragged_cpu_backend
from _util import decoder_kwargs, manifest, rms
from benchdata import synth  # seeded synthetic weights / inputs (test + bench helper, not product code)
from styletts2_amd import engine
from styletts2_amd.decoder import Decoder

T_MAX = 70
FRAMES = [T_MAX, T_MAX - 1, 64, 37]  # T_max, T_max - 1, one 128-column tile at 2 T_b, a length off every tile grid


def _padded(frames, seed):
    B = len(frames)
    asr, F0, N = torch.zeros(B, 512, T_MAX), torch.zeros(B, 2 * T_MAX), torch.zeros(B, 2 * T_MAX)
    noise, s = torch.zeros(B, 600 * T_MAX, 9), torch.zeros(B, 128)
    rows = []
    for b, T in enumerate(frames):
        a, f, n, st, nz = synth.decoder_inputs(1, T, seed + b)
        asr[b, :, :T], F0[b, :2 * T], N[b, :2 * T], s[b], noise[b, :600 * T] = a[0], f[0], n[0], st[0], nz[0]
        rows.append((a, f, n, st, nz))
    return asr, F0, N, s, noise, rows


@pytest.mark.parametrize("tag", ["ljspeech", "libritts"])  # iSTFTNet, HiFi-GAN
def test_ragged_decoder_plan_rows_equal_unpadded_runs(tag):
    dc = manifest(tag)["config"]["decoder"]
    dec = Decoder(**decoder_kwargs(dc)).eval()
    synth.init_synthetic_(dec, 1)
    asr, F0, N, s, noise, rows = _padded(FRAMES, 3)
    with ragged_cpu_backend():
        eng = engine.build_decoder_engine(dec, None)
        wave = eng.decoder_forward(asr, F0, N, s, noise=noise, frames=FRAMES)
        for name in ("ragged_lengths", "act_split_len", "stats_finalize_len", "instnorm_stats_len", "conv1d_direct_len",
                     "adain_leaky_pool_len", "convt_interleave_stats_len", "har_source_len"):
            assert CBR.CALLS.get(name, 0) > 0, "slot %s never ran" % name
        if dc["type"] == "istftnet":
            assert CBR.CALLS.get("stft_mag_phase_len", 0) > 0 and CBR.CALLS.get("istft_len", 0) > 0
        solos = [eng.decoder_forward(*r[:4], noise=r[4]) for r in rows]
        with pytest.raises(ValueError):
            eng.decoder_forward(asr, F0, N, s, noise=noise, frames=FRAMES, taps={})
    assert wave.shape == (len(FRAMES), 1, 600 * T_MAX)
    for b, T in enumerate(FRAMES):
        row = wave[b:b + 1, :, :600 * T]
        assert solos[b].shape == row.shape
        err = rms(row - solos[b])
        assert err < 1e-5 * max(1.0, rms(solos[b])), "%s row %d (T=%d): RMS %g vs the unpadded run" % (tag, b, T, err)
        assert bool((wave[b, :, 600 * T:] == 0).all()), "row %d: tail is not exactly 0" % b


def test_ragged_decoder_plan_full_rows_equal_plain_plan():
    dc = manifest("ljspeech")["config"]["decoder"]
    dec = Decoder(**decoder_kwargs(dc)).eval()
    synth.init_synthetic_(dec, 2)
    asr, F0, N, s, noise = synth.decoder_inputs(2, 9, 4)
    with ragged_cpu_backend():
        eng = engine.build_decoder_engine(dec, None)
        plain = eng.decoder_forward(asr, F0, N, s, noise=noise)
        full = eng.decoder_forward(asr, F0, N, s, noise=noise, frames=[9, 9])
    assert rms(plain - full) < 1e-5


@pytest.mark.parametrize("shift", [False, True])
def test_ragged_prosody_plan_rows_equal_unpadded_runs(shift):
    from styletts2_amd.text import ProsodyPredictor
    pred = ProsodyPredictor(style_dim=128, d_hid=512, nlayers=3, max_dur=50).eval()
    synth.init_synthetic_(pred, 7)
    B, N = len(FRAMES), 9
    g = torch.Generator().manual_seed(3)
    d_cm = torch.randn(B, 640, N, generator=g)
    t_en = torch.randn(B, 512, N, generator=g)
    s = torch.randn(B, 128, generator=g)
    dur = torch.zeros(B, N, dtype=torch.long)
    for b, T in enumerate(FRAMES):  # N tokens whose durations sum to the row's frame count
        base = torch.randint(1, max(2, T // N), (N,), generator=g)
        base[-1] += T - int(base.sum())
        assert int(base[-1]) >= 1
        dur[b] = base
    with ragged_cpu_backend():
        eng = engine.build_predictor_engine(pred, None)
        asr, f0, nn_ = eng.prosody_forward(d_cm, t_en, dur, s, T_MAX, shift=shift, frames=FRAMES)
        assert CBR.CALLS.get("expand_by_durations_len", 0) > 0
        solos = [eng.prosody_forward(d_cm[b:b + 1], t_en[b:b + 1], dur[b:b + 1], s[b:b + 1], T, shift=shift)
                 for b, T in enumerate(FRAMES)]
    for b, T in enumerate(FRAMES):
        a1, f1, n1 = solos[b]
        assert torch.equal(asr[b:b + 1, :, :T], a1)
        for got, ref in ((f0[b:b + 1, :2 * T], f1), (nn_[b:b + 1, :2 * T], n1)):
            assert (got - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())
        assert bool((asr[b, :, T:] == 0).all()) and bool((f0[b, 2 * T:] == 0).all()) and bool((nn_[b, 2 * T:] == 0).all())
