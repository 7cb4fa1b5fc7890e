"""The oracle against the reference at BASELINE.json's full size (10 s = 400 frames, 100 phonemes).

The committed fixtures (tests/golden/reference_vectors.npz) pin oracle/st2_oracle.py at T = 8 frames / N <= 21 tokens.
This file closes the gap at the size the bench and the full-size GPU tests run: the UNMODIFIED reference modules and the
oracle take the same seeded weights and inputs, with the reference's in-forward random draws replayed.  Where a form of the
reference is present (oracle/ref_harness.py: a checkout, or oracle/_ref as built by oracle/make_ref.py) it runs live;
elsewhere its outputs come from tests/golden/fullsize_vectors.npz (oracle/golden_fullsize.py: a fixed seeded sample of
every large output) and the weights from the package's own modules, whose state dicts have the reference's layout.
Measured: waveform RMS 2.5e-7 (iSTFTNet, reference's harmonic features injected when live; its own ones otherwise) /
8.1e-7 (HiFi-GAN, nothing injected), `har_source` bit-equal.
"""
import numpy as np
import pytest
import torch

from _util import decoder_kwargs, manifest
from oracle import golden_fullsize as GF
from oracle import golden_vectors as GV
from oracle import ref_harness as RH
from oracle import st2_oracle as O
from styletts2_amd import models
from benchdata import synth  # seeded synthetic weights / inputs (test + bench helper, not product code)

LIVE = RH.reference_available()
T_FULL, N_FULL = GF.T_FULL, GF.N_FULL


def _stored(prefix):
    vec = np.load(GF.PATH)
    return {k[len(prefix):]: torch.from_numpy(vec[k]) for k in vec.files if k.startswith(prefix)}


def _pick(x, key):
    """The entries of an oracle output that the reference output `key` holds: all of them live, the seeded sample otherwise."""
    return x if LIVE or key not in GF.SAMPLED else GF.sample(x)


@pytest.mark.parametrize("tag,cfgname", list(GF.DECODERS))
def test_oracle_decoder_matches_live_reference_at_full_size(tag, cfgname):
    """Decoder.forward (Modules/istftnet.py:499-528 / Modules/hifigan.py:446-475) on one 10 s utterance."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    dc = manifest(tag)["config"]["decoder"]
    if LIVE:
        ref, sd = GF.decoder_live(cfgname)
        assert ref["wave"].shape == (1, 1, T_FULL * 600)
    else:
        from styletts2_amd.decoder import Decoder
        dec = Decoder(**decoder_kwargs(dc))
        synth.init_synthetic_(dec, 1)
        ref, sd = _stored("dec_%s_" % tag), dec.state_dict()
    asr, F0, N, s, noise = synth.decoder_inputs(1, T_FULL, 3)
    to = {}
    with torch.no_grad():
        # iSTFTNet takes torch.angle of the harmonic STFT as a network input (flips by 2 pi under 1e-8 changes, SURVEY.md
        # App. A): live, the conv path is compared with the reference's own harmonic features injected; HiFi-GAN end to end
        wave = O.decoder(sd, dc, asr, F0, N, s, noise=noise, taps=to)  # own harmonic source: the `har_source` tap
        if "har" in ref:
            wave = O.decoder(sd, dc, asr, F0, N, s, noise=noise, har=ref["har"])
    assert wave.shape == (1, 1, T_FULL * 600)
    hs, wave = _pick(to["har_source"], "har_source"), _pick(wave, "wave")
    assert torch.equal(hs, ref["har_source"]) or (hs - ref["har_source"]).abs().max().item() < 1e-6
    rms = (wave - ref["wave"]).double().pow(2).mean().sqrt().item()
    assert rms < 2e-6, "waveform RMS vs the reference %g" % rms


def test_oracle_front_matches_live_reference_at_full_size():
    """The 100-phoneme LJSpeech front (text encoder, PL-BERT, bert_encoder, 5-step ADPM2 sampler, duration encoder, duration
    head, F0 / N predictor) following Demo/Inference_LJSpeech.ipynb:280-311."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    man = manifest("ljspeech")
    if LIVE:
        ref, sds = GF.front_live()
    else:
        model = models.build_model(models.recursive_munch(man["config"]), None, None, models.load_plbert(man["plbert"]))
        for i, k in enumerate(GV.KEYS):
            synth.init_synthetic_(model[k], 10 + i)
        sds = {k: model[k].state_dict() for k in GV.KEYS}
        ref = _stored("fe_")
    tokens, lengths, noise, step_noise, steps = GF.front_inputs()
    taps = {}
    with torch.no_grad():
        O.front(sds, man["config"], man["plbert"], tokens, lengths, noise, step_noise, diffusion_steps=steps, taps=taps)

    def close(k, tol):
        a, b = _pick(taps[k], k), ref[k]
        return (a.reshape(-1) - b.reshape(-1)).abs().max().item() <= tol * max(b.abs().max().item(), 1.0)
    assert close("t_en", 2e-6)
    assert close("s_pred", 2e-6)
    assert close("d", 5e-6)
    pred_dur = ref["durations"]
    assert torch.equal(taps["durations"].reshape(-1).to(pred_dur.dtype), pred_dur.reshape(-1))  # the path's integer output
    assert close("F0", 1e-5) and close("N", 1e-5)
