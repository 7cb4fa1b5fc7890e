"""Full-size (10 s = 400 frames, 100 phonemes) outputs of the UNMODIFIED reference modules for
tests/test_oracle_fullsize_ref.py, live where the reference is present and stored in tests/golden/fullsize_vectors.npz for
everywhere else.  Weights and inputs come from seeds (benchdata/synth.py); only reference OUTPUTS are stored, and of the
large ones (waveforms, harmonic source, t_en, d) a fixed seeded sample of SAMPLES entries (`sample`).  Run:
python -m oracle.golden_fullsize
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root: benchdata/, oracle/
from benchdata import synth  # noqa: E402  seeded synthetic weights / inputs (test + bench helper, not product code)
from oracle import golden_vectors as GV  # noqa: E402
from oracle import ref_harness as RH  # noqa: E402

PATH = os.path.join(GV.GOLDEN, "fullsize_vectors.npz")
T_FULL, N_FULL = 400, 100  # 10 s of 24 kHz audio: 400 frames x 600 samples; 100 phonemes x 4 frames
SAMPLES = 8192
DECODERS = (("ljspeech", "config.yml"), ("libritts", "config_libritts.yml"))
SAMPLED = ("wave", "har_source", "t_en", "d")


def sample(x):
    """A fixed seeded sample of SAMPLES entries of x (all of it if smaller), flattened, in index order."""
    x = x.reshape(-1)
    if x.numel() <= SAMPLES:
        return x
    idx = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(x.numel()))[:SAMPLES].sort().values
    return x[idx]


def decoder_live(cfgname):
    """Decoder.forward (Modules/istftnet.py:499-528 / Modules/hifigan.py:446-475) on one 10 s utterance.  Returns
    ({"wave", "har_source"[, "har"]}, the decoder's state dict)."""
    model, args, cfg = RH.build_reference_model(cfgname)
    dec = model["decoder"].eval()
    synth.init_synthetic_(dec, 1)
    asr, F0, N, s, noise = synth.decoder_inputs(1, T_FULL, 3)
    taps = {}
    dec.generator.m_source.register_forward_hook(
        lambda m, i, o: taps.__setitem__("har_source", o[0].transpose(1, 2).squeeze(1)))
    if cfg["model_params"]["decoder"]["type"] == "istftnet":
        orig = dec.generator.stft.transform

        def tr(x):
            a, b = orig(x)
            taps["har"] = torch.cat([a, b], 1)
            return a, b
        dec.generator.stft.transform = tr
    with torch.no_grad(), GV.replay_randn_like({noise.shape: [noise]}):
        taps["wave"] = dec(asr, F0, N, s)
    return taps, {k: v.clone() for k, v in dec.state_dict().items()}


def front_inputs():
    B, N, steps = 1, N_FULL, 5
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(1, 178, (B, N), generator=g)
    tokens[:, 0] = 0
    lengths = torch.LongTensor([N] * B)
    noise = torch.randn(B, 1, 256, generator=g)
    step_noise = torch.randn(steps - 1, B, 1, 256, generator=g)
    return tokens, lengths, noise, step_noise, steps


def front_live():
    """The 100-phoneme LJSpeech front (text encoder, PL-BERT, bert_encoder, 5-step ADPM2 sampler, duration encoder, duration
    head, F0 / N predictor) following Demo/Inference_LJSpeech.ipynb:280-311.  Returns ({"t_en", "s_pred", "d", "durations",
    "F0", "N"}, the state dicts)."""
    model, args, cfg = RH.build_reference_model("config.yml")
    ref = RH.load_reference()
    for i, k in enumerate(GV.KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval()
    tokens, lengths, noise, step_noise, steps = front_inputs()
    B, N = tokens.shape
    sampler = ref.sampler.DiffusionSampler(model.diffusion.diffusion, sampler=ref.sampler.ADPM2Sampler(),
                                           sigma_schedule=ref.sampler.KarrasSchedule(sigma_min=0.0001, sigma_max=3.0,
                                                                                     rho=9.0), clamp=False)
    with torch.no_grad():
        mask = torch.gt(torch.arange(N).unsqueeze(0) + 1, lengths.unsqueeze(1))
        t_en = model.text_encoder(tokens, lengths, mask)
        bert_dur = model.bert(tokens, attention_mask=(~mask).int())
        d_en = model.bert_encoder(bert_dur).transpose(-1, -2)
        with GV.replay_randn_like({(B, 1, 256): list(step_noise)}):
            s_pred = sampler(noise, embedding=bert_dur, num_steps=steps, embedding_scale=1).squeeze(0)
        s = s_pred[:, 128:]
        d = model.predictor.text_encoder(d_en, s, lengths, mask)
        x, _ = model.predictor.lstm(d)
        duration = torch.sigmoid(model.predictor.duration_proj(x)).sum(axis=-1)
        pred_dur = torch.round(duration.squeeze()).clamp(min=1)
        pred_dur[-1] += 5
        aln = torch.zeros(N, int(pred_dur.sum()))
        c = 0
        for i in range(N):
            aln[i, c:c + int(pred_dur[i])] = 1
            c += int(pred_dur[i])
        en = d.transpose(-1, -2) @ aln.unsqueeze(0)
        F0, Nn = model.predictor.F0Ntrain(en, s)
    sds = {k: {n: t.clone() for n, t in model[k].state_dict().items()} for k in GV.KEYS}
    return {"t_en": t_en, "s_pred": s_pred, "d": d, "durations": pred_dur, "F0": F0, "N": Nn}, sds


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for tag, cfgname in DECODERS:
        ref, _ = decoder_live(cfgname)
        for k in ("wave", "har_source"):
            out["dec_%s_%s" % (tag, k)] = sample(ref[k])
    ref, _ = front_live()
    for k, v in ref.items():
        out["fe_%s" % k] = sample(v) if k in SAMPLED else v
    np.savez_compressed(PATH, **{k: v.detach().float().numpy() for k, v in out.items()})
    print("wrote %s (%d arrays)" % (PATH, len(out)))


if __name__ == "__main__":
    main()
