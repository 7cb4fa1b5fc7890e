"""Ragged decode A-B: the bench's two ragged workloads with `ragged_decode=False` (one prosody + one
decoder call per distinct frame count, today's default) and `True` (one of each per batch), in one process, after warm-up, on
ONE stream (no decoder-stream window search).

  ljspeech_ragged  bench.ragged_inputs: 32 LJSpeech validation utterances of 47-182 tokens, one right-padded batch,
                   4 frames / token, iSTFTNet, 5 diffusion steps, graphed front (pipeline.GraphedFront)
  longform         bench.LONGFORM_SENTENCES: one 66.9 s passage of 8 sentence units, LibriTTS HiFi-GAN, 5 steps, graphed
                   sampler, 16-token buckets, the whole passage as one front batch (front_batch = 0)

Prints one JSON line per (workload, mode): ms/step, audio-s/s, decoder calls per step, and the largest per-utterance RMS
difference of the two modes.  `--only true` runs the ragged mode alone (for a rocprofv3 --kernel-trace --stats run).

    python tools/probe_ragged_decode.py [--steps 5] [--warmup 2] [--only both|true|false] [--workload both|ragged|longform]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload definitions: ragged_inputs, LONGFORM_SENTENCES, synthetic_inputs)
from benchdata import manifest, synth  # noqa: E402
from styletts2_amd import engine, models, ops, pipeline  # noqa: E402


def _model(tag, dev, graph):
    model = bench.build(manifest(tag))
    for i, k in enumerate(bench.KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval().to(dev)
    return model, models.make_sampler(model, graph=graph)


class _Count:
    """Counts Engine.decoder_forward calls (the product path's decoder entry)."""

    def __init__(self):
        self.n = 0
        self.orig = engine.Engine.decoder_forward

    def __enter__(self):
        orig = self.orig

        def wrapped(eng, *a, **k):
            self.n += 1
            return orig(eng, *a, **k)
        engine.Engine.decoder_forward = wrapped
        return self

    def __exit__(self, *exc):
        engine.Engine.decoder_forward = self.orig


def _time(step, n_warm, n_steps):
    for _ in range(n_warm):
        step()
    torch.cuda.synchronize()
    with _Count() as c:
        step()
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n_steps):
        out = step()
    torch.cuda.synchronize()
    ops.check_status()
    return (time.perf_counter() - t) / n_steps * 1e3, c.n, out


def _diff(a, b):
    return max(float((x.float() - y.float()).pow(2).mean().sqrt()) for x, y in zip(a, b))


def ragged_leg(dev, modes, n_warm, n_steps):
    model, sampler = _model("ljspeech", dev, graph=False)
    front = pipeline.GraphedFront(model, sampler)
    tokens, lengths, noise, dur, lens = bench.ragged_inputs(dev)
    B = len(lens)
    g = torch.Generator().manual_seed(5)
    fixed = dict(step_noise=torch.randn(4, B, 1, 256, generator=g).to(dev),
                 sine_noise=torch.randn(B, 600 * bench.FRAMES_PER_PHONEME * max(lens), 9, generator=g).to(dev))
    audio_s = sum(lens) * bench.FRAMES_PER_PHONEME * 600 / 24000.0
    outs = {}
    for mode in modes:
        def step():
            return pipeline.inference(model, sampler, tokens, lengths, noise, diffusion_steps=5, durations=dur, front=front,
                                      ragged_decode=mode, **fixed)
        ms, calls, out = _time(step, n_warm, n_steps)
        outs[mode] = out
        print(json.dumps({"workload": "ljspeech_ragged", "ragged_decode": mode, "ms_per_step": round(ms, 3),
                          "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "decoder_calls": calls, "utterances": B,
                          "steps": n_steps, "warmup": n_warm}), flush=True)
    if len(outs) == 2:
        print(json.dumps({"workload": "ljspeech_ragged", "max_rms_true_vs_false": _diff(outs[True], outs[False])}), flush=True)


def longform_leg(dev, modes, n_warm, n_steps):
    model, sampler = _model("libritts", dev, graph=True)
    front = pipeline.GraphedFront(model, sampler)
    tokens, _, _, _, ref_s = bench.synthetic_inputs(bench.PER_GPU_BATCH, 1000)
    sents = [tokens[i % bench.PER_GPU_BATCH, :n].clone().to(dev) for i, n in enumerate(bench.LONGFORM_SENTENCES)]
    durs = [torch.full((1, n), bench.FRAMES_PER_PHONEME, dtype=torch.long) for n in bench.LONGFORM_SENTENCES]
    ref_s = ref_s[:1].to(dev)
    K = len(sents)
    g = torch.Generator().manual_seed(6)
    fixed = dict(noises=[torch.randn(1, 1, 256, generator=g).to(dev) for _ in range(K)],
                 step_noises=[torch.randn(4, 1, 1, 256, generator=g).to(dev) for _ in range(K)],
                 sine_noises=[torch.randn(1, 600 * bench.FRAMES_PER_PHONEME * n, 9, generator=g).to(dev)
                              for n in bench.LONGFORM_SENTENCES])
    audio_s = sum(bench.LONGFORM_SENTENCES) * bench.FRAMES_PER_PHONEME * 600 / 24000.0
    outs = {}
    for mode in modes:
        def step():
            return pipeline.synthesize_long(model, sampler, sents, ref_s=ref_s, diffusion_steps=5, durations=durs, bucket=16,
                                            front=front, front_batch=0, decode_streams=1, ragged_decode=mode, **fixed)[0]
        ms, calls, out = _time(step, n_warm, n_steps)
        outs[mode] = out
        print(json.dumps({"workload": "longform", "ragged_decode": mode, "ms_per_step": round(ms, 3),
                          "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "decoder_calls": calls, "sentences": K,
                          "steps": n_steps, "warmup": n_warm}), flush=True)
    if len(outs) == 2:
        print(json.dumps({"workload": "longform", "max_rms_true_vs_false": _diff(outs[True], outs[False])}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["both", "true", "false"], default="both")
    ap.add_argument("--workload", choices=["both", "ragged", "longform"], default="both")
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    modes = {"both": [False, True], "true": [True], "false": [False]}[a.only]
    with torch.no_grad():
        if a.workload in ("both", "ragged"):
            ragged_leg(dev, modes, a.warmup, a.steps)
        if a.workload in ("both", "longform"):
            longform_leg(dev, modes, a.warmup, a.steps)


if __name__ == "__main__":
    main()
