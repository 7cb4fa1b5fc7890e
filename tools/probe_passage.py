"""Passages on the sync-free path, in one warm process on one stream, the modes taking turns:

  pack leg      B = 8 rows of 10 s: the existing pack (`ops.wave_pack` "s16" at 24 kHz, `ops.wave_resample_pack` "ulaw" at 8 kHz)
                against `ops.wave_pack_gaps` with gaps = None (the same two launches), with all gaps 0 (scan, move and a fill
                whose workgroups all leave at once) and with 250 ms behind every row; us per call from device events.
  passage leg   the validation passage -- the first `--sentences` utterances of benchdata/val_phonemes_32.txt as consecutive
                sentences, iSTFTNet, 5 diffusion steps, seeded synthetic weights, PREDICTED durations -- as
                  long_form   `synthesize_long(front_batch=0, ragged_decode=True)`, the path that existed: one host read of
                              the frame counts, padded fp32 rows sliced on the host;
                  eager       `inference(max_frames=, passage=True, gaps=, pack="s16")`;
                  graph       one `GraphedSynthesis(passage=True, max_gap=)` replay;
                ms per passage (host start to device done) and the host ms spent inside the call.

Every step runs under a watchdog: a step that exceeds `--step-timeout` seconds ends the process (exit status 124) instead of
queueing more work behind a hung device; the caller adds an outer `timeout`.

    python tools/probe_passage.py [--steps 5] [--warmup 2] [--rounds 3] [--sentences 8] [--out profiles/passage]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (workload definitions: ragged_inputs)
from probe_sync_free import STEPS_D, Watchdog, _model  # noqa: E402
from styletts2_amd import ops, pipeline  # noqa: E402

spread = lambda v: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def pack_leg(dev, a, emit):
    B, T = 8, 400
    wave = torch.randn(B, 1, 600 * T, device=dev) * 0.3
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    for fmt, rate in (("s16", None), ("ulaw", 8000)):
        hz = 24000 if rate is None else rate
        cap = pipeline.gap_samples(250, hz)
        zero = torch.zeros((B,), dtype=torch.int32, device=dev)
        full = torch.full((B,), cap, dtype=torch.int32, device=dev)
        if rate is None:
            out, offs = ops.wave_pack_gaps(wave, frames, full, cap, fmt=fmt)
            old = lambda: ops.wave_pack(wave, frames, fmt=fmt, out=out, offsets=offs)
        else:
            out, offs = ops.wave_pack_gaps(wave, frames, full, cap, rate=rate, fmt=fmt)
            old = lambda: ops.wave_resample_pack(wave, frames, rate, fmt=fmt, out=out, offsets=offs)
        new = lambda g: (lambda: ops.wave_pack_gaps(wave, frames, g, cap, rate=rate, fmt=fmt, out=out, offsets=offs))
        modes = {"existing": (old, 2), "gaps_none": (new(None), 2), "gaps_zero": (new(zero), 3), "gaps_250ms": (new(full), 3)}
        ts = {m: [] for m in modes}
        for _ in range(5):  # the modes take turns
            for m, (call, _) in modes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with Watchdog(a.step_timeout):
                    call()
                    e0.record()
                    for _ in range(20):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                ts[m].append(e0.elapsed_time(e1) / 20 * 1e3)
        for m, (_, launches) in modes.items():
            emit({"workload": "pack_8x10s", "fmt": fmt, "rate": hz, "mode": m, "gap_samples": cap if m == "gaps_250ms" else 0,
                  "launches_per_call": launches, "us_per_call": spread(ts[m])})


def passage_leg(dev, model, sampler, a, emit):
    K = a.sentences
    tokens, lengths, noise, _, lens = bench.ragged_inputs("cpu")
    lens = lens[:K]
    N = max(lens)
    tokens, lengths, noise = tokens[:K, :N].contiguous().to(dev), lengths[:K], noise[:K].to(dev)
    g = torch.Generator().manual_seed(5)
    step_noise = torch.randn(STEPS_D - 1, K, 1, 256, generator=g).to(dev)
    sentences = [tokens[k, :lens[k]].clone() for k in range(K)]
    noises = [noise[k:k + 1] for k in range(K)]
    step_noises = [step_noise[:, k:k + 1].contiguous() for k in range(K)]
    long_form = lambda: pipeline.synthesize_long(model, sampler, sentences, diffusion_steps=STEPS_D, noises=noises,
                                                 step_noises=step_noises, front_batch=0, overlap=False, ragged_decode=True)
    with Watchdog(a.step_timeout):
        waves, _ = long_form()
        torch.cuda.synchronize()
    tot = [w.numel() // 600 for w in waves]
    T_64 = (max(tot) + 63) // 64 * 64
    del waves
    sine = torch.randn(K, 600 * T_64, 9, device=dev)
    ld = lengths.to(torch.int32).to(dev)
    gap = pipeline.gap_samples(250)
    gaps = torch.full((K,), gap, dtype=torch.int32, device=dev)
    kw = dict(diffusion_steps=STEPS_D, step_noise=step_noise, lj_tail=False)
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, T_64, STEPS_D, pack="s16", lj_tail=False, passage=True, max_gap=gap)
    with Watchdog(a.step_timeout):
        gs(tokens=tokens, lengths=ld, noise=noise, step_noise=step_noise, sine_noise=sine, gaps=gaps)  # fills the buffers, records
        torch.cuda.synchronize()
    modes = {
        "long_form": long_form,
        "eager": lambda: pipeline.inference(model, sampler, tokens, lengths, noise, sine_noise=sine, lengths_dev=ld, max_frames=T_64,
                                            pack="s16", passage=True, gaps=gaps, max_gap=gap, **kw),
        "graph": lambda: gs(),
    }
    total, host = {m: [] for m in modes}, {m: [] for m in modes}
    for m, step in modes.items():
        for _ in range(a.warmup):
            with Watchdog(a.step_timeout):
                step()
                torch.cuda.synchronize()
    for _ in range(a.rounds):  # the modes take turns: drift of the box hits all of them alike
        for m, step in modes.items():
            t_tot = t_host = 0.0
            for _ in range(a.steps):
                with Watchdog(a.step_timeout):
                    t0 = time.perf_counter()
                    step()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                t_tot, t_host = t_tot + (t2 - t0), t_host + (t1 - t0)
            total[m].append(t_tot / a.steps * 1e3)
            host[m].append(t_host / a.steps * 1e3)
    ops.check_status()
    audio_s = sum(tot) * 600 / 24000.0
    for m in modes:
        emit({"workload": "val_passage_predicted", "sentences": K, "mode": m, "frames": tot, "capacity": max(tot) if m == "long_form" else T_64,
              "audio_s": round(audio_s, 1), "break_ms": 0 if m == "long_form" else 250, "ms_per_passage": spread(total[m]),
              "host_ms_in_call": spread(host[m]), "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "passage"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    with torch.no_grad():
        pack_leg(dev, a, emit)
        model, sampler = _model(dev)
        passage_leg(dev, model, sampler, a, emit)
    with open(os.path.join(a.out, "probe_passage.jsonl"), "w") as f:
        f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
