"""Sync-free synthesis A-B: real validation text with PREDICTED durations -- the case in which the
parent path has to read the frame counts back -- in one process, after warm-up, on one stream, the modes taking turns:

  ragged      pipeline.inference(ragged_decode=True): one host read of the durations in the middle of the call
  cap         pipeline.inference(max_frames=T_max, pack="s16"): no host read; T_max = the batch's longest utterance
  cap64       the same at T_max rounded up to the next multiple of 64 (what spare capacity costs)
  graph       pipeline.GraphedSynthesis at the cap64 capacity: tokens -> packed PCM as one hipGraph replay

for B = 1 (validation utterance 3, 84 tokens) and the first B = 8 utterances of benchdata/val_phonemes_32.txt (84-182 tokens;
`--batch 32` takes all 32), iSTFTNet, 5 diffusion steps, seeded synthetic weights.  The seeded duration head predicts 25 frames
per phoneme, six times the 4 of the forced-duration bench legs: 52 s of audio for B = 1, 11 min for B = 8 -- and a decoder
workspace to match, which is why 8 and not 32 utterances is the default.  Per mode:
ms per step (host start to device done) and the host time spent inside the call, min / median / max over `--rounds` turns of
`--steps` steps.  Then `st2_wave_pack` alone at 32 x 10 s (achieved GB/s, both formats) and the device -> host bytes of the
packed result against the padded fp32 batch.  Every step runs under a watchdog: a step that exceeds `--step-timeout` seconds
ends the process (exit status 124) instead of queueing more work behind a hung device.

    python tools/probe_sync_free.py [--steps 5] [--warmup 2] [--rounds 3] [--batch both|1|8|32] [--out profiles/syncfree]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload definitions: ragged_inputs)
from benchdata import manifest, synth  # noqa: E402
from styletts2_amd import models, ops, pipeline  # noqa: E402

STEPS_D = 5


class Watchdog:
    """`with Watchdog(seconds): step()` -- ends the process if the body does not finish in time."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, lambda: (print("step exceeded %d s" % self.seconds, flush=True), os._exit(124)))
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def _model(dev):
    model = bench.build(manifest("ljspeech"))
    for i, k in enumerate(bench.KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval().to(dev)
    return model, models.make_sampler(model)


def leg(dev, model, sampler, rows, a, emit):
    tokens, lengths, noise, _, lens = bench.ragged_inputs("cpu")
    lens = [lens[i] for i in rows]
    B, N = len(rows), max(lens)
    tokens, lengths, noise = tokens[rows][:, :N].contiguous().to(dev), lengths[rows], noise[rows].to(dev)
    g = torch.Generator().manual_seed(5)
    step_noise = torch.randn(STEPS_D - 1, B, 1, 256, generator=g).to(dev)
    kw = dict(diffusion_steps=STEPS_D, step_noise=step_noise)
    tot = pipeline.prepare(model, sampler, tokens, lengths, noise, allow_ragged=True, **kw)["durations"].sum(dim=1).tolist()
    T_max = max(tot)
    T_64 = (T_max + 63) // 64 * 64
    sine = torch.randn(B, 600 * T_64, 9, device=dev)
    ld = lengths.to(torch.int32).to(dev)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_64, STEPS_D, pack="s16")
    gs(tokens=tokens, lengths=ld, noise=noise, step_noise=step_noise, sine_noise=sine)  # fills the buffers and records
    modes = {
        "ragged": lambda: pipeline.inference(model, sampler, tokens, lengths, noise, sine_noise=sine, ragged_decode=True, **kw),
        "cap": lambda: pipeline.inference(model, sampler, tokens, lengths, noise, sine_noise=sine, lengths_dev=ld,
                                          max_frames=T_max, pack="s16", **kw),
        "cap64": lambda: pipeline.inference(model, sampler, tokens, lengths, noise, sine_noise=sine, lengths_dev=ld,
                                            max_frames=T_64, pack="s16", **kw),
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
    sp = lambda v: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
    for m in modes:
        emit({"workload": "val_text_predicted", "B": B, "mode": m, "T_max": T_max, "capacity": {"cap": T_max, "ragged": T_max}.get(m, T_64),
              "frames_total": sum(tot), "audio_s": round(audio_s, 1), "ms_per_step": sp(total[m]), "host_ms_in_call": sp(host[m]),
              "audio_s_per_s": round(audio_s / (statistics.median(total[m]) * 1e-3), 1), "steps": a.steps, "rounds": a.rounds,
              "warmup": a.warmup})
    res = gs()
    with Watchdog(a.step_timeout):
        t0 = time.perf_counter()
        rows_h = res.to_host()
        t_copy = (time.perf_counter() - t0) * 1e3
    emit({"workload": "val_text_predicted", "B": B, "d2h": {"s16_valid_bytes": int(sum(r.nbytes for r in rows_h)),
                                                           "s16_copied_bytes": int(res._buf.numel()),
                                                           "fp32_padded_bytes": int(res.wave.numel() * 4),
                                                           "to_host_ms": round(t_copy, 3)}})


def pack_leg(dev, a, emit):
    B, T = 32, 400  # the headline batch: 32 x 10 s
    wave = torch.randn(B, 1, 600 * T, device=dev) * 0.3
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    for fmt, bytes_per in (("s16", 6), ("f32", 8)):
        out, offs = ops.wave_pack(wave, frames, fmt=fmt)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with Watchdog(a.step_timeout):
                e0.record()
                for _ in range(20):
                    ops.wave_pack(wave, frames, fmt=fmt, out=out, offsets=offs)
                e1.record()
                torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 20)
        n = B * 600 * T
        emit({"workload": "wave_pack_32x10s", "fmt": fmt, "us_per_call": {"min": round(min(ts) * 1e3, 2), "median": round(statistics.median(ts) * 1e3, 2),
                                                                         "max": round(max(ts) * 1e3, 2)},
              "GB_per_s_at_min": round(n * bytes_per / (min(ts) * 1e-3) / 1e9, 1), "launches_per_call": 2,
              "d2h_bytes": n * (2 if fmt == "s16" else 4)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", choices=["both", "1", "8", "32"], default="both")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syncfree"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    with torch.no_grad():
        model, sampler = _model(dev)
        if a.batch in ("both", "1"):
            leg(dev, model, sampler, [3], a, emit)
        if a.batch in ("both", "8"):
            leg(dev, model, sampler, list(range(8)), a, emit)
        if a.batch == "32":
            leg(dev, model, sampler, list(range(32)), a, emit)
        pack_leg(dev, a, emit)
    with open(os.path.join(a.out, "probe_sync_free.jsonl"), "w") as f:
        f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
