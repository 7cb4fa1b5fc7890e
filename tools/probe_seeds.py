"""Refreshing the noise of a recorded synthesis graph at the headline's size -- B = 32, 400 frames, 5
sampler steps -- and at B = 8: the three `st2_noise_fill` launches of a seeded graph against what a caller of a graph without
seeds does for fresh noise, `torch.randn` of the three tensors and the three `copy_` of `GraphedSynthesis.__call__` into the
static buffers.  Device time per refresh from events around `--calls` back-to-back refreshes, host time per refresh from the
clock around issuing them, after a warm-up, the legs taking turns over `--rounds` rounds, in one process.  One JSON line per leg:
min / median / max of the rounds in microseconds, the bytes the leg writes (by arithmetic: 4 per noise value) and, from the
median, the rate at which it writes them.  Needs a HIP device; there is nothing to fall back to.

    python tools/probe_seeds.py [--calls 50] [--rounds 5] [--out FILE]
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

from styletts2_amd import ops  # noqa: E402

T_CAP, STEPS = 400, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_seeds needs a HIP device")
    dev = "cuda"
    legs = {}
    for B in (32, 8):
        shapes = dict(noise=(B, 1, 256), step_noise=(STEPS - 1, B, 1, 256), sine_noise=(B, 600 * T_CAP, 9))
        static = {k: torch.zeros(s, device=dev) for k, s in shapes.items()}
        seeds = torch.arange(B, dtype=torch.int64, device=dev)
        frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
        values = sum(v.numel() for v in static.values())

        def fill(st=static, seeds=seeds, frames=frames):
            ops.noise_fill(seeds, st["noise"], ops.NOISE_SAMPLER)
            ops.noise_fill(seeds, st["step_noise"], ops.NOISE_STEP, streams=STEPS - 1)
            ops.noise_fill(seeds, st["sine_noise"], ops.NOISE_SINE, counts=frames, per_count=5400)

        def sine_only(st=static, seeds=seeds, frames=frames):
            ops.noise_fill(seeds, st["sine_noise"], ops.NOISE_SINE, counts=frames, per_count=5400)

        def sine_bits(st=static, seeds=seeds, frames=frames):  # the same stores without Box-Muller: Philox and the writes alone
            ops.noise_fill(seeds, st["sine_noise"].view(torch.int32), ops.NOISE_SINE, counts=frames, per_count=5400, bits=True)

        def randn_copy(st=static, shapes=shapes):
            for k, s in shapes.items():  # what the caller draws, then GraphedSynthesis.__call__'s copy into the static buffer
                st[k].copy_(torch.randn(s, device=dev).reshape(st[k].shape), non_blocking=True)

        legs["noise_fill x3 B=%d" % B] = (values, fill)
        legs["randn + copy_ x3 B=%d" % B] = (values, randn_copy)
        legs["noise_fill source only B=%d" % B] = (static["sine_noise"].numel(), sine_only)
        legs["noise_fill source only, raw words B=%d" % B] = (static["sine_noise"].numel(), sine_bits)
    dev_us, host_us = {name: [] for name in legs}, {name: [] for name in legs}
    for _, call in legs.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (_, call) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            h1 = time.perf_counter()
            t1.record()
            t1.synchronize()
            dev_us[name].append(1e3 * t0.elapsed_time(t1) / a.calls)
            host_us[name].append(1e6 * (h1 - h0) / a.calls)
    lines = []
    for name, (values, _) in legs.items():
        t, h = dev_us[name], host_us[name]
        lines.append(dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                          host_us_min=round(min(h), 2), host_us_median=round(statistics.median(h), 2), host_us_max=round(max(h), 2),
                          calls=a.calls, rounds=a.rounds, bytes_written=4 * values,
                          write_gb_per_s=round(4 * values / (statistics.median(t) * 1e-6) / 1e9, 1)))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
