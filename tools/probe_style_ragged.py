"""Ragged reference-style A-B: 32 seeded clips of 3-10 s at 24 kHz, LibriTTS-configuration style
encoders with seeded synthetic weights, one warm process, one stream, the two modes taking turns:

  per_clip    today's serving loop: `style.compute_style(model, clip)` once per clip (the parent commit's behaviour)
  ragged      one `style.compute_style(model, wave [B, L_cap], lengths=)` call for the whole batch

Per mode: ms per batch (host start to device done; min / median / max over `--rounds` turns) and kernel launches per batch
(the kernel records of a torch.profiler trace, taken in a turn of its own).  Also the largest difference between
the two results.  Every step runs under a watchdog: a step that exceeds `--step-timeout` seconds ends the process (exit
status 124) instead of queueing more work behind a hung device.

    python tools/probe_style_ragged.py [--batch 32] [--rounds 5] [--warmup 2] [--out profiles/style_ragged]
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

from benchdata import manifest, synth  # noqa: E402
from styletts2_amd import models, style  # noqa: E402
from probe_sync_free import Watchdog  # noqa: E402  (tools/: the per-step watchdog)


def _launches(fn):
    """Kernel launches of one call: the device-side kernel records of a torch.profiler trace (copies and fills, which the
    profiler names Memcpy / Memset, are not launches and are left out)."""
    from torch.profiler import ProfilerActivity, profile
    from torch.autograd import DeviceType
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events()
               if e.device_type == DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_ragged"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    man = manifest("libritts")
    model = models.build_model(models.recursive_munch(man["config"]), None, None, models.load_plbert(man["plbert"]))
    synth.init_spectral_norm_(model.style_encoder, 3)
    synth.init_spectral_norm_(model.predictor_encoder, 4)
    model.style_encoder.to(dev)
    model.predictor_encoder.to(dev)
    g = torch.Generator().manual_seed(0)
    lengths = [int(v) for v in torch.randint(3 * 24000, 10 * 24000 + 1, (a.batch,), generator=g)]
    clips = [(torch.randn(n, generator=g) * 0.1).to(dev) for n in lengths]
    wave = torch.zeros((a.batch, max(lengths)), device=dev)
    for b, c in enumerate(clips):
        wave[b, :lengths[b]] = c
    dev_len = torch.tensor(lengths, dtype=torch.int32, device=dev)
    modes = {"per_clip": lambda: torch.cat([style.compute_style(model, c) for c in clips]),
             "ragged": lambda: style.compute_style(model, wave, lengths=dev_len)}
    times = {k: [] for k in modes}
    outs = {}
    for turn in range(a.warmup + a.rounds):
        for name, fn in modes.items():
            with Watchdog(a.step_timeout):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                if turn >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    res = {"batch": a.batch, "seconds_of_audio": round(sum(lengths) / 24000.0, 1), "L_cap": max(lengths),
           "device": torch.cuda.get_device_name(0),
           "max_abs_diff": float((outs["ragged"] - outs["per_clip"]).abs().max())}
    for name, fn in modes.items():
        ts = times[name]
        res[name] = {"ms_min": round(min(ts), 3), "ms_median": round(statistics.median(ts), 3), "ms_max": round(max(ts), 3)}
        try:
            with Watchdog(a.step_timeout):
                res[name]["launches_per_batch"] = _launches(fn)
        except Exception as e:  # noqa: BLE001 -- the timings above stand; the report says why the count is missing
            res[name]["launches_per_batch"] = None
            res[name]["launches_error"] = repr(e)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe_style_ragged.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
