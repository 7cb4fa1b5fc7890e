"""What the clip ingest costs: 32 reference clips of 10 s each in one warm process, three legs --
8 kHz mu-law, 16 kHz 16-bit PCM, 48 kHz 16-bit PCM -- through `ops.clip_ingest` (decode, resample to 24 kHz, trim at 30 dB,
MIN_CLIP as the minimum length), device time per call from events, min / median / max over `--rounds` turns of `--calls` calls,
beside the `compute_style(wave, lengths=)` call it feeds (the LibriTTS-size style encoders, seeded weights) on the ingest's own
output.  The clips are tone bursts between low-level noise, so the trim has something to cut.  Every timed block runs under a
watchdog: one that exceeds `--step-timeout` seconds ends the process (exit status 124) instead of queueing more work behind a
hung device.

    python tools/probe_ingest.py [--calls 20] [--rounds 5] [--out profiles/ingest]
"""
import argparse
import json
import os
import statistics
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchdata import manifest, synth  # noqa: E402
from styletts2_amd import models, ops, resample, style  # noqa: E402

B, SECONDS = 32, 10
LEGS = [(8000, "ulaw"), (16000, "s16"), (48000, "s16")]


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


def _ulaw(v):
    """int16 -> G.711 mu-law bytes (numpy; the probe's input only)."""
    v = v.astype(np.int64)
    mag = np.minimum((np.where(v < 0, ~v, v) >> 2) + 33, 0x1FFF)
    seg = sum((mag > end).astype(np.int64) for end in (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF))
    code = ((seg << 4) | ((mag >> (seg + 1)) & 0xF)) ^ 0x7F
    return np.where(v < 0, code, code | 0x80).astype(np.uint8)


def clips(rate, fmt, seed=0):
    """[B, rate * SECONDS]: 0.5-1.5 s of noise at -70 dB, a two-partial tone, 0.5-1.5 s of noise again."""
    rng = np.random.default_rng(seed)
    n = rate * SECONDS
    t = np.arange(n) / rate
    x = 2e-4 * rng.standard_normal((B, n))
    for b in range(B):
        a, z = int(rng.uniform(0.5, 1.5) * rate), n - int(rng.uniform(0.5, 1.5) * rate)
        x[b, a:z] += 0.35 * np.sin(2 * np.pi * (110 + 7 * b) * t[a:z]) + 0.15 * np.sin(2 * np.pi * 1330 * t[a:z])
    v = np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int16)
    return torch.from_numpy(v if fmt == "s16" else _ulaw(v))


def timed(step, a):
    ts = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with Watchdog(a.step_timeout):
            e0.record()
            for _ in range(a.calls):
                step()
            e1.record()
            torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.calls)
    return {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    man = manifest("libritts")
    model = models.build_model(models.recursive_munch(man["config"]), None, None, models.load_plbert(man["plbert"]))
    synth.init_spectral_norm_(model.style_encoder, 3)
    synth.init_spectral_norm_(model.predictor_encoder, 4)
    model.style_encoder.to(dev)
    model.predictor_encoder.to(dev)
    with torch.no_grad():
        for rate, fmt in LEGS:
            src = clips(rate, fmt).to(dev)
            n = torch.full((B,), src.shape[1], dtype=torch.int32, device=dev)
            U, D, K, _ = resample.input_table(rate, dev)
            L_cap = resample.output_samples(src.shape[1], U, D)
            out = torch.empty((B, L_cap), device=dev)
            ingest = lambda: ops.clip_ingest(src, n, rate, fmt, top_db=style.TRIM_TOP_DB, L_cap=L_cap, L_min=style.MIN_CLIP, out=out)
            with Watchdog(a.step_timeout):
                wave, length, start, flags = ingest()
                style.compute_style(model, wave, lengths=length)  # warm-up: engines packed, mel weights cached
                torch.cuda.synchronize()
            kept = length.cpu().tolist()
            t_in = timed(ingest, a)
            t_style = timed(lambda: style.compute_style(model, wave, lengths=length), a)
            emit({"workload": "clip_ingest_32x10s", "rate": rate, "fmt": fmt, "U": U, "D": D, "K": K, "L_cap": L_cap,
                  "src_bytes": int(src.numel() * src.element_size()), "fp32_24k_bytes": int(B * L_cap * 4),
                  "kept_s": {"min": round(min(kept) / 24000, 2), "max": round(max(kept) / 24000, 2)},
                  "flags_or": int(np.bitwise_or.reduce(flags.cpu().numpy())), "launches_per_call": 3,
                  "ingest_ms_per_call": t_in, "compute_style_ms_per_call": t_style, "calls": a.calls, "rounds": a.rounds})
        ops.check_status()
    with open(os.path.join(a.out, "probe_ingest.jsonl"), "w") as f:
        f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
