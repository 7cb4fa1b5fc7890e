"""`st2_wave_resample_pack` beside `st2_wave_pack` at the headline's size, 32 rows of 10 s: device time
per call from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns over `--rounds` rounds, in one
process.  One JSON line per leg: min / median / max of the rounds in microseconds, the bytes the leg reads and writes (by
arithmetic) and the device -> host bytes of its packed result.  Needs a HIP device; there is nothing to fall back to.

    python tools/probe_resample.py [--calls 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from styletts2_amd import ops, resample  # noqa: E402

B, SPF, T_CAP = 32, 600, 400  # 32 x 10 s at 24 kHz
LEGS = [("wave_pack s16 24000", None, "s16"), ("resample_pack ulaw 8000", 8000, "ulaw"), ("resample_pack s16 48000", 48000, "s16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_resample needs a HIP device")
    dev = "cuda"
    wave = (torch.randn(B, SPF * T_CAP, generator=torch.Generator().manual_seed(0)) * 0.3).to(dev)
    frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
    n_in = B * SPF * T_CAP

    def call(rate, fmt):
        if rate is None:
            return ops.wave_pack(wave, frames, fmt=fmt, out=outs[(rate, fmt)])
        return ops.wave_resample_pack(wave, frames, rate, fmt=fmt, out=outs[(rate, fmt)])

    outs, times = {}, {}
    for name, rate, fmt in LEGS:
        U, D = (1, 1) if rate is None else resample.table(rate, dev)[:2]
        outs[(rate, fmt)] = torch.empty((B * resample.output_samples(SPF * T_CAP, U, D),), device=dev,
                                        dtype=ops.OUTPUT_FORMATS[fmt][1])
        for _ in range(10):
            call(rate, fmt)
        times[name] = []
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, rate, fmt in LEGS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call(rate, fmt)
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / a.calls)
    lines = []
    for name, rate, fmt in LEGS:
        out = outs[(rate, fmt)]
        t = times[name]
        d2h = out.numel() * out.element_size()
        lines.append(dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                          calls=a.calls, rounds=a.rounds, samples_in=n_in, samples_out=out.numel(), bytes_read=4 * n_in,
                          bytes_written=d2h, device_to_host_bytes=d2h,
                          gb_per_s=round((4 * n_in + d2h) / (statistics.median(t) * 1e-6) / 1e9, 1)))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
