"""`st2_wave_level`, with and without the true-peak launch and the passage scope of `st2_wave_level_ex`, and the gain in the
packing moves at the headline's size, rows of 10 s: device time per
call from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns over `--rounds` rounds, in one
process.  One JSON line per leg: min / median / max of the rounds in microseconds and the bytes the leg reads (by arithmetic: the
level call reads every valid sample once, 4 bytes each).  Needs a HIP device; there is nothing to fall back to.

    python tools/probe_level.py [--calls 100] [--rounds 3] [--out FILE]
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

SPF, T_CAP = 600, 400  # 10 s at 24 kHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_level needs a HIP device")
    dev = "cuda"
    legs = {}
    for B in (8, 32):
        wave = (torch.randn(B, SPF * T_CAP, generator=torch.Generator().manual_seed(B)) * 0.1).to(dev)
        frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
        target = torch.full((B,), -16.0, device=dev)
        level = torch.empty((B, 4), device=dev)
        work = torch.empty((ops.wave_level_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        legs["wave_level B=%d" % B] = (B, lambda w=wave, f=frames, t=target, lv=level, ws=work: ops.wave_level(
            w, f, t, ceiling=0.89, out=lv, workspace=ws))
        tp = resample.true_peak_table(dev)
        starts = torch.zeros((B,), dtype=torch.int32, device=dev)
        starts[::4] = 1  # passages of four sentences
        legs["wave_level true_peak B=%d" % B] = (B, lambda w=wave, f=frames, t=target, lv=level, ws=work, tp=tp: ops.wave_level(
            w, f, t, ceiling=0.89, out=lv, workspace=ws, true_peak=tp))
        legs["wave_level passage B=%d" % B] = (B, lambda w=wave, f=frames, t=target, lv=level, ws=work, st=starts: ops.wave_level(
            w, f, t, ceiling=0.89, out=lv, workspace=ws, starts=st))
        legs["wave_level true_peak passage B=%d" % B] = (B, lambda w=wave, f=frames, t=target, lv=level, ws=work, tp=tp, st=starts:
                                                         ops.wave_level(w, f, t, ceiling=0.89, out=lv, workspace=ws, true_peak=tp, starts=st))
        if B != 32:
            continue
        ops.wave_level(wave, frames, target, ceiling=0.89, out=level, workspace=work)
        for rate, fmt in ((None, "s16"), (8000, "ulaw")):
            U, D = (1, 1) if rate is None else resample.table(rate, dev)[:2]
            out = torch.empty((B * resample.output_samples(SPF * T_CAP, U, D),), device=dev, dtype=ops.OUTPUT_FORMATS[fmt][1])
            for name, lv in (("no gain", None), ("gain", level)):
                legs["pack_level %s %s %s B=32" % (fmt, rate or 24000, name)] = (B, lambda w=wave, f=frames, lv=lv, r=rate, fm=fmt, o=out:
                                                                                  ops.wave_pack_level(w, f, lv, rate=r, fmt=fm, out=o))
    times = {name: [] for name in legs}
    for _, call in legs.values():
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (_, call) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call()
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / a.calls)
    lines = []
    for name, (B, _) in legs.items():
        t, read = times[name], 4 * B * SPF * T_CAP
        lines.append(dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                          calls=a.calls, rounds=a.rounds, bytes_read=read,
                          read_gb_per_s=round(read / (statistics.median(t) * 1e-6) / 1e9, 1)))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
