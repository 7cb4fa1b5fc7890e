"""`st2_wave_limit` at the headline's size, rows of 10 s, and the hand-over with and without it: device
time per call from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns over `--rounds` rounds, in
one process.  One JSON line per leg: min / median / max of the rounds in microseconds.  The rows are noise whose peaks stand 6 dB
over the ceiling after the drive gain, so that every launch has its full work.  Needs a HIP device; there is nothing to fall back
to.  The headline itself (`bench.py`) runs none of this code; it is compared between two checkouts in processes of their own.

    python tools/probe_limit.py [--calls 100] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from styletts2_amd import ops, pipeline, resample  # noqa: E402

SPF, T_CAP, W = 600, 400, 192  # 10 s at 24 kHz; the default window of 8 ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_limit needs a HIP device")
    dev = "cuda"
    legs = {}
    win, tp = resample.limit_window(W, dev), resample.true_peak_table(dev)
    for B in (8, 32):
        wave = (torch.randn(B, SPF * T_CAP, generator=torch.Generator().manual_seed(B)) * 0.1).to(dev)
        frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
        target = torch.zeros((B,), device=dev)  # 0 LUFS: the drive term decides
        level = torch.empty((B, 4), device=dev)
        work = torch.empty((ops.wave_level_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        lwork = torch.empty((ops.wave_limit_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        out, lim = torch.empty_like(wave), torch.empty((B, 2), device=dev)
        legs["wave_level B=%d" % B] = lambda w=wave, f=frames, t=target, lv=level, ws=work: ops.wave_level(
            w, f, t, ceiling=0.89, max_gain_db=60.0, out=lv, workspace=ws)
        for name, more in (("sample", {}), ("true_peak", dict(true_peak=tp))):
            legs["wave_limit %s B=%d" % (name, B)] = lambda w=wave, f=frames, t=target, lv=level, ws=lwork, o=out, l=lim, m=more: \
                ops.wave_limit(w, f, lv, t, win, ceiling=0.89, max_gain_db=60.0, out=o, limit=l, workspace=ws, **m)
        if B != 32:
            continue
        for rate, fmt in ((None, "s16"), (8000, "ulaw")):
            if rate is not None:
                resample.table(rate, dev)
            for name, lv in (("level", pipeline.Level(B, target=0.0, max_gain_db=60.0, device=dev)),
                             ("level+limiter", pipeline.Level(B, target=0.0, max_gain_db=60.0, device=dev, limiter=True))):
                legs["hand_over %s %s %s B=32" % (fmt, rate or 24000, name)] = lambda w=wave, f=frames, lv=lv, r=rate, fm=fmt: \
                    pipeline._hand_over(w, f, 0, fm, SPF, r, level=lv)
    times = {name: [] for name in legs}
    for call in legs.values():  # wave_level B runs before wave_limit B: the table the limiter reads is written
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, call in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call()
            t1.record()
            t1.synchronize()
            times[name].append(1e3 * t0.elapsed_time(t1) / a.calls)
    lines = [dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                  calls=a.calls, rounds=a.rounds) for name, t in times.items()]
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
