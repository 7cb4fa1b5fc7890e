"""`st2_wave_edges` at the headline's size, 32 rows of 10 s, beside the level measurement and the limiter
over the same rows: device time per call from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns
over `--rounds` rounds, in one process.  One JSON line per leg: min / median / max of the rounds in microseconds.  The edges leg
also carries its arithmetic floor -- one read of the valid samples for the block sums, one read and one write of the kept
samples for the move, at the 6.29 TB/s a float4 copy reaches on this part -- and the ratio to it; the floor is arithmetic from
the rows' sizes, not a counter reading.  The rows are half a second of silence, nine seconds of noise and half a second of
silence, so that every row is cut at both ends.  Needs a HIP device; there is nothing to fall back to.  The headline itself
(`bench.py`) runs none of this code; it is compared between two checkouts in processes of their own.

    python tools/probe_edges.py [--calls 100] [--rounds 3] [--out FILE]
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

SPF, T_CAP, W, B = 600, 400, 192, 32  # 10 s at 24 kHz; the limiter's default window of 8 ms
HBM_BYTES_PER_US = 6.29e6             # the measured float4-copy rate, bytes per microsecond


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_edges needs a HIP device")
    dev = "cuda"
    L = SPF * T_CAP
    wave = torch.randn(B, L, generator=torch.Generator().manual_seed(B)) * 0.1
    wave[:, :12000] = 0.0
    wave[:, L - 12000:] = 0.0
    wave = wave.to(dev)
    frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
    target = torch.zeros((B,), device=dev)
    level = torch.empty((B, 4), device=dev)
    work = torch.empty((ops.wave_level_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
    lwork = torch.empty((ops.wave_limit_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
    ework = torch.empty((ops.wave_edges_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
    out, lim, edges = torch.empty_like(wave), torch.empty((B, 2), device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
    e = pipeline.Edges(B, device=dev)
    ramp, win = resample.edge_ramp(e.F, dev), resample.limit_window(W, dev)
    legs = {
        "wave_edges B=32": lambda: ops.wave_edges(wave, frames, e.top_db, e.keep, ramp, out=out, edges=edges, workspace=ework),
        "wave_level B=32": lambda: ops.wave_level(wave, frames, target, ceiling=0.89, max_gain_db=60.0, out=level, workspace=work),
        "wave_limit sample B=32": lambda: ops.wave_limit(wave, frames, level, target, win, ceiling=0.89, max_gain_db=60.0, out=out,
                                                         limit=lim, workspace=lwork),
    }
    for fmt, rate in (("s16", None), ("ulaw", 8000)):
        if rate is not None:
            resample.table(rate, dev)
        legs["hand_over %s %s B=32" % (fmt, rate or 24000)] = lambda fm=fmt, r=rate: pipeline._hand_over(wave, frames, 0, fm, SPF, r)
        legs["hand_over %s %s edges B=32" % (fmt, rate or 24000)] = lambda fm=fmt, r=rate: pipeline._hand_over_edges(wave, frames, 0, fm, SPF, r,
                                                                                                             edges=e)
    times = {name: [] for name in legs}
    for call in legs.values():
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    kept = int(edges[:, 1].sum().item())  # read once, outside the timed rounds
    floor_us = 4.0 * (B * L + 2 * kept) / HBM_BYTES_PER_US
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
    lines[0].update(kept_samples=kept, floor_us_arithmetic=round(floor_us, 2), over_floor=round(lines[0]["us_median"] / floor_us, 2))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
