"""`st2_wave_breaks` at the headline's size, 32 rows of 10 s of 100 tokens with four pauses of 300 ms each,
beside `st2_wave_edges` over the same rows: device time per call from events around `--calls` back-to-back calls, after a
warm-up, the legs taking turns over `--rounds` rounds, in one process.  One JSON line per leg: min / median / max of the rounds
in microseconds.  The breaks leg also carries its arithmetic floor -- one read of the valid samples for the block sums, one
read of them and one write of them with their silence for the move, at the 6.29 TB/s a float4 copy reaches on this part -- and
the ratio to it; the floor is arithmetic from the rows' sizes, not a counter reading.  Needs a HIP device; there is nothing to
fall back to.  The headline itself (`bench.py`) runs none of this code; it is compared between two checkouts in processes of
their own.

    python tools/probe_breaks.py [--calls 50] [--rounds 3] [--out FILE]
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

SPF, T_CAP, B, N = 600, 400, 32, 100  # 10 s at 24 kHz, four frames a token
HBM_BYTES_PER_US = 6.29e6             # the measured float4-copy rate, bytes per microsecond


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_breaks needs a HIP device")
    dev = "cuda"
    L = SPF * T_CAP
    wave = torch.randn(B, L, generator=torch.Generator().manual_seed(B)) * 0.1
    wave[:, :12000] = 0.0
    wave[:, L - 12000:] = 0.0
    wave = wave.to(dev)
    frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
    dur = torch.full((B, N), T_CAP // N, dtype=torch.int64, device=dev)
    ms = [[300.0 if n in (20, 40, 60, 80) else 0.0 for n in range(N)]] * B
    br = pipeline.Breaks(B, N, ms=ms, device=dev)
    e = pipeline.Edges(B, device=dev)
    ramp = resample.edge_ramp(br.F, dev)
    pos = ops.token_marks(dur, frames, T_CAP, samples_per_frame=SPF)
    out = torch.empty((B, L + br.max_break), device=dev)
    ins, cuts = torch.empty((B, N), dtype=torch.int32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev)
    table = torch.empty((B, 2), dtype=torch.int32, device=dev)
    work = torch.empty((ops.wave_breaks_workspace_bytes(B, T_CAP, SPF, N),), dtype=torch.uint8, device=dev)
    ework = torch.empty((ops.wave_edges_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
    eout, edges = torch.empty_like(wave), torch.empty((B, 2), dtype=torch.int32, device=dev)
    tokens = dict(dur=dur, frames=frames, T_cap=T_CAP, lengths=None, shift=False, trim=0, samples_per_frame=SPF)
    legs = {
        "wave_breaks B=32": lambda: ops.wave_breaks(wave, frames, pos, br.samples, br.max_break, ramp, out=out, ins=ins, cuts=cuts,
                                                    breaks=table, workspace=work),
        "wave_edges B=32": lambda: ops.wave_edges(wave, frames, e.top_db, e.keep, ramp, out=eout, edges=edges, workspace=ework),
    }
    for fmt, rate in (("s16", None), ("ulaw", 8000)):
        if rate is not None:
            resample.table(rate, dev)
        legs["hand_over %s %s B=32" % (fmt, rate or 24000)] = lambda fm=fmt, r=rate: pipeline._hand_over(wave, frames, 0, fm, SPF, r)
        legs["hand_over %s %s breaks B=32" % (fmt, rate or 24000)] = lambda fm=fmt, r=rate: pipeline._hand_over_edges(
            wave, frames, 0, fm, SPF, r, breaks=br, tokens=tokens)
    times = {name: [] for name in legs}
    for call in legs.values():
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    inserted = int(table[:, 1].sum().item())  # read once, outside the timed rounds
    floor_us = 4.0 * (3 * B * L + inserted) / HBM_BYTES_PER_US
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
    lines[0].update(inserted_samples=inserted, floor_us_arithmetic=round(floor_us, 2), over_floor=round(lines[0]["us_median"] / floor_us, 2))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
