"""`st2_wave_volume` at the headline's size, rows of 10 s, with default settings and per-token tables
present, beside `wave_dynamics` and `wave_edges` over the same rows, and the hand-over with and without it: device time per call
from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns over `--rounds` rounds, in one process.
One JSON line per leg: min / median / max of the rounds in microseconds; the volume legs also carry the arithmetic floor -- one
read and one write of the valid samples at the float4-copy rate of an MI355X, 6.29 TB/s -- and the multiple of it reached.
The rows are noise; 40 tokens of a quarter of a second each, every third one 3 dB up and every seventh one 6 dB down, under a
row gain of -2 dB, so that every block is scaled and no vector is kept.  Needs a HIP device; there is nothing to fall back to.
The headline itself (`bench.py`) runs none of this code; it is compared between two checkouts in processes of their own.

    python tools/probe_volume.py [--calls 50] [--rounds 3] [--out FILE]
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

SPF, T_CAP, N = 600, 400, 40  # 10 s at 24 kHz
COPY_RATE = 6.29e12  # bytes per second of a float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_volume needs a HIP device")
    dev = "cuda"
    legs, floors = {}, {}
    L = SPF * T_CAP
    for B in (8, 32):
        wave = (torch.randn(B, L, generator=torch.Generator().manual_seed(B)) * 0.1).to(dev)
        frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
        tok = torch.zeros((B, N))
        tok[:, ::3], tok[:, ::7] = 3.0, -6.0
        vo = pipeline.Volume(B, db=-2.0, tok_db=tok, device=dev)
        pos = (torch.arange(N + 1, dtype=torch.int32) * (L // N)).repeat(B, 1).contiguous().to(dev)
        win = resample.limit_window(vo.A, dev)
        work = torch.empty((ops.wave_volume_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        out, vol = torch.empty_like(wave), torch.empty((B, 2), device=dev)
        name = "wave_volume B=%d" % B
        legs[name] = lambda w=wave, f=frames, p=pos, v=vo, o=out, t=vol, ws=work: ops.wave_volume(
            w, f, p, v.db, v.tok_db, win, A=v.A, out=o, volume=t, workspace=ws)
        floors[name] = 1e6 * 2 * 4 * B * L / COPY_RATE
        dy = pipeline.Dynamics(B, device=dev)
        dwin = resample.limit_window(dy.A, dev)
        dwork = torch.empty((ops.wave_dynamics_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        dyn = torch.empty((B, 2), device=dev)
        legs["wave_dynamics B=%d" % B] = lambda w=wave, f=frames, d=dy, o=out, t=dyn, ws=dwork: ops.wave_dynamics(
            w, f, d.params, dwin, A=d.A, rho=d.rho, out=o, dynamics=t, workspace=ws)
        e = pipeline.Edges(B, device=dev)
        ework = torch.empty((ops.wave_edges_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        ramp, etab = resample.edge_ramp(e.F, dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        legs["wave_edges B=%d" % B] = lambda w=wave, f=frames, e=e, o=out, t=etab, ws=ework: ops.wave_edges(
            w, f, e.top_db, e.keep, ramp, out=o, edges=t, workspace=ws)
        if B != 32:
            continue
        dur = torch.full((B, N), T_CAP // N, dtype=torch.int64, device=dev)
        tokens = dict(dur=dur, frames=frames, T_cap=T_CAP, lengths=None, shift=False, trim=0, samples_per_frame=SPF)
        for rate, fmt in ((None, "s16"), (8000, "ulaw")):
            if rate is not None:
                resample.table(rate, dev)
            for kind, more in (("plain", {}), ("volume", dict(volume=vo, tokens=tokens))):
                legs["hand_over %s %s %s B=32" % (fmt, rate or 24000, kind)] = lambda w=wave, f=frames, m=more, r=rate, fm=fmt: \
                    pipeline._hand_over_edges(w, f, 0, fm, SPF, r, **m)
    times = {name: [] for name in legs}
    for call in legs.values():
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
    lines = []
    for name, t in times.items():
        line = dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                    calls=a.calls, rounds=a.rounds)
        if name in floors:
            line.update(floor_us=round(floors[name], 2), times_floor=round(statistics.median(t) / floors[name], 2))
        lines.append(line)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
