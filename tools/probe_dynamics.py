"""`st2_wave_dynamics` at the headline's size, rows of 10 s, beside `wave_limit` and `wave_edges` over the
same rows, and the hand-over with and without it: device time per call from events around `--calls` back-to-back calls, after a
warm-up, the legs taking turns over `--rounds` rounds, in one process.  One JSON line per leg: min / median / max of the rounds in
microseconds.  The rows are noise whose level rises and falls by 30 dB twice a second around the threshold, so that the curve,
the release and the attack all have work.  Needs a HIP device; there is nothing to fall back to.  The headline itself
(`bench.py`) runs none of this code; it is compared between two checkouts in processes of their own.

    python tools/probe_dynamics.py [--calls 50] [--rounds 3] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from styletts2_amd import ops, pipeline, resample  # noqa: E402

SPF, T_CAP = 600, 400  # 10 s at 24 kHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_dynamics needs a HIP device")
    dev = "cuda"
    legs = {}
    L = SPF * T_CAP
    env = 10.0 ** ((-25.0 + 15.0 * torch.sin(torch.arange(L) * (2 * math.pi * 2 / 24000))) / 20.0)
    for B in (8, 32):
        wave = (torch.randn(B, L, generator=torch.Generator().manual_seed(B)) * env).to(dev)
        frames = torch.full((B,), T_CAP, dtype=torch.int32, device=dev)
        dy = pipeline.Dynamics(B, device=dev)
        win = resample.limit_window(dy.A, dev)
        work = torch.empty((ops.wave_dynamics_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        out, dyn = torch.empty_like(wave), torch.empty((B, 2), device=dev)
        legs["wave_dynamics B=%d" % B] = lambda w=wave, f=frames, d=dy, o=out, t=dyn, ws=work: ops.wave_dynamics(
            w, f, d.params, win, A=d.A, rho=d.rho, out=o, dynamics=t, workspace=ws)
        # the limiter over the same rows, behind its level measurement (run once: the table it reads)
        target = torch.zeros((B,), device=dev)
        level = ops.wave_level(wave, frames, target, ceiling=0.89, max_gain_db=60.0)
        lwin = resample.limit_window(192, dev)
        lwork = torch.empty((ops.wave_limit_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        lim = torch.empty((B, 2), device=dev)
        legs["wave_limit B=%d" % B] = lambda w=wave, f=frames, t=target, lv=level, ws=lwork, o=out, l=lim: ops.wave_limit(
            w, f, lv, t, lwin, ceiling=0.89, max_gain_db=60.0, out=o, limit=l, workspace=ws)
        e = pipeline.Edges(B, device=dev)
        ework = torch.empty((ops.wave_edges_workspace_bytes(B, T_CAP, SPF),), dtype=torch.uint8, device=dev)
        ramp, etab = resample.edge_ramp(e.F, dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        legs["wave_edges B=%d" % B] = lambda w=wave, f=frames, e=e, o=out, t=etab, ws=ework: ops.wave_edges(
            w, f, e.top_db, e.keep, ramp, out=o, edges=t, workspace=ws)
        if B != 32:
            continue
        for rate, fmt in ((None, "s16"), (8000, "ulaw")):
            if rate is not None:
                resample.table(rate, dev)
            for name, d in (("plain", None), ("dynamics", dy)):
                legs["hand_over %s %s %s B=32" % (fmt, rate or 24000, name)] = lambda w=wave, f=frames, d=d, r=rate, fm=fmt: \
                    pipeline._hand_over_edges(w, f, 0, fm, SPF, r, **({} if d is None else {"dynamics": d}))
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
