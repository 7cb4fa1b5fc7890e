"""`st2_pitch_shape` at B = 8 and 32 rows of 400 frames and 128 tokens with every table present, beside
`ops.prosody_controls_tok` over the same rows -- the parent's kernel over the same bytes, and the yardstick --: device time per
call from events around `--calls` back-to-back calls, after a warm-up, the legs taking turns over `--rounds` rounds, in one process.
One JSON line per leg: min / median / max of the rounds in microseconds.  The calls work in place, so after a few of them the
curve sits at its clamps; the work of a call does not depend on the values (a clamped column stays voiced and is shaped again).
Needs a HIP device; there is nothing to fall back to.  The headline itself (`bench.py`) runs none of this code; it is compared
between two checkouts in processes of their own.

    python tools/probe_intonation.py [--calls 50] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from styletts2_amd import ops  # noqa: E402

T_CAP, N, K = 400, 128, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_intonation needs a HIP device")
    dev = "cuda"
    legs = {}
    for B in (8, 32):
        g = torch.Generator().manual_seed(B)
        f0 = 80.0 * torch.exp2(2.3 * torch.rand(B, 2 * T_CAP, generator=g))
        f0[torch.rand(B, 2 * T_CAP, generator=g) < 0.3] = 0.0  # unvoiced stretches
        f0, n = f0.to(dev), torch.randn(B, 2 * T_CAP, generator=g).to(dev)
        frames = torch.randint(T_CAP // 2, T_CAP + 1, (B,), generator=g).to(torch.int32).to(dev)
        dur = torch.full((B, N), T_CAP // N, dtype=torch.int64, device=dev)
        rng = (0.5 + torch.rand(B, generator=g)).to(dev)
        tok = (0.5 + torch.rand(B, N, generator=g)).to(dev)
        con = torch.stack([torch.linspace(0, 1, K).expand(B, K), 6.0 * torch.randn(B, K, generator=g)], dim=-1).contiguous().to(dev)
        pitch = torch.empty((B, 4), device=dev)
        legs["pitch_shape B=%d" % B] = lambda f=f0, r=rng, t=tok, d=dur, c=con, fr=frames, p=pitch: ops.pitch_shape(
            f, range=r, tok_range=t, dur=d, contour=c, frames=fr, shift=True, pitch=p)
        legs["pitch_shape measure only B=%d" % B] = lambda f=f0, fr=frames, p=pitch: ops.pitch_shape(f, frames=fr, pitch=p)
        sc = (0.9 + 0.2 * torch.rand(B, N, generator=g)).to(dev)
        sh = (0.1 * torch.randn(B, N, generator=g)).to(dev)
        legs["prosody_controls_tok B=%d" % B] = lambda f=f0.clone(), x=n, d=dur, s=sc, h=sh, fr=frames: ops.prosody_controls_tok(
            f, x, d, s, h, frames=fr, shift=True)
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
