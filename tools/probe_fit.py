"""Fitting a batch's durations to frame targets at B = 32 / N = 512 and at B = 8 / N = 128: the one
`st2_durations_fit` launch next to `st2_frames_from_durations` at the same shapes -- the floor of a one-workgroup-per-row launch
over these rows -- and next to what a caller had to do before: read the durations back, apportion them in numpy, upload them
again for a second call with `durations=` (the read-back waits for the device; the second call itself is not in the figure).
Device time per call from events around `--calls` back-to-back calls, host time per call from the clock around issuing them
(the host leg: around the whole round trip, which ends in a wait), after a warm-up, the legs taking turns over `--rounds`
rounds, in one process.  One JSON line per leg: min / median / max of the rounds in microseconds.  Needs a HIP device; there is
nothing to fall back to.

    python tools/probe_fit.py [--calls 200] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from styletts2_amd import ops  # noqa: E402


def numpy_fit(dur, target):
    """Largest-remainder apportionment of the excess over one frame per token, vectorised over the rows (no held tokens)."""
    v = np.maximum(dur, 1)
    m = v - 1
    M = np.maximum(m.sum(axis=1, keepdims=True), 1)
    R = (target - dur.shape[1])[:, None]
    q, r = R * m // M, R * m % M
    K = R[:, 0] - q.sum(axis=1)
    order = np.argsort(-r, axis=1, kind="stable")
    extra = np.zeros_like(q)
    np.put_along_axis(extra, order, (np.arange(dur.shape[1])[None, :] < K[:, None]).astype(q.dtype), axis=1)
    return 1 + q + extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_fit needs a HIP device")
    dev = "cuda"
    legs = {}
    for B, N in ((32, 512), (8, 128)):
        g = torch.Generator().manual_seed(B)
        dur = torch.randint(1, 12, (B, N), generator=g).to(dev)
        T_cap = int(dur.sum(dim=1).max()) * 2
        target = (dur.sum(dim=1) * 5 // 4).to(torch.int32)
        hold = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        out, rep = torch.empty_like(dur), torch.empty((B, 4), dtype=torch.int32, device=dev)
        want = numpy_fit(dur.cpu().numpy(), target.cpu().numpy().astype(np.int64))
        got, _ = ops.durations_fit(dur, target, T_cap, hold=hold)
        assert np.array_equal(got.cpu().numpy(), want) and got.sum(dim=1).tolist() == target.tolist()

        def fit(dur=dur, target=target, T_cap=T_cap, hold=hold, out=out, rep=rep):
            ops.durations_fit(dur, target, T_cap, hold=hold, out=out, report=rep)

        def frames(dur=dur, T_cap=T_cap):
            ops.frames_from_durations(dur, None, T_cap)

        def host(dur=dur, th=target.cpu().numpy().astype(np.int64)):
            d = dur.cpu().numpy()  # waits for the device
            torch.from_numpy(numpy_fit(d, th)).to(dev, non_blocking=True)

        legs["durations_fit B=%d N=%d" % (B, N)] = fit
        legs["frames_from_durations B=%d N=%d" % (B, N)] = frames
        legs["read back + numpy + upload B=%d N=%d" % (B, N)] = host
    dev_us, host_us = {name: [] for name in legs}, {name: [] for name in legs}
    for call in legs.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, call in legs.items():
            calls = a.calls if not name.startswith("read back") else max(a.calls // 10, 1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h0 = time.perf_counter()
            for _ in range(calls):
                call()
            h1 = time.perf_counter()
            t1.record()
            t1.synchronize()
            dev_us[name].append(1e3 * t0.elapsed_time(t1) / calls)
            host_us[name].append(1e6 * (h1 - h0) / calls)
    lines = []
    for name in legs:
        t, h = dev_us[name], host_us[name]
        lines.append(dict(leg=name, us_min=round(min(t), 2), us_median=round(statistics.median(t), 2), us_max=round(max(t), 2),
                          host_us_min=round(min(h), 2), host_us_median=round(statistics.median(h), 2), host_us_max=round(max(h), 2),
                          calls=a.calls, rounds=a.rounds))
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
