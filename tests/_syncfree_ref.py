"""The contracts of the sync-free entry points (include/st2.h `st2_frames_from_durations`, `st2_wave_pack`; DESIGN.md section
11) restated in numpy / torch-CPU: what tests/test_syncfree_gpu.py compares the kernels against.  Not product code."""
import numpy as np
import torch

PCM_SCALE = np.float32(32767.0)


def frames_from_durations(dur, lengths, T_cap):
    """dur int64 [B, N], lengths [B] or None -> (frames int32 [B], over [B] bool): the row sums over n < lengths[b], clamped to
    1..T_cap; `over` marks the rows whose sum exceeded the capacity (ST2_STATUS_FRAME_CAPACITY)."""
    dur = dur.cpu().long()
    B, N = dur.shape
    if lengths is not None:
        keep = torch.arange(N).unsqueeze(0) < lengths.cpu().long().clamp(0, N).reshape(-1, 1)
        dur = dur * keep
    tot = dur.sum(dim=1)
    return tot.clamp(1, T_cap).to(torch.int32), tot > T_cap


def pcm16(x):
    """fp32 -> int16: rint(clamp(x, -1, 1) * 32767) in fp32 (np.rint rounds half to even), NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    y = np.rint(np.clip(x, np.float32(-1.0), np.float32(1.0)) * PCM_SCALE)
    return np.where(np.isnan(x), np.float32(0.0), y).astype(np.int16)


def wave_pack(wave, frames, T_cap, samples_per_frame=600, trim=0, fmt="s16"):
    """wave fp32 [B, L], frames [B] -> (packed 1-D int16 / float32, offsets int64 [B + 1]): row b's first
    max(0, samples_per_frame * clamp(frames[b], 0, T_cap) - trim) samples, converted, back to back.  fp32 rows are copied
    bit for bit (compare them as uint32: NaN payloads included)."""
    wave = np.asarray(wave, dtype=np.float32)
    n = [max(0, samples_per_frame * min(max(int(f), 0), T_cap) - trim) for f in frames]
    offsets = np.zeros(len(n) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(n)
    rows = [wave[b, :n[b]] for b in range(len(n))]
    if fmt == "s16":
        packed = np.concatenate([pcm16(r) for r in rows]) if rows else np.zeros(0, np.int16)
    else:
        packed = np.concatenate(rows).astype(np.float32, copy=False)
    return packed, offsets
