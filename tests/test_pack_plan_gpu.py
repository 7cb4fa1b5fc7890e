"""One row scan serves `st2_wave_pack`, `st2_wave_resample_pack` and `st2_wave_pack_gaps` (csrc/st2_passage.hip `pack_plan`):
the offsets of all three against the int64 numpy count, across the scan's 64-row chunk, and the packed bytes against the
contract of tests/_passage_ref.py.  Rows are 24 samples at most."""
import numpy as np
import pytest
import torch

import _passage_ref as R
import _resample_ref as RS
import _syncfree_ref as S
from styletts2_amd import ops, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPF, T_CAP, TRIM, MAX_GAP = 8, 3, 5, 9
SENTINEL = {"f32": 7.5, "s16": 0x5A5A, "ulaw": 0x5A}  # differs from every format's silence code
TORCH_DT = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8}
FORMATS = [(None, "f32"), (None, "s16"), (8000, "s16"), (8000, "ulaw"), (44100, "s16"), (44100, "ulaw")]


def _case(B):
    g = np.random.default_rng(100 + B)
    frames = g.choice(np.array([0, 1, 2, 3, 7], dtype=np.int32), size=B)  # 0: no samples (1 and trim = 5 neither); 7: clamped to 3
    gaps = g.choice(np.array([-3, 0, 1, 9, 40], dtype=np.int32), size=B)  # negative: none; 40: clamped to 9
    wave = (g.standard_normal((B, SPF * T_CAP)) * 0.6).astype(np.float32)
    return wave, frames, gaps


def _wrapped(wave, frames, rate, fmt, **kw):
    if rate is None:
        return ops.wave_pack(wave, frames, trim=TRIM, fmt=fmt, samples_per_frame=SPF, **kw)
    return ops.wave_resample_pack(wave, frames, rate, fmt=fmt, trim=TRIM, samples_per_frame=SPF, **kw)


def _counts(frames, rate):
    U, D = (1, 1) if rate is None else resample.ratio(rate)
    n, m = RS.row_counts(frames, T_CAP, SPF, TRIM, U, D)
    want = (np.maximum(0, SPF * np.clip(frames.astype(np.int64), 0, T_CAP) - TRIM) * U + D - 1) // D
    assert np.asarray(m).tolist() == want.tolist()
    return [int(v) for v in want]


@pytest.mark.parametrize("rate,fmt", FORMATS)
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_offsets_and_bytes_of_the_three_entries(B, rate, fmt):
    wave_np, frames_np, gaps_np = _case(B)
    wave, frames = torch.from_numpy(wave_np).to(DEV), torch.from_numpy(frames_np).to(DEV)
    gaps = torch.from_numpy(gaps_np).to(DEV)
    m = _counts(frames_np, rate)
    # the wrapped entry
    packed0, offs0 = _wrapped(wave, frames, rate, fmt)
    want0 = R.offsets(m, None, 0)
    assert offs0.dtype == torch.int64 and offs0.cpu().tolist() == want0.tolist()
    total0 = int(want0[-1])
    p0 = packed0.cpu().numpy()
    if rate is None:  # the plain move against numpy, byte for byte
        ref, roff = S.wave_pack(wave_np, frames_np, T_CAP, SPF, TRIM, fmt)
        assert roff.tolist() == want0.tolist() and p0[:total0].tobytes() == ref.tobytes()
    rows = [p0[want0[b]:want0[b + 1]].copy() for b in range(B)]
    # the gaps entry without gaps: the wrapped entry
    packed1, offs1 = ops.wave_pack_gaps(wave, frames, None, MAX_GAP, rate=rate, fmt=fmt, trim=TRIM, samples_per_frame=SPF)
    assert torch.equal(offs1, offs0) and packed1[:total0].cpu().numpy().tobytes() == p0[:total0].tobytes()
    # and with them
    want, woff, _ = R.pack_gaps(rows, gaps_np.tolist(), MAX_GAP, fmt)
    assert woff.tolist() == R.offsets(m, gaps_np.tolist(), MAX_GAP).tolist()
    packed2, offs2 = ops.wave_pack_gaps(wave, frames, gaps, MAX_GAP, rate=rate, fmt=fmt, trim=TRIM, samples_per_frame=SPF)
    assert offs2.dtype == torch.int64 and offs2.cpu().tolist() == woff.tolist()
    assert packed2[:int(woff[-1])].cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("rate,fmt", [(None, "s16"), (8000, "ulaw")])
def test_nothing_is_written_at_or_past_a_short_out(rate, fmt):
    B = 65
    wave_np, frames_np, gaps_np = _case(B)
    wave, frames = torch.from_numpy(wave_np).to(DEV), torch.from_numpy(frames_np).to(DEV)
    gaps = torch.from_numpy(gaps_np).to(DEV)
    m = _counts(frames_np, rate)
    full = _wrapped(wave, frames, rate, fmt)[0].cpu().numpy()
    off0 = R.offsets(m, None, 0)
    rows = [full[off0[b]:off0[b + 1]].copy() for b in range(B)]
    for g, call in ((None, lambda out: _wrapped(wave, frames, rate, fmt, out=out)),
                    (gaps_np.tolist(), lambda out: ops.wave_pack_gaps(wave, frames, gaps, MAX_GAP, rate=rate, fmt=fmt, trim=TRIM,
                                                                      samples_per_frame=SPF, out=out))):
        total = int(R.offsets(m, g, MAX_GAP)[-1])
        cap = total // 2 + 3  # inside the batch, on no row's boundary in particular
        want, woff, limit = R.pack_gaps(rows, g, MAX_GAP, fmt, cap)
        assert limit == cap < total
        whole = torch.full((total + 64,), SENTINEL[fmt], dtype=TORCH_DT[fmt], device=DEV)
        packed, offs = call(whole[:cap])
        assert offs.cpu().tolist() == woff.tolist()  # the offsets do not depend on the bound
        got = whole.cpu().numpy()
        assert got[:cap].tobytes() == want.tobytes()
        assert got[cap:].tobytes() == np.full(got[cap:].shape, SENTINEL[fmt], dtype=got.dtype).tobytes(), "written at or past the bound"
