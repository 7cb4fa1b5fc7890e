"""The hand-over allocation of the sync-free path as `pipeline._HandOver` states it: the byte offsets of
its four parts, the views of a device buffer and of its host mirror, and `pipeline._hand_over`, which returns that one object
whatever it was asked for.  The `ops` wrappers are spied; no GPU needed."""
import itertools

import pytest
import torch

from styletts2_amd import ops, pipeline

L, SPF, N, MAX_GAP = 1200, 600, 5, 7
SIZE = {"f32": 4, "s16": 2, "ulaw": 1}
DTYPE = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8}


@pytest.fixture
def spied(monkeypatch):
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append(name)
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    return seen


@pytest.mark.parametrize("B,marks,gaps,fmt", list(itertools.product((1, 3), (False, True), (False, True), ("f32", "s16", "ulaw"))))
def test_layout_views_and_the_one_return_type(spied, B, marks, gaps, fmt):
    n_marks = B * (N + 1) if marks else 0
    lay = pipeline._HandOver(B, fmt, n_marks, gaps)
    # the parent's formulas, written out
    assert lay.offsets_at == 0 and lay.marks_at == 8 * (B + 1) and lay.gaps_at == 8 * (B + 1) + 4 * n_marks
    assert lay.samples_at == (8 * (B + 1) + 4 * n_marks + (4 * B if gaps else 0) + 15) // 16 * 16

    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    g = torch.arange(B, dtype=torch.int32) if gaps else None
    ho = pipeline._hand_over(wave, frames, 0, fmt, SPF, None, n_marks=n_marks, gaps=g, max_gap=MAX_GAP if gaps else 0)
    assert type(ho) is pipeline._HandOver and len(spied) == 1
    assert spied[0] == ("wave_pack_gaps" if gaps else "wave_resample_pack" if fmt == "ulaw" else "wave_pack")
    room = B * (L + (MAX_GAP if gaps else 0))
    assert ho.buf.dtype == torch.uint8 and ho.buf.numel() == lay.samples_at + SIZE[fmt] * room
    assert ho.packed.dtype == DTYPE[fmt] and ho.packed.numel() == room
    assert (ho.marks is None) == (not marks) and (ho.gaps is None) == (not gaps)
    if gaps:
        assert ho.gaps.tolist() == g.tolist()

    host = torch.zeros(ho.buf.numel(), dtype=torch.uint8)  # the pinned mirror's stand-in
    at = (lay.offsets_at, lay.marks_at, lay.gaps_at, lay.samples_at)
    sizes = (8 * (B + 1), 4 * n_marks, 4 * B, SIZE[fmt] * room)
    for dev_view, host_view, dev_attr, where, nbytes in zip(lay.views(ho.buf), lay.views(host),
                                                            (ho.offsets, ho.marks, ho.gaps, ho.packed), at, sizes):
        if dev_attr is None:
            assert dev_view is None and host_view is None
            continue
        for v, base in ((dev_view, ho.buf), (host_view, host), (dev_attr, ho.buf)):
            assert v.data_ptr() - base.data_ptr() == where and v.numel() * v.element_size() == nbytes
        assert dev_view.dtype == host_view.dtype == dev_attr.dtype
    assert lay.views(host)[0].dtype == torch.int64 and lay.views(host)[3].dtype == DTYPE[fmt]
