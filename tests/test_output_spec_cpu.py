"""The output options of the sync-free path: every refusal they can run into, with its exception type and
its text as recorded in tests/golden/output_refusals.json; the spec `pipeline._output_spec` makes of them and the hand-over layout
`_hand_over` allocates for that spec, against the formulas of DESIGN.md section 20 written out here; and `SynthesisResult.to_host()` cutting a
hand-filled buffer of that layout into rows, marks and level.  The `ops` wrappers are spied; no GPU needed."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from styletts2_amd import ops, pipeline

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "output_refusals.json")))
L, SPF, N, T = 1200, 600, 5, 2
SIZE = {"f32": 4, "s16": 2, "ulaw": 1}
DTYPE = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8}
NP = {"f32": np.float32, "s16": np.int16, "ulaw": np.uint8}


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _arg(v, dev="cpu"):
    """A table entry as the argument it stands for: {"Level": n} a `Level` of n rows, {"zeros": shape} a tensor of zeros."""
    if isinstance(v, dict) and "Level" in v:
        return pipeline.Level(v["Level"], device=dev)
    if isinstance(v, dict) and "zeros" in v:
        return torch.zeros(v["zeros"], dtype=getattr(torch, v.get("dtype", "float32")), device=dev)
    return v


def call(entry, args):
    """The table's call: two rows of five tokens, or two sentences, and no model -- the refusals come before anything needs one."""
    kw = {k: _arg(v) for k, v in args.items()}
    if entry == "inference":
        return pipeline.inference(None, None, torch.zeros(2, 5, dtype=torch.long), **kw)
    return pipeline.synthesize_long(None, None, [torch.zeros(5, dtype=torch.long), torch.zeros(3, dtype=torch.long)], **kw)


HOST = [c for c in GOLDEN if c["entry"] in ("inference", "synthesize_long")]


@pytest.mark.parametrize("case", HOST, ids=["%s: %s" % (c["entry"], c["fault"]) for c in HOST])
def test_single_fault_calls_raise_the_recorded_type_and_text(case):
    with pytest.raises(Exception) as e:
        call(case["entry"], case["args"])
    assert type(e.value).__name__ == case["raises"] and str(e.value) == case["text"]


def test_the_table_covers_every_entry_point_and_one_fault_reads_the_same_from_all_of_them():
    by_fault = {}
    for c in GOLDEN:
        by_fault.setdefault(c["fault"], {})[c["entry"]] = c["text"]
    assert {e for c in GOLDEN for e in [c["entry"]]} == {"inference", "synthesize_long", "graphed", "inference_device"}
    for fault in ("bad pack", "sample_rate without pack", "bad sample_rate", "gaps without pack", "negative max_gap",
                  "gaps of the wrong count", "gaps of a float dtype", "level of the wrong row count", "level without pack"):
        texts = by_fault[fault]
        assert {"inference", "synthesize_long"} <= set(texts) and len(set(texts.values())) == 1, fault
    assert set(by_fault["bad sample_rate"]) == set(by_fault["level without pack"]) == {"inference", "synthesize_long", "graphed"}
    assert by_fault["gaps without pack"]["inference"] == by_fault["max_gap without pack"]["graphed"]
    # the one statement with its subsets: three of them
    tail = " belong to the capacity-bound path: pass max_frames"
    assert {c["text"][:-len(tail)] for c in GOLDEN if c["text"].endswith(tail)} == {
        "passage / gaps / max_gap / s_prev", "pack / trim / lengths_dev", "pack / sample_rate / marks / gaps / max_gap / level"}


# ---- the spec and the layout it states -----------------------------------------------------------------------------------------
@pytest.fixture
def spied(monkeypatch):
    seen = []

    def spy(name):
        def f(wave, frames, *a, **kw):
            seen.append(name)
            return kw["out"], kw["offsets"]
        return f
    for name in ("wave_pack", "wave_resample_pack", "wave_pack_gaps", "wave_pack_level"):
        monkeypatch.setattr(ops, name, spy(name))
    monkeypatch.setattr(ops, "wave_level", lambda wave, frames, target, **kw: seen.append("wave_level") or kw["out"])
    monkeypatch.setattr(pipeline.resample, "table", lambda rate, dev: pipeline.resample.ratio(rate) + (0, None))
    return seen


def _build(B, fmt, sample_rate, marks, gaps, level, n_marks):
    """The one direct use of the spec function -> (the spec's fields, the hand-over `_hand_over` makes of them, handed on as
    `_decode_capacity` hands them on, the rows as tensors)."""
    wave, frames = torch.zeros(B, 1, L), torch.ones(B, dtype=torch.int32)
    spec, g = pipeline._output_spec(B, True, pack=fmt, trim=0, sample_rate=sample_rate, marks=marks, gaps=gaps, level=level)
    ho = pipeline._hand_over(wave, frames, spec.trim, spec.fmt, SPF, spec.sample_rate, n_marks if spec.marks else 0, g, spec.max_gap,
                             level)
    return spec._asdict(), ho, (wave, frames)


@pytest.mark.parametrize("B,fmt,sample_rate,marks,gaps,level", list(itertools.product(
    (1, 3), ("f32", "s16", "ulaw"), (None, 24000, 16000), (False, True), (False, True), (False, True))))
def test_spec_fields_and_layout_against_the_formulas_written_out(spied, B, fmt, sample_rate, marks, gaps, level):
    n_marks = B * (N + 1) if marks else 0
    gap_list = [3, 0, 7][:B] if gaps else None
    lv = pipeline.Level(B, device="cpu") if level else None
    f, ho, _ = _build(B, fmt, sample_rate, marks, gap_list, lv, B * (N + 1))
    max_gap = max(gap_list) if gaps else 0
    serves = sample_rate in (None, 24000) and fmt in ("f32", "s16")  # `ops.wave_pack`: fp32 / 16-bit PCM at the model's rate
    assert serves == (not pipeline._resamples(fmt, sample_rate))
    assert f == dict(fmt=fmt, trim=0, sample_rate=sample_rate, rate=None if serves else (sample_rate or 24000), marks=marks,
                     max_gap=max_gap)
    assert f["marks"] is marks
    # DESIGN.md section 20's formulas
    marks_at = 8 * (B + 1)
    gaps_at = marks_at + 4 * n_marks
    level_at = gaps_at + (4 * B if gaps else 0)
    samples_at = (level_at + (16 * B if level else 0) + 15) // 16 * 16
    assert type(ho) is pipeline._HandOver
    assert (ho.offsets_at, ho.marks_at, ho.gaps_at, ho.level_at, ho.samples_at) == (0, marks_at, gaps_at, level_at, samples_at)
    U, D = (1, 1) if f["rate"] is None else pipeline.resample.ratio(f["rate"])
    room = B * ((L * U + D - 1) // D + max_gap)
    assert ho.buf.dtype == torch.uint8 and ho.buf.numel() == samples_at + SIZE[fmt] * room
    assert ho.packed.dtype == DTYPE[fmt] and ho.packed.numel() == room and ho.offsets.dtype == torch.int64
    assert (ho.marks is None) == (not marks) and (ho.gaps is None) == (not gaps) and (ho.level is None) == (not level)
    if gaps:
        assert ho.gaps.tolist() == gap_list and ho.gaps.dtype == torch.int32
    assert spied == (["wave_level", "wave_pack_level"] if level else ["wave_pack_gaps"] if gaps else
                     ["wave_pack"] if serves else ["wave_resample_pack"])


# ---- to_host over a hand-filled buffer -------------------------------------------------------------------------------------------
def _result(B, fmt, marks, gaps, level):
    """A result as `_decode_capacity` makes it, over the hand-over of the spied `_hand_over`."""
    f, ho, (wave, frames) = _build(B, fmt, None, marks, gaps, level, B * (N + 1))
    spec = pipeline._Output(**f)
    return pipeline.SynthesisResult(wave, frames, T, spec, ho, marks=ho.marks.view(B, N + 1) if marks else None), ho


@pytest.fixture
def no_device(monkeypatch):
    """`to_host` without a device: pageable memory for the pinned mirror, an event that has nothing to wait for."""
    made, checked = [], []
    empty = torch.empty

    class Event:
        record = synchronize = lambda self, *a: None
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **kw: (made.append(1) if pin_memory else None) or empty(*a, **kw))
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: None)
    monkeypatch.setattr(ops, "check_status", lambda: checked.append(1))
    return made, checked


@pytest.mark.parametrize("fmt,marks,gaps,level", list(itertools.product(("s16", "ulaw"), (False, True), (False, True), (False, True))))
def test_to_host_returns_the_bytes_of_the_buffer(spied, no_device, fmt, marks, gaps, level):
    B, max_gap = 3, 10
    made, checked = no_device
    raw = [4, -9, 50]  # as the caller wrote them; the packing step counted 4, 0 and 10
    res, ho = _result(B, fmt, marks, [4, 0, max_gap] if gaps else None, pipeline.Level(B, device="cpu") if level else None)
    if gaps:
        assert res.max_gap == max_gap
    m = [7, 0, 12]
    g = [4, 0, 10] if gaps else [0, 0, 0]
    offs = [0]
    for b in range(B):
        offs.append(offs[-1] + m[b] + g[b])
    # the buffer by hand, part by part at DESIGN.md section 20's offsets; the pad holds 0xEE
    n_marks = B * (N + 1) if marks else 0
    marks_at = 8 * (B + 1)
    gaps_at = marks_at + 4 * n_marks
    level_at = gaps_at + (4 * B if gaps else 0)
    samples_at = (level_at + (16 * B if level else 0) + 15) // 16 * 16
    buf = np.full(ho.buf.numel(), 0xEE, dtype=np.uint8)
    buf[0:marks_at] = np.asarray(offs, dtype=np.int64).view(np.uint8)
    want_marks = (np.arange(n_marks, dtype=np.int32) * 3 + 1).reshape(B, N + 1) if marks else None
    if marks:
        buf[marks_at:gaps_at] = want_marks.reshape(-1).view(np.uint8)
    if gaps:
        buf[gaps_at:level_at] = np.asarray(raw, dtype=np.int32).view(np.uint8)
    want_level = (np.arange(4 * B, dtype=np.float32) - 23.5).reshape(B, 4) if level else None
    if level:
        buf[level_at:level_at + 16 * B] = want_level.reshape(-1).view(np.uint8)
    n = (buf.size - samples_at) // SIZE[fmt]
    samples = (np.arange(n) % 251 + 1).astype(NP[fmt])
    buf[samples_at:] = samples.view(np.uint8)
    ho.buf.copy_(torch.from_numpy(buf))

    def same(rows, passage=False):
        if passage:
            return rows.dtype == NP[fmt] and rows.tobytes() == samples[:offs[B]].tobytes()
        return len(rows) == B and all(r.dtype == NP[fmt] and r.tobytes() == samples[offs[b]:offs[b] + m[b]].tobytes()
                                      for b, r in enumerate(rows))
    rows = res.to_host()
    assert isinstance(rows, list) and same(rows)
    assert same(res.to_host(passage=True), passage=True)
    if marks:
        rows, mk = res.to_host(marks=True)
        assert same(rows) and mk.dtype == np.int32 and mk.shape == (B, N + 1) and mk.tobytes() == want_marks.tobytes()
    if level:
        rows, lv = res.to_host(level=True)
        assert same(rows) and lv.dtype == np.float32 and lv.shape == (B, 4) and lv.tobytes() == want_level.tobytes()
    if marks and level:
        rows, mk, lv = res.to_host(marks=True, level=True, passage=True)
        assert same(rows, passage=True) and mk.tobytes() == want_marks.tobytes() and lv.tobytes() == want_level.tobytes()
    assert made == [1] and len(checked) >= 2  # one pinned mirror per result; the status word is looked at behind every copy
    assert spied == (["wave_level", "wave_pack_level"] if level else ["wave_pack_gaps"] if gaps else ["wave_pack"] if fmt == "s16"
                     else ["wave_resample_pack"])  # `to_host` packs nothing again


def test_a_result_made_without_pack_packs_as_fp32_once(spied, no_device):
    wave, frames = torch.zeros(2, 1, L), torch.ones(2, dtype=torch.int32)
    res = pipeline.SynthesisResult(wave, frames, T)
    assert res.pack is None and res.packed is None and res.offsets is None and res.trim == 0 and res.sample_rate == 24000
    assert res.samples_per_frame == SPF and res.max_gap == 0 and res.gaps is None and res.level is None and res.marks is None
    rows = res.to_host()
    assert spied == ["wave_pack"] and len(rows) == 2 and all(r.dtype == np.float32 for r in rows)
    assert res.pack is None and res.packed.dtype == torch.float32 and res.packed.numel() == 2 * L and res.offsets.numel() == 3
    res.to_host()
    assert spied == ["wave_pack"] and no_device[0] == [1]
