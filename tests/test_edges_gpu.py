"""Lead and tail silence trimmed on the device: `st2_wave_edges` and `st2_token_marks_edges` against the
numpy contract of tests/_edges_ref.py, bit for bit -- the block sums have one fixed order, everything behind them is integers
and single fp32 operations -- then `edges=` through the pipeline: the packed bytes are the parent path's packers run over the
reference's cut rows.  Shapes are the smallest at which the kernels can still go wrong: rows of more than one 2048-sample tile,
bursts at offsets that are no multiple of 512 or 4, row lengths around one block and one tile, B = 1, 5 and 17."""
import itertools

import numpy as np
import pytest
import torch

import _edges_ref as E
import _marks_ref as MR
from styletts2_amd import _lib, ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _run(c, F):
    """One `ops.wave_edges` call over a batch of `_edges_ref` into a sentinel-filled `out` -> (out bits [B, L], edges [B, 2])."""
    wave = _dev(c["wave"], torch.float32)
    out = torch.full_like(wave, float(E.SENTINEL))
    ramp = resample.edge_ramp(F, DEV) if F else None
    got, edges = ops.wave_edges(wave, _dev(c["frames"], torch.int32), _dev(c["top_db"], torch.float32), _dev(c["keep"], torch.int32),
                                ramp, trim=c["trim"], samples_per_frame=c["spf"], out=out)
    assert got is out and edges.dtype == torch.int32 and tuple(edges.shape) == (len(c["frames"]), 2)
    return _bits(out), edges.cpu().numpy()


def _compare(c, ref, bits, edges):
    sentinel = int(np.array([E.SENTINEL]).view(np.uint32)[0])
    for b, (name, r) in enumerate(zip(c["names"], ref)):
        assert edges[b].tolist() == [r["head"], r["count"]], (b, name)
        assert np.array_equal(bits[b, :r["count"]], r["bits"]), (b, name)
        assert (bits[b, r["count"]:] == sentinel).all(), (b, name, "written at or past count")


@pytest.mark.parametrize("B,geo,trim,F", list(itertools.product(E.BATCHES, E.GEOMETRIES, E.TRIMS, E.FADES)))
def test_wave_edges_equals_the_numpy_contract_bit_for_bit(B, geo, trim, F):
    spf, T_cap = geo
    c = E.batch(B, spf, T_cap, trim)
    ref = E.reference(B, spf, T_cap, trim, F)
    bits, edges = _run(c, F)
    _compare(c, ref, bits, edges)
    n_b = [E.row_samples(f, T_cap, spf, trim) for f in c["frames"]]
    assert sum(r["count"] < n for r, n in zip(ref, n_b)) >= (1 if B == 1 else 2), "the batch cuts something"
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("F", [0, 48, 700])
def test_row_lengths_around_a_block_and_a_tile_and_a_count_below_two_fades(F):
    """n_b in {300, 511, 512, 513, 2047, 2048} as rows of one-sample frames.  With F = 700 the two long rows, cut in front to
    about 1 030 samples, take f = count div 2 of the ramp; the short ones (count < 2 F as well) are cut nowhere and take no fade."""
    c = E.sizes_batch()
    ref = E.reference(0, 1, c["T_cap"], 0, F)
    bits, edges = _run(c, F)
    _compare(c, ref, bits, edges)
    assert [r["count"] for r in ref[:4]] == E.SIZES[:4] and all(0 < r["head"] and r["count"] < 2 * 700 for r in ref[4:])


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch():
    spf, T_cap = E.GEOMETRIES[1]
    c = E.batch(17, spf, T_cap, 3)
    bits, edges = _run(c, 48)
    order = np.arange(17)[::-1].copy()
    flipped = {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    bits2, edges2 = _run(flipped, 48)
    assert np.array_equal(edges2, edges[order]) and np.array_equal(bits2, bits[order])
    one = {k: (v[10:11] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    bits1, edges1 = _run(one, 48)
    assert np.array_equal(edges1[0], edges[10]) and np.array_equal(bits1[0], bits[10])


def test_wrapper_refuses_what_the_library_would():
    w = torch.zeros(2, 1200, device=DEV)
    f = torch.ones(2, dtype=torch.int32, device=DEV)
    td, keep = torch.full((2,), 20.0, device=DEV), torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.St2Error, match="aliases"):
        ops.wave_edges(w, f, td, keep, out=w)
    with pytest.raises(_lib.St2Error, match="F=4097"):
        ops.wave_edges(w, f, td, keep, torch.ones(4097, device=DEV))
    with pytest.raises(_lib.St2Error, match="top_db"):
        ops.wave_edges(w, f, td[:1], keep)
    with pytest.raises(_lib.St2Error, match="too small"):
        ops.wave_edges(w, f, td, keep, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))


# ---- the marks of cut rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [24000, 8000, 44100])
def test_token_marks_edges_equal_the_numpy_contract(rate):
    g = np.random.default_rng(rate)
    B, N, spf, trim = 5, 70, 600, 50
    dur = g.integers(0, 5, size=(B, N)).astype(np.int64)
    dur[4] = 0
    T_cap = int(dur.sum(axis=1).max())
    d = _dev(dur, torch.int64)
    lens = [0, 1, N, N, 33]
    ld = _dev(lens, torch.int32)
    frames = ops.frames_from_durations(d, ld, T_cap)
    fh = frames.cpu().numpy()
    n_smp = np.maximum(0, spf * fh.astype(np.int64) - trim)
    # heads and counts inside the rows, at their ends, empty, and (row 3) past the row: the kernel clamps what it is given
    edges = np.array([[0, n_smp[0]], [n_smp[1] // 3, n_smp[1] // 2], [1537, max(n_smp[2] - 4000, 0)], [700, n_smp[3] + 999],
                      [n_smp[4], 0]], dtype=np.int64)
    e = _dev(edges, torch.int32)
    U, D = resample.ratio(rate)
    for shift in (0, 1):
        m, bd = ops.token_marks_edges(d, frames, T_cap, e, lengths=ld, shift=bool(shift), trim=trim, rate=rate, want_bound=True)
        want = E.marks(dur, lens, fh, T_cap, shift, edges, spf, trim, U, D)
        assert np.array_equal(m.cpu().numpy(), want), shift
        assert np.array_equal(bd.cpu().numpy(), MR.bounds(dur, lens, fh, T_cap, shift))
        # the last mark is the packed sample count of the cut row: what the packers give for frames = count, one-sample frames
        counts = np.minimum(edges[:, 1], np.maximum(n_smp - edges[:, 0], 0))
        cut = torch.zeros(B, spf * T_cap, device=DEV)
        _, offs = (ops.wave_pack(cut, _dev(counts, torch.int32), fmt="s16", samples_per_frame=1) if rate == 24000 else
                   ops.wave_resample_pack(cut, _dev(counts, torch.int32), rate, samples_per_frame=1))
        o = offs.cpu().numpy()
        assert m[:, N].cpu().tolist() == (o[1:] - o[:-1]).tolist()
    same = ops.token_marks(d, frames, T_cap, lengths=ld, trim=trim, rate=rate)
    whole = _dev(np.stack([np.zeros(B, dtype=np.int64), n_smp], axis=1), torch.int32)
    assert torch.equal(ops.token_marks_edges(d, frames, T_cap, whole, lengths=ld, trim=trim, rate=rate), same)
    torch.cuda.synchronize()
    assert ops.status() & ~_lib.STATUS_FRAME_CAPACITY == 0
    ops.status(clear=True)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
# The seeded synthetic model is loud throughout.  A row's first and last frame are half zero padding, about 3 dB under the
# frames inside it, so thresholds of 1 to 2 dB cut every such row at both ends whatever it holds; row 2 is left alone.
TOP_DB = [1.0, 2.0, None, 1.5]


def _cut_rows(res, edges, trim):
    """`_edges_ref` over the result's own wave -> (the cut rows at the front of a zeroed [B, L] device tensor, counts int32 [B] on
    the device, the reference rows)."""
    w = res.wave[:, 0].cpu().numpy()
    fr = res.frames.cpu().numpy()
    spf = res.wave.shape[-1] // res.max_frames
    ramp = resample.edge_ramp_design(edges.F) if edges.F else None
    ref = E.edges_batch(w, fr, res.max_frames, spf, trim, edges.top_db.cpu().numpy(), edges.keep.cpu().numpy(), ramp)
    cut = np.zeros_like(w).view(np.uint32)
    for b, r in enumerate(ref):
        cut[b, :r["count"]] = r["bits"]
    return _dev(cut.view(np.float32), torch.float32), _dev([r["count"] for r in ref], torch.int32), ref


CASES = [("s16", None, None, None), ("ulaw", 8000, None, None), ("s16", None, [80, 0, 160, 40], None),
         ("s16", None, None, dict(target=-18.0)), ("alaw", 16000, [10, 20, 0, 5], dict(target=-18.0, limiter=True))]


@pytest.mark.parametrize("pack,rate,gaps,level", CASES)
def test_end_to_end_packed_bytes_are_the_parent_packers_over_the_reference_rows(pack, rate, gaps, level):
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler = P["model"], P["sampler"]
    edges = pipeline.Edges(K, top_db=TOP_DB, lead_ms=1.0, tail_ms=2.0, fade_ms=2.0)
    lvl = None if level is None else pipeline.Level(K, **level)
    more = dict(P["kw"], max_frames=P["T"], pack=pack, sample_rate=rate, marks=True)
    if gaps is not None:
        more.update(gaps=gaps)
    res = pipeline.inference(model, sampler, P["b"]["tokens"], level=lvl, edges=edges, **more)
    got = res.to_host(marks=True, edges=True)
    rows, marks, eh = got[0], got[1], got[-1]
    cut, counts, ref = _cut_rows(res, edges, P["trim"])
    assert eh.tolist() == [[r["head"], r["count"]] for r in ref] == res.edges.cpu().tolist()
    n_b = [E.row_samples(f, P["T"], 600, P["trim"]) for f in res.frames.cpu().tolist()]
    assert sum(r["count"] < n for r, n in zip(ref, n_b)) >= 2 and ref[2]["count"] == n_b[2], "rows are cut, row 2 is left alone"
    # the parent path's packers over the reference's rows: frames = count, one-sample frames, nothing trimmed
    g = None if gaps is None else torch.tensor(gaps, dtype=torch.int32, device=DEV)
    max_gap = 0 if gaps is None else max(gaps)
    how = dict(fmt=pack, trim=0, samples_per_frame=1)
    if lvl is not None:
        table = ops.wave_level(cut, counts, lvl.target, ceiling=lvl.ceiling, max_gain_db=lvl.max_gain_db, samples_per_frame=1)
        assert table.cpu().numpy().tobytes() == res.level.cpu().numpy().tobytes()
    if lvl is not None and lvl.limiter:
        cut, limit = ops.wave_limit(cut, counts, table, lvl.target, resample.limit_window(lvl.W, DEV), ceiling=lvl.ceiling,
                                    max_gain_db=lvl.max_gain_db, drive_db=lvl.drive_db, samples_per_frame=1)
        assert limit.cpu().numpy().tobytes() == res.limit.cpu().numpy().tobytes()
    if lvl is not None and not lvl.limiter:
        packed, offs = ops.wave_pack_level(cut, counts, table, gaps=g, max_gap=max_gap, rate=rate, **how)
    elif gaps is not None:
        packed, offs = ops.wave_pack_gaps(cut, counts, g, max_gap, rate=rate, **how)
    elif rate is not None:
        packed, offs = ops.wave_resample_pack(cut, counts, rate, **how)
    else:
        packed, offs = ops.wave_pack(cut, counts, **how)
    o = offs.cpu().tolist()
    assert o == res.offsets.cpu().tolist()
    assert packed[:o[-1]].cpu().numpy().tobytes() == res.packed[:o[-1]].cpu().numpy().tobytes()
    gl = [0] * K if gaps is None else gaps
    assert [len(r) for r in rows] == [o[k + 1] - o[k] - gl[k] for k in range(K)]
    # the marks are the cut rows': they end at the row's packed sample count and token 0 starts at its first sample
    assert marks[:, -1].tolist() == [len(r) for r in rows] and (marks[:, 0] == 0).all() and (np.diff(marks, axis=1) >= 0).all()
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_thresholds_without_a_second_capture():
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    ld = b["lengths"].to(torch.int32).to(DEV)
    gs = pipeline.GraphedSynthesis(model, sampler, K, b["tokens"].shape[1], P["T"], STEPS, ref_s=P["ref_s"], trim=P["trim"], lj_tail=False,
                                   pack="s16", edges=pipeline.Edges(K, top_db=TOP_DB, lead_ms=1.0, tail_ms=2.0))
    seen = []
    for call in (dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"]),
                 dict(edges=[None, 1.0, 1.0, 2.0])):
        res = gs(**call)
        graph = gs._g["graph"]
        rows, eh = res.to_host(edges=True)
        eh = eh.copy()
        cut, counts, ref = _cut_rows(res, gs.static["edges"], P["trim"])
        assert eh.tolist() == [[r["head"], r["count"]] for r in ref]
        packed, offs = ops.wave_pack(cut, counts, fmt="s16", trim=0, samples_per_frame=1)
        o = offs.cpu().tolist()
        assert o == res.offsets.cpu().tolist()
        assert packed[:o[-1]].cpu().numpy().tobytes() == res.packed[:o[-1]].cpu().numpy().tobytes()
        seen.append((eh, graph))
    assert seen[0][1] is seen[1][1], "no second capture"
    assert not np.array_equal(seen[0][0], seen[1][0]) and seen[1][0][0].tolist() == [0, E.row_samples(res.frames[0].item(), P["T"], 600, P["trim"])]
    with pytest.raises(ValueError, match="built without edges"):
        pipeline.GraphedSynthesis(model, sampler, K, b["tokens"].shape[1], P["T"], STEPS, ref_s=P["ref_s"], pack="s16")(edges=20.0)
    torch.cuda.synchronize()
    ops.check_status()
