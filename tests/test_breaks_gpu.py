"""Pauses inside a row on the device: `st2_wave_breaks` and `st2_token_marks_breaks` against the numpy
contract of tests/_breaks_ref.py, bit for bit -- the block sums have one fixed order, everything behind them is integers and
single fp32 operations -- then `breaks=` through the pipeline: the packed bytes are the parent path's packers run over the
reference's rows.  Shapes are the smallest at which the kernels can still go wrong: rows of more than one 2048-sample tile of
the sums' launch, row lengths around one block and one 4096-sample tile of the move, spans with no, one and many candidates,
B = 1, 5 and 17, N = 1, 7 and 512."""
import itertools

import numpy as np
import pytest
import torch

import _breaks_ref as R
from styletts2_amd import _lib, ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = int(np.array([R.SENTINEL]).view(np.uint32)[0])


def _dev(v, dtype):
    return torch.tensor(np.asarray(v), dtype=dtype, device=DEV)


def _run(c, F):
    """One `ops.wave_breaks` call over a batch of `_breaks_ref` into a sentinel-filled `out` -> (out bits, ins, cuts, breaks)."""
    wave = _dev(c["wave"], torch.float32)
    B, L = wave.shape
    out = torch.full((B, L + c["max_break"] + 2), float(R.SENTINEL), device=DEV)[:, :L + c["max_break"]]  # a row stride of its own
    ramp = resample.edge_ramp(F, DEV) if F else None
    got, ins, cuts, breaks = ops.wave_breaks(wave, _dev(c["frames"], torch.int32), _dev(c["pos"], torch.int32), _dev(c["brk"], torch.int32),
                                             c["max_break"], ramp, trim=c["trim"], samples_per_frame=c["spf"], out=out)
    assert got is out and all(t.dtype == torch.int32 for t in (ins, cuts, breaks)) and tuple(breaks.shape) == (B, 2)
    return out.cpu().numpy().view(np.uint32), ins.cpu().numpy(), cuts.cpu().numpy(), breaks.cpu().numpy()


def _compare(c, ref, got):
    bits, ins, cuts, breaks = got
    for b, (name, r) in enumerate(zip(c["names"], ref)):
        assert ins[b].tolist() == r["ins"].tolist() and cuts[b].tolist() == r["cuts"].tolist(), (b, name)
        assert breaks[b].tolist() == [r["count"], r["total"]], (b, name)
        assert np.array_equal(bits[b, :r["count"]], r["bits"]), (b, name)
        assert (bits[b, r["count"]:] == SENTINEL).all(), (b, name, "written at or past count'")


@pytest.mark.parametrize("B,N,F", list(itertools.product(R.BATCHES, R.TOKENS, R.FADES)))
def test_wave_breaks_equals_the_numpy_contract_bit_for_bit(B, N, F):
    c, ref = R.batch(B, N), R.reference(B, N, F)
    _compare(c, ref, _run(c, F))
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("F", [0, 48, 700])
def test_row_lengths_around_a_block_and_a_tile_of_the_move_and_fades_longer_than_segments(F):
    """n_b in {0, 63, 64, 127, 128, 129, 4095, 4096, 4097} as rows of one-sample frames; with F = 700 every segment of the short
    rows, and the segments between the cuts of the long ones, take f = length div 2 of the ramp."""
    c, ref = R.sizes_batch(), R.reference(0, 7, F)
    _compare(c, ref, _run(c, F))
    assert [r["count"] - r["total"] for r in ref] == R.SIZES and all(r["total"] == 61 for r in ref)


def test_short_segments_take_half_their_length_of_a_long_fade():
    c, ref = R.batch(17, 7), R.reference(17, 7, 700)
    _compare(c, ref, _run(c, 700))


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch():
    c = R.batch(17, 7)
    got = _run(c, 48)
    order = np.arange(17)[::-1].copy()
    flipped = {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    assert all(np.array_equal(a, b[order]) for a, b in zip(_run(flipped, 48), got))
    one = {k: (v[8:9] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    assert all(np.array_equal(a[0], b[8]) for a, b in zip(_run(one, 48), got))


def test_wrapper_refuses_what_the_library_would():
    w = torch.zeros(2, 1200, device=DEV)
    f = torch.ones(2, dtype=torch.int32, device=DEV)
    pos, brk = torch.zeros(2, 5, dtype=torch.int32, device=DEV), torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.St2Error, match="aliases"):
        ops.wave_breaks(w, f, pos, brk, 0, out=w)
    with pytest.raises(_lib.St2Error, match="F=4097"):
        ops.wave_breaks(w, f, pos, brk, 10, torch.ones(4097, device=DEV))
    with pytest.raises(_lib.St2Error, match="pos"):
        ops.wave_breaks(w, f, pos[:, :4].contiguous(), brk, 10)
    with pytest.raises(_lib.St2Error, match="max_break"):
        ops.wave_breaks(w, f, pos, brk, -1)
    with pytest.raises(_lib.St2Error, match="too small"):
        ops.wave_breaks(w, f, pos, brk, 10, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.St2Error, match="N=513"):
        ops.wave_breaks(w, f, torch.zeros(2, 514, dtype=torch.int32, device=DEV), torch.zeros(2, 513, dtype=torch.int32, device=DEV), 10)


# ---- the marks of rows with pauses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [24000, 8000, 44100])
@pytest.mark.parametrize("N", [7, 512])
def test_token_marks_breaks_equal_the_numpy_contract_and_end_at_the_packed_count(rate, N):
    c, ref = R.batch(5, N), R.reference(5, N, 48)
    n_b = [R.row_samples(f, c["T_cap"], c["spf"], c["trim"]) for f in c["frames"]]
    pos = np.array([R.boundaries(c["pos"][b], n_b[b]) for b in range(5)])  # what `token_marks` hands over: monotone, ending at n_b
    ins = np.array([r["ins"] for r in ref])
    U, D = resample.ratio(rate)
    m = ops.token_marks_breaks(_dev(pos, torch.int32), _dev(ins, torch.int32), rate=rate)
    assert m.dtype == torch.int32 and np.array_equal(m.cpu().numpy(), R.marks(pos, ins, U, D))
    counts = _dev([r["count"] for r in ref], torch.int32)
    rows = torch.zeros(5, c["spf"] * c["T_cap"] + c["max_break"], device=DEV)
    _, offs = (ops.wave_pack(rows, counts, fmt="s16", samples_per_frame=1) if rate == 24000 else
               ops.wave_resample_pack(rows, counts, rate, samples_per_frame=1))
    o = offs.cpu().numpy()
    assert m[:, N].cpu().tolist() == (o[1:] - o[:-1]).tolist(), "the last mark is the row's packed sample count"


# ---- end to end --------------------------------------------------------------------------------------------------------------------
MAX_MS = 50.0  # 1 200 samples a row


def _table(K, N):
    """Pauses for the K = 4 rows of the passage: one, two in adjacent tokens, none, and one that meets the cap of 1 200."""
    t = np.zeros((K, N), dtype=np.int32)
    t[0, 3], t[1, 2], t[1, 3], t[3, 5], t[3, 6] = 240, 100, 50, 1000, 900
    return t


def _reference_rows(res, base, table, br, edges, trim):
    """`_breaks_ref` over the result's own wave -- cut by `_edges_ref` first where the call trims -- with the boundaries the
    PARENT's marks give for the same call without breaks (`base`, s16 at 24 kHz: `st2_token_marks(_edges)` at U = D = 1)
    -> (rows [B, L + max_break] on the device, counts' int32 [B] on the device, the reference rows, pos)."""
    pos = base.to_host(marks=True)[1]
    ramp = resample.edge_ramp_design(br.F) if br.F else None
    if edges is None:
        w, fr = res.wave[:, 0].cpu().numpy(), res.frames.cpu().numpy()
        ref = R.breaks_batch(w, fr, res.max_frames, w.shape[1] // res.max_frames, trim, pos, table, br.max_break, ramp)
    else:
        from test_edges_gpu import _cut_rows
        cut, counts, _ = _cut_rows(res, edges, trim)
        w = cut.cpu().numpy()
        ref = R.breaks_batch(w, counts.cpu().numpy(), w.shape[1], 1, 0, pos, table, br.max_break, ramp)
    rows = np.zeros((w.shape[0], w.shape[1] + br.max_break), dtype=np.uint32)
    for b, r in enumerate(ref):
        rows[b, :r["count"]] = r["bits"]
    return _dev(rows.view(np.float32), torch.float32), _dev([r["count"] for r in ref], torch.int32), ref, pos


CASES = [("s16", None, None, None, False), ("ulaw", 8000, None, None, False), ("s16", None, [80, 0, 160, 40], None, True),
         ("s16", None, None, dict(target=-18.0), True), ("alaw", 16000, [10, 20, 0, 5], dict(target=-18.0, limiter=True), False)]


@pytest.mark.parametrize("pack,rate,gaps,level,trimmed", CASES)
def test_end_to_end_packed_bytes_are_the_parent_packers_over_the_reference_rows(pack, rate, gaps, level, trimmed):
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler = P["model"], P["sampler"]
    N = P["b"]["tokens"].shape[1]
    table = _table(K, N)
    br = pipeline.Breaks(K, N, samples=table.tolist(), max_ms=MAX_MS)
    edges = pipeline.Edges(K, top_db=[1.0, 2.0, None, 1.5], lead_ms=1.0, tail_ms=2.0) if trimmed else None
    lvl = None if level is None else pipeline.Level(K, **level)
    more = dict(P["kw"], max_frames=P["T"], marks=True, **({} if edges is None else {"edges": edges}))
    base = pipeline.inference(model, sampler, P["b"]["tokens"], pack="s16", **more)
    if gaps is not None:
        more.update(gaps=gaps)
    res = pipeline.inference(model, sampler, P["b"]["tokens"], pack=pack, sample_rate=rate, level=lvl, breaks=br, **more)
    got = res.to_host(marks=True, breaks=True)
    rows, marks, bh = got[0], got[1], got[-1]
    cut, counts, ref, pos = _reference_rows(res, base, table, br, edges, P["trim"])
    assert bh.tolist() == [[r["count"], r["total"]] for r in ref] == res.breaks.cpu().tolist()
    assert [r["total"] for r in ref] == [240, 150, 0, 1200] and ref[3]["ins"][[5, 6]].tolist() == [1000, 200], "row 3 meets the cap"
    # the parent path's packers over the reference's rows: frames = count', one-sample frames, nothing trimmed
    g = None if gaps is None else torch.tensor(gaps, dtype=torch.int32, device=DEV)
    max_gap = 0 if gaps is None else max(gaps)
    how = dict(fmt=pack, trim=0, samples_per_frame=1)
    if lvl is not None:
        tab = ops.wave_level(cut, counts, lvl.target, ceiling=lvl.ceiling, max_gain_db=lvl.max_gain_db, samples_per_frame=1)
        assert tab.cpu().numpy().tobytes() == res.level.cpu().numpy().tobytes()
    if lvl is not None and lvl.limiter:
        cut, limit = ops.wave_limit(cut, counts, tab, lvl.target, resample.limit_window(lvl.W, DEV), ceiling=lvl.ceiling,
                                    max_gain_db=lvl.max_gain_db, drive_db=lvl.drive_db, samples_per_frame=1)
        assert limit.cpu().numpy().tobytes() == res.limit.cpu().numpy().tobytes()
    if lvl is not None and not lvl.limiter:
        packed, offs = ops.wave_pack_level(cut, counts, tab, gaps=g, max_gap=max_gap, rate=rate, **how)
    elif gaps is not None:
        packed, offs = ops.wave_pack_gaps(cut, counts, g, max_gap, rate=rate, **how)
    elif rate is not None:
        packed, offs = ops.wave_resample_pack(cut, counts, rate, **how)
    else:
        packed, offs = ops.wave_pack(cut, counts, **how)
    o = offs.cpu().tolist()
    assert o == res.offsets.cpu().tolist()
    assert packed[:o[-1]].cpu().numpy().tobytes() == res.packed[:o[-1]].cpu().numpy().tobytes()
    U, D = resample.ratio(rate or resample.MODEL_RATE)
    assert np.array_equal(marks, R.marks(pos, np.array([r["ins"] for r in ref]), U, D))
    gl = [0] * K if gaps is None else gaps
    assert marks[:, -1].tolist() == [len(r) for r in rows] == [o[k + 1] - o[k] - gl[k] for k in range(K)]
    if (pack, rate, level, trimmed) == ("s16", None, None, False):
        # a break of K samples shows as exactly K zero samples inside its token's marks, and the row is K samples longer
        plain = base.to_host()
        for b, n in ((0, 3), (1, 2), (1, 3), (3, 5), (3, 6)):
            r = ref[b]
            at = int(r["cuts"][n] + r["ins"][:n].sum())
            assert marks[b, n] <= at and at + r["ins"][n] <= marks[b, n + 1] and not rows[b][at:at + r["ins"][n]].any(), (b, n)
        assert [len(x) - len(y) for x, y in zip(rows, plain)] == [240, 150, 0, 1200]
        assert np.array_equal(rows[2], plain[2]), "a row without a break is the parent's row"
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_break_table_without_a_second_capture():
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    N = b["tokens"].shape[1]
    ld = b["lengths"].to(torch.int32).to(DEV)
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, P["T"], STEPS, ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, pack="s16",
                                   marks=True, breaks=True, max_break_ms=MAX_MS)
    assert gs.static["breaks"].max_break == 1200 and not gs.static["breaks"].samples.any()
    other = np.zeros((K, N), dtype=np.int32)
    other[2, 1], other[0, 4] = 333, 77
    graphs = []
    for call, table in ((dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"],
                              breaks=_table(K, N).tolist()), _table(K, N)),
                        (dict(breaks=pipeline.Breaks(K, N, samples=other.tolist(), max_ms=MAX_MS)), other)):
        res = gs(**call)
        graphs.append(gs._g["graph"])
        rows, marks, bh = res.to_host(marks=True, breaks=True)
        want = pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], pack="s16", marks=True,
                                  breaks=pipeline.Breaks(K, N, samples=table.tolist(), max_ms=MAX_MS), **P["kw"])
        w_rows, w_marks, w_bh = want.to_host(marks=True, breaks=True)
        assert np.array_equal(bh, w_bh) and np.array_equal(marks, w_marks) and bh[:, 1].tolist() == np.minimum(table.sum(axis=1), 1200).tolist()
        assert all(np.array_equal(x, y) for x, y in zip(rows, w_rows))
    assert graphs[0] is graphs[1], "no second capture"
    with pytest.raises(ValueError, match="built without breaks"):
        pipeline.GraphedSynthesis(model, sampler, K, N, P["T"], STEPS, ref_s=P["ref_s"], pack="s16")(breaks=other.tolist())
    torch.cuda.synchronize()
    ops.check_status()


def test_synthesize_long_splices_pauses_into_its_sentences():
    from test_controls_gpu import STEPS
    from test_passage_gpu import _passage
    P = _passage("libritts")
    model, sampler = P["model"], P["sampler"]
    sentences = P["sentences"][:2]
    N = max(s.numel() for s in sentences)
    common = dict(ref_s=P["ref_s"], diffusion_steps=STEPS, noises=P["noises"][:2], step_noises=P["step_noises"][:2],
                  sine_noises=P["sines"][:2], max_frames=P["T"], pack="s16", marks=True, trim=P["trim"], front_batch=1)
    # the same rows without a pause (a table of zeros pads the sentences to N as well: a row with no break is a bit copy)
    plain, _ = pipeline.synthesize_long(model, sampler, sentences, breaks=pipeline.Breaks(2, N, max_ms=MAX_MS), **common)
    assert all(r.breaks[0].tolist() == [r.to_host(marks=True)[1][0, -1], 0] for r in plain)
    table = [[0] * N, [0] * N]
    table[0][2], table[1][4] = 120, 360
    results, _ = pipeline.synthesize_long(model, sampler, sentences, breaks=pipeline.Breaks(2, N, samples=table, max_ms=MAX_MS), **common)
    assert len(results) == len(plain) == 2
    for k, (res, old, n) in enumerate(zip(results, plain, (2, 4))):
        rows, marks, bh = res.to_host(marks=True, breaks=True)
        pos = old.to_host(marks=True)[1]
        assert bh[0, 1] == table[k][n] and len(rows[0]) == len(old.to_host()[0]) + table[k][n] == marks[0, -1]
        assert np.array_equal(marks[0, :n + 1], pos[0, :n + 1]) and np.array_equal(marks[0, n + 1:], pos[0, n + 1:] + table[k][n])
        silent = np.flatnonzero(rows[0][marks[0, n]:marks[0, n + 1]] == 0)
        assert len(silent) >= table[k][n], "the pause lies inside its token's marks"
    with pytest.raises(ValueError, match="Breaks of 2 rows of %d tokens" % N):
        pipeline.synthesize_long(model, sampler, sentences, breaks=pipeline.Breaks(2, N + 1), **common)
    torch.cuda.synchronize()
    ops.check_status()
