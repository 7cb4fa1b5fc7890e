"""The volume stage of the hand-over on the device: `st2_wave_volume` against the numpy contract of
tests/_volume_ref.py -- the gains per block to one fp32 ulp, which is the last ulp of fp64 pow, with 0 and 1 exact; over the
device's own gains every output sample bit for bit, kept words included; the report to bits over the device's own output --
then `volume=` through the pipeline.  Shapes are the smallest at which the kernels can still go wrong: row lengths around one
block and one tile of the apply launch at one sample per frame, windows from none to longer than a row, token boundaries at
the block centres."""
import functools

import numpy as np
import pytest
import torch

import _volume_ref as R
from styletts2_amd import _lib, ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = np.float32(-7.25)
INF, NAN = float("inf"), float("nan")
LENGTHS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 31]
L = max(LENGTHS) + 5  # the capacity, at one sample per frame
N = 12
# token n's gain: NaN (= 0), -inf (= silent), a boost, +inf (= +20), -60, +20, 0 dB stretches, a cut, one under the range
TOK_DB = np.array([NAN, -INF, 3.0, INF, -60.0, 20.0, 0.0, -6.5, 0.0, 6.0, -70.0, 0.0], dtype=np.float32)
ROW_DB = [0.0, -3.0, 2.5, INF, -INF, NAN, -60.0, 20.0, 0.0]  # by length; the two longest rows with tokens are at 0 dB themselves
NB = [0, 1, N, 1, 0, N, 0, 1, N]  # the rows' token counts, by length
BATCHES = [(0, 3, 8), (1, 6, 5), (4, 7, 2)]  # three rows of different n each, with Nb = 0, 1 and N


def boundaries(n):
    """int32 [N + 1]: the first tokens collapsed to 0 as after an edge trim, boundaries at 64 k + 31 / 32 / 33, two at one sample,
    a token of several tiles, everything past the row's end at n."""
    raw = [0, 0, 0, 64 + 31, 2 * 64 + 32, 2 * 64 + 32, 4 * 64 + 33, 20 * 64, 40 * 64 + 31, 60 * 64 + 32, 64 * 64 + 33, 100 * 64, n]
    return np.minimum(np.array(raw, dtype=np.int64), n).astype(np.int32)


def samples(n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 0.2).astype(np.float32)
    for at, word in ((0, 0x7fc12345), (5, 0xff800000), (33, 0x7f923456), (70, 0x00000013), (71, 0x807fffff), (1300, 0x7f800000),
                     (1301, 0xffc00001), (2600, 0x7fa00001), (4094, 0x00000001), (4100, 0x7fc00777)):
        if at < n:  # NaN payloads (quiet and signalling), both infinities, denormals: in kept stretches and in scaled ones
            x[at:at + 1].view(np.uint32)[0] = word
    return x


def _win(A):
    return None if A == 0 else resample.limit_window(A, DEV)


def _win_host(A):
    return None if A == 0 else resample.limit_window_design(A)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _t(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def run(wave, frames, pos, lengths, db, tok_db, A, spf=1, trim=0):
    """One `ops.wave_volume` call into a canary-filled `out` with a row stride of its own -> (out, vol, lin) as numpy."""
    B, width = wave.shape
    T_cap = width // spf
    out = torch.full((B, width + 3), float(CANARY), device=DEV)
    work = torch.full((ops.wave_volume_workspace_bytes(B, T_cap, spf) // 4,), float(CANARY), device=DEV)
    got, vol = ops.wave_volume(torch.from_numpy(wave).to(DEV), _t(frames, torch.int32), _t(pos, torch.int32), _t(db, torch.float32),
                               _t(tok_db, torch.float32), _win(A), A=A, lengths=_t(lengths, torch.int32), trim=trim, samples_per_frame=spf,
                               out=out[:, :width], workspace=work.view(torch.uint8))
    assert got.data_ptr() == out.data_ptr() and vol.dtype == torch.float32 and tuple(vol.shape) == (B, 2)
    kcap = (width + 63) // 64
    return out.cpu().numpy(), vol.cpu().numpy(), work.cpu().numpy()[:B * kcap].reshape(B, kcap)


def check_row(x, n, pos, Nb, db, tok_db, A, out, vol, lin, tag):
    """Every bar of the issue for one row: `out` the whole row with its stride pad, `lin` its row of the workspace."""
    assert (out[n:] == CANARY).all(), (tag, "written at or past n, or outside the row's stride")
    K = (n + 63) // 64
    assert (lin[K:] == CANARY).all(), (tag, "lin written past the row's blocks")
    st = R.row_stages(n, pos, Nb, db, tok_db, A, _win_host(A))
    assert R.ulp_diff(lin[:K], st["lin"]).max(initial=0) <= 1, (tag, "lin", R.ulp_diff(lin[:K], st["lin"]).max())
    assert np.array_equal(lin[:K] == 0, st["lin"] == 0) and np.array_equal(lin[:K] == 1, st["lin"] == 1), (tag, "silent and 0 dB are exact")
    want = R.apply_gain(x[:n], lin[:K])
    made = np.isinf(x[:n]) & (R.sample_gain(lin[:K], n) == 0) if n else np.zeros(0, dtype=bool)  # inf * 0: a NaN that is MADE, whose
    #                                  sign an x86 host and the device choose differently; a NaN that came in keeps its payload on both
    assert np.array_equal(bits(out[:n])[~made], bits(want)[~made]) and np.isnan(out[:n][made]).all(), (tag, "rule 5 over the device's lin")
    i = np.arange(n, dtype=np.int64)
    ka = (i >> 6) - ((i & 63) < 32)
    keep = (lin[np.clip(ka, 0, max(K - 1, 0))] == 1) & (lin[np.clip(ka + 1, 0, max(K - 1, 0))] == 1) if n else np.zeros(0, dtype=bool)
    assert np.array_equal(bits(out[:n])[keep], bits(x[:n])[keep]), (tag, "words are kept where both gains are 1")
    assert np.array_equal(bits(vol), bits(R.report(out[:n], lin[:K]))), (tag, vol, R.report(out[:n], lin[:K]))
    return int(keep.sum()), int((lin[:K] == 0).sum())


def _batch(rows):
    """The rows `rows` of the nine lengths as one batch: (wave, frames, pos, lengths, db)."""
    wave = np.stack([np.resize(samples(max(LENGTHS[r], 1), 40 + r), L) for r in rows]).astype(np.float32)
    for b, r in enumerate(rows):
        wave[b, LENGTHS[r]:] = 0.77  # what lies past the row's end must not be read
    return (wave, [LENGTHS[r] for r in rows], np.stack([boundaries(LENGTHS[r]) for r in rows]), [NB[r] for r in rows],
            np.array([ROW_DB[r] for r in rows], dtype=np.float32))


@pytest.mark.parametrize("A", [0, 1, 3, 64])
@pytest.mark.parametrize("rows", BATCHES)
def test_lengths_windows_boundaries_and_hard_values_against_the_contract(rows, A):
    wave, frames, pos, lengths, db = _batch(rows)
    tok = np.stack([np.roll(TOK_DB, b) for b in range(3)])
    out, vol, lin = run(wave, frames, pos, lengths, db, tok, A)
    kept = silent = 0
    for b, r in enumerate(rows):
        k, s = check_row(wave[b], frames[b], pos[b], lengths[b], db[b], tok[b], A, out[b], vol[b], lin[b], (r, frames[b], lengths[b], A))
        kept, silent = kept + k, silent + s
    if 8 in rows and A <= 3:  # (a window of 129 blocks is wider than any token here: it leaves no stretch at 0 dB or silent)
        assert kept > 1000 and silent > 0, "the cases reach the kept words and the silent blocks"
    # absent tables: the row gain alone, the token gains alone, a bit copy
    out, vol, lin = run(wave, frames, pos, None, db, None, A)
    for b, r in enumerate(rows):
        check_row(wave[b], frames[b], pos[b], N, db[b], None, A, out[b], vol[b], lin[b], (r, "db alone"))
    out, vol, lin = run(wave, frames, pos, None, None, None, A)
    for b in range(3):
        assert np.array_equal(bits(out[b, :frames[b]]), bits(wave[b, :frames[b]])) and vol[b, 1] == 0 and (out[b, frames[b]:] == CANARY).all()
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("spf,T_cap,frames,trim", [(5, 1000, [0, 1, 13, 999, 1200], 3), (600, 8, [1, 2, 7, 9, 0], 100)])
def test_rows_in_frames_with_a_trim(spf, T_cap, frames, trim):
    width, B = spf * T_cap, len(frames)
    wave = np.stack([np.resize(samples(4800, 60 + b), width) for b in range(B)]).astype(np.float32)
    ns = [max(0, spf * min(max(f, 0), T_cap) - trim) for f in frames]
    pos = np.stack([np.minimum(boundaries(10 ** 9)[:N + 1] // 2, n).astype(np.int32) for n in ns])
    pos[:, N] = ns
    tok = np.stack([np.roll(TOK_DB, 2 * b) for b in range(B)])
    db = np.array(ROW_DB[:B], dtype=np.float32)
    out, vol, lin = run(wave, frames, pos, [N] * B, db, tok, 3, spf, trim)
    for b in range(B):
        check_row(wave[b], ns[b], pos[b], N, db[b], tok[b], 3, out[b], vol[b], lin[b], (b, ns[b]))
    assert ops.status() == 0


def test_a_row_alone_is_the_row_inside_a_batch():
    rows = (8, 6, 1)
    wave, frames, pos, lengths, db = _batch(rows)
    tok = np.stack([np.roll(TOK_DB, b) for b in range(3)])
    out, vol, lin = run(wave, frames, pos, lengths, db, tok, 3)
    order = [2, 0, 1]
    out2, vol2, lin2 = run(wave[order], [frames[i] for i in order], pos[order], [lengths[i] for i in order], db[order], tok[order], 3)
    for j, i in enumerate(order):
        assert np.array_equal(bits(out2[j]), bits(out[i])) and np.array_equal(bits(vol2[j]), bits(vol[i])) and np.array_equal(bits(lin2[j]), bits(lin[i]))
    for i in range(3):
        o1, v1, l1 = run(wave[i:i + 1], frames[i:i + 1], pos[i:i + 1], lengths[i:i + 1], db[i:i + 1], tok[i:i + 1], 3)
        assert np.array_equal(bits(o1[0]), bits(out[i])) and np.array_equal(bits(v1[0]), bits(vol[i])) and np.array_equal(bits(l1[0]), bits(lin[i]))


def test_a_captured_graph_replayed_with_three_table_sets_equals_three_eager_calls():
    rows, A = (8, 3, 4), 3
    wave, frames, pos, lengths, db = _batch(rows)
    sets = [(db, np.stack([np.roll(TOK_DB, b) for b in range(3)])), (np.array([6.0, NAN, -12.0], dtype=np.float32), np.zeros((3, N), dtype=np.float32)),
            (np.zeros(3, dtype=np.float32), np.stack([np.roll(TOK_DB[::-1], 3 * b) for b in range(3)]))]
    eager = [run(wave, frames, pos, lengths, d, t, A) for d, t in sets]
    w, f, p, ln = torch.from_numpy(wave).to(DEV), _t(frames, torch.int32), _t(pos, torch.int32), _t(lengths, torch.int32)
    s_db, s_tok = torch.zeros(3, device=DEV), torch.zeros((3, N), device=DEV)
    out = torch.full((3, L + 3), float(CANARY), device=DEV)
    vol = torch.zeros((3, 2), device=DEV)
    work = torch.zeros((ops.wave_volume_workspace_bytes(3, L, 1),), dtype=torch.uint8, device=DEV)
    win = _win(A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.wave_volume(w, f, p, s_db, s_tok, win, A=A, lengths=ln, samples_per_frame=1, out=out[:, :L], volume=vol, workspace=work)
    kcap = (L + 63) // 64
    for (d, t), (e_out, e_vol, e_lin) in zip(sets, eager):
        s_db.copy_(torch.from_numpy(d))
        s_tok.copy_(torch.from_numpy(t))
        g.replay()
        torch.cuda.synchronize()
        lin = work.view(torch.float32)[:3 * kcap].reshape(3, kcap).cpu().numpy()
        assert np.array_equal(bits(vol.cpu().numpy()), bits(e_vol))
        for b in range(3):
            n = frames[b]
            assert np.array_equal(bits(out[b].cpu().numpy()), bits(e_out[b])) and np.array_equal(bits(lin[b, :(n + 63) // 64]), bits(e_lin[b, :(n + 63) // 64]))
    assert ops.status() == 0


def test_wrapper_refuses_what_the_library_would():
    w = torch.zeros(2, 1200, device=DEV)
    f = torch.ones(2, dtype=torch.int32, device=DEV)
    p = torch.zeros((2, 5), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.St2Error, match="aliases"):
        ops.wave_volume(w, f, p, None, None, None, A=0, out=w)
    with pytest.raises(_lib.St2Error, match="too small"):
        ops.wave_volume(w, f, p, None, None, None, A=0, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.St2Error, match="A=65"):
        ops.wave_volume(w, f, p, None, None, torch.ones(131, device=DEV), A=65)
    with pytest.raises(_lib.St2Error, match="win"):
        ops.wave_volume(w, f, p, None, None, None, A=2)
    with pytest.raises(_lib.St2Error, match="win"):
        ops.wave_volume(w, f, p, None, None, torch.ones(1, device=DEV), A=0)
    with pytest.raises(_lib.St2Error, match="tok_db"):
        ops.wave_volume(w, f, p, None, torch.zeros((2, 5), device=DEV), None, A=0)
    with pytest.raises(_lib.St2Error, match="db"):
        ops.wave_volume(w, f, p, torch.zeros(3, device=DEV), None, None, A=0)
    with pytest.raises(_lib.St2Error, match="pos"):
        ops.wave_volume(w, f, p[:1], None, None, None, A=0)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
LENS2 = (12, 9)
G6 = np.float32(np.power(10.0, 6.0 / 20.0))


@functools.lru_cache(maxsize=None)
def _setup():
    """The synthetic multi-speaker model, two rows of 12 and 9 tokens with pinned draws, and the smallest capacity they fit."""
    from test_controls_gpu import STEPS, _batch as batch, _kw, _model
    man, model, sampler = _model("libritts")
    b = batch(True, LENS2)
    p0 = pipeline.prepare(model, sampler, b["tokens"], allow_ragged=True, ragged_decode=True, **_kw(b))
    T = max(p0["frames_host"])
    trim = 50 if model.decoder.kind == "hifigan" else 0
    kw = dict(_kw(b), sine_noise=b["sine"], lj_tail=False, trim=trim, max_frames=T)
    torch.cuda.synchronize()
    ops.status(clear=True)
    return dict(model=model, sampler=sampler, b=b, T=T, trim=trim, kw=kw, steps=STEPS, B=len(LENS2), N=max(LENS2))


def _reach(vol):
    """Samples on either side of a token's span that its gain can reach: the window, one block for the centre rule and one for
    the interpolation between centres."""
    return (vol.A + 2) * 64


@pytest.mark.parametrize("pack,rate", [("f32", None), ("s16", None), ("ulaw", 8000), ("alaw", 16000)])
def test_neutral_volume_gives_the_parents_bytes(pack, rate):
    S = _setup()
    more = dict(S["kw"], pack=pack, sample_rate=rate, marks=True)
    base = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], **more)
    res = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], volume=pipeline.Volume.neutral(S["B"], S["N"]), **more)
    total = int(base.offsets[-1])
    assert torch.equal(res.offsets, base.offsets) and torch.equal(res.marks, base.marks)
    assert res.packed[:total].cpu().numpy().tobytes() == base.packed[:total].cpu().numpy().tobytes()
    assert base.volume is None and res.volume[:, 1].tolist() == [0.0, 0.0] and bool((res.volume[:, 0] > 0).all())
    assert res._ho.buf.numel() == base._ho.buf.numel() + (res._ho.samples_at - base._ho.samples_at), "one allocation, one more part"
    torch.cuda.synchronize()
    ops.check_status()


def _confined(rows, base_rows, marks, b, n, reach):
    """Row b differs from the base inside token n's span and its reach alone, by exactly +6 dB well inside; the others not at all."""
    m0, m1 = int(marks[b, n]), int(marks[b, n + 1])
    assert m1 - m0 > 2 * reach + 64, "the token is longer than the two ramps"
    for r, (x, y) in enumerate(zip(rows, base_rows)):
        diff = np.flatnonzero(bits(x) != bits(y))
        if r != b:
            assert len(diff) == 0
            continue
        assert len(diff) and diff.min() >= m0 - reach and diff.max() < m1 + reach, (diff.min(), diff.max(), m0, m1, reach)
        assert np.array_equal(bits(x[m0 + reach:m1 - reach]), bits(y[m0 + reach:m1 - reach] * G6))


def test_a_token_at_plus_six_changes_its_span_and_the_ramps_alone(monkeypatch):
    S = _setup()
    B, N = S["B"], S["N"]
    more = dict(S["kw"], pack="f32", marks=True)
    base = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], **more)
    base_rows, base_marks = base.to_host(marks=True)
    base_rows = [r.copy() for r in base_rows]
    n = int(np.argmax(np.diff(base_marks[1, :LENS2[1] + 1])))  # the longest token of row 1
    tok = np.zeros((B, N), dtype=np.float32)
    tok[1, n] = 6.0
    vol = pipeline.Volume(B, tok_db=tok)
    res = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], volume=vol, **more)
    copies = []
    real = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a, **kw: (copies.append(self.is_pinned()), real(self, src, *a, **kw))[1])
    rows, marks, vh = res.to_host(marks=True, volume=True)
    monkeypatch.undo()
    assert copies == [True], "to_host(volume=True) is one copy, into the pinned mirror"
    assert np.array_equal(marks, base_marks) and torch.equal(res.offsets, base.offsets), "marks and offsets are unchanged"
    _confined(rows, base_rows, marks, 1, n, _reach(vol))
    assert vh.dtype == np.float32 and vh.tobytes() == res.volume.cpu().numpy().tobytes(), "the report comes over in the one copy"
    assert vh[0, 1] == 0 and vh[1, 1] >= (marks[1, n + 1] - marks[1, n]) // 64 - 1
    assert vh[0, 0] == np.abs(rows[0]).max() and vh[1, 0] == np.abs(rows[1]).max()
    with pytest.raises(ValueError, match="volume"):
        base.to_host(volume=True)
    for bad, word in ((pipeline.Volume(B + 1), "Volume of %d rows" % B), (pipeline.Volume(B, N + 1), "of %d tokens" % N),
                      (pipeline.Volume(B, device="cpu"), "holds its tables on cpu")):
        with pytest.raises(ValueError, match=word):
            pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], volume=bad, **more)
    torch.cuda.synchronize()
    ops.check_status()


def test_with_edges_breaks_dynamics_and_level_all_on():
    S = _setup()
    B, N = S["B"], S["N"]
    brk = np.zeros((B, N), dtype=np.int32)
    brk[1, 2], brk[0, 4] = 480, 240
    stages = dict(edges=pipeline.Edges(B), breaks=pipeline.Breaks(B, N, samples=brk.tolist(), max_ms=50.0), dynamics=pipeline.Dynamics(B, threshold_db=-40.0))
    more = dict(S["kw"], pack="f32", marks=True, **stages)
    base = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], **more)
    base_rows, base_marks = base.to_host(marks=True)
    base_rows = [r.copy() for r in base_rows]
    spans = np.diff(base_marks[1, :LENS2[1] + 1])
    spans[2] = 0  # not the token that holds the pause
    n = int(np.argmax(spans))
    tok = np.zeros((B, N), dtype=np.float32)
    tok[1, n] = 6.0
    vol = pipeline.Volume(B, tok_db=tok)
    res = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], volume=vol, **more)
    rows, marks, eh, bh, dh, vh = res.to_host(marks=True, edges=True, breaks=True, dynamics=True, volume=True)
    assert np.array_equal(marks, base_marks) and torch.equal(res.offsets, base.offsets) and np.array_equal(dh, base.dynamics.cpu().numpy())
    _confined(rows, base_rows, marks, 1, n, _reach(vol))  # the boundaries are those of the rows as cut and spliced
    assert vh[0, 1] == 0 and vh[1, 1] > 0
    # and with a level: the counts stay, the loudness is measured on the rows as voiced
    lv = pipeline.Level(B, target=-20.0)
    loud = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], volume=pipeline.Volume(B, db=[0.0, -6.0], tok_db=tok), level=lv, **more)
    plain = pipeline.inference(S["model"], S["sampler"], S["b"]["tokens"], level=lv, **more)
    assert torch.equal(loud.offsets, plain.offsets) and torch.equal(loud.marks, plain.marks)
    lh, ph = loud.level.cpu().numpy(), plain.level.cpu().numpy()
    assert np.array_equal(lh[0], ph[0]) and not np.array_equal(lh[1], ph[1]), "row 0 is at 0 dB: measured as ever"
    assert lh[1, 0] <= ph[1, 0] and lh[1, 1] <= ph[1, 1] and lh[1, 2] >= ph[1, 2], "row 1 was measured quieter and is raised by no less"
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_volume_and_equals_the_eager_call():
    S = _setup()
    B, N, b = S["B"], S["N"], S["b"]
    ld = b["lengths"].to(torch.int32).to(DEV)
    gs = pipeline.GraphedSynthesis(S["model"], S["sampler"], B, N, S["T"], S["steps"], ref_s=b["ref_s"], trim=S["trim"], lj_tail=False, pack="s16",
                                   volume=True)
    assert gs.static["volume"].A == 3 and not gs.static["volume"].db.any() and not gs.static["volume"].tok_db.any()
    tok = np.zeros((B, N), dtype=np.float32)
    tok[0, 3], tok[1, 5] = 6.0, -60.0
    first = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    graphs = []
    for call, vol in ((dict(first, volume=pipeline.Volume(B, db=[-3.0, 2.0], tok_db=tok)), pipeline.Volume(B, db=[-3.0, 2.0], tok_db=tok)),
                      (dict(volume=pipeline.Volume(B, db=[0.0, -12.0])), pipeline.Volume(B, db=[0.0, -12.0])), (dict(), None)):
        res = gs(**call)
        graphs.append(gs._g["graph"])
        rows, vh = res.to_host(volume=True)
        rows, vh = [r.copy() for r in rows], vh.copy()
        want = pipeline.inference(S["model"], S["sampler"], b["tokens"], pack="s16", **S["kw"], **({} if vol is None else {"volume": vol}))
        w_rows = want.to_host()
        assert all(np.array_equal(x, y) for x, y in zip(rows, w_rows))
        assert vol is None and vh[:, 1].tolist() == [0.0, 0.0] or vh.tobytes() == want.volume.cpu().numpy().tobytes()
    assert graphs[0] is graphs[1] is graphs[2], "no second capture"
    with pytest.raises(ValueError, match="ramp_ms is the graph's own"):
        gs(volume=pipeline.Volume(B, ramp_ms=0.0))
    with pytest.raises(ValueError, match="built without volume"):
        pipeline.GraphedSynthesis(S["model"], S["sampler"], B, N, S["T"], S["steps"], ref_s=b["ref_s"], pack="s16")(volume=pipeline.Volume(B))
    torch.cuda.synchronize()
    ops.check_status()


def test_synthesize_long_slices_the_rows_per_front_group():
    S = _setup()
    b, steps = S["b"], S["steps"]
    sentences = [b["tokens"][k, :LENS2[k]].clone() for k in range(2)]
    N = max(LENS2)
    common = dict(ref_s=b["ref_s"][:1], diffusion_steps=steps, noises=[b["noise"][k:k + 1] for k in range(2)],
                  step_noises=[b["step_noise"][:, k:k + 1].contiguous() for k in range(2)], sine_noises=[b["sine"][k:k + 1] for k in range(2)],
                  max_frames=S["T"] * 2, pack="f32", marks=True, trim=S["trim"], front_batch=1)
    plain, _ = pipeline.synthesize_long(S["model"], S["sampler"], sentences, volume=pipeline.Volume.neutral(2, N), **common)
    tok = np.zeros((2, N), dtype=np.float32)
    n = int(np.argmax(np.diff(plain[1].to_host(marks=True)[1][0, :LENS2[1] + 1])))
    tok[1, n] = 6.0
    vol = pipeline.Volume(2, db=[-6.0, 0.0], tok_db=tok)
    results, _ = pipeline.synthesize_long(S["model"], S["sampler"], sentences, volume=vol, **common)
    assert len(results) == len(plain) == 2 and all(tuple(r.volume.shape) == (1, 2) for r in results)
    quiet, old = results[0].to_host()[0], plain[0].to_host()[0].copy()
    assert np.array_equal(bits(quiet), bits(old * np.float32(np.power(10.0, -6.0 / 20.0)))), "sentence 0 takes row 0: its own gain, no token's"
    rows, marks = results[1].to_host(marks=True)
    _confined(rows, [plain[1].to_host()[0].copy()], marks, 0, n, _reach(vol))
    with pytest.raises(ValueError, match="Volume of 2 rows of %d tokens" % N):
        pipeline.synthesize_long(S["model"], S["sampler"], sentences, volume=pipeline.Volume(2, N + 1), **common)
    torch.cuda.synchronize()
    ops.check_status()
