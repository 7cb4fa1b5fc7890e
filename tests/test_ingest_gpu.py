"""`st2_clip_ingest` on the device against the fp64 contract of tests/_ingest_ref.py, and its place in
front of the style path: `compute_style(sample_rate=, encoding=)` from telephony bytes to ref_s, eagerly and in one graph.

The tolerance is derived, not tuned: fp32 fmaf accumulation of K terms differs from the exact sum by at most
(K + 1) 2^-24 sum_k |taps x| (section 15), which the reference computes per sample; no sample is excluded.  `start` / `len` are
exact because every constructed clip keeps its frames 3 dB from the threshold (tests/test_ingest_cpu.py asserts it)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _ingest_ref as I
import _resample_ref as R
from benchdata import manifest, synth
from styletts2_amd import _lib, models, ops, resample, style

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77.25
# what sits in `src` at and past n_b: NaN, or the loudest sample of the format
SRC_FILL = {"f32": np.float32(np.nan), "s16": np.int16(32767), "ulaw": np.uint8(0x00), "alaw": np.uint8(0x2A)}
TORCH = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}
CASES = [(r, f) for r in (8000, 16000, 22050, 44100, 48000) for f in ("f32", "s16")] + [(8000, "ulaw"), (8000, "alaw")]
M_TARGET = 3000  # samples at 24 kHz of a row at capacity: three 1024-sample tiles, the last one partial


def _n_below(target, U, D):
    """The largest n with ceil(n U / D) < target."""
    n = target * D // U + 2
    while resample.output_samples(n, U, D) >= target:
        n -= 1
    return n


def _n_above(target, U, D):
    n = target * D // U - 2
    while resample.output_samples(n, U, D) <= target:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def _edge_batches(rate, fmt):
    """Two batches of six rows: n_b = 0, 1, K // 2, one sample either side of the tile boundary at 1024 (and of the 512 boundary
    at 512 in the second batch), a row at N_cap.  -> [(buf, n, rows of the reference)]"""
    U, D, taps = resample.design_input(rate)
    K = taps.shape[1]
    N_cap = M_TARGET * D // U + 7
    L_cap = resample.output_samples(N_cap, U, D)
    rng = np.random.default_rng(rate + len(fmt))
    out = []
    for edge in (1024, 512):
        n = [0, 1, K // 2, _n_below(edge, U, D), _n_above(edge, U, D), N_cap]
        buf = np.full((len(n), N_cap), SRC_FILL[fmt], dtype=I.NP_DTYPE[fmt])
        for b, nb in enumerate(n):
            buf[b, :nb] = I.encode(np.clip(0.4 * rng.standard_normal(nb), -1, 1), fmt)
        rows = [I.ingest_row(buf[b], n[b], fmt, taps, U, D, 0.0, 0, L_cap) for b in range(len(n))]
        out.append((buf, n, rows))
    return out, L_cap


def _ingest(buf, n, rate, fmt, top_db, L_min=0, L_cap=None):
    """-> (wave on the host with its sentinel, len, start, flags)"""
    U, D, K, _ = resample.input_table(rate, DEV)
    cap = resample.output_samples(buf.shape[1], U, D) if L_cap is None else L_cap
    room = torch.full((buf.shape[0], (cap + 3) // 4 * 4 + 8), SENTINEL, device=DEV)
    src = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    wave, ln, st, fl = ops.clip_ingest(src, torch.tensor(n, dtype=torch.int32, device=DEV), rate, fmt, top_db=top_db,
                                       L_cap=cap, L_min=L_min, out=room)
    torch.cuda.synchronize()
    assert wave.data_ptr() == room.data_ptr()
    return room.cpu().numpy(), ln.cpu().tolist(), st.cpu().tolist(), fl.cpu().tolist()


def _check_rows(got, ln, st, fl, rows, what):
    assert ln == [r["len"] for r in rows], (what, ln, [r["len"] for r in rows])
    assert st == [r["start"] for r in rows], (what, st)
    assert fl == [r["flags"] for r in rows], (what, fl)
    for b, r in enumerate(rows):
        assert (got[b, r["len"]:] == np.float32(SENTINEL)).all(), "%s row %d: written at or past len" % (what, b)
        err = np.abs(got[b, :r["len"]].astype(np.float64) - r["wave"])
        assert (err <= r["bound"]).all(), "%s row %d: %d samples beyond the fp32 bound, worst %g x" % (
            what, b, (err > r["bound"]).sum(), (err / np.maximum(r["bound"], 1e-300)).max())


# ---- resample and decode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt", CASES)
def test_every_rate_and_format_within_the_derived_bound(rate, fmt):
    batches, L_cap = _edge_batches(rate, fmt)
    for buf, n, rows in batches:
        assert [r["len"] for r in rows][:2] == [0, resample.output_samples(1, *resample.design_input(rate)[:2])]
        got, ln, st, fl = _ingest(buf, n, rate, fmt, 0.0)
        assert np.isfinite(got).all(), "a NaN from at or past n_b reached a sum"
        _check_rows(got, ln, st, fl, rows, "rate %d %s" % (rate, fmt))
        assert st == [0] * len(n) and fl == [0] * len(n)


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_24000_is_the_decode_alone_exact_for_all_256_codes(law):
    codes = np.arange(256, dtype=np.uint8)
    buf = np.stack([codes, codes[::-1]])
    got, ln, st, fl = _ingest(buf, [256, 200], 24000, law, 0.0)
    assert ln == [256, 200] and fl == [0, 0]
    want = I.decode(buf, law)
    assert np.array_equal(got[0, :256], want[0]) and np.array_equal(got[1, :200], want[1][:200])
    assert (got[1, 200:] == np.float32(SENTINEL)).all()


def test_a_table_that_leaves_room_for_a_512_sample_tile_only():
    """U = 160, K = 90: beside 57 600 bytes of table a 1024-sample tile no longer fits the kernel's 63 KiB, a 512-sample one
    does -- the kernel's other tile size, which no supported rate reaches.  Straight through the C entry point."""
    U, D, K = 160, 147, 90
    rng = np.random.default_rng(7)
    taps = (rng.standard_normal((U, K)) / K).astype(np.float32)
    n = [1300, 471, 0]
    N_cap = 1300
    L_cap = resample.output_samples(N_cap, U, D)
    x = (0.5 * rng.standard_normal((3, N_cap))).astype(np.float32)
    for b, nb in enumerate(n):
        x[b, nb:] = np.nan
    rows = [I.ingest_row(x[b], n[b], "f32", taps, U, D, 0.0, 0, L_cap) for b in range(3)]
    lib = _lib.load()
    w_bs = (L_cap + 3) // 4 * 4
    room = torch.full((3, w_bs), SENTINEL, device=DEV)
    src, td = torch.from_numpy(x).to(DEV), torch.from_numpy(taps).to(DEV)
    nd = torch.tensor(n, dtype=torch.int32, device=DEV)
    ln, st, fl = (torch.empty(3, dtype=torch.int32, device=DEV) for _ in range(3))
    nbytes = lib.st2_clip_ingest_work_bytes(3, L_cap)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.st2_clip_ingest(src.data_ptr(), N_cap, nd.data_ptr(), 3, N_cap, _lib.PCM_F32, U, D, td.data_ptr(), K, 0.0, 0,
                                   room.data_ptr(), w_bs, L_cap, ln.data_ptr(), st.data_ptr(), fl.data_ptr(), work.data_ptr(),
                                   nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "st2_clip_ingest")
    torch.cuda.synchronize()
    _check_rows(room.cpu().numpy(), ln.cpu().tolist(), st.cpu().tolist(), fl.cpu().tolist(), rows, "512-sample tiles")


@pytest.mark.parametrize("U,D", [(3, 2), (147, 160)])
def test_one_table_through_the_way_in_and_the_way_out_gives_the_same_bits(U, D):
    """`st2_clip_ingest` (not cut: top_db = 0, L_min = 0) and `st2_wave_resample_pack` (F32, trim = 0) on the same fp32 rows,
    ratio and table: both are section 15's chain -- fmaf from 0, k ascending, selected zeros outside the row -- so every valid
    sample agrees bitwise, whatever the tiles: 1024 samples from the row's start on the way in, from the 16-byte grid of a
    destination one float off it on the way out.  Straight through the C entry points."""
    K, SPF, T_CAP, frames = 16, 600, 5, [5, 3, 1]
    rng = np.random.default_rng(U)
    taps = (rng.standard_normal((U, K)) / K).astype(np.float32)
    n = [SPF * f for f in frames]
    N_cap = SPF * T_CAP
    x = (0.5 * rng.standard_normal((3, N_cap))).astype(np.float32)
    for b, nb in enumerate(n):
        x[b, nb:] = np.nan
    m = [resample.output_samples(nb, U, D) for nb in n]
    L_cap = m[0]
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src, td = torch.from_numpy(x).to(DEV), torch.from_numpy(taps).to(DEV)
    # the way in
    w_bs = (L_cap + 3) // 4 * 4
    room = torch.full((3, w_bs), SENTINEL, device=DEV)
    nd = torch.tensor(n, dtype=torch.int32, device=DEV)
    ln, st, fl = (torch.empty(3, dtype=torch.int32, device=DEV) for _ in range(3))
    nbytes = lib.st2_clip_ingest_work_bytes(3, L_cap)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.st2_clip_ingest(src.data_ptr(), N_cap, nd.data_ptr(), 3, N_cap, _lib.PCM_F32, U, D, td.data_ptr(), K, 0.0, 0,
                                   room.data_ptr(), w_bs, L_cap, ln.data_ptr(), st.data_ptr(), fl.data_ptr(), work.data_ptr(),
                                   nbytes, stream), "st2_clip_ingest")
    # the way out
    packed = torch.full((1 + sum(m) + 8,), SENTINEL, device=DEV)
    out = packed[1:]
    assert out.data_ptr() % 16 == 4, "row 0 starts off the 16-byte grid: its tiles are not those of the way in"
    fd = torch.tensor(frames, dtype=torch.int32, device=DEV)
    offs = torch.empty(4, dtype=torch.int64, device=DEV)
    _lib.check(lib.st2_wave_resample_pack(src.data_ptr(), N_cap, fd.data_ptr(), 3, T_CAP, SPF, 0, U, D, td.data_ptr(), K,
                                          _lib.PCM_F32, out.data_ptr(), out.numel(), offs.data_ptr(), stream),
               "st2_wave_resample_pack")
    torch.cuda.synchronize()
    o = offs.cpu().tolist()
    assert ln.cpu().tolist() == m and st.cpu().tolist() == [0, 0, 0] and fl.cpu().tolist() == [0, 0, 0]
    assert o == [0, m[0], m[0] + m[1], sum(m)] and m[0] > 2 * 1024 and m[2] < 1024, "rows of several tiles and of one"
    way_in, way_out = room.cpu().numpy(), out.cpu().numpy()
    assert np.isfinite(way_out[:o[3]]).all() and (way_out[o[3]:] == np.float32(SENTINEL)).all()
    for b in range(3):
        assert np.array_equal(way_in[b, :m[b]].view(np.int32), way_out[o[b]:o[b + 1]].view(np.int32)), "row %d" % b
        assert (way_in[b, m[b]:] == np.float32(SENTINEL)).all()


# ---- trim, minimum length, capacity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt", I.TRIM_RATES)
def test_trim_bounds_are_exact_and_the_samples_hold_the_bound(rate, fmt):
    names, rows, L_cap = I.reference("trim", rate, fmt, 0)
    buf, n = I.stack(I.trim_cases(rate, fmt)[1], fmt, SRC_FILL[fmt])
    got, ln, st, fl = _ingest(buf, n, rate, fmt, I.TOP_DB, L_cap=L_cap)
    _check_rows(got, ln, st, fl, rows, "trim %d %s" % (rate, fmt))


@pytest.mark.parametrize("rate,fmt", I.TRIM_RATES)
def test_minimum_length_rule_and_its_flag(rate, fmt):
    names, rows, L_cap = I.reference("short", rate, fmt, I.L_MIN)
    buf, n = I.stack(I.short_cases(rate, fmt)[1], fmt, SRC_FILL[fmt])
    got, ln, st, fl = _ingest(buf, n, rate, fmt, I.TOP_DB, L_min=I.L_MIN, L_cap=L_cap)
    assert fl == [2, 2, 2, 2] and ln[:3] == [I.L_MIN] * 3 and ln[3] < I.L_MIN
    _check_rows(got, ln, st, fl, rows, "minimum length %d %s" % (rate, fmt))


def test_a_row_beyond_capacity_is_cut_and_flagged_and_leaves_the_others_alone():
    rate, fmt = 16000, "s16"
    buf, n, _ = _edge_batches(rate, fmt)[0][0]
    U, D, taps = resample.design_input(rate)
    L_cap = 2000  # row 5 (3000 samples at capacity) does not fit; the others (<= 1026) do
    rows = [I.ingest_row(buf[b], n[b], fmt, taps, U, D, 0.0, 0, L_cap) for b in range(len(n))]
    assert [r["flags"] for r in rows] == [0, 0, 0, 0, 0, 1] and rows[5]["len"] == L_cap
    got, ln, st, fl = _ingest(buf, n, rate, fmt, 0.0, L_cap=L_cap)
    _check_rows(got, ln, st, fl, rows, "capacity")
    without, ln5, _, fl5 = _ingest(buf[:5], n[:5], rate, fmt, 0.0, L_cap=L_cap)
    assert ln5 == ln[:5] and fl5 == [0] * 5
    assert np.array_equal(got[:5].view(np.int32), without.view(np.int32)), "rows 0-4 bitwise as in a batch without row 5"


# ---- independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt", [(8000, "ulaw"), (44100, "s16")])
def test_a_row_alone_in_the_batch_and_in_the_batch_permuted_bitwise(rate, fmt):
    if (rate, fmt) in I.TRIM_RATES:
        buf, n = I.stack(I.trim_cases(rate, fmt)[1], fmt, SRC_FILL[fmt])
        top_db = I.TOP_DB
    else:
        (buf, n, _), top_db = _edge_batches(rate, fmt)[0][0], 0.0
    a = _ingest(buf, n, rate, fmt, top_db)
    again = _ingest(buf, n, rate, fmt, top_db)
    assert np.array_equal(a[0].view(np.int32), again[0].view(np.int32)) and a[1:] == again[1:], "two calls agree bitwise"
    perm = [3, 5, 0, 4, 1, 2]
    p = _ingest(buf[perm], [n[i] for i in perm], rate, fmt, top_db)
    for at, b in enumerate(perm):
        assert (p[1][at], p[2][at], p[3][at]) == (a[1][b], a[2][b], a[3][b])
        assert np.array_equal(p[0][at, :a[1][b]].view(np.int32), a[0][b, :a[1][b]].view(np.int32)), "row %d permuted" % b
        solo = _ingest(buf[b:b + 1], [n[b]], rate, fmt, top_db)
        assert (solo[1][0], solo[2][0], solo[3][0]) == (a[1][b], a[2][b], a[3][b])
        assert np.array_equal(solo[0][0, :a[1][b]].view(np.int32), a[0][b, :a[1][b]].view(np.int32)), "row %d alone" % b


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def libritts_style():
    man = manifest("libritts")
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    synth.init_spectral_norm_(model.style_encoder, 3)
    synth.init_spectral_norm_(model.predictor_encoder, 4)
    model.style_encoder.to(DEV)
    model.predictor_encoder.to(DEV)
    return model


@functools.lru_cache(maxsize=None)
def _telephony_clips(seed):
    """Three 8 kHz mu-law clips: ~0.25 s of low-level noise, a burst of ~1.25 s, noise again; the burst edges sit 256 samples (at
    24 kHz) inside a frame.  -> (clips, rows of the fp64 reference at L_min = MIN_CLIP)"""
    U, D, taps = resample.design_input(8000)
    clips = []
    for i, (lead, dur, tail) in enumerate([(5888, 30208, 6000), (2816, 31744, 3500), (7936, 29696, 4321)]):
        m = lead + dur + tail
        clips.append(I._to_rate(I._clip24(m, [(lead, lead + dur)], seed + i), U, D, "ulaw"))
    L_cap = max(resample.output_samples(max(len(c) for c in clips), U, D), style.MIN_CLIP)
    rows = [I.ingest_row(c, len(c), "ulaw", taps, U, D, style.TRIM_TOP_DB, style.MIN_CLIP, L_cap) for c in clips]
    assert all(r["margin"] >= 2.0 and r["flags"] == 0 and r["len"] >= style.MIN_CLIP for r in rows)
    return clips, rows


def test_compute_style_from_8_khz_mu_law(libritts_style):
    model = libritts_style
    clips, rows = _telephony_clips(40)
    dev_clips = [torch.from_numpy(c).to(DEV) for c in clips]
    ref_s = style.compute_style(model, dev_clips, sample_rate=8000, encoding="ulaw")
    wave24, n24, flags = style.ingest_clips(dev_clips, sample_rate=8000, encoding="ulaw")
    torch.cuda.synchronize()
    ops.check_status()
    assert n24.cpu().tolist() == [r["len"] for r in rows] and flags.cpu().tolist() == [0, 0, 0]
    assert torch.equal(ref_s, style.compute_style(model, wave24, lengths=n24)), "the ingest, then today's call: the same bits"
    # today's compute_style on the fp64 reference's clips (rounded to fp32), and on a copy perturbed by the resampler's bound
    g = np.random.default_rng(9)
    exact = [torch.from_numpy(r["wave"].astype(np.float32)).to(DEV) for r in rows]
    nudged = [torch.from_numpy((r["wave"] + r["bound"] * g.choice([-1.0, 1.0], size=r["len"])).astype(np.float32)).to(DEV)
              for r in rows]
    s_exact, s_nudged = style.compute_style(model, exact), style.compute_style(model, nudged)
    spread = (s_nudged - s_exact).abs().max().item()
    diff = (ref_s - s_exact).abs().max().item()
    print("ref_s: ingest path vs fp64-reference clips %.3e; the same call on clips perturbed by the bound %.3e" % (diff, spread))
    assert diff <= max(1e-4, 2.0 * spread), (diff, spread)


def test_ingest_and_compute_style_in_one_graph(libritts_style):
    model = libritts_style
    first, _ = _telephony_clips(40)
    other, _ = _telephony_clips(50)
    N_cap = max(len(c) for c in first + other)
    buf = torch.zeros((3, N_cap), dtype=torch.uint8, device=DEV)
    n = torch.zeros(3, dtype=torch.int32, device=DEV)

    def load(clips, rot):
        host, cnt = I.stack([clips[(b + rot) % 3] for b in range(3)], "ulaw", 0x55)
        buf.zero_()
        buf[:, :host.shape[1]] = torch.from_numpy(host).to(DEV)
        n.copy_(torch.tensor(cnt, dtype=torch.int32))

    run = lambda: style.compute_style(model, buf, lengths=n, sample_rate=8000, encoding="ulaw")
    load(first, 0)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run()  # warm-up: the table uploaded, engines packed, mel weights cached
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        out = run()
        with pytest.raises(RuntimeError, match="before a stream capture"):
            resample.input_table(32000, DEV)  # no other test has made this one
    for clips, rot in ((other, 0), (first, 1)):
        load(clips, rot)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        assert torch.equal(replayed, run()), "a replay is bitwise the eager call on the same bytes and lengths"
    ops.check_status()
