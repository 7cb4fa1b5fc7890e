"""The loudness-normalised hand-over on the device: `st2_wave_level` against the fp64 contract of
tests/_level_ref.py on the rows of tests/_level_cases.py, `st2_wave_pack_level` against the existing packing contracts applied to
fl32(x * g_b) with the DEVICE's reported gain, and one graph from tokens to normalised 8 kHz mu-law.

Block count and peak are exact.  L_b is held to `_level_cases.loudness_bound_db` (the W-sample warm-up, fp64 rounding, one
rounding to fp32: about 2e-6 dB), g_b to one fp32 ulp.  Geometry: 24 kHz, rows of 72 000 samples (600 x 120 frames), B = 8, a
row stride larger than the row, NaN bit patterns behind every row's n_b.  The issue's sample counts 5 000 and 11 999 are no
multiple of 600 samples minus a trim of 0 or 50: they are met exactly at one sample per frame, and at 600 samples per frame by
the nearest count above them (`_level_cases.frames_of`); both geometries run."""
import functools

import numpy as np
import pytest
import torch

import _level_cases as Cs
import _level_ref as R
import _passage_ref as PR
import _resample_ref as RR
import _syncfree_ref as SR
from styletts2_amd import ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIDE = Cs.ROW + 608  # w_bs larger than the row
TORCH_DT = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


def _batch(names, spf, trim):
    """-> (wave [B, ROW] device view of stride STRIDE with NaN behind every n_b, frames, targets, host copy of the wave)."""
    B = len(names)
    host = np.full((B, STRIDE), np.nan, dtype=np.float32)
    frames = [Cs.frames_of(n, spf, trim) for n in names]
    for b, name in enumerate(names):
        n_b = Cs.expect(name, spf, trim)[1]["n"]
        host[b, :n_b] = Cs.content()[name][0][:n_b]
    wave = torch.from_numpy(host).to(DEV)[:, :Cs.ROW]
    target = torch.tensor([Cs.ROWS[n][1] for n in names], dtype=torch.float32, device=DEV)
    return wave, torch.tensor(frames, dtype=torch.int32, device=DEV), target, host[:, :Cs.ROW]


def _level(names, spf, trim):
    wave, frames, target, _ = _batch(names, spf, trim)
    lv = ops.wave_level(wave, frames, target, ceiling=Cs.CEILING, max_gain_db=Cs.MAX_GAIN_DB, trim=trim, samples_per_frame=spf,
                        sample_rate=Cs.FS)
    torch.cuda.synchronize()
    assert lv.dtype == torch.float32 and tuple(lv.shape) == (len(names), 4)
    return lv.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _main(spf, trim):
    got = _level(Cs.MAIN, spf, trim)
    got.setflags(write=False)
    return got


def _check_rows(got, names, spf, trim):
    for b, name in enumerate(names):
        want, d = Cs.expect(name, spf, trim)
        assert Cs.gate_distance(name, spf, trim) >= Cs.GUARD_LU, (name, spf, trim)
        bound = Cs.loudness_bound_db(name, spf, trim)
        ulp = float(np.spacing(want[2]))
        print("spf %d trim %d row %-10s n %5d: L %.7f (contract %.9f, |diff| %.2e, bound %.2e) peak %.8g gain %.8g (contract %.8g) "
              "blocks %d" % (spf, trim, name, d["n"], got[b, 0], d["L"], abs(float(got[b, 0]) - d["L"]) if d["passed"].any() else 0.0,
                             bound, got[b, 1], got[b, 2], want[2], got[b, 3]))
        assert got[b, 3] == want[3], (name, got[b], want)
        assert got[b, 1].tobytes() == want[1].tobytes(), (name, got[b], want)
        if d["passed"].any():
            assert abs(float(got[b, 0]) - d["L"]) <= bound, (name, got[b, 0], d["L"], bound)
        else:
            assert got[b, 0] == -np.inf and got[b, 2].tobytes() == np.float32(1.0).tobytes(), (name, got[b])
        assert abs(float(got[b, 2]) - float(want[2])) <= ulp, (name, got[b, 2], want[2])
        if np.isnan(Cs.ROWS[name][1]) or d["peak"] == 0.0:
            assert got[b, 2].tobytes() == np.float32(1.0).tobytes(), (name, got[b])


@pytest.mark.parametrize("spf,trim", Cs.GEOMETRIES)
def test_level_table_equals_the_contract(spf, trim):
    got = _main(spf, trim)
    _check_rows(got, Cs.MAIN, spf, trim)
    if spf == 1:  # the issue's sample counts, exactly
        assert [Cs.expect(n, spf, trim)[1]["n"] for n in ("a", "b", "c", "d")] == [0, 5000, 9600, 11999]
    assert got[0].tolist() == [-np.inf, 0.0, 1.0, 0.0] and got[7].tolist() == [-np.inf, 0.0, 1.0, 0.0]  # no samples; all zero
    assert got[1, 3] == got[2, 3] == 1 and Cs.expect("b", spf, trim)[1]["n"] < 4 * Cs.H  # the short-row rule
    f, g = Cs.expect("f", spf, trim)[1], Cs.expect("g", spf, trim)[1]
    assert (f["l"][:7] == -np.inf).all() and not f["passed"][:7].any(), "the absolute gate drops the silence"
    assert (g["l"] > R.ABS_GATE).all() and 0 < g["passed"].sum() < len(g["z"]), "the relative gate drops the quiet half"
    assert ops.status() == 0


@pytest.mark.parametrize("spf,trim", [(1, 0), (600, 50)])
def test_variants_and_a_row_does_not_depend_on_its_place(spf, trim):
    got = _level(Cs.OTHER, spf, trim)
    _check_rows(got, Cs.OTHER, spf, trim)
    names = list(Cs.OTHER)
    imp = Cs.expect("impulse", spf, trim)
    assert imp[0][1] == 1.0 and imp[0][2] == np.float32(Cs.CEILING / 1.0), "the ceiling wins, not the target or the limit"
    assert got[names.index("impulse"), 2].tobytes() == np.float32(Cs.CEILING).tobytes()
    assert got[names.index("nan_target"), 2] == 1.0 and np.isfinite(got[names.index("nan_target"), 0])
    assert np.isfinite(got[names.index("nan_sample")]).all(), "a NaN sample counts as 0"
    main = _main(spf, trim)
    for name in set(Cs.OTHER) & set(Cs.MAIN):  # the same row at another place in another batch: bitwise
        assert got[names.index(name)].tobytes() == main[Cs.MAIN.index(name)].tobytes(), name
    for name in ("d", "g"):  # and alone
        alone = _level((name,), spf, trim)
        assert alone[0].tobytes() == main[Cs.MAIN.index(name)].tobytes(), name


# ---- the gain in the packing moves -----------------------------------------------------------------------------------------------
def _equal_bits(got, want, what):
    """Byte for byte; where an fp32 reference sample is NaN (NaN x g: IEEE 754 leaves the payload open) the device's is NaN too."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("spf,trim", [(600, 0), (600, 50), (1, 50)])
@pytest.mark.parametrize("names", [Cs.MAIN, Cs.OTHER], ids=["main", "variants"])
def test_plain_move_with_gain_is_the_plain_contract_of_the_scaled_input(names, spf, trim):
    wave, frames, target, host = _batch(names, spf, trim)
    B, T_cap = len(names), Cs.ROW // spf
    lv = ops.wave_level(wave, frames, target, ceiling=Cs.CEILING, max_gain_db=Cs.MAX_GAIN_DB, trim=trim, samples_per_frame=spf)
    gains = lv[:, 2].cpu().numpy()
    assert len(set(gains.tolist())) > 3
    scaled = R.apply_gain(host, frames.cpu().tolist(), T_cap, spf, trim, gains)
    gaps = [(37 * b) % 11 - 2 for b in range(B)]
    gd = torch.tensor(gaps, dtype=torch.int32, device=DEV)
    for fmt in ("f32", "s16"):
        want, woff = SR.wave_pack(scaled, frames.cpu().tolist(), T_cap, spf, trim, fmt)
        total = int(woff[-1])
        out = torch.full((total + 64 + 9 * B,), 77, dtype=TORCH_DT[fmt], device=DEV)
        packed, offs = ops.wave_pack_level(wave, frames, lv, fmt=fmt, trim=trim, out=out[1:], samples_per_frame=spf)  # a head to peel
        assert offs.cpu().tolist() == woff.tolist()
        _equal_bits(packed[:total].cpu().numpy(), want, (fmt, "no gaps"))
        assert (out[1 + total:] == 77).all() and out[0] == 77, "written outside [0, offsets[B])"
        rows = [want[woff[b]:woff[b + 1]] for b in range(B)]
        want_g, woff_g, limit = PR.pack_gaps(rows, gaps, 8, fmt)
        packed, offs = ops.wave_pack_level(wave, frames, lv, gaps=gd, max_gap=8, fmt=fmt, trim=trim, out=out[1:], samples_per_frame=spf)
        assert offs.cpu().tolist() == woff_g.tolist()
        _equal_bits(packed[:limit].cpu().numpy(), want_g, (fmt, "gaps"))
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("rate,fmt", [(8000, "ulaw"), (16000, "s16")])
def test_resampling_move_with_gain_stays_within_the_derived_bounds(rate, fmt):
    spf, trim, names = 600, 50, Cs.MAIN
    wave, frames, target, host = _batch(names, spf, trim)
    B, T_cap = len(names), Cs.ROW // spf
    lv = ops.wave_level(wave, frames, target, ceiling=Cs.CEILING, max_gain_db=Cs.MAX_GAIN_DB, trim=trim, samples_per_frame=spf)
    scaled = R.apply_gain(host, frames.cpu().tolist(), T_cap, spf, trim, lv[:, 2].cpu().numpy())
    U, D, taps = resample.design(rate)
    y, bound, woff = RR.wave_resample(scaled, frames.cpu().tolist(), T_cap, taps, U, D, spf, trim)
    gaps = [5, 0, 3, 9, 1, 0, 7, 2]
    packed, offs = ops.wave_pack_level(wave, frames, lv, gaps=torch.tensor(gaps, dtype=torch.int32, device=DEV), max_gap=6, rate=rate,
                                       fmt=fmt, trim=trim, samples_per_frame=spf)
    m = np.diff(woff)
    want_off = PR.offsets(m, gaps, 6)
    assert offs.cpu().tolist() == want_off.tolist()
    got, z = packed.cpu().numpy(), PR.silence(fmt)
    for b in range(B):
        speech = got[want_off[b]:want_off[b] + m[b]]
        lo, hi = RR.pcm_interval(y[woff[b]:woff[b + 1]], bound[woff[b]:woff[b + 1]])
        if fmt == "s16":
            bad = (speech < lo) | (speech > hi)
        else:  # the byte is the code of some int16 in [lo, hi]: encoding is monotone
            r = RR.rank(speech, fmt)
            bad = (r < RR.rank(RR.ENCODE[fmt](lo), fmt)) | (r > RR.rank(RR.ENCODE[fmt](hi), fmt))
        assert not bad.any(), "row %d: %d samples outside their interval" % (b, bad.sum())
        gap = got[want_off[b] + m[b]:want_off[b + 1]]
        assert len(gap) == min(gaps[b], 6) and (gap == z).all(), "the gaps stay the format's silence code"
    # the gain is in it: row e alone without gain is some 11 dB quieter
    plain, _ = ops.wave_pack_level(wave, frames, None, rate=rate, fmt=fmt, trim=trim, samples_per_frame=spf)
    assert not torch.equal(plain[:int(woff[-1])], packed[:int(woff[-1])])
    assert ops.status() == 0


def test_without_a_level_all_four_entries_write_the_bytes_they_always_wrote():
    """NaN payloads of the fp32 bit copy included: the multiply is skipped, not done by 1.0f."""
    spf, T_cap, trim, B = 5, 8, 3, 6
    g = np.random.default_rng(9)
    frames = [8, 0, 3, 10, 1, 7]
    host = (g.standard_normal((B, spf * T_cap)) * 0.6).astype(np.float32)
    bits = host.view(np.uint32)
    bits[0, 3], bits[0, 17], bits[2, 1] = 0x7FA12345, 0xFFC00001, 0x7F800001  # signalling and quiet NaNs with payloads, inside rows
    for b, f in enumerate(frames):
        host[b, spf * min(f, T_cap):] = np.nan
    wave, fd = torch.from_numpy(host).to(DEV), torch.tensor(frames, dtype=torch.int32, device=DEV)
    gaps = [2, 0, 9, 1, 0, 4]
    gd = torch.tensor(gaps, dtype=torch.int32, device=DEV)
    for fmt in ("f32", "s16"):
        with np.errstate(invalid="ignore"):  # the signalling NaNs of row 0 and 2 in the reference's own arithmetic
            want, woff = SR.wave_pack(host, frames, T_cap, spf, trim, fmt)
        total = int(woff[-1])
        rows = [want[woff[b]:woff[b + 1]] for b in range(B)]
        want_g, woff_g, limit = PR.pack_gaps(rows, gaps, 5, fmt)
        for packed, offs in (ops.wave_pack(wave, fd, trim=trim, fmt=fmt, samples_per_frame=spf),
                             ops.wave_pack_gaps(wave, fd, None, 0, fmt=fmt, trim=trim, samples_per_frame=spf),
                             ops.wave_pack_level(wave, fd, None, fmt=fmt, trim=trim, samples_per_frame=spf)):
            assert offs.cpu().tolist() == woff.tolist() and packed[:total].cpu().numpy().tobytes() == want.tobytes(), fmt
        for packed, offs in (ops.wave_pack_gaps(wave, fd, gd, 5, fmt=fmt, trim=trim, samples_per_frame=spf),
                             ops.wave_pack_level(wave, fd, None, gaps=gd, max_gap=5, fmt=fmt, trim=trim, samples_per_frame=spf)):
            assert offs.cpu().tolist() == woff_g.tolist() and packed[:limit].cpu().numpy().tobytes() == want_g.tobytes(), fmt
    for rate, fmt in ((8000, "ulaw"), (44100, "f32")):  # the resampling move: the new entry without a level IS the old ones, bitwise
        old, ooff = ops.wave_resample_pack(wave, fd, rate, fmt=fmt, trim=trim, samples_per_frame=spf)
        new, noff = ops.wave_pack_level(wave, fd, None, rate=rate, fmt=fmt, trim=trim, samples_per_frame=spf)
        total = int(ooff[-1])
        assert torch.equal(ooff, noff) and old[:total].cpu().numpy().tobytes() == new[:total].cpu().numpy().tobytes()
        U, D, taps = resample.design(rate)
        y, bound, woff = RR.wave_resample(np.nan_to_num(host), frames, T_cap, taps, U, D, spf, trim)
        assert ooff.cpu().tolist() == woff.tolist()
        oldg, ooffg = ops.wave_pack_gaps(wave, fd, gd, 5, rate=rate, fmt=fmt, trim=trim, samples_per_frame=spf)
        newg, noffg = ops.wave_pack_level(wave, fd, None, gaps=gd, max_gap=5, rate=rate, fmt=fmt, trim=trim, samples_per_frame=spf)
        total = int(ooffg[-1])
        assert torch.equal(ooffg, noffg) and oldg[:total].cpu().numpy().tobytes() == newg[:total].cpu().numpy().tobytes()
    torch.cuda.synchronize()
    assert ops.status() == 0


# ---- one graph from tokens to normalised telephony bytes ------------------------------------------------------------------------
def test_one_graph_serves_any_targets_and_the_marks_do_not_move(monkeypatch):
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    T, N = P["T"], b["tokens"].shape[1]
    out = dict(pack="ulaw", sample_rate=8000, marks=True)
    ld = b["lengths"].to(torch.int32).to(DEV)
    feed = dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"])
    build = dict(ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, **out)
    plain = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, **build)
    rows0, marks0 = plain(**feed).to_host(marks=True)
    rows0, marks0 = [r.copy() for r in rows0], marks0.copy()
    assert "level" not in plain.static
    with pytest.raises(ValueError, match="built without level"):
        plain(level=-16.0)
    with pytest.raises(ValueError, match="pack"):
        pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, level=True)
    # a ceiling and a limit that leave the target in charge
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, T, STEPS, level=pipeline.Level(K, target=None, ceiling_db=0.0, max_gain_db=60.0),
                                   **build)
    assert gs.static["level"].target.isnan().all() and gs.static["level"].ceiling == 1.0
    res = gs(**feed)  # every row left alone: the measurement only, and the plain graph's bytes
    graph = gs._g["graph"]
    copies = []
    real = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a, **kw: (copies.append(self.is_pinned()), real(self, src, *a, **kw))[1])
    rows_n, marks_n, lv_n = res.to_host(marks=True, level=True)
    monkeypatch.undo()
    assert copies == [True], "to_host(level=True) is one copy, into the pinned mirror"
    assert lv_n.shape == (K, 4) and lv_n.dtype == np.float32 and np.array_equal(lv_n, res.level.cpu().numpy())
    assert (lv_n[:, 2] == 1.0).all() and all(np.array_equal(x, y) for x, y in zip(rows_n, rows0)) and np.array_equal(marks_n, marks0)
    lv_n = lv_n.copy()
    assert np.isfinite(lv_n[:, 0]).all() and (lv_n[:, 1] > 0).all() and (lv_n[:, 3] >= 1).all(), lv_n
    # two sets of targets 7 dB apart, picked where the contract says neither the ceiling nor the limit binds: below L_b + the
    # row's headroom min(60 dB, -20 log10 peak_b), and inside Level's range
    room = lv_n[:, 0].astype(np.float64) + np.minimum(60.0, -20.0 * np.log10(lv_n[:, 1].astype(np.float64)))
    hi = np.clip(np.floor(room) - 1.0, -63.0, 0.0)
    assert (hi < room).all(), "the seeded model's rows leave no target in Level's range that is not ceiling-bound: %s" % lv_n
    seen = []
    for tg in (hi, hi - 7.0):
        res = gs(level=tg.tolist())
        assert gs._g["graph"] is graph, "no re-record"
        rows, marks, lv = res.to_host(marks=True, level=True)
        assert np.array_equal(marks, marks0), "the marks equal those of the run without level"
        assert [len(r) for r in rows] == [len(r) for r in rows0]
        assert np.array_equal(lv[:, [0, 1, 3]], lv_n[:, [0, 1, 3]]), "the measurement does not depend on the target"
        for k in range(K):
            want = 10.0 ** ((float(np.float32(tg[k])) - float(lv[k, 0])) / 20.0)
            assert want < min(1000.0, 1.0 / float(lv[k, 1]))
            # the device holds L_b in fp64; its fp32 report moves 10^(-L / 20) by at most |L| 2^-24 ln(10) / 20
            assert abs(float(lv[k, 2]) - want) <= want * (2.0 ** -23 + abs(float(lv[k, 0])) * 2.0 ** -24 * 0.1152), (k, lv[k], want)
        seen.append(([r.copy() for r in rows], lv.copy()))
    for k in range(K):
        step = 20.0 * np.log10(float(seen[0][1][k, 2]) / float(seen[1][1][k, 2]))
        print("row %d: L %.4f LUFS, peak %.4g, gains %.6g / %.6g: %.7f dB apart" % (k, lv_n[k, 0], lv_n[k, 1], seen[0][1][k, 2],
                                                                                     seen[1][1][k, 2], step))
        assert abs(step - 7.0) <= 2 * 20.0 * np.log10(1.0 + 2.0 ** -24), "the same fp64 L_b, two roundings of g to fp32"
        assert not np.array_equal(seen[0][0][k], seen[1][0][k])
    # a row left alone is the plain graph's row, byte for byte, beside rows that are not
    mixed = [None, float(hi[1]), float("nan"), float(hi[3])]
    rows_c, lv_c = gs(level=mixed).to_host(level=True)
    assert lv_c[0, 2] == 1.0 and lv_c[2, 2] == 1.0 and np.array_equal(rows_c[0], rows0[0]) and np.array_equal(rows_c[2], rows0[2])
    assert np.array_equal(rows_c[1], seen[0][0][1]) and np.array_equal(rows_c[3], seen[0][0][3])
    torch.cuda.synchronize()
    ops.check_status()
