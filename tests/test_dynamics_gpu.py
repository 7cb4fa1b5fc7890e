"""The compressor of the hand-over on the device: `st2_wave_dynamics` against the numpy contract of
tests/_dynamics_ref.py -- the block sums and, over the device's own gains per block, every output sample bit for bit; the gains
per block and the deepest reduction to one fp32 ulp, which is the last ulp of fp64 log10 / pow; the count of reduced blocks
exact but for the blocks the reference names as sitting within rounding of 0 -- then `dynamics=` through the pipeline.  Shapes
are the smallest at which the kernels can still go wrong: row lengths around one block, three blocks (the detector), one tile of
the sums' launch, one tile of the apply launch and one chunk of the per-row launch; every signal under every setting."""
import numpy as np
import pytest
import torch

import _dynamics_ref as R
from styletts2_amd import _lib, ops, pipeline, resample

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = np.float32(-7.25)
TILE, CHUNK = ops.DYNAMICS_TILE, ops.DYNAMICS_CHUNK
COUNTS = [0, 1, 63, 64, 65, 191, 192, 193, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, 64 * CHUNK - 1, 64 * CHUNK, 64 * CHUNK + 1]
SIGNALS = ("silence", "burst", "ramp", "noise", "nonfinite")
INF = float("inf")
# {threshold_db, slope, knee_db, makeup_db}: the defaults; a row left alone; ratio 1 with a make-up gain; ratio inf; a hard knee;
# values the kernels clamp (slope 1.5 -> 1, knee 90 -> 40, makeup -30 -> -24); a threshold nothing reaches
SETTINGS = [(-24.0, 2.0 / 3.0, 6.0, 0.0), (float("nan"), 0.5, 6.0, 0.0), (-30.0, 0.0, 6.0, 3.0), (-35.0, 1.0, 10.0, 0.0),
            (-28.0, 0.75, 0.0, 2.0), (-40.0, 1.5, 90.0, -30.0), (0.0, 0.5, 0.0, 0.0)]
RHO = 80.0 * 64 / 24000


def signal(kind, n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal(n).astype(np.float32)
    if kind == "silence":
        return np.zeros(n, dtype=np.float32)
    if kind == "burst":  # loud, then 50 dB down: the release shows
        return (x * np.where(np.arange(n) < max(n // 3, 1), 0.4, 0.0012)).astype(np.float32)
    if kind == "ramp":  # -60 .. -6 dBFS: across every threshold and knee of SETTINGS
        return (x * 10.0 ** (np.linspace(-60.0, -6.0, n) / 20.0)).astype(np.float32)
    x = (x * 0.1).astype(np.float32)
    if kind == "nonfinite" and n:
        x[0] = np.nan
        if n >= 3:
            x[n // 2], x[n - 1] = np.inf, -np.inf
        if n > 300:
            x[200:210] = 3.0e19  # squares that overflow a block sum to +inf
    return x


def _win(A):
    return None if A == 0 else resample.limit_window(A, DEV)


def _win_host(A):
    return None if A == 0 else resample.limit_window_design(A)


def run(wave, frames, params, A, spf, trim, rho=RHO):
    """One `ops.wave_dynamics` call into a canary-filled `out` with a row stride of its own -> (out, dyn, lin, s) as numpy."""
    B, L = wave.shape
    T_cap = L // spf
    out = torch.full((B, L + 3), float(CANARY), device=DEV)
    work = torch.full((ops.wave_dynamics_workspace_bytes(B, T_cap, spf) // 4,), float(CANARY), device=DEV)
    got, dyn = ops.wave_dynamics(torch.from_numpy(wave).to(DEV), torch.tensor(frames, dtype=torch.int32, device=DEV),
                                 torch.tensor(np.asarray(params, dtype=np.float32), device=DEV), _win(A), A=A, rho=rho, trim=trim,
                                 samples_per_frame=spf, out=out[:, :L], workspace=work.view(torch.uint8))
    assert got.data_ptr() == out.data_ptr() and dyn.dtype == torch.float32 and tuple(dyn.shape) == (B, 2)
    kcap = (L + 63) // 64
    w = work.cpu().numpy()
    return out.cpu().numpy(), dyn.cpu().numpy(), w[:B * kcap].reshape(B, kcap), w[B * kcap:2 * B * kcap].reshape(B, kcap)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_row(x, n, p, A, rho, out, dyn, lin, s, tag):
    """Every bar of the issue for one row: `out` the whole row with its stride pad, `lin` / `s` its rows of the workspace."""
    assert (out[n:] == CANARY).all(), (tag, "written at or past n_b, or outside the row's stride")
    ref_out, ref_dyn, st = R.reference_row(x[:n], p, A, _win_host(A), rho)
    if st is None:
        assert np.array_equal(bits(out[:n]), bits(x[:n])) and dyn.tolist() == [0.0, 0.0], (tag, "left alone: a bit copy")
        return
    K = (n + 63) // 64
    assert np.array_equal(bits(s[:K]), bits(st["s"])), (tag, "block sums")
    assert (lin[K:] == CANARY).all() and (s[max(K, (K + 31) // 32 * 32):] == CANARY).all(), tag
    assert R.ulp_diff(lin[:K], st["lin"]).max() <= 1, (tag, "lin", R.ulp_diff(lin[:K], st["lin"]).max())
    assert np.array_equal(bits(out[:n]), bits(R.apply_gain(x[:n], lin[:K]))), (tag, "rule 8 over the device's lin")
    fin = np.isfinite(x[:n])
    assert np.array_equal(np.isnan(out[:n]), np.isnan(x[:n])) and np.array_equal(out[:n][~fin & ~np.isnan(x[:n])], x[:n][~fin & ~np.isnan(x[:n])])
    err = np.abs(out[:n][fin].astype(np.float64) - ref_out[fin].astype(np.float64))
    assert (err <= R.out_bound(x[:n], st["lin"])[fin]).all(), (tag, "out against the contract's lin")
    assert R.ulp_diff(dyn[:1], ref_dyn[:1])[0] <= 1, (tag, dyn, ref_dyn)
    lo, hi = R.count_bounds(x[:n], p, A, _win_host(A), rho)
    assert lo <= dyn[1] <= hi and dyn[1] == int(dyn[1]), (tag, dyn, lo, hi)


def _counts_batch():
    L = max(COUNTS) + 7
    wave = np.stack([np.resize(signal(SIGNALS[b % len(SIGNALS)], max(n, 1), 100 + b), L) for b, n in enumerate(COUNTS)])
    for b, n in enumerate(COUNTS):
        wave[b, n:] = 0.77  # what lies past the row's end must not be read into a sum
    params = [SETTINGS[(b // len(SIGNALS) + b) % len(SETTINGS)] for b in range(len(COUNTS))]
    return wave.astype(np.float32), params


@pytest.mark.parametrize("A", [0, 1, 64])
def test_counts_around_every_grid_at_one_sample_per_frame(A):
    wave, params = _counts_batch()
    out, dyn, lin, s = run(wave, COUNTS, params, A, 1, 0)
    for b, n in enumerate(COUNTS):
        check_row(wave[b], n, params[b], A, RHO, out[b], dyn[b], lin[b], s[b], (b, n, SIGNALS[b % len(SIGNALS)], params[b]))
    torch.cuda.synchronize()
    assert ops.status() == 0


@pytest.mark.parametrize("spf,T_cap,frames,trim", [(5, 1000, [0, 1, 13, 40, 999, 1200, 700], 3), (600, 8, [1, 2, 5, 7, 9, 0, 3], 100)])
def test_every_signal_under_every_setting_in_frames_with_a_trim(spf, T_cap, frames, trim):
    """B = 35: each of the five signals under each of the seven settings, row lengths from `frames` (one over the capacity, one
    0), `T_cap` above the longest row, A = 3 (the default attack)."""
    L = spf * T_cap
    combos = [(sig, p) for sig in SIGNALS for p in SETTINGS]
    wave = np.stack([signal(sig, L, 7 * i + spf) for i, (sig, p) in enumerate(combos)])
    fr = [frames[i % len(frames)] for i in range(len(combos))]
    out, dyn, lin, s = run(wave, fr, [p for _, p in combos], 3, spf, trim)
    reduced = 0
    for b, (sig, p) in enumerate(combos):
        n = max(0, spf * min(max(fr[b], 0), T_cap) - trim)
        check_row(wave[b], n, p, 3, RHO, out[b], dyn[b], lin[b], s[b], (b, n, sig, p))
        reduced += dyn[b][1] > 0
        if p[0] == 0.0 and sig != "nonfinite":  # nothing reaches 0 dB: the row comes out as it went in
            assert np.array_equal(bits(out[b, :n]), bits(wave[b, :n])) and dyn[b].tolist() == [0.0, 0.0]
        if p[1] == 0.0 and n:  # ratio 1: the make-up gain alone
            assert np.array_equal(bits(out[b, :n]), bits(wave[b, :n] * np.float32(10.0 ** (np.float64(p[3]) / 20.0)))) or sig == "nonfinite"
    assert reduced >= 10, "the signals reach the thresholds"
    assert ops.status() == 0


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch():
    wave, params = _counts_batch()
    pick = [5, 9, 13, 16]  # 191, 2048, tile + 1 and chunk + 1 samples
    out, dyn, lin, s = run(wave, COUNTS, params, 3, 1, 0)
    order = list(range(len(COUNTS)))[::-1]
    out2, dyn2, lin2, s2 = run(wave[order], [COUNTS[i] for i in order], [params[i] for i in order], 3, 1, 0)
    for j, i in enumerate(order):
        assert np.array_equal(bits(out2[j]), bits(out[i])) and np.array_equal(bits(dyn2[j]), bits(dyn[i]))
        assert np.array_equal(bits(lin2[j]), bits(lin[i]))
    for i in pick:
        o1, d1, l1, _ = run(wave[i:i + 1], COUNTS[i:i + 1], params[i:i + 1], 3, 1, 0)
        assert np.array_equal(bits(o1[0]), bits(out[i])) and np.array_equal(bits(d1[0]), bits(dyn[i])) and np.array_equal(bits(l1[0]), bits(lin[i]))


# ---- rows of several chunks of the per-row launch ----------------------------------------------------------------------------------
LONG_A = (0, 3, 64)
LONG_P = (-55.0, 1.0, 4.0, 0.0)  # ratio inf: a block at -8 dBFS is reduced by 47 dB, and the release from it lasts 220 blocks


def _long_rows():
    """Two rows of more than 2 chunks + 2 * 64 blocks at one sample per frame.  "bursts": quiet noise with two loud bursts that
    end 144 blocks in front of block CHUNK and of block 2 CHUNK -- in front of the 2 A = 128 blocks of halo a span of A = 64
    begins with --, so that g in the first 70 blocks of chunks 2 and 3 is P from the chunk before minus k rho, and chunk 3
    follows a chunk that itself took a carry.  "steps": the level drawn anew every 8 blocks between -60 and -8 dBFS, so that the
    level changes everywhere inside [k0 - 2 A, k0 + 2 A) of both boundaries and the hold and the smoother read both halos."""
    K = 2 * CHUNK + 2 * 64 + 90
    n = 64 * K - 21  # a partial last block
    g = np.random.default_rng(77)
    x = g.standard_normal(64 * K).astype(np.float32)
    amp = np.full(K, 0.0012)
    for end in (CHUNK - 144, 2 * CHUNK - 144):
        amp[end - 60:end] = 0.4
    bursts = (x * np.repeat(amp, 64)).astype(np.float32)
    level = np.repeat(g.uniform(-60.0, -8.0, (K + 7) // 8), 8)[:K]
    steps = (x * np.repeat(10.0 ** (level / 20.0), 64)).astype(np.float32)
    return np.stack([bursts, steps]), n


def _carry_matters(x, A, chunks):
    """True for every chunk of `chunks` if a scan that loses its carry would give another `lin` inside that chunk."""
    st = R.row_stages(x, LONG_P, A, _win_host(A), RHO)
    lost = R.block_gain(R.attack(R.release_without_carry(st["c"], RHO, CHUNK, 2 * A), A, _win_host(A)), 0.0)
    return [bool((lost[CHUNK * j:CHUNK * (j + 1)] != st["lin"][CHUNK * j:CHUNK * (j + 1)]).any()) for j in chunks]


@pytest.mark.parametrize("A", LONG_A)
def test_rows_of_three_chunks_carry_the_scan_and_read_both_halos(A):
    wave, n = _long_rows()
    assert (n + 63) // 64 > 2 * CHUNK + 2 * 64 and all(_carry_matters(wave[0, :n], A, (1, 2))), "the bursts' release crosses both boundaries"
    assert A == 64 or all(_carry_matters(wave[1, :n], A, (1, 2)))
    L = wave.shape[1]
    counts = [n, n, 64 * (CHUNK + 2 * 64) + 1, L]  # and rows that end one block past the first boundary's forward halo, and at capacity
    batch, params = wave[[0, 1, 1, 0]], [LONG_P, LONG_P, (-45.0, 0.8, 0.0, 1.0), LONG_P]
    out, dyn, lin, s = run(batch, counts, params, A, 1, 0)
    for b, m in enumerate(counts):
        check_row(batch[b], m, params[b], A, RHO, out[b], dyn[b], lin[b], s[b], (b, m, params[b]))
    # a release that crosses a boundary: in the first blocks of chunks 2 and 3 of the bursts' row the reduction is far above the curve
    st = R.row_stages(wave[0, :n], LONG_P, A, _win_host(A), RHO)
    for k0 in (CHUNK, 2 * CHUNK):
        assert (st["c"][k0 - 100:k0 + 20] < 0.5).all() and (st["g"][k0 - 100:k0 + 20] > 5.0).all()
        assert (-20.0 * np.log10(lin[0, k0:k0 + 20].astype(np.float64)) > 5.0).all()
    # place independence: each row alone and at another index of another batch
    order = [3, 2, 1, 0]
    out2, dyn2, lin2, _ = run(batch[order], [counts[i] for i in order], [params[i] for i in order], A, 1, 0)
    for j, i in enumerate(order):
        assert np.array_equal(bits(out2[j]), bits(out[i])) and np.array_equal(bits(dyn2[j]), bits(dyn[i])) and np.array_equal(bits(lin2[j]), bits(lin[i]))
    o1, d1, l1, _ = run(batch[:1], counts[:1], params[:1], A, 1, 0)
    assert np.array_equal(bits(o1[0]), bits(out[0])) and np.array_equal(bits(d1[0]), bits(dyn[0])) and np.array_equal(bits(l1[0]), bits(lin[0]))
    assert ops.status() == 0


def test_wrapper_refuses_what_the_library_would():
    w = torch.zeros(2, 1200, device=DEV)
    f = torch.ones(2, dtype=torch.int32, device=DEV)
    p = torch.zeros(2, 4, device=DEV)
    with pytest.raises(_lib.St2Error, match="aliases"):
        ops.wave_dynamics(w, f, p, None, A=0, rho=0.2, out=w)
    with pytest.raises(_lib.St2Error, match="rho"):
        ops.wave_dynamics(w, f, p, None, A=0, rho=0.0)
    with pytest.raises(_lib.St2Error, match="too small"):
        ops.wave_dynamics(w, f, p, None, A=0, rho=0.2, workspace=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.St2Error, match="A=65"):
        ops.wave_dynamics(w, f, p, torch.ones(131, device=DEV), A=65, rho=0.2)
    with pytest.raises(_lib.St2Error, match="win"):
        ops.wave_dynamics(w, f, p, None, A=2, rho=0.2)
    with pytest.raises(_lib.St2Error, match="params"):
        ops.wave_dynamics(w, f, p[:1], None, A=0, rho=0.2)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _order(codes, pack):
    """Packed codes as integers that rise with the value they stand for: int16 as it is; a G.711 mu-law byte is the complement of
    sign | magnitude."""
    if pack == "s16":
        return codes.astype(np.int64)
    u = (~codes.astype(np.uint8)).astype(np.int64)
    return np.where(u & 0x80, u & 0x7f, -(u & 0x7f) - 1)


def _settings(P, under=(6.0, 3.0, None, 10.0)):
    """Settings for the four rows of the passage: thresholds `under` dB below each row's own RMS (None = left alone), so that
    every compressed row is reduced whatever level the tiny model speaks at."""
    rms = [20.0 * np.log10(max(float(w.double().pow(2).mean().sqrt()), 1e-4)) for w in P["waves"]]
    return dict(threshold_db=[None if u is None else float(np.clip(r - u, -70.0, 0.0)) for r, u in zip(rms, under)],
                ratio=[3.0, INF, 2.0, 1.5], knee_db=[6.0, 0.0, 6.0, 12.0], makeup_db=[0.0, 3.0, 0.0, -2.0])


def _pack(rows, frames, pack, rate, trim, spf):
    if pipeline._resamples(pack, rate):
        return ops.wave_resample_pack(rows, frames, 24000 if rate is None else rate, fmt=pack, trim=trim, samples_per_frame=spf)
    return ops.wave_pack(rows, frames, trim=trim, fmt=pack, samples_per_frame=spf)


@pytest.mark.parametrize("pack,rate", [("s16", None), ("ulaw", 8000)])
def test_end_to_end_packed_bytes_are_the_parent_packer_over_the_compressed_rows(pack, rate):
    """The packed bytes of a call with `dynamics=` are the existing pack entry over `ops.wave_dynamics`' rows (held to the contract
    above); a code of two values one fp32 rounding apart may differ, so against the contract's own rows -- through the same
    packer -- the codes are held to one step, as section 27's test argues."""
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler = P["model"], P["sampler"]
    dy = pipeline.Dynamics(K, attack_ms=8.0, release_db_per_s=120.0, **_settings(P))
    more = dict(P["kw"], max_frames=P["T"], marks=True, pack=pack, sample_rate=rate)
    base = pipeline.inference(model, sampler, P["b"]["tokens"], **more)
    res = pipeline.inference(model, sampler, P["b"]["tokens"], dynamics=dy, **more)
    rows, marks, dh = res.to_host(marks=True, dynamics=True)
    assert np.array_equal(marks, base.to_host(marks=True)[1]) and res.offsets.cpu().tolist() == base.offsets.cpu().tolist()
    assert res._ho.buf.numel() == base._ho.buf.numel() + (res._ho.samples_at - base._ho.samples_at), "one allocation, one more part"
    assert dh.dtype == np.float32 and dh.tobytes() == res.dynamics.cpu().numpy().tobytes() and dh[2].tolist() == [0.0, 0.0]
    assert (dh[[0, 1, 3], 1] > 0).all() and (dh[[0, 1, 3], 0] > 0).all(), "the three compressed rows were reduced"
    spf = res.wave.shape[-1] // P["T"]
    comp, table = ops.wave_dynamics(res.wave, res.frames, dy.params, resample.limit_window(dy.A, DEV), A=dy.A, rho=dy.rho, trim=P["trim"],
                                    samples_per_frame=spf)
    assert table.cpu().numpy().tobytes() == dh.tobytes()
    packed, offs = _pack(comp, res.frames, pack, rate, P["trim"], spf)
    o = offs.cpu().tolist()
    assert o == res.offsets.cpu().tolist() and packed[:o[-1]].cpu().numpy().tobytes() == res.packed[:o[-1]].cpu().numpy().tobytes()
    # the contract's rows through the same packer
    w, fr = res.wave[:, 0].cpu().numpy(), res.frames.cpu().tolist()
    want = np.zeros_like(w)
    pp = dy.params.cpu().numpy()
    for k in range(K):
        n = max(0, spf * fr[k] - P["trim"])
        want[k, :n] = R.reference_row(w[k, :n], pp[k], dy.A, resample.limit_window_design(dy.A), dy.rho)[0]
    ref_packed, _ = _pack(torch.from_numpy(want).to(DEV), res.frames, pack, rate, P["trim"], spf)
    a, b = _order(res.packed[:o[-1]].cpu().numpy(), pack), _order(ref_packed[:o[-1]].cpu().numpy(), pack)
    assert np.abs(a - b).max() <= 1
    plain = base.to_host()
    assert np.array_equal(rows[2], plain[2]), "a row that is left alone is the parent's row"
    assert not np.array_equal(rows[0], plain[0])
    torch.cuda.synchronize()
    ops.check_status()


def test_one_graph_serves_any_settings_without_a_second_capture():
    from test_controls_gpu import STEPS
    from test_passage_gpu import K, _passage
    P = _passage("libritts")
    model, sampler, b = P["model"], P["sampler"], P["b"]
    N = b["tokens"].shape[1]
    ld = b["lengths"].to(torch.int32).to(DEV)
    gs = pipeline.GraphedSynthesis(model, sampler, K, N, P["T"], STEPS, ref_s=P["ref_s"], trim=P["trim"], lj_tail=False, pack="s16",
                                   dynamics=True)
    other = dict(_settings(P, under=(None, 4.0, 8.0, 2.0)), ratio=4.0, knee_db=3.0)
    graphs = []
    for call, kw in ((dict(tokens=b["tokens"], lengths=ld, noise=b["noise"], step_noise=b["step_noise"], sine_noise=b["sine"],
                           dynamics=pipeline.Dynamics(K, **_settings(P))), _settings(P)), (dict(dynamics=pipeline.Dynamics(K, **other)), other)):
        res = gs(**call)
        graphs.append(gs._g["graph"])
        rows, dh = res.to_host(dynamics=True)
        rows, dh = [r.copy() for r in rows], dh.copy()
        want = pipeline.inference(model, sampler, b["tokens"], max_frames=P["T"], pack="s16", dynamics=pipeline.Dynamics(K, **kw), **P["kw"])
        w_rows, w_dh = want.to_host(dynamics=True)
        assert dh.tobytes() == w_dh.tobytes() and all(np.array_equal(x, y) for x, y in zip(rows, w_rows))
        assert (dh[:, 1] > 0).sum() == 3
    assert graphs[0] is graphs[1], "no second capture"
    with pytest.raises(ValueError, match="built without dynamics"):
        pipeline.GraphedSynthesis(model, sampler, K, N, P["T"], STEPS, ref_s=P["ref_s"], pack="s16")(dynamics=pipeline.Dynamics(K))
    torch.cuda.synchronize()
    ops.check_status()


def test_without_dynamics_the_hand_over_is_the_parents():
    from test_passage_gpu import K, _passage, _repack
    P = _passage("libritts")
    res = pipeline.inference(P["model"], P["sampler"], P["b"]["tokens"], max_frames=P["T"], pack="s16", passage=True, **P["kw"])
    want_packed, want_offs = _repack(P, "s16", None)
    total = int(want_offs[-1])
    assert torch.equal(res.offsets, want_offs) and torch.equal(res.packed[:total], want_packed[:total])
    assert res.dynamics is None and res._ho.samples_at == pipeline._HandOver(K, "s16").samples_at == (8 * (K + 1) + 15) // 16 * 16
