"""Length-aware reference-style path on the GPU: the four `_len` kernels and st2_style_lengths against
per-row references computed on the row sliced to its own length (NaN in every tail), the plain entry of each of the four
against its `_len` entry at full lengths (one kernel behind both: the same bits), st2_style_forward_ragged against the
oracle and against the engine's own solo runs, `compute_style` on a ragged batch end to end, device against host lengths, the
clamp of an over-long device length, and one graph recorded with device lengths and replayed with others."""
import pytest
import torch

from _cpu_backend_style_ragged import style_lengths_table
from _util import manifest, rms
from benchdata import synth  # seeded synthetic weights / inputs (test + bench helper, not product code)
from oracle import ops_ref as R
from oracle import st2_oracle as O
from styletts2_amd import _lib, engine, models, ops, style

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def lens(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---- kernels ---------------------------------------------------------------------------------------------------------------
def test_stft_frames_len_rows_are_the_clips_alone():
    L, Ls = 24611, [24611, 24000, 23700]
    wave = torch.full((3, L), NAN)
    g = torch.Generator().manual_seed(1)
    for b, n in enumerate(Ls):
        wave[b, :n] = torch.randn(n, generator=g)
    fr, m_len = ops.stft_frames(wave.to(DEV), 1200, 300, 600, lengths=lens(Ls), min_length=23700, want_frames=True)
    fr = fr.cpu()
    assert fr.shape == (3, 1200, L // 300 + 1) and m_len.tolist() == [n // 300 + 1 for n in Ls]
    for b, n in enumerate(Ls):
        M = n // 300 + 1
        assert torch.equal(fr[b:b + 1, :, :M], R.stft_frames(wave[b:b + 1, :n], 1200, 300, 600))   # pure gather: bit-exact
        assert bool((fr[b, :, M:] == 0).all())


def test_log_norm_len_zeroes_the_tail():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(3, 80, 83, generator=g) * 10
    ms = [83, 82, 41]
    for b, m in enumerate(ms):
        x[b, :, m:] = NAN
    got = ops.log_norm_(x.to(DEV).clone(), 1e-5, -4.0, 4.0, lengths=lens(ms)).cpu()
    for b, m in enumerate(ms):
        ref = R.log_norm_(x[b:b + 1, :, :m].clone(), 1e-5, -4.0, 4.0)
        assert (got[b:b + 1, :, :m] - ref).abs().max().item() < 1e-6
        assert bool((got[b, :, m:] == 0).all())


@pytest.mark.parametrize("shape,widths", [((3, 8, 5, 33), [33, 32, 17]), ((2, 10, 64, 11), [11, 6])])
def test_dwconv_and_avgpool_len_rows_are_the_maps_alone(shape, widths):
    B, H, C, W = shape
    g = torch.Generator().manual_seed(3)
    big = torch.randn(B, H + 2, C, W, generator=g)                             # strided interior view of a padded map
    for b, w in enumerate(widths):
        big[b, :, :, w:] = NAN
    wt, bias = torch.randn(C, 3, 3, generator=g), torch.randn(C, generator=g)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    SENT = -12345.0
    out = ops.dwconv3x3s2(big.to(DEV)[:, 1:H + 1], wt.to(DEV), bias.to(DEV), torch.full((B, Ho, C, Wo), SENT, device=DEV),
                          lengths=lens(widths)).cpu()
    outp = ops.avgpool2x2(big.to(DEV)[:, 1:H + 1], torch.full((B, H // 2, C, (W + 1) // 2), SENT, device=DEV),
                          lengths=lens(widths)).cpu()
    for b, w in enumerate(widths):
        xm = big[b:b + 1, 1:H + 1, :, :w]
        wo = (w + 1) // 2
        ref = R.dwconv3x3s2(xm, wt, bias, torch.empty(1, Ho, C, wo))
        assert (out[b:b + 1, :, :, :wo] - ref).abs().max().item() < 1e-5
        assert bool((out[b, :, :, wo:] == SENT).all())
        refp = R.avgpool2x2(xm, torch.empty(1, H // 2, C, wo))
        assert (outp[b:b + 1, :, :, :wo] - refp).abs().max().item() < 1e-6
        assert bool((outp[b, :, :, wo:] == SENT).all())


# ---- the plain entry and the `_len` entry at full lengths: one kernel each, the same bits --------------------------------------
def test_stft_frames_plain_and_full_lengths_agree_bitwise():
    wave = torch.randn(2, 1030, generator=torch.Generator().manual_seed(31)).to(DEV)   # M = 258: a second 256-wide chunk
    plain = ops.stft_frames(wave, 8, 4, 4)
    fr, m_len = ops.stft_frames(wave, 8, 4, 4, lengths=lens([1030, 1030]), want_frames=True)
    assert plain.shape == (2, 8, 258) and m_len.tolist() == [258, 258]
    assert torch.equal(plain, fr)


def test_log_norm_plain_and_full_lengths_agree_bitwise():
    x = (torch.rand(2, 3, 259, generator=torch.Generator().manual_seed(32)) * 10).to(DEV)   # 1 554 elements, 259 columns
    plain = ops.log_norm_(x.clone(), 1e-5, -4.0, 4.0)
    assert torch.equal(plain, ops.log_norm_(x.clone(), 1e-5, -4.0, 4.0, lengths=lens([259, 259])))
    flat = ops.log_norm_(x.reshape(1554).clone(), 1e-5, -4.0, 4.0)                # the flat path covers every element
    assert flat.shape == (1554,) and torch.equal(flat, plain.reshape(1554))
    ref = R.log_norm_(x.cpu().reshape(1554).clone(), 1e-5, -4.0, 4.0)
    assert (flat.cpu() - ref).abs().max().item() < 1e-6


@pytest.mark.parametrize("H,C,W", [(4, 3, 515), (6, 5, 33)])                      # Wo = 258 from an odd W; one chunk, odd W
def test_dwconv_and_avgpool_plain_and_full_lengths_agree_bitwise(H, C, W):
    g = torch.Generator().manual_seed(33)
    x = torch.randn(2, H + 2, C, W, generator=g).to(DEV)[:, 1:H + 1]              # interior view of a padded map
    wt, bias = torch.randn(C, 3, 3, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    SENT = -12345.0

    def fresh(h):
        return torch.full((2, h, C, Wo), SENT, device=DEV)
    plain = ops.dwconv3x3s2(x, wt, bias, fresh(Ho))
    assert torch.equal(plain, ops.dwconv3x3s2(x, wt, bias, fresh(Ho), lengths=lens([W, W])))
    assert bool((plain != SENT).all())
    plain = ops.avgpool2x2(x, fresh(H // 2))
    assert torch.equal(plain, ops.avgpool2x2(x, fresh(H // 2), lengths=lens([W, W])))
    assert bool((plain != SENT).all())


def test_style_lengths_table_and_clamp():
    lib = _lib.load()
    mel_len = [131, 96, 80, 7, 100000]     # the last two are out of range: clamped to 80 / T_cap on the device
    n = lib.st2_style_lengths_count(len(mel_len), 80, 4)
    out = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.st2_style_lengths(lens(mel_len).data_ptr(), len(mel_len), 80, 131, 80, 4, out.data_ptr(), None),
               "st2_style_lengths")
    torch.cuda.synchronize()
    assert out[:n].tolist() == style_lengths_table(mel_len, 80, 131, 80, 4)
    assert out[n:].tolist() == [-7] * 8   # nothing past the table


# ---- encoder ---------------------------------------------------------------------------------------------------------------
def _small():
    enc = style.StyleEncoder(dim_in=16, style_dim=32, max_conv_dim=64).eval()
    synth.init_spectral_norm_(enc, 21)
    return enc


def _padded_mel(widths, cap, seed):
    g = torch.Generator().manual_seed(seed)
    mel = torch.full((len(widths), 1, 80, cap), NAN)
    for b, w in enumerate(widths):
        mel[b, :, :, :w] = torch.randn(1, 80, w, generator=g) * 0.8 - 0.2
    return mel


@pytest.fixture(scope="module")
def small_engine():
    enc = _small()
    return enc, engine.build_style_engine(enc, None, torch.device(DEV))


@pytest.mark.parametrize("widths,cap", [([131, 96, 80], 131), ([300, 257, 80], 300)])   # cap 300: rows on both sides of the 256-column threshold
def test_ragged_encoder_rows_equal_oracle_and_solo(small_engine, widths, cap):
    enc, eng = small_engine
    mel = _padded_mel(widths, cap, 5)
    out = eng.style_forward(0, mel.to(DEV), frames=lens(widths))
    host = eng.style_forward(0, mel.to(DEV), frames=widths)
    torch.cuda.synchronize()
    ops.check_status()
    assert torch.equal(out, host)                                              # device against host lengths: identical bits
    out = out.cpu()
    assert bool(torch.isfinite(out).all())
    sd = enc.state_dict()
    for b, w in enumerate(widths):
        x = mel[b:b + 1, :, :, :w].contiguous()
        ref = O.style_encoder(sd, x)[0]
        assert (out[b] - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item()), (b, w)
        solo = eng.style_forward(0, x.to(DEV)).cpu()[0]
        assert rms(out[b] - solo) <= 1e-6 * max(rms(solo), 1.0), (b, w, rms(out[b] - solo))


def test_ragged_encoder_full_rows_are_bitwise_the_uniform_plan(small_engine):
    _, eng = small_engine
    g = torch.Generator().manual_seed(9)
    for T in (131, 300):
        mel = (torch.randn(3, 1, 80, T, generator=g) * 0.8 - 0.2).to(DEV)
        assert torch.equal(eng.style_forward(0, mel, frames=lens([T] * 3)), eng.style_forward(0, mel))


def test_ragged_encoder_clamps_device_lengths_to_capacity(small_engine):
    _, eng = small_engine
    mel = _padded_mel([131, 96, 80], 131, 6)
    mel[0] = torch.randn(1, 80, 131, generator=torch.Generator().manual_seed(1))
    over = eng.style_forward(0, mel.to(DEV), frames=lens([100000, 96, 80]))
    at_cap = eng.style_forward(0, mel.to(DEV), frames=lens([131, 96, 80]))
    assert torch.equal(over, at_cap)
    under = eng.style_forward(0, mel.to(DEV), frames=lens([131, 7, -3]))       # below 80 frames: the rows at 80 frames
    at_min = eng.style_forward(0, mel.to(DEV), frames=lens([131, 80, 80]))
    assert torch.equal(under, at_min) and bool(torch.isfinite(under).all())


def test_ragged_encoder_full_size_stacked_rows_take_the_xs_path():
    """LibriTTS-size encoder (64 .. 512 channels) at a capacity of 300 columns: the 3 x 64 = 192-channel 3x3 convs and the
    64 -> 128 shortcut run st2_act_split_len + st2_conv1d_xs over the stacked rows; rows 257 and 80 wide among them.  Full
    rows stay bitwise the uniform plan (stages 2-3 keep the per-clip split-K)."""
    enc = style.StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512).eval()
    synth.init_spectral_norm_(enc, 22)
    eng = engine.build_style_engine(enc, None, torch.device(DEV))
    widths = [300, 257, 80]
    mel = _padded_mel(widths, 300, 11)
    out = eng.style_forward(0, mel.to(DEV), frames=lens(widths)).cpu()
    ops.check_status()
    sd = enc.state_dict()
    for b, w in enumerate(widths):
        x = mel[b:b + 1, :, :, :w].contiguous()
        ref = O.style_encoder(sd, x)[0]
        assert (out[b] - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item()), (b, w)
        solo = eng.style_forward(0, x.to(DEV)).cpu()[0]
        assert rms(out[b] - solo) <= 1e-6 * max(rms(solo), 1.0), (b, w, rms(out[b] - solo))
    full = (torch.randn(2, 1, 80, 300, generator=torch.Generator().manual_seed(12)) * 0.8 - 0.2).to(DEV)
    assert torch.equal(eng.style_forward(0, full, frames=lens([300, 300])), eng.style_forward(0, full))


# ---- compute_style end to end ----------------------------------------------------------------------------------------------
CLIPS = [72000, 48123, 23700]


@pytest.fixture(scope="module")
def libritts_style():
    man = manifest("libritts")
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    synth.init_spectral_norm_(model.style_encoder, 3)
    synth.init_spectral_norm_(model.predictor_encoder, 4)
    g = torch.Generator().manual_seed(0)
    clips = [torch.randn(n, generator=g) * 0.1 for n in CLIPS]
    sa, sp = model.style_encoder.state_dict(), model.predictor_encoder.state_dict()
    refs = [O.compute_style(sa, sp, c.unsqueeze(0))[0] for c in clips]       # each clip alone, computed once
    model.style_encoder.to(DEV)
    model.predictor_encoder.to(DEV)
    return model, clips, refs


def _padded_wave(clips, cap):
    wave = torch.full((len(clips), cap), NAN)
    for b, c in enumerate(clips):
        wave[b, :c.numel()] = c
    return wave.to(DEV)


def test_compute_style_ragged_vs_oracle_and_solo(libritts_style):
    model, clips, refs = libritts_style
    wave = _padded_wave(clips, max(CLIPS))
    mel = style.mel_spectrogram_engine(wave, lengths=CLIPS).cpu()
    for b, n in enumerate(CLIPS):
        assert bool((mel[b, :, 1 + n // 300:] == 0).all()) and bool(torch.isfinite(mel[b]).all())
    padded = style.compute_style(model, wave, lengths=lens(CLIPS))
    listed = style.compute_style(model, [c.to(DEV) for c in clips])
    torch.cuda.synchronize()
    ops.check_status()
    assert padded.shape == (3, 256) and torch.equal(padded, listed)
    for b, c in enumerate(clips):
        got = padded[b].cpu()
        assert (got - refs[b]).abs().max().item() < 2e-4 * max(1.0, refs[b].abs().max().item()), b
        solo = style.compute_style(model, c.to(DEV))[0].cpu()
        assert rms(got - solo) <= 1e-6 * max(rms(solo), 1.0), (b, rms(got - solo))


def test_compute_style_ragged_under_graph_capture(libritts_style):
    model, clips, _ = libritts_style
    wave = _padded_wave(clips, max(CLIPS))
    wave = torch.nan_to_num(wave, nan=0.25)                                    # the replay reads further into the rows
    static_len = lens(CLIPS)
    other = [60000, 72000, 30011]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        style.compute_style(model, wave, lengths=static_len)                   # warm-up: engines packed, mel weights cached
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        out = style.compute_style(model, wave, lengths=static_len)
    static_len.copy_(lens(other))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = style.compute_style(model, wave, lengths=lens(other))
    assert torch.equal(replayed, eager)
