"""The length-aware reference-style path without a GPU: C ABI of st2_style_forward_ragged (argument validation before any
launch, the three backend-table sizes, the ABI version), the ragged style plan on HOST memory through the CPU backend of
tests/_cpu_backend_style_ragged.py (every row against the uniform plan run alone at the row's own width, NaN in every tail;
the number of conv launches independent of B) and the Python-side checks of `lengths=`."""
import ctypes as C

import pytest
import torch

import _cpu_backend_style_ragged as CBS
from _cpu_backend_style_ragged import style_ragged_cpu_backend
from benchdata import synth  # seeded synthetic weights (test + bench helper, not product code)
from styletts2_amd import _hooks, _lib, engine, ops, style
from styletts2_amd.style import StyleEncoder

WIDTHS = [131, 96, 80]  # every down-sampling stage is odd for one row and even for another: 131 66 33 17 9 / 96 48 24 12 6 / 80 .. 5
T_CAP = 131


def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_abi_version_stays_23():
    assert _lib.ABI_VERSION == 23 and _lib.load().st2_abi_version() == 23


def test_ragged_style_argument_validation_before_any_launch():
    lib = _lib.load()
    lens = (C.c_int32 * 2)(100, 90)
    lp = C.cast(lens, C.c_void_p)
    dummy = C.c_void_p(256)  # never dereferenced: every call below must fail on its geometry
    assert lib.st2_style_forward_ragged(dummy, 0, dummy, None, 2, 80, 100, dummy, dummy, 1 << 20, None) != 0
    assert "mel_len" in _err(lib)
    for B in (0, -1):
        assert lib.st2_style_forward_ragged(dummy, 0, dummy, lp, B, 80, 100, dummy, dummy, 1 << 20, None) != 0
        assert "B=%d" % B in _err(lib)
    assert lib.st2_style_forward_ragged(dummy, 0, dummy, lp, 2, 80, 79, dummy, dummy, 1 << 20, None) != 0
    assert "T_cap=79" in _err(lib)
    assert lib.st2_style_workspace_bytes_ragged(None, 0, 2, 80, 100) == -1


def test_debug_set_backend_accepts_three_slot_counts():
    lib = _lib.load()
    assert _lib.BACKEND_SLOTS_STYLE == ["dwconv3x3s2_len", "avgpool2x2_len", "style_lengths"]
    old, ragged = len(_lib.BACKEND_SLOTS), len(_lib.BACKEND_SLOTS) + len(_lib.BACKEND_SLOTS_RAGGED)
    full = ragged + len(_lib.BACKEND_SLOTS_STYLE)
    assert (old, ragged) == (33, 44) and full >= 46
    buf = C.create_string_buffer(8)
    ptr = C.cast(buf, C.c_void_p).value
    try:
        for n in (old, ragged, full):
            table = (C.c_void_p * n)(*([ptr] * n))  # never called: only the table's shape is checked here
            assert lib.st2_debug_set_backend(table, n) == 0, _err(lib)
        for n in (ragged + 1, full + 1):
            table = (C.c_void_p * n)(*([ptr] * n))
            assert lib.st2_debug_set_backend(table, n) != 0
            assert "entries" in _err(lib)
    finally:
        assert lib.st2_debug_set_backend(None, 0) == 0


def _small_encoder(seed):
    enc = StyleEncoder(dim_in=16, style_dim=32, max_conv_dim=64).eval()
    synth.init_spectral_norm_(enc, seed)
    return enc


def _padded_mel(widths, cap, seed):
    g = torch.Generator().manual_seed(seed)
    mel = torch.full((len(widths), 1, 80, cap), float("nan"))
    for b, w in enumerate(widths):
        mel[b, :, :, :w] = torch.randn(1, 80, w, generator=g)
    return mel


@pytest.fixture
def nan_workspace(monkeypatch):
    """Every workspace byte starts as 0xFF (fp32 NaN): what a plan does not write before it reads shows up in the result."""
    plain = engine.Engine._workspace

    def filled(self, *a, **k):
        ws, ptr, n = plain(self, *a, **k)
        ws.fill_(255)
        return ws, ptr, n
    monkeypatch.setattr(engine.Engine, "_workspace", filled)


def test_ragged_style_plan_rows_equal_solo_runs(nan_workspace):
    enc = _small_encoder(41)
    mel = _padded_mel(WIDTHS, T_CAP, 5)
    with style_ragged_cpu_backend():
        eng = engine.build_style_engine(enc, None, None)
        out = eng.style_forward(0, mel, frames=WIDTHS)
        for name in _lib.BACKEND_SLOTS_STYLE + ["conv1d_direct_len", "mean_tokens_len"]:
            assert CBS.CALLS.get(name, 0) > 0, "slot %s never ran" % name
        solos = [eng.style_forward(0, mel[b:b + 1, :, :, :w].contiguous()) for b, w in enumerate(WIDTHS)]
        with pytest.raises(_lib.St2Error):
            eng.style_forward(0, mel, frames=[131, 96, 79])        # a host length below 80 frames
        with pytest.raises(_lib.St2Error):
            eng.style_forward(0, mel, frames=[131, 96])            # wrong size
        with pytest.raises(_lib.St2Error):
            eng.style_forward(0, mel, frames=torch.tensor([131, 0, 96, 0, 80, 0], dtype=torch.int32)[::2])  # non-contiguous
    assert out.shape == (3, 32) and bool(torch.isfinite(out).all())
    for b, w in enumerate(WIDTHS):
        ref = solos[b][0]
        err = (out[b] - ref).abs().max().item()
        assert err <= 1e-6 * max(ref.abs().max().item(), 1.0), "row %d (width %d): %g against the solo run" % (b, w, err)


def test_ragged_style_plan_xs_path_rows_equal_solo_runs(nan_workspace):
    """A capacity of 256 columns with 3 x 48 = 144 input channels: the first 3x3 convs leave the fused kernel for
    st2_act_split_len + st2_conv1d_xs over the stacked rows (seam rows of length 0 included); the rows shorter than 256 run
    the fused kernel when alone."""
    enc = StyleEncoder(dim_in=48, style_dim=32, max_conv_dim=64).eval()
    synth.init_spectral_norm_(enc, 43)
    widths = [256, 131, 80]
    mel = _padded_mel(widths, 256, 8)
    with style_ragged_cpu_backend():
        eng = engine.build_style_engine(enc, None, None)
        out = eng.style_forward(0, mel, frames=widths)
        assert CBS.CALLS.get("conv1d_xs", 0) > 0 and CBS.CALLS.get("act_split_len", 0) > 0, CBS.CALLS
        solos = [eng.style_forward(0, mel[b:b + 1, :, :, :w].contiguous()) for b, w in enumerate(widths)]
    assert bool(torch.isfinite(out).all())
    for b, w in enumerate(widths):
        ref = solos[b][0]
        err = (out[b] - ref).abs().max().item()
        assert err <= 1e-6 * max(ref.abs().max().item(), 1.0), "row %d (width %d): %g against the solo run" % (b, w, err)


def test_ragged_style_batch_too_large_for_one_launch_fails_before_any_launch():
    """Full-size encoder: the stacked 3x3 convs of the 20-row stage keep the 6-way split-K of their per-clip launch, so
    B (20 + 2) - 2 rows x 6 slices must fit the 65535 grid rows of one launch (B <= 496).  A larger batch is refused by the
    workspace query and by the forward, with nothing launched."""
    lib = _lib.load()
    enc = StyleEncoder(dim_in=64, style_dim=128, max_conv_dim=512).eval()
    synth.init_spectral_norm_(enc, 44)
    lens = (C.c_int32 * 600)(*([100] * 600))
    dummy = C.c_void_p(256)  # never dereferenced
    with style_ragged_cpu_backend():
        eng = engine.build_style_engine(enc, None, None)
        assert lib.st2_style_workspace_bytes_ragged(eng.h, 0, 400, 80, 100) > 0
        CBS.CALLS.clear()
        assert lib.st2_style_workspace_bytes_ragged(eng.h, 0, 600, 80, 100) == -1
        assert lib.st2_style_forward_ragged(eng.h, 0, dummy, C.cast(lens, C.c_void_p), 600, 80, 100, dummy, dummy, 1 << 40,
                                            None) != 0
        assert "K slices" in _err(lib)
        assert not CBS.CALLS, CBS.CALLS


def test_ragged_style_plan_conv_launches_do_not_depend_on_B(nan_workspace):
    enc = _small_encoder(42)
    counts = []
    with style_ragged_cpu_backend():
        eng = engine.build_style_engine(enc, None, None)
        for widths in ([96, 80], [96, 80, 131, 100]):
            mel = _padded_mel(widths, T_CAP, 7)
            CBS.CALLS.clear()
            out = eng.style_forward(0, mel, frames=widths)
            assert bool(torch.isfinite(out).all())
            counts.append({k: CBS.CALLS.get(k, 0) for k in ("conv1d_f16s", "conv1d_xs", "conv1d_direct_len")})
    assert counts[0] == counts[1], counts
    assert sum(counts[0].values()) >= 1 + 2 * 4 + 2, counts  # first conv, two 3x3 per block, the 5x5 and the Linear at least


def test_python_side_length_checks():
    wave = torch.zeros(2, 24000)
    with pytest.raises(_lib.St2Error, match="23700"):
        style.compute_style(None, wave, lengths=[24000, 23699])                          # below the 80-frame minimum
    with pytest.raises(_lib.St2Error):
        style.compute_style(None, wave, lengths=[24000, 24001])                          # past the buffer
    with pytest.raises(_lib.St2Error):
        style.compute_style(None, wave, lengths=torch.tensor([24000] * 3, dtype=torch.int32))   # wrong size
    with pytest.raises(_lib.St2Error):
        style.compute_style(None, wave, lengths=torch.tensor([24000, 0, 24000, 0], dtype=torch.int32)[::2])  # non-contiguous
    with pytest.raises(_lib.St2Error):
        style.compute_style(None, wave, lengths=torch.tensor([24000, 24000]))            # int64
    with pytest.raises(_lib.St2Error, match="23700"):
        style.compute_style(None, [torch.zeros(24000), torch.zeros(100)])                # a list of clips, one too short
    with pytest.raises(_lib.St2Error, match="HIP device"):
        _small_encoder(1)(torch.zeros(2, 1, 80, 90), lengths=[90, 80])                  # a host mel never reaches the engine
    with _hooks.override(plan="python"):
        for call in (lambda: style.compute_style(None, wave, lengths=[24000, 24000]),
                     lambda: style.mel_spectrogram_engine(wave, lengths=[24000, 24000]),
                     lambda: _small_encoder(1)(torch.zeros(2, 1, 80, 90), lengths=[90, 80])):
            with pytest.raises(_lib.St2Error, match="engine plan"):
                call()
    # the kernel wrappers check `lengths` with _chk_len before anything else: a host tensor never reaches a launch
    lens = torch.tensor([5, 4], dtype=torch.int32)
    x, y = torch.zeros(2, 4, 3, 9), torch.zeros(2, 2, 3, 5)
    for call in (lambda: ops.avgpool2x2(x, y, lengths=lens), lambda: ops.dwconv3x3s2(x, torch.zeros(3, 3, 3), torch.zeros(3), y, lengths=lens),
                 lambda: ops.log_norm_(torch.zeros(2, 3, 9), 1e-5, -4.0, 4.0, lengths=lens),
                 lambda: ops.stft_frames(torch.zeros(2, 4000), 1200, 300, 600, lengths=lens)):
        with pytest.raises(_lib.St2Error, match="lengths"):
            call()
