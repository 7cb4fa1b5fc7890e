"""Tensor-level wrappers over the C ABI (include/st2.h).

Every function takes PyTorch-ROCm tensors (fp32, device memory, unit stride along the last axis),
forwards raw pointers + strides to libst2_hip.so on torch's current HIP stream and returns torch
tensors.  PyTorch is plumbing here (allocation, streams); all arithmetic happens in the HIP kernels.
There is no CPU path: a tensor that is not on a HIP device raises.
"""
import ctypes as C
import json
import warnings

import torch

from . import _hooks, _lib
from .weights import F16S_X_SCALE, SplitConvWeight
from ._lib import (ACT_EXP_SIN, ACT_GELU, ACT_GELU_TANH, ACT_LEAKY, ACT_NONE, ACT_TANH, PRO_ADAIN_LEAKY, PRO_ADAIN_SNAKE,  # noqa: F401
                   PRO_COLNORM, PRO_LEAKY, PRO_NONE, PRO_SNAKE, ConvDesc)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_AUX_STREAMS = {}


def aux_stream(dev, priority=0, index=0):
    """ONE auxiliary stream per (device, priority, index), created on first use and reused by everything that needs "a second stream"
    (graph-capture warm-ups, the long-form front).  HIP maps its streams onto a handful of hardware queues (4 by default); a
    process that keeps asking torch for new streams walks through torch's pool and sooner or later gets one that shares the
    hardware queue of the stream it is meant to overlap with -- the two then serialise (measured: the second model of a process
    138 ms two-stream against 118 for the first; profiles/LAB_NOTES.md round 5).  `index` > 0: further streams of the same kind
    (the long-form decoders of independent sentences, pipeline.synthesize_long decode_streams)."""
    dev = torch.device(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(priority), int(index))
    if key not in _AUX_STREAMS:
        _AUX_STREAMS[key] = torch.cuda.Stream(dev, priority=int(priority))
    return _AUX_STREAMS[key]


_PROBE_BUF = {}


def wait_blocks(waiter, victim, spin_cycles=3_000_000, mode="wait"):
    """Does an event wait queued on `waiter` (mode "wait") -- or a long kernel running on it (mode "kernel") -- hold up kernels
    of `victim`?  HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default): a `hipStreamWaitEvent`
    is a barrier packet at the head of its stream's HARDWARE queue -- until the event fires nothing behind it in that queue runs,
    whatever stream it belongs to.  Probe: a spin kernel (~1.5 ms) on a stream of its own, `waiter` waits for it (or runs the
    spin itself), a tiny kernel goes to `victim`; blocked iff the tiny kernel finishes only after the spin.  Both streams are
    warmed first (the first launch on a stream creates its queue).  Synchronises the device; start-up use only."""
    dev = victim.device
    key = dev.index
    if key not in _PROBE_BUF:
        _PROBE_BUF[key] = (torch.zeros(64, device=dev), torch.cuda.Stream(dev))
    buf, spin = _PROBE_BUF[key]
    for st in (waiter, victim, spin):
        with torch.cuda.stream(st):
            buf.add_(0.0)
    torch.cuda.synchronize(dev)
    e_spin, e_tiny = torch.cuda.Event(), torch.cuda.Event()
    src = waiter if mode == "kernel" else spin
    with torch.cuda.stream(src):
        torch.cuda._sleep(int(spin_cycles))
        e_spin.record(src)
    if mode != "kernel":
        waiter.wait_event(e_spin)
    with torch.cuda.stream(victim):
        buf.add_(1.0)
        e_tiny.record(victim)
    while not e_tiny.query():
        pass
    blocked = e_spin.query()  # the spin was over before the tiny kernel's completion was seen: it sat behind it
    torch.cuda.synchronize(dev)
    return bool(blocked)


def _chk(t, name, ndim=None):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.St2Error("%s must live on a HIP device (got %s); the engine has no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise _lib.St2Error("%s must be float32 (got %s)" % (name, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise _lib.St2Error("%s must be %d-D (got shape %s)" % (name, ndim, tuple(t.shape)))
    if t.dim() > 0 and t.shape[-1] > 1 and t.stride(-1) != 1:
        raise _lib.St2Error("%s must have unit stride along its last axis" % name)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _chk_len(t, name, n, like):
    """Per-row lengths of a ragged batch (include/st2.h, ABI v23): int32 [n], contiguous, on the device of `like`.  Checked
    before anything else of the call, so a bad one never reaches a launch.  Returns the device pointer (0 for None)."""
    if t is None:
        return 0
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise _lib.St2Error("%s must be an int32 tensor (got %s)" % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.numel() != n or not t.is_contiguous():
        raise _lib.St2Error("%s must be a contiguous tensor of %d entries (got shape %s)" % (name, n, tuple(t.shape)))
    if not t.is_cuda or not torch.is_tensor(like) or t.device != like.device:
        raise _lib.St2Error("%s must live on the device of the tensor it describes (%s, got %s)" % (
            name, like.device if torch.is_tensor(like) else None, t.device))
    return t.data_ptr()


def _chk_out(t, name, shape, like):
    """A caller-provided output view: float32, exactly `shape`, unit stride along its last axis, on the device of `like`.
    Checked before anything else of the call (as `_chk_len`), so a bad one never reaches a launch."""
    if t is None:
        return
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _lib.St2Error("%s must be a float32 tensor (got %s)" % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if not torch.is_tensor(like) or tuple(t.shape) != tuple(shape):
        raise _lib.St2Error("%s must have shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))
    if t.device != like.device:
        raise _lib.St2Error("%s must live on the device of the tensors it is computed from (%s, got %s)" % (
            name, like.device, t.device))
    if t.dim() > 0 and t.shape[-1] > 1 and t.stride(-1) != 1:
        raise _lib.St2Error("%s must have unit stride along its last axis" % name)


def _nb(t, ndim=3):
    """Rows of the batch a lengths tensor describes: the leading extent of `t`, or -1 (no lengths tensor fits) when `t` is not
    the `ndim`-D tensor the wrapper goes on to demand."""
    return t.shape[0] if torch.is_tensor(t) and t.dim() == ndim else -1


def _bs_cs(t):
    """(batch stride, channel stride) of an NCL view."""
    return t.stride(0), t.stride(1)


_PRO_NORM = (PRO_ADAIN_LEAKY, PRO_ADAIN_SNAKE, PRO_COLNORM)  # prologues that read stats / gamma / beta
_PRO_SNAKE = (PRO_ADAIN_SNAKE, PRO_SNAKE)  # prologues that read alpha


def _chk_prologue(pro, B, Cc, L, stats, gamma, beta, alpha, gb_seg):
    """Operands of a conv prologue over x [B, Cc, L] (include/st2.h st2_act_split / st2_conv_desc): stats [B, Cc, 2] (AdaIN) or
    [B, L, 2] (PRO_COLNORM), gamma / beta [1 or B, Cc] -- or [G, Cc] with `gb_seg` > 0, see `activate` -- and alpha [Cc]
    (Snake).  Returns the batch stride of gamma / beta (0: one row for the whole batch)."""
    gbs = 0
    if pro in _PRO_NORM:
        _chk(stats, "stats", 3)
        _chk(gamma, "gamma", 2)
        _chk(beta, "beta", 2)
        want = (B, L, 2) if pro == PRO_COLNORM else (B, Cc, 2)
        assert tuple(stats.shape) == want and stats.is_contiguous(), (stats.shape, want)
        assert gamma.shape[1] == Cc and beta.shape[1] == Cc
        gbs = gamma.stride(0) if gamma.shape[0] > 1 else 0
        bbs = beta.stride(0) if beta.shape[0] > 1 else 0
        if gb_seg:
            assert pro == PRO_COLNORM and B == 1 and gamma.shape[0] * gb_seg >= L and beta.shape[0] == gamma.shape[0]
            assert gbs == bbs
        else:
            assert gamma.shape[0] in (1, B) and beta.shape[0] == gamma.shape[0] and gbs == bbs
    if pro in _PRO_SNAKE:
        _chk(alpha, "alpha", 1)
        assert alpha.numel() == Cc and alpha.is_contiguous()
    return gbs


def _chk_split_weight(wt, C_in, C_out, ks):
    if (wt.C_in, wt.C_out, wt.ks) != (C_in, C_out, ks) or not wt.wq.is_cuda or not wt.wq.is_contiguous():
        raise _lib.St2Error("split weight is for (C_in=%d, C_out=%d, ks=%d) on %s, call has (%d, %d, %d)" % (
            wt.C_in, wt.C_out, wt.ks, wt.wq.device, C_in, C_out, ks))


def x_scale_for(pro):
    """Power of two applied to the activated conv input before its f16 hi/lo split.  Normalised inputs (AdaIN /
    LayerNorm prologues: O(1) values) take 8, which keeps the lo halves of typical activations in the normal f16
    range; un-normalised inputs (plain / LeakyReLU / Snake prologues: the decoder's `cat` buffer carries the F0 curve
    in Hz, generator stage outputs, FFN intermediates) take 1, i.e. the full +-65504 of f16 (the lo half is then exact
    to 2^-25 absolute through f16 subnormals).  Beyond the range the kernels clamp and raise STATUS_F16_RANGE."""
    return conv_plan(pro=pro).x_scale


def calibrated_x_scale(max_abs, margin_bits=3):
    """`st2_calibration_scale`: the power of two that puts max |pro(x)| = `max_abs` into the top octave below 2^(16 -
    margin_bits) of the f16 range -- what `Engine.calibrate` installs per conv site (0.0 for max_abs <= 0: keep the rule)."""
    return float(_lib.load().st2_calibration_scale(float(max_abs), int(margin_bits)))


def status(clear=False):
    """The library's sticky device-side status word (include/st2.h `st2_status`): no synchronisation; a bit is visible
    once the kernel that raised it has completed."""
    return _lib.load().st2_status(1 if clear else 0)


lstm_recoveries = 0  # check_status() calls that found ST2_STATUS_LSTM_RECOVERED (bench.py reports it)
frame_capacity_hits = 0  # check_status() calls that found ST2_STATUS_FRAME_CAPACITY (a row truncated to `max_frames`)


def check_status(ignore=0):
    """Raises St2Error if a kernel reported a device-side condition since the last check (and clears it).  Called by
    the pipeline at its existing host synchronisation points and at the start of every call for the previous one's
    kernels, so a failure is never silent and costs no extra synchronisation.  `ignore`: status bits the caller expects
    (pipeline.calibrate provokes F16_RANGE on purpose); every other bit is still reported.

    ST2_STATUS_FRAME_CAPACITY is a warning, not an exception, and takes ST2_STATUS_DURATION_SUM with it: the alignment expansion
    reports the truncated row a second time under that bit.  The word is ONE per process, so a genuine DURATION_SUM (forced
    durations with a wrong `total_frames` on another path) raised between the same two checks is reported as the capacity
    warning too; a caller that mixes both kinds of call and needs them apart checks the status between them."""
    st = status(clear=True)
    if st > 0:
        st &= ~int(ignore)
    if st > 0 and st & _lib.STATUS_LSTM_RECOVERED:  # informational: the outputs are valid, the call lost its latency advantage
        global lstm_recoveries
        lstm_recoveries += 1
        warnings.warn("a cooperative BiLSTM group was not co-resident in time; the call was re-run on the single-CU kernel "
                      "in-stream (results valid; ST2_STATUS_LSTM_RECOVERED)", RuntimeWarning, stacklevel=2)
        st &= ~_lib.STATUS_LSTM_RECOVERED
    if st > 0 and st & _lib.STATUS_FRAME_CAPACITY:  # informational but reported: the call completed, one row is not its solo run
        global frame_capacity_hits
        frame_capacity_hits += 1
        warnings.warn("an utterance needed more frames than the capacity given with the call (`max_frames`) and was synthesised "
                      "truncated to it; the other rows of its batch are unaffected; retry that row with a larger capacity "
                      "(ST2_STATUS_FRAME_CAPACITY)", RuntimeWarning, stacklevel=2)
        # the alignment expansion reports the same row as ST2_STATUS_DURATION_SUM (its durations do not sum to the clamped frame
        # count): with the capacity bit set that is the same event, not a caller's wrong `total_frames`
        st &= ~(_lib.STATUS_FRAME_CAPACITY | _lib.STATUS_DURATION_SUM)
    if st <= 0:
        return
    msgs = []
    if st & _lib.STATUS_F16_RANGE:
        msgs.append("a split-f16 conv operand exceeded the f16 range (|x * x_scale| > 65504) and was clamped: the "
                    "result is finite but wrong; calibrate the operand scales for this checkpoint (pipeline.calibrate / st2_calibrate) and "
                    "check it with tools/validate_checkpoint.py, which names the conv site and its headroom")
    if st & _lib.STATUS_LSTM_TIMEOUT:
        msgs.append("a cooperative BiLSTM group timed out (its workgroups were not co-resident in time) on a launch without "
                    "the recovery pass: outputs of that call are invalid")
    if st & _lib.STATUS_DURATION_SUM:
        msgs.append("a row of the supplied durations does not sum to the frame count given with it (`total_frames`): the "
                    "alignment of that call repeated its last phoneme")
    raise _lib.St2Error("device-side status 0x%x: %s" % (st, "; ".join(msgs)))


class conv_autotune:
    """`with ops.conv_autotune(): forward(...)` -- start-up autotuning of the xs convs (include/st2.h `st2_conv_tune`): the
    first launch of every shape class inside the block times its bitwise-equivalent builds (tile shape / occupancy,
    dispatch-order or XCD-aware tile order) on this box and keeps the fastest; later calls (inside or outside the block, eager or graph-captured) run it.  Boxes of the same SKU differ by
    up to 1.75 x on individual classes with the rule's build, so a serving process runs one forward per batch shape in
    here before taking traffic.  `reset=True` forgets earlier measurements of the current device first."""

    def __init__(self, reset=False):
        self.reset = reset

    def __enter__(self):
        lib = _lib.load()
        if self.reset:
            _lib.check(lib.st2_conv_tune(-1), "st2_conv_tune")
        _lib.check(lib.st2_conv_tune(1), "st2_conv_tune")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _lib.check(_lib.load().st2_conv_tune(0), "st2_conv_tune")
        return False


TUNE_VARIANT_BITS = {1: "128x256 tiles, 2 wg/CU", 2: "XCD-aware tile order"}


def tune_variant_name(v):
    if v < 0:
        return "rule"
    names = [n for b, n in TUNE_VARIANT_BITS.items() if v & b]
    return " + ".join(names) if names else "128x128 tiles, 3 wg/CU, dispatch order"


def conv_tune_table():
    """The autotuner's table for the current device: a list of dicts {ks, C_in, C_out, L, B, chosen, candidates: [{variant,
    name, ms}]} (ms = 0 for classes pinned by hand)."""
    lib = _lib.load()
    n = lib.st2_conv_tune_read(None, 0)
    rows = (C.c_double * (24 * max(n, 1)))()
    n = min(n, lib.st2_conv_tune_read(rows, n))
    out = []
    for i in range(n):
        r = rows[24 * i:24 * i + 24]
        cands = [{"variant": int(r[8 + 2 * j]), "name": tune_variant_name(int(r[8 + 2 * j])), "ms": round(r[9 + 2 * j], 5)}
                 for j in range(int(r[7]))]
        out.append({"ks": int(r[0]), "C_in": int(r[1]), "C_out": int(r[2]), "L": int(r[3]), "B": int(r[4]),
                    "chosen": int(r[6]), "chosen_name": tune_variant_name(int(r[6])), "candidates": cands})
    return out


def conv_tune_set(ks, C_in, C_out, L_out, B, variant):
    """Pins (variant >= 0) or erases (-1) the build of one shape class on the current device (tests, A/B probes)."""
    _lib.check(_lib.load().st2_conv_tune_set(ks, C_in, C_out, L_out, B, variant), "st2_conv_tune_set")


def probe_cu_health():
    """(report dict, CU mask as a list of 32-bit words, number of excluded CUs) -- include/st2.h `st2_probe_cu_health`: which
    CUs of this box run the conv path's workgroups abnormally slowly, and the CU mask of the device without them."""
    buf = C.create_string_buffer(16384)
    mask = (C.c_uint32 * 16)()
    n = C.c_int32(0)
    _lib.check(_lib.load().st2_probe_cu_health(buf, len(buf), mask, 16, C.byref(n)), "st2_probe_cu_health")
    rep = json.loads(buf.value.decode())
    words = (rep["cus"] + 31) // 32
    return rep, [int(mask[i]) for i in range(words)], int(n.value)


class headroom:
    """`with ops.headroom() as h: forward(...)` then `h.rows`: where every split-f16 conv operand of that forward sat in the
    f16 range, BOTH ends (include/st2.h `st2_debug_headroom`; debug hook: extra launches, a scratch allocation, synchronises).
    rows = [{index, kind ("act_split" | "fused conv"), pro, B, C, L, x_scale, max_abs, frac, rel_err, sub_share, site}]:
    frac = max |x_scale * pro(x)| / 65504 (>= 1: clamped, ST2_STATUS_F16_RANGE); rel_err = relative RMS error the hi/lo split
    adds to the operand (fp32 storage: 3.4e-8; all lo halves normal: ~4e-8; an operand at 1e-3 with x_scale 1: ~2e-5);
    sub_share = share of the operand's energy in elements whose lo half is a subnormal f16; site = the engine's conv site
    (Engine.calibration() index) or -1 for per-kernel calls."""

    def __enter__(self):
        _lib.check(_lib.load().st2_debug_headroom(1), "st2_debug_headroom")
        self.rows = []
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        torch.cuda.synchronize()
        _lib.check(lib.st2_debug_headroom(0), "st2_debug_headroom")
        n = lib.st2_debug_headroom_read(None, 0)
        W = _lib.HEADROOM_COLS
        buf = (C.c_double * (W * max(n, 1)))()
        n = min(n, lib.st2_debug_headroom_read(buf, n))
        pro_names = ["none", "leaky", "adain+leaky", "adain+snake", "snake", "layernorm"]
        for i in range(max(n, 0)):
            r = buf[W * i:W * i + W]
            self.rows.append({"index": i, "kind": "fused conv" if int(r[0]) else "act_split", "pro": pro_names[int(r[1])],
                              "B": int(r[2]), "C": int(r[3]), "L": int(r[4]), "x_scale": r[5], "max_abs": r[6], "frac": r[7],
                              "rel_err": r[8], "sub_share": r[9], "site": int(r[10]), "engine": int(r[11])})
        return False


def probe_box(level=0):
    """Micro-measurements of the current device as a dict (include/st2.h `st2_probe_box`; ~0.5 s, synchronises)."""
    buf = C.create_string_buffer(16384)
    _lib.check(_lib.load().st2_probe_box(buf, len(buf), level), "st2_probe_box")
    return json.loads(buf.value.decode())


def conv_plan(B=0, C_in=0, C_out=0, L_in=0, L_out=0, ks=1, pad_left=0, pro=PRO_NONE, want_stats=False, gb_seg=0,
              force_fused=None):
    """`st2_conv_launch_plan` (include/st2.h): how the library issues a split-f16 conv of this geometry
    -- route, operand scale by rule, split-plane geometry, partial-sum layout, split-K workspace -- as a `_lib.ConvPlan`.  The
    C++ plans ask the same entry, so nothing of the rule is restated here.  `force_fused` defaults to the tests' selector
    (`conv_path() == "fused"`).  Host-only: needs no GPU."""
    d = ConvDesc()
    d.B, d.C_in, d.C_out, d.L_in, d.L_out, d.ks, d.dil, d.pad_left, d.pro = B, C_in, C_out, L_in, L_out, ks, 1, pad_left, pro
    p = _lib.ConvPlan()
    force = conv_path() != "xs" if force_fused is None else force_fused
    _lib.check(_lib.load().st2_conv_launch_plan(C.byref(d), int(want_stats), int(gb_seg), int(force), C.byref(p)),
               "st2_conv_launch_plan")
    return p


def __getattr__(name):
    """XS_HALO, XS_MIN_L, CVT_TILE: constants of the library, read from it (importing this module needs no built library)."""
    if name in ("XS_HALO", "XS_MIN_L"):
        return getattr(conv_plan(), {"XS_HALO": "xs_halo", "XS_MIN_L": "xs_min_l"}[name])
    if name == "CVT_TILE":
        return _lib.load().st2_convt_interleave_part_cols()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def prefer_fused(pro, C_in, ks):
    """Layers whose xs pair is HBM-bound take the fused kernel instead, whatever their length: the narrow HiFi-GAN stages
    (C <= 64) and the k = 3 resblock convs at C = 128 (the rule and its measurements: csrc/st2_conv1d_xs.hip)."""
    return bool(conv_plan(C_in=C_in, ks=ks, pro=pro).prefer_fused)


def token_merge_takes_xs(C_in, C_out, cols):
    """Does a k = 1 PRO_COLNORM conv over the token-merged view [1, C_in, cols] take the xs pair (the only route with a
    per-segment affine, `gb_seg`)?  What the C++ sampler plan asks for its q / kv convs, test selector aside."""
    return conv_plan(1, C_in, C_out, cols, cols, pro=PRO_COLNORM, force_fused=False).route == _lib.CONV_ROUTE_XS


def conv_path():
    """How convs over split-f16 weights are issued: "xs" = by the library's launch rule (`conv_plan`): st2_act_split +
    st2_conv1d_xs (activation in an HBM-bound pass of its own, pure MFMA conv, InstanceNorm partial sums from the conv
    epilogue) or st2_conv1d_f16s; "fused" (contract tests only, _hooks.py) = st2_conv1d_f16s everywhere."""
    return _hooks.conv_path


class XsTensor:
    """Pre-activated, pre-split conv operand written by `activate`: `data` is float16 [B, 2, cg, Lp, 8]
    (plane 0 = hi, 1 = lo; 16-byte slots of 8 channels), logical shape [B, C, L], `halo` zero columns in front."""

    def __init__(self, data, C, L, halo, x_scale=F16S_X_SCALE):
        self.data, self.C, self.L, self.halo, self.x_scale = data, C, L, halo, x_scale

    @property
    def cg(self):
        return self.data.shape[2]

    @property
    def Lp(self):
        return self.data.shape[3]


def xs_row_slots(L):
    """Slots per xs row for a tensor of length L: halo + L rounded up to the widest conv tile (512) + room for the
    last tile's taps (checked again inside st2_conv1d_xs)."""
    return conv_plan(L_in=L).xs_lp


def activate(x, *, pro=PRO_NONE, slope=0.0, stats=None, gamma=None, beta=None, gamma_plus_one=False, alpha=None,
              c_pad=32, gb_seg=0, x_scale=None, lengths=None, _plan=None):
    """`st2_act_split`: x [B, C, L] fp32 -> XsTensor holding split_f16(x_scale * pro(x)) with the conv's zero padding
    (x_scale = x_scale_for(pro) unless the caller passes a calibrated power of two, `calibrated_x_scale`).  `gb_seg` > 0 (PRO_COLNORM on a token-merged view [1, C, G * gb_seg]): gamma / beta
    are [G, C] and row l // gb_seg applies at position l (per-utterance AdaLayerNorm affine, include/st2.h).  `lengths` (int32 [B]
    on the device, `st2_act_split_len`): row b ends at lengths[b], the positions past it are written as the conv's zero padding."""
    lp = _chk_len(lengths, "lengths", _nb(x), x)
    if lengths is not None and pro == PRO_COLNORM:
        raise _lib.St2Error("activate: per-row lengths are not defined for PRO_COLNORM (st2_act_split_len)")
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, L = x.shape
    p = _plan or conv_plan(B, Cc, L_in=L, pro=pro)  # the planes' geometry and the scale by rule (`_plan`: conv1d has asked)
    cg = p.xs_cg if c_pad == 32 else (Cc + c_pad - 1) // c_pad * c_pad // 8
    data = torch.empty((B, 2, cg, p.xs_lp, 8), device=x.device, dtype=torch.float16)
    gbs = _chk_prologue(pro, B, Cc, L, stats, gamma, beta, alpha, gb_seg)
    xsc = float(x_scale) if x_scale else p.x_scale
    _lib.check(lib.st2_act_split_len(x.data_ptr(), x.stride(0), x.stride(1), B, Cc, L, pro, slope, _ptr(stats),
                                     _ptr(gamma), _ptr(beta), gbs, int(gb_seg), 1 if gamma_plus_one else 0, _ptr(alpha),
                                     xsc, data.data_ptr(), cg, p.xs_lp, p.xs_halo, lp, _stream()), "st2_act_split_len")
    return XsTensor(data, Cc, L, p.xs_halo, xsc)


def new_part(B, C, nt, device):
    """Buffer for a producer's per-slot partial sums: float2 [B * C][nt] (sum, sum of squares of y - shift) followed by float
    [B * C][nt] (the shifts = each slot's first stored value), include/st2.h `d.part`."""
    return torch.empty((B * C * nt * 3,), device=device, dtype=torch.float32)


def stats_finalize(part, B, C, nt, L, cols=128, eps=1e-5, out=None, lengths=None, len_div=1):
    """`st2_stats_finalize`: the buffer of `new_part` filled by the producer of a [B, C, L] tensor (slots of `cols` columns) ->
    stats [B, C, 2] (mean, rstd) of that tensor.  `lengths` (int32 [B * C / len_div] on the device, `st2_stats_finalize_len`):
    row r of the B * C covers its first lengths[r // len_div] columns; slots past that end are not read."""
    if lengths is None:
        len_div = 1  # no lengths to share between rows: what `st2_stats_finalize` passes
    elif len_div <= 0 or (B * C) % len_div:
        raise _lib.St2Error("stats_finalize: len_div=%d does not divide the %d rows" % (len_div, B * C))
    lp = _chk_len(lengths, "lengths", B * C // len_div, part)
    lib = _lib.load()
    assert part.numel() >= B * C * nt * 3 and part.is_contiguous()
    if out is None:
        out = torch.empty((B, C, 2), device=part.device, dtype=torch.float32)
    _lib.check(lib.st2_stats_finalize_len(part.data_ptr(), B * C, nt, L, eps, out.data_ptr(), int(cols), lp, int(len_div),
                                          _stream()), "st2_stats_finalize_len")
    return out


def conv1d_xs(xs, wt, C_out, ks, *, dil=1, pad_left=0, L_out=None, bias=None, out=None, res=None, res_shift=0,
              res2=None, div=1.0, act=ACT_NONE, act_split=0, act_slope=0.0, want_stats=False, part_cols=None, y_len=None):
    """`st2_conv1d_xs` on an XsTensor; with want_stats returns (out, stats [B, C_out, 2]) where the InstanceNorm
    statistics of `out` come from the conv epilogue's per-tile partial sums + `st2_stats_finalize`.  `y_len` (int32 [B] on the
    device, st2_conv_desc.y_len): row b of the output ends at y_len[b]; nothing is stored past it and the statistics cover
    only its columns (the input's own ends come from `activate(lengths=)`)."""
    if y_len is not None:
        _chk_len(y_len, "y_len", xs.data.shape[0] if isinstance(xs, XsTensor) else -1, xs.data if isinstance(xs, XsTensor) else None)
    lib = _lib.load()
    assert isinstance(xs, XsTensor) and isinstance(wt, SplitConvWeight)
    B, C_in, L_in = xs.data.shape[0], xs.C, xs.L
    _chk_split_weight(wt, C_in, C_out, ks)
    if L_out is None:
        L_out = L_in
    if out is None:
        out = torch.empty((B, C_out, L_out), device=xs.data.device, dtype=torch.float32)
    _chk(out, "out", 3)
    assert out.shape == (B, C_out, L_out), (out.shape, (B, C_out, L_out))
    d = ConvDesc()
    d.B, d.C_in, d.C_out, d.L_in, d.L_out, d.ks, d.dil, d.pad_left = B, C_in, C_out, L_in, L_out, ks, dil, pad_left
    d.xs, d.xs_cg, d.xs_lp, d.xs_halo = xs.data.data_ptr(), xs.cg, xs.Lp, xs.halo
    d.wq, d.wq_co_pad, d.wq_cin_pad = wt.wq.data_ptr(), wt.co_pad, wt.cin_pad
    d.x_scale, d.out_scale, d.w_row_scale = xs.x_scale, 1.0 / xs.x_scale, wt.row_scale.data_ptr()
    _chk(bias, "bias", 1)
    d.bias = _ptr(bias)
    d.y, d.y_bs, d.y_cs = out.data_ptr(), out.stride(0), out.stride(1)
    d.y_len = _ptr(y_len)
    _fill_epilogue(d, B, C_out, L_out, res, res_shift, res2, div, act, act_split, act_slope)
    part = None
    if want_stats:
        # 128, or 64 / 32 on a small grid: the library says which; `part_cols=128` (tests) keeps the 128-column tiles
        pc = part_cols or lib.st2_conv1d_xs_part_cols(C.byref(d))
        nt = (L_out + pc - 1) // pc
        part = new_part(B, C_out, nt, out.device)
        d.part, d.part_nt, d.part_cols = part.data_ptr(), nt, pc
    _launch_conv(lib.st2_conv1d_xs, "st2_conv1d_xs", d)
    if want_stats:
        return out, stats_finalize(part, B, C_out, nt, L_out, cols=d.part_cols or 128, lengths=y_len, len_div=C_out)
    return out


def _fill_epilogue(d, B, C_out, L_out, res, res_shift, res2, div, act, act_split, act_slope):
    if res is not None:
        _chk(res, "res", 3)
        assert res.shape[0] == B and res.shape[1] == C_out and res.shape[2] == (L_out + (1 << res_shift) - 1 >> res_shift)
        d.res, d.res_bs, d.res_cs, d.res_shift = res.data_ptr(), res.stride(0), res.stride(1), res_shift
    if res2 is not None:
        _chk(res2, "res2", 3)
        assert res2.shape == (B, C_out, L_out)
        d.res2, d.res2_bs, d.res2_cs = res2.data_ptr(), res2.stride(0), res2.stride(1)
    d.div = div
    d.act, d.act_split, d.act_slope = act, act_split, act_slope


def _launch_conv(fn, fname, d):
    _lib.check(fn(C.byref(d), _stream()), fname)


def conv1d(x, wt, C_out, ks, *, dil=1, pad_left=0, L_out=None, bias=None, out=None,
           pro=PRO_NONE, slope=0.0, stats=None, gamma=None, beta=None, gamma_plus_one=False, alpha=None,
           res=None, res_shift=0, res2=None, div=1.0, act=ACT_NONE, act_split=0, act_slope=0.0, want_stats=False,
           gb_seg=0, x_scale=None, x_len=None, y_len=None):
    """Fused Conv1d, see `st2_conv1d` / `st2_conv1d_f16s` / `st2_conv1d_xs` in include/st2.h.  wt is either the
    packed K-major fp32 weight [C_in*ks, w_ld] of weights.pack_conv() (exact-fp32 MFMA kernel) or a
    weights.SplitConvWeight from weights.pack_conv_f16s() (split-f16 MFMA kernels, fp32-class accuracy at 5.3x the
    rate ceiling).  With a SplitConvWeight, a prologue and conv_path() == "xs" the call is issued as
    st2_act_split + st2_conv1d_xs.  want_stats=True returns (out, InstanceNorm statistics of out [B, C_out, 2]).  x_len / y_len
    (int32 [B] on the device, st2_conv_desc): per-row ends of the input (zero padding after the prologue) and of the output
    (nothing stored past it, statistics over its columns); split-f16 weights only (st2_conv1d rejects them)."""
    _chk_len(x_len, "x_len", _nb(x), x)
    _chk_len(y_len, "y_len", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x", 3)
    B, C_in, L_in = x.shape
    split = isinstance(wt, SplitConvWeight)
    if L_out is None:
        L_out = L_in
    p = None  # the exact-fp32 kernel has one route and no workspace
    if split:  # refuses gb_seg (per-segment affine of a token-merged view) on the fused route
        p = conv_plan(B, C_in, C_out, L_in, L_out, ks, pad_left, pro, want_stats, gb_seg)
    if p is not None and p.route == _lib.CONV_ROUTE_XS:
        xs = activate(x, pro=pro, slope=slope, stats=stats, gamma=gamma, beta=beta,
                      gamma_plus_one=gamma_plus_one, alpha=alpha, gb_seg=gb_seg, x_scale=x_scale, lengths=x_len, _plan=p)
        return conv1d_xs(xs, wt, C_out, ks, dil=dil, pad_left=pad_left, L_out=L_out, bias=bias, out=out, res=res,
                         res_shift=res_shift, res2=res2, div=div, act=act, act_split=act_split, act_slope=act_slope,
                         want_stats=want_stats, part_cols=p.part_cols, y_len=y_len)
    if gb_seg:  # exact-fp32 weights (the plan has refused it for split ones)
        raise _lib.St2Error("gb_seg (per-segment affine of a token-merged view) exists on the st2_act_split + "
                            "st2_conv1d_xs path only; this call routes to the fused kernel")
    if split:
        _chk_split_weight(wt, C_in, C_out, ks)
    else:
        _chk(wt, "wt", 2)
        if wt.shape[0] != C_in * ks or not wt.is_contiguous():
            raise _lib.St2Error("packed weight has shape %s, expected [%d, >=%d]" % (tuple(wt.shape), C_in * ks,
                                                                                      C_out))
    if out is None:
        out = torch.empty((B, C_out, L_out), device=x.device, dtype=torch.float32)
    _chk(out, "out", 3)
    assert out.shape == (B, C_out, L_out), (out.shape, (B, C_out, L_out))
    d = ConvDesc()
    d.B, d.C_in, d.C_out, d.L_in, d.L_out, d.ks, d.dil, d.pad_left = B, C_in, C_out, L_in, L_out, ks, dil, pad_left
    d.x, d.x_bs, d.x_cs = x.data_ptr(), x.stride(0), x.stride(1)
    if split:
        d.wq, d.wq_co_pad, d.wq_cin_pad = wt.wq.data_ptr(), wt.co_pad, wt.cin_pad
        d.x_scale = float(x_scale) if x_scale else p.x_scale
        d.out_scale, d.w_row_scale = 1.0 / d.x_scale, wt.row_scale.data_ptr()
        fn, fname = lib.st2_conv1d_f16s, "st2_conv1d_f16s"
    else:
        d.wt, d.w_ld = wt.data_ptr(), wt.shape[1]
        fn, fname = lib.st2_conv1d, "st2_conv1d"
    _chk(bias, "bias", 1)
    d.bias = _ptr(bias)
    d.y, d.y_bs, d.y_cs = out.data_ptr(), out.stride(0), out.stride(1)
    d.x_len, d.y_len = _ptr(x_len), _ptr(y_len)
    d.pro, d.slope = pro, slope
    gbs = _chk_prologue(pro, B, C_in, L_in, stats, gamma, beta, alpha, 0)  # gb_seg was refused above
    if pro in _PRO_NORM:
        d.stats, d.gamma, d.beta, d.gb_bs = stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), gbs
        d.gamma_plus_one = 1 if gamma_plus_one else 0
    if pro in _PRO_SNAKE:
        d.alpha = alpha.data_ptr()
    _fill_epilogue(d, B, C_out, L_out, res, res_shift, res2, div, act, act_split, act_slope)
    ws = part = None
    if split and want_stats:  # InstanceNorm statistics of the output from the epilogue's per-tile partial sums
        part = torch.empty((p.part_floats,), device=out.device, dtype=torch.float32)
        d.part, d.part_nt = part.data_ptr(), p.part_nt
    elif split and p.splitk_bytes > 0:  # skinny layers (few workgroups, long k loop) run split-K inside this workspace
        ws = torch.empty((p.splitk_bytes,), device=x.device, dtype=torch.uint8)  # caching allocator: stream- and capture-safe
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), p.splitk_bytes
    _launch_conv(fn, fname, d)
    if want_stats:
        if part is not None:
            return out, stats_finalize(part, B, C_out, p.part_nt, L_out, cols=p.part_cols, lengths=y_len, len_div=C_out)
        return out, instnorm_stats(out, lengths=y_len)
    return out


def conv1d_direct(x, w, bias, stride, pad, L_out=None, out=None, x_len=None, y_len=None):
    """Plain-weight ([C_out, C_in, ks]) direct conv for strided / tiny-C_in layers (`st2_conv1d_direct`).  x_len / y_len
    (int32 [B] on the device, `st2_conv1d_direct_len`): the input row ends (zero padding) at x_len[b], outputs from y_len[b]
    on are exact zeros."""
    xlp = _chk_len(x_len, "x_len", _nb(x), x)
    ylp = _chk_len(y_len, "y_len", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(w, "w", 3)
    _chk(bias, "bias", 1)
    assert w.is_contiguous()
    B, C_in, L_in = x.shape
    C_out, C_in_w, ks = w.shape
    assert C_in_w == C_in
    if L_out is None:
        L_out = (L_in + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty((B, C_out, L_out), device=x.device, dtype=torch.float32)
    _chk(out, "out", 3)
    _lib.check(lib.st2_conv1d_direct_len(x.data_ptr(), x.stride(0), x.stride(1), w.data_ptr(), _ptr(bias), out.data_ptr(),
                                         out.stride(0), out.stride(1), B, C_in, C_out, L_in, L_out, ks, stride, pad,
                                         xlp, ylp, _stream()), "st2_conv1d_direct_len")
    return out


def phase_split(x, stride, pad, Lu):
    """x [B, C, L] -> xp [B, C*stride, Lu], xp[b, c*stride + r, u] = x[b, c, u*stride + r - pad] (`st2_phase_split`)."""
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, L = x.shape
    xp = torch.empty((B, Cc * stride, Lu), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_phase_split(x.data_ptr(), x.stride(0), x.stride(1), B, Cc, L, stride, pad, xp.data_ptr(),
                                   xp.stride(0), xp.stride(1), Lu, _stream()), "st2_phase_split")
    return xp


def instnorm_stats(x, eps=1e-5, out=None, lengths=None):
    """`st2_instnorm_stats`: x [B, C, L] -> (mean, rstd) [B, C, 2]; `lengths` (int32 [B] on the device,
    `st2_instnorm_stats_len`): row b over its first lengths[b] columns."""
    lp = _chk_len(lengths, "lengths", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, L = x.shape
    if out is None:
        out = torch.empty((B, Cc, 2), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_instnorm_stats_len(x.data_ptr(), x.stride(0), x.stride(1), B, Cc, L, eps, out.data_ptr(), lp,
                                          _stream()), "st2_instnorm_stats_len")
    return out


def colnorm_stats(x, eps=1e-5, out=None):
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, L = x.shape
    if out is None:
        out = torch.empty((B, L, 2), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_colnorm_stats(x.data_ptr(), x.stride(0), x.stride(1), B, Cc, L, eps, out.data_ptr(),
                                     _stream()), "st2_colnorm_stats")
    return out


def style_fc(s, wt, bias, act=ACT_NONE, out=None):
    """h = act(s @ wt + bias); wt is [K, J] (already transposed at pack time)."""
    lib = _lib.load()
    _chk(s, "s", 2)
    _chk(wt, "wt", 2)
    _chk(bias, "bias", 1)
    assert s.is_contiguous() and wt.is_contiguous()
    B, K = s.shape
    assert wt.shape[0] == K
    J = wt.shape[1]
    if out is None:
        out = torch.empty((B, J), device=s.device, dtype=torch.float32)
    _lib.check(lib.st2_style_fc(s.data_ptr(), B, K, wt.data_ptr(), _ptr(bias), J, act, out.data_ptr(), _stream()),
               "st2_style_fc")
    return out


def convt_interleave(phases, C_out, stride, pad, L_raw, bias=None, add=None, reflect_left=False, out=None,
                     want_stats=False, q_len=None, out_len=None):
    """`st2_convt_interleave[_stats]`; with want_stats returns (out, InstanceNorm statistics of out [B, C_out, 2]) from
    the kernel's per-tile partial sums + `st2_stats_finalize`.  q_len / out_len (int32 [B] on the device, both or neither,
    `st2_convt_interleave_stats_len`): row b has q_len[b] phase columns and out_len[b] outputs."""
    if (q_len is None) != (out_len is None):
        raise _lib.St2Error("convt_interleave: q_len and out_len go together")
    qlp = _chk_len(q_len, "q_len", _nb(phases), phases)
    olp = _chk_len(out_len, "out_len", _nb(phases), phases)
    lib = _lib.load()
    _chk(phases, "phases", 3)
    _chk(bias, "bias", 1)
    _chk(add, "add", 3)
    B, RC, Lq = phases.shape
    assert RC == stride * C_out
    L_out = L_raw + (1 if reflect_left else 0)
    if out is None:
        out = torch.empty((B, C_out, L_out), device=phases.device, dtype=torch.float32)
    if add is not None:
        assert add.shape == (B, C_out, L_out), (add.shape, (B, C_out, L_out))
    a_bs, a_cs = (add.stride(0), add.stride(1)) if add is not None else (0, 0)
    part, nt = None, 0
    tile = lib.st2_convt_interleave_part_cols()  # positions per tile = per entry of the partial-sum output
    if want_stats:
        nt = (L_out + tile - 1) // tile
        part = new_part(B, C_out, nt, phases.device)
    _lib.check(lib.st2_convt_interleave_stats_len(phases.data_ptr(), phases.stride(0), phases.stride(1), Lq, _ptr(bias),
                                                  _ptr(add), a_bs, a_cs, out.data_ptr(), out.stride(0), out.stride(1), B,
                                                  C_out, stride, pad, L_raw, 1 if reflect_left else 0, _ptr(part), nt,
                                                  qlp, olp, _stream()), "st2_convt_interleave_stats_len")
    if want_stats:
        return out, stats_finalize(part, B, C_out, nt, L_out, cols=tile, lengths=out_len, len_div=C_out)
    return out


def adain_leaky_pool(x, stats, gamma, beta, slope, w, bias, out=None, lengths=None):
    """`st2_adain_leaky_pool`: x [B, C, L] -> [B, C, 2L]; `lengths` (int32 [B] on the device, `st2_adain_leaky_pool_len`): the
    input row ends (zero padding) at lengths[b], 2 * lengths[b] outputs are written and the rest of the row is left as it was."""
    lp = _chk_len(lengths, "lengths", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(stats, "stats", 3)
    _chk(gamma, "gamma", 2)
    _chk(beta, "beta", 2)
    _chk(w, "w", 2)
    _chk(bias, "bias", 1)
    B, Cc, L = x.shape
    assert w.shape == (Cc, 3) and w.is_contiguous() and gamma.stride(0) == beta.stride(0)
    if out is None:
        out = torch.empty((B, Cc, 2 * L), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_adain_leaky_pool_len(x.data_ptr(), x.stride(0), x.stride(1), stats.data_ptr(), gamma.data_ptr(),
                                            beta.data_ptr(), gamma.stride(0), slope, w.data_ptr(), _ptr(bias),
                                            out.data_ptr(), out.stride(0), out.stride(1), B, Cc, L, lp, _stream()),
               "st2_adain_leaky_pool_len")
    return out


def har_source(f0, U, noise, lin_w, lin_b, sine_amp=0.1, noise_std=0.003, voiced_threshold=10.0,
               sample_rate=24000.0, f_len=None, out=None):
    """f0 [B, F] -> har_source [B, F*U]; noise [B, F*U, H] standard-normal draws.  `f_len` (int32 [B] on the device,
    `st2_har_source_len`): row b holds f_len[b] frames, its output is exactly 0 from f_len[b] * U on."""
    lp = _chk_len(f_len, "f_len", _nb(f0, 2), f0)
    lib = _lib.load()
    _chk(f0, "f0", 2)
    _chk(noise, "noise", 3)
    _chk(lin_w, "lin_w")
    _chk(lin_b, "lin_b")
    B, F = f0.shape
    H = noise.shape[2]
    assert f0.is_contiguous() and noise.is_contiguous() and noise.shape == (B, F * U, H)
    assert lin_w.numel() == H and lin_w.is_contiguous()
    scratch = torch.empty((B, H, F), device=f0.device, dtype=torch.float32)
    if out is None:
        out = torch.empty((B, F * U), device=f0.device, dtype=torch.float32)
    _chk(out, "out", 2)
    assert out.shape == (B, F * U) and out.is_contiguous()
    _lib.check(lib.st2_har_source_len(f0.data_ptr(), B, F, U, H, noise.data_ptr(), lin_w.data_ptr(), lin_b.data_ptr(),
                                      sine_amp, noise_std, voiced_threshold, sample_rate, scratch.data_ptr(),
                                      out.data_ptr(), lp, _stream()), "st2_har_source_len")
    return out


def stft_mag_phase(x, n_fft, hop, lengths=None, out=None):
    """x [B, L] -> (|X|, angle X) [B, n_fft + 2, L // hop + 1] (`st2_stft_mag_phase`).  `lengths` (int32 [B] on the device,
    `st2_stft_mag_phase_len`): row b is its first lengths[b] samples (clamped to n_fft / 2 + 1 .. L), reflect-padded at its
    own end; frames past lengths[b] // hop are exact zeros."""
    lp = _chk_len(lengths, "lengths", _nb(x, 2), x)
    lib = _lib.load()
    _chk(x, "x", 2)
    assert x.is_contiguous()
    B, L = x.shape
    M = L // hop + 1
    har = out if out is not None else torch.empty((B, n_fft + 2, M), device=x.device, dtype=torch.float32)
    _chk(har, "out", 3)
    assert har.shape == (B, n_fft + 2, M)
    _lib.check(lib.st2_stft_mag_phase_len(x.data_ptr(), B, L, n_fft, hop, har.data_ptr(), har.stride(0), har.stride(1), lp,
                                          _stream()), "st2_stft_mag_phase_len")
    return har


def istft(sp, n_fft, hop, m_len=None, out=None):
    """sp [B, n_fft+2, M] = cat(spec, phase) -> wave [B, 1, hop*(M-1)].  `m_len` (int32 [B] on the device, `st2_istft_len`):
    row b has m_len[b] frames (clamped to 2..M) and emits hop * (m_len[b] - 1) samples, exact zeros after them."""
    lp = _chk_len(m_len, "m_len", _nb(sp), sp)
    lib = _lib.load()
    _chk(sp, "sp", 3)
    B, Cc, M = sp.shape
    assert Cc == n_fft + 2
    wave = out if out is not None else torch.empty((B, 1, hop * (M - 1)), device=sp.device, dtype=torch.float32)
    _chk(wave, "out", 3)
    assert wave.shape == (B, 1, hop * (M - 1))
    _lib.check(lib.st2_istft_len(sp.data_ptr(), sp.stride(0), sp.stride(1), B, M, n_fft, hop, wave.data_ptr(),
                                 wave.stride(0), lp, _stream()), "st2_istft_len")
    return wave


def attention(q, k, v, heads, scale, out=None, key_len=None):
    """q, k, v: [B, heads*D, N] views with identical strides -> [B, heads*D, N].  key_len (int32 [B] on the device):
    keys m >= key_len[b] (clamped to 1..N) are padding: excluded from the softmax and never read (`st2_attention_keylen`).
    `out`: a float32 [B, heads*D, N] view on q's device (any batch / channel stride, e.g. a channel slice of a wider buffer)."""
    _chk_out(out, "out", q.shape if torch.is_tensor(q) else (), q)
    lib = _lib.load()
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, n, 3)
    B, HD, N = q.shape
    D = HD // heads
    assert k.shape == q.shape and v.shape == q.shape
    assert _bs_cs(q) == _bs_cs(k) == _bs_cs(v)
    lp = _chk_len(key_len, "key_len", B, q)
    if out is None:
        out = torch.empty((B, HD, N), device=q.device, dtype=torch.float32)
    _lib.check(lib.st2_attention_keylen(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), q.stride(1),
                                        out.data_ptr(), out.stride(0), out.stride(1), B, heads, D, N, scale, lp, _stream()),
               "st2_attention")
    return out


def colnorm_apply(x, stats, gamma, beta, *, gamma_plus_one=False, act=ACT_NONE, slope=0.0, lengths=None, out=None):
    """LayerNorm over channels applied (`st2_colnorm_apply`): x [B, C, L], stats [B, L, 2] from colnorm_stats,
    gamma / beta [1 or B, C]; positions l >= lengths[b] (int32 [B] on the device) are written as zero."""
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(stats, "stats", 3)
    _chk(gamma, "gamma", 2)
    _chk(beta, "beta", 2)
    B, Cc, L = x.shape
    assert tuple(stats.shape) == (B, L, 2) and stats.is_contiguous()
    assert gamma.shape[1] == Cc and beta.shape == gamma.shape and gamma.shape[0] in (1, B)
    gbs = gamma.stride(0) if gamma.shape[0] > 1 else 0
    assert (beta.stride(0) if beta.shape[0] > 1 else 0) == gbs and gamma.stride(1) == 1 and beta.stride(1) == 1
    lp = _chk_len(lengths, "lengths", B, x)
    if out is None:
        out = torch.empty((B, Cc, L), device=x.device, dtype=torch.float32)
    _chk(out, "out", 3)
    _lib.check(lib.st2_colnorm_apply(x.data_ptr(), x.stride(0), x.stride(1), stats.data_ptr(), gamma.data_ptr(),
                                     beta.data_ptr(), gbs, 1 if gamma_plus_one else 0, act, slope, lp, out.data_ptr(),
                                     out.stride(0), out.stride(1), B, Cc, L, _stream()), "st2_colnorm_apply")
    return out


_last_lstm_scratch = None  # scratch of the most recent cooperative launch (tests read its status word)


def lstm_mode():
    """"coop": W_hh register-resident over 8 CUs per group, one hidden-state exchange per step (st2_lstm_bidir_coop);
    "single" (tests only, _hooks.py): one CU per (utterance, direction) streaming W_hh from L2 (st2_lstm_bidir) -- the
    kernel the library itself falls back to when a device cannot hold a cooperative launch co-resident."""
    return _hooks.lstm


def lstm_bidir(G, whh_t, lengths=None, out=None):
    """G [B, 8H, N] projected inputs (both directions) -> Y [B, 2H, N]; lengths: int32 [B] on the device or None.
    The cooperative kernel is used when the library accepts the launch (its workgroups must all be co-resident: the
    library checks the device's occupancy and refuses otherwise -- then, and for B > 48, the single-CU kernel runs).
    A cooperative group that times out is repaired in-stream (st2_lstm_bidir_coop_recovering: the single-CU kernel re-runs
    the call into the same output; STATUS_LSTM_RECOVERED, a warning from `check_status()`)."""
    global _last_lstm_scratch
    lib = _lib.load()
    _chk(G, "G", 3)
    _chk(whh_t, "whh_t", 3)
    B, R, N = G.shape
    H = R // 8
    assert whh_t.shape == (2, H, 4 * H) and whh_t.is_contiguous()
    lp = _chk_len(lengths, "lengths", B, G)
    if out is None:
        out = torch.empty((B, 2 * H, N), device=G.device, dtype=torch.float32)
    nbytes = lib.st2_lstm_coop_scratch_bytes(B) if lstm_mode() == "coop" else 0
    if nbytes > 0:
        scratch = torch.empty((nbytes,), device=G.device, dtype=torch.uint8)
        fn = lib.st2_lstm_bidir_coop_recovering if _hooks.lstm_recover else lib.st2_lstm_bidir_coop
        rc = fn(G.data_ptr(), G.stride(0), G.stride(1), whh_t.data_ptr(), lp, B, H, N, out.data_ptr(), out.stride(0),
                out.stride(1), scratch.data_ptr(), nbytes, _stream())
        if rc == 0:
            _last_lstm_scratch = scratch
            return out
        msg = (lib.st2_last_error() or b"").decode()
        if "co-resident" not in msg:
            raise _lib.St2Error("st2_lstm_bidir_coop failed: %s" % msg)
        # refused (host-side occupancy check, nothing was launched): the single-CU kernel for THIS call only -- the
        # answer depends on the device and the batch, so it is asked again next time
    _lib.check(lib.st2_lstm_bidir(G.data_ptr(), G.stride(0), G.stride(1), whh_t.data_ptr(), lp, B, H, N,
                                  out.data_ptr(), out.stride(0), out.stride(1), _stream()), "st2_lstm_bidir")
    return out


def mfma_load(kind=0, workgroups=720, iters=400):
    """Queues one launch of the library's matrix-pipe load generator on the current stream (include/st2.h
    `st2_probe_mfma_stream`: the MFMA cadences next to which round 5's BiLSTM kernels returned wrong bits).  The co-residency
    canaries (tests/test_zz_coresidency_gpu.py, `pipeline.coresidency_selfcheck`) run product kernels on another stream
    meanwhile and demand the idle result bit for bit."""
    _lib.check(_lib.load().st2_probe_mfma_stream(int(kind), int(workgroups), int(iters), _stream()), "st2_probe_mfma_stream")


def lstm_coop_status():
    """Status word of the most recent cooperative LSTM launch (synchronises): 0 = ok, 1 = a spin timed out."""
    if _last_lstm_scratch is None:
        return 0
    return int(_last_lstm_scratch[:4].view(torch.int32).item())


def add_chanvec(x, v, out=None):
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(v, "v", 2)
    B, Cc, N = x.shape
    assert v.shape == (B, Cc)
    if out is None:
        out = torch.empty((B, Cc, N), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_add_chanvec(x.data_ptr(), x.stride(0), x.stride(1), v.data_ptr(), v.stride(0), out.data_ptr(),
                                   out.stride(0), out.stride(1), B, Cc, N, _stream()), "st2_add_chanvec")
    return out


def mean_tokens(x, out=None, lengths=None):
    """m[b, c] = mean over the first lengths[b] tokens (all N when lengths is None; int32 [B] on the device)."""
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, N = x.shape
    lp = _chk_len(lengths, "lengths", B, x)
    if out is None:
        out = torch.empty((B, Cc), device=x.device, dtype=torch.float32)
    _lib.check(lib.st2_mean_tokens_len(x.data_ptr(), x.stride(0), x.stride(1), out.data_ptr(), out.stride(0), B, Cc, N, lp,
                                       _stream()), "st2_mean_tokens")
    return out


def axpbypcz(x, a, y=None, b=0.0, z=None, c=0.0, out=None):
    """out = a*x + b*y + c*z (flat, contiguous)."""
    lib = _lib.load()
    _chk(x, "x")
    assert x.is_contiguous()
    for t in (y, z):
        if t is not None:
            _chk(t, "operand")
            assert t.is_contiguous() and t.numel() == x.numel()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.st2_axpbypcz(x.data_ptr(), a, _ptr(y), b, _ptr(z), c, out.data_ptr(), x.numel(), _stream()),
               "st2_axpbypcz")
    return out


def time_features(t, w, B, out=None):
    """`st2_time_features`: [B, 1 + 2*len(w)] = [t, sin(t w 2 pi), cos(t w 2 pi)] (denoiser time embedding input)."""
    lib = _lib.load()
    _chk(w, "w", 1)
    H2 = w.numel()
    if out is None:
        out = torch.empty((B, 1 + 2 * H2), device=w.device, dtype=torch.float32)
    _lib.check(lib.st2_time_features(float(t), w.data_ptr(), H2, B, out.data_ptr(), _stream()), "st2_time_features")
    return out


def tokens_to_channels(e, out, B=None):
    """`st2_tokens_to_channels`: e [B, N, E] (or [N, E] broadcast over `B`) -> out[b, :E, :N] = e[b].T, `out` an NCL view."""
    lib = _lib.load()
    _chk(e, "e")
    _chk(out, "out", 3)
    assert e.is_contiguous()
    if e.dim() == 2:
        N, E = e.shape
        e_bs = 0
        B = out.shape[0] if B is None else B
    else:
        B, N, E = e.shape
        e_bs = N * E
    assert out.shape[0] == B and out.shape[1] == E and out.shape[2] == N, (out.shape, (B, E, N))
    _lib.check(lib.st2_tokens_to_channels(e.data_ptr(), e_bs, B, N, E, out.data_ptr(), out.stride(0), out.stride(1),
                                          _stream()), "st2_tokens_to_channels")
    return out


def broadcast_cols(x, out):
    """`st2_broadcast_cols`: out[b, c, n] = x[b, c] for every n; x [B, C] (unit stride along C), out an NCL view."""
    lib = _lib.load()
    _chk(x, "x", 2)
    _chk(out, "out", 3)
    B, Cc = x.shape
    assert out.shape[0] == B and out.shape[1] == Cc
    _lib.check(lib.st2_broadcast_cols(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), out.stride(1), B, Cc,
                                      out.shape[2], _stream()), "st2_broadcast_cols")
    return out


def copy_ncl(x, out):
    """`st2_copy_ncl`: strided copy between NCL views of equal shape."""
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(out, "out", 3)
    assert x.shape == out.shape
    B, Cc, L = x.shape
    _lib.check(lib.st2_copy_ncl(x.data_ptr(), x.stride(0), x.stride(1), out.data_ptr(), out.stride(0), out.stride(1), B,
                                Cc, L, _stream()), "st2_copy_ncl")
    return out


def _chk_row(t, name, n, like):
    """A per-row control (include/st2.h "per-request controls"): fp32 [n], contiguous, on the device of `like`.  Checked before
    anything else of the call, as `_chk_len` checks lengths.  Returns the device pointer (0 for None)."""
    if t is None:
        return 0
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _lib.St2Error("%s must be a float32 tensor (got %s)" % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise _lib.St2Error("%s must be a contiguous 1-D tensor of %d entries (got shape %s)" % (name, n, tuple(t.shape)))
    if not t.is_cuda or not torch.is_tensor(like) or t.device != like.device:
        raise _lib.St2Error("%s must live on the device of the tensor it describes (%s, got %s)" % (
            name, like.device if torch.is_tensor(like) else None, t.device))
    return t.data_ptr()


def _chk_tok_row(t, name, B, N, like):
    """A per-token control (include/st2.h "per-token controls"): fp32 [B, N], contiguous, on the device of `like`.  Checked
    before anything else of the call, as `_chk_row` checks the per-row ones.  Returns the device pointer (0 for None)."""
    if t is None:
        return 0
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _lib.St2Error("%s must be a float32 tensor (got %s)" % (name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if tuple(t.shape) != (B, N) or not t.is_contiguous():
        raise _lib.St2Error("%s must be a contiguous [%d, %d] tensor (got shape %s)" % (name, B, N, tuple(t.shape)))
    if not t.is_cuda or not torch.is_tensor(like) or t.device != like.device:
        raise _lib.St2Error("%s must live on the device of the tensor it describes (%s, got %s)" % (
            name, like.device if torch.is_tensor(like) else None, t.device))
    return t.data_ptr()


def duration_head(x, w, bias, lengths=None, tail=0, want_sums=False, speed=None, tok_speed=None):
    """`st2_duration_head`: x [B, K, N] channel-major, w [J, K], bias [J] -> int64 durations [B, N] (and the un-rounded
    sigmoid sums when want_sums).  `speed` (fp32 [B] on the device, `st2_duration_head_rate`): row b's sums are divided by
    speed[b] (clamped to [0.25, 4], NaN -> 1) before they are rounded; the sums handed back stay un-scaled.  `tok_speed` (fp32
    [B, N] on the device, `st2_duration_head_rate_tok`): token n of row b is divided by the clamped fp32 product of speed[b] (1
    without `speed`) and tok_speed[b, n] instead."""
    sp = _chk_row(speed, "speed", _nb(x), x)
    tsp = _chk_tok_row(tok_speed, "tok_speed", _nb(x), x.shape[2] if _nb(x) >= 0 else -1, x)
    lib = _lib.load()
    _chk(x, "x", 3)
    _chk(w, "w", 2)
    _chk(bias, "bias", 1)
    B, K, N = x.shape
    J = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous() and bias.numel() == J
    lp = _chk_len(lengths, "lengths", B, x)
    dur = torch.empty((B, N), device=x.device, dtype=torch.int64)
    sums = torch.empty((B, N), device=x.device, dtype=torch.float32) if want_sums else None
    entry, rate = ("st2_duration_head", ()) if speed is None else ("st2_duration_head_rate", (sp,))
    if tok_speed is not None:
        entry, rate = "st2_duration_head_rate_tok", (sp, tsp)
    _lib.check(getattr(lib, entry)(x.data_ptr(), x.stride(0), x.stride(1), w.data_ptr(), bias.data_ptr(), B, K, J, N,
                                   lp, int(tail), *rate, dur.data_ptr(), _ptr(sums), _stream()), entry)
    return (dur, sums) if want_sums else dur


style_mix_launches = 0  # `st2_style_mix_rows` launches issued through the wrapper and the front (tests count them)


def style_mix_rows(s_pred, s_prev=None, ref_s=None, t=None, alpha=None, beta=None, t0=0.7, alpha0=0.3, beta0=0.7, carry=False):
    """`st2_style_mix_rows`: the front's style mixing as one launch.  s_pred [B, 2 sty] (the sampler's output), s_prev [B, 2 sty]
    (or [1, 2 sty] with `carry`), ref_s [B, 2 sty], per-row weights t / alpha / beta fp32 [B] on the device -- any of them
    None; a missing weight row means the scalar t0 / alpha0 / beta0.  Returns (ref [B, sty], s [B, sty], s_pred [B, 2 sty] =
    ref | s).  `carry`: the rows are consecutive sentences, row k mixes with row k-1's mixed result."""
    B = _nb(s_pred, 2)
    rows = [_chk_row(v, n, B, s_pred) for v, n in ((t, "t"), (alpha, "alpha"), (beta, "beta"))]
    lib = _lib.load()
    _chk(s_pred, "s_pred", 2)
    C2 = s_pred.shape[1]
    if C2 % 2 or not s_pred.is_contiguous():
        raise _lib.St2Error("s_pred must be a contiguous [B, 2 * style_dim] tensor (got %s)" % (tuple(s_pred.shape),))
    for v, name, nb in ((s_prev, "s_prev", 1 if carry else B), (ref_s, "ref_s", B)):
        _chk(v, name, 2)
        if v is not None and (tuple(v.shape) != (nb, C2) or not v.is_contiguous() or v.device != s_pred.device):
            raise _lib.St2Error("%s must be a contiguous [%d, %d] tensor on %s (got %s on %s)" % (
                name, nb, C2, s_pred.device, tuple(v.shape), v.device))
    for v, name in ((t0, "t0"), (alpha0, "alpha0"), (beta0, "beta0")):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError("%s=%r must lie in [0, 1]" % (name, v))
    new = lambda n: torch.empty((B, n), device=s_pred.device, dtype=torch.float32)
    ref, s, out = new(C2 // 2), new(C2 // 2), new(C2)
    global style_mix_launches
    style_mix_launches += 1
    _lib.check(lib.st2_style_mix_rows(s_pred.data_ptr(), _ptr(s_prev), _ptr(ref_s), *rows, float(t0), float(alpha0),
                                      float(beta0), B, C2 // 2, 1 if carry else 0, ref.data_ptr(), s.data_ptr(),
                                      out.data_ptr(), _stream()), "st2_style_mix_rows")
    return ref, s, out


def prosody_controls(f0, n, f0_scale=None, n_shift=None, frames=None):
    """`st2_prosody_controls`, in place: f0[b, l] *= f0_scale[b] and n[b, l] += n_shift[b] for l < 2 * frames[b] (every l
    without `frames`); f0, n [B, L] fp32 of equal strides, f0_scale / n_shift fp32 [B] on the device (clamped to [0.5, 2] /
    [-2, 2] where they are read; None leaves that curve alone), frames int32 [B] on the device.  Nothing at or past a row's
    end is read or written.  Returns (f0, n)."""
    B = _nb(f0, 2)
    fp = _chk_len(frames, "frames", B, f0)
    sc, sh = _chk_row(f0_scale, "f0_scale", B, f0), _chk_row(n_shift, "n_shift", B, f0)
    lib = _lib.load()
    _chk(f0, "f0", 2)
    _chk(n, "n", 2)
    if n.shape != f0.shape or n.stride() != f0.stride() or n.device != f0.device:
        raise _lib.St2Error("f0 and n must have one shape, one layout and one device (got %s / %s)" % (
            tuple(f0.shape), tuple(n.shape)))
    _lib.check(lib.st2_prosody_controls(f0.data_ptr(), n.data_ptr(), f0.stride(0), B, f0.shape[1], sc, sh, fp, _stream()),
               "st2_prosody_controls")
    return f0, n


def prosody_controls_tok(f0, n, dur, tok_f0_scale=None, tok_n_shift=None, frames=None, shift=False):
    """`st2_prosody_controls_tok`, in place: f0[b, l] *= tok_f0_scale[b, idx(b, l // 2)] and n[b, l] += tok_n_shift[b, idx(b,
    l // 2)] for l < 2 * frames[b] (every l without `frames`), idx(b, t) the token `expand_by_durations(.., dur, shift=)` gathers
    frame t from.  f0, n [B, L] fp32 of equal strides, L even; dur int64 [B, N] on the device; the token rows fp32 [B, N] on the
    device (clamped to [0.5, 2] / [-2, 2] where they are read; None leaves that curve alone); frames int32 [B] on the device.
    Nothing at or past a row's end is read or written.  Returns (f0, n)."""
    B = _nb(f0, 2)
    fp = _chk_len(frames, "frames", B, f0)
    N = dur.shape[1] if torch.is_tensor(dur) and dur.dim() == 2 else -1
    sc, sh = _chk_tok_row(tok_f0_scale, "tok_f0_scale", B, N, f0), _chk_tok_row(tok_n_shift, "tok_n_shift", B, N, f0)
    lib = _lib.load()
    _chk(f0, "f0", 2)
    _chk(n, "n", 2)
    if n.shape != f0.shape or n.stride() != f0.stride() or n.device != f0.device:
        raise _lib.St2Error("f0 and n must have one shape, one layout and one device (got %s / %s)" % (
            tuple(f0.shape), tuple(n.shape)))
    _chk_dev(dur, "dur", torch.int64, 2)
    if dur.shape[0] != B or dur.device != f0.device:
        raise _lib.St2Error("dur must hold %d rows on the device of f0 (got %s on %s)" % (B, tuple(dur.shape), dur.device))
    _lib.check(lib.st2_prosody_controls_tok(f0.data_ptr(), n.data_ptr(), f0.stride(0), B, f0.shape[1], dur.data_ptr(), N,
                                            1 if shift else 0, sc, sh, fp, _stream()), "st2_prosody_controls_tok")
    return f0, n


PITCH_POINTS = 8  # the most contour points of a row (`st2_pitch_shape`)


def pitch_shape(f0, range=None, tok_range=None, dur=None, contour=None, frames=None, shift=False, voiced_hz=10.0, lo_hz=40.0,
                hi_hz=1100.0, pitch=None):
    """`st2_pitch_shape`, in place (include/st2.h): the voiced columns of f0[b, :2 * frames[b]] move around
    the row's own voiced mean of log2 F0 -- the deviation times range[b] * tok_range[b, idx(b, l // 2)] (each clamped to [0, 4],
    NaN = 1, the product capped at 4) plus the contour's semitones at the frame's place in the row -- and are clamped to
    [lo_hz, hi_hz]; unvoiced columns (not finite, or <= voiced_hz) and everything at or past a row's end keep their bits.  f0
    [B, L] fp32, L even; range fp32 [B], tok_range fp32 [B, N] with dur int64 [B, N], contour fp32 [B, K, 2] of (position in
    [0, 1], semitones in [-24, 24]) points, K <= 8, a NaN point unused; frames int32 [B]; all on the device of f0, any of them
    None.  `pitch` (fp32 [B, 4] on the device, or True to have one made): {mean in Hz, voiced columns, lowest, highest output} per
    row.  Returns `pitch` or None.  One launch; none when there is nothing to apply and nothing to report."""
    B = _nb(f0, 2)
    fp = _chk_len(frames, "frames", B, f0)
    N = dur.shape[1] if torch.is_tensor(dur) and dur.dim() == 2 else tok_range.shape[1] if torch.is_tensor(tok_range) and \
        tok_range.dim() == 2 else -1
    rp, tp = _chk_row(range, "range", B, f0), _chk_tok_row(tok_range, "tok_range", B, N, f0)
    K = 0
    if contour is not None:
        if not torch.is_tensor(contour) or contour.dtype != torch.float32:
            raise _lib.St2Error("contour must be a float32 tensor (got %s)" % (
                contour.dtype if torch.is_tensor(contour) else type(contour).__name__))
        if contour.dim() != 3 or contour.shape[0] != B or contour.shape[2] != 2 or not contour.is_contiguous():
            raise _lib.St2Error("contour must be a contiguous [%d, K, 2] tensor (got shape %s)" % (B, tuple(contour.shape)))
        if not contour.is_cuda or not torch.is_tensor(f0) or contour.device != f0.device:
            raise _lib.St2Error("contour must live on the device of the tensor it describes (%s, got %s)" % (
                f0.device if torch.is_tensor(f0) else None, contour.device))
        K = contour.shape[1]
    lib = _lib.load()
    _chk(f0, "f0", 2)
    if f0.stride(1) != 1:
        raise _lib.St2Error("f0 must have unit stride along its columns (got strides %s)" % (tuple(f0.stride()),))
    if dur is not None:
        _chk_dev(dur, "dur", torch.int64, 2)
        if dur.shape[0] != B or dur.device != f0.device:
            raise _lib.St2Error("dur must hold %d rows on the device of f0 (got %s on %s)" % (B, tuple(dur.shape), dur.device))
    if pitch is True:
        pitch = torch.empty((B, 4), device=f0.device, dtype=torch.float32)
    elif pitch is not None:
        _chk_out(pitch, "pitch", (B, 4), f0)
    _lib.check(lib.st2_pitch_shape(f0.data_ptr(), f0.stride(0), B, f0.shape[1], fp, rp, tp, _ptr(dur), max(N, 0), 1 if shift else 0,
                                   _ptr(contour) if K else 0, K, float(voiced_hz), float(lo_hz), float(hi_hz), _ptr(pitch), _stream()),
               "st2_pitch_shape")
    return pitch


def expand_by_durations(x, dur, T, shift=False, out=None, lengths=None):
    """`st2_expand_by_durations`: x [B, C, N], dur int64 [B, N] (rows sum to T) -> [B, C, T].  `lengths` (int32 [B] on the
    device, `st2_expand_by_durations_len`): row b's durations sum to lengths[b], its columns from there on are exact zeros."""
    lp = _chk_len(lengths, "lengths", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x", 3)
    B, Cc, N = x.shape
    assert dur.is_cuda and dur.dtype == torch.int64 and dur.shape == (B, N) and dur.is_contiguous()
    if out is None:
        out = torch.empty((B, Cc, T), device=x.device, dtype=torch.float32)
    _chk(out, "out", 3)
    _lib.check(lib.st2_expand_by_durations_len(x.data_ptr(), x.stride(0), x.stride(1), dur.data_ptr(), B, Cc, N, T,
                                               1 if shift else 0, out.data_ptr(), out.stride(0), out.stride(1), lp, _stream()),
               "st2_expand_by_durations_len")
    return out


def ragged_lengths(frames, T_max, coef):
    """`st2_ragged_lengths`: frames int32 [B] on the device, coef = [(mul, add, div), ...] (at most 16, div > 0) -> int32
    [len(coef), B] with out[i][b] = (mul_i * f_b + add_i) // div_i (floor division), f_b = frames[b] clamped to 1..T_max."""
    B = frames.numel() if torch.is_tensor(frames) else -1
    _chk_len(frames, "frames", B, frames)
    lib = _lib.load()
    n = len(coef)
    flat = (C.c_int32 * (3 * max(n, 1)))(*[int(v) for t in coef for v in t])
    out = torch.empty((n, B), device=frames.device, dtype=torch.int32)
    _lib.check(lib.st2_ragged_lengths(frames.data_ptr(), B, int(T_max), n, flat, out.data_ptr(), _stream()), "st2_ragged_lengths")
    return out


def _chk_on_dev(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.St2Error("%s must live on a HIP device (got %s); the engine has no CPU path" % (
            name, t.device if torch.is_tensor(t) else type(t).__name__))


def _chk_dev(t, name, dtype, ndim):
    """A non-fp32 device operand of the sync-free entry points: on a HIP device, of `dtype`, `ndim`-D and contiguous."""
    _chk_on_dev(t, name)
    if t.dtype != dtype or t.dim() != ndim or not t.is_contiguous():
        raise _lib.St2Error("%s must be a contiguous %d-D %s tensor (got %s %s)" % (name, ndim, dtype, t.dtype, tuple(t.shape)))


def frames_from_durations(dur, lengths_dev, T_cap):
    """`st2_frames_from_durations`: dur int64 [B, N] on the device, lengths_dev int32 [B] on the device or None -> int32 [B]
    with frames[b] = clamp(sum_{n < lengths[b]} dur[b][n], 1, T_cap), without a host read.  A row over capacity raises
    ST2_STATUS_FRAME_CAPACITY (ops.check_status) and is synthesised truncated to T_cap frames."""
    _chk_dev(dur, "dur", torch.int64, 2)
    B, N = dur.shape
    lp = _chk_len(lengths_dev, "lengths_dev", B, dur)
    lib = _lib.load()
    frames = torch.empty((B,), device=dur.device, dtype=torch.int32)
    _lib.check(lib.st2_frames_from_durations(dur.data_ptr(), B, N, lp, int(T_cap), frames.data_ptr(), _stream()),
               "st2_frames_from_durations")
    return frames


def token_marks(dur, frames, T_cap, lengths=None, shift=False, trim=0, rate=None, samples_per_frame=600, out=None,
                want_bound=False, _edges=None):
    """`st2_token_marks`: where every token starts in its row's packed samples, without a host read.  dur int64 [B, N] on the
    device, frames int32 [B] on the device (None: every row has T_cap frames), lengths int32 [B] on the device or None ->
    int32 [B, N + 1]: marks[b, n] is the first sample of token n among the row's samples as `wave_pack` (rate None or 24000) /
    `wave_resample_pack` (`rate` one of `resample.RATES`) hand them over with the same `trim` and `samples_per_frame`;
    marks[b, N] is the row's sample count.  `shift`: the HiFi-GAN one-frame right shift of the expansion.  `out`: a contiguous
    int32 [B, N + 1] device tensor to write into.  `want_bound`: also return the boundaries in decoder frames (int32 [B, N + 1])."""
    from . import resample
    _chk_dev(dur, "dur", torch.int64, 2)
    B, N = dur.shape
    lp = _chk_len(lengths, "lengths", B, dur)
    fp = _chk_len(frames, "frames", B, dur)
    U, D = resample.ratio(resample.MODEL_RATE if rate is None else rate)
    if out is None:
        out = torch.empty((B, N + 1), device=dur.device, dtype=torch.int32)
    _chk_dev(out, "out", torch.int32, 2)
    if tuple(out.shape) != (B, N + 1) or out.device != dur.device:
        raise _lib.St2Error("out must be [%d, %d] on the device of dur (got %s on %s)" % (B, N + 1, tuple(out.shape), out.device))
    bound = torch.empty((B, N + 1), device=dur.device, dtype=torch.int32) if want_bound else None
    entry, more = ("st2_token_marks", ()) if _edges is None else ("st2_token_marks_edges", (_edges.data_ptr(),))
    _lib.check(getattr(_lib.load(), entry)(dur.data_ptr(), B, N, lp, fp, int(T_cap), 1 if shift else 0, int(samples_per_frame),
                                           int(trim), U, D, out.data_ptr(), _ptr(bound), *more, _stream()), entry)
    return (out, bound) if want_bound else out


def _chk_edges(edges, B, like):
    """An edges table: int32 with 2 B entries, contiguous, on the device of `like`."""
    _chk_dev(edges, "edges", torch.int32, edges.dim() if torch.is_tensor(edges) else 2)
    if edges.numel() != 2 * B or edges.device != like.device:
        raise _lib.St2Error("edges must hold [%d, 2] values on the device of its rows (got %s on %s)"
                            % (B, tuple(edges.shape), edges.device))
    return edges


def token_marks_edges(dur, frames, T_cap, edges, lengths=None, shift=False, trim=0, rate=None, samples_per_frame=600, out=None,
                      want_bound=False):
    """`st2_token_marks_edges`: `token_marks` for rows that `wave_edges` cut before they were packed.  edges int32 [B, 2] on the
    device, {head, count} as `wave_edges` wrote them; every other argument and the return value as `token_marks`.  A boundary at
    sample s of the uncut row is at clamp(s - head, 0, count) of the cut one, so marks[b, N] is still the row's packed sample
    count.  One launch, no host read."""
    _chk_dev(dur, "dur", torch.int64, 2)
    return token_marks(dur, frames, T_cap, lengths=lengths, shift=shift, trim=trim, rate=rate, samples_per_frame=samples_per_frame,
                       out=out, want_bound=want_bound, _edges=_chk_edges(edges, dur.shape[0], dur))


OUTPUT_FORMATS = {"f32": (_lib.PCM_F32, torch.float32), "s16": (_lib.PCM_S16, torch.int16),
                  "ulaw": (_lib.PCM_ULAW, torch.uint8), "alaw": (_lib.PCM_ALAW, torch.uint8)}
PACK_FORMATS = {k: OUTPUT_FORMATS[k] for k in ("f32", "s16")}  # what the plain move (no rate) writes; _lib.PACK_* are these codes


def _pcm_format(fmt, rate):
    """(format code, dtype) of a sample format of OUTPUT_FORMATS at a rate of `resample.RATES`; ValueError for any other."""
    from . import resample
    if fmt not in OUTPUT_FORMATS:
        raise ValueError("fmt must be one of %s, got %r" % (sorted(OUTPUT_FORMATS), fmt))
    if rate not in resample.RATES:
        raise ValueError("rate must be one of %s, got %r" % (list(resample.RATES), rate))
    return OUTPUT_FORMATS[fmt]


def _pack_operands(wave, frames, samples_per_frame, dtype, out, offsets, out_samples):
    """The operand work of the packing wrappers: wave [B, 1, L] or [B, L] flattened to [B, L], L a whole number of frames;
    frames, `out` (default: B * out_samples(L) entries of `dtype`) and `offsets` checked.
    -> (wave, frames pointer, B, L, samples per frame, out, offsets)"""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf = int(samples_per_frame)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    if out is None:
        out = torch.empty((B * out_samples(L),), device=wave.device, dtype=dtype)
    _chk_dev(out, "out", dtype, 1)
    if offsets is None:
        offsets = torch.empty((B + 1,), device=wave.device, dtype=torch.int64)
    _chk_dev(offsets, "offsets", torch.int64, 1)
    if offsets.numel() != B + 1 or out.device != wave.device or offsets.device != wave.device:
        raise _lib.St2Error("offsets must hold %d entries; out / offsets must live on the device of wave" % (B + 1))
    return wave, lp, B, L, spf, out, offsets


def _wave_pack(entry, wave, frames, rate, fmt, trim, out, offsets, samples_per_frame, plain=None, gaps=None, max_gap=None,
               level=()):
    """The body of the four packing wrappers; `entry` is the C entry the caller chose.  `plain`: the entry's refusal of a
    format outside PACK_FORMATS when there is no rate (the plain move, no table); None: the entry needs a rate.  `max_gap`
    (the gaps entries only): `gaps` and `max_gap` are passed on, and `out` defaults to `max_gap` more samples per row.  `level`
    (the level entry only): a 1-tuple of the table of `wave_level` or of None, passed on behind the stream."""
    from . import resample
    if rate is None and plain is not None:
        if fmt not in PACK_FORMATS:
            raise ValueError(plain % (sorted(PACK_FORMATS), fmt))
        code, dtype = PACK_FORMATS[fmt]
        table = lambda: (1, 1, 0, None)
    else:
        code, dtype = _pcm_format(fmt, rate)
        table = lambda: resample.table(rate, wave.device)  # first asked for once `wave` is known to live on a device
    room = 0 if max_gap is None else max(max_gap, 0)
    wave, lp, B, L, spf, out, offsets = _pack_operands(wave, frames, samples_per_frame, dtype, out, offsets,
                                                       lambda L: resample.output_samples(L, *table()[:2]) + room)
    breaks = () if max_gap is None else (_chk_len(gaps, "gaps", B, wave), max_gap)
    U, D, K, taps = table()
    how = (code,) if entry == "st2_wave_pack" else (U, D, _ptr(taps), K, code)
    gain = tuple(_ptr(_chk_level(t, B, wave)) for t in level)
    _lib.check(getattr(_lib.load(), entry)(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), *how, *breaks,
                                           out.data_ptr(), out.numel(), offsets.data_ptr(), _stream(), *gain), entry)
    return out, offsets


def _chk_level(level, B, wave):
    """A level table: None, or fp32 with 4 B entries, contiguous, on the device of `wave`."""
    if level is None:
        return None
    _chk_dev(level, "level", torch.float32, level.dim() if torch.is_tensor(level) else 2)
    if level.numel() != 4 * B or level.device != wave.device:
        raise _lib.St2Error("level must hold [%d, 4] values on the device of wave (got %s on %s)" % (B, tuple(level.shape), level.device))
    return level


def wave_pack(wave, frames, trim=0, fmt="s16", out=None, offsets=None, samples_per_frame=600):
    """`st2_wave_pack`: wave [B, 1, L] or [B, L] (L a multiple of `samples_per_frame`: the batch's frame capacity), frames
    int32 [B] on the device -> (packed, offsets): the first max(0, samples_per_frame * frames[b] - trim) samples of every row,
    back to back, as int16 PCM ("s16": rint(clamp(x, -1, 1) * 32767), NaN -> 0) or fp32 ("f32": a copy), and their int64
    [B + 1] exclusive prefix sum on the device (offsets[B] = the total).  `out` (1-D, of the format's dtype) bounds what is
    written: nothing at or past min(offsets[B], out.numel()); by default it holds every row at capacity.  No host read."""
    return _wave_pack("st2_wave_pack", wave, frames, None, fmt, trim, out, offsets, samples_per_frame,
                      plain="fmt must be one of %s, got %r")


def wave_resample_pack(wave, frames, rate, fmt="s16", trim=0, out=None, offsets=None, samples_per_frame=600):
    """`st2_wave_resample_pack`: `wave_pack` at an output rate and in an output format.  wave [B, 1, L] or [B, L] at 24 kHz,
    frames int32 [B] on the device -> (packed, offsets): row b's n_b = max(0, samples_per_frame * frames[b] - trim) valid
    samples resampled to `rate` (one of `resample.RATES`; m_b = ceil(n_b U / D) samples, U / D = rate / 24000 reduced) by the
    polyphase table of `resample.design`, back to back as fp32 ("f32"), 16-bit PCM ("s16", `wave_pack`'s rule) or G.711
    mu-law / A-law bytes of that 16-bit sample ("ulaw" / "alaw", uint8), and the int64 [B + 1] exclusive prefix sum of m_b.
    `out` (1-D, of the format's dtype) bounds what is written: nothing at or past min(offsets[B], out.numel()); by default it
    holds every row at capacity, ceil(L U / D) samples each.  No host read; the first call for a (rate, device) designs and
    uploads the table, which therefore must not happen under stream capture."""
    return _wave_pack("st2_wave_resample_pack", wave, frames, rate, fmt, trim, out, offsets, samples_per_frame)


def wave_pack_gaps(wave, frames, gaps, max_gap, rate=None, fmt="s16", trim=0, out=None, offsets=None, samples_per_frame=600):
    """`st2_wave_pack_gaps`: `wave_pack` (rate None: "f32" / "s16" at the model rate) or `wave_resample_pack` (`rate` one of
    `resample.RATES`, any format of OUTPUT_FORMATS) with a break behind every row.  gaps int32 [B] on the device: row b is
    followed by clamp(gaps[b], 0, max_gap) samples of silence at the output rate, in the output format's own code for a zero
    sample (0.0, 0, mu-law 0xFF, A-law 0xD5); None = no gaps, the wrapped entry itself.  -> (packed, offsets): offsets[b] =
    sum_{i < b} (m_i + g_i), the speech of row b at packed[offsets[b] : offsets[b + 1] - g_b], byte for byte what the wrapped entry
    writes.  `out` (1-D, of the format's dtype) bounds what is written: nothing at or past min(offsets[B], out.numel()); by
    default it holds every row at capacity and `max_gap` samples behind each.  No host read; with a rate the first call for a
    (rate, device) designs and uploads the table, which therefore must not happen under stream capture."""
    return _wave_pack("st2_wave_pack_gaps", wave, frames, rate, fmt, trim, out, offsets, samples_per_frame,
                      plain="fmt must be one of %s without a rate, got %r", gaps=gaps, max_gap=int(max_gap))


def wave_pack_level(wave, frames, level, gaps=None, max_gap=0, rate=None, fmt="s16", trim=0, out=None, offsets=None,
                    samples_per_frame=600):
    """`st2_wave_pack_level`: `wave_pack_gaps` whose moves multiply every valid sample of row b by level[b, 2], the gain
    `wave_level` wrote there -- one fp32 multiply as the sample is loaded, so the packed output is what `wave_pack_gaps` gives
    for the input fl32(x * g_b).  level fp32 [B, 4] on the device; None = no gain, `wave_pack_gaps` itself (NaN payloads of the
    fp32 copy included).  Every other argument, the return value and the no-host-read rule as `wave_pack_gaps`."""
    return _wave_pack("st2_wave_pack_level", wave, frames, rate, fmt, trim, out, offsets, samples_per_frame,
                      plain="fmt must be one of %s without a rate, got %r", gaps=gaps, max_gap=int(max_gap), level=(level,))


def wave_level_workspace_bytes(B, T_cap, samples_per_frame=600, sample_rate=24000):
    """`st2_wave_level_ex_workspace_bytes`: what `wave_level(workspace=)` needs, in bytes, with or without `true_peak` / `starts`
    (the true-peak launch writes into the hops' peak slots: the size is `st2_wave_level_workspace_bytes`')."""
    return int(_lib.load().st2_wave_level_ex_workspace_bytes(int(B), int(T_cap), int(samples_per_frame), int(sample_rate)))


def wave_level(wave, frames, target, ceiling=1.0, max_gain_db=20.0, trim=0, samples_per_frame=600, sample_rate=24000, out=None,
               workspace=None, true_peak=None, starts=None):
    """`st2_wave_level`: wave [B, 1, L] or [B, L] at `sample_rate` (L a multiple of `samples_per_frame`: the batch's frame
    capacity), frames int32 [B] on the device, target fp32 [B] on the device (LUFS; NaN = leave the row alone) -> level fp32
    [B, 4] on the device: every row's integrated loudness (ITU-R BS.1770-4, K-weighted and gated; -inf when no block passes the
    gates), its sample peak, the linear gain min(10^((target - L) / 20), 10^(max_gain_db / 20), ceiling / peak) (exactly 1 for a
    NaN target, L = -inf or peak = 0) and the number of gating blocks that passed, measured on the row's first max(0,
    samples_per_frame * frames[b] - trim) samples.  `ceiling` is linear, in (0, 1]; `max_gain_db` in [0, 60].  `out`: a contiguous
    fp32 tensor of 4 B entries to write into; `workspace`: a uint8 device tensor of `wave_level_workspace_bytes` bytes (by
    default allocated here, from the caching allocator).  No host read; legal under stream capture.
    With `true_peak` or `starts` the call is `st2_wave_level_ex`.  `true_peak`: (U, K, taps fp32 [U, K] on the device), what
    `resample.true_peak_table` returns -- the peak the ceiling acts on, and level[b, 1], is the larger of the sample peak and
    the peak of the row interpolated U times (BS.1770-4 Annex 2), one launch more.  `starts`: int32 [B] on the device, 1 where
    a passage begins (row 0 begins one whatever its flag) -- the rows of a passage are measured as one programme and get one
    gain: the same four values in every row of it."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf = int(samples_per_frame)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    _chk_dev(target, "target", torch.float32, 1)
    if target.numel() != B or target.device != wave.device:
        raise _lib.St2Error("target must hold %d values on the device of wave" % B)
    if out is None:
        out = torch.empty((B, 4), device=wave.device, dtype=torch.float32)
    _chk_level(out, B, wave)
    need = wave_level_workspace_bytes(B, L // spf, spf, sample_rate)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    args = (wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), int(sample_rate), target.data_ptr(), float(ceiling),
            float(max_gain_db), out.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream())
    if true_peak is None and starts is None:
        _lib.check(_lib.load().st2_wave_level(*args), "st2_wave_level")
        return out
    U, K, taps = (0, 0, None) if true_peak is None else true_peak
    if taps is not None:
        _chk_dev(taps, "true_peak taps", torch.float32, 2)
        if tuple(taps.shape) != (int(U), int(K)) or taps.device != wave.device:
            raise _lib.St2Error("true_peak must be (U, K, taps [U, K] on the device of wave), got (%r, %r, %s on %s)"
                                % (U, K, tuple(taps.shape), taps.device))
    sp = _chk_len(starts, "starts", B, wave)
    _lib.check(_lib.load().st2_wave_level_ex(*args, _ptr(taps), int(U), int(K), sp), "st2_wave_level_ex")
    return out


LIMIT_TILE = 2048  # st2_wave_limit_tile(): the samples of a tile of the limiter's launches (tests place events at its edges)


def wave_limit_workspace_bytes(B, T_cap, samples_per_frame=600):
    """`st2_wave_limit_workspace_bytes`: what `wave_limit(workspace=)` needs, in bytes.  The workspace begins with the required
    gain r as fp32 [B, samples_per_frame * T_cap]."""
    return int(_lib.load().st2_wave_limit_workspace_bytes(int(B), int(T_cap), int(samples_per_frame)))


def wave_limit(wave, frames, level, target, win, ceiling=1.0, max_gain_db=20.0, drive_db=6.0, trim=0, samples_per_frame=600,
               out=None, limit=None, workspace=None, true_peak=None, starts=None):
    """`st2_wave_limit`: the look-ahead peak limiter behind `wave_level`.  wave, frames, target, ceiling,
    max_gain_db, trim, samples_per_frame, true_peak and starts as `wave_level` got them, `level` the fp32 [B, 4] table it wrote,
    `win` fp32 [2 W + 1] on the device (`resample.limit_window`; W is read from its length), `drive_db` in [0, 24] -> (out, limit):
    `out` fp32 with the shape and strides of wave as [B, L] -- every valid sample times the row's drive gain g' = min(target gain,
    max gain, 10^(drive_db / 20) ceiling / peak) and times q, the smoothed sliding minimum of the gain the sample's neighbourhood
    of 2 W samples either side needs to stay at or under the ceiling; samples at or past a row's end are not written -- and `limit`
    fp32 [B, 2] = {g', min q} per row.  A row whose target is NaN, whose loudness is -inf or whose peak is 0 is copied bit for
    bit, {1, 1}.  `workspace`: a uint8 device tensor of `wave_limit_workspace_bytes` bytes (by default from the caching
    allocator).  No host read; legal under stream capture."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf = int(samples_per_frame)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    _chk_dev(target, "target", torch.float32, 1)
    _chk_dev(win, "win", torch.float32, 1)
    _chk_level(level, B, wave)
    if target.numel() != B or target.device != wave.device or win.device != wave.device or win.numel() % 2 == 0:
        raise _lib.St2Error("target must hold %d values and win 2 W + 1, both on the device of wave" % B)
    if out is None:
        out = torch.empty_strided((B, L), (wave.stride(0), 1), device=wave.device, dtype=torch.float32)
    _chk(out, "out", 2)
    if tuple(out.shape) != (B, L) or out.device != wave.device or (B > 1 and out.stride(0) != wave.stride(0)):
        raise _lib.St2Error("out must be [%d, %d] with the row stride of wave, on its device (got %s)" % (B, L, tuple(out.shape)))
    if limit is None:
        limit = torch.empty((B, 2), device=wave.device, dtype=torch.float32)
    _chk_dev(limit, "limit", torch.float32, limit.dim() if torch.is_tensor(limit) else 2)
    if limit.numel() != 2 * B or limit.device != wave.device:
        raise _lib.St2Error("limit must hold [%d, 2] values on the device of wave" % B)
    need = wave_limit_workspace_bytes(B, L // spf, spf)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    U, K, taps = (0, 0, None) if true_peak is None else true_peak
    if taps is not None:
        _chk_dev(taps, "true_peak taps", torch.float32, 2)
        if tuple(taps.shape) != (int(U), int(K)) or taps.device != wave.device:
            raise _lib.St2Error("true_peak must be (U, K, taps [U, K] on the device of wave), got (%r, %r, %s on %s)"
                                % (U, K, tuple(taps.shape), taps.device))
    sp = _chk_len(starts, "starts", B, wave)
    _lib.check(_lib.load().st2_wave_limit(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), target.data_ptr(),
                                          float(ceiling), float(max_gain_db), level.data_ptr(), _ptr(taps), int(U), int(K), sp,
                                          float(drive_db), win.numel() // 2, win.data_ptr(), out.data_ptr(), limit.data_ptr(),
                                          workspace.data_ptr(), workspace.numel(), _stream()), "st2_wave_limit")
    return out, limit


EDGES_TILE = 2048  # st2_wave_edges_tile(): the samples of a tile of the block sums' launch (tests place events at its edges)


def wave_edges_workspace_bytes(B, T_cap, samples_per_frame=600):
    """`st2_wave_edges_workspace_bytes`: what `wave_edges(workspace=)` needs, in bytes: the rows' 512-sample block sums."""
    return int(_lib.load().st2_wave_edges_workspace_bytes(int(B), int(T_cap), int(samples_per_frame)))


def wave_edges(wave, frames, top_db, keep, ramp=None, trim=0, samples_per_frame=600, out=None, edges=None, workspace=None):
    """`st2_wave_edges`: lead and tail silence trimmed on the device.  wave, frames, trim and
    samples_per_frame as `wave_level` takes them; top_db fp32 [B] on the device (librosa's `effects.trim` threshold in dB under
    the row's loudest frame; NaN or <= 0 = leave the row alone), keep int32 [B, 2] on the device (samples of lead and of tail to
    keep outside the detected bounds; negative = 0), `ramp` fp32 [F] on the device (`resample.edge_ramp`; F <= 4096; None = no
    fade) -> (out, edges): `out` fp32 with the shape and strides of wave as [B, L] -- row b's samples head .. head + count - 1
    moved to its front, bit for bit but for the fade: min(F, count // 2) samples times the ramp at an edge that was cut, none at
    an edge that was not; samples at or past `count` are not written -- and `edges` int32 [B, 2] = {head, count} per row.
    `workspace`: a uint8 device tensor of `wave_edges_workspace_bytes` bytes (by default from the caching allocator).  No host
    read; legal under stream capture."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf = int(samples_per_frame)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    _chk_dev(top_db, "top_db", torch.float32, 1)
    _chk_dev(keep, "keep", torch.int32, keep.dim() if torch.is_tensor(keep) else 2)
    if top_db.numel() != B or keep.numel() != 2 * B or top_db.device != wave.device or keep.device != wave.device:
        raise _lib.St2Error("top_db must hold %d values and keep [%d, 2], both on the device of wave" % (B, B))
    if ramp is not None:
        _chk_dev(ramp, "ramp", torch.float32, 1)
        if ramp.device != wave.device:
            raise _lib.St2Error("ramp must live on the device of wave")
    if out is None:
        out = torch.empty_strided((B, L), (wave.stride(0), 1), device=wave.device, dtype=torch.float32)
    _chk(out, "out", 2)
    if tuple(out.shape) != (B, L) or out.device != wave.device or (B > 1 and out.stride(0) != wave.stride(0)):
        raise _lib.St2Error("out must be [%d, %d] with the row stride of wave, on its device (got %s)" % (B, L, tuple(out.shape)))
    if edges is None:
        edges = torch.empty((B, 2), device=wave.device, dtype=torch.int32)
    _chk_edges(edges, B, wave)
    need = wave_edges_workspace_bytes(B, L // spf, spf)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    _lib.check(_lib.load().st2_wave_edges(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), top_db.data_ptr(),
                                          keep.data_ptr(), _ptr(ramp), 0 if ramp is None else ramp.numel(), out.data_ptr(),
                                          edges.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream()), "st2_wave_edges")
    return out, edges


def _chk_tok_int(t, name, B, N, like):
    """A per-token int32 table of the breaks (include/st2.h `st2_wave_breaks`): [B, N] entries, contiguous, on the device of `like`."""
    _chk_dev(t, name, torch.int32, t.dim() if torch.is_tensor(t) else 2)
    if t.numel() != B * N or t.device != like.device:
        raise _lib.St2Error("%s must hold [%d, %d] values on the device of its rows (got %s on %s)" % (name, B, N, tuple(t.shape), t.device))
    return t


def wave_breaks_workspace_bytes(B, T_cap, samples_per_frame=600, N=1):
    """`st2_wave_breaks_workspace_bytes`: what `wave_breaks(workspace=)` needs, in bytes: the rows' 64-sample block sums and their
    segment tables."""
    return int(_lib.load().st2_wave_breaks_workspace_bytes(int(B), int(T_cap), int(samples_per_frame), int(N)))


def wave_breaks(wave, frames, pos, brk, max_break, ramp=None, trim=0, samples_per_frame=600, out=None, ins=None, cuts=None,
                breaks=None, workspace=None):
    """`st2_wave_breaks`: silence spliced into rows at token spans, on the device.  wave, frames, trim and
    samples_per_frame as `wave_edges` takes them; pos int32 [B, N + 1] on the device (the tokens' boundaries in samples of this
    row: `token_marks` / `token_marks_edges` without a rate), brk int32 [B, N] on the device (samples of silence inside token n;
    <= 0 = none), `max_break` (host int: the most silence one row takes; it sizes `out` and the grids), `ramp` fp32 [F] on the
    device (`resample.edge_ramp`; None = no fade) -> (out, ins, cuts, breaks): `out` fp32 [B, L + max_break] (row stride a
    multiple of 4) -- every row cut at the quietest 128-sample window inside each named token's span, both sides faded, the
    silence between them; samples at or past the row's new count are not written --, `ins` int32 [B, N] (silence inserted per
    token, after the cap), `cuts` int32 [B, N] (the cut's place in the input row, -1 = none) and `breaks` int32 [B, 2] = {the
    row's new count, the silence inserted}.  `workspace`: a uint8 device tensor of `wave_breaks_workspace_bytes` bytes (by
    default from the caching allocator).  No host read; legal under stream capture."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf, max_break = int(samples_per_frame), int(max_break)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    if max_break < 0:
        raise _lib.St2Error("max_break must not be negative, got %d" % max_break)
    _chk_dev(brk, "brk", torch.int32, 2)
    N = brk.shape[1]
    if brk.shape[0] != B or brk.device != wave.device:
        raise _lib.St2Error("brk must be [%d, N] on the device of wave (got %s on %s)" % (B, tuple(brk.shape), brk.device))
    _chk_dev(pos, "pos", torch.int32, 2)
    if tuple(pos.shape) != (B, N + 1) or pos.device != wave.device:
        raise _lib.St2Error("pos must be [%d, %d] on the device of wave (got %s on %s)" % (B, N + 1, tuple(pos.shape), pos.device))
    if ramp is not None:
        _chk_dev(ramp, "ramp", torch.float32, 1)
        if ramp.device != wave.device:
            raise _lib.St2Error("ramp must live on the device of wave")
    room = L + max_break
    if out is None:
        out = torch.empty((B, (room + 3) // 4 * 4), device=wave.device, dtype=torch.float32)[:, :room]
    _chk(out, "out", 2)
    if tuple(out.shape) != (B, room) or out.device != wave.device:
        raise _lib.St2Error("out must be [%d, %d] on the device of wave (got %s on %s)" % (B, room, tuple(out.shape), out.device))
    ins = torch.empty((B, N), device=wave.device, dtype=torch.int32) if ins is None else ins
    cuts = torch.empty((B, N), device=wave.device, dtype=torch.int32) if cuts is None else cuts
    breaks = torch.empty((B, 2), device=wave.device, dtype=torch.int32) if breaks is None else breaks
    _chk_tok_int(ins, "ins", B, N, wave)
    _chk_tok_int(cuts, "cuts", B, N, wave)
    _chk_tok_int(breaks, "breaks", B, 2, wave)
    need = wave_breaks_workspace_bytes(B, L // spf, spf, N)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    _lib.check(_lib.load().st2_wave_breaks(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), pos.data_ptr(),
                                           brk.data_ptr(), N, max_break, _ptr(ramp), 0 if ramp is None else ramp.numel(),
                                           out.data_ptr(), out.stride(0), ins.data_ptr(), cuts.data_ptr(), breaks.data_ptr(),
                                           workspace.data_ptr(), workspace.numel(), _stream()), "st2_wave_breaks")
    return out, ins, cuts, breaks


def token_marks_breaks(pos, ins, rate=None, out=None):
    """`st2_token_marks_breaks`: the timing marks of rows that `wave_breaks` spliced silence into.  pos int32 [B, N + 1] on the
    device (what `wave_breaks` was given), ins int32 [B, N] on the device (what it inserted) -> int32 [B, N + 1]: marks[b, n] =
    ceil((pos[b, n] + sum_{m < n} ins[b, m]) U / D) at `rate` (None or 24000: U = D = 1), so token n's own break lies inside
    [marks[n], marks[n + 1]) and marks[b, N] is the row's packed sample count.  One launch, no host read."""
    from . import resample
    _chk_dev(pos, "pos", torch.int32, 2)
    B, N = pos.shape[0], pos.shape[1] - 1
    _chk_tok_int(ins, "ins", B, max(N, 0), pos)
    U, D = resample.ratio(resample.MODEL_RATE if rate is None else rate)
    if out is None:
        out = torch.empty((B, N + 1), device=pos.device, dtype=torch.int32)
    _chk_dev(out, "out", torch.int32, 2)
    if tuple(out.shape) != (B, N + 1) or out.device != pos.device:
        raise _lib.St2Error("out must be [%d, %d] on the device of pos (got %s on %s)" % (B, N + 1, tuple(out.shape), out.device))
    _lib.check(_lib.load().st2_token_marks_breaks(pos.data_ptr(), ins.data_ptr(), B, N, U, D, out.data_ptr(), _stream()),
               "st2_token_marks_breaks")
    return out


DYNAMICS_BLOCK = 64  # the grid of the compressor's detector and gain (st2_wave_breaks's blocks)
DYNAMICS_TILE = 4096  # st2_wave_dynamics_tile(): the samples of a tile of the apply launch (tests place row ends at its edges)
DYNAMICS_CHUNK = 1024  # st2_wave_dynamics_chunk(): the blocks of a chunk of the per-row launch


def wave_dynamics_workspace_bytes(B, T_cap, samples_per_frame=600):
    """`st2_wave_dynamics_workspace_bytes`: what `wave_dynamics(workspace=)` needs, in bytes.  The workspace begins with the
    gains per block `lin` as fp32 [B, Kcap], then the block sums `s` as fp32 [B, Kcap], Kcap = ceil(samples_per_frame T_cap / 64)."""
    return int(_lib.load().st2_wave_dynamics_workspace_bytes(int(B), int(T_cap), int(samples_per_frame)))


def wave_dynamics(wave, frames, params, win, *, A, rho, trim=0, samples_per_frame=600, out=None, dynamics=None, workspace=None):
    """`st2_wave_dynamics`: a speech compressor over the rows of a ragged batch, on the device.  wave, frames,
    trim and samples_per_frame as `wave_edges` takes them; params fp32 [B, 4] on the device = {threshold_db, slope = 1 - 1 / ratio,
    knee_db, makeup_db} per row (a NaN in a row = leave it alone); `A` the half window of the attack in blocks of 64 samples,
    0..64 (the library refuses another), with `win` fp32 [2 A + 1] on the device (`resample.limit_window(A, device)`; None with A = 0); `rho` the release in dB
    per block -> (out, dyn): `out` fp32 [B, L] (by default with the row stride of wave) -- every valid sample times the gain the
    contract of include/st2.h states; samples at or past a row's end are not written -- and `dyn` fp32 [B, 2] = {the deepest gain
    reduction in dB, the number of 64-sample blocks that were reduced} per row.  `workspace`: a uint8 device tensor of
    `wave_dynamics_workspace_bytes` bytes (by default from the caching allocator).  No host read; legal under stream capture."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf, A = int(samples_per_frame), int(A)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    _chk_dev(params, "params", torch.float32, 2)
    if tuple(params.shape) != (B, 4) or params.device != wave.device:
        raise _lib.St2Error("params must be [%d, 4] on the device of wave (got %s on %s)" % (B, tuple(params.shape), params.device))
    if (win is None) != (A == 0):
        raise _lib.St2Error("win must be None with A = 0 and 2 A + 1 weights otherwise")
    if win is not None:
        _chk_dev(win, "win", torch.float32, 1)
        if win.numel() != 2 * A + 1 or win.device != wave.device:
            raise _lib.St2Error("win must hold 2 A + 1 = %d weights on the device of wave (got %d on %s)" % (2 * A + 1, win.numel(), win.device))
    if out is None:
        out = torch.empty_strided((B, L), (wave.stride(0), 1), device=wave.device, dtype=torch.float32)
    _chk(out, "out", 2)
    if tuple(out.shape) != (B, L) or out.device != wave.device:
        raise _lib.St2Error("out must be [%d, %d] on the device of wave (got %s on %s)" % (B, L, tuple(out.shape), out.device))
    if dynamics is None:
        dynamics = torch.empty((B, 2), device=wave.device, dtype=torch.float32)
    _chk_dev(dynamics, "dynamics", torch.float32, dynamics.dim() if torch.is_tensor(dynamics) else 2)
    if dynamics.numel() != 2 * B or dynamics.device != wave.device:
        raise _lib.St2Error("dynamics must hold [%d, 2] values on the device of wave" % B)
    need = wave_dynamics_workspace_bytes(B, L // spf, spf)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    _lib.check(_lib.load().st2_wave_dynamics(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), params.data_ptr(), A,
                                             _ptr(win), float(rho), out.data_ptr(), out.stride(0), dynamics.data_ptr(),
                                             workspace.data_ptr(), workspace.numel(), _stream()), "st2_wave_dynamics")
    return out, dynamics


VOLUME_BLOCK = 64  # the grid of the volume envelope (st2_wave_breaks's blocks)
VOLUME_TILE = 4096  # the samples of a tile of the apply launch (tests place row ends at its edges)
VOLUME_DB = (-60.0, 20.0)  # what the kernels clamp a gain in dB to; at or under the lower end a block is silent


def wave_volume_workspace_bytes(B, T_cap, samples_per_frame=600):
    """`st2_wave_volume_workspace_bytes`: what `wave_volume(workspace=)` needs, in bytes.  The workspace begins with the gains per
    block `lin` as fp32 [B, Kcap], Kcap = ceil(samples_per_frame T_cap / 64)."""
    return int(_lib.load().st2_wave_volume_workspace_bytes(int(B), int(T_cap), int(samples_per_frame)))


def wave_volume(wave, frames, pos, db, tok_db, win, *, A, lengths=None, trim=0, samples_per_frame=600, out=None, volume=None,
                workspace=None):
    """`st2_wave_volume`: one gain in dB per row and one per token, smoothed and applied on the device.
    wave, frames, trim and samples_per_frame as `wave_edges` takes them; pos int32 [B, N + 1] on the device (the tokens'
    boundaries in samples of this row: what `wave_breaks` is given, or `token_marks_breaks` without a rate behind it); `db` fp32
    [B] and `tok_db` fp32 [B, N] on the device, either may be None (NaN = 0 dB; clamped to `VOLUME_DB`; -60 = silent); `lengths`
    int32 [B] on the device or None; `A` the half window of the ramp in blocks of 64 samples, 0..64, with `win` fp32 [2 A + 1] on
    the device (`resample.limit_window(A, device)`; None if and only if A = 0) -> (out, vol): `out` fp32 [B, L] (by default with
    the row stride of wave) -- every valid sample times the gain the contract of include/st2.h states, a stretch at 0 dB bit for
    bit; samples at or past a row's end are not written -- and `vol` fp32 [B, 2] = {the peak of the row's output, the number of
    64-sample blocks whose gain is not 1}.  `workspace`: a uint8 device tensor of `wave_volume_workspace_bytes` bytes (by default
    from the caching allocator).  No host read; legal under stream capture."""
    lp = _chk_len(frames, "frames", wave.shape[0] if torch.is_tensor(wave) and wave.dim() in (2, 3) else -1, wave)
    _chk(wave, "wave")
    if wave.dim() == 3 and wave.shape[1] == 1:
        wave = wave[:, 0]
    _chk(wave, "wave", 2)
    B, L = wave.shape
    spf, A = int(samples_per_frame), int(A)
    if spf <= 0 or L < spf or L % spf:
        raise _lib.St2Error("wave rows of %d samples are not a whole number of %d-sample frames" % (L, spf))
    _chk_dev(pos, "pos", torch.int32, 2)
    N = pos.shape[1] - 1
    if pos.shape[0] != B or N < 1 or pos.device != wave.device:
        raise _lib.St2Error("pos must be [%d, N + 1] on the device of wave (got %s on %s)" % (B, tuple(pos.shape), pos.device))
    np_ = _chk_len(lengths, "lengths", B, wave)
    for t, name, shape in ((db, "db", (B,)), (tok_db, "tok_db", (B, N))):
        if t is None:
            continue
        _chk_dev(t, name, torch.float32, len(shape))
        if tuple(t.shape) != shape or t.device != wave.device:
            raise _lib.St2Error("%s must be %s on the device of wave (got %s on %s)" % (name, list(shape), tuple(t.shape), t.device))
    if (win is None) != (A == 0):
        raise _lib.St2Error("win must be None with A = 0 and 2 A + 1 weights otherwise")
    if win is not None:
        _chk_dev(win, "win", torch.float32, 1)
        if win.numel() != 2 * A + 1 or win.device != wave.device:
            raise _lib.St2Error("win must hold 2 A + 1 = %d weights on the device of wave (got %d on %s)" % (2 * A + 1, win.numel(), win.device))
    if out is None:
        out = torch.empty_strided((B, L), (wave.stride(0), 1), device=wave.device, dtype=torch.float32)
    _chk(out, "out", 2)
    if tuple(out.shape) != (B, L) or out.device != wave.device:
        raise _lib.St2Error("out must be [%d, %d] on the device of wave (got %s on %s)" % (B, L, tuple(out.shape), out.device))
    if volume is None:
        volume = torch.empty((B, 2), device=wave.device, dtype=torch.float32)
    _chk_dev(volume, "volume", torch.float32, volume.dim() if torch.is_tensor(volume) else 2)
    if volume.numel() != 2 * B or volume.device != wave.device:
        raise _lib.St2Error("volume must hold [%d, 2] values on the device of wave" % B)
    need = wave_volume_workspace_bytes(B, L // spf, spf)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), device=wave.device, dtype=torch.uint8)
    _chk_dev(workspace, "workspace", torch.uint8, 1)
    _lib.check(_lib.load().st2_wave_volume(wave.data_ptr(), wave.stride(0), lp, B, L // spf, spf, int(trim), pos.data_ptr(), np_, N,
                                           _ptr(db), _ptr(tok_db), A, _ptr(win), out.data_ptr(), out.stride(0), volume.data_ptr(),
                                           workspace.data_ptr(), workspace.numel(), _stream()), "st2_wave_volume")
    return out, volume


NOISE_SAMPLER, NOISE_STEP, NOISE_SINE = _lib.NOISE_SAMPLER, _lib.NOISE_STEP, _lib.NOISE_SINE  # st2.h ST2_NOISE_*


def noise_fill(seeds, out, stream0, counts=None, per_count=None, bits=False, streams=None):
    """`st2_noise_fill`: the noise of B requests from their seeds, drawn on the device.  seeds int64 [B] on
    the device; `out` [B, ...] -- or, with `streams=S`, [S, B, ...] -- float32 (int32 with `bits`) on the same device, every
    row's trailing axes dense: row b (of noise stream `stream0`, or `stream0 + s` for out[s]) receives the values 0 .. n - 1 of
    that stream under seeds[b], n the row's element count.  Rows may be strided views (padding between them is not touched).
    `counts` (int32 [B] on the device) with `per_count`: row b receives its first min(n, counts[b] * per_count) values only
    and keeps the rest as it is.  `bits`: the raw 32-bit Philox words instead of normals.  Equal seeds give equal rows, bit for
    bit, whatever B and wherever the row lies.  One launch, no host read; legal under stream capture.  Returns `out`."""
    _chk_dev(seeds, "seeds", torch.int64, 1)
    B = seeds.numel()
    lp = _chk_len(counts, "counts", B, seeds)
    if (counts is None) != (per_count is None):
        raise _lib.St2Error("counts and per_count go together")
    _chk_on_dev(out, "out")
    want = torch.int32 if bits else torch.float32
    lead = 1 if streams is None else 2
    if out.dtype != want or out.device != seeds.device or out.dim() < lead or out.shape[lead - 1] != B or (
            streams is not None and out.shape[0] != int(streams)):
        raise _lib.St2Error("out must be a %s tensor of shape %s on the device of seeds (got %s %s on %s)" % (
            want, ("[%d, ...]" % B) if streams is None else "[%d, %d, ...]" % (int(streams), B), out.dtype, tuple(out.shape), out.device))
    n = 1
    for d in range(out.dim() - 1, lead - 1, -1):  # the trailing axes of a row are dense, in order
        if out.shape[d] != 1 and out.stride(d) != n:
            raise _lib.St2Error("out: the axes behind the batch axis must be dense (shape %s, strides %s)" % (
                tuple(out.shape), tuple(out.stride())))
        n *= out.shape[d]
    S = 1 if streams is None else int(streams)
    if S == 0 or n == 0:
        return out
    _lib.check(_lib.load().st2_noise_fill(seeds.data_ptr(), B, int(stream0), S, _lib.NOISE_BITS if bits else _lib.NOISE_NORMAL,
                                          out.data_ptr(), out.stride(0) if streams is not None else 0, out.stride(lead - 1), n, lp,
                                          0 if per_count is None else int(per_count), _stream()), "st2_noise_fill")
    return out


FIT_OK, FIT_NEAREST, FIT_NOTHING_FREE, FIT_REFUSED = range(4)  # the flag column of st2_durations_fit's report (st2.h)


def durations_fit(dur, target, T_cap, lengths=None, hold=None, out=None, report=None):
    """`st2_durations_fit`: every row of the integer durations rewritten to a stated total of frames (the
    value definition is include/st2.h's).  dur int64 [B, N] on the device, N <= 512; target int32 [B] on the device (<= 0
    leaves the row alone); `lengths` int32 [B] on the device or None (= N); `hold` bool / uint8 [B, N] on the device or None:
    non-zero = the token keeps its duration; `out` int64 [B, N], None = a new tensor, `dur` itself = in place; `report` int32
    [B, 4], None = a new tensor: {S, T', flag, tokens changed} per row.  One launch, no host read; legal under stream
    capture.  Returns (out, report)."""
    _chk_dev(dur, "dur", torch.int64, 2)
    B, N = dur.shape
    lp = _chk_len(lengths, "lengths", B, dur)
    tp = _chk_len(target, "target", B, dur)
    if target is None:
        raise _lib.St2Error("target must be an int32 tensor of %d entries (got None)" % B)
    hp = 0
    if hold is not None:
        _chk_on_dev(hold, "hold")
        if hold.dtype not in (torch.bool, torch.uint8) or tuple(hold.shape) != (B, N) or not hold.is_contiguous() \
                or hold.device != dur.device:
            raise _lib.St2Error("hold must be a contiguous bool / uint8 [%d, %d] tensor on the device of dur (got %s %s on %s)" % (
                B, N, hold.dtype, tuple(hold.shape), hold.device))
        hp = hold.data_ptr()
    if out is None:
        out = torch.empty_like(dur)
    _chk_dev(out, "out", torch.int64, 2)
    if report is None:
        report = torch.empty((B, 4), device=dur.device, dtype=torch.int32)
    _chk_dev(report, "report", torch.int32, 2)
    if out.shape != dur.shape or out.device != dur.device or tuple(report.shape) != (B, 4) or report.device != dur.device:
        raise _lib.St2Error("out must be [%d, %d] and report [%d, 4] on the device of dur (got %s on %s, %s on %s)" % (
            B, N, B, tuple(out.shape), out.device, tuple(report.shape), report.device))
    _lib.check(_lib.load().st2_durations_fit(dur.data_ptr(), B, N, lp, tp, hp, int(T_cap), out.data_ptr(), report.data_ptr(),
                                             _stream()), "st2_durations_fit")
    return out, report


def clip_ingest(src, n, rate, fmt, top_db=30.0, L_cap=None, L_min=0, out=None, want_start=True, want_flags=True):
    """`st2_clip_ingest`: reference clips in a client's rate and sample format -> trimmed fp32 rows at 24 kHz.  src [B, N_cap]
    on the device, of the dtype of `fmt` ("f32" float32, "s16" int16, "ulaw" / "alaw" uint8), n int32 [B] on the device (row
    b's sample count, clamped to 0..N_cap; nothing of src at or past it is read), `rate` one of `resample.RATES` ->
    (wave fp32 [B, >= L_cap], len int32 [B], start int32 [B], flags int32 [B]), all on the device: row b decoded, resampled by
    the polyphase table of `resample.design_input`, cut to librosa's `effects.trim(top_db=)` bounds (top_db <= 0: not cut) and
    widened to L_min samples where the clip has them; wave[b, :len[b]] holds it and nothing at or past len[b] is written.
    flags bit 0: the row was truncated to L_cap (default: ceil(N_cap U / D), what any row can need); bit 1: the minimum-length
    rule moved a bound or the row is still shorter than L_min.  `out`: fp32 [B, w] with w >= L_cap a multiple of 4, 16-byte
    aligned.  No host read; the first call for a (rate, device) designs and uploads the table, which therefore must not happen
    under stream capture."""
    from . import resample
    code, dtype = _pcm_format(fmt, rate)
    lp = _chk_len(n, "n", _nb(src, 2), src)
    _chk_on_dev(src, "src")
    if src.dtype != dtype or src.dim() != 2 or (src.shape[1] > 1 and src.stride(1) != 1):
        raise _lib.St2Error("src must be a 2-D %s tensor with unit stride along its rows for fmt %r (got %s %s)"
                            % (dtype, fmt, src.dtype, tuple(src.shape)))
    B, N_cap = src.shape
    lib = _lib.load()
    U, D, K, taps = resample.input_table(rate, src.device)
    if L_cap is None:
        L_cap = resample.output_samples(N_cap, U, D)
    L_cap = int(L_cap)
    if out is None:
        out = torch.empty((B, (L_cap + 3) // 4 * 4), device=src.device, dtype=torch.float32)
    _chk_dev(out, "out", torch.float32, 2)
    if out.shape[0] != B or out.device != src.device:
        raise _lib.St2Error("out must hold %d rows on the device of src (got %s on %s)" % (B, tuple(out.shape), out.device))
    i32 = lambda: torch.empty((B,), device=src.device, dtype=torch.int32)
    length, start, flags = i32(), i32() if want_start else None, i32() if want_flags else None
    nbytes = max(lib.st2_clip_ingest_work_bytes(B, L_cap), 16)
    work = torch.empty((nbytes,), device=src.device, dtype=torch.uint8)
    _lib.check(lib.st2_clip_ingest(src.data_ptr(), src.stride(0), lp, B, N_cap, code, U, D, taps.data_ptr(), K, float(top_db),
                                   int(L_min), out.data_ptr(), out.stride(0), L_cap, length.data_ptr(), _ptr(start), _ptr(flags),
                                   work.data_ptr(), nbytes, _stream()), "st2_clip_ingest")
    return out, length, start, flags


# ---- reference-audio style path (st2_style.hip) ----------------------------------------------------------------------
def stft_frames(wave, n_win, hop, shift, lengths=None, min_length=None, want_frames=False):
    """`st2_stft_frames`: wave [B, L] -> frames [B, n_win, L // hop + 1] (reflect-padded frame columns of torch.stft).
    `lengths` (int32 [B] on the device, `st2_stft_frames_len`): row b is the clip of lengths[b] samples (clamped to
    [min_length, L]; min_length defaults to the shortest length whose reflection stays inside the clip) -- reflected about its
    own end, frame columns from lengths[b] // hop + 1 on exact zeros, nothing of `wave` at or past lengths[b] read.
    want_frames: also return those frame counts (int32 [B] on the device)."""
    lp = _chk_len(lengths, "lengths", _nb(wave, 2), wave)
    lib = _lib.load()
    _chk(wave, "wave", 2)
    B, L = wave.shape
    M = L // hop + 1
    fr = torch.empty((B, n_win, M), device=wave.device, dtype=torch.float32)
    if lengths is None:
        if want_frames or min_length is not None:
            raise _lib.St2Error("stft_frames: min_length / want_frames need lengths")
        _lib.check(lib.st2_stft_frames(wave.data_ptr(), wave.stride(0), B, L, n_win, hop, shift, fr.data_ptr(), fr.stride(0),
                                       fr.stride(1), _stream()), "st2_stft_frames")
        return fr
    if min_length is None:
        min_length = min(L, max(shift + 1, n_win + 1 - shift, 2))
    m_len = torch.empty((B,), device=wave.device, dtype=torch.int32) if want_frames else None
    _lib.check(lib.st2_stft_frames_len(wave.data_ptr(), wave.stride(0), B, L, n_win, hop, shift, fr.data_ptr(), fr.stride(0),
                                       fr.stride(1), lp, int(min_length), _ptr(m_len), _stream()), "st2_stft_frames_len")
    return (fr, m_len) if want_frames else fr


def power_spectrum(y):
    """`st2_power_spectrum`: y [B, 2K, M] (real rows then imaginary rows) -> [B, K, M]."""
    lib = _lib.load()
    _chk(y, "y", 3)
    B, K2, M = y.shape
    assert K2 % 2 == 0
    p = torch.empty((B, K2 // 2, M), device=y.device, dtype=torch.float32)
    _lib.check(lib.st2_power_spectrum(y.data_ptr(), y.stride(0), y.stride(1), B, K2 // 2, M, p.data_ptr(), p.stride(0),
                                      p.stride(1), _stream()), "st2_power_spectrum")
    return p


def log_norm_(x, eps, mean, std, lengths=None):
    """`st2_log_norm`: x = (log(eps + x) - mean) / std in place (x contiguous).  `lengths` (int32 [B] on the device,
    `st2_log_norm_len`; x [B, C, M]): columns of row b from lengths[b] on are written as exact 0 instead."""
    lp = _chk_len(lengths, "lengths", _nb(x), x)
    lib = _lib.load()
    _chk(x, "x")
    assert x.is_contiguous()
    if lengths is None:
        _lib.check(lib.st2_log_norm(x.data_ptr(), x.numel(), eps, mean, std, _stream()), "st2_log_norm")
        return x
    _chk(x, "x", 3)
    B, Cc, M = x.shape
    _lib.check(lib.st2_log_norm_len(x.data_ptr(), x.stride(0), x.stride(1), B, Cc, M, eps, mean, std, lp, _stream()),
               "st2_log_norm_len")
    return x


def _chk_map(t, name):
    _chk(t, name, 4)  # [B, H, C, W] view, W contiguous


def dwconv3x3s2(x, w, bias, out, lengths=None):
    """`st2_dwconv3x3s2`: x [B, H, C, W] (any strides, W contiguous), w [C, 3, 3], bias [C] -> out [B, Ho, C, Wo].  `lengths`
    (int32 [B] on the device, `st2_dwconv3x3s2_len`): the maps of item b are lengths[b] <= W wide -- zero padding at their own
    end, outputs [0, (lengths[b] + 1) // 2), `out` past them left as it was."""
    lp = _chk_len(lengths, "lengths", _nb(x, 4), x)
    lib = _lib.load()
    _chk_map(x, "x")
    _chk_map(out, "out")
    _chk(w, "w", 3)
    _chk(bias, "bias", 1)
    B, H, Cc, Wd = x.shape
    assert w.shape == (Cc, 3, 3) and w.is_contiguous()
    assert out.shape == (B, (H - 1) // 2 + 1, Cc, (Wd - 1) // 2 + 1), (out.shape, x.shape)
    args = (x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), w.data_ptr(), _ptr(bias), B, Cc, H, Wd, out.data_ptr(),
            out.stride(0), out.stride(1), out.stride(2))
    if lengths is None:
        _lib.check(lib.st2_dwconv3x3s2(*args, _stream()), "st2_dwconv3x3s2")
    else:
        _lib.check(lib.st2_dwconv3x3s2_len(*args, lp, _stream()), "st2_dwconv3x3s2_len")
    return out


def avgpool2x2(x, out, lengths=None):
    """`st2_avgpool2x2`: x [B, H, C, W] -> out [B, H/2, C, (W+1)/2] (odd widths replicate their last column).  `lengths`
    (int32 [B] on the device, `st2_avgpool2x2_len`): the maps of item b are lengths[b] <= W wide -- their own last column is
    the one replicated, outputs [0, (lengths[b] + 1) // 2), `out` past them left as it was."""
    lp = _chk_len(lengths, "lengths", _nb(x, 4), x)
    lib = _lib.load()
    _chk_map(x, "x")
    _chk_map(out, "out")
    B, H, Cc, Wd = x.shape
    assert out.shape == (B, H // 2, Cc, (Wd + 1) // 2), (out.shape, x.shape)
    args = (x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), B, Cc, H, Wd, out.data_ptr(), out.stride(0), out.stride(1),
            out.stride(2))
    if lengths is None:
        _lib.check(lib.st2_avgpool2x2(*args, _stream()), "st2_avgpool2x2")
    else:
        _lib.check(lib.st2_avgpool2x2_len(*args, lp, _stream()), "st2_avgpool2x2_len")
    return out
