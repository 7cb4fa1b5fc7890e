"""Text -> waveform inference glue: the logic that in the reference exists
only inside notebook cells (Demo/Inference_LJSpeech.ipynb:268-315, Demo/Inference_LibriTTS.ipynb:258-325),
batched over utterances and kept on the device.

Differences from the notebooks, all host-side:
  * a batch of B utterances instead of one;
  * the duration -> alignment step is an index gather (`expand_by_durations`) instead of a Python loop building a
    dense one-hot matrix followed by a matmul (`t_en @ pred_aln_trg`); the result is bit-identical because the
    matmul only ever adds zeros;
  * optional `durations=` forces the per-phoneme durations (throughput runs use 4 frames / phoneme so that
    every utterance is exactly 10 s) and removes the only data-dependent host sync.
"""
import functools
import typing

import torch

from . import _hooks, ops, resample


def _engine_path(dev, taps=None):
    """The product path: every stage one C-ABI call into its C++ launch plan (csrc/st2_engine.hip).  The per-kernel Python
    plans run only where a plan has to be stepped through: tap points (`taps`), the tests' `_hooks.override(plan="python")`
    and the CPU plan tests (host tensors; the real kernel wrappers raise on those)."""
    return dev.type == "cuda" and taps is None and _hooks.plan == "engine"


class PartitionedStreams:
    """A pair of HIP streams on complementary compute-unit masks (st2_stream_create_cu_mask, include/st2.h): `front`
    owns `front_cus` of the device's CUs (dealt out evenly over the 8 XCDs by the driver's bit numbering), `main` the
    rest.  The two-stage pipeline of `inference(front_stream=...)` then does not depend on the hardware scheduler
    interleaving two queues.  MEASURED (round 3, DESIGN.md section 3 iv): slower than scheduler-placed two-stream execution
    on every box seen -- 126 / 90 / 75 ms per bench step with 16 / 32 / 64 front CUs against 68 (and 78 single-stream): the
    front's kernels are latency-bound but wide, a small partition starves them, a large one starves the decoder.  Kept as an
    explicit option (`bench.py --schedule partitioned`) for boxes on which two queues do not overlap.  Use as

        ps = PartitionedStreams(dev, front_cus=32)
        with torch.cuda.stream(ps.main):
            wave = inference(..., front_stream=ps.front)
    """

    def __init__(self, dev, front_cus, total_cus=None):
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        dev = torch.device(dev)
        if total_cus is None:
            total_cus = torch.cuda.get_device_properties(dev).multi_processor_count
        if not 0 < front_cus < total_cus:
            raise ValueError("front_cus must be in (0, %d)" % total_cus)
        words = (total_cus + 31) // 32
        self.front_cus, self.total_cus = front_cus, total_cus
        self._handles = []
        with torch.cuda.device(dev):
            streams = []
            for lo, hi in ((0, front_cus), (front_cus, total_cus)):
                mask = (C.c_uint32 * words)()
                for b in range(lo, hi):
                    mask[b // 32] |= 1 << (b % 32)
                h = C.c_void_p()
                _lib.check(lib.st2_stream_create_cu_mask(mask, words, C.byref(h)), "st2_stream_create_cu_mask")
                self._handles.append(h)
                streams.append(torch.cuda.ExternalStream(h.value, device=dev))
        self.front, self.main = streams

    def close(self):
        from . import _lib
        lib = _lib.load()
        for h in self._handles:
            lib.st2_stream_destroy(h)
        self._handles = []


class MaskedStreams:
    """HIP streams confined to one CU mask (st2_stream_create_cu_mask): `main` and `front`, both on the SAME set of CUs --
    e.g. the device without the CUs `ops.probe_cu_health()` reports as slow.  Measured: in batch
    throughput a masked queue loses (the dispatcher still deals a masked XCD its eighth of every grid); no box has reported
    a slow CU since round 4's epilogue fix.  Use as

        rep, mask, n = ops.probe_cu_health()
        if n:
            ms = MaskedStreams(dev, mask)
            with torch.cuda.stream(ms.main):
                wave = inference(..., front_stream=ms.front)
    """

    def __init__(self, dev, mask_words, n_streams=2):
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        dev = torch.device(dev)
        self._handles, streams = [], []
        with torch.cuda.device(dev):
            for _ in range(n_streams):
                mask = (C.c_uint32 * len(mask_words))(*mask_words)
                h = C.c_void_p()
                _lib.check(lib.st2_stream_create_cu_mask(mask, len(mask_words), C.byref(h)), "st2_stream_create_cu_mask")
                self._handles.append(h)
                streams.append(torch.cuda.ExternalStream(h.value, device=dev))
        self.main, self.front = streams[0], streams[1] if n_streams > 1 else None
        self.cus = sum(bin(w).count("1") for w in mask_words)

    def close(self):
        from . import _lib
        lib = _lib.load()
        for h in self._handles:
            lib.st2_stream_destroy(h)
        self._handles = []


def _pad_mask(lengths, N):
    """utils.length_to_mask (reference utils.py:42-46: True where position >= length) at a fixed width N: a bucketed
    batch may be wider than its longest utterance."""
    return torch.arange(N).unsqueeze(0) >= lengths.reshape(-1, 1)


def expand_by_durations(x, dur, T, shift=False):
    """x [B, C, N], dur [B, N] (int64, every row sums to T) -> [B, C, T] with frame t taking the phoneme whose frames
    cover it (== x @ one_hot alignment, Demo/Inference_LJSpeech.ipynb:303-312): one `st2_expand_by_durations` launch
    (prefix sum + binary search + gather on the device) instead of the notebook's Python loop and dense matmul.
    `shift`: the HiFi-GAN flow's one-frame right shift (Demo/Inference_LibriTTS.ipynb:306-319)."""
    return ops.expand_by_durations(x, dur.contiguous(), T, shift=shift)


def predict_durations(model, d, lj_tail=False, input_lengths=None):
    """ipynb:296-301: duration LSTM -> projection -> sum of sigmoids -> round, clamp(min=1), as two launches: the
    BiLSTM (k=1 conv input projection + recurrence) and `st2_duration_head` (Linear 512->50, sigmoid sum, round,
    clamp, pad masking and the LJSpeech +5 tail in one kernel).

    `input_lengths` (host int64 [B]) for a right-padded batch: the BiLSTM runs with packed-sequence semantics (its
    reverse direction starts at each utterance's own last token), pad positions get duration 0 and the LJSpeech
    +5-frame tail lands on each utterance's own last token -- every row is then what the notebook computes for that
    utterance alone."""
    B, N = d.shape[0], d.shape[1]
    if input_lengths is not None and input_lengths.is_cuda:  # device copy of a batch known to be padded
        lens = input_lengths.to(torch.int32)
    else:
        ragged = input_lengths is not None and not bool((input_lengths == N).all())
        lens = input_lengths.to(torch.int32).to(d.device) if ragged else None
    x = model.predictor.lstm.forward_cm(d.transpose(1, 2).contiguous().float(), lens)   # [B, 512, N]
    lin = model.predictor.duration_proj.linear_layer
    return ops.duration_head(x, lin.weight.detach().float().contiguous(), lin.bias.detach().float().contiguous(),
                             lengths=lens, tail=5 if lj_tail else 0)  # LJSpeech notebook only: pred_dur[-1] += 5


class Controls:
    """Per-request controls of a batch (include/st2.h "per-request controls"): one fp32 device tensor of
    six rows of [B] -- speed, alpha, beta, t, f0_scale, n_shift -- read per row by the kernels, so that one batch and one
    recorded graph serve any mix of requests.

        speed     durations = max(1, rint(sum / speed[b]))         [0.25, 4]   absent = 1
        alpha, beta, t   row b's own style mixing weights           [0, 1]      absent = the call's scalar
        f0_scale  F0[b] *= f0_scale[b]                              [0.5, 2]    absent = 1
        n_shift   N[b] += n_shift[b]  (a log-energy: a gain)        [-2, 2]     absent = 0

    Every control is a float (the whole batch), a sequence or a tensor of B values, or left out: an absent control keeps the
    behaviour without it.  Host values are validated here (ValueError when out of range or not finite).  A tensor already on
    the device is not read: it is clamped to the same range by the kernel that reads it (NaN = absent).

    Per-token controls are a second fp32 device tensor of three rows of [B][N] -- tok_speed, tok_f0_scale,
    tok_n_shift -- made only when one of them or `N` is given:

        tok_speed     token n's rate on top of the row's: max(1, rint(sum / clamp(speed[b] * tok_speed[b][n])))   [0.25, 4]  absent = 1
        tok_f0_scale  F0 *= tok_f0_scale[b][n] over token n's frames                                              [0.5, 2]   absent = 1
        tok_n_shift   N += tok_n_shift[b][n] over token n's frames                                                [-2, 2]    absent = 0

    each a float (every token), a [B, N] array or tensor, or left out; the same validation, ABSENT and `slice` rules."""
    NAMES = ("speed", "alpha", "beta", "t", "f0_scale", "n_shift")
    TOK_NAMES = ("tok_speed", "tok_f0_scale", "tok_n_shift")
    TOK_RANGES = {"tok_speed": (0.25, 4.0), "tok_f0_scale": (0.5, 2.0), "tok_n_shift": (-2.0, 2.0)}
    TOK_ABSENT = {"tok_speed": 1.0, "tok_f0_scale": 1.0, "tok_n_shift": 0.0}
    RANGES = {"speed": (0.25, 4.0), "alpha": (0.0, 1.0), "beta": (0.0, 1.0), "t": (0.0, 1.0), "f0_scale": (0.5, 2.0),
              "n_shift": (-2.0, 2.0)}
    # what an absent row holds: the device clamp's neutral value (NaN = "the call's scalar" for the mixing weights)
    ABSENT = {"speed": 1.0, "alpha": float("nan"), "beta": float("nan"), "t": float("nan"), "f0_scale": 1.0, "n_shift": 0.0}

    def __init__(self, B, speed=None, alpha=None, beta=None, t=None, f0_scale=None, n_shift=None, device=None,
                 tok_speed=None, tok_f0_scale=None, tok_n_shift=None, N=None):
        B = int(B)
        if B <= 0:
            raise ValueError("Controls: B must be positive, got %r" % (B,))
        given = dict(speed=speed, alpha=alpha, beta=beta, t=t, f0_scale=f0_scale, n_shift=n_shift)
        tok = dict(tok_speed=tok_speed, tok_f0_scale=tok_f0_scale, tok_n_shift=tok_n_shift)
        on_dev = [v for v in list(given.values()) + list(tok.values()) if torch.is_tensor(v) and v.is_cuda]
        if device is None:
            device = on_dev[0].device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        self.B = B
        self.present = tuple(n for n in self.NAMES if given[n] is not None)
        self.buf = self._table(self.NAMES, self.RANGES, self.ABSENT, given, (B,), device)
        self.N, self.tok_present, self.tok_buf = None, (), None
        if N is None:  # the token width from the one [B, N] array given; nothing when neither a row nor N is given
            dims = [v.shape if torch.is_tensor(v) else torch.as_tensor(v).shape for v in tok.values() if v is not None]
            shapes = {d[-1] for d in dims if len(d) == 2}
            if len(shapes) == 1:
                N = shapes.pop()
            elif any(v is not None for v in tok.values()):
                raise ValueError("Controls: the per-token controls %s need N (the batch's token width) or one [B, N] array"
                                 % ([n for n in self.TOK_NAMES if tok[n] is not None],))
            else:
                return
        N = int(N)
        if N <= 0 or N > 512:
            raise ValueError("Controls: N must lie in 1..512, got %r" % (N,))
        self.tok_buf = self._table(self.TOK_NAMES, self.TOK_RANGES, self.TOK_ABSENT, tok, (B, N), device)
        self.N, self.tok_present = N, tuple(n for n in self.TOK_NAMES if tok[n] is not None)

    @staticmethod
    def _table(names, ranges, absent, given, shape, device):
        """The fp32 [len(names), *shape] device tensor of a set of controls, one row per name: the absent value where `given`
        has None, a host value validated (one value for every entry, or `shape` values) and all of them sent in ONE host ->
        device copy, a device tensor copied in behind it, unread.  The [B] rows take B values of any shape and name the
        offending ones; the [B, N] rows must have that shape."""
        flat = len(shape) == 1
        dims = "%d" % shape if flat else "[%d, %d]" % shape
        host = torch.empty((len(names),) + shape, dtype=torch.float32)
        late = []
        for i, name in enumerate(names):
            v = given[name]
            host[i] = absent[name]
            if v is None:
                continue
            on_dev = torch.is_tensor(v) and v.is_cuda  # never read: clamped where the kernels read it
            rows = v.detach() if on_dev else torch.as_tensor(v, dtype=torch.float64)
            if flat:
                rows = rows.reshape(-1)
            if not on_dev and rows.numel() == 1:
                rows = rows.reshape((1,) * len(shape)).expand(shape)
            if tuple(rows.shape) != shape and on_dev:
                raise ValueError("Controls: %s must %s, got shape %s" % (name, ("hold %s values" if flat else "be %s") % dims,
                                                                        tuple(v.shape)))
            if tuple(rows.shape) != shape:
                raise ValueError("Controls: %s must be one value or %s values, got %s"
                                 % (name, dims, rows.numel() if flat else "shape %s" % (tuple(rows.shape),)))
            if on_dev:
                late.append((i, rows))
                continue
            lo, hi = ranges[name]
            if not bool((torch.isfinite(rows) & (rows >= lo) & (rows <= hi)).all()):
                raise ValueError("Controls: %s must lie in [%g, %g]%s" % (name, lo, hi, ", got %s" % rows.tolist() if flat else ""))
            host[i] = rows.to(torch.float32)
        buf = host.to(device)  # ONE host -> device copy
        for i, rows in late:
            buf[i].copy_(rows.to(torch.float32))
        return buf

    @classmethod
    def neutral(cls, B, alpha=None, beta=None, t=None, device=None, N=None):
        """All six rows present and neutral: speed 1, f0_scale 1, n_shift 0 and the given mixing weights (None = the call's
        scalars).  Equals the call without controls bit for bit.  With `N` the three per-token rows too: 1, 1 and 0."""
        c = cls(B, speed=1.0, alpha=alpha, beta=beta, t=t, f0_scale=1.0, n_shift=0.0, device=device, N=N)
        c.present = cls.NAMES
        if N is not None:
            c.tok_present = cls.TOK_NAMES
        return c

    @property
    def device(self):
        return self.buf.device

    def row(self, name):
        """The fp32 [B] device row of a control, None when it is absent."""
        return self.buf[self.NAMES.index(name)] if name in self.present else None

    def tok_row(self, name):
        """The fp32 [B, N] device rows of a per-token control, None when it is absent."""
        return self.tok_buf[self.TOK_NAMES.index(name)] if name in self.tok_present else None

    def front_rows(self):
        """The present rows `st2_front_forward_ctl` reads (speed and the mixing weights), and under "tok_speed" the per-token
        rate of `st2_front_forward_tok`."""
        rows = {n: self.row(n) for n in ("speed", "alpha", "beta", "t") if n in self.present}
        if "tok_speed" in self.tok_present:
            rows["tok_speed"] = self.tok_row("tok_speed")
        return rows

    def slice(self, i, j):
        """Rows i .. j-1 of the batch as a Controls over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Controls)
        c.B, c.present, c.buf = j - i, self.present, self.buf[:, i:j]
        c.N, c.tok_present, c.tok_buf = self.N, self.tok_present, None if self.tok_buf is None else self.tok_buf[:, i:j]
        return c


class _LevelOptions(type):
    """`Level(B, ..., true_peak=False, scope="row", limiter=False, drive_db=6.0, window_ms=8.0)`: the options of the measurement
    and of the limiter are keyword arguments of the constructor call, judged and stored here, in front of `Level.__init__`, whose
    own parameter list is the rows' and stays as it is.  The limiter's three are instance attributes only where they differ from
    the class's defaults: a `Level` made without them is the object it always was."""

    def __call__(cls, *args, true_peak=False, scope="row", limiter=False, drive_db=6.0, window_ms=8.0, **kw):
        if scope not in Level.SCOPES:
            raise ValueError("Level: scope must be one of %s, got %r" % (list(Level.SCOPES), scope))
        drive_db, window_ms = float(drive_db), float(window_ms)
        if not 0.0 <= drive_db <= 24.0:
            raise ValueError("Level: drive_db must lie in [0, 24], got %r" % (drive_db,))
        if not 0.5 <= window_ms <= 40.0:
            raise ValueError("Level: window_ms must lie in [0.5, 40], got %r" % (window_ms,))
        self = super().__call__(*args, **kw)
        self.true_peak, self.scope = bool(true_peak), scope
        for name, value in (("limiter", bool(limiter)), ("drive_db", drive_db), ("window_ms", window_ms)):
            if value != getattr(Level, name):
                setattr(self, name, value)
        return self


class Level(metaclass=_LevelOptions):
    """Loudness normalisation of the packed hand-over (include/st2.h `st2_wave_level`): every row is
    measured on the device (ITU-R BS.1770-4 integrated loudness and sample peak, at the model rate) and packed with the gain that
    brings it to `target` LUFS -- never more than `max_gain_db`, and never so much that a sample passes `ceiling_db` dBFS.

        target       LUFS, one value or B values; None or NaN in a row = leave this row alone    [-70, 0]
        ceiling_db   dBFS of the largest sample magnitude after the gain                          [-20, 0]
        max_gain_db  the most a quiet row is raised by                                             [0, 60]
        true_peak    the ceiling holds on the true peak (BS.1770-4 Annex 2: the row interpolated 8 x, to 192 kHz) and not
                     on the sample peak, which at 24 kHz reads a crest between two samples up to 3 dB low
        scope        "row": every row on its own; "passage": the rows of a passage (`passage=`) are one programme -- their
                     gating blocks are gated together and they get ONE gain, the first row's target deciding
        limiter      a look-ahead peak limiter holds the ceiling (`ops.wave_limit`): the row's gain may pass
                     ceiling / peak by up to `drive_db`, and a zero-phase gain -- the sliding minimum of what each sample needs,
                     smoothed by a Hann window of 2 W + 1 samples -- brings the peaks back under it
        drive_db     the most the limiter ever digs, and so the most a row's gain passes ceiling / peak by     [0, 24]
        window_ms    the half window: W = round(window_ms * 24) samples.  8 ms holds for 16 ms, longer than a pitch period
                     down to 62 Hz, so that the gain does not ride a voiced waveform                        [0.5, 40]

    Kept as one fp32 [B] device row (`target`), validated on the host like `Controls`; a tensor already on the device is not
    read.  `ceiling` is `ceiling_db` as a linear factor."""

    SCOPES = ("row", "passage")
    true_peak, scope = False, "row"
    limiter, drive_db, window_ms = False, 6.0, 8.0

    @property
    def W(self):
        """The limiter's half window in samples at the model rate."""
        return int(round(self.window_ms * resample.MODEL_RATE / 1000.0))

    def __init__(self, B, target=-16.0, ceiling_db=-1.0, max_gain_db=20.0, device=None):
        B = int(B)
        if B <= 0:
            raise ValueError("Level: B must be positive, got %r" % (B,))
        ceiling_db, max_gain_db = float(ceiling_db), float(max_gain_db)
        if not -20.0 <= ceiling_db <= 0.0:
            raise ValueError("Level: ceiling_db must lie in [-20, 0], got %r" % (ceiling_db,))
        if not 0.0 <= max_gain_db <= 60.0:
            raise ValueError("Level: max_gain_db must lie in [0, 60], got %r" % (max_gain_db,))
        on_dev = torch.is_tensor(target) and target.is_cuda
        if device is None:
            device = target.device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        self.B, self.ceiling_db, self.max_gain_db = B, ceiling_db, max_gain_db
        self.ceiling = min(1.0, 10.0 ** (ceiling_db / 20.0))
        self.target = self.row(target, B).to(device)

    @staticmethod
    def row(target, B):
        """`target` as the fp32 [B] row the kernel reads: a device tensor as it is (unread), host values validated; None = NaN."""
        if torch.is_tensor(target) and target.is_cuda:
            if target.numel() != B:
                raise ValueError("Level: target must hold %d values, got shape %s" % (B, tuple(target.shape)))
            return target.detach().reshape(B).to(torch.float32)
        if target is None:
            target = float("nan")
        if isinstance(target, (list, tuple)):
            target = [float("nan") if v is None else float(v) for v in target]
        rows = torch.as_tensor(target, dtype=torch.float64).reshape(-1)
        if rows.numel() == 1:
            rows = rows.expand(B)
        if rows.numel() != B:
            raise ValueError("Level: target must be one value or %d values, got %d" % (B, rows.numel()))
        if not bool((torch.isnan(rows) | ((rows >= -70.0) & (rows <= 0.0))).all()):
            raise ValueError("Level: target must lie in [-70, 0] LUFS (None / NaN = leave the row alone), got %s" % rows.tolist())
        return rows.to(torch.float32)

    def slice(self, i, j):
        """Rows i .. j-1 as a Level over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Level)
        c.B, c.ceiling_db, c.max_gain_db, c.ceiling, c.target = j - i, self.ceiling_db, self.max_gain_db, self.ceiling, self.target[i:j]
        c.true_peak, c.scope = self.true_peak, self.scope
        c.__dict__.update({k: v for k, v in self.__dict__.items() if k in ("limiter", "drive_db", "window_ms")})
        return c

    def options(self):
        """The keyword options of this Level, as its constructor takes them (what a copy over other rows is made with)."""
        return dict(true_peak=self.true_peak, scope=self.scope, limiter=self.limiter, drive_db=self.drive_db, window_ms=self.window_ms)


class Edges:
    """Lead and tail silence trimmed from every row of the packed hand-over (include/st2.h
    `st2_wave_edges`): the speech of every row is found on the device by librosa's `effects.trim` rule -- the rule the clip
    ingest trims reference clips by -- and the row is cut to it before anything else of the hand-over runs.

        top_db    dB under the row's loudest frame below which a frame is silence, one value or B values;
                  None or NaN in a row = leave this row alone                                              (0, 120]
        lead_ms   speech onsets are soft: this much is kept in front of the first non-silent frame        [0, 500]
        tail_ms   and this much behind the last one                                                        [0, 500]
        fade_ms   a raised-cosine fade over an edge that was cut (never over one that was not); at most
                  `resample.EDGE_MAX_F` samples                                                            [0, 500]

    Kept as one fp32 [B] device row (`top_db`) and one int32 [B, 2] device table (`keep`, samples at the model rate), validated
    on the host like `Level`; a `top_db` tensor already on the device is not read.  `F` is the fade in samples."""

    def __init__(self, B, top_db=40.0, lead_ms=10.0, tail_ms=30.0, fade_ms=2.0, device=None):
        B = int(B)
        if B <= 0:
            raise ValueError("Edges: B must be positive, got %r" % (B,))
        times = {}
        for name, v in (("lead_ms", lead_ms), ("tail_ms", tail_ms), ("fade_ms", fade_ms)):
            v = float(v)
            if not 0.0 <= v <= 500.0:
                raise ValueError("Edges: %s must lie in [0, 500], got %r" % (name, v))
            times[name] = v
        F = self.samples(times["fade_ms"])
        if F > resample.EDGE_MAX_F:
            raise ValueError("Edges: fade_ms=%r is %d samples, the fade holds %d at most" % (times["fade_ms"], F, resample.EDGE_MAX_F))
        on_dev = torch.is_tensor(top_db) and top_db.is_cuda
        if device is None:
            device = top_db.device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        self.B, self.F = B, F
        self.lead_ms, self.tail_ms, self.fade_ms = times["lead_ms"], times["tail_ms"], times["fade_ms"]
        self.top_db = self.row(top_db, B).to(device)
        self.keep = torch.tensor([[self.samples(self.lead_ms), self.samples(self.tail_ms)]] * B, dtype=torch.int32).to(device)

    @staticmethod
    def samples(ms):
        """Milliseconds as samples at the model rate: `gap_samples`' rounding."""
        return int(round(float(ms) * resample.MODEL_RATE / 1000.0))

    @staticmethod
    def row(top_db, B):
        """`top_db` as the fp32 [B] row the kernel reads: a device tensor as it is (unread), host values validated; None = NaN."""
        if torch.is_tensor(top_db) and top_db.is_cuda:
            if top_db.numel() != B:
                raise ValueError("Edges: top_db must hold %d values, got shape %s" % (B, tuple(top_db.shape)))
            return top_db.detach().reshape(B).to(torch.float32)
        if top_db is None:
            top_db = float("nan")
        if isinstance(top_db, (list, tuple)):
            top_db = [float("nan") if v is None else float(v) for v in top_db]
        rows = torch.as_tensor(top_db, dtype=torch.float64).reshape(-1)
        if rows.numel() == 1:
            rows = rows.expand(B)
        if rows.numel() != B:
            raise ValueError("Edges: top_db must be one value or %d values, got %d" % (B, rows.numel()))
        if not bool((torch.isnan(rows) | ((rows > 0.0) & (rows <= 120.0))).all()):
            raise ValueError("Edges: top_db must lie in (0, 120] dB (None / NaN = leave the row alone), got %s" % rows.tolist())
        return rows.to(torch.float32)

    def slice(self, i, j):
        """Rows i .. j-1 as an Edges over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Edges)
        c.B, c.F, c.lead_ms, c.tail_ms, c.fade_ms = j - i, self.F, self.lead_ms, self.tail_ms, self.fade_ms
        c.top_db, c.keep = self.top_db[i:j], self.keep[i:j]
        return c

    def options(self):
        """The three times of this Edges, as its constructor takes them (what a copy over other rows is made with)."""
        return dict(lead_ms=self.lead_ms, tail_ms=self.tail_ms, fade_ms=self.fade_ms)


def break_samples(ms):
    """A break of `ms` milliseconds as samples at the model's 24 kHz, the rate `breaks=` counts in whatever the hand-over's:
    `gap_samples`' rounding.  A scalar gives an int, a sequence (of sequences) a list."""
    return [break_samples(v) for v in ms] if isinstance(ms, (list, tuple)) else gap_samples(ms)


class Breaks:
    """Pauses INSIDE the rows of the packed hand-over (include/st2.h `st2_wave_breaks`): SSML's
    `<break time=.../>` in the middle of a sentence.  The caller names a token per pause -- normally a space or a punctuation
    token, where the model pauses anyway --; the row is cut at the quietest place inside that token's samples, both sides of the
    cut are faded and digital silence of the stated length is spliced in, on the device, before anything else of the hand-over.

        ms / samples   the pause inside token n of row b, [B, N], in milliseconds or in samples at 24 kHz (one of the two;
                       neither = no pause yet, e.g. a graph's static table); <= 0 = none
        fade_ms        the raised-cosine fade on either side of a cut; at most `resample.EDGE_MAX_F` samples      [0, 500]
        max_ms         the most silence ONE row takes: it sizes the output and the grids; what a row asks for
                       beyond it is dropped in token order                                                         [0, 60000]

    Kept as one int32 [B, N] device table (`samples`), `max_break` (samples, a host int) and `F` (the fade in samples),
    validated on the host like `Edges`; a table already on the device is taken unread."""

    def __init__(self, B, N, ms=None, samples=None, fade_ms=2.0, max_ms=2000.0, device=None):
        B, N = int(B), int(N)
        if B <= 0 or not 1 <= N <= 512:
            raise ValueError("Breaks: B must be positive and N lie in 1..512, got B=%r, N=%r" % (B, N))
        if ms is not None and samples is not None:
            raise ValueError("Breaks: pass ms or samples, not both")
        fade_ms, max_ms = float(fade_ms), float(max_ms)
        if not 0.0 <= fade_ms <= 500.0:
            raise ValueError("Breaks: fade_ms must lie in [0, 500], got %r" % (fade_ms,))
        if not 0.0 <= max_ms <= 60000.0:
            raise ValueError("Breaks: max_ms must lie in [0, 60000], got %r" % (max_ms,))
        F = Edges.samples(fade_ms)
        if F > resample.EDGE_MAX_F:
            raise ValueError("Breaks: fade_ms=%r is %d samples, the fade holds %d at most" % (fade_ms, F, resample.EDGE_MAX_F))
        on_dev = torch.is_tensor(samples) and samples.is_cuda
        if device is None:
            device = samples.device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        self.B, self.N, self.F, self.fade_ms, self.max_ms = B, N, F, fade_ms, max_ms
        self.max_break = Edges.samples(max_ms)
        self.samples = self.table(ms, samples, B, N).to(device)

    @staticmethod
    def table(ms, samples, B, N):
        """The pauses as the int32 [B, N] table the kernel reads: a device tensor as it is (unread), host values validated."""
        if torch.is_tensor(samples) and samples.is_cuda:
            if samples.dtype != torch.int32 or tuple(samples.shape) != (B, N):
                raise ValueError("Breaks: samples on the device must be an int32 [%d, %d] tensor, got %s %s"
                                 % (B, N, samples.dtype, tuple(samples.shape)))
            return samples.detach().contiguous()
        if ms is None and samples is None:
            return torch.zeros((B, N), dtype=torch.int32)
        if ms is not None:
            t = torch.as_tensor(ms, dtype=torch.float64)
            if not bool(torch.isfinite(t).all()):
                raise ValueError("Breaks: ms must be finite")
            t = torch.round(t * (resample.MODEL_RATE / 1000.0))  # half to even, as `gap_samples`
        else:
            t = torch.as_tensor(samples)
            if t.dtype.is_floating_point:
                raise ValueError("Breaks: samples must be whole sample counts (pipeline.break_samples converts milliseconds)")
            t = t.to(torch.float64)
        if tuple(t.shape) != (B, N):
            raise ValueError("Breaks: the pauses must be [%d, %d] values, got shape %s" % (B, N, tuple(t.shape)))
        if float(t.abs().max()) >= 2.0 ** 31:
            raise ValueError("Breaks: a pause does not fit int32")
        return t.to(torch.int32)

    def slice(self, i, j):
        """Rows i .. j-1 as a Breaks over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Breaks)
        c.B, c.N, c.F, c.fade_ms, c.max_ms, c.max_break = j - i, self.N, self.F, self.fade_ms, self.max_ms, self.max_break
        c.samples = self.samples[i:j]
        return c

    def options(self):
        """The two times of this Breaks, as its constructor takes them (what a copy over other rows is made with)."""
        return dict(fade_ms=self.fade_ms, max_ms=self.max_ms)


class Dynamics:
    """A speech compressor over every row of the packed hand-over (include/st2.h `st2_wave_dynamics`):
    what a hosted TTS service offers as an SSML dynamic-range-compression effect, for callers on a phone line or in a car, where the
    quiet half of a sentence is lost.  A feed-forward compressor with a soft knee on a centred 8 ms RMS, instant attack under a
    zero-phase look-ahead and a release that is linear in dB; it runs behind `breaks` and in front of `level`, so the loudness
    target holds on the compressed programme and the limiter sees compressed peaks.

        threshold_db       the level above which the gain falls, one value or B values;
                           None or NaN in a row = leave this row alone                                       [-70, 0]
        ratio              dB of input per dB of output above the threshold; `float("inf")` = a limiter's curve  [1, inf]
        knee_db            the width of the soft knee around the threshold                                    [0, 40]
        makeup_db          a gain behind the compressor                                                       [-24, 24]
        attack_ms          the half width of the look-ahead: A = round(attack_ms * 24 / 64) blocks of 64 samples  [0, 170]
        release_db_per_s   how fast the gain comes back: rho = release_db_per_s * 64 / 24000 dB per block       [1, 2000]

    The first four are kept as one fp32 [B, 4] device table (`params` = {threshold_db, 1 - 1 / ratio, knee_db, makeup_db}),
    validated on the host like `Controls` and `Level`; a tensor already on the device is not read.  `A` and `rho` are host
    numbers."""

    RANGES = (("threshold_db", -70.0, 0.0), ("ratio", 1.0, float("inf")), ("knee_db", 0.0, 40.0), ("makeup_db", -24.0, 24.0))

    def __init__(self, B, threshold_db=-24.0, ratio=3.0, knee_db=6.0, makeup_db=0.0, attack_ms=8.0, release_db_per_s=80.0,
                 device=None):
        B = int(B)
        if B <= 0:
            raise ValueError("Dynamics: B must be positive, got %r" % (B,))
        attack_ms, release_db_per_s = float(attack_ms), float(release_db_per_s)
        if not 0.0 <= attack_ms <= 170.0:
            raise ValueError("Dynamics: attack_ms must lie in [0, 170], got %r" % (attack_ms,))
        if not 1.0 <= release_db_per_s <= 2000.0:
            raise ValueError("Dynamics: release_db_per_s must lie in [1, 2000], got %r" % (release_db_per_s,))
        given = (threshold_db, ratio, knee_db, makeup_db)
        if device is None:
            on_dev = [v for v in given if torch.is_tensor(v) and v.is_cuda]
            device = on_dev[0].device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        self.B, self.attack_ms, self.release_db_per_s = B, attack_ms, release_db_per_s
        self.params = self.table(B, *given, device=device)

    @property
    def A(self):
        """The half window of the attack in blocks of `ops.DYNAMICS_BLOCK` samples."""
        return int(round(self.attack_ms * (resample.MODEL_RATE / 1000.0) / ops.DYNAMICS_BLOCK))

    @property
    def rho(self):
        """The release in dB per block."""
        return self.release_db_per_s * ops.DYNAMICS_BLOCK / resample.MODEL_RATE

    @staticmethod
    def column(name, v, B, lo, hi):
        """One of the four settings as the fp32 [B] column of the table: a device tensor as it is (unread), host values validated;
        None = NaN where that means something (`threshold_db`).  `ratio` is stored as the slope 1 - 1 / ratio."""
        if torch.is_tensor(v) and v.is_cuda:
            if v.numel() != B:
                raise ValueError("Dynamics: %s must hold %d values, got shape %s" % (name, B, tuple(v.shape)))
            v = v.detach().reshape(B).to(torch.float32)
            return 1.0 - 1.0 / v if name == "ratio" else v
        free = name == "threshold_db"  # the one setting that may be missing in a row
        if v is None:
            if not free:
                raise ValueError("Dynamics: %s must be a number, got None" % name)
            v = float("nan")
        if isinstance(v, (list, tuple)):
            v = [float("nan") if e is None and free else e for e in v]
            if any(e is None for e in v):
                raise ValueError("Dynamics: %s must be numbers, got %r" % (name, v))
        rows = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
        if rows.numel() == 1:
            rows = rows.expand(B)
        if rows.numel() != B:
            raise ValueError("Dynamics: %s must be one value or %d values, got %d" % (name, B, rows.numel()))
        ok = (rows >= lo) & (rows <= hi)
        if free:
            ok = ok | torch.isnan(rows)
        if not bool(ok.all()):
            raise ValueError("Dynamics: %s must lie in [%g, %g]%s, got %s"
                             % (name, lo, hi, " (None / NaN = leave the row alone)" if free else "", rows.tolist()))
        if name == "ratio":
            rows = 1.0 - 1.0 / rows
        return rows.to(torch.float32)

    @staticmethod
    def table(B, threshold_db, ratio, knee_db, makeup_db, device):
        """The four settings as the fp32 [B, 4] table the kernels read, on `device`."""
        cols = [Dynamics.column(name, v, B, lo, hi).to(device)
                for (name, lo, hi), v in zip(Dynamics.RANGES, (threshold_db, ratio, knee_db, makeup_db))]
        return torch.stack(cols, dim=1).contiguous()

    def slice(self, i, j):
        """Rows i .. j-1 as a Dynamics over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Dynamics)
        c.B, c.attack_ms, c.release_db_per_s, c.params = j - i, self.attack_ms, self.release_db_per_s, self.params[i:j]
        return c

    def options(self):
        """The two times of this Dynamics, as its constructor takes them (what a copy over other rows is made with)."""
        return dict(attack_ms=self.attack_ms, release_db_per_s=self.release_db_per_s)


class Volume:
    """A request's volume (include/st2.h `st2_wave_volume`): SSML's `<prosody volume=>` and the loudness
    part of `<emphasis>` -- one gain in dB per row and one per token on top of it, applied on the device to the rows of the packed
    hand-over behind `dynamics` and in front of `level`: a compressor does not undo an emphasis, a loudness target holds on the
    programme as voiced and the limiter sees the boosted peaks.

        db        the row's gain in dB: a float, B values or a device tensor [B]; None = no table            [-60, +20]
        tok_db    token n's gain in dB on top of the row's (the sum is kept inside the same range): a float, a [B, N] array
                  or a device tensor; None = no table (with `N`: a table of zeros)                            [-60, +20]
        ramp_ms   the half width of the ramp between two gains: A = round(ramp_ms * 24 / 64) blocks of 64 samples, 0..64;
                  0 = the bare linear interpolation between block centres, 2.7 ms                              [0, 170]

    -60 dB, or `float("-inf")`, is SSML's `silent`: exact zeros.  A stretch at 0 dB keeps its bits.  Host values are validated
    here (ValueError: no NaN, inside the range); a tensor already on the device is never read: the kernel cleans it (NaN = 0 dB,
    clamped to the range).  Each table is one fp32 device tensor made by ONE host -> device copy.

    With `Level(scope="row")` a row's `db` is cancelled by the normalisation -- the level is measured behind this stage -- and the
    differences between tokens survive; with `scope="passage"` a quiet sentence stays quiet beside its neighbours."""
    RANGE = ops.VOLUME_DB

    def __init__(self, B, N=None, db=None, tok_db=None, ramp_ms=8.0, device=None):
        B, ramp_ms = int(B), float(ramp_ms)
        if B <= 0:
            raise ValueError("Volume: B must be positive, got %r" % (B,))
        if not 0.0 <= ramp_ms <= 170.0:  # NaN: refused
            raise ValueError("Volume: ramp_ms must lie in [0, 170], got %r" % (ramp_ms,))
        if device is None:
            on_dev = [v for v in (db, tok_db) if torch.is_tensor(v) and v.is_cuda]
            device = on_dev[0].device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        if N is None and tok_db is not None:
            shape = tuple(tok_db.shape) if torch.is_tensor(tok_db) else tuple(torch.as_tensor(tok_db).shape)
            if len(shape) != 2:
                raise ValueError("Volume: tok_db needs N (the batch's token width) or a [B, N] array")
            N = shape[1]
        if N is not None and not 0 < int(N) <= 512:
            raise ValueError("Volume: N must lie in 1..512, got %r" % (N,))
        self.B, self.N, self.ramp_ms = B, None if N is None else int(N), ramp_ms
        if not 0 <= self.A <= 64:
            raise ValueError("Volume: ramp_ms=%r is a half window of %d blocks, outside 0..64" % (ramp_ms, self.A))
        self.device = torch.empty(0, device=device).device  # with its index, as a tensor's
        self.db = self._rows("db", db, (B,), device)
        self.tok_db = None if self.N is None else self._rows("tok_db", 0.0 if tok_db is None else tok_db, (B, self.N), device)

    @property
    def A(self):
        """The half window of the ramp in blocks of `ops.VOLUME_BLOCK` samples."""
        return int(round(self.ramp_ms * (resample.MODEL_RATE / 1000.0) / ops.VOLUME_BLOCK))

    @staticmethod
    def _rows(name, v, shape, device):
        """`db` ([B]) or `tok_db` ([B, N]) as its fp32 device tensor; None stays None."""
        if v is None:
            return None
        dims = "%d" % shape if len(shape) == 1 else "[%d, %d]" % shape
        if torch.is_tensor(v) and v.is_cuda:  # never read: cleaned where the kernel reads it
            if (v.numel() != shape[0]) if len(shape) == 1 else (tuple(v.shape) != shape):
                raise ValueError("Volume: %s must hold %s values, got shape %s" % (name, dims, tuple(v.shape)))
            return v.detach().reshape(shape).to(device=device, dtype=torch.float32).contiguous()
        try:
            rows = torch.as_tensor(v, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("Volume: %s must be numbers, got %r" % (name, v)) from None
        if len(shape) == 1:
            rows = rows.reshape(-1)
        if rows.numel() == 1:
            rows = rows.reshape((1,) * len(shape)).expand(shape)
        if tuple(rows.shape) != shape:
            raise ValueError("Volume: %s must be one value or %s values, got shape %s" % (name, dims, tuple(rows.shape)))
        lo, hi = Volume.RANGE
        if not bool((((rows >= lo) & (rows <= hi)) | (rows == float("-inf"))).all()):
            raise ValueError("Volume: %s must lie in [%g, %g] dB (-inf = silent)%s" % (name, lo, hi, ", got %s" % rows.tolist()
                                                                                     if len(shape) == 1 else ""))
        return rows.to(torch.float32).contiguous().to(device)  # ONE host -> device copy

    @classmethod
    def neutral(cls, B, N=None, ramp_ms=8.0, device=None):
        """Every table present and 0 dB (with `N` the per-token one too).  Equals the call without the object bit for bit."""
        return cls(B, N=N, db=0.0, tok_db=None if N is None else 0.0, ramp_ms=ramp_ms, device=device)

    def slice(self, i, j):
        """Rows i .. j-1 as a Volume over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Volume)
        c.B, c.N, c.ramp_ms, c.device = j - i, self.N, self.ramp_ms, self.device
        c.db, c.tok_db = (None if v is None else v[i:j] for v in (self.db, self.tok_db))
        return c

    def options(self):
        """The one time of this Volume, as its constructor takes it (what a copy over other rows is made with)."""
        return dict(ramp_ms=self.ramp_ms)


# What an engine does for SSML's <emphasis level=>: (speaking rate, pitch scale, pitch range, gain in dB) on the span.  Defaults of
# taste, not measurements: `emphasis_tables(presets=)` takes a replacement.
EMPHASIS_PRESETS = {"strong": (0.90, 1.06, 1.3, 3.0), "moderate": (0.95, 1.03, 1.15, 1.5), "none": (1.0, 1.0, 1.0, 0.0),
                    "reduced": (1.05, 0.98, 0.8, -3.0)}


def emphasis_tables(B, N, spans, presets=None):
    """SSML's `<emphasis>` as the per-token tables of a batch of B rows of N tokens (host only).  `spans`:
    a list of (row, first_token, last_token, level), both tokens included, `level` one of "strong", "moderate", "none" and
    "reduced"; where spans overlap the later one wins ("none" puts its tokens back to neutral).  -> a dict of float32 [B, N] numpy
    arrays, neutral outside the spans: `tok_speed` and `tok_f0_scale` for `Controls`, `tok_range` for `Intonation`, `tok_db` for
    `Volume`.  `presets`: level -> (speed, pitch scale, range, dB) instead of `EMPHASIS_PRESETS`, whose numbers are defaults of
    taste, not measurements -- a voice may want others."""
    import numpy as np
    presets = EMPHASIS_PRESETS if presets is None else presets
    B, N = int(B), int(N)
    if B <= 0 or N <= 0:
        raise ValueError("emphasis_tables: B and N must be positive, got %r and %r" % (B, N))
    names = ("tok_speed", "tok_f0_scale", "tok_range", "tok_db")
    out = {name: np.full((B, N), neutral, dtype=np.float32) for name, neutral in zip(names, (1.0, 1.0, 1.0, 0.0))}
    for span in spans:
        if not isinstance(span, (list, tuple)) or len(span) != 4:
            raise ValueError("emphasis_tables: a span is (row, first_token, last_token, level), got %r" % (span,))
        b, first, last, level = span
        if level not in presets:
            raise ValueError("emphasis_tables: level must be one of %s, got %r" % (sorted(presets), level))
        b, first, last = int(b), int(first), int(last)
        if not (0 <= b < B and 0 <= first <= last < N):
            raise ValueError("emphasis_tables: span %r lies outside %d rows of %d tokens" % (span, B, N))
        values = presets[level]
        if len(values) != 4:
            raise ValueError("emphasis_tables: a preset is (speed, pitch scale, range, dB), got %r" % (values,))
        for name, v in zip(names, values):
            out[name][b, first:last + 1] = v
    return out


class Intonation:
    """A request's intonation (include/st2.h `st2_pitch_shape`): SSML's `<prosody range= contour=>`, applied
    on the device to the prosody predictor's F0 curve around every row's own voiced mean, in front of the flat pitch scales of
    `Controls`.

        range      how far the voice moves around its mean: 0 = monotone, 1 = as predicted, 2 = twice as lively;
                   a float, B values or a device tensor [B]                                                       [0, 4]
        contour    a glide over the sentence: per row at most `K` (position, semitones) pairs, the position a share of the row's
                   own frames -- a list of B such lists, ONE list of pairs for every row, or a device tensor [B, K, 2];
                   linear between the points, flat outside them, two points at one position are a step      [0, 1] x [-24, 24]
        tok_range  token n's range on top of the row's (the product is capped at 4): a float, a [B, N] array or a device
                   tensor                                                                                          [0, 4]

    Host values are validated here (ValueError: finite, in range, positions ascending); a tensor already on the device is never
    read: the kernel clamps it (NaN = absent, a point with a NaN is unused).  Each table is one fp32 device tensor made by ONE host
    -> device copy; rows with fewer than `K` points are padded with NaN.  `voiced_hz` is the voiced rule's threshold (the
    harmonic source's 10 Hz).  The F0 curve is kept inside [LO_HZ, HI_HZ]."""
    RANGE = (0.0, 4.0)
    SEMITONES = (-24.0, 24.0)
    LO_HZ, HI_HZ = 40.0, 1100.0

    def __init__(self, B, range=None, contour=None, tok_range=None, N=None, K=8, voiced_hz=10.0, device=None):
        B, K, voiced_hz = int(B), int(K), float(voiced_hz)
        if B <= 0:
            raise ValueError("Intonation: B must be positive, got %r" % (B,))
        if not 0 <= K <= ops.PITCH_POINTS:
            raise ValueError("Intonation: K must lie in 0..%d, got %r" % (ops.PITCH_POINTS, K))
        if not 0.0 < voiced_hz < self.LO_HZ:
            raise ValueError("Intonation: voiced_hz must lie in (0, %g), got %r" % (self.LO_HZ, voiced_hz))
        if device is None:
            on_dev = [v for v in (range, contour, tok_range) if torch.is_tensor(v) and v.is_cuda]
            device = on_dev[0].device if on_dev else ("cuda" if torch.cuda.is_available() else "cpu")
        if N is None and tok_range is not None:
            shape = tuple(tok_range.shape) if torch.is_tensor(tok_range) else tuple(torch.as_tensor(tok_range).shape)
            if len(shape) != 2:
                raise ValueError("Intonation: tok_range needs N (the batch's token width) or a [B, N] array")
            N = shape[1]
        if N is not None and not 0 < int(N) <= 512:
            raise ValueError("Intonation: N must lie in 1..512, got %r" % (N,))
        self.B, self.K, self.voiced_hz, self.N = B, K, voiced_hz, None if N is None else int(N)
        self.device = torch.empty(0, device=device).device  # with its index, as a tensor's
        self.range = self._rows("range", range, (B,), device)
        self.tok_range = None if self.N is None else self._rows("tok_range", 1.0 if tok_range is None else tok_range, (B, self.N), device)
        self.contour = self._points(contour, B, K, device)

    @staticmethod
    def _rows(name, v, shape, device):
        """`range` ([B]) or `tok_range` ([B, N]) as its fp32 device tensor; None stays None."""
        if v is None:
            return None
        dims = "%d" % shape if len(shape) == 1 else "[%d, %d]" % shape
        if torch.is_tensor(v) and v.is_cuda:  # never read: clamped where the kernel reads it
            if (v.numel() != shape[0]) if len(shape) == 1 else (tuple(v.shape) != shape):
                raise ValueError("Intonation: %s must hold %s values, got shape %s" % (name, dims, tuple(v.shape)))
            return v.detach().reshape(shape).to(device=device, dtype=torch.float32).contiguous()
        rows = torch.as_tensor(v, dtype=torch.float64)
        if len(shape) == 1:
            rows = rows.reshape(-1)
        if rows.numel() == 1:
            rows = rows.reshape((1,) * len(shape)).expand(shape)
        if tuple(rows.shape) != shape:
            raise ValueError("Intonation: %s must be one value or %s values, got shape %s" % (name, dims, tuple(rows.shape)))
        lo, hi = Intonation.RANGE
        if not bool((torch.isfinite(rows) & (rows >= lo) & (rows <= hi)).all()):
            raise ValueError("Intonation: %s must lie in [%g, %g]%s" % (name, lo, hi, ", got %s" % rows.tolist() if len(shape) == 1 else ""))
        return rows.to(torch.float32).contiguous().to(device)  # ONE host -> device copy

    @staticmethod
    def _points(contour, B, K, device):
        """`contour` as its fp32 [B, K, 2] device tensor, short rows padded with NaN; None stays None."""
        if contour is None:
            return None
        if torch.is_tensor(contour) and contour.is_cuda:  # never read
            if tuple(contour.shape) != (B, K, 2):
                raise ValueError("Intonation: contour must be [%d, %d, 2], got shape %s" % (B, K, tuple(contour.shape)))
            return contour.detach().to(device=device, dtype=torch.float32).contiguous()
        rows = contour.tolist() if torch.is_tensor(contour) else list(contour)
        pair = lambda e: isinstance(e, (list, tuple)) and len(e) == 2 and not any(isinstance(x, (list, tuple)) for x in e)
        if all(pair(e) for e in rows):
            rows = [rows] * B  # one list of points for every row
        if len(rows) != B:
            raise ValueError("Intonation: contour must be one list of (position, semitones) pairs or %d of them, got %d" % (B, len(rows)))
        host = torch.full((B, K, 2), float("nan"), dtype=torch.float32)
        (s_lo, s_hi) = Intonation.SEMITONES
        for b, pts in enumerate(rows):
            pts = [] if pts is None else list(pts)
            if len(pts) > K:
                raise ValueError("Intonation: contour row %d has %d points, at most K = %d fit" % (b, len(pts), K))
            if not all(isinstance(e, (list, tuple)) and len(e) == 2 for e in pts):
                raise ValueError("Intonation: contour row %d must be (position, semitones) pairs, got %r" % (b, pts))
            last = 0.0
            for k, (p, v) in enumerate(pts):
                p, v = float(p), float(v)
                if not (0.0 <= p <= 1.0) or not (s_lo <= v <= s_hi):
                    raise ValueError("Intonation: contour point (%r, %r) of row %d must lie in [0, 1] x [%g, %g]" % (p, v, b, s_lo, s_hi))
                if p < last:
                    raise ValueError("Intonation: contour positions of row %d must ascend, got %r" % (b, [float(e[0]) for e in pts]))
                host[b, k, 0], host[b, k, 1], last = p, v, p
        return host.to(device)  # ONE host -> device copy

    @classmethod
    def neutral(cls, B, N=None, K=8, voiced_hz=10.0, device=None):
        """Every table present and neutral: range 1, no point (all NaN), with `N` the token ranges 1.  Equals the call without the
        object bit for bit."""
        return cls(B, range=1.0, contour=[], tok_range=None if N is None else 1.0, N=N, K=K, voiced_hz=voiced_hz, device=device)

    def slice(self, i, j):
        """Rows i .. j-1 as an Intonation over the same memory (long-form: a front group's sentences)."""
        c = object.__new__(Intonation)
        c.B, c.K, c.voiced_hz, c.N, c.device = j - i, self.K, self.voiced_hz, self.N, self.device
        c.range, c.tok_range, c.contour = (None if v is None else v[i:j] for v in (self.range, self.tok_range, self.contour))
        return c


def _check_intonation(intonation, dev, B, taps, front, N):
    """What `intonation=` cannot be combined with: `_check_controls`' refusals, before anything is launched."""
    if not isinstance(intonation, Intonation):
        raise ValueError("intonation must be a pipeline.Intonation, got %s" % type(intonation).__name__)
    if front is not None:
        raise ValueError("intonation cannot be combined with front= (a GraphedFront records no prosody call); use GraphedSynthesis, "
                         "which reads the tables from static buffers")
    if _hooks.plan != "engine":
        raise ValueError("intonation needs the C++ engine plans: the per-kernel Python plans (plan='python') have no twin of the "
                         "pitch kernel")
    if dev.type != "cuda" or taps is not None:
        raise ValueError("intonation needs the C++ engine path (HIP device, no taps)")
    if intonation.B != B or intonation.device != dev:
        raise ValueError("intonation describes %d rows on %s, the batch has %d on %s" % (intonation.B, intonation.device, B, dev))
    if intonation.tok_range is not None and N is not None and intonation.N != N:
        raise ValueError("intonation holds per-token rows of %d tokens, the batch is %d wide" % (intonation.N, N))


def _pitch_shape(intonation, F0, dur, frames=None, sel=None, shift=False):
    """The rows' range and contour applied in place to the prosody call's F0 curve: one launch -> its `pitch` report [b, 4]."""
    pick = lambda v: None if v is None else v if sel is None else sel(v).contiguous()
    tok = pick(intonation.tok_range)
    return ops.pitch_shape(F0, range=pick(intonation.range), tok_range=tok, dur=None if tok is None else dur.contiguous(),
                           contour=pick(intonation.contour) if intonation.K else None, frames=frames, shift=shift,
                           voiced_hz=intonation.voiced_hz, lo_hz=Intonation.LO_HZ, hi_hz=Intonation.HI_HZ, pitch=True)


def _check_controls(controls, dev, B, taps, front, durations, N=None):
    """What `controls=` cannot be combined with: refused before anything is launched."""
    if not isinstance(controls, Controls):
        raise ValueError("controls must be a pipeline.Controls, got %s" % type(controls).__name__)
    if front is not None:
        raise ValueError("controls cannot be combined with front= (a GraphedFront bakes the settings into its graphs); use "
                         "GraphedSynthesis, which reads them from a static buffer")
    if _hooks.plan != "engine":
        raise ValueError("controls need the C++ engine plans: the per-kernel Python plans (plan='python') have no twin of the "
                         "control kernels")
    if dev.type != "cuda" or taps is not None:
        raise ValueError("controls need the C++ engine path (HIP device, no taps)")
    if controls.B != B or controls.device != dev:
        raise ValueError("controls describe %d rows on %s, the batch has %d on %s" % (controls.B, controls.device, B, dev))
    if durations is not None and "speed" in controls.present:
        raise ValueError("controls.speed with forced durations: there is nothing to scale")
    if durations is not None and "tok_speed" in controls.tok_present:
        raise ValueError("controls.tok_speed with forced durations: there is nothing to scale")
    if controls.tok_present and N is not None and controls.N != N:
        raise ValueError("controls hold per-token rows of %d tokens, the batch is %d wide" % (controls.N, N))


def _prosody_controls(controls, F0, N, dur, frames=None, sel=None, shift=False):
    """Row b's pitch scale / energy shift, then token n's over its frames, applied in place to the prosody call's curves: one
    launch each, none for a pair of which both are absent."""
    if controls is None:
        return
    per_row = lambda sc, sh: ops.prosody_controls(F0, N, sc, sh, frames=frames)
    per_token = lambda sc, sh: ops.prosody_controls_tok(F0, N, dur.contiguous(), sc, sh, frames=frames, shift=shift)
    for rows, apply in (([controls.row("f0_scale"), controls.row("n_shift")], per_row),
                        ([controls.tok_row("tok_f0_scale"), controls.tok_row("tok_n_shift")], per_token)):
        if rows[0] is None and rows[1] is None:
            continue
        if sel is not None:
            rows = [None if v is None else sel(v).contiguous() for v in rows]
        apply(*rows)


@torch.no_grad()
def _front_engine(model, dev):
    """The st2_engine handle of the front (text encoder, PL-BERT + bert_encoder, style denoiser, prosody predictor), packed
    once per (weights, device): rebuilt when a front module's parameters were reloaded (in-place version counters) or
    moved (storage addresses)."""
    from . import engine
    mods = [model.text_encoder, model.bert, model.bert_encoder, model.diffusion.diffusion.net, model.predictor]
    stamp = tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())
    dev = engine.norm_device(dev)
    cached = getattr(model.predictor, "_front_engine", None)
    if cached is None or cached[0] != stamp or not engine.same_device(cached[1], dev):
        engine.replaced(cached[1] if cached else None, "front")
        cached = (stamp, engine.build_front_engine(model, dev))
        model.predictor._front_engine = cached
    return cached[1]


def _front_core(model, sampler, tokens, lengths_host, lengths_dev, noise, step_noise, ref_s, s_prev, *, diffusion_steps,
                embedding_scale, alpha, beta, t, predict, lj_tail, carry=False, taps=None, controls=None):
    """The device-only part of the front: text encoder, PL-BERT, style diffusion, style mixing, duration encoder and
    (when `predict`) the duration head.  No host read of device data, no host -> device copy, no random draw: every
    input is a device tensor (`lengths_dev` int32 [B] for a right-padded batch, else None and `lengths_host` decides on
    the host), so the whole function is legal under stream capture (`GraphedFront`).

    `carry`: the B rows are consecutive sentences of ONE passage; row k's sampled style is mixed with row k-1's mixed style
    (`s_prev` [1, 256] or None feeds row 0) -- LFinference's loop as a row scan between the batched sampler and the batched
    duration stages (st2.h st2_front_args.carry).  `controls` (a `Controls`, engine path only): row b's own speaking rate and
    mixing weights (`st2_front_forward_ctl`)."""
    dev = tokens.device
    B, N = tokens.shape
    if _engine_path(dev, taps):  # ONE C-ABI call: st2_front_forward (csrc/st2_engine.hip front_plan)
        from .diffusion import GraphedSampler
        smp = sampler.sampler if isinstance(sampler, GraphedSampler) else sampler
        if lengths_dev is None and lengths_host is not None and not bool((lengths_host == N).all()):
            lengths_dev = lengths_host.to(torch.int32).to(dev)
        if step_noise is None:
            step_noise = torch.randn((diffusion_steps - 1, B, 1, noise.shape[-1]), device=dev, dtype=torch.float32)
        table, sigma0 = smp.step_table(diffusion_steps)
        o = _front_engine(model, dev).front_forward(tokens, noise, step_noise, table, sigma0, lengths=lengths_dev, ref_s=ref_s,
                                                    s_prev=s_prev, embedding_scale=embedding_scale, alpha=alpha, beta=beta,
                                                    t=t, predict=predict, tail=5 if lj_tail else 0, carry=carry,
                                                    controls=None if controls is None else controls.front_rows())
        return dict(t_en=o["t_en"], d=o["d_cm"].transpose(1, 2), s=o["s"], ref=o["ref"], durations=o["durations"],
                    s_mixed=o["s_pred"])  # [B, 2 sty] = (ref | s), written by the plan: no torch.cat on the product path
    if lengths_dev is not None:  # mask built on the device; the modules take the device copy (text.py _device_lengths)
        text_mask = torch.arange(N, device=dev).unsqueeze(0) >= lengths_dev.reshape(-1, 1)
        len_arg = lengths_dev
    else:
        text_mask = torch.zeros((B, N), dtype=torch.bool, device=dev)
        len_arg = lengths_host
    t_en = model.text_encoder(tokens, len_arg, text_mask)                            # [B, 512, N]
    bert_dur = model.bert(tokens, attention_mask=(~text_mask).int())                 # [B, N, 768]
    d_en = model.bert_encoder(bert_dur).transpose(-1, -2)                            # [B, 512, N]
    kw = dict(embedding=bert_dur, embedding_scale=embedding_scale, num_steps=diffusion_steps, step_noise=step_noise)
    if ref_s is not None:
        kw["features"] = ref_s
    if lengths_dev is not None:  # the denoiser attends over / averages each utterance's own tokens only
        kw["lengths"] = lengths_dev
    s_pred = sampler(noise, **kw).squeeze(1)                                          # [B, 256]
    if taps is not None:
        taps["s_pred"] = s_pred
    def mix(sp, prev, rs):
        if prev is not None:
            sp = t * prev + (1 - t) * sp  # convex combination of previous and current style
        s, ref = sp[:, 128:], sp[:, :128]
        if rs is not None:
            ref = alpha * ref + (1 - alpha) * rs[:, :128]
            s = beta * s + (1 - beta) * rs[:, 128:]
        return s, ref

    if carry and B > 1:  # row scan: sentence k mixes with sentence k-1's MIXED style
        rows, prev = [], s_prev
        for k in range(B):
            s_k, ref_k = mix(s_pred[k:k + 1], prev, None if ref_s is None else ref_s[k:k + 1])
            prev = torch.cat([ref_k, s_k], dim=-1)
            rows.append(prev)
        mixed = torch.cat(rows, dim=0)
        s, ref = mixed[:, 128:], mixed[:, :128]
    else:
        s, ref = mix(s_pred, s_prev, ref_s)
    s, ref = s.contiguous(), ref.contiguous()
    d = model.predictor.text_encoder(d_en, s, len_arg, text_mask)                    # [B, N, 640]
    dur = predict_durations(model, d, lj_tail=lj_tail, input_lengths=len_arg) if predict else None
    return dict(t_en=t_en, d=d, s=s, ref=ref, durations=dur)


def _sampler_generation(sampler):
    """Bumped by the denoiser whenever its packed weights are rebuilt: a recorded graph of an older generation is stale."""
    return getattr(sampler.diffusion.net, "_pack_gen", 0)


def _engine_changed(eng, recorded, calib_gen):
    """Is a graph recorded over engine `recorded` at calibration generation `calib_gen` stale now that the model holds `eng`?
    A rebuilt engine (reload, .to()) has other buffers; a re-calibrated one other operand scales, which are kernel arguments."""
    return eng is not recorded or eng.calib_gen != calib_gen


def _record_graph(run, dev):
    """`run` once eagerly, then captured on the current stream of `dev` -> (graph, what the captured run returned).  The eager
    run is the warm-up (weight packing, kernel attributes, the status word, the allocator) and goes onto the auxiliary stream,
    ordered behind the current one and joined again, so that the capture starts on a drained device."""
    cur = torch.cuda.current_stream(dev)
    side = ops.aux_stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()
    cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    return graph, out


def _hand_off(tensors, dst, wait=None):
    """`tensors` (None entries skipped) were allocated on one stream and will be read on the stream `dst`: `dst` is first ordered
    behind `wait` (an event, or the producing stream; None = the caller has ordered it already), then every tensor is marked
    as in use on `dst`, so that the caching allocator does not hand its memory out again while `dst` still reads it."""
    if wait is not None:
        (dst.wait_event if isinstance(wait, torch.cuda.Event) else dst.wait_stream)(wait)
    for v in tensors:
        if v is not None:
            v.record_stream(dst)


def _decoder_inputs(g):
    """What a prepared batch, or one frame-count group of it, hands to the decoder (`frames`: the ragged forms only)."""
    return g["asr"], g["F0"], g["N"], g["ref"], g.get("frames")


class GraphedFront:
    """hipGraph replay of `_front_core` (BASELINE.json configs[4]: latency-bound sentence-by-sentence synthesis).  The
    front of one sentence is ~600 launches of 5-40 us kernels issued from Python (~6 ms of host time against ~4 ms of
    device time at B = 1): the host, not the GPU, paces a passage.  One graph per signature (batch, padded tokens,
    diffusion steps, guidance scale, speaker / carry-over / padding / duration-prediction flags, mixing weights); the
    first call with a new signature runs eagerly once and records, later calls copy their inputs into static buffers,
    replay and return CLONES of the outputs (the next replay may start while the decoder still reads them).  The
    per-step diffusion noise is always an explicit input (drawn here when the caller gives none)."""

    def __init__(self, model, sampler, max_graphs=32):
        self.model = model
        from .diffusion import GraphedSampler
        # a GraphedSampler's eager sampler: one graph, not two nested (DiffusionSampler.sampler is the ADPM2 object)
        self.sampler = sampler.sampler if isinstance(sampler, GraphedSampler) else sampler
        self.max_graphs = max_graphs
        self._graphs = {}

    def _generation(self):
        return _sampler_generation(self.sampler)

    def _pack_refs(self):
        """(module, packed-weight cache) of every front module as of now.  A graph keeps these references -- the device
        memory its kernels read stays allocated -- and is stale as soon as a module holds a different cache object
        (load_state_dict / .to() / refresh() rebuild the packs)."""
        refs = []
        for key in ("text_encoder", "bert", "predictor"):
            for m in self.model[key].modules():
                pk = getattr(m, "_pk", None)
                if pk is not None:
                    refs.append((m, pk))
        return refs

    def _engine_mode(self):
        return _hooks.plan == "engine"

    def _stale(self, g, dev):
        if g["engine"] is not None or self._engine_mode():  # recorded over / now running on the C++ front: same handle?
            if not self._engine_mode():
                return True
            eng = _front_engine(self.model, dev)
            return _engine_changed(eng, g["engine"], g.get("calib_gen"))  # (a Python-front graph has neither)
        return any(getattr(m, "_pk", None) is not pk for m, pk in g["packs"])

    @torch.no_grad()
    def __call__(self, tokens, lengths_host, lengths_dev, noise, step_noise, ref_s, s_prev, **kw):
        dev = tokens.device
        B, N = tokens.shape
        steps = kw["diffusion_steps"]
        if step_noise is None:
            step_noise = torch.randn((steps - 1, B, 1, noise.shape[-1]), device=dev, dtype=torch.float32)
        key = (dev.index, B, N, steps, float(kw["embedding_scale"]), ref_s is not None, s_prev is not None,
               lengths_dev is not None, bool(kw["predict"]), bool(kw["lj_tail"]), float(kw["alpha"]), float(kw["beta"]),
               float(kw["t"]), bool(kw.get("carry", False)))
        g = self._graphs.get(key)
        if g is not None and (g["gen"] != self._generation() or self._stale(g, dev)):  # packed weights were rebuilt
            self._graphs.clear()
            g = None
        if g is None:
            if len(self._graphs) >= self.max_graphs:
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[key] = self._capture(tokens, lengths_host, lengths_dev, noise, step_noise, ref_s, s_prev, kw)
        st = g["static"]
        for name, val in (("tokens", tokens), ("lengths_dev", lengths_dev), ("noise", noise), ("step_noise", step_noise),
                          ("ref_s", ref_s), ("s_prev", s_prev)):
            if val is not None:
                st[name].copy_(val.reshape(st[name].shape))
        g["graph"].replay()
        return {k: (None if v is None else v.clone()) for k, v in g["out"].items()}

    def _capture(self, tokens, lengths_host, lengths_dev, noise, step_noise, ref_s, s_prev, kw):
        clone = lambda v: None if v is None else v.detach().clone()
        st = dict(tokens=clone(tokens), lengths_dev=clone(lengths_dev), noise=clone(noise.float()),
                  step_noise=clone(step_noise.float()), ref_s=clone(ref_s), s_prev=clone(s_prev))
        lh = None if lengths_host is None else lengths_host.clone()

        def run():
            return _front_core(self.model, self.sampler, st["tokens"], lh, st["lengths_dev"], st["noise"],
                               st["step_noise"], st["ref_s"], st["s_prev"], **kw)

        dev = tokens.device
        graph, out = _record_graph(run, dev)
        # the graph's kernels read the packed weights: keep the Python caches / the C++ engine handle they live in alive,
        # and compare identities at replay (a reload or .to() rebuilds them)
        eng = _front_engine(self.model, dev) if self._engine_mode() else None
        return dict(graph=graph, static=st, out=out, gen=self._generation(), packs=self._pack_refs(), engine=eng,
                    calib_gen=None if eng is None else eng.calib_gen)


@torch.no_grad()
def prepare(model, sampler, tokens, input_lengths=None, noise=None, diffusion_steps=5, embedding_scale=1.0,
            ref_s=None, alpha=0.3, beta=0.7, durations=None, step_noise=None, lj_tail=None, s_prev=None, t=0.7,
            taps=None, allow_ragged=False, total_frames=None, lengths_dev=None, front=None, carry=False, group_events=False,
            ragged_decode=False, max_frames=None, controls=None, fit=None, intonation=None):
    """Everything in front of the decoder: text encoder, PL-BERT, style diffusion, style mixing, duration and
    prosody prediction, alignment expansion.  Returns the decoder's inputs {asr, F0, N, ref} plus the mixed style
    vector `s_pred` [B, 256] (what LFinference hands to the next sentence) and the durations.

    `s_prev` / `t`: long-form style carry-over, `s_pred = t * s_prev + (1 - t) * s_pred` applied to the sampler output
    before the speaker mixing (Demo/Inference_LibriTTS.ipynb LFinference; the LJSpeech notebook calls the same weight
    `alpha`).

    Utterances of different total duration cannot share a decoder call (its InstanceNorm spans the utterance).  With
    `allow_ragged` the result then carries `groups`: a list of (utterance indices, {asr, F0, N, ref}) per distinct
    frame count; without it such a batch raises.

    Host <-> device traffic: none on a batch without padding and with forced `durations` that are either a host tensor
    or a device tensor accompanied by `total_frames` (int, or one int per utterance: their row sums).  A pageable
    host -> device copy blocks the host until the stream has drained, i.e. it would serialise the issue of step k+1 with
    the execution of step k; so the pad mask of an unpadded batch is created on the device, and a caller that
    synthesises batch after batch keeps its forced durations on the device.

    `front` (a `GraphedFront`): the device-only part (`_front_core`) is replayed from a hipGraph instead of being issued
    kernel by kernel.

    `carry`: the rows are consecutive sentences of one passage (`_front_core`); `s_prev` is then [1, 256] or None.
    `group_events`: every entry of `groups` also carries `ready`, an event recorded on the current stream behind that group's
    last kernel (a consumer on another stream starts on group 0 while the later groups are still being expanded).

    `ragged_decode` (with `allow_ragged`, C++ engine path): utterances of different frame counts are NOT split into groups;
    ONE ragged prosody call (`st2_prosody_forward_ragged`) returns {asr, F0, N, ref} padded to the longest utterance plus
    `frames` (int32 [B] on the device) and `frames_host` (list), which `model.decoder(..., frames=)` decodes in one call, every
    row as if alone.

    `max_frames` (int; implies `allow_ragged` and `ragged_decode`, C++ engine path, no taps): the sync-free path of DESIGN.md
    section 11.  The caller states the capacity in decoder frames; the frame counts are computed on the device
    (`ops.frames_from_durations`) and never read back, ONE ragged prosody call runs at T = max_frames, and the result carries
    `frames` (device) and no `frames_host`.  The whole call is then legal under stream capture when every input is a device
    tensor; a caller that passes `lengths_dev` gets the padded-batch semantics from it alone (`input_lengths` is not looked
    at: a captured call serves other lengths at replay).  A row whose durations sum to more than `max_frames` is synthesised
    truncated to it and raises ST2_STATUS_FRAME_CAPACITY (a warning at the next `ops.check_status()`).  The result also carries
    `token_lengths`: the device token counts the durations were predicted under (None for forced durations, whose rows count
    whole), which `ops.token_marks` takes as its `lengths`.  Forced `durations`
    take the same route (their rows are summed whole, pad tokens included, as on the other paths).  `allow_ragged` and
    `ragged_decode` are implied whatever the caller passed; `total_frames` and `group_events` are refused.

    `controls` (a `Controls`; C++ engine path, no taps, no `front=`): per-row speaking rate, style mixing weights, pitch scale
    and energy shift.  Rate and weights are read by the front (`st2_front_forward_ctl`: the mixing is
    then one launch), pitch and energy are applied to F0 / N right behind every prosody call (`ops.prosody_controls`).  Nothing
    of it is read on the host; None takes the code paths without it.  Its per-token rows go the same two
    ways: the rate through `st2_front_forward_tok`, pitch and energy through `ops.prosody_controls_tok` right behind
    `ops.prosody_controls`.

    `fit` (with `max_frames`): (targets int32 [B] on the device, hold bool / uint8 [B, N] on the device or
    None) -- the durations, predicted or forced, are rewritten to the targets by ONE launch (`ops.durations_fit`) right in front
    of `ops.frames_from_durations`; the fitted tensor is what the frame counts, the prosody call, the controls' per-token spans
    and the result's `durations` see, and the result carries the launch's report as `fit` (int32 [B, 4], device).

    `intonation` (an `Intonation`; C++ engine path, no taps, no `front=`): per-row pitch range, per-token
    range and contour, applied to F0 by ONE launch (`ops.pitch_shape`) right behind every prosody call and in front of the
    controls' flat pitch scales: the model's own curve is shaped first.  The result carries the launch's report as `pitch` (fp32
    [B, 4], device: {voiced mean in Hz, voiced columns, lowest, highest F0}), a tensor of its own.  Nothing of it is read on the
    host; None takes the code paths without it.  A batch split into `groups` carries each group's report in the group."""
    dev = tokens.device
    B, N = tokens.shape
    if max_frames is None:
        _capacity_only("fit_frames / fit_hold", fit)
    if controls is not None:
        _check_controls(controls, dev, B, taps, front, durations, N)
    if intonation is not None:
        _check_intonation(intonation, dev, B, taps, front, N)
    if max_frames is not None:
        if int(max_frames) <= 0:
            raise ValueError("max_frames must be a positive frame count, got %r" % (max_frames,))
        if not _engine_path(dev, taps):
            raise ValueError("max_frames needs the C++ engine path (HIP device, plan_mode 'engine', no taps)")
        if total_frames is not None or group_events:
            raise ValueError("max_frames: `total_frames` / `group_events` have no meaning on the capacity-bound path (the frame "
                             "counts are computed on the device; there are no per-frame-count groups)")
    ops.check_status() if dev.type == "cuda" else None  # device-side conditions raised by the previous call's kernels
    if max_frames is not None and lengths_dev is not None:
        ragged_n, input_lengths = True, None  # the device lengths are the truth: nothing on the host decides (stream capture)
    else:
        if input_lengths is None:
            input_lengths = torch.full((B,), N, dtype=torch.long)
        input_lengths = input_lengths.detach().cpu().long()
        ragged_n = not bool((input_lengths == N).all())
    if ragged_n and lengths_dev is None:  # ONE host -> device copy of the lengths (none if the caller prepared it)
        lengths_dev = input_lengths.to(torch.int32).to(dev)
    if not ragged_n:
        lengths_dev = None
    multispeaker = ref_s is not None
    hifigan = model.decoder.kind == "hifigan"
    if lj_tail is None:
        lj_tail = not multispeaker
    if noise is None:
        noise = torch.randn(B, 1, 256, device=dev)
    ckw = dict(diffusion_steps=diffusion_steps, embedding_scale=embedding_scale, alpha=alpha, beta=beta, t=t,
               predict=durations is None, lj_tail=lj_tail, carry=bool(carry))
    if front is not None and dev.type == "cuda" and taps is None:
        f = front(tokens, input_lengths, lengths_dev, noise, step_noise, ref_s, s_prev, **ckw)
    else:
        f = _front_core(model, sampler, tokens, input_lengths, lengths_dev, noise, step_noise, ref_s, s_prev, taps=taps,
                        controls=controls, **ckw)
    t_en, d, s, ref = f["t_en"], f["d"], f["s"], f["ref"]
    out = dict(ref=ref, s_pred=f["s_mixed"] if f.get("s_mixed") is not None else torch.cat([ref, s], dim=-1))
    whole = lambda v: v

    def prosody(sel, dur, T, frames):
        """Alignment expansion + F0Ntrain of the rows `sel` picks as ONE C-ABI call (st2_prosody_forward; with `frames` its
        ragged form, every row as if alone), then the rows' pitch / energy controls.  `d_cm` is the branch's: each makes the
        channel-major copy where it always did.  hifigan: one-frame right shift, Demo/Inference_LibriTTS.ipynb:306-319."""
        asr, F0_pred, N_pred = _front_engine(model, dev).prosody_forward(sel(d_cm), sel(t_en), dur, sel(s), T, shift=hifigan,
                                                                         frames=frames)
        shaped = {}
        if intonation is not None:
            shaped["pitch"] = _pitch_shape(intonation, F0_pred, dur, frames=frames, sel=sel, shift=hifigan)
        _prosody_controls(controls, F0_pred, N_pred, dur, frames=frames, sel=sel, shift=hifigan)
        return dict(asr=asr, F0=F0_pred, N=N_pred, **shaped)

    if max_frames is not None:  # capacity-bound: no host read of the durations, one ragged prosody call at T = max_frames
        T_cap = int(max_frames)
        if durations is None:
            durations, len_arg = f["durations"], lengths_dev
            ops.check_status()  # the word is host-mapped: looking needs no synchronisation (whatever has completed is reported)
        else:
            durations, len_arg = durations.long().to(dev), None  # the caller's: pad-token frames count like any other
        durations = durations.contiguous()
        fitted = {}
        if fit is not None:  # out of place: forced durations are the caller's tensor
            durations, fitted["fit"] = ops.durations_fit(durations, fit[0], T_cap, lengths=len_arg, hold=fit[1])
        frames = ops.frames_from_durations(durations, len_arg, T_cap)
        d_cm = d.transpose(-1, -2).contiguous()
        return dict(out, durations=durations, **prosody(whole, durations, T_cap, frames), frames=frames, max_frames=T_cap,
                    token_lengths=len_arg, **fitted)
    if durations is None:
        durations = f["durations"]
        tot = durations.sum(dim=1).tolist()  # the path's one data-dependent host sync: the frame counts
        ops.check_status() if dev.type == "cuda" else None  # everything up to here has completed: free to look
    else:
        durations = durations.long()
        if total_frames is not None:  # the caller knows the row sums: nothing is read back
            tot = [int(total_frames)] * B if isinstance(total_frames, int) else [int(v) for v in total_frames]
            assert len(tot) == B
        else:
            tot = durations.sum(dim=1).tolist()  # host tensor: no device sync; device tensor: one read-back (forced
            #                                      durations are the caller's: pad-token frames are expanded like any other)
    durations = durations.to(dev)
    if taps is not None:
        taps["durations"] = durations
    out["durations"] = durations
    d_cm = d.transpose(-1, -2).contiguous()

    def expand(idx):
        """Alignment expansion + prosody for the utterances `idx` (all of one frame count T)."""
        T = int(tot[idx[0]])
        if len(idx) == B:
            sel = whole
        elif idx == list(range(idx[0], idx[0] + len(idx))):  # consecutive utterances: a view, no index tensor (whose pageable
            sel = lambda v: v[idx[0]:idx[0] + len(idx)]      # host -> device copy would stall the host behind the stream)
        else:
            sel = lambda v: v[torch.as_tensor(idx, device=dev)]
        dur = sel(durations)
        if _engine_path(dev, taps):
            return dict(prosody(sel, dur, T, None), ref=sel(ref), en=None)
        en = expand_by_durations(sel(d_cm), dur, T, shift=hifigan)                    # [b, 640, T]
        asr = expand_by_durations(sel(t_en), dur, T, shift=hifigan)                   # [b, 512, T]
        F0_pred, N_pred = model.predictor.F0Ntrain(en, sel(s))
        return dict(asr=asr, F0=F0_pred, N=N_pred, ref=sel(ref), en=en)

    if len(set(tot)) == 1 and not group_events:
        g = expand(list(range(B)))
        if taps is not None:
            taps.update(F0=g["F0"], N=g["N"], asr=g["asr"], en=g["en"])
        out.update(asr=g["asr"], F0=g["F0"], N=g["N"], **({"pitch": g["pitch"]} if "pitch" in g else {}))
        return out
    if not allow_ragged:
        raise ValueError("utterances of one call must have equal total duration; bucket them, pass `durations`, or "
                         "use inference() which decodes per frame count (frames per utterance: %s)" % tot)
    if ragged_decode:
        if not _engine_path(dev, taps):
            raise ValueError("ragged_decode needs the C++ engine path (HIP device, plan_mode 'engine', no taps)")
        T_max = int(max(tot))
        frames_host = [int(v) for v in tot]
        frames = torch.tensor(frames_host, dtype=torch.int32).to(dev)  # once per batch, before the prosody call is issued
        out.update(prosody(whole, durations, T_max, frames), frames=frames, frames_host=frames_host)
        return out
    groups = {}
    for b, T in enumerate(tot):
        groups.setdefault(int(T), []).append(b)
    out["groups"] = []
    for idx in sorted(groups.values(), key=lambda v: v[0]):  # in the order of each group's first utterance
        g = expand(idx)
        if group_events and dev.type == "cuda":
            g["ready"] = torch.cuda.Event()
            g["ready"].record(torch.cuda.current_stream(dev))
        out["groups"].append((idx, g))
    return out


def _decode_ragged(model, p, sine_noise=None, noise_rows=None):
    """One ragged decoder call over prepare(ragged_decode=True)'s padded batch -> list of [1, 600 T_b] waveforms.
    `sine_noise`: per-utterance SineGen draws (each >= 600 T_b samples), zero-padded here to the batch's T_max."""
    tot = p["frames_host"]
    w = _decode_frames(model, p, sine_noise, noise_rows)
    return [w[b, :, :600 * tot[b]] for b in range(len(tot))]


def _decode_frames(model, p, sine_noise, noise_rows=None, strict=False):
    """The ONE ragged decoder call of a prepared batch that carries `frames`, at the batch's width T (its longest row, or the
    capacity).  The SineGen draws reach it as a [B, 600 T, 9] view of the caller's batch tensor where that is [B, >= 600 T, 9];
    anything else is copied row by row (`noise_rows`, or sine_noise[b]) -- or, with `strict`, refused."""
    B, T = p["asr"].shape[0], p["asr"].shape[-1]
    sn = None
    if sine_noise is not None and noise_rows is None and torch.is_tensor(sine_noise) and sine_noise.dim() == 3 \
            and sine_noise.shape[0] == B and sine_noise.shape[1] >= 600 * T:
        sn = sine_noise[:, :600 * T]  # the batch's own rows: a view (the decoder reads row b only up to 600 frames[b])
    elif sine_noise is not None and strict:
        raise ValueError("sine_noise must be [B, >= 600 * max_frames, 9] on the capacity-bound path")
    elif sine_noise is not None:
        tot = p["frames_host"]
        rows = [sine_noise[b] for b in range(B)] if noise_rows is None else noise_rows
        # rows of different lengths (one per sentence): stacked into the T_max layout; past 600 T_b nothing is read, so
        # the buffer is not cleared
        sn = torch.empty((B, 600 * T, rows[0].shape[-1]), device=p["asr"].device, dtype=torch.float32)
        for b, n in enumerate(rows):
            sn[b, :600 * tot[b]] = n[:600 * tot[b]]
    return model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sn, frames=p["frames"])


class SynthesisResult:
    """What the capacity-bound path returns (`inference(max_frames=)`, `GraphedSynthesis`), all on the
    device and none of it waited for:
      wave     [B, 1, samples_per_frame * max_frames] fp32, exact zeros from row b's samples_per_frame * frames[b] on;
      frames   int32 [B]: every row's frame count, clamped to 1..max_frames;
      packed   (with `pack`) the rows' valid samples minus `trim` each, back to back: int16 PCM ("s16") or fp32 ("f32"), or --
               with `sample_rate` / a G.711 `pack` -- those samples at `sample_rate` as fp32, int16 or mu-law / A-law bytes;
      offsets  (with `pack`) int64 [B + 1]: row b is packed[offsets[b]:offsets[b + 1]];
      sample_rate  the rate of `packed` (24000 unless the call asked for another); `wave` is always at 24 kHz;
      marks    (with `marks=True`) int32 [B, N + 1]: token n of row b is
               packed[offsets[b] + marks[b, n] : offsets[b] + marks[b, n + 1]], marks[b, N] = the row's sample count.  The
               positions are at `sample_rate`, after `trim`; pad tokens and tokens a truncated row lost sit at the row's end.
               Kept in the same allocation, between `offsets` and the samples: `to_host(marks=True)` is still one copy.
      style    [B, 256]: the mixed style rows (`prepare`'s `s_pred`); a passage continues in the next call with
               `s_prev=result.style[-1:]`;
      gaps     (with `gaps=`) int32 [B]: the samples of silence asked for behind every row, as the packing step read them (it
               clamps them to 0..`max_gap`), kept in the same allocation behind the marks.  Row b's speech is then
               packed[offsets[b] : offsets[b + 1] - g_b], its break the g_b samples behind it, and offsets[B] the length of the
               whole passage.  `marks` stay relative to their row: a position in the passage is offsets[b] + marks[b, n], and
               offsets[b + 1] - offsets[b] = marks[b, N] + g_b.
      level    (with `level=`) fp32 [B, 4]: every row's integrated loudness in LUFS (-inf when no block
               passed the gates), its sample peak, the linear gain its packed samples were multiplied by and the number of gating
               blocks that passed -- measured on `wave`, which stays as the decoder made it.  Kept in the same allocation behind
               the gaps: `to_host(level=True)` is still one copy.
      edges    (with `edges=`) int32 [B, 2]: {head, count} at the model rate -- row b's packed samples are
               wave[b, 0, head : head + count], faded at an edge that was cut, through the rest of the hand-over; offsets, marks
               and the level are those of the cut rows.  Kept in the same allocation: `to_host(edges=True)` is still one copy.
      breaks   (with `breaks=`) int32 [B, 2]: {the row's samples with its pauses, the silence inserted} at the
               model rate.  Kept in the same allocation: `to_host(breaks=True)` is still one copy.
      dynamics (with `dynamics=`) float32 [B, 2]: {the deepest gain reduction in dB, the number of 64-sample
               blocks that were reduced}; {0, 0} for a row left alone.  Kept in the same allocation: `to_host(dynamics=True)` is
               still one copy.
      volume   (with `volume=`) float32 [B, 2]: {the peak of the row behind the gains, the number of
               64-sample blocks whose gain is not 1}.  Kept in the same allocation: `to_host(volume=True)` is still one copy.
      fit      (with `fit_frames=`) int32 [B, 4]: {the row's frames before the fit, its frames after,
               flag, the number of tokens whose duration changed}; flag 0 = the target was met, 1 = it was infeasible and the
               nearest feasible total was taken, 2 = nothing to stretch (no token, or every token held), 3 = the row was left
               as it was (its held tokens alone exceed the capacity, or a forced total beyond 2^31 - 1).  A small tensor of its
               own, NOT a part of the hand-over allocation: reading it (`result.fit.cpu()`) is a copy of its own.
      pitch    (with `intonation=`) fp32 [B, 4]: {the row's voiced mean F0 in Hz (geometric), its voiced
               columns, the lowest and the highest F0 after the range and the contour}; {NaN, 0, NaN, NaN} for a row without a
               voiced column.  Like `fit` a small tensor of its own.
    `to_host()` is the one place that waits.  Made with `spec` (an `_Output`, trim resolved: `trim`, `pack`, `sample_rate`, `max_gap`)
    and `ho` (the `_HandOver` that `_hand_over` returned for it, None without `pack`: `packed`, `offsets`, `gaps`, `level`)."""

    def __init__(self, wave, frames, max_frames, spec=None, ho=None, marks=None, style=None, fit=None, pitch=None):
        self.wave, self.frames, self.max_frames = wave, frames, int(max_frames)
        self.samples_per_frame = wave.shape[-1] // self.max_frames
        self.spec = spec = _Output() if spec is None else spec
        self.trim, self.pack, self.sample_rate, self.max_gap = int(spec.trim), spec.fmt, _rate(spec.sample_rate), spec.max_gap
        self.marks, self.style, self.fit, self.pitch = marks, style, fit, pitch
        self._take(ho)
        self._host = None  # the buffer's pinned mirror, allocated by the first to_host()

    def _take(self, ho):
        """offsets, marks, gaps, level and packed are views of the hand-over's one allocation: one copy takes all."""
        self._ho, self._buf = ho, None if ho is None else ho.buf
        self.packed, self.offsets, self.gaps = (None, None, None) if ho is None else (ho.packed, ho.offsets, ho.gaps)
        self.level = None if ho is None or ho.level is None else ho.level.view(-1, 4)
        self.limit = None if ho is None or ho.limit is None else ho.limit.view(-1, 2)
        self.edges = None if ho is None or ho.edges is None else ho.edges.view(-1, 2)
        self.breaks = None if ho is None or ho.breaks is None else ho.breaks.view(-1, 2)
        self.dynamics = None if ho is None or ho.dynamics is None else ho.dynamics.view(-1, 2)
        self.volume = None if ho is None or ho.volume is None else ho.volume.view(-1, 2)

    def to_host(self, marks=False, passage=False, level=False, limit=False, edges=False, breaks=False, dynamics=False,
                volume=False):
        """The list of per-utterance 1-D numpy arrays (int16 for "s16", uint8 for "ulaw" / "alaw", else float32; `trim` applied,
        at `sample_rate`): ONE device -> host copy
        into pinned memory of the offsets and the samples together, then one wait for it, then `ops.check_status()` -- the
        copy has waited for every kernel of the call, so a row truncated to `max_frames` (ST2_STATUS_FRAME_CAPACITY) is
        reported here, also on a graph replay, which runs no Python in between.  A result made without `pack` is packed as
        fp32 first.  The pinned buffer is allocated once per result object (a pinned allocation costs milliseconds) and the
        arrays are views of it: a `GraphedSynthesis` hands out the same result at every replay, so consume or copy them
        before the next `to_host()`.  The copy takes the buffer at capacity, not at offsets[B]: sizing it by the total
        would need a second wait.  `marks=True` (a result made with `marks=True`): returns (arrays, marks) with the timing marks as
        an int32 [B, N + 1] numpy array out of the same copy.  A result with `gaps` gives every row's speech WITHOUT its break,
        as a result without gaps does; `passage=True` gives instead the ONE contiguous array packed[:offsets[B]], speech and
        breaks as a client plays them.  `level=True` (a result made with `level=`): the level table as a float32 [B, 4] numpy
        array out of the same copy, behind whatever else is returned: (arrays, level) or (arrays, marks, level).  `limit=True` (a
        result made with a limiting `Level`): the limiter's {drive gain, smallest gain factor} as a float32 [B, 2] numpy array, out
        of the same copy, behind those.  `edges=True` (a result made with `edges=`): {head, count} per row as an int32 [B, 2] numpy
        array, out of the same copy, behind those.  `breaks=True` (a result made with `breaks=`): {the row's samples with its pauses,
        the silence inserted} at the model rate as an int32 [B, 2] numpy array, out of the same copy, behind those.  `dynamics=True` (a
        result made with `dynamics=`): {deepest reduction in dB, blocks reduced} per row as a float32 [B, 2] numpy array, out of the
        same copy, behind those.  `volume=True` (a result made with `volume=`): {peak, blocks with a gain} per row as a float32 [B, 2]
        numpy array, out of the same copy, last."""
        if volume and self.volume is None:
            raise ValueError("this result carries no volume table: ask for it with inference(..., volume=Volume(...))")
        if dynamics and self.dynamics is None:
            raise ValueError("this result carries no dynamics table: ask for it with inference(..., dynamics=Dynamics(...))")
        if breaks and self.breaks is None:
            raise ValueError("this result carries no breaks table: ask for it with inference(..., breaks=Breaks(...))")
        if edges and self.edges is None:
            raise ValueError("this result carries no edges table: ask for it with inference(..., edges=Edges(...))")
        if level and self.level is None:
            raise ValueError("this result carries no level table: ask for it with inference(..., level=Level(...))")
        if limit and self.limit is None:
            raise ValueError("this result carries no limit table: ask for it with inference(..., level=Level(..., limiter=True))")
        if marks and self.marks is None:
            raise ValueError("this result carries no timing marks: ask for them with inference(..., marks=True)")
        if self._ho is None:
            self._take(_hand_over(self.wave, self.frames, self.trim, "f32", self.samples_per_frame))
        if self._host is None or self._host.shape != self._buf.shape:
            self._host = torch.empty(self._buf.shape, dtype=torch.uint8, pin_memory=True)
        self._host.copy_(self._buf, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self._buf.device))
        done.synchronize()
        ops.check_status()
        B = self.frames.numel()
        offs, m, g, samples, lv = self._ho.views(self._host)  # the layout the buffer was allocated with
        offs, samples = offs.tolist(), samples.numpy()
        if passage:
            rows = samples[:offs[B]]
        elif g is None:
            rows = [samples[offs[b]:offs[b + 1]] for b in range(B)]
        else:  # the breaks as the packing step counted them: clamped to 0..max_gap
            g = g.clamp(0, self.max_gap).tolist()
            rows = [samples[offs[b]:offs[b + 1] - g[b]] for b in range(B)]
        more = ((m.numpy().reshape(tuple(self.marks.shape)),) if marks else ()) + ((lv.numpy().reshape(B, 4),) if level else ())
        if limit:
            more += (self._ho.limit_view(self._host).numpy().reshape(B, 2),)
        if edges:
            more += (self._ho.edges_view(self._host).numpy().reshape(B, 2),)
        if breaks:
            more += (self._ho.breaks_view(self._host).numpy().reshape(B, 2),)
        if dynamics:
            more += (self._ho.dynamics_view(self._host).numpy().reshape(B, 2),)
        if volume:
            more += (self._ho.volume_view(self._host).numpy().reshape(B, 2),)
        return (rows,) + more if more else rows


def _rate(sample_rate):
    """The rate of the packed samples: the caller's `sample_rate`, None = the model's 24 kHz."""
    return resample.MODEL_RATE if sample_rate is None else int(sample_rate)


def gap_samples(ms, sample_rate=None):
    """A break of `ms` milliseconds as samples of the hand-over at `sample_rate` (None: the model's 24 kHz): rint(ms * rate /
    1000), ties to even -- the one conversion between SSML's break times and `gaps=`.  A scalar gives an int, a sequence a list."""
    rate = _rate(sample_rate)
    one = lambda v: int(round(float(v) * rate / 1000.0))  # Python's round: half to even, as rint
    return [one(v) for v in ms] if isinstance(ms, (list, tuple)) else one(ms)


def _passage_controls(controls, starts, B, dev):
    """The start flags of `inference(passage=[...])` as mixing weight t = 0 on the flagged rows: a `Controls` over a copy of the
    caller's rows (all absent when there are none) whose `t` row -- what `st2_style_mix_rows` weighs the previous style with -- is
    0 where a passage begins and the caller's value (NaN = the call's scalar) elsewhere.  mix2(0, prev, 1, cur) is cur for a finite
    prev.  A device tensor of flags is never read on the host."""
    if torch.is_tensor(starts) and starts.is_cuda:
        flag = starts.reshape(-1) != 0
    else:
        flag = torch.as_tensor(starts).reshape(-1) != 0
    if flag.numel() != B:
        raise ValueError("passage must be True or %d start flags, got %d" % (B, flag.numel()))
    flag = flag.to(dev)
    if controls is None:
        controls = Controls(B, device=dev)
    c = controls.slice(0, B)
    c.buf = controls.buf.clone()
    i = Controls.NAMES.index("t")
    c.buf[i] = torch.where(flag, torch.zeros((), device=dev), controls.buf[i])
    c.present = tuple(n for n in Controls.NAMES if n in controls.present or n == "t")
    return c


def _passage_starts(passage, B, dev):
    """The start flags of a call's `passage` as the int32 [B] device row `ops.wave_level(starts=)` reads: None / True = the rows
    are one passage, [1, 0, ..., 0]; flags = the caller's, nonzero = 1.  A device tensor of flags is never read on the host."""
    if passage is None or passage is True:
        flag = torch.zeros((B,), dtype=torch.int32, device=dev)
        flag[:1] = 1
        return flag
    flag = passage if torch.is_tensor(passage) else torch.as_tensor(passage)
    return (flag.reshape(-1) != 0).to(device=dev, dtype=torch.int32)


def _resamples(fmt, sample_rate):
    """True when the packing step is `ops.wave_resample_pack`: another rate than the model's, or a G.711 format.  24 kHz fp32 /
    16-bit PCM stays `ops.wave_pack`."""
    return sample_rate not in (None, resample.MODEL_RATE) or fmt not in ops.PACK_FORMATS


class _HandOver:
    """The layout of the ONE allocation of the hand-over, stated here and nowhere else:

        [offsets int64 [B + 1] | marks int32 [n_marks] | gaps int32 [B] | level float32 [4 B] | limit float32 [2 B] |
         edges int32 [2 B] | breaks int32 [2 B] | dynamics float32 [2 B] | volume float32 [2 B] | pad to 16 bytes |
         samples of `fmt`]

    with `n_marks` = 0 / no gaps / no level / no limit / no edges / no breaks / no dynamics / no volume the layout is the one without them, byte for byte.  `*_at` are the byte offsets of the
    ten parts (`samples_at` is the header's size); `views(buf)` gives the first four parts and the samples of a byte buffer of
    this layout, on the device or its pinned mirror, `limit_view`, `edges_view`, `breaks_view`, `dynamics_view` and `volume_view` the later
    ones; `allocate` makes the device buffer, after which `buf`, `offsets`, `marks`, `gaps`, `level`, `limit`, `edges`, `breaks`,
    `dynamics`, `volume` and `packed` are the buffer and its views (None for a part the layout does not have)."""

    def __init__(self, B, fmt, n_marks=0, with_gaps=False, with_level=False, with_limit=False, with_edges=False, with_breaks=False,
                 with_dynamics=False, with_volume=False):
        self.B, self.n_marks, self.with_gaps, self.dtype = int(B), int(n_marks), bool(with_gaps), ops.OUTPUT_FORMATS[fmt][1]
        self.with_level, self.with_limit, self.with_edges = bool(with_level), bool(with_limit), bool(with_edges)
        self.with_breaks = bool(with_breaks)
        self.offsets_at = 0
        self.marks_at = 8 * (self.B + 1)
        self.gaps_at = self.marks_at + 4 * self.n_marks
        self.level_at = self.gaps_at + (4 * self.B if self.with_gaps else 0)
        self.limit_at = self.level_at + (16 * self.B if self.with_level else 0)
        self.edges_at = self.limit_at + (8 * self.B if self.with_limit else 0)
        self.breaks_at = self.edges_at + (8 * self.B if self.with_edges else 0)
        self.with_dynamics = bool(with_dynamics)
        self.dynamics_at = self.breaks_at + (8 * self.B if self.with_breaks else 0)
        self.with_volume = bool(with_volume)
        self.volume_at = self.dynamics_at + (8 * self.B if self.with_dynamics else 0)
        self.samples_at = (self.volume_at + (8 * self.B if self.with_volume else 0) + 15) // 16 * 16
        self.buf = self.offsets = self.marks = self.gaps = self.packed = self.level = self.limit = self.edges = self.breaks = None
        self.dynamics = self.volume = None

    def limit_view(self, buf):
        """The sixth part, float32 [2 B] (`ops.wave_limit`'s {g', min q} per row), of a uint8 buffer of this
        layout, or None.  Apart from `views`, whose five parts stay the five they were."""
        return buf[self.limit_at:self.limit_at + 8 * self.B].view(torch.float32) if self.with_limit else None

    def edges_view(self, buf):
        """The seventh part, int32 [2 B] (`ops.wave_edges`'s {head, count} per row), of a uint8 buffer of this
        layout, or None.  Apart from `views`, as `limit_view` is."""
        return buf[self.edges_at:self.edges_at + 8 * self.B].view(torch.int32) if self.with_edges else None

    def breaks_view(self, buf):
        """The eighth part, int32 [2 B] (`ops.wave_breaks`'s {count', silence inserted} per row), of a uint8
        buffer of this layout, or None.  Apart from `views`, as `limit_view` is."""
        return buf[self.breaks_at:self.breaks_at + 8 * self.B].view(torch.int32) if self.with_breaks else None

    def dynamics_view(self, buf):
        """The ninth part, float32 [2 B] (`ops.wave_dynamics`'s {deepest reduction, blocks reduced} per row),
        of a uint8 buffer of this layout, or None.  Apart from `views`, as `limit_view` is."""
        return buf[self.dynamics_at:self.dynamics_at + 8 * self.B].view(torch.float32) if self.with_dynamics else None

    def volume_view(self, buf):
        """The tenth part, float32 [2 B] (`ops.wave_volume`'s {peak, blocks with a gain} per row), of a uint8
        buffer of this layout, or None.  Apart from `views`, as `limit_view` is."""
        return buf[self.volume_at:self.volume_at + 8 * self.B].view(torch.float32) if self.with_volume else None

    def views(self, buf):
        """-> (offsets int64 [B + 1], marks int32 [n_marks] or None, gaps int32 [B] or None, samples, level float32 [4 B] or
        None) of a uint8 buffer: the parts the layout began with.  The later parts have a view function each."""
        i32 = lambda at, n: buf[at:at + 4 * n].view(torch.int32)
        return (buf[self.offsets_at:self.marks_at].view(torch.int64), i32(self.marks_at, self.n_marks) if self.n_marks else None,
                i32(self.gaps_at, self.B) if self.with_gaps else None, buf[self.samples_at:].view(self.dtype),
                buf[self.level_at:self.level_at + 16 * self.B].view(torch.float32) if self.with_level else None)

    def allocate(self, samples, device):
        self.buf = torch.empty((self.samples_at + samples * self.dtype.itemsize,), device=device, dtype=torch.uint8)
        self.offsets, self.marks, self.gaps, self.packed, self.level = self.views(self.buf)
        self.limit = self.limit_view(self.buf)
        self.edges = self.edges_view(self.buf)
        self.breaks = self.breaks_view(self.buf)
        self.dynamics = self.dynamics_view(self.buf)
        self.volume = self.volume_view(self.buf)
        return self


class _Output(typing.NamedTuple):
    """What the packed hand-over of ONE call is: the output options as `_output_spec` settled them, stated
    here and read by `_decode_capacity`, which hands them to `_hand_over`, by `GraphedSynthesis` and by `SynthesisResult`."""
    fmt: typing.Optional[str] = None          # `pack`; None: nothing is packed before the first `to_host()`
    trim: typing.Optional[int] = 0            # samples dropped from every row's end; None until `_decode_capacity` knows the decoder
    sample_rate: typing.Optional[int] = None  # as the caller gave it
    rate: typing.Optional[int] = None         # the rate the packing step resamples to; None: `ops.wave_pack` serves (`_resamples`)
    marks: bool = False
    max_gap: int = 0                          # 0 without gaps


def _capacity_only(names, *given):
    """The one statement that options belong to the capacity-bound path, over the subset `names` an entry point names."""
    if any(v is not None for v in given):
        raise ValueError("%s belong to the capacity-bound path: pass max_frames" % names)


def _output_spec(B, capacity, pack=None, trim=None, sample_rate=None, marks=False, gaps=None, max_gap=None, level=None, graph=False,
                 passage=None, front_groups=1, edges=None, breaks=None, N=None, dynamics=None, volume=None,
                 device=None):
    """The seven output options of a call of B rows -> (`_Output`, `gaps` as an int32 [B] tensor, host or device as given), and
    every refusal about them, for `inference`, `synthesize_long(max_frames=)` and `GraphedSynthesis` alike, before anything is
    launched: `pack` one of `ops.OUTPUT_FORMATS` or None; `sample_rate` one of `resample.RATES` or None; `level` a `Level` of the
    B rows; `max_gap` not negative, and a bound of `gaps` -- a host sequence defaults it to its own maximum, a device tensor is
    never read and needs it; and all of them but `trim` only with `pack` on the capacity-bound path.
    `capacity`: the call has a `max_frames`.  `graph`: the caller is `GraphedSynthesis`, to which `max_frames` is no option --
    its `marks` refusal names `pack` alone.  `trim` goes through as given: `_decode_capacity` resolves None.  `passage`: the
    call's `passage`, and `front_groups`: the front calls `synthesize_long` cuts the passage into -- what a `Level` of
    scope "passage" is judged by, and looked at for nothing else.  `edges`: an `Edges` of the B rows, judged here and handed on by
    the caller (the spec does not carry it, as it does not carry `level`).  `breaks`: a `Breaks` of the B rows and of the call's `N`
    tokens (None: the caller has no token count to judge by), likewise.  `dynamics`: a `Dynamics` of the B rows, likewise.  `volume`: a `Volume` of the B rows, of the
    call's `N` tokens where it holds a per-token table and on the call's `device` (None: the caller has none to judge by), likewise."""
    if pack is not None and pack not in ops.OUTPUT_FORMATS:
        raise ValueError("pack must be None or one of %s, got %r" % (sorted(ops.OUTPUT_FORMATS), pack))
    if sample_rate is not None and pack is None:
        raise ValueError("sample_rate is the rate of the packed samples: pass pack")
    if sample_rate is not None and sample_rate not in resample.RATES:
        raise ValueError("sample_rate must be None or one of %s, got %r" % (list(resample.RATES), sample_rate))
    if level is not None and (pack is None or not capacity):
        raise ValueError("level is a gain in the packed samples of the capacity-bound path: pass max_frames and pack")
    if level is not None and (not isinstance(level, Level) or level.B != B):
        raise ValueError("level must be a pipeline.Level of %d rows" % B)
    if level is not None and level.scope == "passage" and (passage is None or passage is False):
        raise ValueError("level of scope 'passage' is one gain for the rows of a passage: pass passage")
    if level is not None and level.scope == "passage" and front_groups > 1:
        raise ValueError("level of scope 'passage' is one gain for the rows of ONE call, and front_batch cuts this passage into %d: "
                         "pass front_batch=0" % front_groups)
    if edges is not None and (pack is None or not capacity):
        raise ValueError("edges are cut from the packed samples of the capacity-bound path: pass max_frames and pack")
    if edges is not None and (not isinstance(edges, Edges) or edges.B != B):
        raise ValueError("edges must be a pipeline.Edges of %d rows" % B)
    if breaks is not None and (pack is None or not capacity):
        raise ValueError("breaks are spliced into the packed samples of the capacity-bound path: pass max_frames and pack")
    if breaks is not None and (not isinstance(breaks, Breaks) or breaks.B != B or (N is not None and breaks.N != N)):
        raise ValueError("breaks must be a pipeline.Breaks of %d rows%s" % (B, "" if N is None else " of %d tokens" % N))
    if dynamics is not None and (pack is None or not capacity):
        raise ValueError("dynamics compress the packed samples of the capacity-bound path: pass max_frames and pack")
    if dynamics is not None and (not isinstance(dynamics, Dynamics) or dynamics.B != B):
        raise ValueError("dynamics must be a pipeline.Dynamics of %d rows" % B)
    if volume is not None and (pack is None or not capacity):
        raise ValueError("volume is a gain in the packed samples of the capacity-bound path: pass max_frames and pack")
    if volume is not None and (not isinstance(volume, Volume) or volume.B != B or (N is not None and volume.N not in (None, N))):
        raise ValueError("volume must be a pipeline.Volume of %d rows%s" % (B, "" if N is None else " of %d tokens" % N))
    if volume is not None and device is not None and volume.device != torch.empty(0, device=device).device:
        raise ValueError("volume holds its tables on %s, the batch is on %s" % (volume.device, device))
    if not capacity:
        _capacity_only("passage / gaps / max_gap / s_prev", gaps, max_gap)
    if pack is None and (gaps is not None or max_gap is not None):
        raise ValueError("gaps are silence in the packed samples: pass pack")
    if max_gap is not None and int(max_gap) < 0:
        raise ValueError("max_gap must not be negative, got %r" % (max_gap,))
    if gaps is None and max_gap is not None:
        raise ValueError("max_gap bounds `gaps`: pass gaps")
    if torch.is_tensor(gaps) and gaps.is_cuda:
        if max_gap is None:
            raise ValueError("gaps on the device are never read on the host: pass max_gap, the longest break in samples")
        if gaps.dtype != torch.int32 or gaps.numel() != B:
            raise ValueError("gaps must be an int32 tensor of %d entries, got %s %s" % (B, gaps.dtype, tuple(gaps.shape)))
    elif gaps is not None:
        gaps = torch.as_tensor(gaps).reshape(-1)
        if gaps.numel() != B or gaps.dtype.is_floating_point or int(gaps.abs().max()) >= 2 ** 31:
            raise ValueError("gaps must be %d whole sample counts (pipeline.gap_samples converts milliseconds)" % B)
        if max_gap is None:
            max_gap = max(int(gaps.max()), 0)
        gaps = gaps.to(torch.int32)
    if marks and (not capacity or pack is None):
        raise ValueError("marks are positions in the packed samples" + (
            ": pass pack" if graph else " of the capacity-bound path: pass max_frames and pack"))
    if not capacity:
        _capacity_only("pack / trim / lengths_dev", pack, trim)
    rate = _rate(sample_rate) if pack is not None and _resamples(pack, sample_rate) else None
    max_gap = 0 if gaps is None else int(max_gap)
    return _Output(pack, trim, sample_rate, rate, bool(marks), max_gap), gaps


def _hand_over(wave, frames, trim, fmt, samples_per_frame, sample_rate=None, n_marks=0, gaps=None, max_gap=0, level=None, starts=None):
    """The hand-over without an edge trim: `_hand_over_edges` with `edges=None`, under the name and the parameter list it has
    always had."""
    return _hand_over_edges(wave, frames, trim, fmt, samples_per_frame, sample_rate, n_marks, gaps, max_gap, level, starts)


def _hand_over_edges(wave, frames, trim, fmt, samples_per_frame, sample_rate=None, n_marks=0, gaps=None, max_gap=0, level=None,
                     starts=None, edges=None, breaks=None, tokens=None, dynamics=None, volume=None):
    """The packing step into ONE device allocation (`_HandOver`, returned with its views), the samples at capacity -- ceil(L U /
    D) per row, and `max_gap` more with `gaps` -- so that a single copy brings all of it to the host.  Which wrapper packs:
    with `gaps` (int32 [B], host or device) `ops.wave_pack_gaps`, which reads them from the header they
    are copied into here; else, where `_resamples`, `ops.wave_resample_pack`; else `ops.wave_pack`.  With `level` (a `Level`;
    DESIGN.md section 23) `ops.wave_level` measures the rows into the header's level part -- its workspace comes from the caching
    allocator, under capture from the graph's own pool, which lives as long as the graph -- and `ops.wave_pack_level` packs them
    with the gains it reads there, with or without gaps and a rate.  A `Level` with `true_peak` has `ops.wave_level` read the
    table of `resample.true_peak_table`; one of scope "passage" has it read `starts` (int32 [B] on the device, 1 where a
    passage begins; None = the rows are one passage).  A plain `Level` passes neither argument on.  A `Level` with `limiter`
    (DESIGN.md section 27): measure as above, then `ops.wave_limit` into a buffer of the caching allocator with {g', min q} into
    the header's limit part, then the wrapper a call WITHOUT a level takes, over the limited rows.  With `edges` (an `Edges`;
    DESIGN.md section 28) `ops.wave_edges` runs FIRST, into a buffer of the caching allocator with {head, count} into the header's
    edges part, and everything above runs unchanged over the cut rows: their sample counts are the frame counts of rows of
    one-sample frames, nothing trimmed -- frames = count, samples_per_frame = 1, trim = 0.  With `breaks` (a `Breaks`; DESIGN.md
    section 29) `ops.wave_breaks` runs behind the trim and in front of everything else, in the same manner: the tokens' boundaries
    in samples of the (cut) rows come from one `ops.token_marks` / `ops.token_marks_edges` launch without a rate over `tokens`
    (that wrapper's dur, T_cap, lengths and shift), the rows with their silence go to a buffer of the caching allocator of
    `max_break` more samples per row, {count', inserted} into the header's breaks part, and the rest runs over frames = count'.
    The boundaries and the inserted silence stay with the hand-over (`pos`, `ins`) for the marks.  With `dynamics` (a `Dynamics`;
    DESIGN.md section 30) `ops.wave_dynamics` runs behind the breaks and in front of the level, into a buffer of the caching
    allocator with {deepest reduction, blocks reduced} into the header's dynamics part: sample counts do not change, so frames,
    trim and samples_per_frame go on as they came, and the loudness target holds on the compressed programme.  With `volume` (a
    `Volume`) `ops.wave_volume` runs behind the compressor and in front of the level, in the same manner, with
    {peak, blocks with a gain} into the header's volume part.  The tokens' boundaries it reads are those of the rows as they are
    by then, from ONE marks launch without a rate over `tokens`: `ops.token_marks_breaks` over the `pos` and `ins` the breaks left
    where there are breaks, else the `ops.token_marks` / `ops.token_marks_edges` launch the breaks would have taken."""
    B, L = wave.shape[0], wave.shape[-1]
    rate = None if not _resamples(fmt, sample_rate) else (resample.MODEL_RATE if sample_rate is None else sample_rate)
    U, D = (1, 1) if rate is None else resample.table(rate, wave.device)[:2]
    room = resample.output_samples(L, U, D) + (0 if gaps is None else max_gap)
    if breaks is not None:
        room += resample.output_samples(breaks.max_break, U, D)
    limiting = level is not None and level.limiter
    ho = _HandOver(B, fmt, n_marks, gaps is not None, with_level=level is not None, with_limit=limiting,
                   with_edges=edges is not None, **({} if breaks is None else {"with_breaks": True}),
                   **({} if dynamics is None else {"with_dynamics": True}),
                   **({} if volume is None else {"with_volume": True})).allocate(B * room, wave.device)

    def boundaries():  # in the decoder's geometry (`tokens`), moved by the trim below where there is one
        marks_of = ops.token_marks if edges is None else functools.partial(ops.token_marks_edges, edges=ho.edges)
        return marks_of(tokens["dur"], tokens["frames"], tokens["T_cap"], lengths=tokens["lengths"], shift=tokens["shift"],
                        trim=tokens["trim"], samples_per_frame=tokens["samples_per_frame"])
    if edges is not None:
        wave, _ = ops.wave_edges(wave, frames, edges.top_db, edges.keep, resample.edge_ramp(edges.F, wave.device) if edges.F else None,
                                 trim=trim, samples_per_frame=samples_per_frame, edges=ho.edges)
        frames, trim, samples_per_frame = ho.edges.view(B, 2)[:, 1].contiguous(), 0, 1  # the counts as a row of their own
    if breaks is not None:
        ho.pos = boundaries()
        wave, ho.ins, _, _ = ops.wave_breaks(wave, frames, ho.pos, breaks.samples, breaks.max_break,
                                             resample.edge_ramp(breaks.F, wave.device) if breaks.F else None, trim=trim,
                                             samples_per_frame=samples_per_frame, breaks=ho.breaks)
        frames, trim, samples_per_frame = ho.breaks.view(B, 2)[:, 0].contiguous(), 0, 1
    if dynamics is not None:
        A = dynamics.A
        wave, _ = ops.wave_dynamics(wave, frames, dynamics.params, resample.limit_window(A, wave.device) if A else None, A=A,
                                    rho=dynamics.rho, trim=trim, samples_per_frame=samples_per_frame, dynamics=ho.dynamics)
    if volume is not None:
        A = volume.A
        pos = boundaries() if breaks is None else ops.token_marks_breaks(ho.pos, ho.ins)
        wave, _ = ops.wave_volume(wave, frames, pos, volume.db, volume.tok_db, resample.limit_window(A, wave.device) if A else None,
                                  A=A, lengths=tokens["lengths"], trim=trim, samples_per_frame=samples_per_frame, volume=ho.volume)
    into = dict(trim=trim, fmt=fmt, out=ho.packed, offsets=ho.offsets, samples_per_frame=samples_per_frame)
    if gaps is not None:
        ho.gaps.copy_(gaps.reshape(B), non_blocking=True)
    if level is not None:
        more = {}
        if level.true_peak:
            more.update(true_peak=resample.true_peak_table(wave.device))
        if level.scope == "passage":
            more.update(starts=_passage_starts(starts, B, wave.device))
        ops.wave_level(wave, frames, level.target, ceiling=level.ceiling, max_gain_db=level.max_gain_db, trim=trim,
                       samples_per_frame=samples_per_frame, sample_rate=resample.MODEL_RATE, out=ho.level, **more)
    if limiting:
        # the limited rows in a buffer of the caching allocator (under capture: the graph's pool), then the packing wrappers
        # below as they are, without a level: the packed bytes are what they give for that input
        wave, _ = ops.wave_limit(wave, frames, ho.level, level.target, resample.limit_window(level.W, wave.device),
                                 ceiling=level.ceiling, max_gain_db=level.max_gain_db, drive_db=level.drive_db, trim=trim,
                                 samples_per_frame=samples_per_frame, limit=ho.limit, **more)
    elif level is not None:
        ops.wave_pack_level(wave, frames, ho.level, gaps=ho.gaps, max_gap=max_gap, rate=rate, **into)
        return ho
    if gaps is not None:
        ops.wave_pack_gaps(wave, frames, ho.gaps, max_gap, rate=rate, **into)
    elif rate is not None:
        ops.wave_resample_pack(wave, frames, rate, **into)
    else:
        ops.wave_pack(wave, frames, **into)
    return ho


def _decode_capacity(model, p, sine_noise, spec, gaps, level, starts=None, edges=None, breaks=None, dynamics=None, volume=None):
    """ONE ragged decoder call at the capacity of prepare(max_frames=) and, with `spec.fmt`, the packed samples: nothing is read
    back, nothing is sliced on the host.  `spec.marks`: one `ops.token_marks` launch behind the packing writes the timing marks
    into the hand-over allocation.  `gaps`: the breaks behind the rows, `level`: their loudness normalisation, `starts`: the call's `passage`
    for a level of scope "passage" (`_hand_over`), `edges`: their trim (`_hand_over_edges`; the marks are then `ops.token_marks_edges`'),
    `breaks`: the pauses inside them (`_hand_over_edges`; the marks are then `ops.token_marks_breaks`'), `dynamics`: their compressor
    (`_hand_over_edges`; it moves no sample, so the marks are what they are without it), `volume`: their gains, likewise."""
    T_cap = p["max_frames"]
    w = _decode_frames(model, p, sine_noise, strict=True)  # the noise as a view or not at all: nothing is copied here
    hifigan = model.decoder.kind == "hifigan"
    if spec.trim is None:  # read here and nowhere else: `inference`'s default, Demo/Inference_LibriTTS.ipynb:325 `[..., :-50]`
        spec = spec._replace(trim=50 if hifigan else 0)
    if spec.fmt is None:
        return SynthesisResult(w, p["frames"], T_cap, spec, style=p["s_pred"], fit=p.get("fit"), pitch=p.get("pitch"))
    dur = p["durations"]
    B, N = dur.shape
    spf = w.shape[-1] // T_cap
    more = {} if edges is None else {"edges": edges}  # the optional stages of the hand-over; none: `_hand_over` as ever
    if breaks is not None and breaks.N != N:
        raise ValueError("breaks must be a pipeline.Breaks of %d rows of %d tokens" % (B, N))
    if volume is not None and volume.N not in (None, N):
        raise ValueError("volume must be a pipeline.Volume of %d rows of %d tokens" % (B, N))
    if breaks is not None or volume is not None:  # the stages that read the tokens' boundaries
        more.update(tokens=dict(dur=dur, frames=p["frames"], T_cap=T_cap, lengths=p.get("token_lengths"), shift=hifigan,
                                trim=spec.trim, samples_per_frame=spf))
    if breaks is not None:
        more.update(breaks=breaks)
    if dynamics is not None:
        more.update(dynamics=dynamics)
    if volume is not None:
        more.update(volume=volume)
    hand_over = functools.partial(_hand_over_edges, **more) if more else _hand_over
    ho = hand_over(w, p["frames"], spec.trim, spec.fmt, spf, spec.sample_rate, B * (N + 1) if spec.marks else 0, gaps, spec.max_gap,
                   level, starts)
    m = None
    if spec.marks and breaks is not None:
        m = ops.token_marks_breaks(ho.pos, ho.ins, rate=spec.sample_rate, out=ho.marks.view(B, N + 1))
    elif spec.marks:
        m = ho.marks.view(B, N + 1)
        marks_of = ops.token_marks if edges is None else functools.partial(ops.token_marks_edges, edges=ho.edges)
        marks_of(dur, p["frames"], T_cap, lengths=p.get("token_lengths"), shift=hifigan, trim=spec.trim,
                 rate=spec.sample_rate, samples_per_frame=spf, out=m)
    return SynthesisResult(w, p["frames"], T_cap, spec, ho, marks=m, style=p["s_pred"], fit=p.get("fit"), pitch=p.get("pitch"))


class GraphedSynthesis:
    """tokens -> (packed) waveform as ONE hipGraph: `inference(max_frames=, lengths_dev=)` captured on
    one stream -- the capture has no side stream, the graph is a linear chain -- over static input buffers

        tokens int64 [B, N], lengths_dev int32 [B], noise [B, 1, 256], step_noise [steps - 1, B, 1, 256],
        sine_noise [B, 600 max_frames, 9], ref_s [B, 256] (multi-speaker models)

    which `__call__` fills from whatever the caller hands in (anything left out keeps its previous contents; the `static` dict
    gives direct access) before it replays.  The returned `SynthesisResult` refers to the graph's own output buffers: consume
    it (`to_host()`) before the next replay.  Recorded on the first call; recorded again when the front's or the decoder's
    engine was rebuilt or re-calibrated (the operand scales are kernel arguments), by the rule `GraphedFront` follows.

    Per-request controls are one more static buffer, `static["controls"]` (a `Controls` with all six rows):
    the graph is recorded over it holding the neutral values, `__call__(controls=)` copies the caller's rows in and a call
    without them resets it to neutral.  Other controls never re-record.

    `marks=True`: the marks launch is recorded in the graph and the result carries `marks`.
    `token_controls` (default: `marks`): the static `Controls` also holds the three per-token rows, neutral, and the graph is
    recorded with the kernels that read them, so that one graph serves any token controls too; without it the graph issues
    the launches it always did and refuses a `Controls` with token rows.

    `pack` / `sample_rate` as in `inference`: with an output rate or a G.711 format the packing step inside the graph is
    `ops.wave_resample_pack`, whose filter table is designed and uploaded here, before any capture.

    `passage=True` / `max_gap`: the graph records the style carry-over and, with `max_gap` (which needs
    `pack`), the gap-aware pack, over three more static buffers -- `starts` (int32 [B]: 1 where a row begins a passage; at first
    row 0 alone), `s_prev` ([1, 256]: the style row 0 continues from unless its start flag is set) and `gaps` (int32 [B], zeros:
    samples of silence behind every row, clamped to 0..max_gap by the kernel).  `__call__(starts=, s_prev=, gaps=)` fills them
    (what is left out keeps its contents): one recorded graph serves any breaks up to `max_gap`, any start flags and any
    `s_prev`.  `t` is the carry-over's weight.  Built without them, the graph records exactly what it recorded before.

    `level=True` (or a `Level`; needs `pack`): the graph records the level measurement and the gain-applying
    pack over one more static buffer, `static["level"]` (a `Level`; at first -16 LUFS in every row, or the one given):
    `__call__(level=)` -- a `Level`, one target or B of them, None / NaN = leave the row alone -- copies the targets into its
    row, so one graph serves any targets; the ceiling and the gain limit are the graph's own.  Without it the graph records
    exactly what it recorded before.

    `seeds=True`: the graph draws its own noise.  `static["seeds"]` (int64 [B], zeros at first) takes the
    place of the three noise buffers, which such a graph does not have; the three `ops.noise_fill` launches are recorded in the
    graph and read the seeds on the device, so one recorded graph serves any seeds: `__call__(seeds=)` -- an int64 [B] tensor
    or B ints -- copies them in, and a call without them replays the seeds it holds, i.e. the same rendition.  `noise` /
    `step_noise` / `sine_noise` are refused by such a graph, `seeds` by a graph built without it, which has no such key and
    records exactly what it recorded before.

    `fit=True`: the graph records the one `ops.durations_fit` launch over two more static buffers,
    `static["fit_frames"]` (int32 [B], zeros: every row left alone) and `static["fit_hold"]` (uint8 [B, N], zeros: no token
    held), both read on the device, so one recorded graph serves any targets: `__call__(fit_frames=, fit_hold=)` copies them in
    (what is left out keeps its contents) and the result carries `fit`.  A graph built without it has neither key, refuses both
    arguments and records exactly what it recorded before.

    `edges=True` (or an `Edges`; needs `pack`): the graph records the trim in front of the hand-over over one
    more static buffer, `static["edges"]` (an `Edges`; at first 40 dB in every row, or the one given): `__call__(edges=)` -- an
    `Edges`, one `top_db` or B of them, None / NaN = leave the row alone -- copies the thresholds into its row, so one graph
    serves any thresholds; the pads and the fade are the graph's own.  Without it the graph records exactly what it recorded
    before.

    `breaks=True` (or a `Breaks`; needs `pack`) with `max_break_ms` (the cap of the silence in one row, 2 000 by
    default): the graph records the pauses inside the rows over one more static buffer, `static["breaks"]` (a `Breaks`; at first
    no pause anywhere, or the table given): `__call__(breaks=)` -- a `Breaks` or an int [B, N] table of samples at 24 kHz --
    copies the table into it, so one graph serves any pauses up to the cap; the cap and the fade are the graph's own.  Without
    it the graph records exactly what it recorded before.

    `dynamics=True` (or a `Dynamics`; needs `pack`): the graph records the compressor over one more static
    buffer, `static["dynamics"]` (a `Dynamics`; at first the defaults in every row, or the one given): `__call__(dynamics=)` -- a
    `Dynamics` of B rows -- copies its table into it, so one graph serves any thresholds, ratios, knees and make-up gains;
    `attack_ms` and `release_db_per_s` are the graph's own, fixed at construction.  Without it the graph records exactly what it
    recorded before.

    `intonation=True` (or an `Intonation`, whose `K` and `voiced_hz` are taken): the graph records the one
    `ops.pitch_shape` launch over one more static object, `static["intonation"]` (an `Intonation` with every table present and
    neutral: range 1, no contour point, and -- with `token_controls` or `marks` -- token ranges of 1): `__call__(intonation=)`
    copies the caller's tables in, a table it lacks and a call without the argument reset to neutral, so one graph serves any
    ranges and contours; `K` and `voiced_hz` are the graph's own.  The result carries `pitch`.  Without it the graph records
    exactly what it recorded before and refuses the argument.

    `volume=True` (or a `Volume`, whose `ramp_ms` is taken; needs `pack`): the graph records the gain stage
    over one more static object, `static["volume"]` (a `Volume` with both tables present and 0 dB): `__call__(volume=)` copies the
    caller's tables in, a table it lacks and a call without the argument reset to 0 dB, so one graph serves any gains; `ramp_ms`
    is the graph's own.  The result carries `volume`.  Without it the graph records exactly what it recorded before and refuses
    the argument."""

    def __init__(self, model, sampler, B, N, max_frames, diffusion_steps, ref_s=None, pack=None, trim=None,
                 embedding_scale=1.0, alpha=0.3, beta=0.7, lj_tail=None, device=None, sample_rate=None, marks=False,
                 token_controls=None, passage=False, max_gap=None, t=0.7, level=None, seeds=False, fit=False, edges=None,
                 breaks=None, max_break_ms=None, dynamics=None, intonation=None, volume=None):
        from .diffusion import GraphedSampler
        if volume is not None and not isinstance(volume, (bool, Volume)):
            raise ValueError("volume must be True or a pipeline.Volume, got %s" % type(volume).__name__)
        if intonation is not None and not isinstance(intonation, (bool, Intonation)):
            raise ValueError("intonation must be True or a pipeline.Intonation, got %s" % type(intonation).__name__)
        if isinstance(intonation, Intonation) and intonation.B != B:
            raise ValueError("intonation must be a pipeline.Intonation of %d rows" % B)
        self.model = model
        self.sampler = sampler.sampler if isinstance(sampler, GraphedSampler) else sampler  # one graph, not two nested
        dev = torch.device(device) if device is not None else next(model.decoder.parameters()).device
        if not _engine_path(dev):
            raise ValueError("GraphedSynthesis needs the C++ engine path (HIP device, plan_mode 'engine')")
        self.device, self.max_frames, self.steps = dev, int(max_frames), int(diffusion_steps)
        self.passage, self.max_gap = bool(passage), None if max_gap is None else int(max_gap)
        level = Level(B, device=dev) if level is True else None if level is False else level
        edges = Edges(B, device=dev) if edges is True else None if edges is False else edges
        if max_break_ms is not None and not breaks:
            raise ValueError("max_break_ms bounds `breaks`: pass breaks=True")
        if breaks is True:
            breaks = Breaks(B, N, device=dev, **({} if max_break_ms is None else {"max_ms": max_break_ms}))
        elif breaks is False:
            breaks = None
        elif isinstance(breaks, Breaks) and max_break_ms is not None and Edges.samples(max_break_ms) != breaks.max_break:
            raise ValueError("max_break_ms=%r is not the cap of the Breaks given (%r ms)" % (max_break_ms, breaks.max_ms))
        dynamics = Dynamics(B, device=dev) if dynamics is True else None if dynamics is False else dynamics
        if volume is False:
            volume = None
        elif volume is not None:  # recorded over tables of its own, 0 dB everywhere: only the ramp of a `Volume` given is taken
            volume = Volume.neutral(B, N, device=dev, **({} if volume is True else volume.options()))
        # the output as `inference` will judge it at every recording, over the static gaps: device gaps with `max_gap`
        gaps = None if max_gap is None else torch.zeros((B,), device=dev, dtype=torch.int32)
        spec, _ = _output_spec(B, True, pack, trim, sample_rate, marks, gaps, max_gap, level, graph=True, passage=self.passage,
                               **({} if edges is None else {"edges": edges}),
                               **({} if breaks is None else {"breaks": breaks}),
                               **({} if dynamics is None else {"dynamics": dynamics}),
                               **({} if volume is None else {"volume": volume, "device": dev}),
                               **({} if breaks is None and volume is None else {"N": N}))
        if spec.rate is not None:
            resample.table(spec.rate, dev)
        if level is not None and level.true_peak:
            resample.true_peak_table(dev)  # as the rate's table: made before the capture that reads it
        if level is not None and level.limiter:
            resample.limit_window(level.W, dev)  # and the limiter's window
        if edges is not None and edges.F:
            resample.edge_ramp(edges.F, dev)  # and the fade of a cut edge
        if breaks is not None and breaks.F:
            resample.edge_ramp(breaks.F, dev)  # and that of a pause's two sides
        if dynamics is not None and dynamics.A:
            resample.limit_window(dynamics.A, dev)  # and the compressor's look-ahead window
        if volume is not None and volume.A:
            resample.limit_window(volume.A, dev)  # and the ramp of the gains
        self.kw = dict(diffusion_steps=self.steps, embedding_scale=embedding_scale, alpha=alpha, beta=beta, lj_tail=lj_tail,
                       max_frames=self.max_frames, pack=pack, trim=trim, sample_rate=sample_rate, marks=bool(marks),
                       max_gap=self.max_gap, t=t)
        z = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.float32)
        drawn = None if seeds else True  # a seeded graph has no noise buffers: `inference(seeds=)` draws into its own
        self.static = dict(tokens=torch.zeros((B, N), device=dev, dtype=torch.int64),
                           lengths_dev=torch.full((B,), N, device=dev, dtype=torch.int32), noise=drawn and z(B, 1, 256),
                           step_noise=drawn and z(max(self.steps - 1, 0), B, 1, 256),
                           sine_noise=drawn and z(B, 600 * self.max_frames, 9),
                           ref_s=None if ref_s is None else ref_s.detach().to(dev, torch.float32).reshape(-1, 256)
                           .expand(B, -1).contiguous())
        if seeds:
            self.static["seeds"] = torch.zeros((B,), device=dev, dtype=torch.int64)
        if fit:
            self.static.update(fit_frames=torch.zeros((B,), device=dev, dtype=torch.int32),
                               fit_hold=torch.zeros((B, N), device=dev, dtype=torch.uint8))
        tok = bool(marks) if token_controls is None else bool(token_controls)
        self.static["controls"] = Controls.neutral(B, device=dev, N=N if tok else None)  # NaN weights: the call's own scalars
        self._neutral = self.static["controls"].buf.clone()
        self._neutral_tok = self.static["controls"].tok_buf.clone() if tok else None
        if intonation is not None and intonation is not False:
            own = {} if intonation is True else dict(K=intonation.K, voiced_hz=intonation.voiced_hz)
            self.static["intonation"] = Intonation.neutral(B, N=N if tok else None, device=dev, **own)
        if self.passage:
            starts = torch.zeros((B,), device=dev, dtype=torch.int32)
            starts[:1] = 1
            self.static.update(starts=starts, s_prev=z(1, 256))
        if gaps is not None:
            self.static["gaps"] = gaps
        if level is not None:
            self.static["level"] = Level(B, target=level.target.to(dev).clone(), ceiling_db=level.ceiling_db,
                                         max_gain_db=level.max_gain_db, device=dev, **level.options())
        if edges is not None:
            self.static["edges"] = Edges(B, top_db=edges.top_db.to(dev).clone(), device=dev, **edges.options())
        if breaks is not None:
            self.static["breaks"] = Breaks(B, N, samples=breaks.samples.to(dev).clone(), device=dev, **breaks.options())
        if dynamics is not None:
            own = self.static["dynamics"] = dynamics.slice(0, B)
            own.params = dynamics.params.to(dev).clone()
        if volume is not None:
            self.static["volume"] = volume
        self._g = None

    def _run(self):
        st = self.static  # a buffer the graph was built without is None here, as in a call that leaves the argument out
        return inference(self.model, self.sampler, st["tokens"], noise=st["noise"], step_noise=st["step_noise"],
                         sine_noise=st["sine_noise"], ref_s=st["ref_s"], lengths_dev=st["lengths_dev"],
                         controls=st["controls"], passage=st.get("starts"), s_prev=st.get("s_prev"), gaps=st.get("gaps"),
                         level=st.get("level"), **self.kw, **({"seeds": st["seeds"]} if "seeds" in st else {}),
                         **({"fit_frames": st["fit_frames"], "fit_hold": st["fit_hold"]} if "fit_frames" in st else {}),
                         **({"edges": st["edges"]} if "edges" in st else {}),
                         **({"breaks": st["breaks"]} if "breaks" in st else {}),
                         **({"dynamics": st["dynamics"]} if "dynamics" in st else {}),
                         **({"intonation": st["intonation"]} if "intonation" in st else {}),
                         **({"volume": st["volume"]} if "volume" in st else {}))

    def _engines(self):
        engs = model_engines(self.model, self.device)
        return [engs["front"], engs["decoder"]]

    def _record(self):
        graph, out = _record_graph(self._run, self.device)
        engs = self._engines()
        return dict(graph=graph, out=out, gen=_sampler_generation(self.sampler), engines=[(e, e.calib_gen) for e in engs])

    @torch.no_grad()
    def __call__(self, tokens=None, lengths=None, noise=None, step_noise=None, sine_noise=None, ref_s=None, controls=None,
                 starts=None, s_prev=None, gaps=None, level=None, seeds=None, fit_frames=None, fit_hold=None, edges=None,
                 breaks=None, dynamics=None, intonation=None, volume=None):
        st = self.static
        if volume is not None and "volume" not in st:
            raise ValueError("this graph was built without volume: pass volume=True")
        if "volume" in st:
            own = st["volume"]
            if volume is not None:
                if not isinstance(volume, Volume) or volume.B != own.B or volume.N not in (None, own.N):
                    raise ValueError("volume must be a pipeline.Volume of %d rows of %d tokens" % (own.B, own.N))
                if volume.options() != own.options():
                    raise ValueError("ramp_ms is the graph's own (%r); the Volume given has %r" % (own.options(), volume.options()))
        if intonation is not None and "intonation" not in st:
            raise ValueError("this graph was built without intonation: pass intonation=True")
        if "intonation" in st:
            own = st["intonation"]
            if intonation is not None:
                if not isinstance(intonation, Intonation) or intonation.B != own.B:
                    raise ValueError("intonation must be a pipeline.Intonation of %d rows" % own.B)
                if (intonation.K, intonation.voiced_hz) != (own.K, own.voiced_hz):
                    raise ValueError("K and voiced_hz are the graph's own (%r); the Intonation given has %r"
                                     % ((own.K, own.voiced_hz), (intonation.K, intonation.voiced_hz)))
                if intonation.tok_range is not None and own.tok_range is None:
                    raise ValueError("per-token ranges need a graph built with token_controls=True (or marks=True)")
                if intonation.tok_range is not None and intonation.N != own.N:
                    raise ValueError("intonation holds per-token rows of %d tokens, this graph's are %d wide" % (intonation.N, own.N))
            for name, absent in (("range", 1.0), ("contour", float("nan")), ("tok_range", 1.0)):
                mine, given = getattr(own, name), None if intonation is None else getattr(intonation, name)
                if mine is not None:
                    mine.fill_(absent) if given is None else mine.copy_(given, non_blocking=True)
        if fit_frames is not None or fit_hold is not None:
            if "fit_frames" not in st:
                raise ValueError("this graph was built without fit: pass fit=True")
            rows, hold = _check_fit(st["fit_frames"] if fit_frames is None else fit_frames, fit_hold, *st["fit_hold"].shape,
                                    self.max_frames)  # as `inference` judges them; a hold alone goes with the targets held here
            if fit_frames is not None:
                st["fit_frames"].copy_(rows if torch.is_tensor(rows) else torch.tensor(rows, dtype=torch.int32), non_blocking=True)
            if hold is not None:
                st["fit_hold"].copy_(hold, non_blocking=True)
        if "seeds" in st and (noise is not None or step_noise is not None or sine_noise is not None):
            raise ValueError("this graph draws noise, step_noise and sine_noise from its seeds: pass seeds, one or the other")
        if seeds is not None:
            if "seeds" not in st:
                raise ValueError("this graph was built without seeds: pass seeds=True")
            rows = seed_rows(seeds, st["seeds"].numel())
            st["seeds"].copy_(rows if torch.is_tensor(rows) else torch.tensor(rows, dtype=torch.int64), non_blocking=True)
        built_by = dict(starts="passage=True", s_prev="passage=True", gaps="max_gap")  # the buffers a plain graph lacks
        for name, val in (("starts", starts), ("s_prev", s_prev), ("gaps", gaps), ("tokens", tokens), ("lengths_dev", lengths),
                          ("noise", noise), ("step_noise", step_noise), ("sine_noise", sine_noise), ("ref_s", ref_s)):
            if val is None:
                continue
            if st.get(name) is None:
                raise ValueError("this graph was built without %s" % name + (": pass %s" % built_by[name] if name in built_by else ""))
            if name in built_by:  # host lists too
                val = torch.as_tensor(val)
                if val.numel() != st[name].numel():
                    raise ValueError("%s must hold %d values, got %d" % (name, st[name].numel(), val.numel()))
            elif name == "sine_noise":
                val = val[:, :st[name].shape[1]]
            st[name].copy_(val.reshape(st[name].shape), non_blocking=True)
        if level is not None:
            if st.get("level") is None:
                raise ValueError("this graph was built without level: pass level=True")
            row = level.target if isinstance(level, Level) else Level.row(level, st["level"].B)
            if row.numel() != st["level"].B:
                raise ValueError("level must hold %d targets, got %d" % (st["level"].B, row.numel()))
            st["level"].target.copy_(row, non_blocking=True)
        if edges is not None:
            if st.get("edges") is None:
                raise ValueError("this graph was built without edges: pass edges=True")
            row = edges.top_db if isinstance(edges, Edges) else Edges.row(edges, st["edges"].B)
            if row.numel() != st["edges"].B:
                raise ValueError("edges must hold %d thresholds, got %d" % (st["edges"].B, row.numel()))
            st["edges"].top_db.copy_(row, non_blocking=True)
        if breaks is not None:
            if st.get("breaks") is None:
                raise ValueError("this graph was built without breaks: pass breaks=True")
            own = st["breaks"]
            if isinstance(breaks, Breaks) and (breaks.B, breaks.N) != (own.B, own.N):
                raise ValueError("breaks must be a pipeline.Breaks of %d rows of %d tokens" % (own.B, own.N))
            table = breaks.samples if isinstance(breaks, Breaks) else Breaks.table(None, breaks, own.B, own.N)
            own.samples.copy_(table, non_blocking=True)
        if dynamics is not None:
            if st.get("dynamics") is None:
                raise ValueError("this graph was built without dynamics: pass dynamics=True")
            own = st["dynamics"]
            if not isinstance(dynamics, Dynamics) or dynamics.B != own.B:
                raise ValueError("dynamics must be a pipeline.Dynamics of %d rows" % own.B)
            if dynamics.options() != own.options():
                raise ValueError("attack_ms and release_db_per_s are the graph's own (%r); the Dynamics given has %r"
                                 % (own.options(), dynamics.options()))
            own.params.copy_(dynamics.params, non_blocking=True)
        if controls is not None:
            if not isinstance(controls, Controls) or controls.B != st["controls"].B:
                raise ValueError("controls must be a pipeline.Controls of %d rows" % st["controls"].B)
            if controls.tok_present and self._neutral_tok is None:
                raise ValueError("per-token controls need a graph built with token_controls=True (or marks=True)")
            if controls.tok_buf is not None and self._neutral_tok is not None and controls.N != st["controls"].N:
                raise ValueError("controls hold per-token rows of %d tokens, this graph's token_controls are %d wide"
                                 % (controls.N, st["controls"].N))
            st["controls"].buf.copy_(controls.buf, non_blocking=True)  # an absent row holds its neutral value
        else:
            st["controls"].buf.copy_(self._neutral, non_blocking=True)
        if self._neutral_tok is not None:
            has_tok = controls is not None and controls.tok_buf is not None
            st["controls"].tok_buf.copy_(controls.tok_buf if has_tok else self._neutral_tok, non_blocking=True)
        if "volume" in st:  # judged at the top; written here, behind every refusal of the call
            for name in ("db", "tok_db"):
                given = None if volume is None else getattr(volume, name)
                getattr(st["volume"], name).zero_() if given is None else getattr(st["volume"], name).copy_(given, non_blocking=True)
        g = self._g
        if g is not None and (g["gen"] != _sampler_generation(self.sampler)
                              or any(_engine_changed(e, rec, gen) for e, (rec, gen) in zip(self._engines(), g["engines"]))):
            g = None
        if g is None:
            g = self._g = self._record()
        g["graph"].replay()
        return g["out"]


def _decode_groups(model, groups, dec, main, noise_of, ready=None, first=0):
    """One decoder call per frame-count group `(idx, g)` of a prepared batch, in the groups' order -> (idx, wave [len(idx), 1,
    600 T], event or None) per group.  `dec`: the auxiliary decoder streams (empty: every call runs on the current stream);
    `main`: the caller's stream when streams are in play at all, else None (nothing is handed over); `noise_of(idx, g)`: the
    group's SineGen draws.

    * Group n of the CALL SEQUENCE goes to dec[n % len(dec)]: `first` is the number of groups decoded before these, so that the
      round-robin runs on across the front calls of a passage.
    * The decoder's stream waits for the group's own `ready` event where `prepare(group_events=True)` recorded one, else for
      `ready` (the front call's); with neither the caller has ordered the streams already (`inference`: they wait for `main`).
    * The noise rows are stacked on the stream that reads them, i.e. inside the stream block: stacked on the caller's stream
      they raced the decoder (r05r).
    * A wave made on a decoder stream is marked as in use on `main`, which takes it over behind the returned event.
    * With decoder streams NOTHING is yielded before every decoder of `groups` has been queued, so the caller's stream takes its
      per-group waits only after that.  A wait packet sits at the head of the caller's hardware queue until its decoder is
      done, and HIP multiplexes streams onto ~4 such queues: an auxiliary stream that shares the caller's queue had its NEXT
      decoder queued behind that wait -- the decoders serialised, and a passage took 74-114 ms instead of 52 depending on
      which streams the process happened to get (rounds 5-6: "stream roulette").  Queued last, the waits block nothing.
      Without decoder streams every group is yielded as soon as it is queued: a consumer (`on_chunk`) sees it at once."""
    queued = []
    for n, (idx, g) in enumerate(groups, first):
        ds = dec[n % len(dec)] if dec else main
        if main is not None:
            _hand_off(_decoder_inputs(g), ds, g.get("ready", ready))
        if not dec:
            yield idx, model.decoder(g["asr"], g["F0"], g["N"], g["ref"], noise=noise_of(idx, g)), None
            continue
        with torch.cuda.stream(ds):
            w = model.decoder(g["asr"], g["F0"], g["N"], g["ref"], noise=noise_of(idx, g))
            ev = torch.cuda.Event()
            ev.record(ds)
        w.record_stream(main)
        queued.append((idx, w, ev))
    yield from queued


def _check_capacity_args(tokens, max_frames, lengths_dev, passage, s_prev, controls, taps, front, durations, decode_streams):
    """What `inference` refuses about the arguments of the capacity-bound path that are not about the output (`_output_spec`,
    which it calls first), before anything is launched, and what it settles on the way -> (carry, controls): whether the rows
    are a passage, and the controls with the start flags of `passage=[...]` in their `t` row."""
    if max_frames is None:
        _capacity_only("passage / gaps / max_gap / s_prev", passage, s_prev)
        _capacity_only("pack / trim / lengths_dev", lengths_dev)
    carry = passage is not None and passage is not False
    if s_prev is not None and not carry:
        raise ValueError("s_prev is the style a passage continues from: pass passage")
    if carry and passage is not True:
        if controls is not None:
            _check_controls(controls, tokens.device, tokens.shape[0], taps, front, durations, tokens.shape[1])
        controls = _passage_controls(controls, passage, tokens.shape[0], tokens.device)
    if max_frames is not None and decode_streams:
        raise ValueError("max_frames: there is ONE decoder call, on the current stream; `decode_streams` has no meaning here")
    return carry, controls


def seed_rows(seeds, K):
    """`seeds` of K rows as the host list of K ints a sequence gives, or the int64 [K] device tensor as it is.  One int s means
    s, s + 1, ..., s + K - 1, wrapping from 2^63 - 1 to -2^63 (the seed is 64 bits, read as unsigned by the generator)."""
    if isinstance(seeds, int) and not isinstance(seeds, bool):
        seeds = [(seeds + k + 2 ** 63) % 2 ** 64 - 2 ** 63 for k in range(K)]
    if torch.is_tensor(seeds):
        if seeds.dtype != torch.int64 or seeds.dim() != 1 or seeds.numel() != K:
            raise ValueError("seeds must be an int64 tensor of %d entries, got %s %s" % (K, seeds.dtype, tuple(seeds.shape)))
        return seeds if seeds.is_cuda else seeds.tolist()
    seeds = list(seeds)
    if len(seeds) != K or not all(isinstance(v, int) and not isinstance(v, bool) and -2 ** 63 <= v < 2 ** 63 for v in seeds):
        raise ValueError("seeds must be %d whole numbers in the int64 range, got %r" % (K, seeds))
    return seeds


def _check_seeds(seeds, B, max_frames, noise, step_noise, sine_noise):
    """What `inference` refuses about `seeds` (an input, not an output option: DESIGN.md section 25), before anything is
    launched -> the seeds as `seed_rows` gives them."""
    if max_frames is None:
        _capacity_only("seeds", seeds)
    if noise is not None or step_noise is not None or sine_noise is not None:
        raise ValueError("seeds draw noise, step_noise and sine_noise on the device: pass one or the other")
    return seed_rows(seeds, B)


def _seeds_on(seeds, dev):
    return seeds if torch.is_tensor(seeds) else torch.tensor(seeds, dtype=torch.int64).to(dev, non_blocking=True)


def _seeded_front_noise(seeds, B, steps, dev):
    """The sampler's start noise [B, 1, 256] and its per-step draws [steps - 1, B, 1, 256] under `seeds`: two launches."""
    e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    return (ops.noise_fill(seeds, e(B, 1, 256), ops.NOISE_SAMPLER),
            ops.noise_fill(seeds, e(max(steps - 1, 0), B, 1, 256), ops.NOISE_STEP, streams=max(steps - 1, 0)))


def _seeded_sine_noise(seeds, frames, max_frames):
    """The harmonic source's draws [B, 600 max_frames, 9] under `seeds`: one launch behind the front, which writes row b's
    600 frames[b] * 9 values and no more -- the ragged source kernel reads no further (st2_har_source_len)."""
    out = torch.empty((seeds.numel(), 600 * int(max_frames), 9), device=seeds.device, dtype=torch.float32)
    return ops.noise_fill(seeds, out, ops.NOISE_SINE, counts=frames, per_count=600 * 9)


def fit_frames(seconds, trim=0):
    """A length of `seconds` as the frame target of `inference(fit_frames=)`: round((24000 seconds +
    trim) / 600), ties to even, at least 1 -- the row then hands over 600 T - `trim` samples at 24 kHz, `trim` being the
    samples the hand-over drops from the row's end (`inference(trim=)`: by default 50 for a HiFi-GAN decoder, 0 for iSTFTNet).
    One frame is 600 samples, 25 ms: that is the granularity, a target lands within 12.5 ms of the length asked for.  What is
    fitted is everything the durations hold: the LJSpeech flow's five tail frames on the last token and forced `durations=`
    are part of the total.  A scalar gives an int, a sequence a list."""
    one = lambda s: max(int(round((resample.MODEL_RATE * float(s) + trim) / 600.0)), 1)
    return one(seconds) if isinstance(seconds, (int, float)) else [one(s) for s in seconds]


def _check_fit(fit_frames, fit_hold, B, N, max_frames):
    """What `inference` refuses about `fit_frames` / `fit_hold` (inputs, not output options: DESIGN.md section 26), before
    anything is launched -> (the targets as a host list of B ints or the int32 [B] device tensor as it is, fit_hold).  A host
    list is judged here -- no negative entry, none above `max_frames` --; a device tensor is never read: the kernel clamps its
    entries to what is feasible and says so in the report's flag."""
    if max_frames is None:
        _capacity_only("fit_frames / fit_hold", fit_frames, fit_hold)
    if fit_frames is None:
        raise ValueError("fit_hold marks the tokens that fit_frames leaves as they are: pass fit_frames")
    if torch.is_tensor(fit_frames) and fit_frames.is_cuda:
        if fit_frames.dtype != torch.int32 or fit_frames.dim() != 1 or fit_frames.numel() != B:
            raise ValueError("fit_frames must be an int32 tensor of %d entries, got %s %s" % (B, fit_frames.dtype, tuple(fit_frames.shape)))
    else:
        rows = fit_frames.tolist() if torch.is_tensor(fit_frames) and fit_frames.dim() == 1 else fit_frames
        rows = list(rows) if isinstance(rows, (list, tuple)) else None
        if rows is None or len(rows) != B or not all(isinstance(v, int) and not isinstance(v, bool) for v in rows):
            raise ValueError("fit_frames must be %d whole frame counts (pipeline.fit_frames converts seconds), got %r" % (B, fit_frames))
        if any(v < 0 or v > int(max_frames) for v in rows):
            raise ValueError("fit_frames must lie in 0..max_frames = %d (0 leaves the row alone), got %r" % (int(max_frames), rows))
        fit_frames = rows
    if fit_hold is not None and (not torch.is_tensor(fit_hold) or not fit_hold.is_cuda or fit_hold.dtype not in (torch.bool, torch.uint8)
                                 or tuple(fit_hold.shape) != (B, N)):
        raise ValueError("fit_hold must be a bool / uint8 device tensor of shape [%d, %s], got %s" % (
            B, N, "%s %s on %s" % (fit_hold.dtype, tuple(fit_hold.shape), fit_hold.device) if torch.is_tensor(fit_hold)
            else type(fit_hold).__name__))
    return fit_frames, fit_hold


def _fit_on(fit, dev):
    """`_check_fit`'s pair with the targets on the device: what `prepare(fit=)` takes."""
    rows, hold = fit
    rows = rows if torch.is_tensor(rows) else torch.tensor(rows, dtype=torch.int32).to(dev, non_blocking=True)
    return rows, None if hold is None else hold.contiguous()


@torch.no_grad()
def inference(model, sampler, tokens, input_lengths=None, noise=None, diffusion_steps=5, embedding_scale=1.0,
              ref_s=None, alpha=0.3, beta=0.7, durations=None, step_noise=None, sine_noise=None, lj_tail=None,
              taps=None, front_stream=None, inputs_on_main=False, total_frames=None, front=None, decode_streams=None,
              ragged_decode=False, max_frames=None, pack=None, trim=None, lengths_dev=None, controls=None,
              sample_rate=None, marks=False, passage=None, gaps=None, max_gap=None, s_prev=None, t=0.7, level=None,
              seeds=None, fit_frames=None, fit_hold=None, edges=None, breaks=None, dynamics=None, intonation=None, volume=None):
    """tokens [B, N] int64 (id 0 prepended, ipynb:277) -> waveform [B, 1, 600*T] on the device.

    Single-speaker (LJSpeech) when `ref_s` is None, else the multi-speaker flow with style mixing
    (Demo/Inference_LibriTTS.ipynb:285-286).  The decoder's InstanceNorm spans the whole utterance, so padding frames
    would change results (section 7.3-6): utterances whose (predicted) durations sum to different frame counts are
    decoded in one decoder call per distinct frame count and the result is then a LIST of B waveforms [1, 600*T_b] in
    utterance order; a batch of equal frame counts (forced `durations`, throughput runs) returns one tensor.  A
    right-padded batch (`input_lengths`) gives every utterance the result of its own un-padded run.

    `front_stream` (a torch.cuda.Stream): everything in front of the decoder is issued on that stream and handed to
    the decoder (on the current stream) through an event.  A caller that synthesises batch after batch thereby
    overlaps batch k+1's front -- a long chain of small, latency-bound kernels (BiLSTM recurrences on 64 CUs, 100-token
    transformer layers) -- with batch k's decoder, whose big convolutions fill whatever CUs the front leaves idle.
    Results are identical to the single-stream call.  The caller's input tensors must be complete when the front
    stream reaches them: inputs resident from earlier synchronised work (the bench, a server's staging buffers) need
    nothing; inputs still being produced on the CURRENT stream (a per-call torch.randn, an async H2D copy) need
    `inputs_on_main=True`, which makes the front stream wait for the current stream first -- at the price of also
    waiting for the previous call's decoder queued there, i.e. of the overlap.

    `decode_streams` (a list of torch streams; ragged batches only): the per-frame-count decoder calls -- independent of each
    other, one utterance each for real text -- are dealt round-robin onto these streams instead of running one after the other
    on the current one; the current stream waits for all of them before the call returns.  One utterance's decoder launches
    grids of 2 x 23 tiles for 256 CUs: two or three of them fill each other's idle CUs (the long-form path does the same,
    `synthesize_long(decode_streams=)`).  Bitwise the sequential result.

    `ragged_decode=True`: a batch of different frame counts takes ONE ragged prosody call and ONE ragged decoder call
    (`prepare(ragged_decode=True)`) instead of one pair per frame count; the waveforms come back as the
    same list, each row sliced to its own 600 T_b samples (`decode_streams` is then moot).

    `max_frames` (int): the sync-free path (`prepare(max_frames=)`): the caller states the capacity in
    decoder frames, the host reads nothing back, ONE ragged prosody and ONE ragged decoder call run at T = max_frames, and the
    return value is a `SynthesisResult`: `wave` [B, 1, 600 max_frames] with exact zeros past each row's 600 frames[b] samples
    and `frames` (int32 [B] on the device).  `sine_noise`, if given, is [B, >= 600 max_frames, 9] (handed over as a view; each
    row is read up to 600 frames[b] only); absent, it is drawn on the device at capacity.  `pack` ("s16" / "f32"): the result also
    carries `packed` (every row's valid samples back to back: 16-bit PCM or fp32, `ops.wave_pack`) and `offsets` (int64 [B + 1],
    device); `trim` samples are dropped from every row's end -- by default the notebooks' rule, 50 for a HiFi-GAN decoder and 0
    for iSTFTNet.  `pack` also takes "ulaw" / "alaw" (ITU-T G.711 bytes) and `sample_rate` (with `pack` only) one of 8000, 16000,
    22050, 24000, 32000, 44100 and 48000: the packing step then resamples on the device (`ops.wave_resample_pack`, DESIGN.md
    section 15) and `packed` holds ceil(n_b U / D) samples per row at that rate; fp32 / 16-bit PCM at 24 kHz is the path above,
    unchanged.  `result.to_host()` is the one place that waits.  `lengths_dev` (int32 [B] on the device): the token counts of
    a right-padded batch without any host copy (stream capture, `GraphedSynthesis`).  `decode_streams` and `total_frames` are
    refused with `max_frames`.

    `controls` (a `Controls`): per-row speaking rate, style mixing weights, pitch scale and energy shift, and their per-token
    forms, see `prepare`.

    `marks=True` (with `max_frames` and `pack`): the result also carries `marks`, int32 [B, N + 1] on the
    device -- where every token starts among its row's packed samples -- from one more launch (`ops.token_marks`);
    `result.to_host(marks=True)` brings them over in its one copy.

    `passage` (with `max_frames`): True -- the B rows are consecutive sentences of ONE passage: row k's
    sampled style is mixed with row k-1's mixed style with weight `t` (`prepare(carry=True)`), and `s_prev` ([1, 256] or None)
    feeds row 0.  A [B] host sequence or device tensor of start flags -- one batch, several passages: every flagged row begins a
    new one (its mixing weight is 0, through the `Controls` `t` row); row 0 begins one unless `s_prev` is given.  A device
    tensor is never read on the host.  `result.style[-1:]` is the `s_prev` of the call that continues the passage.
    `gaps` (with `max_frames` and `pack`): per-row samples of silence behind every row, at the hand-over's rate and in its format
    (`ops.wave_pack_gaps`; `gap_samples(ms, sample_rate)` converts milliseconds) -- an int32 [B] device tensor, which needs
    `max_gap` (the packing step clamps to 0..max_gap and sizes its allocation by it), or a host list, whose maximum is the
    default.  `marks` stay relative to their row (`SynthesisResult`).

    `level` (a `Level` of B rows, with `max_frames` and `pack`): every row is measured on the device
    (`ops.wave_level`: BS.1770-4 integrated loudness and sample peak) and packed with the gain that brings it to its target
    loudness under the peak ceiling (`ops.wave_pack_level`); the result carries the table as `level` and `to_host(level=True)`
    brings it over in its one copy.  `wave` stays as the decoder made it, marks and sample counts do not move.

    `seeds` (with `max_frames`): one int64 seed per row -- an int64 [B] device tensor, never read on the
    host, or a host sequence of B ints -- instead of `noise`, `step_noise` and `sine_noise` (one or the other): the three are
    drawn on the device by `ops.noise_fill`, three launches, under the noise stream ids of include/st2.h.  A row's draws depend
    on its seed alone: the same seed gives the same draws in any batch and at any place in it.  Without `seeds` the call
    issues exactly the launches it always did.

    `fit_frames` (with `max_frames`): "say this in exactly T frames" -- a host sequence of B whole frame
    counts, or an int32 [B] device tensor, which is never read on the host; 0 leaves the row alone (`pipeline.fit_frames`
    converts seconds).  One launch (`ops.durations_fit`) between the front and the frame counts rewrites every row's integer
    durations -- predicted or forced -- to its target by largest-remainder apportionment of the excess over one frame per
    token; the frame counts, the expansion, the marks, the per-token prosody spans and the result's `durations` all follow.
    `fit_hold` (bool / uint8 [B, N] on the device): tokens that keep their duration.  A host target is refused when it is
    negative or above `max_frames`; a feasible target (at least one frame per free token plus the held ones) is met exactly,
    any other is replaced by the nearest feasible total.  The result carries `fit`, int32 [B, 4]: {frames before, frames
    after, flag, tokens changed} per row.  Without the two arguments the call issues exactly the launches it always did.

    `edges` (an `Edges` of B rows, with `max_frames` and `pack`): the silence the model makes in front of and
    behind every row's speech is trimmed on the device (`ops.wave_edges`, the first step of the hand-over), so that `gaps` are
    the pauses a listener hears and `marks[b, 0]` / `marks[b, N]` bracket speech.  Level, limiter, gaps, resampling and G.711 run
    over the cut rows; the result carries {head, count} as `edges` and `to_host(edges=True)` brings them over in its one copy.
    `wave` stays as the decoder made it.  Without `edges` the call issues exactly the launches it always did.

    `breaks` (a `Breaks` of B rows of N tokens, with `max_frames` and `pack`): pauses INSIDE the rows --
    `breaks.samples[b, n]` samples of digital silence at 24 kHz inside token n of row b, spliced in on the device at the quietest
    place of that token's samples, both sides faded (`ops.wave_breaks`, behind the trim of `edges` and in front of everything
    else of the hand-over).  The marks are those of the rows with their pauses: token n's pause lies inside [marks[b, n],
    marks[b, n + 1]).  The result carries {samples with the pauses, silence inserted} as `breaks`.  `fit_frames` keeps meaning
    frames of speech: the pauses come on top.  Without `breaks` the call issues exactly the launches it always did.

    `dynamics` (a `Dynamics` of B rows, with `max_frames` and `pack`): a compressor over every row, on the
    device (`ops.wave_dynamics`, behind `breaks` and in front of `level`, so a loudness target holds on the compressed programme
    and the limiter sees compressed peaks).  No sample moves: marks, gaps, resampling and G.711 run unchanged.  The result carries
    {deepest reduction in dB, blocks reduced} as `dynamics`.  Without it the call issues exactly the launches it always did.

    `intonation` (an `Intonation` of B rows; with and without `max_frames`): per-row pitch range, per-token
    range and pitch contour on the device, see `prepare`; on the capacity-bound path the result carries the report as `pitch`.
    Without it the call issues exactly the launches it always did.

    `volume` (a `Volume` of B rows, with `max_frames` and `pack`): SSML's `<prosody volume=>` -- one gain in
    dB per row and one per token, ramped over `ramp_ms`, on the device (`ops.wave_volume`, behind `dynamics` and in front of
    `level`, over the tokens' boundaries as `edges` and `breaks` left them).  No sample moves: marks, gaps, resampling and G.711
    run unchanged; a stretch at 0 dB keeps its bits.  The result carries {peak, blocks with a gain} as `volume`.  Under a
    `Level` of scope "row" the row's own `db` is cancelled by the normalisation and the differences between tokens survive;
    under scope "passage" a quiet sentence stays quiet beside its neighbours.  `emphasis_tables` makes the per-token tables of
    `<emphasis>`.  Without it the call issues exactly the launches it always did.
    """
    if intonation is not None:
        _check_intonation(intonation, tokens.device, tokens.shape[0], taps, front, tokens.shape[1])
    spec, gaps = _output_spec(tokens.shape[0], max_frames is not None, pack, trim, sample_rate, marks, gaps, max_gap, level,
                              passage=passage, **({} if edges is None else {"edges": edges}),
                              **({} if breaks is None else {"breaks": breaks}),
                              **({} if dynamics is None else {"dynamics": dynamics}),
                              **({} if volume is None else {"volume": volume, "device": tokens.device}),
                              **({} if breaks is None and volume is None else {"N": tokens.shape[1]}))
    carry, controls = _check_capacity_args(tokens, max_frames, lengths_dev, passage, s_prev, controls, taps, front, durations,
                                           decode_streams)
    if seeds is not None:
        seeds = _seeds_on(_check_seeds(seeds, tokens.shape[0], max_frames, noise, step_noise, sine_noise), tokens.device)
    fit = None
    if fit_frames is not None or fit_hold is not None:
        fit = _fit_on(_check_fit(fit_frames, fit_hold, tokens.shape[0], tokens.shape[1], max_frames), tokens.device)
    kw = dict(input_lengths=input_lengths, noise=noise, diffusion_steps=diffusion_steps,
              embedding_scale=embedding_scale, ref_s=ref_s, alpha=alpha, beta=beta, durations=durations,
              step_noise=step_noise, lj_tail=lj_tail, taps=taps, allow_ragged=True, total_frames=total_frames,
              front=front, ragged_decode=ragged_decode, controls=controls)
    if max_frames is not None:
        kw.update(max_frames=max_frames, lengths_dev=lengths_dev)
    if carry:
        kw.update(carry=True, s_prev=s_prev, t=t)
    if fit is not None:
        kw.update(fit=fit)
    if intonation is not None:
        kw.update(intonation=intonation)
    seeded = lambda: {} if seeds is None else dict(zip(("noise", "step_noise"), _seeded_front_noise(
        seeds, tokens.shape[0], diffusion_steps, tokens.device)))  # drawn on the stream the front reads them on
    if front_stream is None:
        p = prepare(model, sampler, tokens, **dict(kw, **seeded()))
    else:
        main = torch.cuda.current_stream(tokens.device)
        if inputs_on_main or seeds is not None or fit is not None:  # (seeds / targets may just have been copied in on the current stream)
            front_stream.wait_stream(main)
        with torch.cuda.stream(front_stream):
            p = prepare(model, sampler, tokens, **dict(kw, **seeded()))
            ready = torch.cuda.Event()
            ready.record(front_stream)
        _hand_off([v for g in ([p] if "groups" not in p else [g for _, g in p["groups"]]) for v in _decoder_inputs(g)],
                  main, ready)  # allocated on the front stream, consumed on the main stream
    if seeds is not None:
        sine_noise = _seeded_sine_noise(seeds, p["frames"], max_frames)
    if max_frames is not None:
        return _decode_capacity(model, p, sine_noise, spec, gaps, level, passage, **({} if edges is None else {"edges": edges}),
                                **({} if breaks is None else {"breaks": breaks}),
                                **({} if dynamics is None else {"dynamics": dynamics}),
                                **({} if volume is None else {"volume": volume}))
    if "frames" in p:
        return _decode_ragged(model, p, sine_noise)
    if "groups" not in p:
        return model.decoder(p["asr"], p["F0"], p["N"], p["ref"], noise=sine_noise)
    waves = [None] * tokens.shape[0]
    dec = list(decode_streams) if decode_streams else []
    main = torch.cuda.current_stream(tokens.device) if dec else None
    for st in dec:
        st.wait_stream(main)  # the front's outputs (and the caller's inputs) are ordered on the current stream
    # every utterance's own draws, cut to the group's 600 T samples
    noise_of = lambda idx, g: None if sine_noise is None else torch.stack([sine_noise[b][:g["F0"].shape[1] * 300] for b in idx])
    for idx, w, ev in _decode_groups(model, p["groups"], dec, main, noise_of):
        for j, b in enumerate(idx):
            waves[b] = w[j]
        if ev is not None:
            main.wait_event(ev)
    return waves


def _front_chunks(front_batch, K):
    """`synthesize_long(front_batch=)` -> [(first sentence, one past the last)] per front call of a passage of K sentences: the
    chunk sizes in turn, the last one repeating; 0 / None = everything that is left."""
    sizes = list(front_batch) if isinstance(front_batch, (list, tuple)) else [front_batch]
    starts, i = [], 0
    while i < K:
        n = sizes[min(len(starts), len(sizes) - 1)]
        n = K - i if not n else max(1, min(int(n), K - i))
        starts.append((i, i + n))
        i += n
    return starts


def _decode_stream_list(decode_streams, use_streams, make):
    """`synthesize_long(decode_streams=)` -> the auxiliary decoder streams: a sequence of two or more streams as given, a count
    above 1 as that many of `make(0)`, `make(1)`, ...; none without `use_streams` or where one stream (the caller's) decodes."""
    if use_streams and isinstance(decode_streams, (list, tuple)):
        return list(decode_streams) if len(decode_streams) > 1 else []
    if use_streams and decode_streams and int(decode_streams) > 1:
        return [make(i) for i in range(int(decode_streams))]
    return []


def _stack_group(sentences, ids, npad, durations, noises, step_noises, ref_s, dev):
    """The inputs of ONE front call over the sentences `ids` of a passage, stacked at the token width `npad`: `tokens`
    right-padded with id 0 (the pad: text_utils / ipynb:277), `dur` (forced durations) zero-padded -- pad tokens get no frames --,
    `noise` / `step_noise` concatenated along their batch axis, `ref_s` repeated per row, and the sentences' token counts as
    `lengths` (host int64) and `lens_dev` (device int32), both None for a group no row of which is padded."""
    ns = [sentences[k].numel() for k in ids]
    tokens = torch.zeros((len(ids), npad), dtype=sentences[ids[0]].dtype, device=dev)
    for j, k in enumerate(ids):
        tokens[j, :ns[j]] = sentences[k].reshape(-1)
    dur = None
    if durations is not None:
        dur = torch.zeros((len(ids), npad), dtype=torch.long, device=dev)
        for j, k in enumerate(ids):
            dur[j, :ns[j]] = durations[k].reshape(-1).long().to(dev)
    lengths = torch.LongTensor(ns) if any(n != npad for n in ns) else None
    cat = lambda seq, dim: None if seq is None else torch.cat([seq[k] for k in ids], dim=dim)
    return dict(tokens=tokens, dur=dur, lengths=lengths, lens_dev=None if lengths is None else lengths.to(torch.int32).to(dev),
                noise=cat(noises, 0), step_noise=cat(step_noises, 1),
                ref_s=None if ref_s is None else ref_s.reshape(1, -1).expand(len(ids), -1).contiguous())


@torch.no_grad()
def synthesize_long(model, sampler, sentences, ref_s=None, alpha=0.3, beta=0.7, t=0.7, diffusion_steps=5,
                    embedding_scale=1.0, noises=None, step_noises=None, sine_noises=None, durations=None, trim=None,
                    overlap=True, on_chunk=None, bucket=0, front=None, side_stream=None, front_batch=1, decode_streams=1,
                    ragged_decode=False, controls=None, max_frames=None, pack=None, sample_rate=None, marks=False, gaps=None,
                    max_gap=None, level=None, seeds=None, fit_frames=None, edges=None, breaks=None, dynamics=None,
                    intonation=None, volume=None):
    """Long-form synthesis (BASELINE.json configs[4]; Demo/Inference_LibriTTS.ipynb LFinference + its driver loop,
    Demo/Inference_LJSpeech.ipynb "Long-form generation"): `sentences` is a list of token tensors [N_i] (id 0
    prepended); each sentence is synthesised with the previous sentence's mixed style carried over
    (`s_pred = t * s_prev + (1 - t) * s_pred`) and its waveform is handed out as soon as it is ready.

    The passage is sequential in the style vector only, and that vector is final before the sentence's decoder
    runs.  So the engine streams in two stages on two HIP streams: the front of sentence k+1 (text encoder, PL-BERT,
    diffusion, duration / prosody prediction; its one host sync is the predicted frame count) is issued on a side
    stream while the decoder + vocoder of sentence k (>= 2/3 of the sentence's time) still occupies the main stream;
    an event hands the decoder inputs over.  Returns (list of waveforms [600*T_i - trim], final style [1, 256]);
    `on_chunk(k, wave)` is called per sentence, in sentence order, for streaming consumers.  `trim` samples are dropped from
    every sentence's end as the notebooks do ("weird pulse at the end of the model": 100 multi-speaker, 0 single-speaker).

    `front_batch`: how many consecutive sentences share ONE front call.  1 = the notebooks' schedule, sentence by sentence
    (lowest time to the first waveform).  0 / None = the whole passage, n = groups of n, a sequence = those group sizes in turn
    with the last one repeating ((2, 0): the first two sentences, then the rest while their decoders run): the sentences' text encoder, PL-BERT,
    style diffusion and duration stages run as one right-padded batch (pad tokens masked everywhere: every row is the
    sentence's own un-padded result) with the style carry-over as a row scan in between (`_front_core(carry=True)`) -- a
    100-token sentence alone leaves its ~1 500 token GEMMs and BiLSTM steps latency-bound, ten of them fill the same
    launches.  The alignment expansion / prosody predictor and the decoder still run per sentence (their InstanceNorm
    spans the utterance), in sentence order, each waiting only for its own inputs.

    `decode_streams` > 1 (with `overlap`): the decoder calls are dealt round-robin onto that many auxiliary streams instead
    of the caller's.  One sentence's decoder is ~400 launches whose grids cover a fraction of the chip (2 x 23 tiles for 256
    CUs); with a batched front the next sentences' inputs are ready long before, so independent sentences' decoders fill each
    other's idle CUs.  The caller's stream waits for sentence k's decoder before `on_chunk(k, ...)` and for all of them before
    the call returns: the waveforms are ordered on the caller's stream exactly as before.  A list of torch streams is used as
    given: HIP multiplexes streams onto ~4 hardware queues in creation order, and two decoder streams that share a queue with
    each other or with the front's stream serialise (or worse: 113 ms against 65 on one stream) -- a serving process
    measures its candidates once at start-up, as bench.py does.

    `bucket` > 0: every sentence's token row is right-padded to a multiple of `bucket` (the pad tokens are masked
    everywhere: packed-sequence BiLSTMs, key-padded attention, length-aware mean -- results are those of the un-padded
    sentence), so that a `GraphedSampler` (models.make_sampler(graph=True)) replays ONE captured hipGraph per bucket
    instead of capturing one per sentence length.

    `ragged_decode=True`: every front group's sentences take ONE ragged prosody call and ONE ragged decoder call on the
    caller's stream (`prepare(ragged_decode=True)`) instead of one pair per distinct frame count;
    `decode_streams` is then moot.

    `controls` (a `Controls` of one row per SENTENCE): per-sentence speaking rate, mixing weights (`t` of row k weighs sentence
    k-1's style into sentence k), pitch scale and energy shift.  A front group's carry-over is then ONE launch
    (`st2_style_mix_rows`) instead of five per sentence.

    `max_frames` (int): the passage on the sync-free path.  Every front group is ONE
    `inference(max_frames=, passage=True, s_prev=<the previous group's style[-1:]>)` on the caller's stream: the token counts
    come from the sentences' shapes, nothing is read back, and the return value is (list of `SynthesisResult`, one per front
    group, final style [1, 256]); `on_chunk(k, result)` is called per GROUP.  `pack`, `sample_rate`, `marks` and `gaps` (one
    break per sentence: a host list, or an int32 device tensor with `max_gap`) are `inference`'s and need `max_frames`; so is
    `level` (a `Level` of one row per SENTENCE: every sentence is normalised on its own).
    `sine_noises` rows are stacked, zero-padded, to the capacity.  Per-token controls are served here: the rows are
    right-padded to the controls' width N, which must be the longest sentence's.  `decode_streams` > 1 is refused (there is one
    decoder call per group, on the caller's stream); `overlap`, `front`, `side_stream` and `ragged_decode` have no meaning.
    `seeds` (needs `max_frames`): one seed per SENTENCE -- K ints or an int64 [K] device tensor -- or one
    int s, which stands for s, s + 1, ..., s + K - 1 (wrapping from 2^63 - 1 to -2^63: the seed is 64 bits), instead of `noises`,
    `step_noises` and `sine_noises`: every sentence's noise is drawn on the device from its own seed (`inference(seeds=)`), the
    same draws whatever `front_batch` groups it with.
    `fit_frames` (needs `max_frames`): one frame target per SENTENCE -- K whole frame counts or an int32 [K]
    device tensor, 0 = leave the sentence alone --: every sentence's durations are fitted to its own target
    (`inference(fit_frames=)`); the breaks between sentences are not part of it.
    `edges` (needs `max_frames` and `pack`): an `Edges` of one row per SENTENCE: every sentence is cut to its
    speech (`inference(edges=)`), so that the breaks of `gaps` are the pauses between sentences.
    `breaks` (needs `max_frames` and `pack`): a `Breaks` of one row per SENTENCE, its N the longest sentence's
    token count -- shorter sentences are right-padded to it, as with per-token controls --: the pauses inside the sentences
    (`inference(breaks=)`).
    `dynamics` (needs `max_frames` and `pack`): a `Dynamics` of one row per SENTENCE: the compressor over every
    sentence (`inference(dynamics=)`).
    `intonation` (with and without `max_frames`): an `Intonation` of one row per SENTENCE, sliced per front
    group: every sentence's own pitch range and contour (`prepare(intonation=)`).  Its per-token ranges are served with
    `max_frames` only, under the rule of the per-token controls: N is the longest sentence's token count.
    `volume` (needs `max_frames` and `pack`): a `Volume` of one row per SENTENCE, sliced per front group: every
    sentence's own gain and its tokens' (`inference(volume=)`); a per-token table is as wide as the longest sentence.
    """
    dev = sentences[0].device
    if intonation is not None and (not isinstance(intonation, Intonation) or intonation.B != len(sentences)):
        raise ValueError("intonation must be a pipeline.Intonation of one row per sentence (%d)" % len(sentences))
    if controls is not None and (not isinstance(controls, Controls) or controls.B != len(sentences)):
        raise ValueError("controls must be a pipeline.Controls of one row per sentence (%d)" % len(sentences))
    if max_frames is not None:
        return _synthesize_long_capacity(
            model, sampler, sentences, ref_s=ref_s, alpha=alpha, beta=beta, t=t, diffusion_steps=diffusion_steps,
            embedding_scale=embedding_scale, noises=noises, step_noises=step_noises, sine_noises=sine_noises, durations=durations,
            trim=trim, on_chunk=on_chunk, bucket=bucket, front=front, front_batch=front_batch, decode_streams=decode_streams,
            controls=controls, max_frames=max_frames, pack=pack, sample_rate=sample_rate, marks=marks, gaps=gaps, max_gap=max_gap,
            level=level, seeds=seeds, fit_frames=fit_frames, edges=edges, breaks=breaks, dynamics=dynamics, intonation=intonation,
            volume=volume)
    _capacity_only("pack / sample_rate / marks / gaps / max_gap / level", pack, sample_rate, marks or None, gaps, max_gap, level)
    _capacity_only("edges", edges)
    _capacity_only("breaks", breaks)
    _capacity_only("dynamics", dynamics)
    _capacity_only("volume", volume)
    _capacity_only("seeds", seeds)
    _capacity_only("fit_frames / fit_hold", fit_frames)
    if controls is not None and controls.tok_present:
        raise ValueError("per-token controls are not served on the long-form path (sentences differ in width)")
    if intonation is not None:
        if intonation.tok_range is not None:
            raise ValueError("per-token ranges are not served on the long-form path (sentences differ in width): pass max_frames")
        _check_intonation(intonation, dev, len(sentences), None, front, None)
    multispeaker = ref_s is not None
    if trim is None:
        trim = 100 if multispeaker else 0
    use_streams = overlap and dev.type == "cuda"
    main = torch.cuda.current_stream(dev) if use_streams else None
    side = (side_stream if side_stream is not None else ops.aux_stream(dev)) if use_streams else None  # (a caller may
    #                                                  hand in a CU-masked side stream: pipeline.MaskedStreams)
    K = len(sentences)
    # per-call inputs are prepared (padded, stacked, moved to the device) BEFORE the streaming loop: a pageable
    # host -> device copy inside it would block the host until the issuing stream has drained
    prepped = []
    for i, i_end in _front_chunks(front_batch, K):
        ids = list(range(i, i_end))
        ns = [sentences[k].numel() for k in ids]
        npad = max(ns)
        if bucket and npad % bucket:
            npad = (npad + bucket - 1) // bucket * bucket
        frames = None  # the host's frame sums of forced durations it can read: no sync for them later
        if durations is not None and not durations[i].is_cuda:
            frames = [int(durations[k].long().sum()) for k in ids]
        prepped.append(dict(_stack_group(sentences, ids, npad, durations, noises, step_noises, ref_s, dev), ids=ids, frames=frames))
    dec = _decode_stream_list(decode_streams, use_streams, lambda i: ops.aux_stream(dev, 0, index=i + 1))
    if use_streams:
        # weights and inputs produced on the caller's stream -- including the rows stacked just above -- are visible to the other streams
        for st in [side] + dec:
            st.wait_stream(main)
        for q in prepped:  # allocated on the caller's stream, read on the side stream
            _hand_off([v for v in q.values() if torch.is_tensor(v) and v.is_cuda], side)
    s_prev, waves, emitted, n_dec, done = None, [None] * K, 0, 0, {}

    def emit(emitted):
        while emitted < K and waves[emitted] is not None:
            if done[emitted] is not None:
                main.wait_event(done[emitted])
            if on_chunk is not None:
                on_chunk(emitted, waves[emitted])
            emitted += 1
        return emitted
    for q in prepped:
        ids = q["ids"]
        kw = dict(input_lengths=q["lengths"], noise=q["noise"], diffusion_steps=diffusion_steps,
                  embedding_scale=embedding_scale, ref_s=q["ref_s"], alpha=alpha, beta=beta, lj_tail=False, s_prev=s_prev, t=t,
                  step_noise=q["step_noise"], durations=q["dur"], total_frames=q["frames"], lengths_dev=q["lens_dev"],
                  front=front, carry=len(ids) > 1, allow_ragged=True, group_events=use_streams and len(ids) > 1,
                  ragged_decode=ragged_decode, controls=None if controls is None else controls.slice(ids[0], ids[-1] + 1),
                  **({} if intonation is None else {"intonation": intonation.slice(ids[0], ids[-1] + 1)}))
        if use_streams:
            with torch.cuda.stream(side):
                p = prepare(model, sampler, q["tokens"], **kw)
                ready = torch.cuda.Event()
                ready.record(side)
        else:
            p, ready = prepare(model, sampler, q["tokens"], **kw), None
        s_prev = p["s_pred"][-1:]
        if "frames" in p:  # one ragged decoder call for the whole front group, on the caller's stream
            if use_streams:
                _hand_off(_decoder_inputs(p), main, ready)  # allocated on the side stream, consumed on the caller's
            rows = None if sine_noises is None else [sine_noises[k].reshape(-1, sine_noises[k].shape[-1]) for k in ids]
            decoded = [(list(range(len(ids))), _decode_ragged(model, p, sine_noise=rows, noise_rows=rows), None)]
        else:  # one decoder call per distinct frame count, in the order of each group's first sentence
            groups = p["groups"] if "groups" in p else [(list(range(len(ids))), p)]
            noise_of = lambda idx, g: None if sine_noises is None else torch.cat([sine_noises[ids[j]] for j in idx], dim=0)
            decoded = _decode_groups(model, groups, dec, main, noise_of, ready=ready, first=n_dec)
            n_dec += len(groups)
        for idx, w, ev in decoded:
            for j, b in enumerate(idx):
                wave = w[j].reshape(-1)
                waves[ids[b]] = wave[:-trim] if trim else wave
                done[ids[b]] = ev
            emitted = emit(emitted)  # (with decoder streams every decoder of the front group is queued by now: _decode_groups)
    if use_streams:
        _hand_off((s_prev,), main)  # allocated on the side stream, handed to the caller's
    return waves, s_prev


def _synthesize_long_capacity(model, sampler, sentences, *, ref_s, alpha, beta, t, diffusion_steps, embedding_scale, noises,
                              step_noises, sine_noises, durations, trim, on_chunk, bucket, front, front_batch, decode_streams,
                              controls, max_frames, pack, sample_rate, marks, gaps, max_gap, level, seeds, fit_frames, edges=None,
                              breaks=None, dynamics=None, intonation=None, volume=None):
    """`synthesize_long(max_frames=)`: see there.  Everything a group needs is stacked before the first group is issued."""
    dev = sentences[0].device
    K = len(sentences)
    T_cap = int(max_frames)
    if seeds is not None:  # judged once for the K sentences; every group's slice is, again, by `inference`
        seeds = _seeds_on(_check_seeds(seeds, K, max_frames, noises, step_noises, sine_noises), dev)
    if fit_frames is not None:  # likewise: a host list stays on the host, every group uploads its own slice
        fit_frames, _ = _check_fit(fit_frames, None, K, None, max_frames)
    if isinstance(decode_streams, (list, tuple)) and len(decode_streams) > 1 or \
            not isinstance(decode_streams, (list, tuple)) and decode_streams and int(decode_streams) > 1:
        raise ValueError("max_frames: there is ONE decoder call per front group, on the current stream; `decode_streams` has no "
                         "meaning here")
    if front is not None:
        raise ValueError("max_frames: the front runs inside inference(max_frames=); a GraphedFront has no place here")
    if trim is None:
        trim = 100 if ref_s is not None else 0
    ns_all = [s.numel() for s in sentences]
    tok_ctl = controls is not None and controls.tok_buf is not None or breaks is not None  # rows as wide as the longest sentence
    tok_ctl = tok_ctl or volume is not None and getattr(volume, "tok_db", None) is not None
    if intonation is not None:
        _check_intonation(intonation, dev, K, None, front, max(ns_all) if intonation.tok_range is not None else None)
        tok_ctl = tok_ctl or intonation.tok_range is not None
    if tok_ctl and controls is not None and controls.tok_buf is not None and controls.N != max(ns_all):
        raise ValueError("controls hold per-token rows of %d tokens, the longest sentence has %d" % (controls.N, max(ns_all)))
    # the K sentences' output, judged once (a `max_gap` without `gaps` is not looked at, as ever); every group's slice is, again
    chunks = _front_chunks(front_batch, K)
    spec, gaps = _output_spec(K, True, pack, trim, sample_rate, marks, gaps, None if gaps is None else max_gap, level, passage=True,
                              front_groups=len(chunks), **({} if edges is None else {"edges": edges}),
                              **({} if breaks is None else {"breaks": breaks}),
                              **({} if dynamics is None else {"dynamics": dynamics}),
                              **({} if volume is None else {"volume": volume, "device": dev}),
                              **({} if breaks is None and volume is None else {"N": max(ns_all)}))
    prepped = []
    for i, i_end in chunks:
        ids = list(range(i, i_end))
        ns = ns_all[i:i_end]
        npad = max(ns_all) if tok_ctl else max(ns)
        if bucket and npad % bucket and not tok_ctl:
            npad = (npad + bucket - 1) // bucket * bucket
        sine = None
        if sine_noises is not None:  # every sentence's own draws (>= 600 x its frames), zero-padded to the capacity
            rows = [sine_noises[k].reshape(-1, sine_noises[k].shape[-1])[:600 * T_cap] for k in ids]
            sine = torch.zeros((len(ids), 600 * T_cap, rows[0].shape[-1]), device=dev, dtype=torch.float32)
            for j, r in enumerate(rows):
                sine[j, :r.shape[0]] = r
        prepped.append(dict(_stack_group(sentences, ids, npad, durations, noises, step_noises, ref_s, dev), ids=ids, sine=sine))
    s_prev, results = None, []
    for k, q in enumerate(prepped):
        i, j = q["ids"][0], q["ids"][-1] + 1
        more = {} if gaps is None else dict(gaps=gaps[i:j], max_gap=spec.max_gap)
        if edges is not None:
            more.update(edges=edges.slice(i, j))
        if breaks is not None:
            more.update(breaks=breaks.slice(i, j))
        if dynamics is not None:
            more.update(dynamics=dynamics.slice(i, j))
        if intonation is not None:
            more.update(intonation=intonation.slice(i, j))
        if volume is not None:
            more.update(volume=volume.slice(i, j))
        res = inference(model, sampler, q["tokens"], input_lengths=q["lengths"], lengths_dev=q["lens_dev"], noise=q["noise"],
                        diffusion_steps=diffusion_steps, embedding_scale=embedding_scale, ref_s=q["ref_s"], alpha=alpha, beta=beta,
                        lj_tail=False, step_noise=q["step_noise"], sine_noise=q["sine"], durations=q["dur"], max_frames=T_cap,
                        pack=pack, trim=trim, sample_rate=sample_rate, marks=marks, passage=True, s_prev=s_prev, t=t,
                        controls=None if controls is None else controls.slice(i, j),
                        level=None if level is None else level.slice(i, j),
                        seeds=None if seeds is None else seeds[i:j],
                        fit_frames=None if fit_frames is None else fit_frames[i:j], **more)
        s_prev = res.style[-1:]
        results.append(res)
        if on_chunk is not None:
            on_chunk(k, res)
    return results, s_prev


# ---------------------------------------------------------------------------------------------------------------------
# per-layer operand scales of the split-f16 convs (include/st2.h st2_calibrate)
# ---------------------------------------------------------------------------------------------------------------------
def calibrate(run, margin_bits=3, max_passes=3, engines=None, accumulate=False):
    """Start-up calibration of a serving process: `run()` issues one or more representative forwards through the product
    path (e.g. `lambda: inference(model, sampler, tokens, ...)`, plus `style.compute_style(model, wave)` for a zero-shot
    model); every split-f16 conv of every live engine that was launched gets its own power-of-two operand scale from the
    largest input it saw (the reference's convs are fp32 at every magnitude, Modules/istftnet.py:68-74; by rule the scale is
    8 / 1, which is fp32-class for O(1) tensors only).  A pass whose launches ran into the f16 clamp at their old scale only
    bounds those layers from below, so the recording is repeated (at most `max_passes` times).  Calibrate BEFORE recording
    hipGraphs (GraphedFront re-records by itself); results stay bitwise reproducible for a given table.  `run()` should cover the
    spread of the traffic (several utterances, several reference styles): a site keeps 8 x headroom over the largest operand seen
    after a normalising prologue and 32 x where its input is free-ranging (F0 in Hz, stage outputs, FFN intermediates); beyond that
    the clamp + ST2_STATUS_F16_RANGE stay as the net.  `accumulate=True` widens the existing table with what this call sees instead
    of starting over (more utterances later, same checkpoint): no site's scale grows by it, whether the table was calibrated here
    or installed by `load_calibration_state`.  Starting over clears the tables of `engines` when given, else of the engines that
    `run()` launched -- another model loaded in the same process keeps its calibration.  Returns
    {"passes", "sites_set", "clamped_last_pass", "headroom": rows of the last pass (ops.headroom)}."""
    from . import _lib, engine
    rows, nset, clamped, passes = [], 0, 0, 0
    ops.check_status()  # whatever earlier calls raised is theirs: reported now, not swallowed by the passes below
    if not accumulate and engines is not None:
        for eng in engines:
            eng.set_calibration(None)  # st2_calibrate accumulates maxima: a fresh calibration starts from the rule
    for _ in range(max(1, int(max_passes))):
        with ops.headroom() as h:
            run()
        ops.check_status(ignore=_lib.STATUS_F16_RANGE)  # a clamp during calibration is what the pass is there to find
        rows, passes = h.rows, passes + 1
        nset = clamped = 0
        launched = {r["engine"] for r in rows if r["site"] >= 0}
        for eng in (engines if engines is not None else engine.live_engines()):
            if engines is None and not accumulate and passes == 1 and eng.h.value in launched:
                # Without `engines=` the calibration belongs to the engines `run()` launches, and only the first pass says which:
                # they start over here (their first pass ran at whatever scales they had: a site's maximum is max |hi| / x_scale,
                # the same f16 value at any power of two that does not clamp -- and a clamp repeats the pass).  Every other
                # engine of the process -- another loaded model -- keeps its table and its calib_gen.
                eng.set_calibration(None)
            n, c = eng.calibrate(margin_bits)
            nset, clamped = nset + n, clamped + c
        if clamped == 0:
            break
    return {"passes": passes, "sites_set": nset, "clamped_last_pass": clamped, "headroom": rows}


def model_engines(model, dev):
    """{"front": ..., "decoder": ..., "style": ...}: the st2_engine handles behind a model's product path on `dev`, built if
    they are not yet (same caches as the forward calls use)."""
    from . import engine, style
    dev = engine.norm_device(dev)
    dec = model.decoder
    if getattr(dec, "_eng", None) is None or not engine.same_device(dec._eng, dev):
        engine.replaced(getattr(dec, "_eng", None), "decoder")
        dec._eng = engine.build_decoder_engine(dec, dev)
    out = {"front": _front_engine(model, dev), "decoder": dec._eng}
    se, pe = model.get("style_encoder"), model.get("predictor_encoder")
    on_dev = lambda m: all(engine.norm_device(p.device) == dev for p in m.parameters())
    if isinstance(se, style.StyleEncoder) and isinstance(pe, style.StyleEncoder) and on_dev(se) and on_dev(pe):
        out["style"] = style._style_engine(model, dev)  # (a process that never moved the style encoders to `dev` has no such engine)
    return out


def calibration_state(model, dev):
    """JSON-serialisable {"front": [x_scale per conv site], "decoder": [...], ...} (0.0 = by rule): what a process saves
    beside a checkpoint, and what rank 0 sends to the other ranks (`parallel.broadcast_calibration`)."""
    return {k: e.calibration_scales() for k, e in model_engines(model, dev).items()}


def load_calibration_state(model, dev, state):
    """Installs a table made by `calibration_state` on a process holding the same model (same conv layout: checked)."""
    engs = model_engines(model, dev)
    for k, scales in state.items():
        if k in engs:
            engs[k].set_calibration(scales)
