"""The launch sequence of every C++ plan, pinned: each plan of styletts2_amd/csrc/st2_engine.hip runs once on HOST memory
through the full 47-entry CPU backend table with every entry wrapped by a recorder, and the record -- slot, every integer and
float argument, every pointer as null / outside the workspace / offset into the workspace, the conv descriptors field by
field -- must equal the one in tests/golden/plan_trace.json, as must every `*_workspace_bytes` query.  A change of the host
layer that moves, adds, drops or re-targets a launch, or moves a buffer inside the workspace, shows up here without a GPU.

The fixture is written by `python tests/test_plan_trace_cpu.py --write` (run it on the commit whose behaviour is to be
kept, then change the code).  A second case covers st2_debug_set_backend: a shorter table after a longer one, NULL, and the
two refusals.
"""
import collections
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the writer runs outside pytest
    sys.path.insert(0, ROOT)

import pytest
import torch

import _cpu_backend as CB
import _cpu_backend_ragged as CBR
import _cpu_backend_style_ragged as CBS
from _util import decoder_kwargs, manifest
from benchdata import synth  # seeded synthetic weights / inputs (test + bench helper, not product code)
from styletts2_amd import _lib, engine, models

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_trace.json")
ALL_SLOTS = _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE


# ---- the recorder ---------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.log = []        # one list per launch: [slot, argument, ...]
        self.ws = (0, 0)     # (base, bytes) of the workspace of the call being recorded
        self.queries = {}    # workspace query -> bytes

    def clear(self):
        self.log, self.queries = [], {}

    def ptr(self, v):
        if not v:
            return "null"
        base, n = self.ws
        return "ws+%d" % (v - base) if base <= v < base + n else "ext"

    def enc(self, ctype, v):
        if ctype in (C.c_float, C.c_double):
            return float(v).hex()
        if ctype is C.c_void_p:
            return self.ptr(v)
        return int(v)

    def wrap(self, name, argtypes, fn):
        def run(*a):
            row = [name]
            for t, v in zip(argtypes, a):
                if t == C.POINTER(_lib.ConvDesc):
                    row.append([self.enc(ft, getattr(v.contents, fn_)) for fn_, ft in _lib.ConvDesc._fields_])
                elif t == C.POINTER(C.c_int32):  # st2_ragged_lengths: n (mul, add, div) triples on the host
                    row.append([int(v[i]) for i in range(3 * a[3])] if v else "null")
                else:
                    row.append(self.enc(t, v))
            self.log.append(row)
            return fn(*a)
        return run


def _cpu_fn(name):
    if name in CBS._OVERRIDES:
        return CBS._OVERRIDES[name]
    for mod, names in ((CBS, _lib.BACKEND_SLOTS_STYLE), (CBR, _lib.BACKEND_SLOTS_RAGGED)):
        if name in names:
            return getattr(mod, name)
    return getattr(CB, name)


def install(rec, names, fn_of=_cpu_fn):
    """A table of `names` (a prefix of ALL_SLOTS) whose compute entries report to `rec` before they run; the memory entries
    are not part of a plan and stay unrecorded.  The return value must be kept alive while the table is installed."""
    table = (C.c_void_p * len(names))()
    cbs = []
    for i, name in enumerate(names):
        if name in CB._MEM_TYPES:
            cb = CB._MEM_TYPES[name](getattr(CB, name))
        else:
            res, args = _lib._SIGNATURES["st2_" + name]
            ctype = CB._SPECIAL_TYPES.get(name) or C.CFUNCTYPE(res, *args)
            cb = ctype(CB._guard(rec.wrap(name, ctype._argtypes_, fn_of(name))))
        cbs.append(cb)
        table[i] = C.cast(cb, C.c_void_p)
    _lib.check(_lib.load().st2_debug_set_backend(table, len(names)), "st2_debug_set_backend")
    return cbs, table


class recording:
    """CB.cpu_backend() (host memory, engines torn down on the host) with the recording 47-entry table inside, and
    Engine._workspace reporting each call's workspace and query to the recorder."""

    def __init__(self, rec, names=ALL_SLOTS):
        self.rec, self.names = rec, names

    def __enter__(self):
        self.cm = CB.cpu_backend()
        self.cm.__enter__()
        self.keep = install(self.rec, self.names)
        self.plain = plain = engine.Engine._workspace
        rec = self.rec

        def reporting(eng, dev, query, *a, **k):
            ws, ptr, n = plain(eng, dev, query, *a, **k)
            rec.ws = (ptr, n)
            rec.queries[query] = n
            return ws, ptr, n
        engine.Engine._workspace = reporting
        return self.rec

    def __exit__(self, *exc):
        engine.Engine._workspace = self.plain
        return self.cm.__exit__(*exc)


# ---- the plans, at the small shapes of test_engine_cpu.py / test_ragged_plan_cpu.py / test_style_ragged_cpu.py --------------
def _decoder(tag):
    from styletts2_amd.decoder import Decoder
    dec = Decoder(**decoder_kwargs(manifest(tag)["config"]["decoder"])).eval()
    synth.init_synthetic_(dec, 1)
    return engine.build_decoder_engine(dec, None)


def _decoder_plans(tag):
    eng = _decoder(tag)
    asr, F0, N, s, noise = synth.decoder_inputs(2, 6, 3)
    yield "decoder_%s" % tag, lambda: eng.decoder_forward(asr, F0, N, s, noise=noise)
    asr, F0, N, s, noise = synth.decoder_inputs(2, 9, 4)
    yield "decoder_%s_ragged" % tag, lambda: eng.decoder_forward(asr, F0, N, s, noise=noise, frames=[9, 7])


def _durations(frames, N, g):
    dur = torch.zeros(len(frames), N, dtype=torch.long)
    for b, T in enumerate(frames):  # N tokens whose durations sum to the row's frame count
        dur[b] = torch.randint(1, max(2, T // N), (N,), generator=g)
        dur[b, -1] += T - int(dur[b].sum())
    return dur


def _predictor_plans():
    from styletts2_amd.text import ProsodyPredictor
    pred = ProsodyPredictor(style_dim=128, d_hid=512, nlayers=3, max_dur=50).eval()
    synth.init_synthetic_(pred, 7)
    eng = engine.build_predictor_engine(pred, None)
    g = torch.Generator().manual_seed(3)
    B, N, T = 2, 5, 12
    d_cm, t_en, s = torch.randn(B, 640, N, generator=g), torch.randn(B, 512, N, generator=g), torch.randn(B, 128, generator=g)
    yield "prosody", lambda: eng.prosody_forward(d_cm, t_en, _durations([T, T], N, g), s, T)
    yield "prosody_ragged", lambda: eng.prosody_forward(d_cm, t_en, _durations([T, 9], N, g), s, T, shift=True, frames=[T, 9])
    d_en, s3 = torch.randn(3, 512, 11, generator=g), torch.randn(3, 128, generator=g)
    yield "duration", lambda: eng.duration_forward(d_en, s3, torch.tensor([11, 7, 10], dtype=torch.int32), tail=5)


def _text_plans():
    from styletts2_amd.text import TextEncoder
    enc = TextEncoder(channels=512, kernel_size=5, depth=3, n_symbols=178).eval()
    synth.init_synthetic_(enc, 9)
    eng = engine.build_text_engine(enc, None)
    tokens = torch.randint(1, 178, (3, 13), generator=torch.Generator().manual_seed(6))
    yield "text", lambda: eng.text_forward(tokens, torch.tensor([13, 8, 11], dtype=torch.int32))


def _bert_plans():
    bert = models.load_plbert(manifest("ljspeech")["plbert"]).eval()
    synth.init_synthetic_(bert, 15)
    eng = engine.build_bert_engine(bert, None)
    tokens = torch.randint(1, 178, (2, 17), generator=torch.Generator().manual_seed(12))
    yield "bert", lambda: eng.bert_forward(tokens, torch.tensor([17, 12], dtype=torch.int32))


def _table(steps):
    """A step table of dyadic numbers: the plans only copy its entries into launch arguments, and the record must not depend
    on the libm that would evaluate the real schedule."""
    return [(1 + (7 * i + j) % 13) / 16.0 for i in range(steps - 1) for j in range(_lib.SAMPLER_TABLE_COLS)], 2.5


def _sampler_plans():
    args = models.recursive_munch(manifest("ljspeech")["config"])  # single speaker; the front below is the multispeaker net
    tr = models.Transformer1d(channels=256, context_embedding_features=768, context_features=256, **args.diffusion.transformer)
    diff = models.AudioDiffusionConditional(tr, sigma_data=0.2).eval()
    synth.init_synthetic_(diff, 2)
    eng = engine.build_denoiser_engine(tr, None)
    B, N, steps = 2, 19, 4
    g = torch.Generator().manual_seed(5)
    noise, emb = torch.randn(B, 1, 256, generator=g), torch.randn(B, N, 768, generator=g)
    step_noise = torch.randn(steps - 1, B, 1, 256, generator=g)
    table, sigma0 = _table(steps)
    yield "sampler", lambda: eng.sampler_run(noise, emb, None, step_noise, torch.tensor([N, N - 6], dtype=torch.int32), steps,
                                              1.5, table, sigma0)


def _front_plans():
    man = manifest("libritts")
    model = models.build_model(models.recursive_munch(man["config"]), None, None, models.load_plbert(man["plbert"]))
    for i, k in enumerate(["diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]):
        synth.init_synthetic_(model[k], 20 + i)
        model[k].eval()
    eng = engine.build_front_engine(model, None)
    B, N, steps = 3, 12, 3
    g = torch.Generator().manual_seed(31)
    tokens = torch.randint(1, 178, (B, N), generator=g)
    lengths = torch.tensor([9, 12, 7], dtype=torch.int32)
    noise, step_noise = torch.randn(B, 1, 256, generator=g), torch.randn(steps - 1, B, 1, 256, generator=g)
    ref_s, s_prev = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
    table, sigma0 = _table(steps)
    kw = dict(lengths=lengths, ref_s=ref_s, embedding_scale=1.5, alpha=0.25, beta=0.5, t=0.75)
    yield "front", lambda: eng.front_forward(tokens, noise, step_noise, table, sigma0, s_prev=s_prev, tail=5, **kw)
    yield "front_carry", lambda: eng.front_forward(tokens, noise, step_noise, table, sigma0, s_prev=s_prev[:1].contiguous(),
                                                   carry=True, predict=False, **kw)


def _style_plans():
    from styletts2_amd.style import StyleEncoder
    enc = StyleEncoder(dim_in=16, style_dim=32, max_conv_dim=64).eval()
    synth.init_spectral_norm_(enc, 41)
    eng = engine.build_style_engine(enc, None, None)
    mel = torch.randn(3, 1, 80, 131, generator=torch.Generator().manual_seed(5))
    yield "style", lambda: eng.style_forward(0, mel[:2].contiguous())
    yield "style_ragged", lambda: eng.style_forward(0, mel, frames=[131, 96, 80])


GROUPS = {"decoder_ljspeech": lambda: _decoder_plans("ljspeech"), "decoder_libritts": lambda: _decoder_plans("libritts"),
          "predictor": _predictor_plans, "text": _text_plans, "bert": _bert_plans, "sampler": _sampler_plans,
          "front": _front_plans, "style": _style_plans}


def trace(group):
    """{plan: {launches, slots, sha256, workspace_bytes}} of the plans of one group."""
    out = {}
    rec = Recorder()
    with recording(rec), torch.no_grad():
        for name, run in GROUPS[group]():
            rec.clear()
            run()
            text = json.dumps(rec.log, separators=(",", ":"))
            out[name] = {"launches": len(rec.log), "slots": dict(sorted(collections.Counter(r[0] for r in rec.log).items())),
                         "sha256": hashlib.sha256(text.encode()).hexdigest(), "workspace_bytes": dict(sorted(rec.queries.items()))}
            if os.environ.get("ST2_PLAN_TRACE_DUMP"):  # the whole record, to find what moved when the digest does
                with open(os.path.join(os.environ["ST2_PLAN_TRACE_DUMP"], name + ".json"), "w") as f:
                    f.write("\n".join(json.dumps(r) for r in rec.log))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_plan_launch_records_are_the_recorded_ones(group, golden):
    got = trace(group)
    assert got, group
    for name, g in got.items():
        want = golden[name]
        assert g["workspace_bytes"] == want["workspace_bytes"], name
        assert g["slots"] == want["slots"] and g["launches"] == want["launches"], name
        assert g["sha256"] == want["sha256"], "%s: same launches, other arguments (ST2_PLAN_TRACE_DUMP=<dir> writes them)" % name


def test_fixture_covers_every_plan(golden):
    plans = {"decoder_ljspeech", "decoder_ljspeech_ragged", "decoder_libritts", "decoder_libritts_ragged", "prosody",
             "prosody_ragged", "text", "bert", "duration", "sampler", "front", "front_carry", "style", "style_ragged"}
    assert set(golden) == plans
    ran = set().union(*(set(g["slots"]) for g in golden.values()))
    assert ran == set(ALL_SLOTS) - set(CB._MEM_TYPES), sorted(set(ALL_SLOTS) - set(CB._MEM_TYPES) - ran)


# ---- st2_debug_set_backend ------------------------------------------------------------------------------------------------------
def _err(lib):
    m = lib.st2_last_error()
    return m.decode() if m else ""


def test_set_backend_refusals_keep_their_messages():
    lib = _lib.load()
    buf = C.create_string_buffer(8)
    ptr = C.cast(buf, C.c_void_p).value  # never called: only the table is checked
    try:
        n = len(_lib.BACKEND_SLOTS) + 1
        assert (len(_lib.BACKEND_SLOTS), len(ALL_SLOTS)) == (33, 47)
        assert lib.st2_debug_set_backend((C.c_void_p * n)(*([ptr] * n)), n) != 0
        assert _err(lib) == ("st2_debug_set_backend: 34 entries, expected 47 (or 44: without the ragged style slots, or 33: the "
                             "slots before ABI v23)")
        table = (C.c_void_p * 47)(*([ptr] * 47))
        table[45] = None
        assert lib.st2_debug_set_backend(table, 47) != 0
        assert _err(lib) == "st2_debug_set_backend: entry 45 is null"
    finally:
        assert lib.st2_debug_set_backend(None, 0) == 0


def _shorter_table_after_longer():
    """Runs in a process of its own that sees no HIP device: the slots a short table leaves out go back to the HIP entry
    points, and those must fail their launch here, not run on host memory."""
    assert not torch.cuda.is_available(), "this check must not see a HIP device"
    lib = _lib.load()
    first, second = Recorder(), Recorder()
    with recording(first), torch.no_grad():
        eng = _decoder("ljspeech")
        asr, F0, N, s, noise = synth.decoder_inputs(2, 9, 4)
        eng.decoder_forward(asr, F0, N, s, noise=noise, frames=[9, 7])
        ragged = {r[0] for r in first.log} & set(_lib.BACKEND_SLOTS_RAGGED)
        assert "ragged_lengths" in ragged and len(ragged) >= 9, ragged
        first.clear()
        keep = install(second, _lib.BACKEND_SLOTS)  # 33 entries after 47: the length-aware slots leave the first table ...
        with pytest.raises(_lib.St2Error, match="st2_ragged_lengths"):  # ... for the HIP entry points (no device: refused)
            eng.decoder_forward(asr, F0, N, s, noise=noise, frames=[9, 7])
        assert not first.log and not second.log, (first.log[:1], second.log[:1])
        eng.decoder_forward(asr, F0, N, s, noise=noise)  # the uniform plan needs the 33 plain slots only
        assert not first.log and second.log and not {r[0] for r in second.log} & set(_lib.BACKEND_SLOTS_RAGGED)
        assert lib.st2_debug_set_backend(None, 0) == 0  # NULL: everything back on the HIP entry points
        second.clear()
        with pytest.raises(_lib.St2Error):
            eng.decoder_forward(asr, F0, N, s, noise=noise)
        assert not first.log and not second.log
        del keep
    print("shorter-table-ok")


def test_shorter_table_after_longer_leaves_the_rest_on_hip():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shorter-table"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "shorter-table-ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


if __name__ == "__main__":
    if "--shorter-table" in sys.argv:
        _shorter_table_after_longer()
    elif "--write" in sys.argv:
        result = {}
        for grp in sorted(GROUPS):
            result.update(trace(grp))
        with open(FIXTURE, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s: %d plans, %d launches" % (FIXTURE, len(result), sum(v["launches"] for v in result.values())))
    else:
        sys.exit("usage: test_plan_trace_cpu.py --write")
