#!/usr/bin/env python
"""End-to-end throughput bench: audio-seconds per wall-second (RTF^-1) of the text->waveform hot path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config NAME] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

`--gpus N` without a torch.distributed.run environment makes the script spawn its own N ranks (one process per GPU).

Workloads (`--config`, BASELINE.json `configs`; default = the one the metric is quoted on, configs[1]):
  ljspeech           configs[1]  LJSpeech single-speaker, iSTFTNet, 5 diffusion steps, 32 x 10 s per GPU
  libritts_hifigan   configs[2]  LibriTTS multispeaker (ref-audio style vector), HiFi-GAN, 10 steps, 32 x 10 s per GPU
  libritts_istftnet  configs[3]  LibriTTS zero-shot with the iSTFTNet decoder, 5 steps, 32 x 10 s per GPU (256 over 8 GPUs)
  longform           configs[4]  one >= 60 s passage as 8 sentence units with style carry-over, hipGraph-captured sampler; the
                                 sentences' fronts run as ONE right-padded batch with the carry-over as a row scan
                                 (--longform-front-batch 0; 1 = sentence by sentence as the notebooks loop, same waveforms) and
                                 their independent decoders on --longform-decode-streams streams picked by measurement
                                 (`config.front_batch`, `config.decode_streams`, candidates in `schedules_ms_per_step`)
Synthetic 100-phoneme sequences with durations forced to 4 frames / phoneme (=> exactly 10.0 s of 24 kHz audio per
utterance), seeded random weights of the reference architecture (no checkpoints offline).  One "step" is one full pass
token ids -> waveform over the per-GPU batch (longform: over the passage); inputs are resident in HBM, outputs stay in
HBM, the random draws the reference makes inside forward (SineGen noise, ADPM2 step noise) are made inside the timed
region.  Multi-GPU is weak scaling: every rank synthesises its own utterances, no collective in steady state; the
only collective is the start-up weight broadcast over RCCL.

Schedules (`--schedule`, default `auto`): consecutive steps may share the GPU on one stream, on two streams (front of step
k+1 under the decoder of step k) or on two streams with complementary CU masks; `auto` times a few steps of the first two
during the warm-up and runs the timed region on the faster -- MI355X boxes differ in how they co-schedule two queues (DESIGN.md
section 6) -- and reports all of them in `config.schedules_ms_per_step`.

A plain run sets up (weights, operand-scale calibration, autotuned set-up step, schedule calibration), warms up, times --steps
steps and prints the line.  `--full` adds everything else the bench measures or checks: the box fingerprint, per-launch conv
events in the timed region (`roofline`), the un-overlapped conv classes, host issue and device -> host times, the bitwise
check against one stream, and for the default config at N = 1 `other_configs` (short legs -- 3 warm-up + 5 steps, autotuned,
schedule calibrated -- of BASELINE.json configs[2..4], real ragged text and a B = 1 / 10 s latency point; the headline fields
stay configs[1]) and `cpu_baseline` = the UNMODIFIED reference modules on the host cores (`kind: "reference"`, from
oracle/_ref = the same modules as bytecode when oracle/make_ref.py has built them), the oracle port beside it.
`--dump-outputs DIR` writes the waveforms of the last timed step as .npy files; the timed steps draw from a fixed seed.
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PER_GPU_BATCH = 32
N_PHONEMES = 100
FRAMES_PER_PHONEME = 4
AUDIO_S_PER_UTT = N_PHONEMES * FRAMES_PER_PHONEME * 600 / 24000.0  # 10.0
# MI355X_MICROARCH.md: dense f16/bf16 MFMA peak ~2.5 PFLOP/s (v_mfma_f32_32x32x16_f16, 1024 FLOP/clk/SIMD).  The
# dominant kernel evaluates every fp32-class multiply as THREE f16 MFMA products (hi*hi + hi*lo + lo*hi, fp32
# accumulate), so the roof for ALGORITHMIC conv FLOPs is a third of that.
F16_MFMA_PEAK_TFLOPS = 2500.0
F16S_PRODUCTS = 3
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_dominant.json")  # written by tools/pmc_summary.py --json (rocprofv3 --pmc passes)
KEYS = ["decoder", "diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]
LONGFORM_SENTENCES = [87, 100, 64, 93, 71, 100, 58, 96]  # phonemes per sentence unit: 669 x 4 frames = 66.9 s

CONFIGS = {
    "ljspeech": dict(manifest="ljspeech", steps=5, multispeaker=False, baseline_config=1,
                     workload="LJSpeech single-speaker, batch=32x10 s synthetic phoneme seqs per GPU, iSTFTNet, 5 "
                              "diffusion steps, 1xMI355X per rank (BASELINE.json configs[1])"),
    "libritts_hifigan": dict(manifest="libritts", steps=10, multispeaker=True, baseline_config=2,
                             workload="LibriTTS multispeaker (reference-style vector ref_s), batch=32x10 s per GPU, "
                                      "10 diffusion steps, HiFi-GAN decoder (BASELINE.json configs[2])"),
    "libritts_istftnet": dict(manifest="libritts_istftnet", steps=5, multispeaker=True, baseline_config=3,
                              workload="LibriTTS zero-shot (multispeaker, ref_s) with the iSTFTNet decoder, 32x10 s "
                                       "per GPU = 256 utterances over 8 GPUs, 5 diffusion steps (BASELINE.json "
                                       "configs[3])"),
    "longform": dict(manifest="libritts", steps=5, multispeaker=True, baseline_config=4, longform=True,
                     workload="long-form streaming synthesis: one 66.9 s passage as 8 sentence units (58-100 phonemes) "
                              "with style carry-over (LFinference, t=0.7), hipGraph-captured diffusion sampler with "
                              "16-token length buckets, front of sentence k+1 overlapped with the decoder of sentence "
                              "k, HiFi-GAN decoder (BASELINE.json configs[4])"),
}


def build(man):
    from styletts2_amd import models
    args = models.recursive_munch(man["config"])
    return models.build_model(args, None, None, models.load_plbert(man["plbert"]))


def synthetic_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(1, 178, (B, N_PHONEMES), generator=g)
    tokens[:, 0] = 0  # the notebooks prepend the pad id, Demo/Inference_LJSpeech.ipynb:277
    noise = torch.randn(B, 1, 256, generator=g)
    durations = torch.full((B, N_PHONEMES), FRAMES_PER_PHONEME, dtype=torch.long)
    lengths = torch.full((B,), N_PHONEMES, dtype=torch.long)
    ref_s = torch.randn(B, 256, generator=g)  # style vector of the reference audio (style encoders run once per speaker)
    return tokens, lengths, noise, durations, ref_s


DRAW_SEED = 4321  # torch's global generators, seeded right before the timed steps (their in-step draws; + rank)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, out):
    """--dump-outputs: what a caller of the timed path received from the last timed step, as float32 .npy files --
    `waveform.npy` [B, 1, samples] (30.7 MB for 32 x 10 s), or for long-form `waveform_00.npy` ... one per sentence."""
    import numpy as np
    waves = {"waveform": out} if torch.is_tensor(out) else {"waveform_%02d" % i: w for i, w in enumerate(out)}
    nbytes = sum(w.numel() * 4 for w in waves.values())
    if nbytes > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d B of outputs exceed the %d B bound" % (nbytes, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, w in waves.items():
        np.save(os.path.join(path, name + ".npy"), w.detach().float().cpu().numpy())
    log("outputs of the last timed step written to %s (%d arrays, %d B)" % (path, len(waves), nbytes))


T0 = time.time()


def log(msg):
    """Progress to stderr (stdout carries exactly one JSON line)."""
    print("[bench %7.1fs] %s" % (time.time() - T0, msg), file=sys.stderr, flush=True)


def _emit(res, detail_out):
    """The full result object goes to `detail_out` (tune table, every conv class, the box fingerprint: ~25 KB); stdout gets ONE
    line of < 8 KB with the contract's fields (benchdata/line.py; the driver could not parse round 5's 25 KB line)."""
    from benchdata import line as benchline
    path = None
    if detail_out:
        try:
            with open(detail_out, "w") as f:
                json.dump(res, f, indent=1)
            path = detail_out
            log("full result object written to %s" % detail_out)
        except OSError as e:
            log("detail file not written: %r" % (e,))
    print(benchline.dumps(res, path), flush=True)


def _time_best(fn, threads, budget_s=30.0):
    """1 warm-up + best of up to 3 runs of fn() at `threads` host threads; a cold run over the budget is reported as is."""
    torch.set_num_threads(threads)
    best = None
    for it in range(4):
        t0 = time.time()
        with torch.no_grad():
            fn()
        dt = time.time() - t0
        log("cpu_baseline run %d: %.2f s on %d threads" % (it, dt, threads))
        if it > 0 or dt > budget_s:
            best = dt if best is None else min(best, dt)
        if dt > budget_s:  # keep the bench bounded on a slow host: a single (cold) run is reported as such
            break
    return best


def cpu_baseline(man, sds, cfg):
    """The reference path on the host cores, on a bounded sample of the same workload: ONE 10 s utterance (100 phonemes,
    the config's diffusion steps and decoder), 1 warm-up + best of 3, at 8 / 16 / 32 / 64 threads (oneDNN / MKL stop
    scaling far below the GPU box's core count), best reported with its thread count.  kind = "reference": the
    UNMODIFIED reference modules through oracle/ref_harness.py -- from /root/reference where that exists (build
    container), else from oracle/_ref (the same modules compiled to bytecode by oracle/make_ref.py, which is what
    travels to the GPU box); the oracle port (oracle/st2_oracle.py, the CPU restatement the parity tests check against)
    is timed beside it at the reference's best thread count and reported as `port`.  kind = "port" only when neither
    form of the reference is present."""
    from oracle import st2_oracle as O
    steps = cfg["steps"]
    tokens, lengths, noise, durations, ref_s = synthetic_inputs(1, 0)
    g = torch.Generator().manual_seed(1)
    step_noise = torch.randn(steps - 1, 1, 1, 256, generator=g)
    sine_noise = torch.randn(1, int(AUDIO_S_PER_UTT * 24000), 9, generator=g)
    rs = ref_s if cfg["multispeaker"] else None

    def run_port():
        O.inference(sds, man["config"], man["plbert"], tokens, lengths, noise, step_noise, sine_noise,
                    diffusion_steps=steps, ref_s=rs, durations=durations)

    kind, fn, origin = "port", run_port, None
    try:
        from oracle import ref_harness as RH
        if RH.reference_available():
            fn = _reference_runner(RH, man, sds, cfg, tokens, lengths, noise, rs, durations)
            kind, origin = "reference", "%s (%s)" % (RH.REFERENCE_ROOT, RH.reference_kind())
    except Exception as e:  # the reference needs its import stubs; fall back to the port and say so
        log("reference harness unavailable (%s): timing the oracle port" % e)
    ncpu = os.cpu_count() or 1
    env = os.environ.get("ST2_CPU_THREADS")
    sweep = [int(env)] if env else sorted({min(t, ncpu) for t in (8, 16, 32, 64)})
    results = {}
    t_start = time.time()
    for th in sweep:
        results[th] = _time_best(fn, th)
        if time.time() - t_start > 45.0:  # keep the whole leg bounded
            break
    best_th = min(results, key=results.get)
    best = results[best_th]
    out = {"value": AUDIO_S_PER_UTT / best, "unit": "audio-s/s", "cores": best_th, "kind": kind,
           "host_cores": ncpu, "threads_tried": {str(k): round(v, 3) for k, v in results.items()},
           "sample": "1 utterance x 10 s (100 phonemes, %d diffusion steps, %s decoder%s), best of 3 after 1 warm-up "
                     "at the best of %s threads, %.2f s wall" % (steps, man["config"]["decoder"]["type"],
                                                                  ", ref_s features" if rs is not None else "",
                                                                  sorted(results), best)}
    if kind == "reference":
        out["reference_modules"] = origin
        tp = _time_best(run_port, best_th)
        out["port"] = {"value": AUDIO_S_PER_UTT / tp, "unit": "audio-s/s", "cores": best_th, "wall_s": round(tp, 3),
                       "what": "oracle/st2_oracle.py (the CPU restatement the parity tests check against) on the same "
                               "utterance and thread count"}
    return out


def _reference_runner(RH, man, sds, cfg, tokens, lengths, noise, ref_s, durations):
    """One utterance through the UNMODIFIED reference modules, following the notebooks' inference cell with forced
    durations (same synthetic inputs and weights as the GPU run)."""
    from oracle.make_golden import istftnet_decoder_override
    ov = {"ljspeech": ("config.yml", None), "libritts": ("config_libritts.yml", None),
          "libritts_istftnet": ("config_libritts.yml", istftnet_decoder_override())}[cfg["manifest"]]
    model, args, rcfg = RH.build_reference_model(ov[0], overrides=ov[1], replace_keys=("decoder",) if ov[1] else ())
    ref = RH.load_reference()
    for k in KEYS:
        model[k].load_state_dict(sds[k])
    sampler = ref.sampler.DiffusionSampler(model.diffusion.diffusion, sampler=ref.sampler.ADPM2Sampler(),
                                           sigma_schedule=ref.sampler.KarrasSchedule(sigma_min=0.0001, sigma_max=3.0,
                                                                                     rho=9.0), clamp=False)
    N = tokens.shape[1]
    hifigan = man["config"]["decoder"]["type"] == "hifigan"

    def run():
        mask = torch.gt(torch.arange(N).unsqueeze(0) + 1, lengths.unsqueeze(1))
        t_en = model.text_encoder(tokens, lengths, mask)
        bert_dur = model.bert(tokens, attention_mask=(~mask).int())
        d_en = model.bert_encoder(bert_dur).transpose(-1, -2)
        kw = dict(embedding=bert_dur, embedding_scale=1, num_steps=cfg["steps"])
        if ref_s is not None:
            kw["features"] = ref_s
        s_pred = sampler(noise, **kw).squeeze(1)
        s, rf = s_pred[:, 128:], s_pred[:, :128]
        if ref_s is not None:
            rf = 0.3 * rf + 0.7 * ref_s[:, :128]
            s = 0.7 * s + 0.3 * ref_s[:, 128:]
        d = model.predictor.text_encoder(d_en, s, lengths, mask)
        T = int(durations[0].sum())
        aln = torch.zeros(N, T)
        c = 0
        for i in range(N):
            aln[i, c:c + int(durations[0, i])] = 1
            c += int(durations[0, i])
        en = d.transpose(-1, -2) @ aln.unsqueeze(0)
        asr = t_en @ aln.unsqueeze(0)
        if hifigan:
            en = torch.cat([en[:, :, :1], en[:, :, :-1]], dim=2)
            asr = torch.cat([asr[:, :, :1], asr[:, :, :-1]], dim=2)
        F0, Nn = model.predictor.F0Ntrain(en, s)
        return model.decoder(asr, F0, Nn, rf.squeeze().unsqueeze(0))
    return run


def roofline(by_class):
    """Per shape class of the split-f16 convs (HIP events around every launch on its launch stream inside the timed
    region): `achieved` = algorithmic conv FLOPs (2*B*C_in*C_out*ks*L) / mean launch time; `peak` = dense f16 MFMA
    peak / 3 products (see above), so `frac` is also (f16 MFMA FLOPs executed / s) / 2.5 PFLOP/s.  The headline object
    describes the DOMINANT class (largest total time); `classes` lists every class above 2 % of the conv time.
    `traffic` = HBM bytes per launch of the dominant class from rocprofv3 PMC passes (FETCH_SIZE x2 per the gfx950
    correction in MI355X_MICROARCH.md + WRITE_SIZE), read from the committed profiles/pmc_dominant.json; the HBM-side
    view (algorithmic bytes / s vs 8 TB/s) is reported beside it."""
    peak = F16_MFMA_PEAK_TFLOPS / F16S_PRODUCTS
    rows = []
    total = sum(sum(v) for v in by_class.values()) or 1.0
    for (ks, ci, co, L, b), durs in by_class.items():
        flop = 2.0 * b * ci * co * ks * L
        avg = sum(durs) / len(durs)
        # HBM side of the same launch: the planes it reads (4 B per input element), the fp32 output it writes and -- every
        # second conv of a resblock -- the residual it adds (the 2.5 x of `alg_bytes` below, per class); a class whose
        # arithmetic intensity is below the machine balance (~90 FLOP/B at 488 TFLOP/s : 5.4 TB/s) is judged on hbm_frac
        nbytes = 4.0 * b * L * (ci + 1.5 * co)
        rows.append(dict(ks=ks, C_in=ci, C_out=co, L=L, B=b, launches=len(durs), avg_launch_ms=avg,
                         total_ms=sum(durs), share=sum(durs) / total, algorithmic_flop_per_launch=flop,
                         achieved=flop / (avg * 1e-3) / 1e12, frac=flop / (avg * 1e-3) / 1e12 / peak,
                         flop_per_byte=flop / nbytes, hbm_frac=nbytes / (avg * 1e-3) / 8e12))
    rows.sort(key=lambda r: -r["total_ms"])
    if not rows:
        return {"bound": "mfma", "achieved": None, "peak": peak, "unit": "TFLOP/s", "frac": None, "traffic": None}
    dom = rows[0]
    # every launch reads x and writes y (fp32); every second one (convs2) also reads the residual; weights are L2 resident
    alg_bytes = 2.5 * dom["B"] * dom["C_out"] * dom["L"] * 4
    traffic, note = None, "no PMC summary committed"
    if os.path.exists(PMC_FILE):
        pm = json.load(open(PMC_FILE))
        if (pm.get("shape") or [11, 128, 128, 48001]) == [dom["ks"], dom["C_in"], dom["C_out"], dom["L"]]:
            traffic, note = pm.get("hbm_bytes_per_launch"), pm.get("note")
        else:
            note = "the committed PMC summary is for another shape class"
    return {"bound": "mfma",
            "kernel": "st2_conv1d_xs ks=%d C=%d->%d L=%d B=%d (split-f16 MFMA conv on pre-activated planes; bias / "
                      "residual / statistics epilogue)" % (dom["ks"], dom["C_in"], dom["C_out"], dom["L"], dom["B"]),
            "achieved": dom["achieved"], "peak": peak, "unit": "TFLOP/s", "frac": dom["frac"],
            "traffic": traffic, "traffic_note": note,
            "peak_note": "2500 TFLOP/s dense f16 MFMA / 3 products per fp32-class multiply",
            "ceiling_note": "a bare MFMA loop of this kernel (everything else compiled out: tools/xs_bench.hip, ablation mask 15) "
                            "reaches 0.585 of `peak` on random operands on MI355X -- the matrix pipe's clock is power-limited "
                            "(1.64 GHz on random operands, 2.18 GHz on zeros; `ceiling_live` = this box's probe) -- and the "
                            "kernel 72 % of that loop (epilogue 12.7 %, activation staging 5 %, weight stream 4.5 %): "
                            "profiles/r04/r04ac_ablations.log",
            "mfma_tflops_executed": dom["achieved"] * F16S_PRODUCTS,
            "launches_timed": dom["launches"], "avg_launch_ms": dom["avg_launch_ms"],
            "algorithmic_flop_per_launch": dom["algorithmic_flop_per_launch"],
            "algorithmic_bytes_per_launch": alg_bytes,
            "hbm_view": {"achieved_GBps": alg_bytes / (dom["avg_launch_ms"] * 1e-3) / 1e9, "peak_GBps": 8000.0},
            "classes": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
                        for r in rows if r["share"] >= 0.02]}


def _read_conv_classes(lib):
    """Per-launch durations recorded by the st2_conv_timing hook, grouped by (ks, C_in, C_out, L, B)."""
    import ctypes

    from styletts2_amd import _lib
    n_rec = lib.st2_conv_timing_read(None, 0)
    rows = (ctypes.c_double * (6 * max(n_rec, 1)))()
    _lib.check(0 if lib.st2_conv_timing_read(rows, n_rec) == n_rec else 1, "st2_conv_timing_read")
    by_class = {}
    for i in range(n_rec):
        ks, ci, co, L, b, ms = rows[6 * i:6 * i + 6]
        by_class.setdefault((int(ks), int(ci), int(co), int(L), int(b)), []).append(ms)
    return by_class


def _all_classes(by_class):
    """Every shape class of a recording (no 2 % cut), largest total time first: ks, C_in, C_out, L, B, launches, ms, frac."""
    peak = F16_MFMA_PEAK_TFLOPS / F16S_PRODUCTS
    rows = []
    for (ks, ci, co, L, b), durs in by_class.items():
        flop = 2.0 * b * ci * co * ks * L
        avg = sum(durs) / len(durs)
        rows.append({"ks": ks, "C_in": ci, "C_out": co, "L": L, "B": b, "launches": len(durs),
                     "avg_launch_ms": round(avg, 4), "min_launch_ms": round(min(durs), 4),
                     "max_launch_ms": round(max(durs), 4), "total_ms": round(sum(durs), 3),
                     "achieved": round(flop / (avg * 1e-3) / 1e12, 2), "frac": round(flop / (avg * 1e-3) / 1e12 / peak, 4)})
    rows.sort(key=lambda r: -r["total_ms"])
    return rows


def _dom_key(roof):
    c = (roof.get("classes") or [{}])[0]
    return (c.get("ks"), c.get("C_in"), c.get("C_out"), c.get("L"))


def _attach_unoverlapped(roof, unoverlapped):
    """roof["unoverlapped"] = the dominant class of the timed region as measured in the untimed single-stream steps (an extra:
    any inconsistency leaves the line as it is)."""
    try:
        if not unoverlapped:
            return
        un = roofline(unoverlapped)
        if un.get("frac") is not None:
            # the dominant class of the TIMED region leads (it need not be the dominant one here); every class follows
            dom = [c for c in _all_classes(unoverlapped) if (c["ks"], c["C_in"], c["C_out"], c["L"]) == _dom_key(roof)]
            head = dom[0] if dom else None
            roof["unoverlapped"] = {"frac": head["frac"] if head else None, "achieved": head["achieved"] if head else None,
                                    "avg_launch_ms": head["avg_launch_ms"] if head else None,
                                    "launches_timed": head["launches"] if head else 0,
                                    "classes": _all_classes(unoverlapped),
                                    "what": "every launch class -- the front's token GEMMs (k = 1) included: its graph is "
                                            "replaced by eager issue for these steps -- in two untimed single-stream steps "
                                            "(no other queue on the chip), the timed region's dominant class first; `frac` "
                                            "above is the timed region's"}
    except Exception as e:
        print("[bench] un-overlapped roofline not attached: %r" % (e,), file=sys.stderr, flush=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawned_rank(rank, world, port, argv):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    sys.argv = argv
    main()


_STREAMS = {}


def _calibrate_decode_streams(a, active, step, time_steps):
    """Long-form: the independent sentences' decoders on --longform-decode-streams streams or on the caller's one, whichever is
    faster in THIS process (whether two more streams get hardware queues of their own depends on how many the process already
    made: `shared_stream`).  Untimed part of the warm-up; returns {label: ms per passage} for `schedules_ms_per_step`."""
    from styletts2_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    n = max(1, int(a.longform_decode_streams))
    cands = {"decode-streams-1": 1}
    if n > 1:
        # n consecutive auxiliary streams starting at index 1, 2, ...: which of them serialise behind the caller's stream (whose
        # queue carries the per-sentence event waits) depends on how many streams the process made before.  Round 6 tried to
        # replace the timing of these windows by a two-kernel overlap probe (are the streams on distinct hardware queues?):
        # the probe's pick ran a passage in 78 ms against 64 on one stream and 52 for the best window -- streams that share a
        # hardware queue still overlap small independent kernels (no barrier bit between different streams' packets), so
        # "overlaps" is not "does not block".  A second probe (ops.wait_blocks, tools/probe_queues.py: does an event wait or a long
        # kernel on one stream hold up a tiny kernel on another?) maps the streams onto their hardware queues cleanly -- 4 classes by
        # default, pairs at GPU_MAX_HW_QUEUES = 8 -- and streams it calls mutually free still ran the passage in 75 ms (the ragged
        # batch in 266) against 48 (160) for the best window: queue sharing is not the whole story, and only the passage itself
        # tells (profiles/LAB_NOTES.md round 6).
        # 2 ... n streams (round 6: a passage of 8 one-utterance decoders ran in 47.7 ms on two streams, 44.8 on three, 43.0 on four --
        # each decoder is a chain of kernel latencies that fills a fraction of the chip; the ragged batch of 29 decoders is fastest on two)
        for m in range(2, n + 1):
            for first in range(1, 5):
                cands["decode-streams-%d@%d" % (m, first)] = [ops.aux_stream(dev, 0, index=first + i) for i in range(m)]
    calib = {}
    for name, c in cands.items():
        active["decode_streams"] = c
        step()  # first use of these streams: allocator warm-up, the pipeline fills
        step()
        calib[name] = time_steps(3)
    best = min(calib, key=calib.get)
    active["decode_streams"] = cands[best]
    active["decode_streams_name"] = best
    log("long-form decoder streams: %s -> %s" % ({k: round(v, 2) for k, v in calib.items()}, best))
    return calib


def shared_stream(dev, priority):
    """ONE second stream per (device, priority) for the whole process.  HIP multiplexes its streams onto a handful of hardware queues
    (4 by default); every `torch.cuda.Stream()` is another stream of torch's pool, and once a process has touched more of them than
    there are hardware queues a NEW front stream can land on the queue the decoder's stream already uses: the two then serialise --
    the second model of a process measured two-stream 138 ms against 118 for the first (HiFi-GAN config, profiles/LAB_NOTES.md
    round 5).  A serving process should likewise create its streams once."""
    from styletts2_amd import ops
    return ops.aux_stream(dev, priority)


def _calibrate(a, model, dev, step):
    """Start-up calibration of the split-f16 operand scales (pipeline.calibrate), as a serving process runs it after loading a
    checkpoint: one pass of the workload itself with the operand telemetry on.  Returns what goes into `config.operand_scales`."""
    from styletts2_amd import pipeline
    if a.calibrate == "off":
        return {"mode": "rule (x_scale 8 after a normalising prologue, else 1)"}
    t = time.perf_counter()
    rep = pipeline.calibrate(lambda: (step(), torch.cuda.synchronize()))
    rows = rep["headroom"]
    out = {"mode": "calibrated per conv site (st2_calibrate, margin 3 bits)", "sites_set": rep["sites_set"], "passes": rep["passes"],
           "launches_seen": len(rows), "wall_s": round(time.perf_counter() - t, 2)}
    if rows:  # by rule, as recorded during the calibration pass: the two ends of the f16 range this checkpoint uses
        out["by_rule"] = {"top_frac_of_65504": round(max(r["frac"] for r in rows), 5),
                          "worst_split_rel_err": float("%.3g" % max(r["rel_err"] for r in rows)),
                          "launches_rel_err_above_3e-7": sum(r["rel_err"] > 3e-7 for r in rows)}
    log("operand scales calibrated: %d sites, %d pass(es), %.2f s" % (rep["sites_set"], rep["passes"], out["wall_s"]))
    return out


def _same_bits(a, b):
    """Bitwise equality of two step results (a waveform tensor, or long-form's list of per-sentence waveforms)."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def _fixed_draws(dev, steps_d, sentences, B):
    """Keyword arguments that pin what a step otherwise draws per call (the ADPM2 ancestral noise, the SineGen noise; for a
    passage also the initial noise of every sentence), so that two steps can be compared bit for bit.  Only the bitwise check
    uses them: the timed steps draw as a serving call does."""
    gen = torch.Generator(device=dev).manual_seed(4242)
    r = lambda *s: torch.randn(*s, generator=gen, device=dev)
    if sentences is None:
        return {"step_noise": r(steps_d - 1, B, 1, 256), "sine_noise": r(B, int(AUDIO_S_PER_UTT * 24000), 9)}
    return {"noises": [r(1, 1, 256) for _ in sentences], "step_noises": [r(steps_d - 1, 1, 1, 256) for _ in sentences],
            "sine_noises": [r(1, n * FRAMES_PER_PHONEME * 600, 9) for n in sentences]}


def _bitwise_vs_single(step_chosen, step_single, n=3):
    """OUTSIDE the timed region: `n` steps of the schedule that was timed and one single-stream / sequential step on the same
    inputs; True when every one of them is the single-stream result bit for bit.  The two-stream and multi-decode-stream schedules
    reorder nothing inside a kernel, so anything but equality means a kernel computed something else because of what ran beside
    it -- round 5's BiLSTM did (a gfx950 packed-f32 op_sel hazard next to another queue's MFMAs), and a
    `finite` check cannot see that.  Returns {"equal": bool, "steps": n} (+ "error")."""
    try:
        torch.cuda.synchronize()
        ref = step_single()
        torch.cuda.synchronize()
        ref = [w.clone() for w in ref] if isinstance(ref, (list, tuple)) else ref.clone()
        ok = True
        for _ in range(n):
            out = step_chosen()
            torch.cuda.synchronize()
            ok = ok and _same_bits(out, ref)
        if not ok:
            log("WARNING: the timed schedule is NOT bitwise the single-stream run on the same inputs")
        return {"equal": bool(ok), "steps": n}
    except Exception as e:  # noqa: BLE001 -- a check, never in the way of the line
        log("bitwise_vs_single check failed to run: %r" % (e,))
        return {"equal": None, "steps": 0, "error": repr(e)[:160]}


def _dominant_of(by_class):
    rows = _all_classes(by_class)
    if not rows:
        return None
    r = rows[0]
    return {"kernel": "st2_conv1d_xs k%d C%d->%d L%d B%d" % (r["ks"], r["C_in"], r["C_out"], r["L"], r["B"]),
            "avg_launch_ms": r["avg_launch_ms"], "launches": r["launches"], "frac": r["frac"],
            "share_of_xs_conv_time": round(r["total_ms"] / max(sum(x["total_ms"] for x in rows), 1e-9), 3)}


def _leg(name, a, dev, n_warm=3, n_steps=5):
    """One short leg of another BASELINE.json configuration on this process's GPU: build + seeded weights, operand-scale
    calibration, autotuned set-up step, schedule calibration (single vs two-stream, 2 steps each), `n_steps` timed steps with
    the per-launch conv events on.  Same step definition as the headline (tokens -> waveform over the per-GPU batch)."""
    from benchdata import manifest, synth
    from styletts2_amd import _lib, models, ops, pipeline
    cfg = CONFIGS[name]
    longform = bool(cfg.get("longform"))
    t_leg = time.perf_counter()
    man = manifest(cfg["manifest"])
    model = build(man)
    for i, k in enumerate(KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval().to(dev)
    sampler = models.make_sampler(model, graph=longform)
    tokens, lengths, noise, durations, ref_s = synthetic_inputs(PER_GPU_BATCH, 1000)
    tokens, noise, durations_dev = tokens.to(dev), noise.to(dev), durations.to(dev)
    ref_s = ref_s.to(dev) if cfg["multispeaker"] else None
    front = None if a.eager_front else pipeline.GraphedFront(model, sampler)
    steps_d, frames = cfg["steps"], N_PHONEMES * FRAMES_PER_PHONEME
    sched = {"single": None, "two-stream": shared_stream(dev, a.front_priority)}
    active = {"name": "two-stream"}
    first_chunk = []
    fixed = {}  # the per-call random draws (ADPM2 step noise, SineGen noise), pinned by _fixed_draws for the bitwise check only
    if longform:
        sents = [tokens[i % PER_GPU_BATCH, :n].clone() for i, n in enumerate(LONGFORM_SENTENCES)]
        durs = [torch.full((1, n), FRAMES_PER_PHONEME, dtype=torch.long) for n in LONGFORM_SENTENCES]
        audio_s = sum(LONGFORM_SENTENCES) * FRAMES_PER_PHONEME * 600 / 24000.0
        sched = {"two-stream": None}

        def step(front=front, sequential=False):
            t_start = time.perf_counter()

            def on_chunk(k, w):
                if k == 0:
                    w[-1].item()
                    first_chunk.append((time.perf_counter() - t_start) * 1e3)
            if sequential:  # the reference of `bitwise_vs_single`: one stream, one sentence's decoder at a time
                return pipeline.synthesize_long(model, sampler, sents, ref_s=ref_s[:1], diffusion_steps=steps_d, durations=durs,
                                                overlap=False, bucket=16, front=front, front_batch=a.longform_front_batch, **fixed)[0]
            return pipeline.synthesize_long(model, sampler, sents, ref_s=ref_s[:1], diffusion_steps=steps_d, durations=durs,
                                            overlap=True, bucket=16, on_chunk=on_chunk, front=front,
                                            side_stream=shared_stream(dev, 0), front_batch=a.longform_front_batch,
                                            decode_streams=active.get("decode_streams", 1), **fixed)[0]
    else:
        audio_s = PER_GPU_BATCH * AUDIO_S_PER_UTT

        def step(front=front, sequential=False):
            return pipeline.inference(model, sampler, tokens, lengths, noise, diffusion_steps=steps_d, embedding_scale=1.0,
                                      ref_s=ref_s, durations=durations_dev, total_frames=frames,
                                      front_stream=None if sequential else sched[active["name"]], front=front, **fixed)
    import contextlib
    cal = _calibrate(a, model, dev, lambda: step(front=None))  # eager: before the front's hipGraph is recorded
    with (contextlib.nullcontext() if a.no_autotune else ops.conv_autotune(reset=False)):
        step()
        torch.cuda.synchronize()
    for _ in range(n_warm):
        step()
    torch.cuda.synchronize()

    def time_steps(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            out = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3, out
    calib = {}
    if len(sched) > 1:
        for nm in sched:
            active["name"] = nm
            step()  # first use of this stream pair: allocator warm-up, the pipeline fills
            step()
            calib[nm] = time_steps(3)[0]
        active["name"] = min(calib, key=calib.get)
    if longform:
        calib = _calibrate_decode_streams(a, active, step, lambda n: time_steps(n)[0])
    first_chunk.clear()
    lib = _lib.load()
    lib.st2_conv_timing(1)
    ms, out = time_steps(n_steps)
    lib.st2_conv_timing(0)
    by_class = _read_conv_classes(lib)
    ops.check_status()
    finite = all(bool(torch.isfinite(w).all()) for w in out) if longform else bool(torch.isfinite(out).all())
    fixed.update(_fixed_draws(dev, steps_d, LONGFORM_SENTENCES if longform else None, PER_GPU_BATCH))
    bitwise = _bitwise_vs_single(step, lambda: step(sequential=True))
    fixed.clear()
    ops.check_status()
    res = {"workload": cfg["workload"], "baseline_config_index": cfg["baseline_config"], "ms_per_step": round(ms, 3),
           "audio_s_per_step": audio_s, "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "steps": n_steps, "warmup": n_warm,
           "schedule": active["name"], "schedules_ms_per_step": {k: round(v, 3) for k, v in calib.items()},
           "decoder": man["config"]["decoder"]["type"], "diffusion_steps": steps_d, "finite": finite,
           "bitwise_vs_single": bitwise["equal"], "bitwise_check": bitwise,
           "operand_scales": {k: cal[k] for k in ("mode", "sites_set") if k in cal},
           "xs_conv_ms_per_step": round(sum(sum(v) for v in by_class.values()) / n_steps, 3),
           "dominant": _dominant_of(by_class), "wall_s": None}
    if longform:
        res["first_chunk_latency_ms"] = round(min(first_chunk), 2) if first_chunk else None
        res["sentences"] = LONGFORM_SENTENCES
        res["front_batch"] = a.longform_front_batch
        res["decode_streams"] = active.get("decode_streams_name", "decode-streams-1")
    del model, sampler, front
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    res["wall_s"] = round(time.perf_counter() - t_leg, 1)
    return res


def _latency_b1(a, dev, model, sampler, front, n_warm=3, n_steps=10):
    """B = 1, one 10 s utterance, tokens -> waveform, one stream, each call synchronised: the latency point of the headline
    model (BASELINE.json configs[0]'s shape on the GPU)."""
    from styletts2_amd import _lib, ops, pipeline
    tokens, lengths, noise, durations, _ = synthetic_inputs(1, 77)
    tokens, noise, dur = tokens.to(dev), noise.to(dev), durations.to(dev)
    steps_d, frames = CONFIGS[a.config]["steps"], N_PHONEMES * FRAMES_PER_PHONEME

    fixed = {}

    def step():
        return pipeline.inference(model, sampler, tokens, lengths, noise, diffusion_steps=steps_d, embedding_scale=1.0,
                                  durations=dur, total_frames=frames, front=front, **fixed)
    import contextlib
    with (contextlib.nullcontext() if a.no_autotune else ops.conv_autotune(reset=False)):
        step()
        torch.cuda.synchronize()
    for _ in range(n_warm):
        step()
    lib = _lib.load()
    lib.st2_conv_timing(1)
    ts = []
    for _ in range(n_steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    lib.st2_conv_timing(0)
    by_class = _read_conv_classes(lib)
    ops.check_status()
    fixed.update(_fixed_draws(dev, steps_d, None, 1))
    bitwise = _bitwise_vs_single(step, step)  # one stream already: run-to-run reproducibility of the latency path
    fixed.clear()
    return {"bitwise_vs_single": bitwise["equal"], "workload": "B = 1, one 10 s utterance (100 phonemes, %d diffusion steps, %s), one stream, graph-replayed front; "
                        "every call synchronised" % (steps_d, a.config),
            "latency_ms": {"mean": round(sum(ts) / len(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)},
            "audio_s_per_s": round(AUDIO_S_PER_UTT / (min(ts) * 1e-3), 1), "steps": n_steps, "warmup": n_warm,
            "finite": bool(torch.isfinite(out).all()),
            "xs_conv_ms_per_step": round(sum(sum(v) for v in by_class.values()) / n_steps, 3), "dominant": _dominant_of(by_class)}


def ragged_inputs(dev):
    """The first 32 utterances of the reference's LJSpeech validation list (benchdata/val_phonemes_32.txt, written by
    benchdata/make_val_phonemes.py from Data/val_list.txt) through `TextCleaner` (text_utils.py:3-26): a right-padded token batch
    with its lengths, and forced durations of FRAMES_PER_PHONEME frames on every real token so that audio-seconds are defined
    (Demo/Inference_LJSpeech.ipynb:268-315 with the duration head's output replaced, as in every other leg)."""
    from styletts2_amd.text_utils import TextCleaner
    tc = TextCleaner()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "benchdata", "val_phonemes_32.txt")
    rows = [tc.encode(line.rstrip("\n")) for line in open(path, encoding="utf-8") if line.strip()]
    lens = [len(r) for r in rows]
    N = max(lens)
    tokens = torch.zeros((len(rows), N), dtype=torch.long)
    dur = torch.zeros((len(rows), N), dtype=torch.long)
    for b, r in enumerate(rows):
        tokens[b, :len(r)] = torch.tensor(r)
        dur[b, :len(r)] = FRAMES_PER_PHONEME
    g = torch.Generator().manual_seed(2024)
    noise = torch.randn(len(rows), 1, 256, generator=g)
    return tokens.to(dev), torch.LongTensor(lens), noise.to(dev), dur.to(dev), lens


def _leg_ragged(a, dev, model, sampler, front, n_warm=2, n_steps=3):
    """Real, ragged text through the headline model: 32 validation utterances of 47-182 tokens as ONE right-padded batch.  The
    front runs batched (pad tokens masked everywhere); the decoder's InstanceNorm spans an utterance, so every distinct frame
    count is its own decoder call -- 32 calls of one utterance here, which is what a serving process pays for real text unless
    it buckets by length.  Reports audio-s/s, the padding efficiency of the token batch and the number of decoder calls."""
    from styletts2_amd import ops, pipeline
    tokens, lengths, noise, dur, lens = ragged_inputs(dev)
    steps_d = CONFIGS[a.config]["steps"]
    fixed = {}
    active = {"streams": None}

    def step(sequential=False):
        return pipeline.inference(model, sampler, tokens, lengths, noise, diffusion_steps=steps_d, embedding_scale=1.0,
                                  durations=dur, front=front, decode_streams=None if sequential else active["streams"], **fixed)
    import contextlib
    with (contextlib.nullcontext() if a.no_autotune else ops.conv_autotune(reset=False)):
        out = step()
        torch.cuda.synchronize()

    def time_steps(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            o = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3, o
    # the per-utterance decoder calls on the caller's stream, or dealt onto two auxiliary streams (measured windows, as long-form)
    cands = {"decode-streams-1": None}
    for first in range(1, 5):
        cands["decode-streams-2@%d" % first] = [ops.aux_stream(dev, 0, index=first + i) for i in range(2)]
    calib = {}
    for name, c in cands.items():
        active["streams"] = c
        step()
        calib[name] = time_steps(2)[0]
    best = min(calib, key=calib.get)
    active["streams"] = cands[best]
    for _ in range(n_warm):
        step()
    ms, out = time_steps(n_steps)
    ops.check_status()
    assert isinstance(out, list) and [w.shape[-1] for w in out] == [600 * FRAMES_PER_PHONEME * n for n in lens]
    audio_s = sum(lens) * FRAMES_PER_PHONEME * 600 / 24000.0
    B = len(lens)
    fixed.update({"step_noise": torch.randn(steps_d - 1, B, 1, 256, device=dev),
                  "sine_noise": torch.randn(B, 600 * FRAMES_PER_PHONEME * max(lens), 9, device=dev)})
    bitwise = _bitwise_vs_single(step, lambda: step(sequential=True))
    fixed.clear()
    return {"schedules_ms_per_step": {k: round(v, 3) for k, v in calib.items()},
            "workload": "LJSpeech validation text: %d real utterances of %d-%d tokens (Data/val_list.txt through TextCleaner), one "
                        "right-padded batch, %d frames / token forced, iSTFTNet, %d diffusion steps" % (B, min(lens), max(lens),
                                                                                                         FRAMES_PER_PHONEME, steps_d),
            "ms_per_step": round(ms, 3), "audio_s_per_step": round(audio_s, 2), "audio_s_per_s": round(audio_s / (ms * 1e-3), 1),
            "steps": n_steps, "warmup": n_warm, "utterances": B, "phonemes_per_utterance": [min(lens), max(lens)],
            "padding_efficiency": round(sum(lens) / (B * max(lens)), 4), "decoder_calls": len(set(lens)),
            "schedule": best, "finite": all(bool(torch.isfinite(w).all()) for w in out),
            "bitwise_vs_single": bitwise["equal"]}


def other_configs(a, dev, model, sampler, front, skip):
    """BASELINE.json configs[2..4] + the B = 1 latency point as short legs in the same process (rank 0, N = 1): a run of the
    default command carries every workload the baseline names.  A failing leg reports its error and never costs the line."""
    out = {}
    for name in ("libritts_hifigan", "libritts_istftnet", "longform"):
        if name == skip:
            continue
        try:
            out[name] = _leg(name, a, dev)
            log("other config %-18s %.1f ms/step = %.0f audio-s/s (%s, %.1f s)" % (name, out[name]["ms_per_step"],
                                                                                  out[name]["audio_s_per_s"], out[name]["schedule"],
                                                                                  out[name]["wall_s"]))
        except Exception as e:  # noqa: BLE001
            out[name] = {"error": repr(e)}
            log("other config %s failed: %r" % (name, e))
            torch.cuda.empty_cache()
    if a.config == "ljspeech":
        try:
            out["ljspeech_ragged"] = _leg_ragged(a, dev, model, sampler, front)
            log("ragged real text: %.1f ms/step = %.0f audio-s/s (padding efficiency %.2f, %d decoder calls)" % (
                out["ljspeech_ragged"]["ms_per_step"], out["ljspeech_ragged"]["audio_s_per_s"],
                out["ljspeech_ragged"]["padding_efficiency"], out["ljspeech_ragged"]["decoder_calls"]))
        except Exception as e:  # noqa: BLE001
            out["ljspeech_ragged"] = {"error": repr(e)}
            log("ragged leg failed: %r" % (e,))
            torch.cuda.empty_cache()
    try:
        out["latency_b1_10s"] = _latency_b1(a, dev, model, sampler, front)
        log("B = 1 latency: %.2f ms (min)" % out["latency_b1_10s"]["latency_ms"]["min"])
    except Exception as e:  # noqa: BLE001
        out["latency_b1_10s"] = {"error": repr(e)}
        log("B = 1 latency leg failed: %r" % (e,))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="ljspeech")
    ap.add_argument("--longform-decode-streams", type=int, default=4,
                    help="long-form: the per-sentence decoder calls are dealt onto 2 ... this many streams, whichever measures "
                         "fastest (1 = the caller's stream)")
    ap.add_argument("--longform-front-batch", type=lambda v: [int(x) for x in str(v).split(",")], default=[0],
                    help="long-form: sentences per front call (0 = the whole passage in one batched front, 1 = sentence by "
                         "sentence as the notebooks' loop, '2,0' = the first two, then the rest; identical waveforms, "
                         "pipeline.synthesize_long)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--schedule", choices=["auto", "single", "two-stream", "partitioned"], default="auto",
                    help="how consecutive steps share the GPU: `single` = everything on one stream; `two-stream` = front "
                         "of step k+1 on a second (high-priority) stream under the decoder of step k, placement left to "
                         "the hardware scheduler; `partitioned` = the same pipeline on two streams with complementary CU "
                         "masks (--front-cus); `auto` (default) = time --calib-steps steps of `single` and `two-stream` "
                         "during the warm-up and run the timed region on the faster (boxes differ in how they co-schedule "
                         "two queues)")
    ap.add_argument("--single-stream", action="store_true", help="same as --schedule single")
    ap.add_argument("--front-cus", type=int, default=64, help="CUs given to the front stream by --schedule partitioned")
    ap.add_argument("--calib-steps", type=int, default=3)
    ap.add_argument("--calib-partitioned", action="store_true",
                    help="let --schedule auto also time the CU-partitioned schedule")
    ap.add_argument("--calib-decoder-priority", action="store_true",
                    help="let --schedule auto also time two streams with the DECODER's queue at high priority and the front's at "
                         "normal priority")
    ap.add_argument("--front-priority", type=int, default=-1, help="HIP stream priority of the front stream (-1 = high)")
    ap.add_argument("--eager-front", action="store_true",
                    help="issue the device-only front of a step / sentence (text encoder, PL-BERT, sampler, duration "
                         "encoder) kernel by kernel from Python instead of replaying it from one hipGraph")
    ap.add_argument("--lstm", choices=["coop", "single"], default="coop",
                    help="diagnostic: `single` replaces the cooperative BiLSTM (spin-waiting 8-CU groups) by the single-CU "
                         "kernel the library falls back to; never the measured configuration")
    ap.add_argument("--lstm-block", type=int, default=0, choices=[0, 1, 2, 4, 8],
                    help="diagnostic: utterances per cooperative BiLSTM group (0 = the library's rule)")
    ap.add_argument("--no-autotune", action="store_true",
                    help="diagnostic: keep every xs conv on the rule's build instead of measuring the bitwise-equivalent "
                         "builds per shape class during the set-up step (st2_conv_tune)")
    ap.add_argument("--cu-mask", choices=["auto", "off"], default="auto",
                    help="`auto` (default): run the CU health probe (st2_probe_cu_health); if it finds slow CUs, streams "
                         "confined to the healthy ones are calibrated beside the plain schedules and the fastest runs; `off`: "
                         "plain streams only")
    ap.add_argument("--calibrate", choices=["on", "off"], default="on",
                    help="`on` (default): what a serving process does after loading a checkpoint -- one pass with the operand "
                         "telemetry on gives every split-f16 conv its own power-of-two operand scale (pipeline.calibrate; "
                         "fp32-class precision at every input magnitude); `off`: the rule (8 after a normalising prologue, 1 "
                         "otherwise)")
    ap.add_argument("--other-configs", choices=["auto", "on", "off"], default="auto",
                    help="short legs of BASELINE.json configs[2..4] + a B = 1 latency point after the timed region (`auto`: "
                         "on with --full for the default config at N = 1)")
    ap.add_argument("--no-box-probe", action="store_true", help="skip the box fingerprint / micro-probe (`box` in the line; "
                                                                 "--full only)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: box probe, per-launch conv events in the timed region (roofline), "
                         "un-overlapped conv classes, host issue and device -> host times, the bitwise check against one "
                         "stream, other_configs and cpu_baseline.  Off: set-up, warm-up, the timed steps and the line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as float32 DIR/<name>.npy (the "
                         "waveform batch; long-form: one waveform per sentence); the timed steps draw from a fixed seed")
    ap.add_argument("--detail-out", default=None,
                    help="side file for the full result object (the printed line is its < 8 KB summary); '' = none "
                         "(default: bench_detail.json with --full, none without)")
    ap.add_argument("--dry-run", action="store_true", help="launch / rendezvous / reduction path only (gloo on CPU, no "
                                                           "compute): what the CPU tests use to cover the N-rank launch")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.detail_out is None:
        a.detail_out = "bench_detail.json" if a.full else ""

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: one process per GPU, spawned here (the driver's torch.distributed.run
        # launch sets WORLD_SIZE and takes the other branch)
        import torch.multiprocessing as mp
        mp.spawn(_spawned_rank, args=(a.gpus, _free_port(), list(sys.argv)), nprocs=a.gpus, join=True)
        return

    from styletts2_amd import parallel

    rank, local_rank, world = parallel.init_distributed()
    assert world == a.gpus, "world size %d != --gpus %d" % (world, a.gpus)
    if a.dry_run:
        parallel.barrier()
        t_b = time.perf_counter()
        nb = parallel.broadcast_module_weights(torch.nn.Linear(8, 8), src=0)
        bc_s = time.perf_counter() - t_b
        mine = 0.001 * (rank + 1)
        dt = parallel.max_over_ranks(mine, torch.device("cpu"))
        per_rank = parallel.gather_over_ranks(mine, torch.device("cpu"))
        parallel.barrier()
        if rank == 0:
            line = json.dumps({"dry_run": True, "n_gpus": world, "max_over_ranks": dt,
                               "per_rank_ms_per_step": [round(v * 1e3, 4) for v in per_rank],
                               "broadcast_s": round(bc_s, 4), "broadcast_bytes": nb}, allow_nan=False)
            from benchdata import line as benchline
            assert len(line) < benchline.LIMIT
            print(line, flush=True)
        return

    from benchdata import manifest, synth  # workload definitions: model manifests, seeded synthetic weights
    from styletts2_amd import _hooks, _lib, models, ops, pipeline
    _hooks.lstm = a.lstm  # the per-kernel Python plans; the C++ plans (the product path) follow the library hook below
    _lib.load().st2_lstm_coop_set_block(-1 if a.lstm == "single" else a.lstm_block)

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    _lib.load()
    cfg = CONFIGS[a.config]
    longform = bool(cfg.get("longform"))

    log("rank %d/%d on %s (%d host cores), config %s" % (rank, world, torch.cuda.get_device_name(local_rank),
                                                          os.cpu_count(), a.config))
    man = manifest(cfg["manifest"])
    model = build(man)
    if rank == 0:  # seeded random weights of the reference architecture, generated once ...
        for i, k in enumerate(KEYS):
            synth.init_synthetic_(model[k], 10 + i)
    sds = {k: {n: t.clone() for n, t in model[k].state_dict().items()} for k in KEYS} if rank == 0 else None
    for k in KEYS:
        model[k].eval().to(dev)
    torch.cuda.synchronize()
    t_b = time.perf_counter()
    nbytes = parallel.broadcast_model(model, KEYS, src=0)  # ... and broadcast over RCCL/xGMI (no-op for N=1)
    torch.cuda.synchronize()
    broadcast_s = time.perf_counter() - t_b
    sampler = models.make_sampler(model, graph=longform)
    log("weights ready (%d B broadcast in %.3f s)" % (nbytes, broadcast_s))
    # What box is this?  Device properties, sysfs (partition modes, DPM tables, power cap, firmware) and the library's
    # micro-probe (matrix-pipe clock, cache-level latencies, weight-stream / HBM bandwidth, workgroup census), taken with
    # the GPU otherwise idle: the line of a run on a box nobody can log into must explain its own per-class conv times.
    box = None
    if rank == 0 and a.full and not a.no_box_probe:
        from benchdata import boxinfo
        try:
            box = boxinfo.fingerprint(local_rank, probe=True, level=0)
            pr = box.get("probe", {})
            log("box probe: %s CUs, mfma random %.0f TFLOP/s @ %.2f GHz, %.1f s" % (
                pr.get("cus"), pr.get("mfma", {}).get("random", {}).get("tflops", 0.0),
                pr.get("mfma", {}).get("random", {}).get("clock_ghz", 0.0), pr.get("wall_s", 0.0)))
        except Exception as e:
            box = {"error": repr(e)}
            log("box probe failed: %r" % (e,))

    steps_d = cfg["steps"]
    B = 1 if longform else PER_GPU_BATCH
    tokens, lengths, noise, durations, ref_s = synthetic_inputs(PER_GPU_BATCH, 1000 + rank)
    tokens, noise = tokens.to(dev), noise.to(dev)
    durations_dev = durations.to(dev)  # forced durations live on the device: no host -> device copy inside a step
    frames = N_PHONEMES * FRAMES_PER_PHONEME
    ref_s = ref_s.to(dev) if cfg["multispeaker"] else None

    # Schedules (see --schedule).  Every step is one complete pass tokens -> waveform over the batch in all of them; they
    # differ only in which HIP stream the front of a step (text encoder, PL-BERT, diffusion sampler, duration / prosody
    # predictors: latency-bound small kernels) is issued on, i.e. in whether it may overlap the previous step's decoder.
    if a.single_stream:
        a.schedule = "single"
    if longform and a.schedule in ("auto", "partitioned"):
        a.schedule = "two-stream"  # synthesize_long owns its side stream
    sched = {}  # name -> (main stream or None = torch's current, front stream or None)
    ps = None
    # CU health: the conv kernel with per-workgroup stamps says when every XCD finished and whether any
    # CU ran its workgroups > 3 x slower than the chip's median; if so the same schedules are also offered on streams confined
    # to the other CUs -- chosen only if the calibration says they are faster (they never were in throughput mode).
    cu_health, healthy = None, None
    if a.cu_mask == "auto":
        try:
            rep, mask_words, n_excl = ops.probe_cu_health()
            cu_health = rep
            log("CU health: %d slow CUs of %d (launch %.0f us, XCD ends %s us)" % (rep["n_slow_cus"], rep["cus"],
                                                                                  rep["launch_us"], rep["xcd_end_us"]))
            if n_excl > 0:
                healthy = pipeline.MaskedStreams(dev, mask_words)
                log("streams on the %d healthy CUs are schedule candidates" % healthy.cus)
        except Exception as e:  # a diagnostic: never in the way of the measurement
            log("CU health probe unavailable: %r" % (e,))
            healthy = None
    if not longform:
        # `auto` calibrates the two schedules that have ever won; the CU-partitioned one (75-126 ms against 66-72 on every
        # box of round 3, DESIGN.md section 3 iv) is measured on request only (--schedule partitioned / --calib-partitioned)
        want = (("single", "two-stream") + (("partitioned",) if a.calib_partitioned else ())) if a.schedule == "auto" \
            else (a.schedule,)
        if "single" in want:
            sched["single"] = (None, None)
        if "two-stream" in want:
            sched["two-stream"] = (None, shared_stream(dev, a.front_priority))
            if a.schedule == "auto" and a.calib_decoder_priority:
                # the reverse assignment: the decoder's queue high, the front's normal (the front has slack: ~15 ms of
                # latency-bound kernels per ~65 ms step)
                sched["two-stream/decoder-priority"] = (torch.cuda.Stream(dev, priority=-1), torch.cuda.Stream(dev, priority=0))
        if "partitioned" in want:
            try:
                ps = pipeline.PartitionedStreams(dev, a.front_cus)
                sched["partitioned"] = (ps.main, ps.front)
            except Exception as e:  # CU masks refused by this driver: the schedule is simply not a candidate
                log("partitioned streams unavailable: %s" % e)
                if a.schedule == "partitioned":
                    raise
        if healthy is not None and a.schedule == "auto":
            sched["two-stream/healthy-CUs"] = (healthy.main, healthy.front)
            sched["single/healthy-CUs"] = (healthy.main, None)
        for m, f in sched.values():
            for st in (m, f):
                if st is not None:
                    st.wait_stream(torch.cuda.current_stream(dev))
    # the set-up step (autotuning) runs on the plain streams: in the throughput configurations the CU-masked schedules have
    # lost every calibration so far (74.1 vs 69.0 ms, profiles/r04/r04m1_*)
    active = {"name": a.schedule if a.schedule != "auto" else "two-stream"}

    first_chunk_ms = []
    fixed = {}  # pinned random draws, for the bitwise check after the timed region only (_fixed_draws)
    # The device-only front of a step / sentence (text encoder, PL-BERT, diffusion sampler, style mixing, duration
    # encoder: ~600 launches of 5-70 us kernels) is replayed from ONE hipGraph per shape (pipeline.GraphedFront; captured
    # during the warm-up steps): host issue time per step 6.0 -> 1.8 ms, throughput +0.7-1.3 % (profiles/archive/r02/r02x_*).  The
    # per-step random draws stay outside the graph.  --eager-front issues it kernel by kernel.
    lf_front = None if a.eager_front else pipeline.GraphedFront(model, sampler)
    if longform:
        sents = [tokens[i % PER_GPU_BATCH, :n].clone() for i, n in enumerate(LONGFORM_SENTENCES)]
        durs = [torch.full((1, n), FRAMES_PER_PHONEME, dtype=torch.long) for n in LONGFORM_SENTENCES]
        audio_s = sum(LONGFORM_SENTENCES) * FRAMES_PER_PHONEME * 600 / 24000.0

        def step(front=lf_front, sequential=False):
            t_start = time.perf_counter()

            def on_chunk(k, w):
                if k == 0:
                    w[-1].item()  # the first sentence's waveform has left the GPU queue: a streaming consumer has it
                    first_chunk_ms.append((time.perf_counter() - t_start) * 1e3)
            if sequential:  # reference of `bitwise_vs_single`: one stream, sentence after sentence
                return pipeline.synthesize_long(model, sampler, sents, ref_s=ref_s[:1], diffusion_steps=steps_d, durations=durs,
                                                overlap=False, bucket=16, front=front, front_batch=a.longform_front_batch, **fixed)[0]
            with torch.cuda.stream(healthy.main if healthy is not None else torch.cuda.current_stream(dev)):
                waves, _ = pipeline.synthesize_long(model, sampler, sents, ref_s=ref_s[:1], diffusion_steps=steps_d,
                                                    durations=durs, overlap=a.schedule != "single", bucket=16,
                                                    on_chunk=on_chunk, front=front, front_batch=a.longform_front_batch,
                                                    decode_streams=active.get("decode_streams", 1),
                                                    side_stream=healthy.front if healthy is not None else shared_stream(dev, 0),
                                                    **fixed)
            return waves
    else:
        audio_s = B * AUDIO_S_PER_UTT

        def step(front=lf_front, sequential=False):
            main_s, front_s = sched[active["name"]]
            if sequential:  # reference of `bitwise_vs_single`: everything on the caller's stream
                main_s, front_s = None, None
            with torch.cuda.stream(main_s if main_s is not None else torch.cuda.current_stream(dev)):
                return pipeline.inference(model, sampler, tokens, lengths, noise, diffusion_steps=steps_d,
                                          embedding_scale=1.0, ref_s=ref_s, durations=durations_dev, total_frames=frames,
                                          front_stream=front_s, front=front, **fixed)

    def step_eager():
        return step(front=None)

    # Set-up, not a warm-up step: (i) the xs convs are AUTOTUNED here -- the first launch of every shape class times its
    # bitwise-equivalent builds (tile shape / occupancy, dispatch-order or XCD-aware tile order) on this box and keeps the
    # fastest (st2_conv_tune; what a serving process does at start-up: boxes differ by up to 1.75 x per class on the rule's
    # build); (ii) the hipGraph of the front is recorded (one eager pass + the capture), so that --warmup 0 puts neither
    # inside the timed region.  Nothing else runs on the GPU during this step: the measurements are un-overlapped.
    import contextlib
    calibration = _calibrate(a, model, dev, step_eager)  # before the front's hipGraph is recorded: scales are kernel arguments
    if world > 1 and a.calibrate != "off":
        # every rank holds rank 0's table: all shards compute the same function of their inputs (a few hundred floats, start-up only)
        try:
            calibration["broadcast_scales"] = parallel.broadcast_calibration(model, dev)
        except Exception as e:  # deterministic across ranks (same model, same code path): every rank skips the collective
            calibration["broadcast_scales"] = "skipped: %r" % (e,)
            log("operand-scale broadcast skipped: %r" % (e,))
    tune_ctx = contextlib.nullcontext() if a.no_autotune else ops.conv_autotune(reset=True)
    t_tune = time.perf_counter()
    with tune_ctx:
        out = step()
        torch.cuda.synchronize()
    try:
        tune_table = [] if a.no_autotune else ops.conv_tune_table()
    except Exception as e:  # the table is a report; the builds it chose are already in the library
        tune_table = []
        log("autotune table unreadable: %r" % (e,))
    log("set-up step done in %.2f s (%s%d conv classes tuned, %d off the rule)" % (
        time.perf_counter() - t_tune, "front graph recorded, " if lf_front is not None else "", len(tune_table),
        sum(1 for r in tune_table if r["candidates"] and r["chosen"] != r["candidates"][0]["variant"])))
    for i in range(a.warmup):
        out = step()
        torch.cuda.synchronize()
        log("warm-up step %d done" % i)

    def time_steps(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / n * 1e3

    # Calibration (untimed, part of the warm-up): ms/step of every schedule on THIS box.  Boxes of the same SKU differ in
    # how their command processor co-schedules two queues, so the schedule is chosen by measurement,
    # the way a serving process would at start-up; all candidates are reported in `config.schedules_ms_per_step`.
    calib = {}
    sensors = None
    if not longform and a.calib_steps > 0:
        smp = None
        if rank == 0 and box is not None:
            try:  # a diagnostic: never in the way of the measurement
                from benchdata import boxinfo
                smp = boxinfo.Sampler(local_rank)
                smp.__enter__()
            except Exception as e:
                smp = None
                log("sensor sampler unavailable: %r" % (e,))
        for name in sched:
            active["name"] = name
            step()  # first use of these streams: allocator warm-up
            calib[name] = time_steps(a.calib_steps)
            log("calibration: %-11s %.2f ms/step" % (name, calib[name]))
        if smp is not None:
            try:
                smp.__exit__(None, None, None)
                sensors = smp.summary()
            except Exception as e:
                log("sensor summary unavailable: %r" % (e,))
        # N > 1: every rank picks the fastest of ITS OWN candidates (its GPU may or may not report slow CUs; nothing in
        # steady state crosses GPUs, so ranks need not agree); the line reports rank 0's calibration and choice
        active["name"] = min(calib, key=calib.get) if a.schedule == "auto" else a.schedule
        log("schedule: %s" % active["name"])
    elif not longform:
        active["name"] = a.schedule if a.schedule != "auto" else "two-stream"
    if longform and a.schedule != "single":
        calib = _calibrate_decode_streams(a, active, step, time_steps)
    # The same conv launches WITHOUT the other queue's kernels on their CUs: two untimed single-stream steps with the per-launch
    # events on (reported beside the timed region's figures as `roofline.unoverlapped`; the contract's `frac` stays the one of
    # the timed region, where the front of the next batch shares the chip with the decoder's convs and stretches them).
    lib = _lib.load()
    unoverlapped, front_ms_alone = None, None
    single_name = "single/healthy-CUs" if ("healthy" in active["name"] and "single/healthy-CUs" in sched) else "single"
    if a.full and not longform and single_name in sched and active["name"] != single_name:
        chosen = active["name"]
        try:
            active["name"] = single_name
            step(front=None)  # EAGER front in these steps: a graph replay hides its launches from the timing hook, and
            lib.st2_conv_timing(1)  # the token GEMMs of the denoiser / PL-BERT (k = 1 classes) belong in "all classes"
            torch.cuda.synchronize()
            for _ in range(2):
                step(front=None)
            torch.cuda.synchronize()
            lib.st2_conv_timing(0)
            if rank == 0:
                unoverlapped = _read_conv_classes(lib)
            # the front alone (graph replay as in the timed region), nothing else on the chip
            torch.cuda.synchronize()
            t_f = time.perf_counter()
            for _ in range(3):
                pipeline.prepare(model, sampler, tokens, lengths, noise, diffusion_steps=steps_d, embedding_scale=1.0, ref_s=ref_s,
                                 durations=durations_dev, total_frames=frames, front=lf_front)
            torch.cuda.synchronize()
            front_ms_alone = (time.perf_counter() - t_f) / 3 * 1e3
        except Exception as e:  # a measurement extra: never in the way of the timed region
            lib.st2_conv_timing(0)
            log("un-overlapped conv timing skipped: %r" % (e,))
            unoverlapped = None
        active["name"] = chosen
        torch.cuda.synchronize()
    first_chunk_ms.clear()
    # the draws the timed steps make (ADPM2 step noise, SineGen noise) start from a fixed seed, whatever the calibration above
    # ran: the same arguments give the same inputs to every timed step (--dump-outputs compares builds output for output)
    torch.manual_seed(DRAW_SEED + rank)
    if a.full:  # roofline leg: per-launch HIP events around every split-f16 conv launch, by shape class
        lib.st2_conv_timing(1)  # C-ABI hook: event pairs inside st2_conv1d_xs itself, so the C++ plans' launches are seen
    torch.cuda.synchronize()
    parallel.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize()
    parallel.barrier()
    dt = time.perf_counter() - t0
    lib.st2_conv_timing(0)
    per_rank = parallel.gather_over_ranks(dt / max(a.steps, 1) * 1e3, dev)  # every rank's own ms/step (rank order)
    dt = parallel.max_over_ranks(dt, dev)
    log("timed %d steps: %.1f ms/step" % (a.steps, dt / a.steps * 1e3))
    if longform:
        assert len(out) == len(LONGFORM_SENTENCES) and all(bool(torch.isfinite(w).all()) for w in out)
        assert sum(w.numel() + 100 for w in out) == int(round(audio_s * 24000))  # 100 samples trimmed per sentence
    else:
        assert out.shape == (B, 1, int(AUDIO_S_PER_UTT * 24000)) and bool(torch.isfinite(out).all())
    ops.check_status()  # raises if a cooperative BiLSTM group timed out or a split-f16 operand left the f16 range
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out)
    host_issue, d2h_ms, bitwise = [], None, None
    if a.full:
        # host issue time of one step (outside the timed region): wall time until the call has queued everything, GPU idle
        # at the start and not waited for
        for _ in range(3):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = step()
            host_issue.append((time.perf_counter() - t1) * 1e3)
        torch.cuda.synchronize()
        # Waveform device -> pinned host memory (reported beside `value`, never part of it -- the boundary
        # hands over device tensors): one step's output, best of 3.
        try:
            src = torch.cat([w.reshape(-1) for w in out]) if longform else out
            host_buf = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
            ts_d2h = []
            for _ in range(3):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                host_buf.copy_(src, non_blocking=True)
                torch.cuda.synchronize()
                ts_d2h.append((time.perf_counter() - t1) * 1e3)
            d2h_ms = min(ts_d2h)
            del host_buf, src
        except Exception as e:  # pinned allocation refused: the line goes out without the figure
            log("D2H measurement skipped: %r" % (e,))
        fixed.update(_fixed_draws(dev, steps_d, LONGFORM_SENTENCES if longform else None, B))
        bitwise = _bitwise_vs_single(step, lambda: step(sequential=True))
        fixed.clear()
        ops.check_status()

    if rank == 0:
        roof = None
        if a.full:
            by_class = _read_conv_classes(lib)
            roof = roofline(by_class)
            _attach_unoverlapped(roof, unoverlapped)
            try:  # the probe's dependent-free MFMA loop on random operands on THIS box: what `peak` is at the clock the chip sustains
                mf = (box or {}).get("probe", {}).get("mfma", {}).get("random", {})
                if mf.get("tflops"):
                    roof["ceiling_live"] = {"mfma_tflops_random_operands": mf["tflops"], "clock_ghz": mf.get("clock_ghz"),
                                            "frac_of_peak": mf["tflops"] / F16S_PRODUCTS / roof["peak"],
                                            "kernel_frac_of_it": roof["frac"] * roof["peak"] * F16S_PRODUCTS / mf["tflops"]}
            except Exception as e:  # a report, never in the way of the line
                log("ceiling_live unavailable: %r" % (e,))
            roof["conv_ms_per_step_all_classes"] = sum(sum(v) for v in by_class.values()) / max(a.steps, 1)
            roof["conv_ms_note"] = ("decoder + prosody convs of the timed region; the front's token GEMMs are replayed from its "
                                    "hipGraph there and appear in `unoverlapped.classes` (eager front) only")
            if front_ms_alone is not None:
                roof["front_ms_alone"] = round(front_ms_alone, 3)
        name = active["name"]
        streams = {"single": "1", "two-stream": "2 (front of step k+1 overlaps decoder of step k)",
                   "partitioned": "2 on complementary CU masks (front %d CUs, decoder the rest)" % a.front_cus,
                   "two-stream/decoder-priority": "2 (front of step k+1 overlaps decoder of step k; the decoder's queue at high "
                                                  "priority, the front's at normal)",
                   "single/healthy-CUs": "1, confined to the CUs the health probe found sound",
                   "two-stream/healthy-CUs": "2 (front of step k+1 overlaps decoder of step k), both confined to the CUs "
                                             "the health probe found sound"}[name]
        res = {
            "metric": "audio-seconds/sec (RTF^-1) end-to-end, 10 s utterance batch",
            "value": world * audio_s * a.steps / dt,
            "unit": "audio-s/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt / a.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (convs/linears: f16 hi/lo split, 3 MFMA products, fp32 accumulate)", "data": "synthetic",
            "config": {"workload": cfg["workload"], "name": a.config, "baseline_config_index": cfg["baseline_config"],
                       "global_batch": world * B, "per_gpu_batch": B, "phonemes": N_PHONEMES,
                       "diffusion_steps": steps_d, "decoder": man["config"]["decoder"]["type"],
                       "audio_s_per_step_per_gpu": audio_s, "parallelism": "utterance-sharded x%d" % world,
                       "streams": streams, "schedule": name, "schedule_requested": a.schedule,
                       "schedules_ms_per_step": {k: round(v, 3) for k, v in calib.items()},
                       "weights": "seeded random init, broadcast %d B from rank 0" % nbytes,
                       "broadcast_bytes": nbytes, "broadcast_s": round(broadcast_s, 4),
                       "per_rank_ms_per_step": [round(v, 3) for v in per_rank],
                       "conv_autotune": ("off (--no-autotune)" if a.no_autotune else
                                         [{"class": "k%d C%d->%d L%d B%d" % (r["ks"], r["C_in"], r["C_out"], r["L"], r["B"]),
                                           "chosen": r["chosen_name"],
                                           "ms": {c["name"]: c["ms"] for c in r["candidates"]}} for r in tune_table]),
                       "operand_scales": calibration,
                       "plan": _hooks.plan, "lstm": a.lstm, "graphed_front": not a.eager_front},
        }
        if a.full:
            res["config"].update({
                "bitwise_vs_single": bitwise["equal"], "bitwise_check": bitwise,
                "host_issue_ms_per_step": None if longform else round(min(host_issue), 3),
                "d2h_ms_per_step": None if d2h_ms is None else round(d2h_ms, 3),
                "value_with_d2h": None if d2h_ms is None else round(audio_s * world / (dt / a.steps + d2h_ms * 1e-3), 1)})
            res["roofline"] = roof
        if cu_health is not None:
            if box is None:
                box = {}
            box["cu_health"] = cu_health
            box["healthy_cu_streams"] = None if healthy is None else {"cus": healthy.cus, "used": "healthy-CUs" in name or longform}
        if box is not None:
            if sensors is not None:
                box["sensors_during_calibration"] = sensors
            res["box"] = box
        if longform:
            res["metric"] = "audio-seconds/sec (RTF^-1) end-to-end, long-form streaming passage"
            res["config"]["sentences"] = LONGFORM_SENTENCES
            # sentences per front call: the passage is sequential in its 256-float style vector only, so the sentences' text
            # encoder / PL-BERT / diffusion / duration stages run as one right-padded batch with the carry-over as a row scan
            # (pipeline.synthesize_long front_batch; 1 = the notebooks' sentence-by-sentence schedule, same waveforms)
            res["config"]["front_batch"] = a.longform_front_batch  # group sizes in turn, 0 = all that is left
            # independent sentences' decoders dealt onto that many streams (@ = index of the first auxiliary stream of the window)
            res["config"]["decode_streams"] = active.get("decode_streams_name", "decode-streams-1")
            res["config"]["first_chunk_latency_ms"] = {"mean": sum(first_chunk_ms) / max(len(first_chunk_ms), 1),
                                                       "min": min(first_chunk_ms) if first_chunk_ms else None}
            res["scaling"] = "weak"  # replicas only: a passage is sequential in its style vector
        if world == 1 and (a.other_configs == "on" or (a.other_configs == "auto" and a.full and a.config == "ljspeech")):
            res["other_configs"] = other_configs(a, dev, model, sampler, lf_front, skip=a.config)
        if world == 1 and a.full and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(man, sds, cfg)
        _emit(res, a.detail_out)
    if healthy is not None:
        torch.cuda.synchronize()
        healthy.close()
    if ps is not None:  # the CU-masked streams are this process's: destroyed before the runtime's own exit handlers run
        torch.cuda.synchronize()
        ps.close()


if __name__ == "__main__":
    main()
