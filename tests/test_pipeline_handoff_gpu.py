"""The cross-stream hand-off of a prepared batch (pipeline.inference(front_stream=)): in every decode mode -- one decoder call
per frame-count group (sequential, or dealt onto two decoder streams), one ragged call, the capacity-bound call -- the front
on a side stream gives bit for bit what the single-stream call gives, the device `frames` included; and a `GraphedSynthesis`
replay is the eager capacity-bound call.  B = 3 right-padded rows, 2 diffusion steps, forced durations."""
import pytest
import torch

from _util import manifest
from benchdata import synth  # seeded synthetic weights (test + bench helper, not product code)
from styletts2_amd import models, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ["decoder", "diffusion", "predictor", "text_encoder", "bert_encoder", "bert"]
STEPS, B, N = 2, 3, 6
LENS = [6, 4, 5]
# forced durations per row (pad tokens: no frames).  "pair": rows 0 and 2 share a frame count and are not adjacent -- one
# group with a non-consecutive index, one single row, and a ragged tail in the padded batch; "distinct": three groups.
DURATIONS = {"pair": [[2, 2, 2, 2, 2, 2], [2, 2, 2, 1, 0, 0], [3, 3, 2, 2, 2, 0]],        # 12 / 7 / 12 frames
             "distinct": [[2, 1, 1, 1, 1, 1], [3, 3, 3, 3, 0, 0], [4, 4, 3, 3, 3, 0]]}    # 7 / 12 / 17 = 12 + 5 frames


@pytest.fixture(scope="module")
def c():
    """The model and the inputs, built once for the module."""
    man = manifest("ljspeech")
    args = models.recursive_munch(man["config"])
    model = models.build_model(args, None, None, models.load_plbert(man["plbert"]))
    for i, k in enumerate(KEYS):
        synth.init_synthetic_(model[k], 10 + i)
        model[k].eval().to(DEV)
    g = torch.Generator().manual_seed(41)
    tokens = torch.randint(1, 178, (B, N), generator=g)
    tokens[:, 0] = 0
    for b, n in enumerate(LENS):
        tokens[b, n:] = 0
    return dict(model=model, sampler=models.make_sampler(model), tokens=tokens.to(DEV), lengths=torch.LongTensor(LENS),
                noise=torch.randn(B, 1, 256, generator=g).to(DEV),
                step_noise=torch.randn(STEPS - 1, B, 1, 256, generator=g).to(DEV),
                sine=torch.randn(B, 600 * 20, 9, generator=g).to(DEV))  # 20 = the largest frame count + 3


def _rows(out):
    """Every mode's result as a list of per-row tensors (+ the device frame counts on the capacity-bound path)."""
    if isinstance(out, pipeline.SynthesisResult):
        return [out.wave[b] for b in range(B)] + [out.frames]
    return [out[b] for b in range(B)]


@pytest.mark.parametrize("mode", ["groups", "groups on two decode streams", "ragged_decode", "max_frames"])
@pytest.mark.parametrize("case", sorted(DURATIONS))
def test_front_on_a_side_stream_is_bitwise_the_single_stream_call(c, case, mode):
    dur = torch.tensor(DURATIONS[case], dtype=torch.long)
    tot = dur.sum(dim=1).tolist()
    assert tot == {"pair": [12, 7, 12], "distinct": [7, 12, 17]}[case]
    kw = dict(diffusion_steps=STEPS, durations=dur, step_noise=c["step_noise"], sine_noise=c["sine"])
    if mode == "groups on two decode streams":
        kw["decode_streams"] = [torch.cuda.Stream(), torch.cuda.Stream()]
    elif mode == "ragged_decode":
        kw["ragged_decode"] = True
    elif mode == "max_frames":
        kw["max_frames"] = max(tot) + 3

    def run(front_stream):
        out = pipeline.inference(c["model"], c["sampler"], c["tokens"], c["lengths"], c["noise"], front_stream=front_stream, **kw)
        torch.cuda.synchronize()
        return _rows(out)

    ref = run(None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = run(side)
    if mode == "max_frames":
        assert ref[-1].cpu().tolist() == tot and ref[0].shape == (1, 600 * (max(tot) + 3))
    else:
        assert [w.shape for w in ref] == [(1, 600 * t) for t in tot]
    assert len(got) == len(ref)
    for b, (a, r) in enumerate(zip(got, ref)):
        assert a.shape == r.shape and torch.equal(a, r), "%s, %s: row %d" % (case, mode, b)
    assert all(bool(torch.isfinite(r.float()).all()) for r in ref)


def test_graphed_synthesis_replayed_twice_is_the_eager_capacity_call(c):
    model, sampler = c["model"], c["sampler"]
    ld = c["lengths"].to(torch.int32).to(DEV)
    # the capacity from a host-read run: no frame count of the seeded weights is assumed
    need = pipeline.prepare(model, sampler, c["tokens"], c["lengths"], c["noise"], diffusion_steps=STEPS,
                            step_noise=c["step_noise"], allow_ragged=True)["durations"].sum(dim=1).tolist()
    T_cap = max(need) + 3
    sine = torch.randn(B, 600 * T_cap, 9, generator=torch.Generator().manual_seed(43)).to(DEV)
    gs = pipeline.GraphedSynthesis(model, sampler, B, N, T_cap, STEPS)
    replays = []
    for _ in range(2):
        res = gs(tokens=c["tokens"], lengths=ld, noise=c["noise"], step_noise=c["step_noise"], sine_noise=sine)
        torch.cuda.synchronize()
        replays.append((res.wave.clone(), res.frames.clone()))
    eager = pipeline.inference(model, sampler, c["tokens"], noise=c["noise"], step_noise=c["step_noise"], sine_noise=sine,
                               lengths_dev=ld, diffusion_steps=STEPS, max_frames=T_cap)
    torch.cuda.synchronize()
    assert eager.frames.cpu().tolist() == need
    for i, (wave, frames) in enumerate(replays):
        assert torch.equal(frames, eager.frames) and torch.equal(wave, eager.wave), "replay %d" % i
