"""What `pipeline.inference` / `pipeline.synthesize_long` do BETWEEN `prepare` and the decoder, without a device: which rows
share a decoder call, which sine-noise rows that call receives, where its waveform lands, the trim rule and the `on_chunk`
order -- on CPU tensors, with `prepare` replaced by canned results and the decoder by a stub whose waveform names its row.
Plus the two pure helpers of `synthesize_long` (front-batch chunking, decoder-stream list) against tables written from the
inlined code they replaced."""
import types

import pytest
import torch

from styletts2_amd import pipeline

SPF = 600  # samples per decoder frame


# ---- the two pure helpers -------------------------------------------------------------------------------------------------
ALL5 = [(0, 5)]
CHUNKS = {  # (front_batch, K) -> [(first sentence, one past the last)] per front call
    1: {1: [(0, 1)], 5: [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]},
    0: {1: [(0, 1)], 5: ALL5},
    None: {1: [(0, 1)], 5: ALL5},
    3: {1: [(0, 1)], 5: [(0, 3), (3, 5)]},
    (2, 0): {1: [(0, 1)], 5: [(0, 2), (2, 5)]},
    (1, 2): {1: [(0, 1)], 5: [(0, 1), (1, 3), (3, 5)]},
    10: {1: [(0, 1)], 5: ALL5},
}
CHUNK_CASES = [(fb, K) for fb in CHUNKS for K in (1, 5)]


@pytest.mark.parametrize("front_batch,K", CHUNK_CASES)
def test_front_chunks_table(front_batch, K):
    assert pipeline._front_chunks(front_batch, K) == CHUNKS[front_batch][K]
    if isinstance(front_batch, tuple):  # a list is a tuple
        assert pipeline._front_chunks(list(front_batch), K) == CHUNKS[front_batch][K]


@pytest.mark.parametrize("overlap", [True, False])
def test_decode_stream_list_table(overlap):
    made = []

    def make(i):
        made.append(i)
        return "aux%d" % i

    one, two = ["a"], ["a", "b"]
    want = {1: [], 0: [], 2: ["aux0", "aux1"] if overlap else []}
    for n, w in want.items():
        assert pipeline._decode_stream_list(n, overlap, make) == w, n
    assert made == ([0, 1] if overlap else [])  # streams are made only where they are used
    assert pipeline._decode_stream_list(one, overlap, make) == []  # one stream is the caller's own: nothing to deal onto
    got = pipeline._decode_stream_list(two, overlap, make)
    assert got == (two if overlap else []) and got is not two  # used as given, in a list of the call's own
    assert pipeline._decode_stream_list(tuple(two), overlap, make) == (two if overlap else [])
    assert len(made) == (2 if overlap else 0)


# ---- stubs -----------------------------------------------------------------------------------------------------------------
class _Decoder:
    """Row j of the waveform is `tag * 1e6 + sample index`, the tag being what the canned `asr` row holds (exact in fp32)."""
    kind = "istftnet"

    def __init__(self, log):
        self.calls, self.log = [], log

    def __call__(self, asr, F0, N, ref, noise=None, frames=None):
        tags = [int(v) for v in asr[:, 0, 0].tolist()]
        self.calls.append(dict(tags=tags, noise=noise, frames=frames, F0=F0))
        self.log.append(("decode", tags))
        return asr[:, :1, :1] * 1e6 + torch.arange(SPF * asr.shape[-1], dtype=torch.float32).reshape(1, 1, -1)


def _wave(tag, T):
    return tag * 1e6 + torch.arange(SPF * T, dtype=torch.float32)


def _g(tags, T, **more):
    """A decoder-input dict as `prepare` returns it (a whole batch, or one frame-count group): row j is utterance tags[j]."""
    b = len(tags)
    asr = torch.tensor(tags, dtype=torch.float32).reshape(b, 1, 1).expand(b, 2, T).contiguous()
    return dict(asr=asr, F0=torch.zeros(b, 2 * T), N=torch.zeros(b, 2 * T), ref=torch.zeros(b, 4), en=None, **more)


def _patch(monkeypatch, results, log):
    """`pipeline.prepare` hands out `results` in turn; returns (model stub, the keyword arguments of every call)."""
    seen, it = [], iter(results)

    def prepare(model, sampler, tokens, **kw):
        seen.append(dict(kw, tokens=tokens))
        log.append(("prepare", tokens.shape[0]))
        return next(it)

    monkeypatch.setattr(pipeline, "prepare", prepare)
    return types.SimpleNamespace(decoder=_Decoder(log)), seen


def _sentences(K):
    return [torch.arange(3 + k % 3, dtype=torch.long) for k in range(K)]


# ---- inference ---------------------------------------------------------------------------------------------------------------
def test_inference_uniform_batch_is_one_decoder_call_on_the_callers_noise(monkeypatch):
    log = []
    model, seen = _patch(monkeypatch, [_g([1, 2], 3)], log)
    sine = torch.randn(2, SPF * 3 + 50, 9)
    out = pipeline.inference(model, None, torch.zeros(2, 5, dtype=torch.long), sine_noise=sine)
    assert torch.is_tensor(out) and out.shape == (2, 1, SPF * 3)
    assert torch.equal(out[0, 0], _wave(1, 3)) and torch.equal(out[1, 0], _wave(2, 3))
    assert len(model.decoder.calls) == 1 and model.decoder.calls[0]["noise"] is sine and model.decoder.calls[0]["frames"] is None
    assert seen[0]["allow_ragged"] is True and "max_frames" not in seen[0]


def test_inference_groups_land_in_utterance_order_with_their_own_noise_rows(monkeypatch):
    log = []
    T = {1: 2, 2: 4, 3: 3, 4: 2}  # utterances 1 and 4 (rows 0 and 3: not adjacent) share a frame count
    groups = [([0, 3], _g([1, 4], 2)), ([1], _g([2], 4)), ([2], _g([3], 3))]
    model, _ = _patch(monkeypatch, [dict(groups=groups)], log)
    sine = torch.randn(4, SPF * 4 + 11, 9)
    waves = pipeline.inference(model, None, torch.zeros(4, 5, dtype=torch.long), sine_noise=sine)
    assert isinstance(waves, list) and len(waves) == 4
    for b, w in enumerate(waves):
        assert w.shape == (1, SPF * T[b + 1]) and torch.equal(w[0], _wave(b + 1, T[b + 1])), b
    assert [c["tags"] for c in model.decoder.calls] == [[1, 4], [2], [3]]  # one call per group, in the groups' order
    for c, (idx, g) in zip(model.decoder.calls, groups):  # every row cut to the group's 300 * F0 frames, then stacked
        n = 300 * g["F0"].shape[1]
        assert c["noise"].shape == (len(idx), n, 9) and c["frames"] is None
        assert all(torch.equal(c["noise"][j], sine[b, :n]) for j, b in enumerate(idx))
    # without sine noise every call gets None
    model, _ = _patch(monkeypatch, [dict(groups=groups)], log)
    pipeline.inference(model, None, torch.zeros(4, 5, dtype=torch.long))
    assert [c["noise"] for c in model.decoder.calls] == [None] * 3


@pytest.mark.parametrize("form", ["batch tensor", "rows", "none"])
def test_inference_frames_form_is_one_ragged_call(monkeypatch, form):
    log = []
    tot = [2, 4, 3]
    frames = torch.tensor(tot, dtype=torch.int32)
    model, _ = _patch(monkeypatch, [_g([1, 2, 3], 4, frames=frames, frames_host=tot)], log)
    rows = [torch.randn(SPF * t + 5 * b, 9) for b, t in enumerate(tot)]  # each at least its own 600 T_b samples
    sine = {"batch tensor": torch.randn(3, SPF * 4 + 7, 9), "rows": rows, "none": None}[form]
    waves = pipeline.inference(model, None, torch.zeros(3, 5, dtype=torch.long), sine_noise=sine)
    assert [w.shape for w in waves] == [(1, SPF * t) for t in tot]
    assert all(torch.equal(w[0], _wave(b + 1, tot[b])) for b, w in enumerate(waves))  # every row cut to its own frames
    (c,) = model.decoder.calls
    assert c["frames"] is frames
    if form == "none":
        assert c["noise"] is None
    elif form == "batch tensor":  # a view of the caller's tensor at the batch's width
        assert c["noise"].shape == (3, SPF * 4, 9) and c["noise"].data_ptr() == sine.data_ptr() and torch.equal(c["noise"], sine[:, :SPF * 4])
    else:  # copied into the T_max layout; past 600 T_b nothing is defined
        assert c["noise"].shape == (3, SPF * 4, 9)
        assert all(torch.equal(c["noise"][b, :SPF * t], rows[b][:SPF * t]) for b, t in enumerate(tot))


# ---- synthesize_long ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front_batch,K", CHUNK_CASES)
def test_long_form_front_calls_follow_the_chunk_table(monkeypatch, front_batch, K):
    log = []
    want = CHUNKS[front_batch][K]
    results = [dict(_g(list(range(i + 1, j + 1)), 2), s_pred=torch.full((j - i, 4), float(j))) for i, j in want]
    model, seen = _patch(monkeypatch, results, log)
    order = []
    waves, style = pipeline.synthesize_long(model, None, _sentences(K), overlap=False, front_batch=front_batch,
                                            on_chunk=lambda k, w: order.append(k))
    assert [s["tokens"].shape[0] for s in seen] == [j - i for i, j in want]
    assert [s["carry"] for s in seen] == [j - i > 1 for i, j in want]
    assert order == list(range(K)) and all(torch.equal(w, _wave(k + 1, 2)) for k, w in enumerate(waves))
    assert torch.equal(style, torch.full((1, 4), float(K)))


@pytest.mark.parametrize("ref_s,trim,dropped", [(None, None, 0), (torch.zeros(1, 8), None, 100), (None, 7, 7),
                                                (torch.zeros(1, 8), 0, 0)])
def test_long_form_groups_across_front_calls(monkeypatch, ref_s, trim, dropped):
    """Five sentences as front calls of 2 + 3: the first comes back as one group (the single-group form), the second as two
    groups of which the first holds sentences 2 and 4 (not adjacent)."""
    log = []
    T = [2, 2, 3, 2, 3]
    p0 = dict(_g([1, 2], 2), s_pred=torch.full((2, 4), 10.0))
    p0["s_pred"][-1] = 11.0
    p1 = dict(groups=[([0, 2], _g([3, 5], 3)), ([1], _g([4], 2))], s_pred=torch.full((3, 4), 20.0))
    p1["s_pred"][-1] = 21.0
    model, seen = _patch(monkeypatch, [p0, p1], log)
    sine = [torch.randn(1, SPF * t, 9) for t in T]
    waves, style = pipeline.synthesize_long(model, None, _sentences(5), ref_s=ref_s, trim=trim, overlap=False, front_batch=(2, 0),
                                            sine_noises=sine, on_chunk=lambda k, w: log.append(("chunk", k, w)))
    # which wave lands where, and the trim rule (100 samples with a reference style, else 0, unless given)
    for k, w in enumerate(waves):
        full = _wave(k + 1, T[k])
        assert w.dim() == 1 and torch.equal(w, full[:-dropped] if dropped else full), k
    # the decoder calls in the groups' order; `on_chunk` in sentence order, as soon as every earlier sentence is there
    assert [(e[0], e[1]) for e in log] == [("prepare", 2), ("decode", [1, 2]), ("chunk", 0), ("chunk", 1), ("prepare", 3),
                                           ("decode", [3, 5]), ("chunk", 2), ("decode", [4]), ("chunk", 3), ("chunk", 4)]
    assert all(e[2] is waves[e[1]] for e in log if e[0] == "chunk")
    # each call's noise: the sentences' own rows, concatenated in the group's order
    got = [c["noise"] for c in model.decoder.calls]
    assert torch.equal(got[0], torch.cat([sine[0], sine[1]])) and torch.equal(got[1], torch.cat([sine[2], sine[4]]))
    assert torch.equal(got[2], sine[3])
    # the style hand-over: the last row of a front call feeds the next call, the last one is returned
    assert seen[0]["s_prev"] is None and torch.equal(seen[1]["s_prev"], torch.full((1, 4), 11.0))
    assert torch.equal(style, torch.full((1, 4), 21.0))
    assert all(s["allow_ragged"] and not s["group_events"] and s["lj_tail"] is False for s in seen)
    assert (seen[0]["ref_s"] is None) == (ref_s is None) and (ref_s is None or seen[1]["ref_s"].shape == (3, 8))


@pytest.mark.parametrize("with_noise", [True, False])
def test_long_form_frames_form_is_one_ragged_call_per_front_group(monkeypatch, with_noise):
    log = []
    tot = [2, 4, 3]
    frames = torch.tensor(tot, dtype=torch.int32)
    p = dict(_g([1, 2, 3], 4, frames=frames, frames_host=tot), s_pred=torch.full((3, 4), 5.0))
    model, seen = _patch(monkeypatch, [p], log)
    sine = [torch.randn(1, SPF * t + 3, 9) for t in tot] if with_noise else None
    waves, style = pipeline.synthesize_long(model, None, _sentences(3), overlap=False, front_batch=0, ragged_decode=True,
                                            trim=7, sine_noises=sine, on_chunk=lambda k, w: log.append(("chunk", k)))
    assert seen[0]["ragged_decode"] is True
    assert all(torch.equal(w, _wave(k + 1, tot[k])[:-7]) for k, w in enumerate(waves))
    assert log == [("prepare", 3), ("decode", [1, 2, 3]), ("chunk", 0), ("chunk", 1), ("chunk", 2)]
    (c,) = model.decoder.calls
    assert c["frames"] is frames
    if with_noise:
        assert c["noise"].shape == (3, SPF * 4, 9)
        assert all(torch.equal(c["noise"][b, :SPF * t], sine[b][0, :SPF * t]) for b, t in enumerate(tot))
    else:
        assert c["noise"] is None
    assert torch.equal(style, torch.full((1, 4), 5.0))
