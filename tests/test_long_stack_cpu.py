"""`synthesize_long` with and without `max_frames` stacks a front group's inputs by one helper (`pipeline._stack_group`): both
hand their front calls the same tokens, durations, noises, reference style and device lengths, group by group.  `prepare` and
`inference` are recorders; no GPU needed."""
import torch

from styletts2_amd import pipeline

K, STEPS = 5, 3
NS = (5, 3, 7, 2, 6)


class _Result:
    def __init__(self, B):
        self.style = torch.zeros(B, 256)


def test_both_long_form_paths_stack_their_groups_alike(monkeypatch):
    front, capacity = [], []

    def prepare(model, sampler, tokens, **kw):
        front.append(dict(kw, tokens=tokens))
        return dict(s_pred=torch.zeros(tokens.shape[0], 256), groups=[])

    def inference(model, sampler, tokens, **kw):
        capacity.append(dict(kw, tokens=tokens))
        return _Result(tokens.shape[0])
    monkeypatch.setattr(pipeline, "prepare", prepare)
    monkeypatch.setattr(pipeline, "inference", inference)
    g = torch.Generator().manual_seed(5)
    sentences = [torch.randint(1, 100, (n,), generator=g) for n in NS]
    kw = dict(ref_s=torch.randn(1, 256, generator=g), durations=[torch.randint(1, 4, (n,), generator=g) for n in NS],
              noises=[torch.randn(1, 1, 256, generator=g) for _ in NS],
              step_noises=[torch.randn(STEPS - 1, 1, 1, 256, generator=g) for _ in NS], diffusion_steps=STEPS,
              front_batch=(2, 0), bucket=4)
    pipeline.synthesize_long(None, None, sentences, **kw)
    pipeline.synthesize_long(None, None, sentences, max_frames=64, pack="s16", **kw)
    assert len(front) == len(capacity) == 2
    for a, b, ids in zip(front, capacity, ((0, 1), (2, 3, 4))):
        ns = [NS[k] for k in ids]
        assert tuple(a["tokens"].shape) == (len(ids), 8)  # 5 -> 8 and 7 -> 8: the bucket of 4
        for j, k in enumerate(ids):  # and they are what the sentences say, not merely equal
            assert a["tokens"][j].tolist() == sentences[k].tolist() + [0] * (8 - NS[k])
            assert a["durations"][j].tolist() == kw["durations"][k].tolist() + [0] * (8 - NS[k])
        assert a["lengths_dev"].dtype == torch.int32 and a["lengths_dev"].tolist() == ns
        assert a["input_lengths"].tolist() == ns
        for name in ("tokens", "durations", "noise", "step_noise", "ref_s", "lengths_dev", "input_lengths"):
            assert a[name].dtype == b[name].dtype and torch.equal(a[name], b[name]), name
        assert tuple(a["noise"].shape) == (len(ids), 1, 256) and tuple(a["step_noise"].shape) == (STEPS - 1, len(ids), 1, 256)
        assert torch.equal(a["ref_s"], kw["ref_s"].expand(len(ids), -1))
        assert a["total_frames"] == [int(kw["durations"][k].sum()) for k in ids]  # the host's own: no read-back later
