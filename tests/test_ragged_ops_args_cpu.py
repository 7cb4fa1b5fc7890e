"""The length-aware keyword arguments of styletts2_amd.ops (include/st2.h, ABI v23) reject lengths of the wrong dtype, size or
device before anything else of the call runs -- no launch, no device needed.  (tests/test_ragged_kernels_gpu.py runs them.)"""
import pytest
import torch

from styletts2_amd import ops
from styletts2_amd._lib import St2Error

B = 3
BAD = [(torch.zeros(B, dtype=torch.int64), "int32"),           # dtype
       (torch.zeros(B + 1, dtype=torch.int32), "entries"),      # size
       (torch.zeros(2 * B, dtype=torch.int32)[::2], "entries"),  # not contiguous
       (torch.zeros(B, dtype=torch.int32), "device"),            # host memory (every operand of a launch lives on the device)
       ([1, 2, 3], "int32")]                                     # not a tensor


def _calls(n):
    x = torch.zeros(B, 4, 16)
    st = torch.zeros(B, 4, 2)
    gb = torch.zeros(B, 4)
    return {
        "activate": lambda: ops.activate(x, pro=ops.PRO_LEAKY, slope=0.2, lengths=n),
        "conv1d x_len": lambda: ops.conv1d(x, torch.zeros(12, 4), 4, 3, pad_left=1, x_len=n),
        "conv1d y_len": lambda: ops.conv1d(x, torch.zeros(12, 4), 4, 3, pad_left=1, y_len=n),
        "instnorm_stats": lambda: ops.instnorm_stats(x, lengths=n),
        "stats_finalize": lambda: ops.stats_finalize(torch.zeros(B * 4 * 3), B, 4, 1, 16, lengths=n, len_div=4),
        "conv1d_direct x_len": lambda: ops.conv1d_direct(x, torch.zeros(2, 4, 3), None, 1, 1, x_len=n),
        "conv1d_direct y_len": lambda: ops.conv1d_direct(x, torch.zeros(2, 4, 3), None, 1, 1, y_len=n),
        "convt_interleave": lambda: ops.convt_interleave(torch.zeros(B, 8, 9), 4, 2, 1, 16, q_len=n, out_len=n),
        "adain_leaky_pool": lambda: ops.adain_leaky_pool(x, st, gb, gb, 0.2, torch.zeros(4, 3), None, lengths=n),
        "har_source": lambda: ops.har_source(torch.zeros(B, 4), 10, torch.zeros(B, 40, 9), torch.zeros(9), torch.zeros(1), f_len=n),
        "stft_mag_phase": lambda: ops.stft_mag_phase(torch.zeros(B, 100), 20, 5, lengths=n),
        "istft": lambda: ops.istft(torch.zeros(B, 22, 9), 20, 5, m_len=n),
        "expand_by_durations": lambda: ops.expand_by_durations(x, torch.ones(B, 16, dtype=torch.int64), 16, lengths=n),
        "ragged_lengths": lambda: ops.ragged_lengths(n, 10, [(1, 0, 1)]),
    }


# ragged_lengths takes its batch size from `frames` itself: a longer tensor is not a wrong size there
CASES = [(name, bad, what) for name in sorted(_calls(None)) for i, (bad, what) in enumerate(BAD)
         if not (name == "ragged_lengths" and i == 1)]


@pytest.mark.parametrize("name,bad,what", CASES, ids=["%s-%s" % (c[0].replace(" ", "_"), c[2]) for c in CASES])
def test_length_arguments_are_checked_before_any_launch(name, bad, what):
    with pytest.raises(St2Error, match=what):
        _calls(bad)[name]()


def test_convt_interleave_lengths_go_together():
    n = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(St2Error, match="together"):
        ops.convt_interleave(torch.zeros(B, 8, 9), 4, 2, 1, 16, q_len=n)


def test_stats_finalize_len_div_must_divide_the_rows():
    with pytest.raises(St2Error, match="len_div"):
        ops.stats_finalize(torch.zeros(B * 4 * 3), B, 4, 1, 16, lengths=torch.zeros(B, dtype=torch.int32), len_div=5)


BAD_OUT = [(lambda: torch.zeros(B, 128, 15), "shape"),                        # one column short
           (lambda: torch.zeros(B, 64, 16), "shape"),                         # half the channels
           (lambda: torch.zeros(B * 128 * 16), "shape"),                      # flat
           (lambda: torch.zeros(B, 128, 16, dtype=torch.float64), "float32"),  # dtype
           (lambda: torch.zeros(B, 128, 16, dtype=torch.float16), "float32"),
           (lambda: torch.zeros(B, 128, 16, device="meta"), "device"),        # not where q, k, v live
           (lambda: torch.zeros(B, 128, 32)[:, :, ::2], "unit stride"),       # strided along the tokens
           (lambda: [0.0], "float32")]                                        # not a tensor


@pytest.mark.parametrize("make,what", BAD_OUT, ids=["%s%d" % (w.replace(" ", "_"), i) for i, (_, w) in enumerate(BAD_OUT)])
def test_attention_out_is_checked_before_any_launch(make, what):
    q = torch.zeros(B, 128, 16)
    with pytest.raises(St2Error, match=what):
        ops.attention(q, q, q, 2, 0.125, out=make())
