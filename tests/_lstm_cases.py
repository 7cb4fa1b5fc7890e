"""Inputs of tests/test_lstm_edges_gpu.py with their float64 references (tests/_lstm_ref.py), made on the host and cached so
that both recurrence kernels are judged by one reference.  The conditions that make a hard case hard are properties of the
reference alone: tests/test_lstm_ref_cpu.py asserts them without a GPU, the GPU tests assert them again beside the kernel."""
import functools

import numpy as np
import torch

import _lstm_ref as L

H = 256  # the only hidden size the library builds


def whh(seed, bound=1.0 / 16):
    """W_hh^T per direction as nn.LSTM draws it: uniform +- 1 / sqrt(H)."""
    gen = torch.Generator().manual_seed(seed)
    return ((torch.rand(2, H, 4 * H, generator=gen) * 2 - 1) * bound).contiguous()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def block_lengths(B, N):
    """Row b gets PATTERN[b % 8]: every block of 8 (and every other block of 4) holds len = 1, len = N and len = N - 1 side by
    side with the longest row second, the blocks of 4 in between have their longest row (33) second too."""
    pattern = [1, N, N - 1, 17, 9, 33, 2, 25]
    assert N >= 34
    return [pattern[b % 8] for b in range(B)]


class Case:
    """G, whh_t (fp32 torch), lens (list or None), ref (float64 numpy) and, where asked for, e32 = max |fp32 contract - ref|,
    the cell states c and the pre-activations a of the float64 run."""

    def __init__(self, G, whh_t, lens, e32=False, state=False):
        self.G, self.whh_t, self.lens = G, whh_t, lens
        self.B, _, self.N = G.shape
        Gn, Wn = G.numpy(), whh_t.numpy()
        if state:
            self.ref, self.c, self.a = L.lstm_bidir(Gn, Wn, lens, want_state=True)
        else:
            self.ref = L.lstm_bidir(Gn, Wn, lens)
        self.e32 = float(np.abs(L.lstm_bidir(Gn, Wn, lens, dtype=np.float32) - self.ref).max()) if e32 else None
        self.valid = L.valid_mask(lens, self.B, self.N)


@functools.lru_cache(maxsize=None)
def build_case(B, ragged, N=40):
    lens = None
    if ragged:
        lens = block_lengths(B, N) if B > 1 else [N - 1]
    return Case(randn(1000 + B, B, 8 * H, N), whh(1), lens)


LONG_N = (400, 1201)


@functools.lru_cache(maxsize=2)
def long_case(N):
    """B = 5, one row at full length, one of a single step, one that ends one step early."""
    return Case(randn(2000 + N, 5, 8 * H, N), whh(2), [N // 2 + 1, N, 1, N - 1, 77], e32=True)


HARD_N, HARD_B = 300, 4
HARD_LENS = [HARD_N, HARD_N - 1, 157, 64]
HARD_KINDS = ("saturated", "long_memory", "large_whh")


@functools.lru_cache(maxsize=None)
def hard_case(kind):
    """N = 300, B = 4.
    benign       G ~ N(0, 1), W_hh uniform +- 1/16: the yardstick of `large_whh`.
    saturated    G's rows scaled by 40 (every 8th), 10 (two of 8) or 1: sigmoids and tanh deep in saturation on both signs,
                 exp(-a) overflowing (a < -88.7) and underflowing in float32.
    long_memory  forget gate + 6 (f = 0.9975: a time constant of 400 steps), input gate + 2: c is a random walk that grows for
                 hundreds of steps instead of forgetting.
    large_whh    W_hh uniform +- 0.25: the recurrent Jacobian is no longer strongly contractive, round-off is carried along."""
    G = randn({"benign": 3004, "saturated": 3001, "long_memory": 3002, "large_whh": 3004}[kind], HARD_B, 8 * H, HARD_N)
    W = whh(4)
    if kind == "saturated":
        scale = torch.ones(8 * H)
        scale[0::8] = 40.0
        scale[1::8] = 10.0
        scale[2::8] = 10.0
        G = G * scale.view(1, -1, 1)
    elif kind == "long_memory":
        G = G.clone()
        for d in range(2):
            G[:, d * 4 * H + 0 * H:d * 4 * H + 1 * H] += 2.0  # i
            G[:, d * 4 * H + 1 * H:d * 4 * H + 2 * H] += 6.0  # f
    elif kind == "large_whh":
        W = whh(4, 0.25)
    else:
        assert kind == "benign"
    return Case(G.contiguous(), W, HARD_LENS, e32=True, state=True)


def hard_condition(kind):
    """The property of the float64 run that makes `kind` the case it is meant to be; returns a description of what was found
    (asserts inside)."""
    case = hard_case(kind)
    if kind == "saturated":
        a = case.a[np.broadcast_to(case.valid, case.a.shape)]
        share20, top, low = float((np.abs(a) > 20).mean()), float(a.max()), float(a.min())
        assert share20 >= 0.01 and top > 100 and low < -100, (share20, top, low)
        assert float(np.abs(a).max()) > 90
        return "%.1f %% of the pre-activations beyond +-20, range %.0f .. %.0f" % (100 * share20, low, top)
    if kind == "long_memory":
        cmax = float(np.abs(case.c).max())
        assert cmax > 20, cmax
        return "max |c| = %.1f" % cmax
    base = hard_case("benign").e32
    assert case.e32 >= 4 * base, (case.e32, base)
    return "e32 = %.2e against %.2e with +- 1/16" % (case.e32, base)
