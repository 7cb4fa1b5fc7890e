"""The numpy reference of tests/test_lstm_edges_gpu.py (tests/_lstm_ref.py) against two independent statements of the same
recurrence, so that the thing the kernels are held to is not the thing that is wrong: torch.nn.LSTM in float64 with
pack_padded_sequence / pad_packed_sequence, and oracle/ops_ref.lstm_bidir (a per-row Python loop in float32)."""
import numpy as np
import pytest
import torch

import _lstm_ref as L
from oracle import ops_ref as R


def _torch_case(seed, B, N, H, I, lengths):
    """nn.LSTM(I, H, bidirectional).double() on a ragged batch -> (G [B, 8H, N], whh_t [2, H, 4H], reference [B, 2H, N])."""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, N, I, dtype=torch.float64)
    lens = torch.tensor(lengths)
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False)
        ref, _ = torch.nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=N)
        sd = lstm.state_dict()
        G = torch.cat([x @ sd["weight_ih_l0" + sfx].t() + sd["bias_ih_l0" + sfx] + sd["bias_hh_l0" + sfx]
                       for sfx in ("", "_reverse")], dim=2).transpose(1, 2)
        whh_t = torch.stack([sd["weight_hh_l0"].t(), sd["weight_hh_l0_reverse"].t()])
    return G.contiguous().numpy(), whh_t.contiguous().numpy(), ref.transpose(1, 2).numpy()


@pytest.mark.parametrize("B,N,H,lengths", [(1, 9, 8, [9]), (1, 9, 8, [1]), (4, 13, 16, [13, 1, 12, 6]),
                                           (7, 40, 256, [1, 40, 39, 17, 1, 29, 40])])
def test_reference_is_torch_lstm_in_float64(B, N, H, lengths):
    G, whh_t, ref = _torch_case(100 + B + N, B, N, H, 24, lengths)
    out = L.lstm_bidir(G, whh_t, lengths)
    assert out.dtype == np.float64 and out.shape == ref.shape
    e = np.abs(out - ref).max()
    print("ref vs nn.LSTM double: %.3e" % e)
    assert e < 1e-12
    for b, n in enumerate(lengths):
        assert not out[b, :, n:].any(), "outputs past the length are exact zeros"
        assert np.abs(out[b, :, :n]).min() > 0


def test_reference_without_lengths_is_the_full_rows():
    G, whh_t, ref = _torch_case(7, 3, 11, 8, 5, [11, 11, 11])
    assert np.array_equal(L.lstm_bidir(G, whh_t), L.lstm_bidir(G, whh_t, [11, 11, 11]))
    assert np.abs(L.lstm_bidir(G, whh_t) - ref).max() < 1e-12


def test_reference_matches_the_oracle_contract_in_float32():
    """oracle/ops_ref.lstm_bidir is fp32 with another summation order (h @ Wt per row): both fp32 runs sit at fp32 round-off of
    the float64 run, |h| < 1 and twelve steps of a contractive recurrence (2e-6 = 30 ulp of 1.0)."""
    gen = torch.Generator().manual_seed(5)
    B, N, H = 3, 12, 16
    G = torch.randn(B, 8 * H, N, generator=gen)
    whh_t = (torch.rand(2, H, 4 * H, generator=gen) * 2 - 1) / 4
    lens = torch.tensor([12, 1, 7])
    want = R.lstm_bidir(G, whh_t, lens).numpy()
    got32 = L.lstm_bidir(G.numpy(), whh_t.numpy(), lens.numpy(), dtype=np.float32)
    got64 = L.lstm_bidir(G.numpy(), whh_t.numpy(), lens.numpy())
    assert got32.dtype == np.float32
    e = [np.abs(got32 - want).max(), np.abs(want - got64).max(), np.abs(got32 - got64).max()]
    print("fp32 ref vs oracle %.3e, oracle vs fp64 %.3e, fp32 ref vs fp64 %.3e" % tuple(e))
    assert max(e) < 2e-6
    assert not got32[1, :, 1:].any() and not want[1, :, 1:].any()


def test_reference_clamps_lengths_and_never_reads_padding():
    G, whh_t, _ = _torch_case(9, 5, 10, 8, 6, [10, 3, 1, 10, 4])
    lens = [10, 3, 1, 10, 4]
    base = L.lstm_bidir(G, whh_t, lens)
    wild = L.lstm_bidir(G, whh_t, [17, 3, 1, 10, 4])       # N + 7 is N
    assert np.array_equal(base, wild)
    for bad in (0, -3):                                     # 0 and a negative length: an all-zero row, the others untouched
        out = L.lstm_bidir(G, whh_t, [10, bad, 1, 10, 4])
        assert not out[1].any()
        assert np.array_equal(np.delete(out, 1, axis=0), np.delete(base, 1, axis=0))
    Gn = G.copy()
    Gn[~np.broadcast_to(L.valid_mask(lens, 5, 10), G.shape)] = np.nan
    assert np.isnan(Gn).any()
    assert np.array_equal(L.lstm_bidir(Gn, whh_t, lens), base)
    assert not L.lstm_bidir(G, whh_t, [0] * 5).any()


def test_reference_returns_cell_states_and_pre_activations():
    """c and a are what the recurrence used: h = o * tanh(c) with o = sigmoid(a_o), zeros past the length."""
    G, whh_t, _ = _torch_case(11, 3, 8, 8, 6, [8, 5, 1])
    H = 8
    y, c, a = L.lstm_bidir(G, whh_t, [8, 5, 1], want_state=True)
    assert c.shape == y.shape and a.shape == G.shape
    for d in range(2):
        o = 1.0 / (1.0 + np.exp(-a[:, d * 4 * H + 3 * H:(d + 1) * 4 * H]))
        v = L.valid_mask([8, 5, 1], 3, 8)
        assert np.abs(np.where(v, o * np.tanh(c[:, d * H:(d + 1) * H]), 0.0) - y[:, d * H:(d + 1) * H]).max() < 1e-15
    assert not c[1, :, 5:].any() and not a[2, :, 1:].any()
    # the first step of each direction starts from h = 0: its pre-activation is G's column
    assert np.array_equal(a[:, :4 * H, 0], G[:, :4 * H, 0])
    assert np.array_equal(a[1, 4 * H:, 4], G[1, 4 * H:, 4])


@pytest.mark.parametrize("kind", ["saturated", "long_memory", "large_whh"])
def test_hard_cases_meet_their_conditions(kind):
    """The seeds of tests/_lstm_cases.py make each hard case of tests/test_lstm_edges_gpu.py what it is meant to be, judged by
    the float64 run alone: saturation shares, max |c| > 20, an fp32 error of at least 4 x the benign case's."""
    import _lstm_cases as K
    print("%s: %s" % (kind, K.hard_condition(kind)))
    case = K.hard_case(kind)
    assert np.isfinite(case.ref).all() and np.abs(case.ref).max() <= 1.0
