"""numpy restatement of the contract of oracle/ops_ref.lstm_bidir (include/st2.h `st2_lstm_bidir`), vectorised over the batch
and both directions so that a chain of a thousand steps is a thousand small matrix products.

    a_t = G[:, t] + h_{t-1} W_hh^T      gate order i, f, g, o (PyTorch); whh_t is [2][H][4H] = W_hh transposed per direction
    i, f, o = 1 / (1 + exp(-a)),  g = tanh(a);   c_t = f c_{t-1} + i g;   h_t = o tanh(c_t)

Packed-sequence semantics: row b runs len[b] steps, forward from t = 0, reverse from t = len[b] - 1; outputs at t >= len[b] are
exact zeros and nothing of G at t >= len[b] enters the result (NaN there is harmless).  Lengths are clamped to [0, N], as the
kernels clamp a device length.

`dtype` is the precision of EVERY operation: float64 is the reference the kernels are held to, the same code in float32 is
"the fp32 contract" whose own distance from the float64 run sets the bar of the long and hard cases (it writes the sigmoid as
the kernels do, so exp overflows to inf and the quotient to 0 exactly where theirs does)."""
import numpy as np


def clamp_lengths(lengths, B, N):
    if lengths is None:
        return np.full((B,), N, dtype=np.int64)
    lens = np.asarray(lengths).astype(np.int64).reshape(-1)
    assert lens.shape == (B,), (lens.shape, B)
    return np.clip(lens, 0, N)


def valid_mask(lengths, B, N):
    """[B, 1, N] bool: t < len[b] (clamped)."""
    return (np.arange(N)[None, :] < clamp_lengths(lengths, B, N)[:, None])[:, None, :]


def lstm_bidir(G, whh_t, lengths=None, dtype=np.float64, want_state=False):
    """G [B, 8H, N] (rows 0..4H-1 forward, 4H..8H-1 reverse), whh_t [2, H, 4H], lengths [B] or None -> Y [B, 2H, N] in `dtype`.
    want_state: also the cell states c [B, 2H, N] and the gate pre-activations a [B, 8H, N] (zeros at t >= len)."""
    dtype = np.dtype(dtype).type
    G = np.asarray(G)
    W =np.ascontiguousarray(np.asarray(whh_t), dtype=dtype)
    B, R, N = G.shape
    H = R // 8
    assert R == 8 * H and W.shape == (2, H, 4 * H), (G.shape, W.shape)
    lens = clamp_lengths(lengths, B, N)
    Gt = np.ascontiguousarray(G.reshape(B, 2, 4 * H, N).transpose(1, 3, 0, 2))  # [2, N, B, 4H] in the caller's precision
    Yt = np.zeros((2, N, B, H), dtype=dtype)
    Ct = np.zeros((2, N, B, H), dtype=dtype) if want_state else None
    At = np.zeros((2, N, B, 4 * H), dtype=dtype) if want_state else None
    h = np.zeros((2, B, H), dtype=dtype)
    c = np.zeros((2, B, H), dtype=dtype)
    rows = np.arange(B)
    one = dtype(1.0)
    with np.errstate(over="ignore"):  # exp(-a) = inf for a < -88.7 in float32: 1 / (1 + inf) = 0, the contract's value
        for s in range(int(lens.max()) if B else 0):
            act = s < lens
            t_rev = np.clip(lens - 1 - s, 0, N - 1)  # rows that are done gather a column they never use
            x = np.stack([Gt[0, min(s, N - 1)], Gt[1, t_rev, rows]]).astype(dtype)  # [2, B, 4H]
            a = x + np.matmul(h, W)
            iv = one / (one + np.exp(-a[..., :H]))
            fv = one / (one + np.exp(-a[..., H:2 * H]))
            gv = np.tanh(a[..., 2 * H:3 * H])
            ov = one / (one + np.exp(-a[..., 3 * H:]))
            cn = fv * c + iv * gv
            hn = ov * np.tanh(cn)
            m = act[None, :, None]
            c = np.where(m, cn, c)
            h = np.where(m, hn, h)
            live = rows[act]
            Yt[0, s, live] = hn[0, live]
            Yt[1, t_rev[live], live] = hn[1, live]
            if want_state:
                Ct[0, s, live] = cn[0, live]
                Ct[1, t_rev[live], live] = cn[1, live]
                At[0, s, live] = a[0, live]
                At[1, t_rev[live], live] = a[1, live]
    back = lambda T: np.ascontiguousarray(T.transpose(2, 0, 3, 1)).reshape(B, -1, N)  # [2, N, B, X] -> [B, 2X, N]
    Y = back(Yt)
    return (Y, back(Ct), back(At)) if want_state else Y
