"""The contract of `st2_durations_fit` (include/st2.h) in plain numpy and Python ints: every row of the
integer durations rewritten to a stated total of frames by largest-remainder apportionment of the excess over one frame per
token.  `fit` is the statement the kernel is held to bit for bit; `fit_row_brute` apportions by sorting (-r, index) tuples and
shares no line of step 6 with it."""
import numpy as np

I32_MAX = 2 ** 31 - 1
OK, NEAREST, NOTHING_FREE, REFUSED = range(4)  # the flag column of the report


def _sums(dur, n_b, hold):
    v = [max(int(d), 1) for d in dur[:n_b]]
    held = [hold is not None and bool(hold[n]) for n in range(n_b)]
    S = sum(min(x, 2 ** 31) for x in v)  # a term is saturated so that 512 of them cannot wrap; S <= 2^31 - 1 is exact either way
    return v, held, S


def _unfitted(dur, n_b, target, hold, T_cap):
    """Steps 1-5: (out, report) of a row that is not apportioned, else (None, (v, held, S, lo, T', flag))."""
    N = len(dur)
    n_b = min(max(int(n_b), 0), N)
    v, held, S = _sums(dur, n_b, hold)
    S_rep = min(S, I32_MAX)
    same = [int(d) for d in dur]
    if target <= 0:
        return same, (S_rep, S_rep, OK, 0)
    if n_b == 0:
        return [0] * N, (0, 0, NOTHING_FREE, 0)
    if S > I32_MAX:
        return same, (S_rep, S_rep, REFUSED, 0)
    lo = sum(x if h else 1 for x, h in zip(v, held))
    if lo > T_cap:
        return same, (S, S, REFUSED, 0)
    if all(held):
        return same, (S, S, NOTHING_FREE, 0)
    T = min(max(int(target), lo), int(T_cap))
    return None, (v, held, S, lo, T, OK if T == target else NEAREST)


def fit_row(dur, n_b, target, hold, T_cap):
    """One row: dur a sequence of N ints, n_b its token count (clamped to 0..N), target its frame target, hold a sequence of N
    flags or None -> (out: list of N ints, report: (S, T', flag, changed))."""
    N = len(dur)
    out, rest = _unfitted(dur, n_b, target, hold, T_cap)
    if out is not None:
        return out, rest
    v, held, S, lo, T, flag = rest
    n_b = len(v)
    m = [0 if h else x - 1 for x, h in zip(v, held)]
    R, M = T - lo, sum(m)
    if M == 0:  # every free token is one frame long
        m = [0 if h else 1 for h in held]
        M = sum(m)
    q = [R * x // M for x in m]
    r = [R * x % M for x in m]
    K = R - sum(q)
    # a token's rank: how many tokens with m > 0 come before it -- a larger remainder, or the same one at a lower index
    rr, live, idx = np.array(r, dtype=np.int64), np.array(m, dtype=np.int64) > 0, np.arange(n_b)
    before = ((rr[None, :] > rr[:, None]) | ((rr[None, :] == rr[:, None]) & (idx[None, :] < idx[:, None]))) & live[None, :]
    rank = before.sum(axis=1)
    extra = [int(live[n] and rank[n] < K) for n in range(n_b)]
    out = [(v[n] if held[n] else 1 + q[n] + extra[n]) for n in range(n_b)] + [0] * (N - n_b)
    return out, (S, T, flag, sum(int(out[n] != int(dur[n])) for n in range(n_b)))


def fit_row_brute(dur, n_b, target, hold, T_cap):
    """The same row with step 6 as a sort of (-r, index) tuples."""
    N = len(dur)
    out, rest = _unfitted(dur, n_b, target, hold, T_cap)
    if out is not None:
        return out, rest
    v, held, S, lo, T, flag = rest
    free = [n for n in range(len(v)) if not held[n]]
    w = {n: v[n] - 1 for n in free}
    if not any(w.values()):
        w = {n: 1 for n in free}
    R, M = T - lo, sum(w.values())
    got = {n: 1 + R * w[n] // M for n in free}
    order = sorted((-(R * w[n] % M), n) for n in free if w[n] > 0)
    for _, n in order[:T - lo - sum(g - 1 for g in got.values())]:
        got[n] += 1
    out = [got.get(n, v[n]) for n in range(len(v))] + [0] * (N - len(v))
    return out, (S, T, flag, sum(int(out[n] != int(dur[n])) for n in range(len(v))))


def fit(dur, lengths, target, hold, T_cap, row=fit_row):
    """dur [B][N] (any integers), lengths [B] or None, target [B], hold [B][N] or None -> (out int64 [B, N], report int32 [B, 4])."""
    dur = [[int(x) for x in r] for r in np.asarray(dur, dtype=object).tolist()]
    B, N = len(dur), len(dur[0])
    outs, reps = [], []
    for b in range(B):
        o, rep = row(dur[b], N if lengths is None else int(lengths[b]), int(target[b]), None if hold is None else hold[b], T_cap)
        outs.append(o)
        reps.append(rep)
    return np.array(outs, dtype=np.int64).reshape(B, N), np.array(reps, dtype=np.int32).reshape(B, 4)


def random_row(rng, N=None, kind=None):
    """One random case of the property tests: (dur, n_b, target, hold, T_cap) with held / free mixes, all-ones rows and targets
    from 1 to 3 S, under a capacity that sometimes binds."""
    N = int(rng.integers(1, 41)) if N is None else N
    kind = int(rng.integers(0, 4)) if kind is None else kind
    dur = rng.integers(0, 30, size=N) if kind else np.ones(N, dtype=np.int64)  # (0 counts as 1)
    if kind == 3:
        dur = np.full(N, int(rng.integers(1, 9)))  # all equal: every remainder ties
    n_b = N if rng.random() < 0.5 else int(rng.integers(0, N + 1))
    hold = None if rng.random() < 0.4 else (rng.random(N) < rng.choice([0.1, 0.5, 1.0])).astype(np.uint8)
    S = int(np.maximum(dur[:n_b], 1).sum())
    target = int(rng.integers(1, 3 * max(S, 1) + 1))
    T_cap = int(rng.choice([max(S // 2, 1), max(S, 1), 4 * max(S, 1)]))
    return [int(x) for x in dur], n_b, target, None if hold is None else [int(h) for h in hold], T_cap
