"""TEST INFRASTRUCTURE: the CPU backend of tests/_cpu_backend.py extended to the ragged plans (ABI v23).

`ragged_cpu_backend()` installs the FULL backend table (`_lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED`): the CPU contracts of
tests/_cpu_backend.py for the existing slots, length-aware CPU contracts for the two conv slots (the existing ones ignore the
st2_conv_desc x_len / y_len fields and would take statistics over the padding), and CPU contracts for the new slots.  The
simplest contract throughout: slice row b to its own length, call the oracle/ops_ref function on it, leave or zero the tail as
the header specifies.  tests/_cpu_backend.py is imported, not edited.
"""
import contextlib
import ctypes as C

import torch

import _cpu_backend as CB
from _cpu_backend import _epilogue_kwargs, _gb, _ncl, _prologue_kwargs, _t, _weight
from oracle import ops_ref as R
from styletts2_amd import _lib


def _lens(ptr, B):
    return [int(v) for v in _t(ptr, (B,), (1,), torch.int32)] if ptr else None


def _row_sums(part_ptr, rows, nt, cols, row0, y):
    """Shifted (sum, sum of squares) slots of rows [row0, row0 + C) over y's columns only (y [C, L_b]); slots past them are
    left untouched (st2_stats_finalize_len never reads them)."""
    Cc, L = y.shape
    ns = -(-L // cols)
    part = _t(part_ptr, (rows, nt, 2), (nt * 2, 2, 1))
    shifts = _t(part_ptr + rows * nt * 2 * 4, (rows, nt), (nt, 1))
    for i in range(ns):
        seg = y[:, i * cols:min((i + 1) * cols, L)].double()
        dv = seg - seg[:, :1]
        part[row0:row0 + Cc, i, 0] = dv.sum(-1).float()
        part[row0:row0 + Cc, i, 1] = (dv * dv).sum(-1).float()
        shifts[row0:row0 + Cc, i] = seg[:, 0].float()


def _row_desc(d, b, L_in, L_out):
    """A B = 1 copy of the descriptor addressing row b, at the row's own lengths."""
    r = _lib.ConvDesc()
    C.pointer(r)[0] = d
    r.B, r.L_in, r.L_out = 1, L_in, L_out
    r.x_len = r.y_len = None
    r.part = None
    if d.x:
        r.x = d.x + b * d.x_bs * 4
    r.y = d.y + b * d.y_bs * 4
    if d.res:
        r.res = d.res + b * d.res_bs * 4
    if d.res2:
        r.res2 = d.res2 + b * d.res2_bs * 4
    if d.stats:
        r.stats = d.stats + b * d.C_in * 2 * 4
    if d.gamma and d.gb_bs:
        r.gamma = d.gamma + b * d.gb_bs * 4
        r.beta = d.beta + b * d.gb_bs * 4
    return r


def _conv_rows(d, x_of_row, cols):
    xl, yl = _lens(d.x_len, d.B), _lens(d.y_len, d.B)
    for b in range(d.B):
        Li = min(xl[b], d.L_in) if xl else d.L_in  # values above L_in / L_out are clamped (include/st2.h)
        Lo = min(yl[b], d.L_out) if yl else d.L_out
        r = _row_desc(d, b, Li, Lo)
        y = R._conv1d(x_of_row(r, b, Li), _weight(d), d.C_out, d.ks, **_epilogue_kwargs(r))
        if d.part:
            _row_sums(d.part, d.B * d.C_out, d.part_nt, cols, b * d.C_out, y[0])


def conv1d_f16s(dp, stream):
    d = dp.contents
    if not (d.x_len or d.y_len):
        return CB.conv1d_f16s(dp, stream)

    def x_row(r, b, Li):
        x = _ncl(r.x, r.x_bs, r.x_cs, 1, r.C_in, Li)
        return R.activate(x, **_prologue_kwargs(r.pro, r.slope, r.stats, r.gamma, r.beta, r.gb_bs, r.gamma_plus_one,
                                                r.alpha, 1, r.C_in, Li))
    _conv_rows(d, x_row, 128)
    return 0


def conv1d_xs(dp, stream):
    d = dp.contents
    if not (d.x_len or d.y_len):
        return CB.conv1d_xs(dp, stream)
    planes = _t(d.xs, (d.B, 2, d.xs_cg, d.xs_lp, 8), (2 * d.xs_cg * d.xs_lp * 8, d.xs_cg * d.xs_lp * 8, d.xs_lp * 8, 8, 1),
                torch.float16)
    u = (planes[:, 0].float() + planes[:, 1].float()) / d.x_scale
    u = u.permute(0, 1, 3, 2).reshape(d.B, d.xs_cg * 8, d.xs_lp)[:, :d.C_in, d.xs_halo:d.xs_halo + d.L_in]

    def x_row(r, b, Li):
        return u[b:b + 1, :, :Li].contiguous()
    _conv_rows(d, x_row, getattr(d, "part_cols", 0) or 128)
    return 0


def act_split_len(x, x_bs, x_cs, B, Cc, L, pro, slope, stats, gamma, beta, gb_bs, gb_seg, gamma_plus_one, alpha, x_scale, xs,
                  xs_cg, Lp, halo, length, stream):
    rc = CB.act_split(x, x_bs, x_cs, B, Cc, L, pro, slope, stats, gamma, beta, gb_bs, gb_seg, gamma_plus_one, alpha, x_scale,
                      xs, xs_cg, Lp, halo, stream)
    planes = _t(xs, (B, 2, xs_cg, Lp, 8), (2 * xs_cg * Lp * 8, xs_cg * Lp * 8, Lp * 8, 8, 1), torch.float16)
    for b, n in enumerate(_lens(length, B)):
        planes[b, :, :, halo + n:] = 0  # a select: whatever the activation made of the tail is dropped
    return rc


def instnorm_stats_len(x, x_bs, x_cs, B, Cc, L, eps, stats, length, stream):
    st = _t(stats, (B, Cc, 2), (Cc * 2, 2, 1))
    for b, n in enumerate(_lens(length, B)):
        R.instnorm_stats(_ncl(x + b * x_bs * 4, x_bs, x_cs, 1, Cc, n), eps, out=st[b:b + 1])
    return 0


def stats_finalize_len(part, rows, nt, L, eps, stats, cols, length, len_div, stream):
    lens = _lens(length, rows // len_div)
    p = _t(part, (rows, nt, 2), (nt * 2, 2, 1)).double()
    shift = _t(part + rows * nt * 2 * 4, (rows, nt), (nt, 1)).double()
    st = _t(stats, (rows, 2), (2, 1))
    for r in range(rows):
        Lr = lens[r // len_div]
        ns = -(-Lr // cols)
        n = torch.tensor([min(cols, Lr - i * cols) for i in range(ns)], dtype=torch.float64)
        s1, s2 = p[r, :ns, 0], p[r, :ns, 1]
        mi = shift[r, :ns] + s1 / n
        mean = (n * mi).sum() / Lr
        m2 = ((s2 - s1 * s1 / n) + n * (mi - mean) ** 2).sum()
        var = max(float(m2 / Lr), 0.0)
        st[r, 0] = float(mean)
        st[r, 1] = float(1.0 / (var + eps) ** 0.5)
    return 0


def conv1d_direct_len(x, x_bs, x_cs, w, bias, y, y_bs, y_cs, B, C_in, C_out, L_in, L_out, ks, stride, pad, x_len, y_len,
                      stream):
    xl, yl = _lens(x_len, B), _lens(y_len, B)
    wt = _t(w, (C_out, C_in, ks), (C_in * ks, ks, 1))
    bt = _t(bias, (C_out,), (1,))
    for b in range(B):
        out = _ncl(y + b * y_bs * 4, y_bs, y_cs, 1, C_out, L_out)
        n = xl[b] if xl else L_in
        xr = torch.zeros(1, C_in, L_in)  # the row's own end is its zero padding
        xr[..., :n] = _ncl(x + b * x_bs * 4, x_bs, x_cs, 1, C_in, n)
        R.conv1d_direct(xr, wt, bt, stride, pad, L_out=L_out, out=out)
        if yl:
            out[..., yl[b]:] = 0.0
    return 0


def adain_leaky_pool_len(x, x_bs, x_cs, stats, gamma, beta, gb_bs, slope, w, bias, y, y_bs, y_cs, B, Cc, L, length, stream):
    st = _t(stats, (B, Cc, 2), (Cc * 2, 2, 1))
    g, be = _gb(gamma, gb_bs, B, Cc).expand(B, Cc), _gb(beta, gb_bs, B, Cc).expand(B, Cc)
    for b, n in enumerate(_lens(length, B)):
        R.adain_leaky_pool(_ncl(x + b * x_bs * 4, x_bs, x_cs, 1, Cc, n), st[b:b + 1], g[b:b + 1], be[b:b + 1], slope,
                           _t(w, (Cc, 3), (3, 1)), _t(bias, (Cc,), (1,)), out=_ncl(y + b * y_bs * 4, y_bs, y_cs, 1, Cc, 2 * n))
    return 0


def convt_interleave_stats_len(ph, p_bs, p_cs, Lq, bias, add, a_bs, a_cs, out, o_bs, o_cs, B, Cc, stride, pad, L_raw,
                               reflect_left, part, part_nt, q_len, out_len, stream):
    ql, ol = _lens(q_len, B), _lens(out_len, B)
    for b in range(B):
        Lo = ol[b]
        y = R._convt_interleave(_ncl(ph + b * p_bs * 4, p_bs, p_cs, 1, stride * Cc, ql[b]), Cc, stride, pad,
                                Lo - reflect_left, bias=_t(bias, (Cc,), (1,)),
                                add=_ncl(add + b * a_bs * 4, a_bs, a_cs, 1, Cc, Lo) if add else None,
                                reflect_left=bool(reflect_left), out=_ncl(out + b * o_bs * 4, o_bs, o_cs, 1, Cc, Lo))
        if part:
            _row_sums(part, B * Cc, part_nt, 1024, b * Cc, y[0])
    return 0


def har_source_len(f0, B, Fr, U, H, noise, lin_w, lin_b, sine_amp, noise_std, vthr, sr, scratch, out, f_len, stream):
    o = _t(out, (B, Fr * U), (Fr * U, 1))
    for b, n in enumerate(_lens(f_len, B)):
        y = R.har_source(_t(f0 + b * Fr * 4, (1, n), (Fr, 1)), U,
                         _t(noise + b * Fr * U * H * 4, (1, n * U, H), (Fr * U * H, H, 1)), _t(lin_w, (H,), (1,)),
                         _t(lin_b, (1,), (1,)), sine_amp=sine_amp, noise_std=noise_std, voiced_threshold=vthr, sample_rate=sr)
        o[b, :n * U] = y[0]
        o[b, n * U:] = 0.0
    return 0


def stft_mag_phase_len(x, B, L, n_fft, hop, har, har_bs, har_cs, length, stream):
    h = _ncl(har, har_bs, har_cs, B, n_fft + 2, L // hop + 1)
    for b, n in enumerate(_lens(length, B)):
        n = min(max(n, n_fft // 2 + 1), L)  # clamped as the kernel clamps it (include/st2.h)
        M = n // hop + 1
        h[b, :, :M] = R.stft_mag_phase(_t(x + b * L * 4, (1, n), (L, 1)), n_fft, hop)[0]
        h[b, :, M:] = 0.0
    return 0


def istft_len(sp, sp_bs, sp_cs, B, M, n_fft, hop, wave, wave_bs, m_len, stream):
    w = _t(wave, (B, hop * (M - 1)), (wave_bs, 1))
    for b, m in enumerate(_lens(m_len, B)):
        y = R.istft(_ncl(sp + b * sp_bs * 4, sp_bs, sp_cs, 1, n_fft + 2, m), n_fft, hop)
        w[b, :hop * (m - 1)] = y.reshape(-1)
        w[b, hop * (m - 1):] = 0.0
    return 0


def expand_by_durations_len(x, x_bs, x_cs, dur, B, Cc, N, T, shift, y, y_bs, y_cs, length, stream):
    d = _t(dur, (B, N), (N, 1), torch.int64)
    yv = _ncl(y, y_bs, y_cs, B, Cc, T)
    for b, n in enumerate(_lens(length, B)):
        yv[b:b + 1, :, :n] = R.expand_by_durations(_ncl(x + b * x_bs * 4, x_bs, x_cs, 1, Cc, N), d[b:b + 1], n,
                                                   shift=bool(shift))
        yv[b, :, n:] = 0.0
    return 0


def ragged_lengths(frames, B, T_max, n, coef, out, stream):
    f = [min(max(v, 1), T_max) for v in _lens(frames, B)]
    o = _t(out, (n, B), (B, 1), torch.int32)
    for i in range(n):
        mul, add, div = coef[3 * i], coef[3 * i + 1], coef[3 * i + 2]
        for b in range(B):
            o[i, b] = (mul * f[b] + add) // div
    return 0


_OVERRIDES = {"conv1d_f16s": conv1d_f16s, "conv1d_xs": conv1d_xs}
CALLS = {}  # slot name -> number of calls since the last install (the test checks that the new slots actually ran)


def _counted(name, fn):
    def run(*a):
        CALLS[name] = CALLS.get(name, 0) + 1
        return fn(*a)
    return run


def install():
    """The full table: existing slots (tests/_cpu_backend.py, conv slots length-aware), then the ragged slots."""
    lib = _lib.load()
    names = _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED
    table = (C.c_void_p * len(names))()
    cbs = []
    CALLS.clear()
    for i, name in enumerate(names):
        if name in _OVERRIDES:
            fn = _OVERRIDES[name]
        elif name in _lib.BACKEND_SLOTS_RAGGED:
            fn = globals()[name]
        else:
            fn = getattr(CB, name)
        if name in CB._MEM_TYPES:
            cb = CB._MEM_TYPES[name](fn)
        elif name in CB._SPECIAL_TYPES:
            cb = CB._SPECIAL_TYPES[name](CB._guard(fn))
        else:
            res, args = _lib._SIGNATURES["st2_" + name]
            cb = C.CFUNCTYPE(res, *args)(CB._guard(_counted(name, fn)))
        cbs.append(cb)
        table[i] = C.cast(cb, C.c_void_p)
    _lib.check(lib.st2_debug_set_backend(table, len(names)), "st2_debug_set_backend")
    return cbs, table


@contextlib.contextmanager
def ragged_cpu_backend():
    """tests/_cpu_backend.cpu_backend() (host memory, engine teardown on the host) with the full table installed inside."""
    with CB.cpu_backend():
        keep = install()
        yield keep
