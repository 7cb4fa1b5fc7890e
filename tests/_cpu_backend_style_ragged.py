"""TEST INFRASTRUCTURE: the CPU backend extended to the ragged style plan (st2_style_forward_ragged).

`style_ragged_cpu_backend()` installs the FULL backend table (`_lib.BACKEND_SLOTS + BACKEND_SLOTS_RAGGED + BACKEND_SLOTS_STYLE`):
CPU contracts for the three new slots, the two conv slots made aware of rows of length 0 (the seam rows of the stacked
launches: nothing computed, nothing stored), and tests/_cpu_backend.py / tests/_cpu_backend_ragged.py for the rest.  The
contracts follow the header: slice item b to its own width, evaluate the uniform oracle/ops_ref function on the slice, leave
everything past it untouched.  Neither existing helper is edited.
"""
import contextlib
import ctypes as C

import torch

import _cpu_backend as CB
import _cpu_backend_ragged as CBR
from _cpu_backend import _epilogue_kwargs, _ncl, _prologue_kwargs, _t, _weight
from _cpu_backend_ragged import _lens, _row_desc
from oracle import ops_ref as R
from styletts2_amd import _lib


def _runs(d):
    """(first row, rows, L_in, L_out) of every maximal run of consecutive batch rows with equal lengths and L_out > 0."""
    xl, yl = _lens(d.x_len, d.B), _lens(d.y_len, d.B)
    rows = [(min(xl[b], d.L_in) if xl else d.L_in, min(yl[b], d.L_out) if yl else d.L_out) for b in range(d.B)]
    b = 0
    while b < d.B:
        n = 1
        while b + n < d.B and rows[b + n] == rows[b]:
            n += 1
        if rows[b][1] > 0:
            yield b, n, rows[b][0], rows[b][1]
        b += n


def _run_desc(d, b0, n, Li, Lo):
    r = _row_desc(d, b0, Li, Lo)
    r.B = n
    return r


def conv1d_f16s(dp, stream):
    d = dp.contents
    if not (d.x_len or d.y_len) or d.part:
        return CBR.conv1d_f16s(dp, stream)
    for b0, n, Li, Lo in _runs(d):
        r = _run_desc(d, b0, n, Li, Lo)
        x = R.activate(_ncl(r.x, r.x_bs, r.x_cs, n, r.C_in, Li),
                       **_prologue_kwargs(r.pro, r.slope, r.stats, r.gamma, r.beta, r.gb_bs, r.gamma_plus_one, r.alpha, n,
                                          r.C_in, Li))
        R._conv1d(x, _weight(d), d.C_out, d.ks, **_epilogue_kwargs(r))
    return 0


def conv1d_xs(dp, stream):
    d = dp.contents
    if not (d.x_len or d.y_len) or d.part:
        return CBR.conv1d_xs(dp, stream)
    planes = _t(d.xs, (d.B, 2, d.xs_cg, d.xs_lp, 8), (2 * d.xs_cg * d.xs_lp * 8, d.xs_cg * d.xs_lp * 8, d.xs_lp * 8, 8, 1),
                torch.float16)
    for b0, n, Li, Lo in _runs(d):
        u = (planes[b0:b0 + n, 0].float() + planes[b0:b0 + n, 1].float()) / d.x_scale
        u = u.permute(0, 1, 3, 2).reshape(n, d.xs_cg * 8, d.xs_lp)[:, :d.C_in, d.xs_halo:d.xs_halo + Li].contiguous()
        R._conv1d(u, _weight(d), d.C_out, d.ks, **_epilogue_kwargs(_run_desc(d, b0, n, Li, Lo)))
    return 0


def _widths(w_len, B, W):
    return [min(max(v, 1), W) for v in _lens(w_len, B)]


def dwconv3x3s2_len(x, x_bs, x_hs, x_cs, w, bias, B, Cc, H, W, y, y_bs, y_hs, y_cs, w_len, stream):
    Ho = (H - 1) // 2 + 1
    for b, Wb in enumerate(_widths(w_len, B, W)):
        R.dwconv3x3s2(_t(x + b * x_bs * 4, (1, H, Cc, Wb), (x_bs, x_hs, x_cs, 1)), _t(w, (Cc, 3, 3), (9, 3, 1)),
                      _t(bias, (Cc,), (1,)), _t(y + b * y_bs * 4, (1, Ho, Cc, (Wb + 1) // 2), (y_bs, y_hs, y_cs, 1)))
    return 0


def avgpool2x2_len(x, x_bs, x_hs, x_cs, B, Cc, H, W, y, y_bs, y_hs, y_cs, w_len, stream):
    for b, Wb in enumerate(_widths(w_len, B, W)):
        R.avgpool2x2(_t(x + b * x_bs * 4, (1, H, Cc, Wb), (x_bs, x_hs, x_cs, 1)),
                     _t(y + b * y_bs * 4, (1, H // 2, Cc, (Wb + 1) // 2), (y_bs, y_hs, y_cs, 1)))
    return 0


def style_lengths_table(mel_len, T_min, T_cap, H, stages):
    """The table of include/st2.h st2_style_lengths as a Python list (also the reference of the GPU kernel's test)."""
    B = len(mel_len)
    w = [[min(max(int(v), T_min), T_cap) for v in mel_len]]
    for _ in range(stages):
        w.append([(v + 1) // 2 for v in w[-1]])
    out = [v for row in w for v in row] + [v - 4 for v in w[-1]]
    for i in range(stages + 1):
        h = H >> i
        for r in range(B * (h + 2) - 2):
            b, k = divmod(r + 1, h + 2)
            out.append(0 if k in (0, h + 1) else w[i][b])
    return out


def style_lengths(mel_len, B, T_min, T_cap, H, stages, out, stream):
    tab = style_lengths_table(_lens(mel_len, B), T_min, T_cap, H, stages)
    _t(out, (len(tab),), (1,), torch.int32).copy_(torch.tensor(tab, dtype=torch.int32))
    return 0


_OVERRIDES = {"conv1d_f16s": conv1d_f16s, "conv1d_xs": conv1d_xs}
CALLS = {}  # slot name -> calls since the last install


def _counted(name, fn):
    def run(*a):
        CALLS[name] = CALLS.get(name, 0) + 1
        return fn(*a)
    return run


def install():
    lib = _lib.load()
    names = _lib.BACKEND_SLOTS + _lib.BACKEND_SLOTS_RAGGED + _lib.BACKEND_SLOTS_STYLE
    table = (C.c_void_p * len(names))()
    cbs = []
    CALLS.clear()
    for i, name in enumerate(names):
        if name in _OVERRIDES:
            fn = _OVERRIDES[name]
        elif name in _lib.BACKEND_SLOTS_STYLE:
            fn = globals()[name]
        elif name in _lib.BACKEND_SLOTS_RAGGED:
            fn = getattr(CBR, name)
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
def style_ragged_cpu_backend():
    """tests/_cpu_backend.cpu_backend() (host memory, engine teardown on the host) with the full table installed inside."""
    with CB.cpu_backend():
        keep = install()
        yield keep
