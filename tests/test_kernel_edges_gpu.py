"""Edge shapes and hard inputs for the kernels around the convs: attention, style_fc, the two statistics reductions, STFT /
iSTFT, the harmonic source, adain_leaky_pool and mean_tokens.

The reference is always the contract of oracle/ops_ref.py evaluated on float64 copies of the inputs on the CPU (torch.stft /
torch.istft in their complex128 form with a float64 window); R.har_source stays fp32: it is an op-order contract.  Shapes sit on,
one before and one past every tile / chunk / branch edge of the kernel they are for (named beside each list).

Bars.  Benign data at a new shape is held to the bar the plain test of that kernel asserts in tests/test_ops_gpu.py.  On hard
inputs (large logits, offset-dominated sums, K = 2048 dot products) the reachable error is set by the conditioning of the
input, so the fp32 evaluation of the same contract is measured against the same fp64 reference ON THE SAME INPUTS and the
kernel is held to max(plain bar, 4 x that error) -- 4 for a different but legitimate summation order; the kernel's own output
never enters the bar.  Each hard case prints its (kernel error, fp32-reference error) pair before it asserts (pytest -s); the
pairs measured on an MI355X are written beside the cases."""
import functools
import math

import pytest
import torch

from _util import rel_err
from oracle import ops_ref as R
from styletts2_amd import ops
from styletts2_amd._lib import St2Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
NAN = float("nan")
PI32 = torch.tensor(math.pi, dtype=torch.float32)


@pytest.fixture(autouse=True)
def _own_status():
    """Each case is judged by the status bits of its own launches only (the word is sticky)."""
    torch.cuda.synchronize()
    ops.status(clear=True)


def g(t):
    return None if t is None else t.to(DEV)


def d(t):
    return None if t is None else t.double()


def hard_bar(what, e_kernel, e_fp32, plain):
    """max(plain bar, 4 x the fp32 contract's own error on these inputs); prints the measured pair."""
    bar = max(plain, 4.0 * e_fp32)
    print("HARD %s: kernel %.3e  fp32-contract %.3e  bar %.3e" % (what, e_kernel, e_fp32, bar))
    return bar


# ---- attention --------------------------------------------------------------------------------------------------------------
# attention_kernel: key chunks of 128 (AKT), query blocks of 128 (AQB), MFMA tiles of 32 keys
HEADS, HD = 8, 64
SCALE = HD ** -0.5


def _split(qkv):
    C = HEADS * HD
    return qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]


# one before / on / one past 32, 128, 256, 512; 160 = a whole number of MFMA tiles that is no whole chunk; 513: five query blocks
@pytest.mark.parametrize("N", [1, 31, 32, 33, 127, 128, 129, 160, 255, 256, 257, 511, 513])
def test_attention_boundary_shapes(N):
    gen = torch.Generator().manual_seed(1000 + N)
    qkv = torch.randn(2, 3 * HEADS * HD, N, generator=gen)
    q, k, v = _split(qkv)
    ref = R.attention(d(q), d(k), d(v), HEADS, SCALE)
    t = g(qkv)
    out = ops.attention(*_split(t), HEADS, SCALE)
    assert out.shape == ref.shape
    e = rel_err(out, ref)
    print("attention N=%d: %.3e" % (N, e))
    assert e < 1e-5
    assert ops.status() == 0


def _keylen_cases():
    """B = 4: two lengths from {1, 32, 33, 127, 128, 129, 256, N} (every one of them that fits N is used once per N), one row
    with 0 and one with N + 7 -- the kernel's contract clamps both to 1..N."""
    cases = []
    for N in (129, 257, 300):
        pool = [v for v in (1, 32, 33, 127, 128, 129, 256, N) if v <= N]
        pool = sorted(set(pool))
        for i in range(0, len(pool), 2):
            pair = pool[i:i + 2] if i + 1 < len(pool) else [pool[i], pool[0]]
            # the short row first or last in turn, the out-of-range rows in between
            cases.append((N, (pair[1], 0, N + 7, pair[0]) if (i // 2) % 2 else (0, pair[0], pair[1], N + 7)))
    return cases


KEYLEN_CASES = _keylen_cases()


@functools.lru_cache(maxsize=None)
def _keylen_data(N, lens_):
    gen = torch.Generator().manual_seed(2000 + N + sum(lens_))
    q, k, v = (torch.randn(4, HEADS * HD, N, generator=gen) for _ in range(3))
    clamped = torch.tensor([min(max(n, 1), N) for n in lens_], dtype=torch.int32)
    ref = R.attention(d(q), d(k), d(v), HEADS, SCALE, key_len=clamped)
    return q, k, v, clamped, ref


@pytest.mark.parametrize("N,lens_", KEYLEN_CASES, ids=["N%d_%s" % (n, "_".join(map(str, l))) for n, l in KEYLEN_CASES])
def test_attention_key_len_across_chunks(N, lens_):
    """key_len and N in different key chunks, a last chunk of one key, key_len 0 and N + 7 (clamped to 1 and N): all N query
    columns of every row against the fp64 contract at the clamped lengths."""
    q, k, v, clamped, ref = _keylen_data(N, lens_)
    kl = torch.tensor(lens_, dtype=torch.int32, device=DEV)
    out = ops.attention(g(q), g(k), g(v), HEADS, SCALE, key_len=kl)
    e = max(rel_err(out[b], ref[b]) for b in range(4))  # per row: a short row is not judged by its neighbour's scale
    print("attention key_len N=%d %s: %.3e" % (N, lens_, e))
    assert e < 2e-5
    assert ops.status() == 0


@pytest.mark.parametrize("N,lens_", KEYLEN_CASES, ids=["N%d_%s" % (n, "_".join(map(str, l))) for n, l in KEYLEN_CASES])
def test_attention_padding_keys_are_never_read(N, lens_):
    """K and V columns >= key_len[b] hold NaN: the output is bit for bit that of the run with finite padding."""
    q, k, v, clamped, ref = _keylen_data(N, lens_)
    kl = torch.tensor(lens_, dtype=torch.int32, device=DEV)
    pad = torch.arange(N).view(1, 1, N) >= clamped.view(4, 1, 1)
    kn, vn = k.masked_fill(pad, NAN), v.masked_fill(pad, NAN)
    assert bool(torch.isnan(kn).any()) and bool(torch.isnan(vn).any())
    qg = g(q)
    plain = ops.attention(qg, g(k), g(v), HEADS, SCALE, key_len=kl)
    nan = ops.attention(qg, g(kn), g(vn), HEADS, SCALE, key_len=kl)
    assert bool(torch.isfinite(nan).all())
    assert torch.equal(plain, nan)
    assert ops.status() == 0


def _hard_softmax(kind):
    """N = 257: three key chunks, the last of one key."""
    B, N = 2, 257
    gen = torch.Generator().manual_seed({"large": 31, "dominant": 32, "uniform": 33}[kind])
    q, k, v = (torch.randn(B, HEADS, HD, N, generator=gen) for _ in range(3))
    if kind == "large":       # |logit| up to ~80
        q, k = q * 4.0, k * 4.0
    elif kind == "dominant":  # one key per query ~40 above the rest: key 5 (first tile) for even queries, key 256 (last chunk) for odd
        k[:, :, 0, 256] = 40.0
        k[:, :, 1, 5] = 40.0
        q[:, :, 0, 1::2] = 8.0
        q[:, :, 1, 0::2] = 8.0
    else:                     # every key the same: a uniform softmax (the output is the mean of V) at logits of 60 +- 20 %
        k0 = torch.randn(B, HEADS, HD, 1, generator=gen)
        k = k0.expand(B, HEADS, HD, N).contiguous()
        lvl = 60.0 / SCALE * (1.0 + 0.1 * torch.randn(B, HEADS, 1, N, generator=gen).clamp(-2, 2))
        q = k0 * lvl / k0.pow(2).sum(dim=2, keepdim=True)
    return tuple(t.reshape(B, HEADS * HD, N).contiguous() for t in (q, k, v))


# measured on an MI355X (kernel error, fp32-contract error), both relative to the largest output:
#   large    (|logit| <= 91): 5.6e-6, 5.6e-6 -> bar 2.3e-5        dominant (|logit| <= 44): 1.2e-10, 1.2e-10 -> bar 1e-5
#   uniform  (|logit| <= 72): 4.2e-7, 3.2e-7 -> bar 1e-5
@pytest.mark.parametrize("kind", ["large", "dominant", "uniform"])
def test_attention_hard_softmax(kind):
    """The online-softmax state (running max, the exp(mx - nmx) rescale of the accumulators and of the denominator) under
    logits an unshifted exp cannot take, with the maximum arriving in the first tile and in the very last key."""
    q, k, v = _hard_softmax(kind)
    ref = R.attention(d(q), d(k), d(v), HEADS, SCALE)
    sim = torch.einsum("bhdn,bhdm->bhnm", d(q).reshape(2, HEADS, HD, -1), d(k).reshape(2, HEADS, HD, -1)) * SCALE
    top = sim.abs().max().item()
    assert top > (55.0 if kind != "dominant" else 35.0), "the case is meant to have large logits (%g)" % top
    if kind == "uniform":
        assert rel_err(ref, d(v).mean(dim=2, keepdim=True).expand_as(ref)) < 1e-9
    if kind == "dominant":  # the planted key holds (nearly) all the weight, early for even queries and late for odd ones
        am = sim.argmax(dim=-1)
        assert bool((am[..., 0::2] == 5).all()) and bool((am[..., 1::2] == 256).all())
    e32 = rel_err(R.attention(q, k, v, HEADS, SCALE), ref)
    out = ops.attention(g(q), g(k), g(v), HEADS, SCALE)
    assert bool(torch.isfinite(out).all())
    e = rel_err(out, ref)
    assert e <= hard_bar("attention %s (|logit| <= %.0f)" % (kind, top), e, e32, 1e-5)
    assert ops.status() == 0


@pytest.mark.parametrize("N", [129, 257])
def test_attention_writes_into_channel_slice(N):
    """q, k, v are slices of one [B, 3 * 512, N] buffer; out is a [:, 3:3 + 512] slice of a [B, 518, N + 5] buffer (batch and
    channel strides of its own): everything around the slice is left as it was."""
    gen = torch.Generator().manual_seed(3000 + N)
    B, C = 2, HEADS * HD
    qkv = torch.randn(B, 3 * C, N, generator=gen)
    ref = R.attention(*(d(t) for t in _split(qkv)), HEADS, SCALE)
    t = g(qkv)
    big = torch.full((B, C + 6, N + 5), SENT, device=DEV)
    out = ops.attention(*_split(t), HEADS, SCALE, out=big[:, 3:3 + C, :N])
    assert out.data_ptr() == big[:, 3:3 + C, :N].data_ptr()
    assert rel_err(big[:, 3:3 + C, :N], ref) < 1e-5
    assert bool((big[:, :3] == SENT).all()) and bool((big[:, 3 + C:] == SENT).all()) and bool((big[:, :, N:] == SENT).all())
    assert ops.status() == 0


# ---- style_fc ---------------------------------------------------------------------------------------------------------------
# style_fc_kernel: 8 batch rows x 64 outputs x 16 k-slices per workgroup; K = 2048 is the maximum (96 KB of dynamic LDS)
#   (8, 2048, 130): B = 8 exactly, the LDS maximum, three output blocks with a tail of 2
#   (9, 2047, 64):  a second batch block of one row, K % 4 != 0 (scalar LDS reads, a slice tail loop), J = 64 exactly
#   (1, 3, 5), (32, 37, 63): K < 64 -- most k-slices are empty -- and J < 64;  (3, 64, 1): one output, 4 k per slice
# measured on an MI355X (kernel error, fp32-contract error) over bias x act:  K = 2048: 1.9e-7 .. 3.0e-7, 4.1e-7 .. 8.7e-7;
#   K = 2047: 1.4e-7 .. 2.7e-7, 3.6e-7 .. 6.3e-7 (16 fixed-order k-slices beat one long dot product) -> bar 1e-5 throughout
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_GELU], ids=["none", "gelu"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,K,J", [(8, 2048, 130), (9, 2047, 64), (1, 3, 5), (32, 37, 63), (3, 64, 1)])
def test_style_fc_edges(B, K, J, with_bias, act):
    gen = torch.Generator().manual_seed(4000 + K + J)
    s = torch.randn(B, K, generator=gen)
    wt = torch.randn(K, J, generator=gen) / math.sqrt(K)
    bias = torch.randn(J, generator=gen) if with_bias else None
    ref = R.style_fc(d(s), d(wt), d(bias), act)
    out = ops.style_fc(g(s), g(wt), g(bias), act)
    assert out.shape == ref.shape
    e = rel_err(out, ref)
    bar = 1e-5
    if K >= 2047:  # hard: 2048-term fp32 dot products
        bar = hard_bar("style_fc B=%d K=%d J=%d bias=%d act=%d" % (B, K, J, with_bias, act), e,
                       rel_err(R.style_fc(s, wt, bias, act), ref), 1e-5)
    else:
        print("style_fc B=%d K=%d J=%d: %.3e" % (B, K, J, e))
    assert e <= bar
    assert ops.status() == 0


def test_style_fc_refuses_k_above_2048():
    s, wt = torch.zeros(1, 2049, device=DEV), torch.zeros(2049, 4, device=DEV)
    with pytest.raises(St2Error, match="too large"):
        ops.style_fc(s, wt, None)


# ---- colnorm_stats ----------------------------------------------------------------------------------------------------------
# colnorm_stats_kernel: 64 positions x 16 waves over the channels; the unrolled loop takes 128 channels a turn, the tail loop 16
#   C = 200: both loops;  C = 7: tail loop only, nine waves without a channel;  C = 1: variance 0;  C = 1160 = 9 x 128 + 8: both,
#   L = 1;  C = 128: the unrolled loop alone, L = 63 one short of a block;  L = 64 / 129 / 65: a whole block, two and a bit, one past
@pytest.mark.parametrize("variant", ["plain", "slice", "offset"])
@pytest.mark.parametrize("B,C,L", [(2, 200, 64), (1, 7, 129), (2, 1, 65), (1, 1160, 1), (2, 128, 63)])
def test_colnorm_stats_edges(B, C, L, variant):
    """`slice`: x is [:, 5:5 + C, :L] of a wider tensor (batch and channel strides of its own).  `offset`: 1e3 + randn, the
    E[x^2] - mean^2 form in anything less than fp64 loses the variance.  Measured on an MI355X (kernel error, fp32-contract
    error): 0 .. 9.7e-8, 0 (the contract reduces in fp64 itself; one fp32 rounding of the result apart) -> bar 1e-5."""
    gen = torch.Generator().manual_seed(5000 + C + L)
    x = torch.randn(B, C, L, generator=gen) + (1e3 if variant == "offset" else 0.5)
    ref = R.colnorm_stats(d(x))
    if variant == "slice":
        big = torch.full((B, C + 9, L + 3), NAN, device=DEV)
        big[:, 5:5 + C, :L] = g(x)
        xg = big[:, 5:5 + C, :L]
    else:
        xg = g(x)
    out = ops.colnorm_stats(xg)
    assert out.shape == ref.shape == (B, L, 2)
    e_m, e_r = rel_err(out[..., 0], ref[..., 0]), rel_err(out[..., 1], ref[..., 1])
    bar = 1e-5
    if variant == "offset":  # hard (the contract reduces in fp64 whatever the input type: its fp32 evaluation is the same numbers)
        e32 = max(rel_err(R.colnorm_stats(x)[..., i], ref[..., i]) for i in (0, 1))
        bar = hard_bar("colnorm_stats offset B=%d C=%d L=%d" % (B, C, L), max(e_m, e_r), e32, 1e-5)
    assert e_m <= bar and e_r <= bar, (e_m, e_r)  # mean and rstd each on its own scale
    assert ops.status() == 0


# ---- instnorm_stats ---------------------------------------------------------------------------------------------------------
# instnorm_stats_kernel: 64 threads up to L = 2048, 256 above; 16-byte loads on an aligned row, scalar loads otherwise.  C = 3:
# an odd L puts rows 1 and 2 (and every row of batch item 1) off 16-byte alignment; `shifted` starts the tensor one float into
# its buffer, so an L that is a multiple of 4 has no aligned row at all.
INST_L = [1, 3, 4, 2047, 2048, 2049]


def _inst_dev(x, shifted):
    if not shifted:
        return g(x)
    buf = torch.empty(x.numel() + 1, device=DEV)
    xg = buf[1:].view(x.shape)
    xg.copy_(x)
    assert xg.data_ptr() % 16 == 4
    return xg


def _inst_check(out, ref, what, e32=None):
    e_m, e_r = rel_err(out[..., 0], ref[..., 0]), rel_err(out[..., 1], ref[..., 1])
    bm, br = 1e-6, 1e-5
    if e32 is not None:
        bm, br = hard_bar(what + " mean", e_m, e32[0], 1e-6), hard_bar(what + " rstd", e_r, e32[1], 1e-5)
    assert e_m <= bm and e_r <= br, (what, e_m, e_r)


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("L", INST_L)
def test_instnorm_stats_edges(L, shifted):
    gen = torch.Generator().manual_seed(6000 + L)
    x = torch.randn(2, 3, L, generator=gen) * 2.0 + 5.0
    ref = R.instnorm_stats(d(x))
    xg = _inst_dev(x, shifted)
    out = ops.instnorm_stats(xg)
    _inst_check(out, ref, "instnorm_stats L=%d" % L)
    assert torch.equal(out, ops.instnorm_stats(xg)), "reduction must be bitwise reproducible"
    # the length-aware entry on the same rows (its own branch on an unaligned row)
    lens_ = torch.tensor([L, max(1, L - 1)], dtype=torch.int32)
    out_l = ops.instnorm_stats(xg, lengths=lens_.to(DEV))
    ref_l = torch.stack([R.instnorm_stats(d(x[b:b + 1, :, :int(lens_[b])]))[0] for b in range(2)])
    _inst_check(out_l, ref_l, "instnorm_stats_len L=%d" % L)
    assert ops.status() == 0


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("L", INST_L)
def test_instnorm_stats_constant_rows(L, shifted):
    """A constant row: the mean is the constant exactly, the variance is (clamped to) 0 and rstd = 1 / sqrt(eps) to fp32 rounding."""
    vals = torch.tensor([[2.5, -3.7, 0.0], [1e4, -1e-3, 7.0]])
    x = vals.unsqueeze(-1).expand(2, 3, L).contiguous()
    xg = _inst_dev(x, shifted)
    out = ops.instnorm_stats(xg).cpu()
    assert torch.equal(out[..., 0], vals)
    want = 1.0 / math.sqrt(1e-5)
    ulp = 2.0 ** -15  # of an fp32 number in [256, 512)
    assert float((out[..., 1].double() - want).abs().max()) <= ulp, out[..., 1]
    assert ops.status() == 0


# measured on an MI355X (kernel error, fp32-contract error): mean 0, 0 at every case; rstd 0 .. 1.2e-7, 0 (the contract reduces in
# fp64 itself: the kernel differs from it by at most one fp32 rounding of rstd) -> bars 1e-6 / 1e-5
@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("off", [1e3, 1e4])
@pytest.mark.parametrize("L", [3, 2047, 2048, 2049])
def test_instnorm_stats_offset_dominated(L, off, shifted):
    """off + randn: |mean| is 1e3 .. 1e4 standard deviations.  E[x^2] - mean^2 is safe only because the sums are fp64 -- a float
    accumulator loses rstd altogether here."""
    gen = torch.Generator().manual_seed(6100 + L)
    x = torch.randn(2, 3, L, generator=gen) + off
    ref = R.instnorm_stats(d(x))
    if L > 1000:
        assert 0.9 < float(ref[..., 1].min()) and float(ref[..., 1].max()) < 1.1  # the variance is that of the noise, not lost
    ref32 = R.instnorm_stats(x)
    out = ops.instnorm_stats(_inst_dev(x, shifted))
    _inst_check(out, ref, "instnorm_stats off=%g L=%d" % (off, L),
                e32=(rel_err(ref32[..., 0], ref[..., 0]), rel_err(ref32[..., 1], ref[..., 1])))
    assert ops.status() == 0


# ---- STFT / iSTFT -----------------------------------------------------------------------------------------------------------
def _stft64(x, n_fft, hop):
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    X = torch.stft(x.double(), n_fft, hop, n_fft, window=win, return_complex=True)
    assert X.dtype == torch.complex128
    return torch.cat([X.abs(), X.angle()], dim=1)


def _istft64(sp, n_fft, hop):
    nb = n_fft // 2 + 1
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    sp = sp.double()
    y = torch.istft(sp[:, :nb] * torch.exp(sp[:, nb:] * 1j), n_fft, hop, n_fft, window=win)
    assert y.dtype == torch.float64
    return y.unsqueeze(-2)


def _stft_check(out, ref, nb):
    assert out.shape == ref.shape
    out = out.cpu()
    e_mag = (out[:, :nb].double() - ref[:, :nb]).abs().max().item()
    # phase is ill-conditioned where |X| ~ 0 and wraps at +-pi: compare on the unit circle, weighted by magnitude
    dp = torch.remainder(out[:, nb:].double() - ref[:, nb:] + math.pi, 2 * math.pi) - math.pi
    e_ph = (dp.abs() * ref[:, :nb]).max().item()
    assert e_mag < 2e-5 and e_ph < 5e-5, (e_mag, e_ph)
    # DC and Nyquist have an exactly zero imaginary part: their phase is exactly 0 or +pi, never -pi
    for kbin in (0, nb - 1):
        ph = out[:, nb + kbin]
        assert bool(((ph == 0.0) | (ph == PI32)).all()), "bin %d: %s" % (kbin, ph[(ph != 0.0) & (ph != PI32)][:4])


# L = n_fft / 2 + 1: the shortest row the entry takes -- one frame reflects at both ends; (32, 1): a frame per sample;
# (2, 1): DC and Nyquist only; (20, 7): hop divides neither n_fft nor L; 4003 / 5 + 1 = 801 frames: four workgroups with a tail
STFT_CASES = [(20, 5, 11), (20, 5, 4003), (16, 4, 9), (32, 8, 1000), (32, 1, 300), (2, 1, 50), (20, 7, 1001)]


@pytest.mark.parametrize("n_fft,hop,L", STFT_CASES)
def test_stft_edges(n_fft, hop, L):
    gen = torch.Generator().manual_seed(7000 + n_fft + hop + L)
    x = torch.tanh(torch.randn(2, L, generator=gen))
    ref = _stft64(x, n_fft, hop)
    out = ops.stft_mag_phase(g(x), n_fft, hop)
    _stft_check(out, ref, n_fft // 2 + 1)
    assert ops.status() == 0


@pytest.mark.parametrize("n_fft,hop,L", [(20, 5, 4003), (16, 4, 9)])
def test_stft_writes_into_strided_out(n_fft, hop, L):
    gen = torch.Generator().manual_seed(7100 + L)
    x = torch.tanh(torch.randn(2, L, generator=gen))
    ref = _stft64(x, n_fft, hop)
    M = L // hop + 1
    big = torch.full((2, n_fft + 7, M + 4), SENT, device=DEV)
    view = big[:, 2:2 + n_fft + 2, 1:1 + M]
    ops.stft_mag_phase(g(x), n_fft, hop, out=view)
    _stft_check(view, ref, n_fft // 2 + 1)
    assert torch.equal(view, ops.stft_mag_phase(g(x), n_fft, hop)), "the strides must not change a bit"
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, 2:2 + n_fft + 2, 1:1 + M] = False
    assert bool((big[keep] == SENT).all())
    assert ops.status() == 0


def test_stft_dc_phase_of_a_negative_signal_is_exactly_pi():
    """x = -1 - 0.1 rand: every DC bin is real and negative, its phase is float32(pi) bit for bit (atan2(+0, re < 0))."""
    gen = torch.Generator().manual_seed(7200)
    x = -1.0 - 0.1 * torch.rand(2, 403, generator=gen)
    ref = _stft64(x, 20, 5)
    assert bool((ref[:, 11] == math.pi).all())  # the reference's own DC phases
    out = ops.stft_mag_phase(g(x), 20, 5)
    _stft_check(out, ref, 11)
    assert bool((out[:, 11].cpu() == PI32).all())
    assert ops.status() == 0


# FRP, m_base, m_lo and the twiddle index wrap all depend on (n_fft, hop); 2 to 32 frames overlap at a sample.
# M = 2: the shortest signal (hop samples);  3: every sample still sees a signal edge;  52: one workgroup;  801: several at hop >= 1
ISTFT_PAIRS = [(20, 5), (16, 4), (32, 8), (32, 16), (20, 10), (20, 4), (8, 2), (4, 1), (2, 1), (32, 1)]


def _istft_input(n_fft, hop, M, B=2):
    gen = torch.Generator().manual_seed(8000 + 100 * n_fft + 10 * hop + M)
    nb = n_fft // 2 + 1
    return torch.cat([torch.exp(torch.randn(B, nb, M, generator=gen)),
                      (torch.rand(B, nb, M, generator=gen) * 2.0 - 1.0) * math.pi], 1)


@pytest.mark.parametrize("M", [2, 3, 52, 801])
@pytest.mark.parametrize("n_fft,hop", ISTFT_PAIRS)
def test_istft_edges(n_fft, hop, M):
    sp = _istft_input(n_fft, hop, M)
    ref = _istft64(sp, n_fft, hop)
    out = ops.istft(g(sp), n_fft, hop).cpu()
    assert out.shape == ref.shape == (2, 1, hop * (M - 1))
    e = (out.double() - ref).abs().max().item()
    assert e < 2e-5 * ref.abs().max().item() + 1e-6, e
    assert ops.status() == 0


@pytest.mark.parametrize("n_fft,hop,M", [(20, 5, 52), (16, 4, 801), (32, 16, 2)])
def test_istft_strided_operands(n_fft, hop, M):
    """sp is a channel / column slice of a wider tensor, out a row of a wider buffer (wave_bs > hop * (M - 1)): the slack
    behind every row is left as it was."""
    sp = _istft_input(n_fft, hop, M)
    ref = _istft64(sp, n_fft, hop)
    big = torch.full((2, n_fft + 5, M + 4), NAN, device=DEV)
    big[:, 1:1 + n_fft + 2, 2:2 + M] = g(sp)
    Lw = hop * (M - 1)
    wide = torch.full((2, 1, Lw + 9), SENT, device=DEV)
    ops.istft(big[:, 1:1 + n_fft + 2, 2:2 + M], n_fft, hop, out=wide[:, :, :Lw])
    e = (wide[:, :, :Lw].cpu().double() - ref).abs().max().item()
    assert e < 2e-5 * ref.abs().max().item() + 1e-6, e
    assert torch.equal(wide[:, :, :Lw], ops.istft(g(sp), n_fft, hop)), "the strides must not change a bit"
    assert bool((wide[:, :, Lw:] == SENT).all())
    assert ops.status() == 0


# ---- har_source -------------------------------------------------------------------------------------------------------------
# sinegen_phase_kernel: one wave per (b, h) row, lane i scans ceil(F / 64) frames: F = 1 (one lane, i1 = min(1, F - 1) = 0),
# 64 (one frame a lane), 65 (two: the last lanes are empty), 1025 / 2048 (17 / 32 a lane, past the 2^10 frames the kernel's
# exactness note speaks of), 130 x 7 (an odd up-sampling factor: the frame-rate source index is a whole number).
# Measured on an MI355X at F = 1025 / 2048: max |difference| 1.5e-8 .. 1.5e-7, no sample above 1e-4 -- the fp64 prefix sums of
# these rows are still exact (terms of 24 bits, none below 2^-9 but exact zeros, 2^11 of them: 44 bits), so the scan order is free.
HAR_SMALL = [(1, 300), (64, 300), (65, 300), (130, 7)]
HAR_LONG = [(1025, 300), (2048, 60)]
HAR_CASES = ([(F, U, H, "base") for F, U in HAR_SMALL for H in (1, 9, 64)] + [(F, U, H, "base") for F, U in HAR_LONG for H in (1, 9)] +
             [(F, U, 9, v) for F, U in HAR_SMALL + HAR_LONG for v in ("zero_row", "nondefault")])


@pytest.mark.parametrize("F,U,H,variant", HAR_CASES)
def test_har_source_edges(F, U, H, variant):
    """Against R.har_source (fp32: the contract is ATen-CPU's op order) at 2e-5 absolute.  Every row mixes voiced frames,
    0 Hz, negative F0 and frames EXACTLY at voiced_threshold (the contract compares with a strict >); `zero_row`: row 1 is 0 Hz
    throughout; `nondefault`: sine_amp 0.2, noise_std 0.01, voiced_threshold 55."""
    gen = torch.Generator().manual_seed(9000 + F + U + H)
    B = 2
    kw = dict(sine_amp=0.2, noise_std=0.01, voiced_threshold=55.0) if variant == "nondefault" else {}
    thr = kw.get("voiced_threshold", 10.0)
    f0 = torch.rand(B, F, generator=gen) * 300.0 + 80.0
    f0[0, : F // 4] = 0.0
    f0[1, F // 2: F // 2 + 3] = -40.0
    f0[:, 2::7] = thr               # exactly at the threshold: unvoiced
    f0[1, 3::11] = thr * 0.5        # below it
    if variant == "zero_row":
        f0[1] = 0.0
    noise = torch.randn(B, F * U, H, generator=gen)
    lw = torch.randn(H, generator=gen) * 0.5
    lb = torch.randn(1, generator=gen) * 0.1
    ref = R.har_source(f0, U, noise, lw, lb, **kw)
    out = ops.har_source(g(f0), U, g(noise), g(lw), g(lb), **kw).cpu()
    assert out.shape == ref.shape == (B, F * U)
    diff = (out - ref).abs()
    print("har_source F=%d U=%d H=%d %s: max %.3e, frac > 1e-4: %.3e" % (F, U, H, variant, diff.max().item(),
                                                                         (diff > 1e-4).float().mean().item()))
    assert diff.max().item() < 2e-5, "max %g, frac>1e-4: %g" % (diff.max().item(), (diff > 1e-4).float().mean().item())
    assert ops.status() == 0


def test_har_source_refuses_more_than_64_harmonics():
    f0 = torch.full((1, 4), 100.0, device=DEV)
    with pytest.raises(St2Error, match="bad geometry"):
        ops.har_source(f0, 10, torch.zeros(1, 40, 65, device=DEV), torch.zeros(65, device=DEV), torch.zeros(1, device=DEV))


# ---- adain_leaky_pool, mean_tokens ------------------------------------------------------------------------------------------
# adain_leaky_pool_kernel: 256 outputs a workgroup, 2 L outputs a row: L = 1 (both outputs see the zero padding), 2, 128 (2 L = 256:
# a full block), 129 (258: two outputs in a second block), 600 (five blocks)
@pytest.mark.parametrize("variant", ["plain", "strided", "nobias"])
@pytest.mark.parametrize("L", [1, 2, 128, 129, 600])
def test_adain_leaky_pool_edges(L, variant):
    gen = torch.Generator().manual_seed(10000 + L)
    B, C = 2, 5
    x = torch.randn(B, C, L, generator=gen) + 1.0
    st = R.instnorm_stats(x)
    h = torch.randn(B, 2 * C, generator=gen) * 0.3
    w = torch.randn(C, 3, generator=gen)
    b = None if variant == "nobias" else torch.randn(C, generator=gen)
    ref = R.adain_leaky_pool(d(x), d(st), d(h[:, :C]), d(h[:, C:]), 0.2, d(w), d(b))
    hg = g(h)
    if variant == "strided":
        big_in = torch.full((B, C + 3, L + 5), NAN, device=DEV)
        big_in[:, 1:1 + C, :L] = g(x)
        big_out = torch.full((B, C + 4, 2 * L + 6), SENT, device=DEV)
        view = big_out[:, 2:2 + C, :2 * L]
        out = ops.adain_leaky_pool(big_in[:, 1:1 + C, :L], g(st), hg[:, :C], hg[:, C:], 0.2, g(w), g(b), out=view)
        keep = torch.ones_like(big_out, dtype=torch.bool)
        keep[:, 2:2 + C, :2 * L] = False
        assert bool((big_out[keep] == SENT).all())
    else:
        out = ops.adain_leaky_pool(g(x), g(st), hg[:, :C], hg[:, C:], 0.2, g(w), g(b))
    assert out.shape == ref.shape == (B, C, 2 * L)
    assert rel_err(out, ref) < 1e-5
    assert ops.status() == 0


# mean_tokens_kernel: one wave a row: N = 1 (one lane), 64 (one token a lane), 65 (lane 0 has two)
# measured on an MI355X at 1e4 + randn (kernel error, fp32-contract error): N = 1: 0, 0;  64: 4.9e-8, 1.1e-7;  65: 4.8e-8, 1.3e-7
# -> bar 1e-6
@pytest.mark.parametrize("variant", ["plain", "slice", "offset"])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_mean_tokens_edges(N, variant):
    gen = torch.Generator().manual_seed(11000 + N)
    B, C = 3, 40
    x = torch.randn(B, C, N, generator=gen) + (1e4 if variant == "offset" else 0.0)
    ref = R.mean_tokens(d(x))
    if variant == "slice":
        big = torch.full((B, C + 9, N + 3), NAN, device=DEV)
        big[:, 5:5 + C, :N] = g(x)
        xg = big[:, 5:5 + C, :N]
    else:
        xg = g(x)
    out = ops.mean_tokens(xg)
    assert out.shape == ref.shape == (B, C)
    e = rel_err(out, ref)
    bar = 1e-6
    if variant == "offset":
        bar = hard_bar("mean_tokens offset N=%d" % N, e, rel_err(R.mean_tokens(x), ref), 1e-6)
    assert e <= bar
    assert ops.status() == 0
