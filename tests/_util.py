"""Shared helpers for the parity tests."""
import json
import math
import os

import torch

from oracle import ops_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Parity bars from BASELINE.json's north_star: "within 1e-3 mel L1 and 1e-4 waveform RMS".
WAVE_RMS_TOL = 1e-4
MEL_L1_TOL = 1e-3


def manifest(tag):
    from benchdata import manifest as _m  # benchdata/manifests/manifest_<tag>.json
    return _m(tag)


def decoder_kwargs(dc, hidden=512, style_dim=128, n_mels=80):
    kw = dict(dim_in=hidden, style_dim=style_dim, dim_out=n_mels,
              resblock_kernel_sizes=dc["resblock_kernel_sizes"], upsample_rates=dc["upsample_rates"],
              upsample_initial_channel=dc["upsample_initial_channel"],
              resblock_dilation_sizes=dc["resblock_dilation_sizes"],
              upsample_kernel_sizes=dc["upsample_kernel_sizes"], kind=dc["type"])
    if dc["type"] == "istftnet":
        kw.update(gen_istft_n_fft=dc["gen_istft_n_fft"], gen_istft_hop_size=dc["gen_istft_hop_size"])
    return kw


def rms(x):
    return x.detach().double().pow(2).mean().sqrt().item()


def phase_err_weighted(har_a, har_b, nb):
    """|wrap(phase_a - phase_b)| * |X|: the harmonic-STFT phase is ill-conditioned where |X| ~ 0 and wraps at
    +-pi, so it is compared on the unit circle weighted by the magnitude."""
    d = torch.remainder(har_a[:, nb:] - har_b[:, nb:] + math.pi, 2 * math.pi) - math.pi
    return (d.abs() * har_b[:, :nb]).max().item()


def mel_l1(wave_a, wave_b):
    """The second parity metric of BASELINE.json's north_star: L1 distance between the reference's normalised log-mel
    spectrograms ((log(1e-5 + mel) + 4) / 4 of MelSpectrogram(n_mels=80, n_fft=2048, win_length=1200, hop_length=300),
    meldataset.py:58-66) of two waveforms [..., L], evaluated on the CPU."""
    from oracle.mel_ref import mel_spectrogram_t  # fp64 evaluation of torchaudio's documented algorithm: not product code
    a = mel_spectrogram_t(wave_a.detach().cpu().float().reshape(-1, wave_a.shape[-1]))
    b = mel_spectrogram_t(wave_b.detach().cpu().float().reshape(-1, wave_b.shape[-1]))
    return (a - b).abs().mean().item()


# ---- per-kernel parity helpers (tests/test_ops_gpu.py, tests/test_ragged_kernels_gpu.py) ----
def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def make_conv_case(seed, B, C_in, C_out, L, ks, dil, pro, act=R.ACT_NONE, res=False, res2=False, res_shift=0,
                   div=1.0, pad_left=None, L_out=None, bias=True, sliced=False):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    x = r(B, C_in, L) * 1.5 + 0.3
    w = r(C_out, C_in, ks) / math.sqrt(C_in * ks)
    kw = dict(dil=dil, pad_left=(ks - 1) * dil // 2 if pad_left is None else pad_left, L_out=L_out,
              bias=r(C_out) if bias else None, pro=pro, div=div, act=act)
    Lo = L if L_out is None else L_out
    if pro in (R.PRO_LEAKY, R.PRO_ADAIN_LEAKY):
        kw["slope"] = 0.2
    if pro in (R.PRO_ADAIN_LEAKY, R.PRO_ADAIN_SNAKE):
        kw["stats"] = R.instnorm_stats(x)
        h = r(B, 2 * C_in + 3) * 0.5
        kw["gamma"], kw["beta"] = h[:, 1:1 + C_in], h[:, 1 + C_in:1 + 2 * C_in]
    if pro == R.PRO_COLNORM:
        kw["stats"] = R.colnorm_stats(x)
        kw["gamma"], kw["beta"] = r(1, C_in), r(1, C_in)
    if pro in (R.PRO_ADAIN_SNAKE, R.PRO_SNAKE):
        kw["alpha"] = torch.rand(C_in, generator=gen) + 0.5
    if res:
        kw["res"] = r(B, C_out, (Lo + (1 << res_shift) - 1) >> res_shift)
        kw["res_shift"] = res_shift
    if res2:
        kw["res2"] = r(B, C_out, Lo)
    if act == R.ACT_EXP_SIN:
        kw["act_split"] = C_out // 2
    if act == R.ACT_LEAKY:
        kw["act_slope"] = 0.1
    return x, w, kw
