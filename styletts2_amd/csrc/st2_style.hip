// Reference-audio style path: the pieces of the mel front-end (meldataset.py:58-66 ->
// torchaudio MelSpectrogram) and of StyleEncoder (models.py:139-164) that are not a Conv1d-shaped GEMM.  The GEMM-shaped
// parts -- the windowed DFT (a k=1 conv over frame columns), the mel filter bank, every 3x3 / 5x5 / 1x1 Conv2d (as a
// Conv1d over the width with the kernel rows stacked along the channels, see styletts2_amd/style.py) -- run on the
// split-f16 MFMA conv kernels.  Everything here is HBM-bound elementwise / gather work on small tensors.
//
// 2-D feature maps are stored row-major over (h, c, w): element (b, h, c, w) at x + b*x_bs + h*x_hs + c*x_cs + w, so
// that one image row (all channels) is an NCL tensor [C][W] and three consecutive rows are the 3C-channel input of the
// row-stacked Conv1d.
#include "st2_common.h"

namespace {

// Row lengths: every map / frame kernel below takes a nullable `len` (int32 [B] on the device).  NULL is the plain entry point:
// every row at capacity.  Otherwise row b is the clip / map of its own length: whatever the memory past that length holds is
// never read (a select), and a workgroup whose chunk lies wholly past the row's end leaves at once.

// frames[b][c][m] = wave[b][reflect(m*hop + c - shift)], c < n_win, m < M: the columns of torch.stft's frame matrix
// (center=True, pad_mode="reflect") restricted to the n_win taps where the zero-padded window is non-zero
// (shift = n_fft/2 - (n_fft - n_win)/2).  The reflection is about the row's own [0, L_b), L_b = len[b] clamped to [L_min, L]
// (L without len); frame columns at or past M_b = L_b / hop + 1 are written as exact zeros (the k = 1 DFT and filter-bank convs
// behind it then never see the tail).  m_len (optional, with len only): M_b per row, for the passes behind the convs.
__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ wave, int64_t w_bs, int L, int L_min,
                                                          int n_win, int hop, int shift, int M,
                                                          const int32_t* __restrict__ len, float* __restrict__ fr,
                                                          int64_t f_bs, int f_cs, int32_t* __restrict__ m_len) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const int b = blockIdx.z;
  const int Lb = len ? min(max(len[b], L_min), L) : L;
  const int Mb = Lb / hop + 1;
  if (m_len && blockIdx.x == 0 && c == 0 && threadIdx.x == 0) m_len[b] = Mb;
  if (m >= M) return;
  float v = 0.f;
  if (m < Mb) {
    int i = m * hop + c - shift;
    if (i < 0) i = -i;
    if (i >= Lb) i = 2 * (Lb - 1) - i;
    v = wave[(int64_t)b * w_bs + min(max(i, 0), Lb - 1)];  // the clamp never moves an index either entry point admitted
  }
  fr[(int64_t)b * f_bs + (int64_t)c * f_cs + m] = v;
}

// p[b][k][m] = y[b][k][m]^2 + y[b][K + k][m]^2   (|X_k|^2 from the stacked real / imaginary DFT rows)
__global__ __launch_bounds__(256) void power_spectrum_kernel(const float* __restrict__ y, int64_t y_bs, int y_cs, int K,
                                                             int M, float* __restrict__ p, int64_t p_bs, int p_cs) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  const int b = blockIdx.z;
  if (m >= M) return;
  const float re = y[(int64_t)b * y_bs + (int64_t)k * y_cs + m];
  const float im = y[(int64_t)b * y_bs + (int64_t)(K + k) * y_cs + m];
  p[(int64_t)b * p_bs + (int64_t)k * p_cs + m] = re * re + im * im;
}

// x[b][c][m] = m < len[b] ? (log(eps + x[b][c][m]) - mean) / std : 0  in place (meldataset.py:63-65).  The flat plain entry is
// the one-row case (B = C = 1, M = n, no len): the column index is 64-bit for it.
__global__ __launch_bounds__(256) void log_norm_kernel(float* __restrict__ x, int64_t x_bs, int x_cs, int64_t M, float eps,
                                                       float mean, float stdv, const int32_t* __restrict__ len) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  const int b = blockIdx.z;
  if (m >= M) return;
  float* p = x + (int64_t)b * x_bs + (int64_t)c * x_cs + m;
  *p = (!len || m < len[b]) ? (logf(eps + *p) - mean) / stdv : 0.f;
}

// Depthwise Conv2d(C, C, 3, stride 2, padding 1, groups = C) -- LearnedDownSample('half'), models.py:27-42:
// y[b][ho][c][wo] = bias[c] + sum_{dh,dw} w[c][dh][dw] * x[b][2ho + dh - 1][c][2wo + dw - 1], zero outside the map.
// Rows of width W_b = w_len[b] clamped to 1 .. W (W without w_len): zero padding at the row's own right end, outputs
// [0, (W_b + 1) / 2), nothing stored past them.
__global__ __launch_bounds__(256) void dwconv3x3s2_kernel(const float* __restrict__ x, int64_t x_bs, int64_t x_hs,
                                                          int x_cs, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int H, int Wmax, int Ho,
                                                          const int32_t* __restrict__ w_len, float* __restrict__ y,
                                                          int64_t y_bs, int64_t y_hs, int y_cs) {
  const int b = blockIdx.z / Ho, ho = blockIdx.z % Ho;
  const int W = w_len ? min(max(w_len[b], 1), Wmax) : Wmax;
  const int Wo = (W + 1) / 2;
  if ((int)blockIdx.x * 256 >= Wo) return;
  const int wo = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (wo >= Wo) return;
  const float* wc = w + c * 9;
  float acc = bias ? bias[c] : 0.f;
#pragma unroll
  for (int dh = 0; dh < 3; ++dh) {
    const int h = 2 * ho + dh - 1;
    if (h < 0 || h >= H) continue;
    const float* xr = x + (int64_t)b * x_bs + (int64_t)h * x_hs + (int64_t)c * x_cs;
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      const int ww = 2 * wo + dw - 1;
      if (ww >= 0 && ww < W) acc += wc[dh * 3 + dw] * xr[ww];
    }
  }
  y[(int64_t)b * y_bs + (int64_t)ho * y_hs + (int64_t)c * y_cs + wo] = acc;
}

// DownSample('half'), models.py:72-75: the last column is replicated when the width is odd, then F.avg_pool2d(x, 2).  Rows of
// width W_b as in dwconv3x3s2_kernel: the row's own last column is the one replicated.
__global__ __launch_bounds__(256) void avgpool2x2_kernel(const float* __restrict__ x, int64_t x_bs, int64_t x_hs, int x_cs,
                                                         int Wmax, int Ho, const int32_t* __restrict__ w_len,
                                                         float* __restrict__ y, int64_t y_bs, int64_t y_hs, int y_cs) {
  const int b = blockIdx.z / Ho, ho = blockIdx.z % Ho;
  const int W = w_len ? min(max(w_len[b], 1), Wmax) : Wmax;
  const int Wo = (W + 1) / 2;
  if ((int)blockIdx.x * 256 >= Wo) return;
  const int wo = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (wo >= Wo) return;
  const float* r0 = x + (int64_t)b * x_bs + (int64_t)(2 * ho) * x_hs + (int64_t)c * x_cs;
  const float* r1 = r0 + x_hs;
  const int w0 = 2 * wo, w1 = min(2 * wo + 1, W - 1);
  const float s = ((r0[w0] + r0[w1]) + r1[w0]) + r1[w1];
  y[(int64_t)b * y_bs + (int64_t)ho * y_hs + (int64_t)c * y_cs + wo] = s * 0.25f;
}

// Every per-row length of the ragged style plan from mel_len [B] (layout: st2.h st2_style_lengths).  One thread per entry.
__global__ __launch_bounds__(64) void style_lengths_kernel(const int32_t* __restrict__ mel_len, int B, int T_min, int T_cap,
                                                           int H, int S, int32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int b, stage, v_sub = 0;
  bool seam = false;
  if (i < (S + 2) * B) {  // per-clip tables: W_0 .. W_S, then W_S - 4
    stage = min(i / B, S);
    b = i % B;
    if (i / B == S + 1) v_sub = 4;
  } else {  // per-stacked-row tables of stage 0 .. S: B (h + 2) - 2 rows each, centre = padded row r + 1
    int j = i - (S + 2) * B;
    stage = 0;
    int h = H;
    while (stage < S && j >= B * (h + 2) - 2) {
      j -= B * (h + 2) - 2;
      ++stage;
      h >>= 1;
    }
    const int r = (j + 1) % (h + 2);
    b = min((j + 1) / (h + 2), B - 1);
    seam = r == 0 || r == h + 1;
  }
  // clamped: a caller's out-of-range count gives a wrong row, never a length past the buffers T_cap sizes
  int w = min(max(mel_len[b], T_min), T_cap);
  for (int k = 0; k < stage; ++k) w = (w + 1) / 2;
  out[i] = seam ? 0 : w - v_sub;
}

// The launches behind the plain and the `_len` entry points (len / w_len == NULL: the plain one), after their own first checks;
// `fn` names the entry point in the messages.
int stft_frames(const char* fn, const float* wave, int64_t w_bs, int B, int L, int L_min, int n_win, int hop, int shift,
                float* frames, int64_t f_bs, int f_cs, const int32_t* len, int32_t* m_len, void* stream) {
  const int M = L / hop + 1;
  dim3 grid(st2_cdiv(M, 256), n_win, B);
  hipLaunchKernelGGL(stft_frames_kernel, grid, dim3(256), 0, (hipStream_t)stream, wave, w_bs, L, L_min, n_win, hop, shift, M,
                     len, frames, f_bs, f_cs, m_len);
  ST2_CHECK_LAUNCH(fn);
  return 0;
}

int log_norm(const char* fn, float* x, int64_t x_bs, int x_cs, int B, int C, int64_t M, float eps, float mean, float stdv,
             const int32_t* len, void* stream) {
  hipLaunchKernelGGL(log_norm_kernel, dim3(st2_cdiv(M, 256), C, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, x_cs, M, eps,
                     mean, stdv, len);
  ST2_CHECK_LAUNCH(fn);
  return 0;
}

int dwconv3x3s2(const char* fn, const float* x, int64_t x_bs, int64_t x_hs, int x_cs, const float* w, const float* bias, int B,
                int C, int H, int W, float* y, int64_t y_bs, int64_t y_hs, int y_cs, const int32_t* w_len, void* stream) {
  ST2_REQUIRE(x && w && y && B > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments", fn);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  ST2_REQUIRE((int64_t)B * Ho <= 65535 && C <= 65535, "%s: grid too large", fn);
  dim3 grid(st2_cdiv(Wo, 256), C, B * Ho);
  hipLaunchKernelGGL(dwconv3x3s2_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, x_bs, x_hs, x_cs, w, bias, H, W, Ho,
                     w_len, y, y_bs, y_hs, y_cs);
  ST2_CHECK_LAUNCH(fn);
  return 0;
}

int avgpool2x2(const char* fn, const float* x, int64_t x_bs, int64_t x_hs, int x_cs, int B, int C, int H, int W, float* y,
               int64_t y_bs, int64_t y_hs, int y_cs, const int32_t* w_len, void* stream) {
  ST2_REQUIRE(x && y && B > 0 && C > 0 && H > 1 && W > 0, "%s: bad arguments", fn);
  ST2_REQUIRE(H % 2 == 0, "%s: odd height %d (the reference pads the width only, models.py:72-75)", fn, H);
  const int Ho = H / 2, Wo = (W + 1) / 2;
  ST2_REQUIRE((int64_t)B * Ho <= 65535 && C <= 65535, "%s: grid too large", fn);
  dim3 grid(st2_cdiv(Wo, 256), C, B * Ho);
  hipLaunchKernelGGL(avgpool2x2_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, x_bs, x_hs, x_cs, W, Ho, w_len, y, y_bs,
                     y_hs, y_cs);
  ST2_CHECK_LAUNCH(fn);
  return 0;
}

}  // namespace

extern "C" int st2_stft_frames(const float* wave, int64_t w_bs, int32_t B, int32_t L, int32_t n_win, int32_t hop,
                               int32_t shift, float* frames, int64_t f_bs, int32_t f_cs, void* stream) {
  ST2_REQUIRE(wave && frames && B > 0 && L > 1 && n_win > 0 && hop > 0, "st2_stft_frames: bad arguments");
  // The last frame starts at (L / hop) * hop and reads positions up to i = (L / hop) * hop + n_win - 1 - shift; a single
  // reflection maps i > L - 1 to 2 (L - 1) - i, which must not go negative (and the left one, shift - j, not past L - 1).
  ST2_REQUIRE(shift >= 0 && shift < L && (int64_t)(L / hop) * hop + n_win - 1 - shift <= 2 * (int64_t)(L - 1),
              "st2_stft_frames: reflection reaches past the signal (L=%d, n_win=%d, hop=%d, shift=%d)", L, n_win, hop, shift);
  return stft_frames("st2_stft_frames", wave, w_bs, B, L, L, n_win, hop, shift, frames, f_bs, f_cs, nullptr, nullptr, stream);
}

extern "C" int st2_stft_frames_len(const float* wave, int64_t w_bs, int32_t B, int32_t L, int32_t n_win, int32_t hop,
                                   int32_t shift, float* frames, int64_t f_bs, int32_t f_cs, const int32_t* len,
                                   int32_t L_min, int32_t* m_len, void* stream) {
  ST2_REQUIRE(wave && frames && len && B > 0 && L > 1 && n_win > 0 && hop > 0, "st2_stft_frames_len: bad arguments");
  ST2_REQUIRE(B <= 65535 && n_win <= 65535, "st2_stft_frames_len: grid too large");
  // Every admitted row length L_b in [L_min, L] must keep the single reflection inside [0, L_b): the last frame reads up to
  // (L_b / hop) * hop + n_win - 1 - shift <= L_b + n_win - 1 - shift, which must not pass 2 (L_b - 1); the first one shift - 0.
  ST2_REQUIRE(L_min >= 2 && L_min <= L && shift >= 0 && shift < L_min && (int64_t)L_min + n_win - 1 - shift <= 2 * (int64_t)(L_min - 1),
              "st2_stft_frames_len: reflection reaches past the shortest admitted row (L_min=%d, L=%d, n_win=%d, hop=%d, shift=%d)",
              L_min, L, n_win, hop, shift);
  return stft_frames("st2_stft_frames_len", wave, w_bs, B, L, L_min, n_win, hop, shift, frames, f_bs, f_cs, len, m_len, stream);
}

extern "C" int st2_power_spectrum(const float* y, int64_t y_bs, int32_t y_cs, int32_t B, int32_t K, int32_t M, float* p,
                                  int64_t p_bs, int32_t p_cs, void* stream) {
  ST2_REQUIRE(y && p && B > 0 && K > 0 && M > 0, "st2_power_spectrum: bad arguments");
  dim3 grid(st2_cdiv(M, 256), K, B);
  hipLaunchKernelGGL(power_spectrum_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, y_bs, y_cs, K, M, p, p_bs, p_cs);
  ST2_CHECK_LAUNCH("st2_power_spectrum");
  return 0;
}

extern "C" int st2_log_norm(float* x, int64_t n, float eps, float mean, float stdv, void* stream) {
  ST2_REQUIRE(x && n > 0 && stdv != 0.f, "st2_log_norm: bad arguments");
  return log_norm("st2_log_norm", x, 0, 0, 1, 1, n, eps, mean, stdv, nullptr, stream);  // flat: one row of n columns
}

extern "C" int st2_log_norm_len(float* x, int64_t x_bs, int32_t x_cs, int32_t B, int32_t C, int32_t M, float eps, float mean,
                                float stdv, const int32_t* len, void* stream) {
  ST2_REQUIRE(x && len && B > 0 && C > 0 && M > 0 && stdv != 0.f, "st2_log_norm_len: bad arguments");
  ST2_REQUIRE(B <= 65535 && C <= 65535, "st2_log_norm_len: grid too large");
  return log_norm("st2_log_norm_len", x, x_bs, x_cs, B, C, M, eps, mean, stdv, len, stream);
}

extern "C" int st2_dwconv3x3s2(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, const float* w,
                               const float* bias, int32_t B, int32_t C, int32_t H, int32_t W, float* y, int64_t y_bs,
                               int64_t y_hs, int32_t y_cs, void* stream) {
  return dwconv3x3s2("st2_dwconv3x3s2", x, x_bs, x_hs, x_cs, w, bias, B, C, H, W, y, y_bs, y_hs, y_cs, nullptr, stream);
}

extern "C" int st2_dwconv3x3s2_len(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, const float* w,
                                   const float* bias, int32_t B, int32_t C, int32_t H, int32_t W, float* y, int64_t y_bs,
                                   int64_t y_hs, int32_t y_cs, const int32_t* w_len, void* stream) {
  ST2_REQUIRE(w_len, "st2_dwconv3x3s2_len: bad arguments");
  return dwconv3x3s2("st2_dwconv3x3s2_len", x, x_bs, x_hs, x_cs, w, bias, B, C, H, W, y, y_bs, y_hs, y_cs, w_len, stream);
}

extern "C" int st2_avgpool2x2(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, int32_t B, int32_t C, int32_t H,
                              int32_t W, float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs, void* stream) {
  return avgpool2x2("st2_avgpool2x2", x, x_bs, x_hs, x_cs, B, C, H, W, y, y_bs, y_hs, y_cs, nullptr, stream);
}

extern "C" int st2_avgpool2x2_len(const float* x, int64_t x_bs, int64_t x_hs, int32_t x_cs, int32_t B, int32_t C, int32_t H,
                                  int32_t W, float* y, int64_t y_bs, int64_t y_hs, int32_t y_cs, const int32_t* w_len,
                                  void* stream) {
  ST2_REQUIRE(w_len, "st2_avgpool2x2_len: bad arguments");
  return avgpool2x2("st2_avgpool2x2_len", x, x_bs, x_hs, x_cs, B, C, H, W, y, y_bs, y_hs, y_cs, w_len, stream);
}

extern "C" int64_t st2_style_lengths_count(int32_t B, int32_t H, int32_t stages) {
  if (B <= 0 || H <= 0 || stages < 0 || stages > 8 || (H >> stages) < 1) return -1;
  int64_t n = (int64_t)(stages + 2) * B;
  for (int i = 0; i <= stages; ++i) n += (int64_t)B * ((H >> i) + 2) - 2;
  return n;
}

extern "C" int st2_style_lengths(const int32_t* mel_len, int32_t B, int32_t T_min, int32_t T_cap, int32_t H, int32_t stages,
                                 int32_t* out, void* stream) {
  const int64_t n = st2_style_lengths_count(B, H, stages);
  ST2_REQUIRE(mel_len && out && n > 0 && n < ((int64_t)1 << 30) && T_min >= 1 && T_cap >= T_min,
              "st2_style_lengths: bad arguments");
  ST2_REQUIRE(((T_min - 1) >> stages) + 1 > 4, "st2_style_lengths: T_min=%d leaves no column for the 5-wide valid conv after %d "
              "halvings", T_min, stages);
  hipLaunchKernelGGL(style_lengths_kernel, dim3(st2_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, mel_len, B, T_min, T_cap, H,
                     stages, out, (int)n);
  ST2_CHECK_LAUNCH("st2_style_lengths");
  return 0;
}
