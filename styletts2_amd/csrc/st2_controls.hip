// Per-request controls (st2.h, added under ABI 23): what a request brings as a SETTING -- style mixing
// weights, pitch scale, energy shift -- read per row from device memory, like the lengths are.  Two kernels: the style mixing
// of the front as ONE launch (with the long-form carry-over as a row scan inside it) and the per-row pitch / energy controls
// over the prosody predictor's F0 / N curves.  (The third control kernel, the duration head with a per-row rate, is a twin
// instantiation of duration_head_kernel in st2_glue.hip.)
#include "st2_common.h"

namespace {

struct Weight {
  float w, cw;  // the weight and its complement (float)(1.0 - (double)w): the scalar path's arithmetic (front_plan)
};

// Row b's weight: clamped to [0, 1] where it is read; NaN or no row = the call's scalar pair.
__device__ __forceinline__ Weight row_weight(const float* __restrict__ row, int b, Weight scalar) {
  if (!row) return scalar;
  const float r = row[b];
  if (r != r) return scalar;
  const float w = fminf(fmaxf(r, 0.0f), 1.0f);
  return {w, (float)(1.0 - (double)w)};
}

// v = a x; v += b y: axpbypcz_kernel's two roundings (the library builds with -ffp-contract=off: no FMA)
__device__ __forceinline__ float mix2(float a, float x, float b, float y) {
  float v = a * x;
  v += b * y;
  return v;
}

// One channel per thread.  carry == 0: workgroup (chunk, b) mixes row b.  carry != 0: workgroup (chunk, 0) walks the rows
// 0 .. B-1 -- row k's previous style is row k-1's MIXED style, which is this thread's own last result: no exchange between lanes.
__global__ __launch_bounds__(256) void style_mix_rows_kernel(const float* __restrict__ sp, const float* __restrict__ s_prev,
                                                             const float* __restrict__ ref_s, const float* __restrict__ t_row,
                                                             const float* __restrict__ a_row, const float* __restrict__ b_row,
                                                             Weight t0, Weight a0, Weight b0, int B, int sty, int carry,
                                                             float* __restrict__ ref, float* __restrict__ s,
                                                             float* __restrict__ s_pred_out) {
  const int C2 = 2 * sty;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C2) return;
  const int b_lo = carry ? 0 : blockIdx.y;
  const int b_hi = carry ? B : b_lo + 1;
  float last = 0.f;
  for (int b = b_lo; b < b_hi; ++b) {
    const int64_t i = (int64_t)b * C2 + c;
    float cur = sp[i];
    const bool has_prev = carry ? (b > 0 || s_prev != nullptr) : s_prev != nullptr;
    if (has_prev) {
      const float prev = carry ? (b > 0 ? last : s_prev[c]) : s_prev[i];
      const Weight t = row_weight(t_row, b, t0);
      cur = mix2(t.w, prev, t.cw, cur);
    }
    if (ref_s) {
      const Weight m = c < sty ? row_weight(a_row, b, a0) : row_weight(b_row, b, b0);
      cur = mix2(m.w, cur, m.cw, ref_s[i]);
    }
    if (c < sty) ref[(int64_t)b * sty + c] = cur; else s[(int64_t)b * sty + (c - sty)] = cur;
    if (s_pred_out) s_pred_out[i] = cur;
    last = cur;
  }
}

constexpr int CTL_THREADS = 256;
constexpr int CTL_ITERS = 4;

// Workgroup (chunk, b) covers CTL_THREADS * CTL_ITERS columns of row b of BOTH curves; one whose chunk lies at or past the
// row's end (2 T_b) leaves at once.  One operation per element: a multiply for F0, an add for N (x itself where the shift is
// 0, so that -0.0 survives); nothing at or past the row's end is read or written.
__global__ __launch_bounds__(CTL_THREADS) void prosody_controls_kernel(float* __restrict__ f0, float* __restrict__ n, int64_t bs,
                                                                       int L, const float* __restrict__ f0_scale,
                                                                       const float* __restrict__ n_shift,
                                                                       const int32_t* __restrict__ frames) {
  const int b = blockIdx.y;
  const int len = frames ? (int)min(2LL * max(frames[b], 0), (long long)L) : L;
  const int l0 = blockIdx.x * (CTL_THREADS * CTL_ITERS);
  if (l0 >= len) return;
  float sc = 1.0f, sh = 0.0f;
  if (f0_scale) {
    const float v = f0_scale[b];
    sc = v != v ? 1.0f : fminf(fmaxf(v, 0.5f), 2.0f);
  }
  if (n_shift) {
    const float v = n_shift[b];
    sh = v != v ? 0.0f : fminf(fmaxf(v, -2.0f), 2.0f);
  }
  float* __restrict__ fr = f0 + (int64_t)b * bs;
  float* __restrict__ nr = n + (int64_t)b * bs;
#pragma unroll
  for (int it = 0; it < CTL_ITERS; ++it) {
    const int l = l0 + it * CTL_THREADS + threadIdx.x;
    if (l >= len) break;
    if (f0_scale) fr[l] = fr[l] * sc;
    if (n_shift) {
      const float x = nr[l];
      nr[l] = sh == 0.0f ? x : x + sh;
    }
  }
}

}  // namespace

extern "C" int st2_sizeof_controls(void) { return (int)sizeof(st2_controls); }

extern "C" int st2_style_mix_rows(const float* s_pred, const float* s_prev, const float* ref_s, const float* t,
                                  const float* alpha, const float* beta, double t0, double alpha0, double beta0, int32_t B,
                                  int32_t style_dim, int32_t carry, float* ref, float* s, float* s_pred_out, void* stream) {
  ST2_REQUIRE(s_pred && ref && s, "st2_style_mix_rows: s_pred / ref / s is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535 && style_dim > 0 && style_dim <= (1 << 20),
              "st2_style_mix_rows: bad geometry (B=%d, style_dim=%d)", B, style_dim);
  const auto in01 = [](double w) { return w >= 0.0 && w <= 1.0; };  // false for NaN
  ST2_REQUIRE(in01(t0) && in01(alpha0) && in01(beta0), "st2_style_mix_rows: scalar weights t=%g / alpha=%g / beta=%g must lie in [0, 1]",
              t0, alpha0, beta0);
  const Weight wt = {(float)t0, (float)(1.0 - t0)}, wa = {(float)alpha0, (float)(1.0 - alpha0)},
               wb = {(float)beta0, (float)(1.0 - beta0)};
  hipLaunchKernelGGL(style_mix_rows_kernel, dim3(st2_cdiv(2 * (int64_t)style_dim, 256), carry ? 1 : B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), s_pred, s_prev, ref_s, t, alpha, beta, wt, wa, wb, B, style_dim,
                     carry ? 1 : 0, ref, s, s_pred_out);
  ST2_CHECK_LAUNCH("st2_style_mix_rows");
  return 0;
}

extern "C" int st2_prosody_controls(float* f0, float* n, int64_t bs, int32_t B, int32_t L, const float* f0_scale,
                                    const float* n_shift, const int32_t* frames, void* stream) {
  ST2_REQUIRE(f0 && n, "st2_prosody_controls: f0 / n is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535 && L > 0 && (B == 1 || bs >= L), "st2_prosody_controls: bad geometry (B=%d, L=%d, bs=%lld)", B, L,
              (long long)bs);
  if (!f0_scale && !n_shift) return 0;  // nothing to apply: no launch
  hipLaunchKernelGGL(prosody_controls_kernel, dim3(st2_cdiv(L, CTL_THREADS * CTL_ITERS), B), dim3(CTL_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), f0, n, bs, L, f0_scale, n_shift, frames);
  ST2_CHECK_LAUNCH("st2_prosody_controls");
  return 0;
}
