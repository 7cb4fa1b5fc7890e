// Intonation (st2.h st2_pitch_shape, added under ABI 23): a request's pitch RANGE -- how far the voice
// moves around its own mean, per row and per token -- and pitch CONTOUR -- a glide over the sentence in semitones -- applied to
// the prosody predictor's F0 curve in front of the flat scales of st2_prosody_controls[_tok].  Both act on log2 F0 around the
// row's own voiced mean, which is a reduction over the ragged row: one workgroup per row measures, then applies.
#include "st2_common.h"
#include "st2_tokens.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_POINTS = 8;  // the most contour points of a row

// The voiced rule of the harmonic source (st2_source.hip: f0 > voiced_threshold), with a NaN or an Inf unvoiced
__device__ __forceinline__ bool voiced(float v, float voiced_hz) { return fabsf(v) <= 3.402823466e+38f && v > voiced_hz; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// One workgroup per row.  Phase 1: every thread walks the row's valid columns with a stride of the workgroup and sums log2 of
// the voiced ones in fp64; lanes by shuffles, the four waves through LDS in wave order.  Meanwhile wave 0 has rebuilt the token
// boundaries and one thread has cleaned the row's contour points into LDS: one barrier publishes all three.  Phase 2: one frame
// (two columns) per thread and iteration, its token and its contour value found once.  Only a voiced column that changes is
// written; nothing at or past the row's end is read or written.  APPLY == false: the launch only measures (st2.h).
template <bool APPLY>
__global__ __launch_bounds__(PS_THREADS) void pitch_shape_kernel(float* __restrict__ f0, int64_t bs, int T, const int32_t* __restrict__ frames,
                                                                 const float* __restrict__ range, const float* __restrict__ tok_range,
                                                                 const long long* __restrict__ dur, int N, int shift,
                                                                 const float* __restrict__ contour, int K, float voiced_hz, float lo_hz,
                                                                 float hi_hz, float* __restrict__ pitch) {
  __shared__ int cum[512];
  __shared__ double w_sum[PS_WAVES];
  __shared__ int w_cnt[PS_WAVES];
  __shared__ float w_min[PS_WAVES], w_max[PS_WAVES];
  __shared__ float cp[PS_POINTS], cv[PS_POINTS];
  __shared__ int c_used;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int T_b = frames ? min(max(frames[b], 0), T) : T;
  const float nan = __int_as_float(0x7fc00000);
  if (T_b == 0) {  // the whole workgroup: no barrier has been reached
    if (pitch && tid == 0) {
      float* __restrict__ pr = pitch + (int64_t)b * 4;
      pr[0] = nan, pr[1] = 0.0f, pr[2] = nan, pr[3] = nan;
    }
    return;
  }
  const int len = 2 * T_b;
  float* __restrict__ fr = f0 + (int64_t)b * bs;

  double s = 0.0;
  int cnt = 0;
  for (int l = tid; l < len; l += PS_THREADS) {
    const float v = fr[l];
    if (voiced(v, voiced_hz)) {
      s += log2((double)v);
      ++cnt;
    }
  }
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  if (lane == 0) w_sum[wave] = s, w_cnt[wave] = cnt;
  if constexpr (APPLY) {
    if (tok_range && tid < 64) scan_durations(dur + (int64_t)b * N, N, N, T, cum);
    if (tid == 0) {  // the used points: NaN ones dropped, positions clamped to [0, 1] and made ascending, offsets to [-24, 24]
      int used = 0;
      float run = 0.0f;
      for (int k = 0; k < K; ++k) {
        const float p = contour[((int64_t)b * K + k) * 2], v = contour[((int64_t)b * K + k) * 2 + 1];
        if (p != p || v != v) continue;
        run = fmaxf(fminf(fmaxf(p, 0.0f), 1.0f), run);
        cp[used] = run;
        cv[used] = fminf(fmaxf(v, -24.0f), 24.0f);
        ++used;
      }
      c_used = used;
    }
  }
  __syncthreads();
  double sum = w_sum[0];
  int n_v = w_cnt[0];
#pragma unroll
  for (int w = 1; w < PS_WAVES; ++w) sum += w_sum[w], n_v += w_cnt[w];
  if (n_v == 0) {  // uniform: the row is left alone
    if (pitch && tid == 0) {
      float* __restrict__ pr = pitch + (int64_t)b * 4;
      pr[0] = nan, pr[1] = 0.0f, pr[2] = nan, pr[3] = nan;
    }
    return;
  }
  const double m = sum / (double)n_v;

  float r_b = 1.0f;
  int used = 0;
  if constexpr (APPLY) {
    if (range) {
      const float v = range[b];
      r_b = v != v ? 1.0f : fminf(fmaxf(v, 0.0f), 4.0f);
    }
    used = c_used;
  }
  const float* __restrict__ tr = APPLY && tok_range ? tok_range + (int64_t)b * N : nullptr;
  float mn = __int_as_float(0x7f800000), mx = __int_as_float(0xff800000);
  for (int t = tid; t < T_b; t += PS_THREADS) {
    const int l = 2 * t;
    const float x0 = fr[l], x1 = fr[l + 1];
    const bool v0 = voiced(x0, voiced_hz), v1 = voiced(x1, voiced_hz);
    if (!v0 && !v1) continue;
    float y0 = x0, y1 = x1;
    if constexpr (APPLY) {
      float r = r_b;
      if (tr) {
        const float v = tr[token_of_frame(cum, N, t, shift)];
        const float q = v != v ? 1.0f : fminf(fmaxf(v, 0.0f), 4.0f);
        r = fminf(r_b * q, 4.0f);
      }
      double c = 0.0;
      if (used > 0) {
        const double x = ((double)t + 0.5) / (double)T_b;
        int j = 0;
        while (j < used && (double)cp[j] <= x) ++j;
        if (j == 0) c = (double)cv[0];
        else if (j == used) c = (double)cv[used - 1];
        else {
          const double pa = (double)cp[j - 1], va = (double)cv[j - 1];
          c = va + ((double)cv[j] - va) * ((x - pa) / ((double)cp[j] - pa));
        }
      }
      if (!(r == 1.0f && c == 0.0)) {
        const double semis = c / 12.0;
        if (v0) {
          const double y = (m + (double)r * (log2((double)x0) - m)) + semis;
          y0 = (float)fmin(fmax(exp2(y), (double)lo_hz), (double)hi_hz);
          fr[l] = y0;
        }
        if (v1) {
          const double y = (m + (double)r * (log2((double)x1) - m)) + semis;
          y1 = (float)fmin(fmax(exp2(y), (double)lo_hz), (double)hi_hz);
          fr[l + 1] = y1;
        }
      }
    }
    if (v0) mn = fminf(mn, y0), mx = fmaxf(mx, y0);
    if (v1) mn = fminf(mn, y1), mx = fmaxf(mx, y1);
  }
  if (!pitch) return;  // uniform
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (lane == 0) w_min[wave] = mn, w_max[wave] = mx;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PS_WAVES; ++w) mn = fminf(mn, w_min[w]), mx = fmaxf(mx, w_max[w]);
    float* __restrict__ pr = pitch + (int64_t)b * 4;
    pr[0] = (float)exp2(m), pr[1] = (float)n_v, pr[2] = mn, pr[3] = mx;
  }
}

}  // namespace

extern "C" int st2_pitch_shape(float* f0, int64_t bs, int32_t B, int32_t L, const int32_t* frames, const float* range,
                               const float* tok_range, const int64_t* dur, int32_t N, int32_t shift, const float* contour, int32_t K,
                               float voiced_hz, float lo_hz, float hi_hz, float* pitch, void* stream) {
  ST2_REQUIRE(f0, "st2_pitch_shape: f0 is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535, "st2_pitch_shape: B=%d must lie in 1..65535", B);
  ST2_REQUIRE(L > 0 && L % 2 == 0, "st2_pitch_shape: L=%d must be positive and even (two columns per frame)", L);
  ST2_REQUIRE(B == 1 || bs >= L, "st2_pitch_shape: row stride bs=%lld is less than L=%d", (long long)bs, L);
  ST2_REQUIRE(!tok_range || dur, "st2_pitch_shape: tok_range needs dur");
  ST2_REQUIRE(!tok_range || (N > 0 && N <= 512), "st2_pitch_shape: N=%d tokens must lie in 1..512", N);
  ST2_REQUIRE(K >= 0 && K <= PS_POINTS, "st2_pitch_shape: K=%d contour points must lie in 0..%d", K, PS_POINTS);
  ST2_REQUIRE(K == 0 || contour, "st2_pitch_shape: contour is NULL with K=%d", K);
  ST2_REQUIRE(voiced_hz > 0.0f && voiced_hz <= 1000.0f, "st2_pitch_shape: voiced_hz=%g must lie in (0, 1000]", (double)voiced_hz);
  ST2_REQUIRE(voiced_hz < lo_hz && lo_hz < hi_hz && hi_hz <= 20000.0f,
              "st2_pitch_shape: need voiced_hz=%g < lo_hz=%g < hi_hz=%g <= 20000", (double)voiced_hz, (double)lo_hz, (double)hi_hz);
  const bool apply = range || tok_range || (contour && K > 0);
  if (!apply && !pitch) return 0;  // nothing to apply, nothing to report: no launch
  auto kernel = apply ? pitch_shape_kernel<true> : pitch_shape_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(PS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), f0, bs, L / 2, frames, range,
                     tok_range, reinterpret_cast<const long long*>(dur), N, shift ? 1 : 0, contour && K > 0 ? contour : nullptr,
                     contour ? K : 0, voiced_hz, lo_hz, hi_hz, pitch);
  ST2_CHECK_LAUNCH("st2_pitch_shape");
  return 0;
}
