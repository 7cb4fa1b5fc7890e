// st2_wave_level (st2.h, added under ABI 23): per-row integrated loudness (ITU-R BS.1770-4: K-weighting,
// 400 ms blocks at 75 % overlap, absolute and relative gate) and sample peak of a ragged batch of waveforms, measured on the
// device from every row's valid samples at the model rate, and from them the per-row linear gain that brings the row to a
// target loudness under a peak ceiling.  The gain is applied by st2_wave_pack_level (st2_passage.hip) inside the packing moves.
// Two launches, no allocation, no synchronisation: legal under stream capture.
//
// Launch 1, one workgroup per (run of R hops, row).  A hop is h = sample_rate / 10 samples.  The workgroup stages its input --
// the R hops and W samples in front of them -- in LDS with 16-byte loads, a non-finite sample as 0.  Each of the 256 / R lanes
// of a hop runs the two biquads in fp64 (direct form I, the operation order of tests/_level_ref.py) over its own sub-span of
// ceil(h R / 256) samples: it starts from zero state W samples earlier, or at the row's first sample if that is nearer -- then
// its samples are the contract's, bit for bit.  The lanes' sums of y^2 and their peaks are added up per hop in lane order by
// one lane: no atomics, and a hop's numbers depend on the row's samples alone, not on where the row lies in the batch.
//
// W = 4 ceil(0.032 sample_rate) samples, 128 ms (3072 at 24 kHz).  The cascade's impulse response h_K decays with the high
// pass's pole radius, 0.990072 at 24 kHz: 0.990072^3072 = 4.9e-14, and T(W) = sum_{m >= W} |h_K[m]| = 1.2e-12 (the same at
// every rate: W grows with it).  A chain that starts W samples late is off by at most T(W) peak_b on every y, so a block of
// mean square z is off by at most (2 T(W) peak_b / sqrt(z) + (T(W) peak_b)^2 / z) relative.  For a block above the absolute
// gate (sqrt(z) >= 3.4e-4) of a row that peaks at full scale or below that is 7.0e-9, against the 1e-6 the design allows; it
// stays below 1e-6 up to a crest of peak_b / sqrt(z) = 4e5 (112 dB).
//
// Launch 2, one wave per row: the blocks from the hop energies, both gates (in the linear domain: l_k > -70 is z_k > 10^-6.9309,
// the relative gate z_k > mean / 10), loudness and gain in fp64 with one rounding to fp32, lane-strided sums folded by a fixed
// shuffle tree.
//
// st2_wave_level_ex adds, with a table, the true-peak launch between the two (below, at its kernel) and, with start flags, the
// gate kernel's group loop: the rows of a passage as one programme with one gain.  With neither it is st2_wave_level.
#include <cmath>

#include "st2_polyphase.h"

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_LDS_FLOATS = 15360;  // 60 KiB of staged input beside the 3 KiB of lane partials
constexpr double LV_OFFSET = -0.691, LV_ABS_GATE = -70.0;

// Stage 1 (high shelf): b10 b11 b12 / 1 a11 a12; stage 2 (high pass): 1 -2 1 / 1 a21 a22
struct kw_coef {
  double b10, b11, b12, a11, a12, a21, a22;
};

// The K-weighting of one sample from the six values of state: v -> shelf -> high pass
struct kw_state {
  double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0, w1 = 0.0, w2 = 0.0;
  __device__ __forceinline__ double step(const kw_coef& c, double v) {
    const double y = c.b10 * v + c.b11 * x1 + c.b12 * x2 - c.a11 * y1 - c.a12 * y2;
    const double w = 1.0 * y + -2.0 * y1 + 1.0 * y2 - c.a21 * w1 - c.a22 * w2;
    x2 = x1; x1 = v; y2 = y1; y1 = y; w2 = w1; w1 = w;
    return w;
  }
};

__global__ __launch_bounds__(LV_THREADS) void level_hops_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                int h, int W, int R, kw_coef c, int nhop_cap,
                                                                double* __restrict__ energy, float* __restrict__ peaks) {
  __shared__ __attribute__((aligned(16))) float xs[LV_LDS_FLOATS];
  __shared__ double part_e[LV_THREADS];
  __shared__ float part_p[LV_THREADS];
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * R * h;  // the run's first sample
  if (t0 >= n) return;                                  // behind the row's end: the grid is sized by the capacity
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  const long long a0 = max(0LL, t0 - W) & ~3LL;
  const long long a1 = min(n, t0 + (long long)R * h);
  const int cnt = (int)(a1 - a0);  // <= W + R h + 3, and rounded up to 4 still <= LV_LDS_FLOATS (the host's choice of R)
  for (int q = threadIdx.x; 4 * q < cnt; q += LV_THREADS) {
    const long long i = a0 + 4LL * q;
    float4 x;
    if (i + 4 <= a1) {
      x = load_f32x4(src + i);
    } else {  // the row's end: every sample on its own, loaded only where it is valid
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = i + r < a1 ? src[i + r] : 0.0f;
      x = make_float4(e[0], e[1], e[2], e[3]);
    }
    *reinterpret_cast<float4*>(xs + 4 * q) =
        make_float4(finite_or_zero(x.x), finite_or_zero(x.y), finite_or_zero(x.z), finite_or_zero(x.w));
  }
  __syncthreads();
  const int P = LV_THREADS / R, S = (h + P - 1) / P;  // lanes of a hop, samples of a lane
  const int r = threadIdx.x / P, q = threadIdx.x % P;
  const long long hop0 = t0 + (long long)r * h;
  const long long s0 = hop0 + (long long)q * S;
  const long long s1 = min(min(s0 + S, hop0 + h), n);
  double e = 0.0;
  float pk = 0.0f;
  if (s0 < s1) {
    kw_state st;
    // xs[i] = sample a0 + i of the row; a0 <= max(0, s0 - W) and s1 <= a1
    const int i0 = (int)(max(0LL, s0 - W) - a0), i1 = (int)(s0 - a0), i2 = (int)(s1 - a0);
    for (int i = i0; i < i1; ++i) st.step(c, (double)xs[i]);
    for (int i = i1; i < i2; ++i) {
      const float v = xs[i];
      const double w = st.step(c, (double)v);
      e += w * w;
      pk = fmaxf(pk, fabsf(v));
    }
  }
  part_e[threadIdx.x] = e;
  part_p[threadIdx.x] = pk;
  __syncthreads();
  if (q == 0 && hop0 < n) {
    for (int l = 1; l < P; ++l) {
      e += part_e[threadIdx.x + l];
      pk = fmaxf(pk, part_p[threadIdx.x + l]);
    }
    const long long at = (long long)b * nhop_cap + (long long)blockIdx.x * R + r;  // hop < ceil(n / h) <= nhop_cap
    energy[at] = e;
    peaks[at] = pk;
  }
}

// The true-peak launch (st2_wave_level_ex with a table), between launch 1 and the gate: one workgroup per
// (hop, row), the grid sized by the capacity.  It stages the table [U][K] and the hop's input span -- the hop and K - 1 samples
// of halo, zeros selected outside the row, a non-finite sample as 0 -- and every lane makes all the phases of TP_J input
// positions PP_THREADS apart: per tap it reads its TP_J staged samples once (consecutive lanes read consecutive words: no
// bank conflict) and PB table words at wave-uniform addresses (broadcasts) for TP_J PB accumulators.  Every output is
// st2_polyphase.h's chain -- fp32 fmaf from 0, k ascending -- and a maximum does not depend on order, so the hop's reading is
// the same wherever the row lies.  One lane folds it into the hop's slot of `peaks`, which launch 1 wrote before it in stream
// order: no atomics, and the gate reads max(sample peak, interpolated peak) where it read the sample peak.
constexpr int TP_J = 5;  // 10 positions per lane at 24 kHz (h = 2400): two full passes

template <int PB>  // phases per pass: 8 where U is a multiple of 8, else 1
__global__ __launch_bounds__(PP_THREADS) void level_true_peak_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                     const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                     int h, const float* __restrict__ taps, int U, int K,
                                                                     int nhop_cap, float* __restrict__ peaks) {
  __shared__ __attribute__((aligned(16))) float lds[LV_LDS_FLOATS];
  __shared__ float part[PP_THREADS / 64];
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * h;  // the hop's first input position
  if (t0 >= n) return;                              // behind the row's end
  const int len = (int)min((long long)h, n - t0);
  float* __restrict__ tab = lds;
  float* __restrict__ xs = lds + pp_round4(U * K);  // the host checked that the span fits behind the table
  const pp_tile g = pp_tile_of(t0 * U, len * U, U, 1, K);  // outputs [U t0, U (t0 + len)): phase 0 of position t0 first
  pp_stage_table(tab, taps, U * K);
  pp_stage_span<ST2_PCM_F32, true>(xs, wave + (int64_t)b * w_bs, n, g);
  __syncthreads();
  float m = 0.0f;
  for (int q0 = threadIdx.x; q0 < len; q0 += PP_THREADS * TP_J) {
    const float* __restrict__ xw[TP_J];  // xw[j][k] = x[c_j - (K - 1) / 2 + k]; a position past the hop's end reads q0's window
    bool valid[TP_J];
#pragma unroll
    for (int j = 0; j < TP_J; ++j) {
      valid[j] = q0 + j * PP_THREADS < len;
      xw[j] = xs + g.x0 + (valid[j] ? q0 + j * PP_THREADS : q0);
    }
    for (int p0 = 0; p0 < U; p0 += PB) {
      const float* __restrict__ tp = tab + p0 * K;
      float acc[TP_J][PB];
#pragma unroll
      for (int j = 0; j < TP_J; ++j)
#pragma unroll
        for (int p = 0; p < PB; ++p) acc[j][p] = 0.0f;
#pragma unroll 2
      for (int k = 0; k < K; ++k) {
        float t[PB];
#pragma unroll
        for (int p = 0; p < PB; ++p) t[p] = tp[p * K + k];
#pragma unroll
        for (int j = 0; j < TP_J; ++j) {
          const float x = xw[j][k];
#pragma unroll
          for (int p = 0; p < PB; ++p) acc[j][p] = fmaf(t[p], x, acc[j][p]);
        }
      }
#pragma unroll
      for (int j = 0; j < TP_J; ++j)
#pragma unroll
        for (int p = 0; p < PB; ++p)
          if (valid[j]) m = fmaxf(m, fabsf(acc[j][p]));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PP_THREADS / 64; ++w) m = fmaxf(m, part[w]);
    const long long at = (long long)b * nhop_cap + blockIdx.x;  // the slot launch 1 wrote: t0 < n
    peaks[at] = fmaxf(peaks[at], m);
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// GROUPED (st2_wave_level_ex with start flags): row b's wave measures its whole group -- the flagged row at or in front of b
// and the unflagged rows behind it -- as one programme: the blocks of the group's rows in row order, every row's by its own
// rule, one peak, one target (the first row's).  Every lane's sums run over the rows in row order and, within a row, over the
// blocks it takes in a row of its own, so a group of one row is the ungrouped kernel operation for operation, and the rows of
// a group, which all run this one sequence over the same data, agree bit for bit.
template <bool GROUPED>
__global__ __launch_bounds__(64) void level_gate_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim, int h,
                                                        int nhop_cap, const double* __restrict__ energy,
                                                        const float* __restrict__ peaks, const float* __restrict__ target,
                                                        const int32_t* __restrict__ start, double abs_thr, double ceiling,
                                                        double max_gain, float* __restrict__ level) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int r0 = b, r1 = b;
  if constexpr (GROUPED) {
    while (r0 > 0 && start[r0] == 0) --r0;  // row 0 begins a group whatever its flag
    while (r1 + 1 < (int)gridDim.x && start[r1 + 1] == 0) ++r1;
  }
  float pk = 0.0f;
  for (int r = r0; r <= r1; ++r) {
    const long long n = pack_row_samples(frames, r, T_cap, spf, trim);
    const int nh = (int)((n + h - 1) / h);  // hops that hold samples, the last one perhaps in part
    for (int j = lane; j < nh; j += 64) pk = fmaxf(pk, peaks[(long long)r * nhop_cap + j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pk = fmaxf(pk, __shfl_down(pk, off, 64));
  pk = __shfl(pk, 0, 64);
  // the blocks of rows r0 .. r1 above the absolute gate and, with `relative`, above rel_thr: this lane's share of their sum and count
  auto gate = [&](bool relative, double rel_thr, double& sum, double& count) {
    for (int r = r0; r <= r1; ++r) {
      const long long n = pack_row_samples(frames, r, T_cap, spf, trim);
      const int nh = (int)((n + h - 1) / h);
      const double* __restrict__ e = energy + (long long)r * nhop_cap;
      const bool whole = n < 4LL * h;  // the short-row rule: one block, the whole row
      const int nb = whole ? (n > 0 ? 1 : 0) : (int)(n / h) - 3;
      double z_whole = 0.0;
      if (whole && n > 0) {
        double s = 0.0;
        for (int j = lane; j < nh; j += 64) s += e[j];
        z_whole = wave_sum(s) / (double)n;
      }
      for (int k = lane; k < nb; k += 64) {
        const double z = whole ? z_whole : (e[k] + e[k + 1] + e[k + 2] + e[k + 3]) / (double)(4 * h);
        if (z > abs_thr && (!relative || z > rel_thr)) { sum += z; count += 1.0; }
      }
    }
  };
  double sum = 0.0, count = 0.0;
  gate(false, 0.0, sum, count);
  sum = wave_sum(sum);
  count = wave_sum(count);
  double L = -INFINITY, passed = 0.0;
  if (count > 0.0) {
    const double rel_thr = sum / count / 10.0;  // -10 LU under the mean of the absolutely gated blocks
    sum = 0.0; count = 0.0;
    gate(true, rel_thr, sum, count);
    sum = wave_sum(sum);
    passed = wave_sum(count);
    if (passed > 0.0) L = LV_OFFSET + 10.0 * log10(sum / passed);
  }
  if (lane == 0) {
    const float tg = target[r0];  // the group's target is its first row's
    double g = 1.0;
    if (tg == tg && passed > 0.0 && pk > 0.0f) g = fmin(fmin(pow(10.0, ((double)tg - L) / 20.0), max_gain), ceiling / (double)pk);
    float* __restrict__ o = level + 4 * b;
    o[0] = (float)L; o[1] = pk; o[2] = (float)g; o[3] = (float)passed;
  }
}

// h, W and R (hops per workgroup: the most of 8, 4, 2, 1 whose staged span fits) of a rate; false where even one hop does not fit
bool level_tiling(int sample_rate, int* h, int* W, int* R) {
  *h = sample_rate / 10;
  *W = 4 * (int)((32LL * sample_rate + 999) / 1000);
  for (int r = 8; r >= 1; r >>= 1) {
    if ((long long)*W + (long long)r * *h + 8 <= LV_LDS_FLOATS) {  // the span, floored to 4 in front and rounded up to 4 behind
      *R = r;
      return true;
    }
  }
  return false;
}

// The two biquads at a rate, in double: the analog prototypes of BS.1770-4 through the bilinear transform
kw_coef level_coefficients(double fs) {
  const double pi = 3.14159265358979323846;
  double K = std::tan(pi * 1681.974450955533 / fs), Q = 0.7071752369554196;
  const double Vh = std::pow(10.0, 3.999843853973347 / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
  double a0 = 1.0 + K / Q + K * K;
  kw_coef c;
  c.b10 = (Vh + Vb * K / Q + K * K) / a0;
  c.b11 = 2.0 * (K * K - Vh) / a0;
  c.b12 = (Vh - Vb * K / Q + K * K) / a0;
  c.a11 = 2.0 * (K * K - 1.0) / a0;
  c.a12 = (1.0 - K / Q + K * K) / a0;
  K = std::tan(pi * 38.13547087602444 / fs);
  Q = 0.5003270373238773;
  a0 = 1.0 + K / Q + K * K;
  c.a21 = 2.0 * (K * K - 1.0) / a0;
  c.a22 = (1.0 - K / Q + K * K) / a0;
  return c;
}

}  // namespace

extern "C" int64_t st2_wave_level_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t sample_rate) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0 || sample_rate <= 0 || sample_rate % 10) return 0;
  const int64_t nhop = ((int64_t)samples_per_frame * T_cap + sample_rate / 10 - 1) / (sample_rate / 10);
  return ((int64_t)B * nhop * (int64_t)(sizeof(double) + sizeof(float)) + 15) / 16 * 16;
}

// Both entries: every refusal under the entry's name `who`, then the launches.  taps == NULL: sample peaks, no third launch;
// start == NULL: every row its own group.  With both NULL these are st2_wave_level's two launches.
static int level_plan(const char* who, const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                      int32_t samples_per_frame, int32_t trim, int32_t sample_rate, const float* target, double ceiling,
                      double max_gain_db, float* level, void* workspace, int64_t workspace_bytes, void* stream, const float* taps,
                      int32_t up, int32_t taps_per_phase, const int32_t* start) {
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(target && level && workspace, "%s: target / level / workspace is NULL", who);
  ST2_REQUIRE(sample_rate > 0 && sample_rate % 10 == 0, "%s: sample_rate=%d must be a positive multiple of 10 (the hop is a tenth of it)",
              who, sample_rate);
  ST2_REQUIRE(ceiling > 0.0 && ceiling <= 1.0, "%s: ceiling=%g is outside (0, 1]", who, ceiling);
  ST2_REQUIRE(max_gain_db >= 0.0 && max_gain_db <= 60.0, "%s: max_gain_db=%g is outside [0, 60]", who, max_gain_db);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(wave) % 4 == 0 && reinterpret_cast<uintptr_t>(target) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(level) % 4 == 0,
              "%s: wave / target / level is not aligned to float", who);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: workspace is not aligned to 8 bytes", who);
  const int64_t need = st2_wave_level_workspace_bytes(B, T_cap, samples_per_frame, sample_rate);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);
  int h, W, R;
  ST2_REQUIRE(level_tiling(sample_rate, &h, &W, &R), "%s: one hop of sample_rate=%d and its lead-in do not fit the %d bytes of LDS",
              who, sample_rate, LV_LDS_FLOATS * 4);
  const int64_t nhop = (row + h - 1) / h;
  ST2_REQUIRE(nhop <= (1 << 24), "%s: a row of %lld samples is too long", who, (long long)row);
  if (taps) {
    if (pp_check(who, up, 1, taps_per_phase, ST2_PCM_F32)) return 1;
    const long long fit = (long long)pp_round4(up * taps_per_phase) + pp_span_cap((long long)h * up, up, 1, taps_per_phase);
    ST2_REQUIRE(fit <= LV_LDS_FLOATS, "%s: the table (up=%d, taps_per_phase=%d) does not fit the %d bytes of LDS beside one hop of %d samples",
                who, up, taps_per_phase, LV_LDS_FLOATS * 4, h);
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(taps) % 4 == 0, "%s: taps is not aligned to float", who);
  }
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(start) % 4 == 0, "%s: start is not aligned to int32", who);

  const kw_coef c = level_coefficients((double)sample_rate);
  double* energy = reinterpret_cast<double*>(workspace);
  float* peaks = reinterpret_cast<float*>(energy + (int64_t)B * nhop);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(level_hops_kernel, dim3(st2_cdiv(nhop, R), B), dim3(LV_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, h, W, R, c, (int)nhop, energy, peaks);
  ST2_CHECK_LAUNCH(who);
  if (taps) {  // folds the interpolated maxima into the hops' peaks, behind launch 1 in stream order
    auto tp = up % 8 == 0 ? level_true_peak_kernel<8> : level_true_peak_kernel<1>;
    hipLaunchKernelGGL(tp, dim3(nhop, B), dim3(PP_THREADS), 0, s, wave, w_bs, frames, T_cap, samples_per_frame, trim, h, taps, up,
                       taps_per_phase, (int)nhop, peaks);
    ST2_CHECK_LAUNCH(who);
  }
  auto gate = start ? level_gate_kernel<true> : level_gate_kernel<false>;
  hipLaunchKernelGGL(gate, dim3(B), dim3(64), 0, s, frames, T_cap, samples_per_frame, trim, h, (int)nhop, energy, peaks, target, start,
                     std::pow(10.0, (LV_ABS_GATE - LV_OFFSET) / 10.0), ceiling, std::pow(10.0, max_gain_db / 20.0), level);
  ST2_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int st2_wave_level(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                              int32_t samples_per_frame, int32_t trim, int32_t sample_rate, const float* target, double ceiling,
                              double max_gain_db, float* level, void* workspace, int64_t workspace_bytes, void* stream) {
  return level_plan("st2_wave_level", wave, w_bs, frames, B, T_cap, samples_per_frame, trim, sample_rate, target, ceiling, max_gain_db,
                    level, workspace, workspace_bytes, stream, nullptr, 0, 0, nullptr);
}

// st2_wave_level_ex (st2.h): st2_wave_level with a true-peak table and / or start flags; without either it IS st2_wave_level.
// The true-peak launch writes into the hops' peak slots, so the workspace is st2_wave_level's.
extern "C" int64_t st2_wave_level_ex_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t sample_rate) {
  return st2_wave_level_workspace_bytes(B, T_cap, samples_per_frame, sample_rate);
}

extern "C" int st2_wave_level_ex(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                 int32_t samples_per_frame, int32_t trim, int32_t sample_rate, const float* target, double ceiling,
                                 double max_gain_db, float* level, void* workspace, int64_t workspace_bytes, void* stream,
                                 const float* taps, int32_t up, int32_t taps_per_phase, const int32_t* start) {
  return level_plan(taps || start ? "st2_wave_level_ex" : "st2_wave_level", wave, w_bs, frames, B, T_cap, samples_per_frame, trim,
                    sample_rate, target, ceiling, max_gain_db, level, workspace, workspace_bytes, stream, taps, up, taps_per_phase, start);
}
