// The rational polyphase rule of st2_wave_resample_pack (st2_resample.hip, the way out) and st2_clip_ingest (st2_ingest.hip,
// the way in), stated once (DESIGN.md sections 15 and 16).  Output sample j of a row of n input samples is
//   y[j] = sum_k taps[p][k] x[c - h + k],  c = floor(j D / U), p = j D - c U, h = (K - 1) / 2,
// in fp32, fmaf, from 0, k ascending, with x = 0 in front of the row and at / past n.  A workgroup makes a tile of consecutive
// output samples from a phase table and an input span it stages in LDS; every sample is that one chain wherever the tile
// boundaries fall and wherever the row lies in the batch, so the result does not depend on either, bit for bit.
#pragma once
#include "st2_pcm.h"

constexpr int PP_THREADS = 256;  // lanes of a workgroup of either kernel

__host__ __device__ constexpr int pp_round4(int v) { return (v + 3) & ~3; }
// Upper bound of the input span (in floats, from its 4-sample-aligned start) of a tile of `samples` output samples
__host__ __device__ constexpr long long pp_span_cap(long long samples, int U, int D, int K) { return samples * D / U + K + 8; }

// The input span of the output samples [j0, j0 + len) of a row
struct pp_tile {
  unsigned p0;     // the phase of sample j0
  long long a0;    // the span's first staged input sample: c(j0) - h floored to a multiple of 4
  int n4;          // 4-sample vectors of the span, up to the tile's last input sample c(j0 + len - 1) - h + K - 1
  int x0;          // where input sample c(j0) - h lies in the staged span
};

__device__ __forceinline__ pp_tile pp_tile_of(long long j0, int len, int U, int D, int K) {
  const int h = (K - 1) / 2;
  const long long c0 = j0 * D / U;
  const unsigned p0 = (unsigned)(j0 * D - c0 * U);
  const long long i_lo = c0 - h;
  const long long i_hi = c0 + ((long long)p0 + (long long)(len - 1) * D) / U - h + K - 1;  // the last input sample of the tile
  const long long a0 = i_lo & ~3LL;  // floor to a multiple of 4, also for a negative start
  return {p0, a0, (int)((i_hi - a0) / 4 + 1), (int)(i_lo - a0)};
}

// The phase table [nt = U K] to LDS with 16-byte loads
__device__ __forceinline__ void pp_stage_table(float* __restrict__ tab, const float* __restrict__ taps, int nt) {
  for (int q = threadIdx.x; 4 * q + 4 <= nt; q += PP_THREADS) *reinterpret_cast<float4*>(tab + 4 * q) = load_f32x4(taps + 4 * q);
  if ((int)threadIdx.x < (nt & 3)) tab[(nt & ~3) + threadIdx.x] = taps[(nt & ~3) + threadIdx.x];
}

// The tile's input span of a row of n samples in format FMT, decoded, to LDS; a sample in front of the row or at / past n is
// a SELECTED zero -- nothing of `row` at or past n is read.  `gain` (st2_pcm.h): the row's gain on every loaded sample; the
// default is none.  CLEAN (the true-peak launch of st2_level.hip; off for the two resamplers): a non-finite sample is staged
// as 0.
template <int FMT, bool CLEAN = false>
__device__ __forceinline__ void pp_stage_span(float* __restrict__ xs, const typename pcm_fmt<FMT>::type* __restrict__ row,
                                              long long n, const pp_tile& g, const row_gain gain = row_gain{false, 1.0f}) {
  for (int q = threadIdx.x; q < g.n4; q += PP_THREADS) {
    const long long i = g.a0 + 4LL * q;
    float4 x;
    if (i >= 0 && i + 4 <= n) {
      x = gain(pcm_decode4<FMT>(row + i));
    } else {  // an edge of the row: every sample on its own, loaded only where it is valid
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = 0.0f;
        if (i + r >= 0 && i + r < n) e[r] = gain(pcm_decode<FMT>(row[i + r]));
      }
      x = make_float4(e[0], e[1], e[2], e[3]);
    }
    if constexpr (CLEAN) x = make_float4(finite_or_zero(x.x), finite_or_zero(x.y), finite_or_zero(x.z), finite_or_zero(x.w));
    *reinterpret_cast<float4*>(xs + 4 * q) = x;
  }
}

// Sample j0 + jj of the tile from the staged table and span
__device__ __forceinline__ float pp_chain(const float* __restrict__ tab, const float* __restrict__ xs, const pp_tile& g, int jj,
                                          int U, int D, int K) {
  // < 2^23: D <= 1024 and jj <= 4111, the resampling pack's 4096-byte tile with its head (the ingest's jj stays below 1024)
  const unsigned t = g.p0 + (unsigned)jj * (unsigned)D;
  const unsigned c = t / (unsigned)U;
  const float* __restrict__ tp = tab + (t - c * (unsigned)U) * K;
  const float* __restrict__ xp = xs + g.x0 + c;
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) acc = fmaf(tp[k], xp[k], acc);
  return acc;
}

// The operands both entry points take, checked under the entry point's `name`: 0, or 1 with the error set
inline int pp_check(const char* name, int up, int down, int taps_per_phase, int fmt) {
  ST2_REQUIRE(up >= 1 && up <= 1024 && down >= 1 && down <= 1024, "%s: bad ratio %d / %d (each 1..1024)", name, up, down);
  ST2_REQUIRE(taps_per_phase >= 1 && taps_per_phase <= 512, "%s: taps_per_phase=%d is outside 1..512", name, taps_per_phase);
  ST2_REQUIRE(fmt == ST2_PCM_F32 || fmt == ST2_PCM_S16 || fmt == ST2_PCM_ULAW || fmt == ST2_PCM_ALAW, "%s: unknown format %d",
              name, fmt);
  return 0;
}
