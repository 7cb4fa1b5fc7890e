// The silence-trim rule of st2_clip_ingest (st2_ingest.hip, the way in) and st2_wave_edges (st2_edges.hip, the way out), stated
// once (st2.h rule 3 of st2_clip_ingest; DESIGN.md sections 16 and 28): librosa's effects.trim(y, top_db, ref=max,
// frame_length=2048, hop_length=512) with centred, zero-padded frames, from the sums of squares of the row's 512-sample blocks.
//   block sum   wave w of the workgroup sums block w of a tile staged in LDS: lane l the samples l, l + 64, ... ascending by
//               fmaf from 0, then the 64 partial sums by a butterfly -- one fixed order, no atomics;
//   energy      e_f = max(((s[f - 2] + s[f - 1]) + (s[f] + s[f + 1])) / 2048, 1e-10), s = 0 outside the row's blocks,
//               f = 0 .. m div 512 for a row of m samples;
//   non-silent  e_f > max_f e_f * threshold, threshold = (float) 10^(-top_db / 10); the maximal frame whatever the rounding;
//   bounds      start = 512 first, end = min(m, 512 (last + 1)).
// Both kernels run these functions over their own rows, so a row's bounds are the same bits on either path.
#pragma once
#include "st2_common.h"

constexpr int TRIM_HOP = 512;       // the trim's hop: a frame of 2048 samples is four block sums
constexpr int TRIM_THREADS = 256;   // lanes of a workgroup of either user: four waves

// (float) 10^(-top_db / 10), in double with one rounding: on the host for the way in, on the device for the way out
__host__ __device__ __forceinline__ float trim_threshold(float top_db) { return (float)pow(10.0, -(double)top_db / 10.0); }

// The block sums of a tile of `tile` samples (a multiple of TRIM_HOP) staged at `ys` in LDS, zeros where the row has ended,
// into sums[0 .. tile / TRIM_HOP).  Called by all TRIM_THREADS lanes behind the barrier that completes `ys`.
__device__ __forceinline__ void trim_block_sums(const float* __restrict__ ys, int tile, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  for (int blk = threadIdx.x >> 6; blk * TRIM_HOP < tile; blk += TRIM_THREADS / 64) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < TRIM_HOP / 64; ++i) {
      const float v = ys[blk * TRIM_HOP + i * 64 + lane];
      s = fmaf(v, v, s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) sums[blk] = s;
  }
}

// Reductions of the bounds search over its 256 lanes: a butterfly inside each wave, the four wave results through LDS.
template <class T, class F>
__device__ __forceinline__ T trim_block_reduce(T v, T* __restrict__ slot, F op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  __syncthreads();  // the slots of the reduction before this one have been read
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(slot[0], slot[1]), op(slot[2], slot[3]));
}

// The bounds of a row of m samples from its block sums `s` (ceil(m / 512) of them): frame energies, their maximum, the first
// and the last non-silent frame.  Called by all TRIM_THREADS lanes of a workgroup (it holds barriers); every lane gets the result.
__device__ __forceinline__ void trim_bounds(const float* __restrict__ s, int m, float threshold, float* __restrict__ slot_f,
                                            int* __restrict__ slot_i, int* __restrict__ start, int* __restrict__ end) {
  const int nblk = (m + TRIM_HOP - 1) / TRIM_HOP, nf = m / TRIM_HOP + 1;
  auto block = [&](int i) { return i >= 0 && i < nblk ? s[i] : 0.0f; };
  auto energy = [&](int f) {
    return fmaxf(((block(f - 2) + block(f - 1)) + (block(f) + block(f + 1))) * (1.0f / 2048.0f), 1e-10f);
  };
  float top = 0.0f;
  for (int f = threadIdx.x; f < nf; f += TRIM_THREADS) top = fmaxf(top, energy(f));
  top = trim_block_reduce(top, slot_f, [](float a, float c) { return fmaxf(a, c); });
  const float lim = top * threshold;
  int first = 0x7fffffff, last = -1;
  for (int f = threadIdx.x; f < nf; f += TRIM_THREADS) {
    const float e = energy(f);
    if (e > lim || e >= top) {  // the maximal frame is non-silent whatever the rounding of `lim`
      first = min(first, f);
      last = max(last, f);
    }
  }
  first = trim_block_reduce(first, slot_i, [](int a, int c) { return min(a, c); });
  last = trim_block_reduce(last, slot_i, [](int a, int c) { return max(a, c); });
  *start = TRIM_HOP * first;
  *end = (int)min((long long)m, (long long)TRIM_HOP * (last + 1));
}
