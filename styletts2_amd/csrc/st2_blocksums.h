// The 64-sample block sums of st2_wave_breaks' rule 2 (st2.h), stated once for the two units that launch
// them: st2_breaks.hip (the window energies of a cut) and st2_dynamics.hip (the detector of the compressor, section 30).  Both
// units are built with -fno-slp-vectorize, so that both run the same instructions.
#pragma once
#include "st2_pcm.h"

namespace {

constexpr int BR_THREADS = 256;
constexpr int BR_BLOCK = 64;    // samples of a block sum: one per lane
constexpr int BR_TILE = 2048;   // samples of a workgroup: eight blocks per wave
static_assert(BR_TILE % (4 * BR_THREADS) == 0 && BR_TILE % BR_BLOCK == 0, "whole vectors, whole blocks");

// One workgroup per (tile of BR_TILE samples, row): the tile goes to LDS with 16-byte loads, a non-finite sample and everything
// at or past n_b as 0; wave w squares block w, w + 4, ... one sample per lane and folds the 64 squares by a butterfly: one read
// of the valid samples.  `nb_row` is the stride of a row of `sums` and `nb_keep` the blocks of it that may be written: a caller
// whose rows are the capacity rounded up to the tile passes nb_row twice.
__global__ __launch_bounds__(BR_THREADS) void breaks_sums_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                 const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                 float* __restrict__ sums, int nb_row, int nb_keep) {
  __shared__ __attribute__((aligned(16))) float ys[BR_TILE];
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long j0 = (long long)blockIdx.x * BR_TILE;
  if (j0 >= n) return;  // behind the row's end: the grid is sized by the capacity
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
#pragma unroll
  for (int q = threadIdx.x; 4 * q < BR_TILE; q += BR_THREADS) {
    const long long i = j0 + 4LL * q;
    float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i + 4 <= n) {
      const float4 x = load_f32x4(src + i);
      e[0] = x.x; e[1] = x.y; e[2] = x.z; e[3] = x.w;
    } else {  // the row's end: every sample on its own, loaded only where it is valid
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i + r < n) e[r] = src[i + r];
    }
    *reinterpret_cast<float4*>(ys + 4 * q) =
        make_float4(finite_or_zero(e[0]), finite_or_zero(e[1]), finite_or_zero(e[2]), finite_or_zero(e[3]));
  }
  __syncthreads();
  // blocks j0 / 64 .. + 31 of the row
  const int k0 = (int)(j0 / BR_BLOCK);
  float* __restrict__ out = sums + (int64_t)b * nb_row + k0;
  const int lane = threadIdx.x & 63;
  for (int blk = threadIdx.x >> 6; blk * BR_BLOCK < BR_TILE; blk += BR_THREADS / 64) {
    const float v = ys[blk * BR_BLOCK + lane];
    float s = v * v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0 && k0 + blk < nb_keep) out[blk] = s;
  }
}

}  // namespace
