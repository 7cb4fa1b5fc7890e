// Row b's token boundaries in decoder frames (st2.h "the boundary rule"): the one scan that the timing marks, the per-token
// prosody controls (st2_marks.hip) and the per-token pitch range (st2_intonation.hip) look a frame's token up by.
#pragma once
#include "st2_common.h"

namespace {

// c[i + 1] = min(T_cap, sum_{m <= i, m < n_b} dur[m]) into cum[i], i < N <= 512: the expansion kernel's chunked 64-lane scan
// by ONE wave (the caller's first 64 threads), with every duration clamped to 0..T_cap first -- the saturated sum is that of
// the unclamped 64-bit one, and 512 terms of at most 2^31 cannot wrap.
__device__ __forceinline__ void scan_durations(const long long* __restrict__ db, int N, int n_b, int T_cap, int* cum) {
  long long carry = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + (int)threadIdx.x;
    long long v = i < n_b ? min(max(db[i], 0LL), (long long)T_cap) : 0LL;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long u = __shfl_up(v, off, 64);
      if ((int)threadIdx.x >= off) v += u;
    }
    if (i < N) cum[i] = (int)min(v + carry, (long long)T_cap);
    carry += __shfl(v, 63, 64);
  }
}

// idx(b, t) of the expansion kernel: the first m with cum[m] > ts, ts = the frame under the HiFi-GAN one-frame right shift;
// the last token owns whatever the durations leave over.
__device__ __forceinline__ int token_of_frame(const int* cum, int N, int t, int shift) {
  const int ts = shift ? max(t - 1, 0) : t;
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= ts) lo = mid + 1; else hi = mid;
  }
  return min(lo, N - 1);
}

}  // namespace
