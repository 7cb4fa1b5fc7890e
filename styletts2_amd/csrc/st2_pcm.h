// What the two packing entry points share (st2_pack.hip: st2_wave_pack; st2_resample.hip: st2_wave_resample_pack): a row's
// valid sample count, the row-offset scan, the 4-byte-aligned 16-byte source vector and the sample conversions.
#pragma once
#include "st2_common.h"

// n_b = max(0, spf * clamp(frames[b], 0, T_cap) - trim): the row's valid samples at the model rate
__device__ __forceinline__ long long pack_row_samples(const int32_t* __restrict__ frames, int b, int T_cap, int spf, int trim) {
  const long long f = min(max(frames[b], 0), T_cap);  // clamped to the capacity: never a read past the row
  return max(0LL, f * spf - trim);
}

// offsets[b] = sum_{i < b} count(i), offsets[B] = the total: one wave scanning the rows in chunks of 64
template <class F>
__device__ __forceinline__ void pack_scan_rows(int B, long long* __restrict__ offsets, F count) {
  long long carry = 0;
  for (int base = 0; base < B; base += 64) {
    const int b = base + threadIdx.x;
    const long long n = b < B ? count(b) : 0;
    long long v = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long u = __shfl_up(v, off, 64);
      if ((int)threadIdx.x >= off) v += u;
    }
    if (b < B) offsets[b] = carry + v - n;
    carry += __shfl(v, 63, 64);
  }
  if (threadIdx.x == 0) offsets[B] = carry;
}

// The source of a row's aligned body starts wherever the destination's alignment puts it: 4-byte aligned only.
struct __attribute__((packed, aligned(4))) f32x4_u {
  float v[4];
};

__device__ __forceinline__ int16_t pcm16(float x) {
  // (int16) rint(clamp(x, -1, 1) * 32767): v_rndne = round-to-nearest-even as np.rint; NaN -> 0 (fminf / fmaxf would turn
  // it into a full-scale sample)
  const float c = fminf(fmaxf(x, -1.0f), 1.0f);
  return x != x ? (int16_t)0 : (int16_t)(int)rintf(c * 32767.0f);
}

// ITU-T G.711 of a 16-bit sample, by the segment rule of the standard's reference code (G.191): the magnitude of a negative
// sample is its one's complement; mu-law keeps 14 bits, adds the bias 33 and clips at 0x1FFF, A-law keeps 13 bits.
__device__ __forceinline__ uint8_t g711_ulaw(int s) {
  const int a = min(((s < 0 ? ~s : s) >> 2) + 33, 0x1FFF);  // 33..8191: the leading one sits at bit 5..12
  const int seg = 26 - __clz(a);
  const int code = ((seg << 4) | ((a >> (seg + 1)) & 15)) ^ 0x7F;
  return (uint8_t)(s < 0 ? code : code | 0x80);
}

__device__ __forceinline__ uint8_t g711_alaw(int s) {
  int ix = (s < 0 ? ~s : s) >> 4;  // 0..2047
  if (ix > 15) {
    const int e = 28 - __clz(ix);  // 1..7: the leading one at bit e + 3
    ix = (ix >> (e - 1)) - 16 + (e << 4);
  }
  return (uint8_t)((s < 0 ? ix : ix | 0x80) ^ 0x55);
}
