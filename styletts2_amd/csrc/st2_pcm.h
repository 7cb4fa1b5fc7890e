// What the packing entry points and the clip ingest share (st2_pack.hip: st2_wave_pack; st2_resample.hip:
// st2_wave_resample_pack; st2_ingest.hip: st2_clip_ingest): a row's valid sample count, the row-offset scan, the packed source
// vectors and the sample conversions, both ways.
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
// Four 16-bit / 8-bit samples of a client's clip: a row starts wherever its sample type may.
struct __attribute__((packed, aligned(2))) s16x4_u {
  int16_t v[4];
};
struct __attribute__((packed, aligned(1))) u8x4_u {
  uint8_t v[4];
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

// The way back, ITU-T G.711 expansion to the 16-bit value at the centre of the code's interval: mu-law takes the bias off again
// (the two zero codes 0xFF / 0x7F both give 0), A-law's smallest magnitudes are +-8.
__device__ __forceinline__ int g711_ulaw_decode(int code) {
  const int inv = ~code & 0xFF;
  const int lin = ((((inv & 15) << 3) + 0x84) << ((inv >> 4) & 7)) - 0x84;  // 0..32124
  return code < 0x80 ? -lin : lin;
}

__device__ __forceinline__ int g711_alaw_decode(int code) {
  const int ix = (code ^ 0x55) & 0x7F;
  const int e = ix >> 4;
  const int man = e > 0 ? (ix & 15) + 16 : (ix & 15);
  const int lin = ((man << 4) + 8) << (e > 0 ? e - 1 : 0);  // 8..32256
  return code > 127 ? lin : -lin;
}
