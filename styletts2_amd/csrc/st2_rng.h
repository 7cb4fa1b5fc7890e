// Counter-based noise (st2_noise_fill, st2.h): the device-inline generator.  This header is the one
// statement of which value every element of a request's noise has -- the whole reproducibility contract.
//
// Generator: Philox4x32-10 as published (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// library): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between
// rounds.  Known answers: tests/_rng_ref.py.
//
// Value: element i of noise stream s of a row with seed k is output (i mod 4) of the four values made from
//     Philox(counter = (i div 4, 0, s, 0), key = (lo32(k), hi32(k))),      k the int64 seed read as uint64,
// for i < 2^34 (i div 4 fills the counter's first word).  Nothing else enters: not the row's place in the batch, not the batch
// size, not the launch shape.
//
// ST2_NOISE_BITS: the four values are the four 32-bit words x0 x1 x2 x3.
// ST2_NOISE_NORMAL: two Box-Muller pairs, from the words (x0, x1) and (x2, x3).  For a pair (x, x'):
//     u1 = ((x >> 8) + 0.5) 2^-24           in (0, 1), never 0
//     r  = sqrt(-2 ln u1)                    <= sqrt(50 ln 2) = 5.887
//     a  = 2 ((x' >> 8) 2^-24)               in [0, 2), exact in fp32: no angle-rounding error enters
//     the pair is (r cos(pi a), r sin(pi a)).
// (x >> 8) + 0.5 has 25 significant bits.  fp32 rounds it once x >> 8 reaches 2^23, by 2^-25 in u1 -- which, next to u1 = 1,
// where ln u1 is about u1 - 1, is the whole of r (u1 = 1 - 2^-25 would round to 1 and r = 2.4e-4 to 0).  So the rounding error
// e = u1 - fl(u1), itself exact in fp32, is put back to first order: ln u1 = logf(fl(u1)) + e / fl(u1), the neglected term
// below 2^-51.  logf, sqrtf and sincospif are the library's full-precision functions, no fast-math intrinsic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct st2_philox_words {
  uint32_t x[4];
};

__host__ __device__ __forceinline__ st2_philox_words st2_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                                       uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {{c0, c1, c2, c3}};
}

// The four words of counter `q` (= i div 4) of noise stream `s` under the seed `k`
__host__ __device__ __forceinline__ st2_philox_words st2_noise_words(uint64_t k, uint32_t s, uint32_t q) {
  return st2_philox4x32_10(q, 0u, s, 0u, (uint32_t)k, (uint32_t)(k >> 32));
}

// One Box-Muller pair from the words (x, xa): *z0 = r cos, *z1 = r sin
__device__ __forceinline__ void st2_noise_pair(uint32_t x, uint32_t xa, float* z0, float* z1) {
  const float m = (float)(x >> 8);           // exact: 24 bits
  const float h = m + 0.5f;                  // rounds from m = 2^23 on
  const float e = (m - h) + 0.5f;            // what the rounding took: -0.5, 0 or 0.5, exact
  const float uh = h * 0x1p-24f;
  const float ln_u = logf(uh) + (e * 0x1p-24f) / uh;
  const float r = sqrtf(-2.0f * ln_u);
  float sn, cs;
  sincospif(2.0f * ((float)(xa >> 8) * 0x1p-24f), &sn, &cs);
  *z0 = r * cs;
  *z1 = r * sn;
}
