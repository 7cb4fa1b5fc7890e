// st2_noise_fill (st2.h, added under ABI 23): the noise of a request from its seed, drawn on the device.
// The values are st2_rng.h's; this file is the launch.  One launch over (blocks, B, S), one thread per Philox counter, i.e. per
// four consecutive elements of a row: a 16-byte store where the row's base is 16-byte aligned and all four elements lie inside
// the row's limit, else one 4-byte store per element inside it.  Nothing outside [0, limit) of a row is written.  The seeds and
// the counts are read on the device: a captured launch serves any of them.  No allocation, no synchronisation.
#include <algorithm>

#include "st2_common.h"
#include "st2_rng.h"

namespace {

constexpr int RNG_THREADS = 256;
constexpr int RNG_MAX_BLOCKS = 1 << 20;  // of grid.x; a longer row's threads stride on (n < 2^34: at most 2^32 counters)

template <bool BITS>
__global__ __launch_bounds__(RNG_THREADS) void noise_fill_kernel(const int64_t* __restrict__ seeds, uint32_t stream0,
                                                                 uint32_t* __restrict__ out, int64_t s_stride, int64_t b_stride,
                                                                 int64_t n, const int32_t* __restrict__ counts,
                                                                 int64_t per_count, int64_t full_count) {
  const int b = blockIdx.y;
  int64_t limit = n;
  if (counts) {  // full_count = ceil(n / per_count): a smaller count's product is below n, no overflow
    const int32_t c = counts[b];
    if (c < full_count) limit = (int64_t)(c > 0 ? c : 0) * per_count;
  }
  const uint64_t key = (uint64_t)seeds[b];
  const uint32_t s = stream0 + blockIdx.z;
  uint32_t* __restrict__ row = out + (int64_t)blockIdx.z * s_stride + (int64_t)b * b_stride;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int64_t step = (int64_t)gridDim.x * RNG_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * RNG_THREADS + threadIdx.x; 4 * q < limit; q += step) {
    const st2_philox_words w = st2_noise_words(key, s, (uint32_t)q);
    uint32_t v[4] = {w.x[0], w.x[1], w.x[2], w.x[3]};  // stored as bit patterns either way: no float move touches the words
    if (!BITS) {
      float z[4];
      st2_noise_pair(w.x[0], w.x[1], &z[0], &z[1]);
      st2_noise_pair(w.x[2], w.x[3], &z[2], &z[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = __float_as_uint(z[j]);
    }
    const int64_t i = 4 * q;
    if (aligned && i + 4 <= limit) {
      *reinterpret_cast<uint4*>(row + i) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < limit) row[i + j] = v[j];
    }
  }
}

}  // namespace

extern "C" int st2_noise_fill(const int64_t* seeds, int32_t B, uint32_t stream0, int32_t S, int32_t kind, float* out,
                              int64_t s_stride, int64_t b_stride, int64_t n, const int32_t* counts, int64_t per_count,
                              void* stream) {
  const char* who = "st2_noise_fill";
  ST2_REQUIRE(seeds && out, "%s: seeds / out is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && S > 0 && S <= 65535, "%s: bad geometry (B=%d, S=%d: 1..65535 each)", who, B, S);
  ST2_REQUIRE(n >= 0, "%s: n=%lld must not be negative", who, (long long)n);
  ST2_REQUIRE(n < ((int64_t)1 << 34), "%s: n=%lld is too long: a row holds fewer than 2^34 elements (the counter's first word)",
              who, (long long)n);
  ST2_REQUIRE(kind == ST2_NOISE_NORMAL || kind == ST2_NOISE_BITS, "%s: unknown kind %d", who, kind);
  ST2_REQUIRE((uint64_t)stream0 + (uint64_t)(S - 1) <= 0xFFFFFFFFull, "%s: noise streams %u .. +%d pass 2^32", who, stream0, S - 1);
  ST2_REQUIRE(B == 1 || b_stride >= n, "%s: b_stride=%lld is less than the n=%lld elements of a row", who, (long long)b_stride,
              (long long)n);
  ST2_REQUIRE(B == 1 || b_stride < ((int64_t)1 << 40), "%s: b_stride=%lld is 2^40 or more", who, (long long)b_stride);
  ST2_REQUIRE(S == 1 || s_stride >= (int64_t)(B - 1) * b_stride + n,
              "%s: s_stride=%lld is less than the %lld elements the B rows of a noise stream cover", who, (long long)s_stride,
              (long long)((int64_t)(B - 1) * b_stride + n));
  ST2_REQUIRE(!counts || per_count > 0, "%s: counts given with per_count=%lld, which must be positive", who, (long long)per_count);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(seeds) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(counts) % 4 == 0,
              "%s: seeds / out / counts is not aligned to its element", who);
  if (n == 0) return 0;
  const int64_t full_count = !counts ? 0 : per_count >= n ? 1 : (n + per_count - 1) / per_count;
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  const int blocks = (int)std::min<int64_t>(((n + 3) / 4 + RNG_THREADS - 1) / RNG_THREADS, RNG_MAX_BLOCKS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (kind == ST2_NOISE_BITS)
    hipLaunchKernelGGL(noise_fill_kernel<true>, dim3(blocks, B, S), dim3(RNG_THREADS), 0, st, seeds, stream0, o, s_stride,
                       b_stride, n, counts, per_count, full_count);
  else
    hipLaunchKernelGGL(noise_fill_kernel<false>, dim3(blocks, B, S), dim3(RNG_THREADS), 0, st, seeds, stream0, o, s_stride,
                       b_stride, n, counts, per_count, full_count);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
