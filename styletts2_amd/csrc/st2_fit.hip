// st2_durations_fit (st2.h, added under ABI 23): every row of the integer durations rewritten to a stated
// total of frames by largest-remainder apportionment of the excess over one frame per token.  The values are the header's;
// this file is the launch.  One workgroup of 256 threads per row, thread t holds tokens t and t + 256 (N <= 512) in registers:
// every global read of the row happens before the first barrier and every write behind the last, and a thread writes only the
// two entries it read, so `out` may be `dur`.  The sums are integer block sums in a fixed order (64-lane tree, then the four
// waves in turn).  A token's rank among the remainders is a count over the row's keys (r << 10 | 1023 - n: larger = earlier,
// all distinct, 0 = takes no part) read from LDS, every lane the same address: a broadcast, no bank conflict.  All integer
// arithmetic; no atomics, no allocation, no synchronisation.  len, target and hold are read here: a captured launch serves any.
#include "st2_common.h"

namespace {

constexpr int FIT_THREADS = 256;
constexpr int FIT_WAVES = FIT_THREADS / 64;
constexpr int FIT_MAX_N = 2 * FIT_THREADS;
constexpr long long FIT_I32_MAX = 0x7FFFFFFFLL;

// The block's sums of V values per thread, to every thread.  `red` is reused from call to call: the leading barrier keeps a
// fast wave's stores behind the previous call's reads.
template <int V>
__device__ __forceinline__ void fit_block_sum(long long (&v)[V], long long (*red)[FIT_WAVES]) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
}

// dur and out may be the same buffer: no __restrict__ on either.
__global__ __launch_bounds__(FIT_THREADS) void durations_fit_kernel(const long long* dur, int N, const int32_t* __restrict__ len,
                                                                    const int32_t* __restrict__ target,
                                                                    const uint8_t* __restrict__ hold, int T_cap, long long* out,
                                                                    int32_t* __restrict__ report) {
  __shared__ unsigned long long key[FIT_MAX_N];
  __shared__ long long red[4][FIT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_b = len ? min(max(len[b], 0), N) : N;
  const long long tgt = target[b];
  const int64_t row = (int64_t)b * N;
  long long d[2], v[2];
  bool in[2], held[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = tid + j * FIT_THREADS;
    d[j] = n < N ? dur[row + n] : 0;
    in[j] = n < n_b;
    v[j] = in[j] ? min(max(d[j], 1LL), FIT_I32_MAX + 1) : 0;  // saturated: 512 of them cannot wrap, S <= 2^31 - 1 stays exact
    held[j] = in[j] && hold && hold[row + n] != 0;
  }
  long long s[4] = {0, 0, 0, 0};  // S, lo, M, the number of free tokens
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!in[j]) continue;
    s[0] += v[j];
    s[1] += held[j] ? v[j] : 1;
    s[2] += held[j] ? 0 : v[j] - 1;
    s[3] += held[j] ? 0 : 1;
  }
  fit_block_sum(s, red);
  const long long S = s[0], lo = s[1], n_free = s[3];
  const int S_rep = (int)min(S, FIT_I32_MAX);
  // the rows that are not apportioned (the conditions are the block's: no thread is left behind at a barrier)
  int flag = -1;
  if (tgt <= 0) flag = 0;
  else if (n_b == 0) flag = 2;
  else if (S > FIT_I32_MAX || lo > T_cap) flag = 3;
  else if (n_free == 0) flag = 2;
  if (flag >= 0) {
    const bool zeros = tgt > 0 && n_b == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = tid + j * FIT_THREADS;
      if (n < N) out[row + n] = zeros ? 0 : d[j];
    }
    if (report && tid == 0) {
      int32_t* rep = report + 4 * (int64_t)b;
      rep[0] = S_rep; rep[1] = S_rep; rep[2] = flag; rep[3] = 0;
    }
    return;
  }
  const long long T = min(max(tgt, lo), (long long)T_cap);
  const long long R = T - lo;
  const bool flat = s[2] == 0;  // every free token is one frame long: they share R equally, the earlier ones first
  const long long M = flat ? n_free : s[2];
  long long q[2], sq[1] = {0};
  bool takes[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = tid + j * FIT_THREADS;
    const long long m = in[j] && !held[j] ? (flat ? 1 : v[j] - 1) : 0;
    const unsigned long long p = (unsigned long long)(R * m);  // < 2^62
    q[j] = (long long)(p / (unsigned long long)M);
    const unsigned long long r = p % (unsigned long long)M;  // < M < 2^31
    takes[j] = m > 0;
    key[n] = takes[j] ? (r << 10) | (unsigned long long)(1023 - n) : 0ULL;
    sq[0] += q[j];
  }
  fit_block_sum(sq, red);  // its barriers also publish the keys
  const long long K = R - sq[0];
  int ahead[2] = {0, 0};
  if (K > 0) {
    const unsigned long long mine[2] = {key[tid], key[tid + FIT_THREADS]};
    for (int i = 0; i < n_b; ++i) {
      const unsigned long long k = key[i];
      ahead[0] += k > mine[0];
      ahead[1] += k > mine[1];
    }
  }
  long long o[2], ch[1] = {0};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    o[j] = !in[j] ? 0 : held[j] ? v[j] : 1 + q[j] + (takes[j] && ahead[j] < K ? 1 : 0);
    ch[0] += in[j] && o[j] != d[j];
  }
  fit_block_sum(ch, red);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = tid + j * FIT_THREADS;
    if (n < N) out[row + n] = o[j];
  }
  if (report && tid == 0) {
    int32_t* rep = report + 4 * (int64_t)b;
    rep[0] = S_rep; rep[1] = (int32_t)T; rep[2] = T == tgt ? 0 : 1; rep[3] = (int32_t)ch[0];
  }
}

}  // namespace

extern "C" int st2_durations_fit(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* target,
                                 const uint8_t* hold, int32_t T_cap, int64_t* out, int32_t* report, void* stream) {
  const char* who = "st2_durations_fit";
  ST2_REQUIRE(dur && target && out, "%s: dur / target / out is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535, "%s: bad geometry (B=%d: 1..65535)", who, B);
  ST2_REQUIRE(N > 0 && N <= FIT_MAX_N, "%s: bad geometry (N=%d: 1..%d, the tokens of PL-BERT's position table)", who, N, FIT_MAX_N);
  ST2_REQUIRE(T_cap > 0, "%s: T_cap=%d must be positive", who, T_cap);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(dur) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(len) % 4 == 0 && reinterpret_cast<uintptr_t>(target) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(report) % 4 == 0,
              "%s: dur / out / len / target / report is not aligned to its element", who);
  hipLaunchKernelGGL(durations_fit_kernel, dim3(B), dim3(FIT_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(dur), N, len, target, hold, T_cap, reinterpret_cast<long long*>(out), report);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
