// st2_wave_volume (st2.h, added under ABI 23): per-request and per-token gain envelopes in the hand-over,
// behind the compressor and in front of the level measurement -- SSML's <prosody volume=> and the loudness part of <emphasis>.
// The row is finished before the hand-over starts and the smoothing is a local window on the 64-sample grid of st2_wave_breaks,
// so nothing here is a scan and nothing needs a workgroup per row but the last reduction.  Three launches, no atomics, no
// allocation, no synchronisation, no host read: legal under stream capture.  Grids are sized by the capacity, the work by
// `frames`.
//
// Launch 1, one workgroup per (chunk of VO_CHUNK blocks, row), fp64: the chunk's blocks and A of halo each side look their token
//   up (a binary search over the row's boundaries) and put d, the wanted gain in dB, into LDS; every block of the chunk then
//   runs the window's chain over its neighbours -- neighbouring lanes on neighbouring LDS words, the window word at a
//   wave-uniform address --, takes one pow and writes lin.  The number of blocks whose lin is not 1 is folded by shuffles and
//   four LDS words into one partial per workgroup.
// Launch 2, one workgroup per (tile of VO_TILE samples, row): st2_dynamics.hip's apply launch -- the 66 gains a tile can need in
//   LDS, a lane's 4-sample vector between two of them, 16-byte accesses wherever the row allows -- over 32-bit words, so that a
//   vector between two gains of exactly 1 is moved as it is; max |y| is folded into one partial per workgroup.
// Launch 3, one workgroup per row: the maximum of the peak partials and the sum of the count partials -- both exactly
//   associative -- into vol[b].
#include <cfloat>
#include <cmath>
#include <initializer_list>

#include "st2_pcm.h"

namespace {

constexpr int VO_THREADS = 256;
constexpr int VO_BLOCK = 64;                             // samples of a block of the gain grid (st2_wave_breaks's)
constexpr int VO_VEC = 4;                                // 4-sample vectors of a lane of launch 2, VO_THREADS apart
constexpr int VO_TILE = VO_THREADS * 4 * VO_VEC;         // samples of a workgroup of launch 2
constexpr int VO_GAINS = VO_TILE / VO_BLOCK + 2;         // the tile's blocks and one neighbour each side
constexpr int VO_CHUNK = VO_THREADS;                     // blocks of a workgroup of launch 1: one per lane
constexpr int VO_MAX_A = 64;
constexpr int VO_SPAN = VO_CHUNK + 2 * VO_MAX_A;         // a chunk and A blocks each side, at most
constexpr int VO_MAX_N = 512;
static_assert(VO_GAINS <= VO_THREADS && VO_TILE % VO_BLOCK == 0, "one gain per lane; whole blocks");

struct __attribute__((packed, aligned(4))) vo_u32x4 {
  uint32_t v[4];
};

// Rule 1: a dB value as the kernels read it -- NaN is 0, everything else inside [-60, +20]
__device__ __forceinline__ float vo_clean(float v) { return v != v ? 0.0f : fminf(fmaxf(v, -60.0f), 20.0f); }

// Rule 2's search: the largest i in [0, nb) with p[i] <= c, 0 where there is none; p does not decrease.  Not st2_tokens.h's
// token_of_frame, which takes the FIRST m with cum[m] > ts over cumulated frames and falls back to the last token: here the
// boundaries are samples, several may sit at one sample and the last of them must win, and a miss falls back to token 0.
__device__ __forceinline__ int vo_token_of_sample(const int32_t* __restrict__ p, int nb, long long c) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)p[mid] <= c) lo = mid + 1; else hi = mid;
  }
  return max(lo - 1, 0);
}

__global__ __launch_bounds__(VO_THREADS) void volume_gains_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  const int32_t* __restrict__ pos, const int32_t* __restrict__ lengths,
                                                                  int N, const float* __restrict__ db, const float* __restrict__ tok_db,
                                                                  const float* __restrict__ win, int A, float* __restrict__ lin, int kcap,
                                                                  int32_t* __restrict__ cnt_part, int nchunks) {
  __shared__ double D[VO_SPAN];  // d of block clamp(k0 - A + i, 0, K - 1) at [i]
  __shared__ int red[VO_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const int K = (int)((n + VO_BLOCK - 1) / VO_BLOCK);
  const int k0 = blockIdx.x * VO_CHUNK;
  if (k0 >= K) return;  // behind the row's end: the grid is sized by the capacity, and launch 3 reads no partial from here
  const int nb = lengths ? min(max(lengths[b], 0), N) : N;
  const double row_db = db ? (double)vo_clean(db[b]) : 0.0;
  const int32_t* __restrict__ p = pos + (int64_t)b * (N + 1);
  const int S = VO_CHUNK + 2 * A;
  for (int i = tid; i < S; i += VO_THREADS) {
    const int k = min(max(k0 - A + i, 0), K - 1);
    double t = 0.0;
    if (tok_db && nb > 0) {
      const long long c = min(64LL * k + 32, n - 1);
      t = (double)vo_clean(tok_db[(int64_t)b * N + vo_token_of_sample(p, nb, c)]);
    }
    D[i] = fmin(fmax(row_db + t, -60.0), 20.0);
  }
  __syncthreads();
  const int k = k0 + tid;
  int cnt = 0;
  if (k < K) {
    const double dk = D[tid + A];
    double acc = 0.0;
    for (int j = 0; j <= 2 * A && A > 0; ++j) acc = acc + (double)win[j] * (D[tid + j] - dk);  // D[tid + j]: block k - A + j
    const double e = dk + acc;
    const float g = e <= -60.0 ? 0.0f : (float)pow(10.0, e / 20.0);
    lin[(int64_t)b * kcap + k] = g;
    cnt = g != 1.0f ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int u = 1; u < VO_THREADS / 64; ++u) cnt += red[u];
    cnt_part[(int64_t)b * nchunks + blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(VO_THREADS) void volume_apply_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                  const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  const float* __restrict__ lin, int kcap, float* __restrict__ out,
                                                                  int64_t o_bs, float* __restrict__ peak_part, int ntiles) {
  __shared__ float sl[VO_GAINS];  // sl[j] = lin[clamp(t0 / 64 - 1 + j, 0, K - 1)]
  __shared__ float red[VO_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * VO_TILE;
  if (t0 >= n) return;  // behind the row's end: launch 3 reads no partial from here
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(wave + (int64_t)b * w_bs);
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + (int64_t)b * o_bs);
  const int K = (int)((n + VO_BLOCK - 1) / VO_BLOCK);
  const int kf = (int)(t0 / VO_BLOCK) - 1;
  if (tid < VO_GAINS) sl[tid] = lin[(int64_t)b * kcap + min(max(kf + tid, 0), K - 1)];
  __syncthreads();
  uint32_t x[VO_VEC][4];
#pragma unroll
  for (int v = 0; v < VO_VEC; ++v) {
    const long long i = t0 + 4LL * (v * VO_THREADS + tid);
    if (i >= n) break;
    if (i + 4 <= n) {
      const vo_u32x4 q = *reinterpret_cast<const vo_u32x4*>(src + i);
      x[v][0] = q.v[0]; x[v][1] = q.v[1]; x[v][2] = q.v[2]; x[v][3] = q.v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[v][e] = i + e < n ? src[i + e] : 0u;
    }
  }
  float peak = 0.0f;
#pragma unroll
  for (int v = 0; v < VO_VEC; ++v) {
    const long long i = t0 + 4LL * (v * VO_THREADS + tid);
    if (i >= n) break;
    // the four samples lie in one half of block i / 64: between the centres of blocks ka and ka + 1
    const int ka = (int)(i >> 6) - ((i & 63) < 32 ? 1 : 0);
    const float la = sl[ka - kf], lb = sl[ka + 1 - kf], dl = lb - la;
    const bool keep = la == 1.0f && lb == 1.0f;  // rule 6: the words as they are, NaN payloads included
    const int m = 2 * (int)(i - 64LL * ka) - 63;  // t = m / 128, exact: 1 <= m <= 127
    vo_u32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = __uint_as_float(x[v][e]) * fmaf((float)(m + 2 * e) * 0.0078125f, dl, la);
      y.v[e] = keep ? x[v][e] : __float_as_uint(g);
    }
    if (i + 4 <= n) {
      *reinterpret_cast<vo_u32x4*>(dst + i) = y;
#pragma unroll
      for (int e = 0; e < 4; ++e) peak = fmaxf(peak, fabsf(__uint_as_float(y.v[e])));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) {
          dst[i + e] = y.v[e];
          peak = fmaxf(peak, fabsf(__uint_as_float(y.v[e])));
        }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) peak = fmaxf(peak, __shfl_xor(peak, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = peak;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int u = 1; u < VO_THREADS / 64; ++u) peak = fmaxf(peak, red[u]);
    peak_part[(int64_t)b * ntiles + blockIdx.x] = peak;
  }
}

__global__ __launch_bounds__(VO_THREADS) void volume_final_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  const int32_t* __restrict__ cnt_part, int nchunks,
                                                                  const float* __restrict__ peak_part, int ntiles,
                                                                  float* __restrict__ vol) {
  __shared__ float red_pk[VO_THREADS / 64];
  __shared__ int red_ct[VO_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const int K = (int)((n + VO_BLOCK - 1) / VO_BLOCK);
  const int chunks = (K + VO_CHUNK - 1) / VO_CHUNK, tiles = (int)((n + VO_TILE - 1) / VO_TILE);  // the partials that were written
  float peak = 0.0f;
  int cnt = 0;
  for (int i = tid; i < tiles; i += VO_THREADS) peak = fmaxf(peak, peak_part[(int64_t)b * ntiles + i]);
  for (int i = tid; i < chunks; i += VO_THREADS) cnt += cnt_part[(int64_t)b * nchunks + i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    peak = fmaxf(peak, __shfl_xor(peak, off, 64));
    cnt += __shfl_xor(cnt, off, 64);
  }
  if ((tid & 63) == 0) {
    red_pk[tid >> 6] = peak;
    red_ct[tid >> 6] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int u = 1; u < VO_THREADS / 64; ++u) {
      peak = fmaxf(peak, red_pk[u]);
      cnt += red_ct[u];
    }
    vol[2 * b] = peak;
    vol[2 * b + 1] = (float)cnt;
  }
}

// Blocks, chunks of launch 1 and tiles of launch 2 of a row at capacity
int64_t volume_blocks(int64_t row) { return (row + VO_BLOCK - 1) / VO_BLOCK; }
int64_t volume_chunks(int64_t row) { return (volume_blocks(row) + VO_CHUNK - 1) / VO_CHUNK; }
int64_t volume_tiles(int64_t row) { return (row + VO_TILE - 1) / VO_TILE; }

}  // namespace

// lin fp32 [B][Kcap] | count partials int32 [B][chunks] | peak partials fp32 [B][tiles]
extern "C" int64_t st2_wave_volume_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0) return 0;
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  return ((int64_t)B * (volume_blocks(row) + volume_chunks(row) + volume_tiles(row)) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int st2_wave_volume(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                               int32_t samples_per_frame, int32_t trim, const int32_t* pos, const int32_t* lengths, int32_t N,
                               const float* db, const float* tok_db, int32_t A, const float* win, float* out, int64_t o_bs, float* vol,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "st2_wave_volume";
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(row <= INT32_MAX - VO_TILE, "%s: a row of %lld samples is too long for the int32 counts", who, (long long)row);
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(B == 1 || o_bs >= row, "%s: o_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)o_bs,
              (long long)row);
  ST2_REQUIRE(pos && out && vol && workspace, "%s: pos / out / vol / workspace is NULL", who);
  ST2_REQUIRE(N >= 1 && N <= VO_MAX_N, "%s: N=%d is outside 1..%d", who, N, VO_MAX_N);
  ST2_REQUIRE(A >= 0 && A <= VO_MAX_A, "%s: A=%d is outside 0..%d", who, A, VO_MAX_A);
  ST2_REQUIRE(A == 0 || win, "%s: win is NULL with A=%d", who, A);
  ST2_REQUIRE(A > 0 || !win, "%s: win must be NULL with A=0", who);
  for (const void* p : {(const void*)wave, (const void*)db, (const void*)tok_db, (const void*)win, (const void*)out,
                        (const void*)vol, (const void*)workspace})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, "%s: wave / db / tok_db / win / out / vol / workspace is not aligned to float",
                who);
  for (const void* p : {(const void*)frames, (const void*)pos, (const void*)lengths})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, "%s: frames / pos / lengths is not aligned to int32", who);
  // floats from the first sample of row 0 to the last of row B - 1, of either buffer
  const int64_t w_extent = (int64_t)(B - 1) * w_bs + row, o_extent = (int64_t)(B - 1) * o_bs + row;
  ST2_REQUIRE(out + o_extent <= wave || wave + w_extent <= out, "%s: out aliases wave", who);
  const int64_t need = st2_wave_volume_workspace_bytes(B, T_cap, samples_per_frame);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);

  const int kcap = (int)volume_blocks(row), nchunks = (int)volume_chunks(row), ntiles = (int)volume_tiles(row);
  float* lin = reinterpret_cast<float*>(workspace);
  int32_t* cnt_part = reinterpret_cast<int32_t*>(lin + (int64_t)B * kcap);
  float* peak_part = reinterpret_cast<float*>(cnt_part + (int64_t)B * nchunks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(volume_gains_kernel, dim3(nchunks, B), dim3(VO_THREADS), 0, s, frames, T_cap, samples_per_frame, trim, pos, lengths,
                     N, db, tok_db, A > 0 ? win : nullptr, A, lin, kcap, cnt_part, nchunks);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(volume_apply_kernel, dim3(ntiles, B), dim3(VO_THREADS), 0, s, wave, w_bs, frames, T_cap, samples_per_frame, trim,
                     lin, kcap, out, o_bs, peak_part, ntiles);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(volume_final_kernel, dim3(B), dim3(VO_THREADS), 0, s, frames, T_cap, samples_per_frame, trim, cnt_part, nchunks,
                     peak_part, ntiles, vol);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
