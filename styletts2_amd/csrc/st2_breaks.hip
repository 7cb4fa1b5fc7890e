// st2_wave_breaks and st2_token_marks_breaks (st2.h, added under ABI 23): pauses INSIDE a row.  Every row
// of a ragged batch of waveforms at the model rate is cut inside the spans of the tokens the caller names -- at the quietest
// 128-sample window of the span, on the 64-sample grid --, both sides of a cut are faded by st2_wave_edges' ramp and digital
// silence of the stated length is spliced in.  Three launches, no atomics, no allocation, no synchronisation, no host read:
// legal under stream capture.  Grids are sized by the capacity, the work by `frames` (launch 1) and by the row's new count
// (launch 3).
//
// Launch 1, one workgroup per (tile of BR_TILE samples, row): the tile goes to LDS with 16-byte loads, a non-finite sample and
//   everything at or past n_b as 0; wave w squares block w, w + 4, ... one sample per lane and folds the 64 squares by a
//   butterfly: one read of the valid samples (st2_blocksums.h, which st2_dynamics.hip launches too).
// Launch 2, one workgroup per row: the boundaries clamped and made monotone, the cap and the exclusive scan of `ins` by wave 0,
//   then a wave per token with a break for the arg-min over its candidates; the row's segment table goes to the workspace.
// Launch 3, one workgroup per (BR_MOVE output samples, row): the table goes to LDS, a lane finds the segment of each of its four
//   4-sample vectors by binary search and moves it as 32-bit words (source 4-byte aligned, destination 16 bytes wherever `out`
//   and its row stride are); a vector that touches silence, a fade or a cut goes sample by sample.  Nothing is accumulated
//   across samples and the sums' order is fixed, so a row's output and its numbers depend neither on the tiling nor on the row's
//   place in the batch.
#include <initializer_list>

#include "st2_blocksums.h"

namespace {

constexpr int BR_VEC = 4;                         // 4-sample vectors of a lane of launch 3, BR_THREADS apart
constexpr int BR_MOVE = BR_THREADS * 4 * BR_VEC;  // output samples of a workgroup of launch 3
constexpr int BR_MAX_F = 4096;
constexpr int BR_MAX_N = 512;
// A row's table in the workspace: {m, count'} and two pad words, then a[0 .. m + 1] (a segment's first source sample; a[m + 1] =
// n_b) and d[0 .. m] (its first output sample), m <= 512 cuts
constexpr int BR_TAB_A = 4, BR_TAB_D = BR_TAB_A + BR_MAX_N + 2, BR_TAB = BR_TAB_D + BR_MAX_N + 2;
static_assert(BR_TAB % 4 == 0, "whole vectors");

struct __attribute__((packed, aligned(4))) u32x4_u {
  uint32_t v[4];
};

// Inclusive 64-lane scans of one chunk, by one wave
__device__ __forceinline__ long long wave_scan_add(long long v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long u = __shfl_up(v, off, 64);
    if ((int)(threadIdx.x & 63) >= off) v += u;
  }
  return v;
}
__device__ __forceinline__ int wave_scan_max(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if ((int)(threadIdx.x & 63) >= off) v = max(v, u);
  }
  return v;
}

__global__ __launch_bounds__(BR_THREADS) void breaks_plan_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                 const int32_t* __restrict__ pos, const int32_t* __restrict__ brk,
                                                                 int N, int max_break, const float* __restrict__ sums, int nb_row,
                                                                 int32_t* __restrict__ ins, int32_t* __restrict__ cuts,
                                                                 int32_t* __restrict__ breaks, int32_t* __restrict__ tables) {
  __shared__ int q[BR_MAX_N + 1];    // the boundaries, clamped and monotone
  __shared__ int done[BR_MAX_N];     // silence inserted up to and including token i
  __shared__ int slot[BR_MAX_N];     // the cut's number 1 .. m, 0 = token i has none
  const int b = blockIdx.x;
  const int n = (int)pack_row_samples(frames, b, T_cap, spf, trim);  // the host refused a capacity beyond int32
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* __restrict__ pb = pos + (int64_t)b * (N + 1);
  const int32_t* __restrict__ kb = brk + (int64_t)b * N;
  int32_t* __restrict__ tab = tables + (int64_t)b * BR_TAB;
  if (wave == 0) {
    int top = 0;  // rule 1: pos[0] = 0, pos[N] = n_b, clamped to 0 .. n_b, the running maximum
    for (int base = 0; base <= N; base += 64) {
      const int i = base + lane;
      int v = 0;
      if (i <= N) v = i == 0 ? 0 : i == N ? n : min(max(pb[i], 0), n);
      v = max(wave_scan_max(v), top);
      if (i <= N) q[i] = v;
      top = __shfl(v, 63, 64);
    }
    long long asked = 0;  // rule 4: the breaks asked for up to here, in 64 bits; inserted = min(asked, max_break)
    int m = 0;
    for (int base = 0; base < N; base += 64) {
      const int i = base + lane;
      const long long want = i < N ? max(kb[i], 0) : 0;
      const long long incl = wave_scan_add(want) + asked;
      const int after = (int)min(incl, (long long)max_break), before = (int)min(incl - want, (long long)max_break);
      const int number = (int)wave_scan_add(after > before ? 1 : 0) + m;
      if (i < N) {
        done[i] = after;
        slot[i] = after > before ? number : 0;
        ins[(int64_t)b * N + i] = after - before;
        if (after == before) cuts[(int64_t)b * N + i] = -1;
      }
      asked = __shfl(incl, 63, 64);
      m = __shfl(number, 63, 64);
    }
    if (lane == 0) {
      const int total = (int)min(asked, (long long)max_break);
      tab[0] = m;
      tab[1] = n + total;
      tab[BR_TAB_A] = 0;
      tab[BR_TAB_A + m + 1] = n;
      tab[BR_TAB_D] = 0;
      breaks[2 * b] = n + total;
      breaks[2 * b + 1] = total;
    }
  }
  __syncthreads();
  const float* __restrict__ s = sums + (int64_t)b * nb_row;
  for (int i = wave; i < N; i += BR_THREADS / 64) {  // rule 3: a wave per token with a break
    const int j = slot[i];
    if (j == 0) continue;
    const int p0 = q[i], p1 = q[i + 1];
    const int k_lo = (p0 + BR_BLOCK - 1) / BR_BLOCK + 1, k_hi = p1 / BR_BLOCK - 1;  // 64 (k - 1) >= p0, 64 (k + 1) <= p1
    float e = 0.0f;
    int at = 0x7fffffff;
    for (int k = k_lo + lane; k <= k_hi; k += 64) {  // ascending in a lane: < keeps the smallest k of equal windows
      const float w = s[k - 1] + s[k];
      if (at == 0x7fffffff || w < e) {
        e = w;
        at = k;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float e2 = __shfl_xor(e, off, 64);
      const int at2 = __shfl_xor(at, off, 64);
      if (at2 != 0x7fffffff && (at == 0x7fffffff || e2 < e || (e2 == e && at2 < at))) {
        e = e2;
        at = at2;
      }
    }
    if (lane == 0) {
      const int c = at != 0x7fffffff ? BR_BLOCK * at : (int)(((long long)p0 + p1) / 2);
      cuts[(int64_t)b * N + i] = c;
      tab[BR_TAB_A + j] = c;
      tab[BR_TAB_D + j] = c + done[i];
    }
  }
}

__global__ __launch_bounds__(BR_THREADS) void breaks_move_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                 const int32_t* __restrict__ tables, const float* __restrict__ ramp,
                                                                 int F, float* __restrict__ out, int64_t o_bs) {
  __shared__ int sa[BR_MAX_N + 2];  // a[0 .. m + 1]
  __shared__ int sd[BR_MAX_N + 1];  // d[0 .. m]
  __shared__ int sr[BR_MAX_N + 2];  // r[0 .. m + 1]: region j is silence [r[j], d[j]) and then segment j, [d[j], r[j + 1])
  const int b = blockIdx.y;
  const int32_t* __restrict__ tab = tables + (int64_t)b * BR_TAB;
  const int m = tab[0];
  const long long count = tab[1];
  const long long t0 = (long long)blockIdx.x * BR_MOVE;
  if (t0 >= count) return;
  for (int j = threadIdx.x; j <= m + 1; j += BR_THREADS) {
    const int a = tab[BR_TAB_A + j];
    sa[j] = a;
    if (j <= m) sd[j] = tab[BR_TAB_D + j];
    // r[j] = a[j] + what was inserted in front of cut j = a[j] + d[j - 1] - a[j - 1]
    sr[j] = j == 0 ? 0 : a + tab[BR_TAB_D + j - 1] - tab[BR_TAB_A + j - 1];
  }
  __syncthreads();
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(wave + (int64_t)b * w_bs);
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + (int64_t)b * o_bs);
  // sample k of the output, which lies in region j or behind it: a zero, a copied word, or a word of a fade times the ramp
  auto sample = [&](int k, int& j) -> uint32_t {
    while (j < m && sr[j + 1] <= k) ++j;
    if (k < sd[j]) return 0u;
    const int len = sa[j + 1] - sa[j], f = min(F, len / 2), at = k - sd[j];
    const uint32_t w = src[sa[j] + at];
    if (j > 0 && at < f) return __float_as_uint(__uint_as_float(w) * ramp[at]);
    if (j < m && at >= len - f) return __float_as_uint(__uint_as_float(w) * ramp[len - 1 - at]);
    return w;
  };
  u32x4_u x[BR_VEC];
#pragma unroll
  for (int v = 0; v < BR_VEC; ++v) {
    const long long i64 = t0 + 4LL * (v * BR_THREADS + (int)threadIdx.x);
    if (i64 >= count) break;
    const int i = (int)i64;
    int lo = 0, hi = m;  // the last region that starts at or before i (regions 1 .. m are not empty)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sr[mid] <= i) lo = mid; else hi = mid - 1;
    }
    int j = lo;
    const int len = sa[j + 1] - sa[j], f = min(F, len / 2);
    if (i >= sd[j] + (j > 0 ? f : 0) && i + 4 <= sd[j] + len - (j < m ? f : 0)) {
      x[v] = *reinterpret_cast<const u32x4_u*>(src + sa[j] + (i - sd[j]));
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) x[v].v[r] = i64 + r < count ? sample(i + r, j) : 0u;
    }
  }
#pragma unroll
  for (int v = 0; v < BR_VEC; ++v) {
    const long long i = t0 + 4LL * (v * BR_THREADS + (int)threadIdx.x);
    if (i >= count) break;
    if (i + 4 <= count) {
      *reinterpret_cast<u32x4_u*>(dst + i) = x[v];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i + r < count) dst[i + r] = x[v].v[r];
    }
  }
}

// One wave per row: marks[n] = ceil((pos[n] + the silence inserted in front of token n) * U / D), in 64 bits
__global__ __launch_bounds__(64) void token_marks_breaks_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ ins,
                                                                int N, int U, int D, int32_t* __restrict__ marks) {
  const int b = blockIdx.x;
  long long carry = 0;
  for (int base = 0; base <= N; base += 64) {
    const int n = base + (int)threadIdx.x;
    const long long v = n < N ? max(ins[(int64_t)b * N + n], 0) : 0;
    const long long incl = wave_scan_add(v) + carry;
    if (n <= N) {
      const long long at = max(pos[(int64_t)b * (N + 1) + n], 0) + (incl - v);
      marks[(int64_t)b * (N + 1) + n] = (int32_t)min((at * U + D - 1) / D, (long long)INT32_MAX);
    }
    carry = __shfl(incl, 63, 64);
  }
}

// Blocks of a row of the sums: the capacity rounded up to launch 1's tile
int64_t breaks_blocks(int64_t row) { return (row + BR_TILE - 1) / BR_TILE * (BR_TILE / BR_BLOCK); }

bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace

// block sums fp32 [B][ceil(row / BR_TILE) * 32], then the rows' tables int32 [B][BR_TAB]; N sizes nothing (a table holds 512 cuts)
extern "C" int64_t st2_wave_breaks_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame, int32_t N) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0 || N <= 0 || N > BR_MAX_N) return 0;
  return ((int64_t)B * (breaks_blocks((int64_t)samples_per_frame * T_cap) + BR_TAB) * 4 + 15) / 16 * 16;
}

extern "C" int st2_wave_breaks(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                               int32_t samples_per_frame, int32_t trim, const int32_t* pos, const int32_t* brk, int32_t N,
                               int32_t max_break, const float* ramp, int32_t F, float* out, int64_t o_bs, int32_t* ins,
                               int32_t* cuts, int32_t* breaks, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "st2_wave_breaks";
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  ST2_REQUIRE(N >= 1 && N <= BR_MAX_N, "%s: N=%d is outside 1..%d", who, N, BR_MAX_N);
  ST2_REQUIRE(max_break >= 0, "%s: max_break=%d must not be negative", who, max_break);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(row + max_break <= INT32_MAX - BR_MOVE, "%s: a row of %lld samples and %d of silence is too long for the int32 counts",
              who, (long long)row, max_break);
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(B == 1 || o_bs >= row + max_break, "%s: o_bs=%lld is less than the %lld samples of a row at capacity with its breaks",
              who, (long long)o_bs, (long long)(row + max_break));
  ST2_REQUIRE(pos && brk && ins && cuts && breaks, "%s: pos / brk / ins / cuts / breaks is NULL", who);
  ST2_REQUIRE(out && workspace, "%s: out / workspace is NULL", who);
  ST2_REQUIRE(F >= 0 && F <= BR_MAX_F, "%s: F=%d is outside 0..%d", who, F, BR_MAX_F);
  ST2_REQUIRE(F == 0 || ramp, "%s: ramp is NULL with F=%d", who, F);
  for (const void* p : {(const void*)wave, (const void*)out, (const void*)ramp, (const void*)workspace})
    ST2_REQUIRE(aligned4(p), "%s: wave / out / ramp / workspace is not aligned to float", who);
  for (const void* p : {(const void*)frames, (const void*)pos, (const void*)brk, (const void*)ins, (const void*)cuts, (const void*)breaks})
    ST2_REQUIRE(aligned4(p), "%s: frames / pos / brk / ins / cuts / breaks is not aligned to int32", who);
  // floats from the first sample of row 0 to the last of row B - 1, of either buffer
  const int64_t w_extent = (int64_t)(B - 1) * w_bs + row, o_extent = (int64_t)(B - 1) * o_bs + row + max_break;
  ST2_REQUIRE(out + o_extent <= wave || wave + w_extent <= out, "%s: out aliases wave", who);
  const int64_t need = st2_wave_breaks_workspace_bytes(B, T_cap, samples_per_frame, N);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);

  float* sums = reinterpret_cast<float*>(workspace);
  const int nb_row = (int)breaks_blocks(row);
  int32_t* tables = reinterpret_cast<int32_t*>(sums + (int64_t)B * nb_row);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(breaks_sums_kernel, dim3(st2_cdiv(row, BR_TILE), B), dim3(BR_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, sums, nb_row, nb_row);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(breaks_plan_kernel, dim3(B), dim3(BR_THREADS), 0, s, frames, T_cap, samples_per_frame, trim, pos, brk, N,
                     max_break, sums, nb_row, ins, cuts, breaks, tables);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(breaks_move_kernel, dim3(st2_cdiv(row + max_break, BR_MOVE), B), dim3(BR_THREADS), 0, s, wave, w_bs, tables,
                     F > 0 ? ramp : nullptr, F, out, o_bs);
  ST2_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int st2_token_marks_breaks(const int32_t* pos, const int32_t* ins, int32_t B, int32_t N, int32_t up, int32_t down,
                                      int32_t* marks, void* stream) {
  const char* who = "st2_token_marks_breaks";
  ST2_REQUIRE(pos && ins && marks, "%s: pos / ins / marks is NULL", who);
  ST2_REQUIRE(aligned4(pos) && aligned4(ins) && aligned4(marks), "%s: pos / ins / marks is not aligned to int32", who);
  ST2_REQUIRE(B > 0 && N >= 1 && N <= BR_MAX_N, "%s: bad geometry (B=%d, N=%d; N lies in 1..%d)", who, B, N, BR_MAX_N);
  ST2_REQUIRE(up >= 1 && up <= 1024 && down >= 1 && down <= 1024, "%s: up=%d / down=%d must lie in 1..1024", who, up, down);
  hipLaunchKernelGGL(token_marks_breaks_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), pos, ins, N, up, down,
                     marks);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
