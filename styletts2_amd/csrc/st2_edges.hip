// st2_wave_edges (st2.h, added under ABI 23): the way out's counterpart of st2_clip_ingest's trim.  Every
// row of a ragged batch of waveforms at the model rate is cut to its speech -- librosa's effects.trim rule, stated once in
// st2_trim.h for both directions -- with a per-row threshold and per-row pads read on the device, moved to the front of a
// second buffer with a short fade at every cut edge, and reported as {head, count}.  Three launches, no atomics, no
// allocation, no synchronisation, no host read: legal under stream capture.  Grids are sized by the capacity, the work by
// `frames` (launch 1) and by `edges` (launch 3).
//
// Launch 1, one workgroup per (tile of ED_TILE samples, row): the tile goes to LDS with 16-byte loads, a non-finite sample and
//   everything at or past n_b as 0, and its four block sums leave by st2_trim.h's rule: one read of the valid samples.
// Launch 2, one workgroup per row: the threshold from top_db[b] in double with one rounding, st2_trim.h's bounds, the pads in
//   64-bit integers; lane 0 writes edges[b].  A row that is left alone never reads its sums.
// Launch 3, one workgroup per (ED_MOVE samples, row): lane l moves four samples at a time as 32-bit words -- the source at
//   wave + head + i is 4-byte aligned only, the destination vector is 16 bytes wherever `out` and its row stride are -- and
//   multiplies the words of a fade, nothing else, as floats.  Nothing is accumulated across samples and the sums' order is
//   fixed, so a row's output and its two numbers depend neither on the tiling nor on the row's place in the batch.
#include <initializer_list>

#include "st2_pcm.h"
#include "st2_trim.h"

namespace {

constexpr int ED_TILE = 2048;                      // samples of a workgroup of launch 1: one 512-sample block per wave
constexpr int ED_VEC = 4;                          // 4-sample vectors of a lane of launch 3, TRIM_THREADS apart
constexpr int ED_MOVE = TRIM_THREADS * 4 * ED_VEC; // samples of a workgroup of launch 3
constexpr int ED_MAX_F = 4096;
static_assert(ED_TILE % TRIM_HOP == 0 && ED_TILE % (4 * TRIM_THREADS) == 0, "whole blocks, whole vectors per lane");

struct __attribute__((packed, aligned(4))) u32x4_u {
  uint32_t v[4];
};

__global__ __launch_bounds__(TRIM_THREADS) void edges_sums_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                  const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  float* __restrict__ sums, int nb_row) {
  __shared__ __attribute__((aligned(16))) float ys[ED_TILE];
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long j0 = (long long)blockIdx.x * ED_TILE;
  if (j0 >= n) return;  // behind the row's end: the grid is sized by the capacity
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
#pragma unroll
  for (int q = threadIdx.x; 4 * q < ED_TILE; q += TRIM_THREADS) {
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
  // blocks j0 / 512 .. + 3 of the row: all four lie below nb_row, which is sized by the capacity rounded up to the tile
  trim_block_sums(ys, ED_TILE, sums + (int64_t)b * nb_row + j0 / TRIM_HOP);
}

__global__ __launch_bounds__(TRIM_THREADS) void edges_bounds_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                    const float* __restrict__ top_db,
                                                                    const int32_t* __restrict__ keep,
                                                                    const float* __restrict__ sums, int nb_row,
                                                                    int32_t* __restrict__ edges) {
  __shared__ float slot_f[4];
  __shared__ int slot_i[4];
  const int b = blockIdx.x;
  const int n = (int)pack_row_samples(frames, b, T_cap, spf, trim);  // the host refused a capacity beyond int32
  const float td = top_db[b];
  int s0 = 0, s1 = n;
  if (td > 0.0f && n > 0)  // NaN: false.  Uniform over the workgroup: trim_bounds holds barriers
    trim_bounds(sums + (int64_t)b * nb_row, n, trim_threshold(td), slot_f, slot_i, &s0, &s1);
  if (threadIdx.x != 0) return;
  const long long lead = max(keep[2 * b], 0), tail = max(keep[2 * b + 1], 0);
  const long long head = max(0LL, (long long)s0 - lead);
  const long long stop = min((long long)n, (long long)s1 + tail);
  edges[2 * b] = (int32_t)head;
  edges[2 * b + 1] = (int32_t)(stop - head);
}

__global__ __launch_bounds__(TRIM_THREADS) void edges_move_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                  const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  const int32_t* __restrict__ edges, const float* __restrict__ ramp,
                                                                  int F, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  // launch 2 wrote 0 <= head and head + count <= n; clamped again so that no value of `edges` moves anything out of the row
  const long long head = min(max((long long)edges[2 * b], 0LL), n);
  const long long count = min(max((long long)edges[2 * b + 1], 0LL), n - head);
  const long long t0 = (long long)blockIdx.x * ED_MOVE;
  if (t0 >= count) return;
  const int f = (int)min((long long)F, count / 2);
  const long long lead_end = head > 0 ? f : 0;                     // samples [0, lead_end) fade in
  const long long tail_at = head + count < n ? count - f : count;  // samples [tail_at, count) fade out
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(wave + (int64_t)b * w_bs) + head;
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + (int64_t)b * w_bs);
  u32x4_u x[ED_VEC];
#pragma unroll
  for (int v = 0; v < ED_VEC; ++v) {
    const long long i = t0 + 4LL * (v * TRIM_THREADS + (int)threadIdx.x);
    if (i + 4 <= count) {
      x[v] = *reinterpret_cast<const u32x4_u*>(src + i);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) x[v].v[r] = i + r < count ? src[i + r] : 0u;
    }
  }
#pragma unroll
  for (int v = 0; v < ED_VEC; ++v) {
    const long long i = t0 + 4LL * (v * TRIM_THREADS + (int)threadIdx.x);
    if (i >= count) break;
    if (i < lead_end || i + 4 > tail_at) {  // a vector that touches a fade: one fp32 multiply on the samples inside it
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long k = i + r;
        if (k < lead_end) x[v].v[r] = __float_as_uint(__uint_as_float(x[v].v[r]) * ramp[k]);
        else if (k >= tail_at && k < count) x[v].v[r] = __float_as_uint(__uint_as_float(x[v].v[r]) * ramp[count - 1 - k]);
      }
    }
    if (i + 4 <= count) {
      *reinterpret_cast<u32x4_u*>(dst + i) = x[v];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i + r < count) dst[i + r] = x[v].v[r];
    }
  }
}

// Blocks of a row of the sums: the capacity rounded up to launch 1's tile
int64_t edges_blocks(int64_t row) { return (row + ED_TILE - 1) / ED_TILE * (ED_TILE / TRIM_HOP); }

}  // namespace

extern "C" int32_t st2_wave_edges_tile(void) { return ED_TILE; }

// block sums fp32 [B][ceil(row / ED_TILE) * 4]
extern "C" int64_t st2_wave_edges_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0) return 0;
  return ((int64_t)B * edges_blocks((int64_t)samples_per_frame * T_cap) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int st2_wave_edges(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                              int32_t samples_per_frame, int32_t trim, const float* top_db, const int32_t* keep, const float* ramp,
                              int32_t F, float* out, int32_t* edges, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "st2_wave_edges";
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(row <= INT32_MAX - ED_MOVE, "%s: a row of %lld samples is too long for the int32 edges", who, (long long)row);
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(top_db && keep && out && edges && workspace, "%s: top_db / keep / out / edges / workspace is NULL", who);
  ST2_REQUIRE(F >= 0 && F <= ED_MAX_F, "%s: F=%d is outside 0..%d", who, F, ED_MAX_F);
  ST2_REQUIRE(F == 0 || ramp, "%s: ramp is NULL with F=%d", who, F);
  for (const void* p : {(const void*)wave, (const void*)top_db, (const void*)out, (const void*)ramp, (const void*)workspace})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, "%s: wave / top_db / out / ramp / workspace is not aligned to float", who);
  for (const void* p : {(const void*)frames, (const void*)keep, (const void*)edges})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, "%s: frames / keep / edges is not aligned to int32", who);
  const int64_t extent = (int64_t)(B - 1) * w_bs + row;  // floats from the first sample of row 0 to the last of row B - 1
  ST2_REQUIRE(out + extent <= wave || wave + extent <= out, "%s: out aliases wave", who);
  const int64_t need = st2_wave_edges_workspace_bytes(B, T_cap, samples_per_frame);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);

  float* sums = reinterpret_cast<float*>(workspace);
  const int nb_row = (int)edges_blocks(row);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(edges_sums_kernel, dim3(st2_cdiv(row, ED_TILE), B), dim3(TRIM_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, sums, nb_row);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(edges_bounds_kernel, dim3(B), dim3(TRIM_THREADS), 0, s, frames, T_cap, samples_per_frame, trim, top_db, keep,
                     sums, nb_row, edges);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(edges_move_kernel, dim3(st2_cdiv(row, ED_MOVE), B), dim3(TRIM_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, edges, F > 0 ? ramp : nullptr, F, out);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
