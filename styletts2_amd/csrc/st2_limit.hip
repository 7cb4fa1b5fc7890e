// st2_wave_limit (st2.h, added under ABI 23): a zero-phase look-ahead peak limiter between the level
// measurement (st2_level.hip) and the packing moves.  The decoder has made the whole row before the hand-over starts, so the
// limiter looks both ways: a sliding minimum of the gain every sample needs (the hold) and an FIR smoother over it.  Neither has
// a recurrence: every output sample is a function of the 4 W + 1 samples around it, and the contract (st2.h; tests/_limit_ref.py)
// is exact.  Four launches, no allocation, no synchronisation, no host read: legal under stream capture.  Grids are sized by
// the capacity, the work by `frames`.
//
// Launch 1, one lane per row: the drive gain g'_b from the level table (rule 1), in fp64 with one rounding, and whether the row
//   is left alone.  Launch 2, one workgroup per (tile, row): the envelope and the required gain r (rules 2 and 3) into the
//   workspace -- with a table the staging and the chain of st2_polyphase.h, every lane all the phases of its positions, as the
//   true-peak launch of st2_level.hip.  Launch 3, one workgroup per (tile, row): r over the tile and 2 W of halo each side in
//   LDS; the hold by doubling -- pass s makes the minima over 2 s samples from those over s, log2(2 W + 1) passes over the span
//   and one that joins two of them to the window, not 2 W + 1 compares per sample; then rule 5's chain, one LDS word and one
//   window word (at a wave-uniform address) per fmaf; then the product with 16-byte loads and stores and the tile's minimum of
//   q.  Launch 4, one wave per row: the row's minimum from its tiles'.  A minimum does not depend on order and nothing is
//   accumulated across samples, so a row's output and its two numbers depend neither on the tiling nor on the row's place in the
//   batch, bit for bit; there are no atomics.
#include <cmath>
#include <initializer_list>

#include "st2_polyphase.h"

namespace {

constexpr int LM_TILE = 2048;                    // samples of a tile of launches 2 and 3 (ops.LIMIT_TILE)
constexpr int LM_J = LM_TILE / PP_THREADS;       // positions of a lane, PP_THREADS apart
constexpr int LM_MAX_W = 1024;
constexpr int LM_ENV_LDS_FLOATS = 15360;         // launch 2 with a table: the table and the tile's span, 60 KiB at most
constexpr int LM_LDS_BYTES = 65536;              // what launch 3 may ask for
static_assert(LM_TILE % (4 * PP_THREADS) == 0, "a lane takes whole 4-sample vectors and LM_J positions");

// The staged span of launch 3 in floats: the tile, 2 W each side, and up to 3 samples in front of it down to a multiple of 4
__host__ __device__ constexpr int lm_span(int W) { return LM_TILE + 4 * W + 4; }

// Rule 3 for one sample: fp64 with one rounding to fp32; 1 where the envelope is 0
__device__ __forceinline__ float lm_required(float e, double g, double ceiling) {
  return e > 0.0f ? (float)fmin(1.0, ceiling / ((double)e * g)) : 1.0f;
}

// Four samples at i .. i + 3 of a row whose valid samples are [0, n): one 16-byte load inside, selected `fill` outside
__device__ __forceinline__ float4 lm_load4(const float* __restrict__ row, long long i, long long n, float fill) {
  if (i >= 0 && i + 4 <= n) return load_f32x4(row + i);
  float e[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) e[r] = (i + r >= 0 && i + r < n) ? row[i + r] : fill;
  return make_float4(e[0], e[1], e[2], e[3]);
}

__device__ __forceinline__ void lm_store4(float* __restrict__ row, long long i, long long n, float4 v) {
  if (i + 4 <= n) {
    f32x4_u o;
    o.v[0] = v.x; o.v[1] = v.y; o.v[2] = v.z; o.v[3] = v.w;
    *reinterpret_cast<f32x4_u*>(row + i) = o;
  } else {
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i + r < n) row[i + r] = e[r];
  }
}

// Launch 1.  info[b] = {g'_b, 1 where the row is left alone else 0}; limit[b] = {g'_b, 1} (launch 4 writes the minimum)
__global__ __launch_bounds__(64) void limit_gain_kernel(const float* __restrict__ level, const float* __restrict__ target,
                                                        const int32_t* __restrict__ start, int B, double ceiling, double max_gain,
                                                        double drive, float* __restrict__ limit, float* __restrict__ info) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int r0 = b;
  if (start)
    while (r0 > 0 && start[r0] == 0) --r0;  // the group's first row: its target decides (row 0 begins a group whatever its flag)
  const float tg = target[r0], L = level[4 * b], pk = level[4 * b + 1];
  const bool alone = !(tg == tg) || L == -INFINITY || !(pk > 0.0f);
  float g = 1.0f;
  if (!alone) g = (float)fmin(fmin(pow(10.0, ((double)tg - (double)L) / 20.0), max_gain), drive * ceiling / (double)pk);
  info[2 * b] = g;
  info[2 * b + 1] = alone ? 1.0f : 0.0f;
  limit[2 * b] = g;
  limit[2 * b + 1] = 1.0f;
}

// Launch 2 without a table: e = |x|
__global__ __launch_bounds__(PP_THREADS) void limit_envelope_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                    const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                    const float* __restrict__ info, double ceiling,
                                                                    float* __restrict__ req, int64_t row) {
  const int b = blockIdx.y;
  if (info[2 * b + 1] != 0.0f) return;  // left alone: nothing reads its r
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * LM_TILE;
  if (t0 >= n) return;  // behind the row's end: the grid is sized by the capacity
  const double g = (double)info[2 * b];
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  float* __restrict__ dst = req + (int64_t)b * row;
  for (int q = threadIdx.x; 4 * q < LM_TILE; q += PP_THREADS) {
    const long long i = t0 + 4LL * q;
    if (i >= n) break;
    const float4 x = lm_load4(src, i, n, 0.0f);
    lm_store4(dst, i, n,
              make_float4(lm_required(fabsf(finite_or_zero(x.x)), g, ceiling), lm_required(fabsf(finite_or_zero(x.y)), g, ceiling),
                          lm_required(fabsf(finite_or_zero(x.z)), g, ceiling), lm_required(fabsf(finite_or_zero(x.w)), g, ceiling)));
  }
}

// Launch 2 with a table [U][K]: e[i] = max(|x[i]|, max_p |y[U i + p]|), y the chain of st2_polyphase.h with D = 1 over the cleaned
// row.  The tile's span (the tile and K - 1 samples of halo) and the table are staged as the true-peak launch of st2_level.hip
// stages them, and a lane makes all the phases of TPJ positions PP_THREADS apart: per tap it reads its staged samples once
// (consecutive lanes, consecutive words) and PB table words at wave-uniform addresses.
constexpr int LM_TPJ = 4;

template <int PB>  // phases per pass: 8 where U is a multiple of 8, else 1
__global__ __launch_bounds__(PP_THREADS) void limit_envelope_tp_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                       const int32_t* __restrict__ frames, int T_cap, int spf,
                                                                       int trim, const float* __restrict__ taps, int U, int K,
                                                                       const float* __restrict__ info, double ceiling,
                                                                       float* __restrict__ req, int64_t row) {
  __shared__ __attribute__((aligned(16))) float lds[LM_ENV_LDS_FLOATS];
  const int b = blockIdx.y;
  if (info[2 * b + 1] != 0.0f) return;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * LM_TILE;
  if (t0 >= n) return;
  const int len = (int)min((long long)LM_TILE, n - t0);
  const double gd = (double)info[2 * b];
  float* __restrict__ tab = lds;
  float* __restrict__ xs = lds + pp_round4(U * K);  // the host checked that the span fits behind the table
  const pp_tile g = pp_tile_of(t0 * U, len * U, U, 1, K);  // outputs [U t0, U (t0 + len)): phase 0 of position t0 first
  pp_stage_table(tab, taps, U * K);
  pp_stage_span<ST2_PCM_F32, true>(xs, wave + (int64_t)b * w_bs, n, g);
  __syncthreads();
  float* __restrict__ dst = req + (int64_t)b * row + t0;
  const int centre = g.x0 + (K - 1) / 2;  // xs[centre + q] = the cleaned sample t0 + q
  for (int q0 = threadIdx.x; q0 < len; q0 += PP_THREADS * LM_TPJ) {
    const float* __restrict__ xw[LM_TPJ];  // xw[j][k] = x[c_j - (K - 1) / 2 + k]; a position past the tile's end reads q0's window
    bool valid[LM_TPJ];
    float e[LM_TPJ];
#pragma unroll
    for (int j = 0; j < LM_TPJ; ++j) {
      valid[j] = q0 + j * PP_THREADS < len;
      const int at = valid[j] ? q0 + j * PP_THREADS : q0;
      xw[j] = xs + g.x0 + at;
      e[j] = fabsf(xs[centre + at]);
    }
    for (int p0 = 0; p0 < U; p0 += PB) {
      const float* __restrict__ tp = tab + p0 * K;
      float acc[LM_TPJ][PB];
#pragma unroll
      for (int j = 0; j < LM_TPJ; ++j)
#pragma unroll
        for (int p = 0; p < PB; ++p) acc[j][p] = 0.0f;
#pragma unroll 2
      for (int k = 0; k < K; ++k) {
        float t[PB];
#pragma unroll
        for (int p = 0; p < PB; ++p) t[p] = tp[p * K + k];
#pragma unroll
        for (int j = 0; j < LM_TPJ; ++j) {
          const float x = xw[j][k];
#pragma unroll
          for (int p = 0; p < PB; ++p) acc[j][p] = fmaf(t[p], x, acc[j][p]);
        }
      }
#pragma unroll
      for (int j = 0; j < LM_TPJ; ++j)
#pragma unroll
        for (int p = 0; p < PB; ++p) e[j] = fmaxf(e[j], fabsf(acc[j][p]));
    }
#pragma unroll
    for (int j = 0; j < LM_TPJ; ++j)
      if (valid[j]) dst[q0 + j * PP_THREADS] = lm_required(e[j], gd, ceiling);
  }
}

// Launch 3.  LDS: two buffers of lm_span(W) floats.  A[i] = r[a0 + i], a0 = t0 - 2 W floored to a multiple of 4, 1 outside the
// row.  After the passes, D[i] = 1 - m[t0 - W + i] for i in [0, LM_TILE + 2 W); then S[i] = s[t0 + i] in the other buffer.
__global__ __launch_bounds__(PP_THREADS) void limit_apply_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                 const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                 const float* __restrict__ info, const float* __restrict__ req,
                                                                 int64_t row, const float* __restrict__ win, int W,
                                                                 float* __restrict__ out, float* __restrict__ tile_min, int ntile) {
  extern __shared__ __attribute__((aligned(16))) float lm_lds[];
  __shared__ float part[PP_THREADS / 64];
  const int b = blockIdx.y;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * LM_TILE;
  if (t0 >= n) return;
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  float* __restrict__ dst = out + (int64_t)b * w_bs;
  if (info[2 * b + 1] != 0.0f) {  // left alone: the valid samples' bits, NaN payloads as they are
    const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(dst);
    const long long t1 = min(n, t0 + LM_TILE);
    for (long long i = t0 + threadIdx.x; i < t1; i += PP_THREADS) d32[i] = s32[i];
    if (threadIdx.x == 0) tile_min[(long long)b * ntile + blockIdx.x] = 1.0f;
    return;
  }
  const float g = info[2 * b];
  const float* __restrict__ rr = req + (int64_t)b * row;
  const int span = lm_span(W);
  float* __restrict__ cur = lm_lds;
  float* __restrict__ nxt = lm_lds + span;
  const long long a0 = (t0 - 2LL * W) & ~3LL;  // floor to a multiple of 4, also for a negative start
  const int off = (int)(t0 - 2LL * W - a0);
  for (int q = threadIdx.x; 4 * q < span; q += PP_THREADS)
    *reinterpret_cast<float4*>(cur + 4 * q) = lm_load4(rr, a0 + 4LL * q, n, 1.0f);
  __syncthreads();
  // cur[i] = min A[i .. i + p) where that lies inside the span; an entry whose run leaves it is never read for a valid one
  const int w = 2 * W + 1;
  int p = 1;
  for (; 2 * p <= w; p *= 2) {
    for (int i = threadIdx.x; i < span; i += PP_THREADS) nxt[i] = i + p < span ? fminf(cur[i], cur[i + p]) : cur[i];
    __syncthreads();
    float* __restrict__ t = cur; cur = nxt; nxt = t;
  }
  // the window of 2 W + 1 from two runs of p (p <= w < 2 p): m[t0 - W + i] = min A[off + i .. off + i + w)
  for (int i = threadIdx.x; i < LM_TILE + 2 * W; i += PP_THREADS) nxt[i] = 1.0f - fminf(cur[off + i], cur[off + i + w - p]);
  __syncthreads();
  const float* __restrict__ D = nxt;
  float* __restrict__ S = cur;
  const int len = (int)min((long long)LM_TILE, n - t0);
  {
    float acc[LM_J];
    const float* __restrict__ d[LM_J];
#pragma unroll
    for (int j = 0; j < LM_J; ++j) {
      acc[j] = 0.0f;
      d[j] = D + (j * PP_THREADS < len ? j * PP_THREADS : 0) + threadIdx.x;  // a run of lanes past the row's end redoes run 0
    }
#pragma unroll 4
    for (int k = 0; k < w; ++k) {
      const float c = win[k];
#pragma unroll
      for (int j = 0; j < LM_J; ++j) acc[j] = fmaf(c, d[j][k], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < LM_J; ++j) S[j * PP_THREADS + threadIdx.x] = 1.0f - acc[j];
  }
  __syncthreads();
  float mn = 1.0f;
  for (int q = threadIdx.x; 4 * q < len; q += PP_THREADS) {
    const long long i = t0 + 4LL * q;
    const float4 x = lm_load4(src, i, n, 0.0f);
    const float4 r4 = lm_load4(rr, i, n, 1.0f);
    const float4 s4 = *reinterpret_cast<const float4*>(S + 4 * q);
    const float q0 = fminf(s4.x, r4.x), q1 = fminf(s4.y, r4.y), q2 = fminf(s4.z, r4.z), q3 = fminf(s4.w, r4.w);
    lm_store4(dst, i, n,
              make_float4((finite_or_zero(x.x) * g) * q0, (finite_or_zero(x.y) * g) * q1, (finite_or_zero(x.z) * g) * q2,
                          (finite_or_zero(x.w) * g) * q3));
    const float e[4] = {q0, q1, q2, q3};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i + r < n) mn = fminf(mn, e[r]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_down(mn, o, 64));
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < PP_THREADS / 64; ++v) mn = fminf(mn, part[v]);
    tile_min[(long long)b * ntile + blockIdx.x] = mn;
  }
}

// Launch 4: limit[b][1] = the minimum over the row's tiles (launch 1 wrote 1 for a row without samples)
__global__ __launch_bounds__(64) void limit_fold_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                        const float* __restrict__ tile_min, int ntile, float* __restrict__ limit) {
  const int b = blockIdx.x;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const int nt = (int)((n + LM_TILE - 1) / LM_TILE);
  float mn = 1.0f;
  for (int j = threadIdx.x; j < nt; j += 64) mn = fminf(mn, tile_min[(long long)b * ntile + j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_down(mn, o, 64));
  if (threadIdx.x == 0) limit[2 * b + 1] = mn;
}

}  // namespace

extern "C" int32_t st2_wave_limit_tile(void) { return LM_TILE; }

// r fp32 [B][row] | the tiles' minima fp32 [B][ceil(row / LM_TILE)] | {g', left alone} fp32 [B][2]
extern "C" int64_t st2_wave_limit_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0) return 0;
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  return ((int64_t)B * (row + (row + LM_TILE - 1) / LM_TILE + 2) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int st2_wave_limit(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                              int32_t samples_per_frame, int32_t trim, const float* target, double ceiling, double max_gain_db,
                              const float* level, const float* taps, int32_t up, int32_t taps_per_phase, const int32_t* start,
                              double drive_db, int32_t W, const float* win, float* out, float* limit, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  const char* who = "st2_wave_limit";
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(level && target && out && limit && win && workspace, "%s: level / target / out / limit / win / workspace is NULL", who);
  ST2_REQUIRE(ceiling > 0.0 && ceiling <= 1.0, "%s: ceiling=%g is outside (0, 1]", who, ceiling);
  ST2_REQUIRE(max_gain_db >= 0.0 && max_gain_db <= 60.0, "%s: max_gain_db=%g is outside [0, 60]", who, max_gain_db);
  ST2_REQUIRE(drive_db >= 0.0 && drive_db <= 24.0, "%s: drive_db=%g is outside [0, 24]", who, drive_db);
  ST2_REQUIRE(W >= 1 && W <= LM_MAX_W, "%s: W=%d is outside 1..%d", who, W, LM_MAX_W);
  for (const void* p : {(const void*)wave, (const void*)target, (const void*)level, (const void*)out, (const void*)limit,
                        (const void*)win, (const void*)workspace, (const void*)taps})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0,
                "%s: wave / target / level / out / limit / win / workspace / taps is not aligned to float", who);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(start) % 4 == 0, "%s: start is not aligned to int32", who);
  const int64_t extent = (int64_t)(B - 1) * w_bs + row;  // floats from the first sample of row 0 to the last of row B - 1
  ST2_REQUIRE(out + extent <= wave || wave + extent <= out, "%s: out aliases wave", who);
  const int64_t need = st2_wave_limit_workspace_bytes(B, T_cap, samples_per_frame);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);
  const int64_t ntile = (row + LM_TILE - 1) / LM_TILE;
  ST2_REQUIRE(ntile <= (1 << 24), "%s: a row of %lld samples is too long", who, (long long)row);
  const int lds = 2 * lm_span(W) * (int)sizeof(float);
  ST2_REQUIRE(lds <= LM_LDS_BYTES, "%s: a tile of %d samples and its halo of 2 W = %d each side do not fit the %d bytes of LDS", who,
              LM_TILE, 2 * W, LM_LDS_BYTES);
  if (taps) {
    if (pp_check(who, up, 1, taps_per_phase, ST2_PCM_F32)) return 1;
    const long long fit = (long long)pp_round4(up * taps_per_phase) + pp_span_cap((long long)LM_TILE * up, up, 1, taps_per_phase);
    ST2_REQUIRE(fit <= LM_ENV_LDS_FLOATS, "%s: the table (up=%d, taps_per_phase=%d) does not fit the %d bytes of LDS beside one tile of %d samples",
                who, up, taps_per_phase, LM_ENV_LDS_FLOATS * 4, LM_TILE);
  }

  float* req = reinterpret_cast<float*>(workspace);
  float* tile_min = req + (int64_t)B * row;
  float* info = tile_min + (int64_t)B * ntile;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(limit_gain_kernel, dim3(st2_cdiv(B, 64)), dim3(64), 0, s, level, target, start, B, ceiling,
                     std::pow(10.0, max_gain_db / 20.0), std::pow(10.0, drive_db / 20.0), limit, info);
  ST2_CHECK_LAUNCH(who);
  if (taps) {
    auto env = up % 8 == 0 ? limit_envelope_tp_kernel<8> : limit_envelope_tp_kernel<1>;
    hipLaunchKernelGGL(env, dim3(ntile, B), dim3(PP_THREADS), 0, s, wave, w_bs, frames, T_cap, samples_per_frame, trim, taps, up,
                       taps_per_phase, info, ceiling, req, row);
  } else {
    hipLaunchKernelGGL(limit_envelope_kernel, dim3(ntile, B), dim3(PP_THREADS), 0, s, wave, w_bs, frames, T_cap, samples_per_frame,
                       trim, info, ceiling, req, row);
  }
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(limit_apply_kernel, dim3(ntile, B), dim3(PP_THREADS), lds, s, wave, w_bs, frames, T_cap, samples_per_frame, trim,
                     info, req, row, win, W, out, tile_min, (int)ntile);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(limit_fold_kernel, dim3(B), dim3(64), 0, s, frames, T_cap, samples_per_frame, trim, tile_min, (int)ntile, limit);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
