// st2_clip_ingest (st2.h, added under ABI 23): the way in of a zero-shot request.  A ragged batch of
// reference clips in a client's rate and sample format -- fp32, 16-bit PCM or G.711 mu-law / A-law -- is decoded, resampled to
// the model's 24 kHz by st2_wave_resample_pack's polyphase rule, trimmed of leading and trailing silence by librosa's
// effects.trim rule and handed over as fp32 rows with their device lengths: three launches, no host read and no allocation, so
// the call is legal under stream capture and runs straight into the style path.
#include "st2_polyphase.h"
#include "st2_trim.h"

namespace {

constexpr int IN_THREADS = PP_THREADS;
constexpr int IN_HOP = TRIM_HOP;    // the trim's hop (st2_trim.h): a frame of 2048 samples is four block sums
static_assert(IN_THREADS == TRIM_THREADS, "the trim rule's functions are written for this workgroup");
constexpr int IN_TILE_MAX = 1024;   // output samples of a workgroup, a multiple of IN_HOP; rows of `work` are padded to it
constexpr int IN_LDS_BYTES = 63 * 1024;

constexpr int64_t in_row_stride(int64_t L_cap) { return (L_cap + IN_TILE_MAX - 1) / IN_TILE_MAX * IN_TILE_MAX; }

// n_b = clamp(n[b], 0, N_cap) source samples; `full` = ceil(n_b U / D) samples at 24 kHz before the capacity cuts them
__device__ __forceinline__ long long in_row_samples(const int32_t* __restrict__ n, int b, int N_cap, int U, int D) {
  const long long v = min(max(n[b], 0), N_cap);
  return (v * U + D - 1) / D;
}

// Launch one.  Workgroup (t, b) makes the 24 kHz samples [j0, j0 + tile) of row b, zeros from m_b on, into `work` and the sums
// of squares of the tile's 512-sample blocks into `sums`:
//   1. the phase table and the tile's decoded input span [c(j0) - h, c(j1 - 1) - h + K) go to LDS (st2_polyphase.h);
//   2. lane l makes the samples j0 + l, j0 + l + 256, ... by the chain of st2_polyphase.h;
//   3. the tile leaves with one 16-byte store per lane and pass, and its block sums by the rule of st2_trim.h.
// A workgroup whose tile lies behind the row's end leaves before any barrier: the grid is sized by the capacity.
template <int FMT>
__global__ __launch_bounds__(IN_THREADS) void ingest_resample_kernel(
    const typename pcm_fmt<FMT>::type* __restrict__ src, int64_t src_bs, const int32_t* __restrict__ n_in, int N_cap, int U, int D,
    const float* __restrict__ taps, int K, int tile, int L_cap, float* __restrict__ work, int64_t wk_bs,
    float* __restrict__ sums, int nb_row) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y;
  const long long n = min(max(n_in[b], 0), N_cap);
  const long long m = min((long long)L_cap, (n * U + D - 1) / D);
  const long long j0 = (long long)blockIdx.x * tile;
  if (j0 >= m) return;
  const int len = (int)min((long long)tile, m - j0);
  const pp_tile tg = pp_tile_of(j0, len, U, D, K);

  float* __restrict__ tab = lds;
  float* __restrict__ xs = lds + pp_round4(U * K);
  float* __restrict__ ys = xs + pp_round4((int)pp_span_cap(tile, U, D, K));
  // -- 1. stage
  pp_stage_table(tab, taps, U * K);
  pp_stage_span<FMT>(xs, src + (int64_t)b * src_bs, n, tg);
  __syncthreads();
  // -- 2. filter
  for (int jj = threadIdx.x; jj < tile; jj += IN_THREADS) ys[jj] = jj < len ? pp_chain(tab, xs, tg, jj, U, D, K) : 0.0f;
  __syncthreads();
  // -- 3. store and block sums
  float* __restrict__ dst = work + (int64_t)b * wk_bs + j0;  // 16-byte aligned: wk_bs and j0 are multiples of 512
  for (int q = threadIdx.x; 4 * q < tile; q += IN_THREADS)
    *reinterpret_cast<float4*>(dst + 4 * q) = *reinterpret_cast<const float4*>(ys + 4 * q);
  trim_block_sums(ys, tile, sums + (int64_t)b * nb_row + j0 / IN_HOP);
}

// Launch two, one workgroup per row: the bounds from the block sums (st2_trim.h: frame energies, their maximum, the first and
// last non-silent frame), the minimum-length rule; writes len / start / flags and the row's start for the gather.
__global__ __launch_bounds__(IN_THREADS) void ingest_bounds_kernel(const int32_t* __restrict__ n_in, int N_cap, int U, int D,
                                                                   int L_cap, float threshold /* < 0: no trim */, int L_min,
                                                                   const float* __restrict__ sums, int nb_row,
                                                                   int32_t* __restrict__ len, int32_t* __restrict__ start,
                                                                   int32_t* __restrict__ flags, int32_t* __restrict__ cut) {
  __shared__ float slot_f[4];
  __shared__ int slot_i[4];
  const int b = blockIdx.x;
  const long long full = in_row_samples(n_in, b, N_cap, U, D);
  const int m = (int)min((long long)L_cap, full);
  int s0 = 0, s1 = m;
  if (threshold >= 0.0f) {
    trim_bounds(sums + (int64_t)b * nb_row, m, threshold, slot_f, slot_i, &s0, &s1);
  }
  if (threadIdx.x != 0) return;
  int fl = full > L_cap ? 1 : 0;
  if (s1 - s0 < L_min) {
    fl |= 2;
    s1 = (int)min((long long)m, (long long)s0 + L_min);
    s0 = max(0, s1 - L_min);
  }
  len[b] = s1 - s0;
  cut[b] = s0;
  if (start) start[b] = s0;
  if (flags) flags[b] = fl;
}

// Launch three: wave[b][i] = work[b][cut[b] + i] for i < len[b].  The source is 4-byte aligned at cut[b] (the minimum-length
// rule may put it anywhere), the destination 16-byte aligned; the vector the row's end cuts is peeled sample by sample.
__global__ __launch_bounds__(IN_THREADS) void ingest_gather_kernel(const float* __restrict__ work, int64_t wk_bs,
                                                                   const int32_t* __restrict__ cut,
                                                                   const int32_t* __restrict__ len, float* __restrict__ wave,
                                                                   int64_t w_bs) {
  const int b = blockIdx.y;
  const int L = len[b];
  const long long i = ((long long)blockIdx.x * IN_THREADS + threadIdx.x) * 4;
  if (i >= L) return;
  const float* __restrict__ s = work + (int64_t)b * wk_bs + cut[b] + i;
  float* __restrict__ d = wave + (int64_t)b * w_bs + i;
  if (i + 4 <= L) {
    *reinterpret_cast<float4*>(d) = load_f32x4(s);
  } else {
    for (int r = 0; i + r < L; ++r) d[r] = s[r];
  }
}

}  // namespace

// work: [B][stride] fp32 rows at 24 kHz | [B][stride / 512] block sums | [B] int32 starts, stride = L_cap rounded up to 1024
extern "C" int64_t st2_clip_ingest_work_bytes(int32_t B, int32_t L_cap) {
  if (B <= 0 || L_cap <= 0) return 0;
  const int64_t stride = in_row_stride(L_cap);
  return ((int64_t)B * (stride * 4 + stride / IN_HOP * 4 + 4) + 15) / 16 * 16;
}

extern "C" int st2_clip_ingest(const void* src, int64_t src_bs, const int32_t* n, int32_t B, int32_t N_cap, int32_t fmt, int32_t up,
                               int32_t down, const float* taps, int32_t taps_per_phase, float top_db, int32_t L_min, float* wave,
                               int64_t w_bs, int32_t L_cap, int32_t* len, int32_t* start, int32_t* flags, void* work,
                               int64_t work_bytes, void* stream) {
  ST2_REQUIRE(src && n && taps && wave && len && work, "st2_clip_ingest: src / n / taps / wave / len / work is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535 && N_cap > 0 && L_cap > 0, "st2_clip_ingest: bad geometry (B=%d, N_cap=%d, L_cap=%d)", B, N_cap,
              L_cap);
  ST2_REQUIRE(w_bs >= L_cap && w_bs % 4 == 0, "st2_clip_ingest: w_bs=%lld must be a multiple of 4 and hold L_cap=%d samples",
              (long long)w_bs, L_cap);
  ST2_REQUIRE(B == 1 || src_bs >= N_cap, "st2_clip_ingest: src_bs=%lld is less than the N_cap=%d samples of a row",
              (long long)src_bs, N_cap);
  if (pp_check("st2_clip_ingest", up, down, taps_per_phase, fmt)) return 1;
  ST2_REQUIRE(L_min >= 0 && L_min <= L_cap, "st2_clip_ingest: L_min=%d is outside 0..L_cap=%d", L_min, L_cap);
  ST2_REQUIRE(top_db == top_db, "st2_clip_ingest: top_db is NaN");
  const int64_t need = st2_clip_ingest_work_bytes(B, L_cap);
  ST2_REQUIRE(work_bytes >= need, "st2_clip_ingest: work_bytes=%lld is less than the %lld st2_clip_ingest_work_bytes asks for",
              (long long)work_bytes, (long long)need);
  const int size = pcm_sample_bytes(fmt);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(src) % size == 0 && reinterpret_cast<uintptr_t>(taps) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(wave) % 16 == 0 && reinterpret_cast<uintptr_t>(work) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(n) % 4 == 0 && reinterpret_cast<uintptr_t>(len) % 4 == 0,
              "st2_clip_ingest: src / taps / n / len is not aligned to its sample type, or wave / work not to 16 bytes");
  // the largest tile (a multiple of the trim's 512-sample hop) whose input span and output fit beside the table
  int tile = IN_TILE_MAX;
  auto lds_floats = [&](int t) {
    return (long long)pp_round4(up * taps_per_phase) + pp_round4((int)pp_span_cap(t, up, down, taps_per_phase)) + t;
  };
  while (tile >= IN_HOP && lds_floats(tile) * 4 > IN_LDS_BYTES) tile /= 2;
  ST2_REQUIRE(tile >= IN_HOP, "st2_clip_ingest: a table of %d x %d taps at ratio %d / %d does not fit the %d bytes of LDS", up,
              taps_per_phase, up, down, IN_LDS_BYTES);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t wk_bs = in_row_stride(L_cap);
  const int nb_row = (int)(wk_bs / IN_HOP);
  float* rows = reinterpret_cast<float*>(work);
  float* sums = rows + (int64_t)B * wk_bs;
  int32_t* cut = reinterpret_cast<int32_t*>(sums + (int64_t)B * nb_row);
  pcm_dispatch(fmt, [&](auto f) {
    hipLaunchKernelGGL((ingest_resample_kernel<f()>), dim3(st2_cdiv(L_cap, tile), B), dim3(IN_THREADS),
                       (size_t)lds_floats(tile) * 4, s, reinterpret_cast<const typename pcm_fmt<f()>::type*>(src), src_bs, n, N_cap,
                       up, down, taps, taps_per_phase, tile, L_cap, rows, wk_bs, sums, nb_row);
  });
  ST2_CHECK_LAUNCH("st2_clip_ingest (resample)");
  const float threshold = top_db > 0.0f ? trim_threshold(top_db) : -1.0f;
  hipLaunchKernelGGL(ingest_bounds_kernel, dim3(B), dim3(IN_THREADS), 0, s, n, N_cap, up, down, L_cap, threshold, L_min, sums,
                     nb_row, len, start, flags, cut);
  ST2_CHECK_LAUNCH("st2_clip_ingest (bounds)");
  hipLaunchKernelGGL(ingest_gather_kernel, dim3(st2_cdiv(L_cap, IN_THREADS * 4), B), dim3(IN_THREADS), 0, s, rows, wk_bs, cut, len,
                     wave, w_bs);
  ST2_CHECK_LAUNCH("st2_clip_ingest (gather)");
  return 0;
}
