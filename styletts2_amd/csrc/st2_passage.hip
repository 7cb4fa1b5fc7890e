// st2_wave_pack_gaps (st2.h, added under ABI 23): the packing step of the sync-free path with a BREAK
// behind every row -- silence of a per-row length read from device memory, in the hand-over's own rate and sample format.  The
// rows of one batch are then the sentences of a passage, laid out as a client plays them.  Here too is the pack plan that serves
// all three packing entries (st2_pcm.h): a scan that counts every row's samples and its gap, the move kernel of st2_wave_pack
// or st2_wave_resample_pack (it takes a row's start from offsets[b] and its length from the frames), and a fill of the gaps.
#include "st2_polyphase.h"

namespace {

// g_b = clamp(gaps[b], 0, gap_cap) output samples
__device__ __forceinline__ long long gap_samples(const int32_t* __restrict__ gaps, int b, int gap_cap) {
  return min(max(gaps[b], 0), gap_cap);
}

// offsets[b] = sum_{i < b} (m_i + g_i), offsets[B] = the total: one wave scanning the rows in chunks of 64.  gaps == NULL: no
// g_i; U = D = 1: m_i = n_i, st2_wave_pack's count.
__global__ __launch_bounds__(64) void pack_offsets_kernel(const int32_t* __restrict__ frames, int B, int T_cap, int spf, int trim,
                                                          int U, int D, const int32_t* __restrict__ gaps, int gap_cap,
                                                          long long* __restrict__ offsets) {
  long long carry = 0;
  for (int base = 0; base < B; base += 64) {
    const int b = base + threadIdx.x;
    long long n = 0;
    if (b < B) n = pack_row_out_samples(frames, b, T_cap, spf, trim, U, D) + (gaps ? gap_samples(gaps, b, gap_cap) : 0LL);
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

constexpr int FILL_THREADS = 256;
constexpr int FILL_ITERS = 4;  // 16-byte stores per lane and workgroup

// Workgroup (chunk, b) writes FILL_THREADS * FILL_ITERS 16-byte vectors of the ALIGNED body of row b's gap -- the g_b samples
// in front of offsets[b + 1] -- with the format's code of a zero sample; chunk 0 also writes the gap's head (the samples in front
// of the first 16-byte boundary of the destination) and its tail, both shorter than one vector.  A workgroup whose chunk lies
// behind the gap's end -- or behind the write bound -- leaves at once: the grid is sized by gap_cap, the work by g_b.
template <int FMT>
__global__ __launch_bounds__(FILL_THREADS) void gap_fill_kernel(const int32_t* __restrict__ gaps, int gap_cap, int B,
                                                                typename pcm_fmt<FMT>::type* __restrict__ out,
                                                                long long out_capacity, const long long* __restrict__ offsets) {
  using OUT = typename pcm_fmt<FMT>::type;
  constexpr int V = 16 / (int)sizeof(OUT);
  const int b = blockIdx.y;
  const long long limit = min(offsets[B], out_capacity);  // nothing at or past it is written
  const long long g = gap_samples(gaps, b, gap_cap);
  const long long start = offsets[b + 1] - g;  // = offsets[b] + m_b: the scan counted the same g
  const long long n = min(g, max(limit - start, 0LL));
  if (n <= 0) return;
  OUT* __restrict__ dst = out + start;
  const long long head = min(n, (long long)((16 - (int)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / (long long)sizeof(OUT));
  const long long nvec = (n - head) / V;
  const long long v0 = (long long)blockIdx.x * (FILL_THREADS * FILL_ITERS);
  if (v0 >= nvec && blockIdx.x != 0) return;
  const OUT z = pcm_encode<FMT>(0.0f);  // silence as the format's own encoder states it: 0.0f, 0, mu-law 0xFF, A-law 0xD5
  union {
    OUT s[V];
    uint4 q;
  } zv;
#pragma unroll
  for (int r = 0; r < V; ++r) zv.s[r] = z;
#pragma unroll
  for (int it = 0; it < FILL_ITERS; ++it) {
    const long long v = v0 + it * FILL_THREADS + threadIdx.x;
    if (v >= nvec) break;
    *reinterpret_cast<uint4*>(dst + head + v * V) = zv.q;
  }
  if (blockIdx.x == 0) {
    const long long t0 = head + nvec * V;  // head < V and n - t0 < V, V <= 16: one lane per sample
    long long i = -1;
    if ((long long)threadIdx.x < head) i = threadIdx.x;
    else if (threadIdx.x >= 64 && t0 + (threadIdx.x - 64) < n) i = t0 + (threadIdx.x - 64);
    if (i >= 0) dst[i] = z;
  }
}

}  // namespace

int pack_plan(const char* who, const pack_args& a) {
  const bool rs = a.taps != nullptr;  // the resampling move; else the plain one
  ST2_REQUIRE(a.wave && a.frames && a.out && a.offsets,
              rs ? "%s: wave / frames / taps / out / offsets is NULL" : "%s: wave / frames / out / offsets is NULL", who);
  ST2_REQUIRE(a.B > 0 && a.B <= 65535 && a.T_cap > 0 && a.samples_per_frame > 0,
              "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)", who, a.B, a.T_cap, a.samples_per_frame);
  ST2_REQUIRE(a.trim >= 0 && a.out_capacity >= 0, "%s: trim=%d / out_capacity=%lld must not be negative", who, a.trim,
              (long long)a.out_capacity);
  if (rs) {
    if (pp_check(who, a.up, a.down, a.taps_per_phase, a.fmt)) return 1;
  } else {
    ST2_REQUIRE(a.fmt == ST2_PCM_F32 || a.fmt == ST2_PCM_S16, "%s: unknown format %d", who, a.fmt);
  }
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(a.out) % pcm_sample_bytes(a.fmt) == 0 && reinterpret_cast<uintptr_t>(a.wave) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(a.taps) % 4 == 0,
              rs ? "%s: wave / taps / out is not aligned to its sample type" : "%s: wave / out is not aligned to its sample type", who);
  const int64_t row = (int64_t)a.samples_per_frame * a.T_cap;
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(a.level) % 4 == 0, "%s: level is not aligned to float", who);
  ST2_REQUIRE(a.B == 1 || a.w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who,
              (long long)a.w_bs, (long long)row);
  int tile = 0;
  if (rs && pack_resample_tile(who, a, &tile)) return 1;

  const bool fill = a.gaps && a.gap_cap > 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
  long long* offs = reinterpret_cast<long long*>(a.offsets);
  hipLaunchKernelGGL(pack_offsets_kernel, dim3(1), dim3(64), 0, s, a.frames, a.B, a.T_cap, a.samples_per_frame, a.trim, a.up,
                     a.down, fill ? a.gaps : nullptr, a.gap_cap, offs);
  ST2_CHECK_LAUNCH(who);
  if (rs ? pack_resample_move(who, a, tile) : pack_move(who, a)) return 1;
  if (!fill) return 0;
  const int gx = st2_cdiv(st2_cdiv(a.gap_cap, 16 / pcm_sample_bytes(a.fmt)), FILL_THREADS * FILL_ITERS);  // >= 1: gap_cap > 0
  pcm_dispatch(a.fmt, [&](auto f) {
    hipLaunchKernelGGL((gap_fill_kernel<f()>), dim3(gx, a.B), dim3(FILL_THREADS), 0, s, a.gaps, a.gap_cap, a.B,
                       reinterpret_cast<typename pcm_fmt<f()>::type*>(a.out), (long long)a.out_capacity, offs);
  });
  ST2_CHECK_LAUNCH(who);
  return 0;
}

// What st2_wave_pack_gaps and st2_wave_pack_level refuse themselves, in the entry's own name, and the plan behind them
static int pack_gaps_entry(const char* who, const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                           int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                           int32_t taps_per_phase, int32_t fmt, const int32_t* gaps, int32_t gap_cap, void* out,
                           int64_t out_capacity, int64_t* offsets, void* stream, const float* level) {
  ST2_REQUIRE(gap_cap >= 0, "%s: gap_cap=%d must not be negative", who, gap_cap);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(gaps) % 4 == 0, "%s: gaps is not aligned to int32", who);
  if (!taps) {  // this entry's own words for what the plain move cannot do
    ST2_REQUIRE(up == 1 && down == 1, "%s: without taps the rows are moved as they are: up=%d / down=%d must be 1", who, up, down);
    ST2_REQUIRE(fmt == ST2_PCM_F32 || fmt == ST2_PCM_S16,
                "%s: format %d needs the resampling move (taps); without taps fp32 and 16-bit PCM only", who, fmt);
  }
  return pack_plan(who, pack_args{wave, w_bs, frames, B, T_cap, samples_per_frame, trim, up, down, taps, taps_per_phase, fmt, gaps,
                                  gap_cap, out, out_capacity, offsets, stream, level});
}

extern "C" int st2_wave_pack_gaps(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                  int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                                  int32_t taps_per_phase, int32_t fmt, const int32_t* gaps, int32_t gap_cap, void* out,
                                  int64_t out_capacity, int64_t* offsets, void* stream) {
  return pack_gaps_entry("st2_wave_pack_gaps", wave, w_bs, frames, B, T_cap, samples_per_frame, trim, up, down, taps, taps_per_phase,
                         fmt, gaps, gap_cap, out, out_capacity, offsets, stream, nullptr);
}

// st2_wave_pack_level: st2_wave_pack_gaps whose moves multiply every input sample of row b by level[b][2],
// the gain st2_wave_level (st2_level.hip) wrote there; level == NULL: st2_wave_pack_gaps itself.
extern "C" int st2_wave_pack_level(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                   int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                                   int32_t taps_per_phase, int32_t fmt, const int32_t* gaps, int32_t gap_cap, void* out,
                                   int64_t out_capacity, int64_t* offsets, void* stream, const float* level) {
  return pack_gaps_entry("st2_wave_pack_level", wave, w_bs, frames, B, T_cap, samples_per_frame, trim, up, down, taps, taps_per_phase,
                         fmt, gaps, gap_cap, out, out_capacity, offsets, stream, level);
}
