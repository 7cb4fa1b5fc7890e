// st2_wave_resample_pack (st2.h, added under ABI 23): the packing step of the sync-free path with a
// rational polyphase resampler in it.  Every row's valid samples are read once at the model rate and written back to back at
// the rate and in the sample format a client asked for -- fp32, 16-bit PCM or G.711 mu-law / A-law -- with no host read and no
// allocation, so the call is legal under stream capture.
#include "st2_polyphase.h"

namespace {

constexpr int RS_THREADS = PP_THREADS;
constexpr int RS_TILE_BYTES = RS_THREADS * 16;  // a tile of output: one 16-byte store per lane
// Static LDS, 63 KiB: [phase table U x K | the tile's input span | the tile's converted output + one vector of head room]
constexpr int RS_LDS_FLOATS = 16128;
constexpr int RS_OUT_FLOATS = (RS_TILE_BYTES + 16) / 4;

// Workgroup (t, b) makes the output samples [j0, j1) of row b: tile 0 starts at the row's first sample and ends `tile` samples
// behind the first 16-byte boundary of the destination, every later tile starts and ends on such a boundary (`tile` samples
// are a whole number of 16-byte vectors).  Three phases with a barrier between them:
//   1. the phase table and the tile's input span [c(j0) - h, c(j1 - 1) - h + K) go to LDS (st2_polyphase.h);
//   2. lane l makes the samples j0 + l, j0 + l + 256, ... by the chain of st2_polyphase.h, converts and puts each where it
//      lies in the destination's 16-byte grid;
//   3. every 16-byte vector that lies wholly inside [j0, j1) leaves with one store per lane; the vector the row's start cuts
//      (tile 0) and the one its end cuts (the last tile) are peeled sample by sample.
// A workgroup whose tile lies behind the row's end -- or behind the write bound -- leaves before any barrier: the grid is sized
// by the capacity, the work by the frames.
template <int FMT>
__global__ __launch_bounds__(RS_THREADS) void wave_resample_pack_kernel(
    const float* __restrict__ wave, int64_t w_bs, const int32_t* __restrict__ frames, int B, int T_cap, int spf, int trim, int U,
    int D, const float* __restrict__ taps, int K, int tile, typename pcm_fmt<FMT>::type* __restrict__ out, long long out_capacity,
    const long long* __restrict__ offsets, const float* __restrict__ level) {
  using OUT = typename pcm_fmt<FMT>::type;
  constexpr int V = 16 / (int)sizeof(OUT);
  __shared__ __attribute__((aligned(16))) float lds[RS_LDS_FLOATS];
  const int b = blockIdx.y;
  const long long off = offsets[b];
  const long long limit = min(offsets[B], out_capacity);  // nothing at or past it is written
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long m = min((n * U + D - 1) / D, max(limit - off, 0LL));
  OUT* __restrict__ dst = out + off;
  const int mis = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
  const long long head = min(m, (long long)(((16 - mis) & 15) / (int)sizeof(OUT)));
  const long long j0 = blockIdx.x == 0 ? 0 : head + (long long)blockIdx.x * tile;
  if (j0 >= m) return;
  const long long j1 = min(m, head + ((long long)blockIdx.x + 1) * tile);
  const int len = (int)(j1 - j0);  // <= tile + head
  const pp_tile tg = pp_tile_of(j0, len, U, D, K);

  float* __restrict__ tab = lds;
  float* __restrict__ xs = lds + pp_round4(U * K);
  unsigned char* __restrict__ ys = reinterpret_cast<unsigned char*>(lds + (RS_LDS_FLOATS - RS_OUT_FLOATS));
  // -- 1. stage
  pp_stage_table(tab, taps, U * K);
  pp_stage_span<ST2_PCM_F32>(xs, wave + (int64_t)b * w_bs, n, tg, pack_row_gain(level, b));
  __syncthreads();
  // -- 2. filter and convert
  const int mis0 = blockIdx.x == 0 ? mis : 0;  // where sample j0 lies in its 16-byte vector of the destination
  OUT* __restrict__ yo = reinterpret_cast<OUT*>(ys + mis0);
  for (int jj = threadIdx.x; jj < len; jj += RS_THREADS) yo[jj] = pcm_encode<FMT>(pp_chain(tab, xs, tg, jj, U, D, K));
  __syncthreads();
  // -- 3. store
  const int end = mis0 + len * (int)sizeof(OUT);  // bytes of the 16-byte grid this tile covers: [mis0, end)
  unsigned char* __restrict__ g = reinterpret_cast<unsigned char*>(dst + j0) - mis0;  // 16-byte aligned
  for (int q = threadIdx.x; 16 * q < end; q += RS_THREADS) {
    if (16 * q >= mis0 && 16 * q + 16 <= end) {
      *reinterpret_cast<uint4*>(g + 16 * q) = *reinterpret_cast<const uint4*>(ys + 16 * q);
    } else {
#pragma unroll
      for (int r = 0; r < V; ++r) {
        const int at = 16 * q + r * (int)sizeof(OUT);
        if (at >= mis0 && at < end) *reinterpret_cast<OUT*>(g + at) = *reinterpret_cast<const OUT*>(ys + at);
      }
    }
  }
}

}  // namespace

int pack_resample_tile(const char* who, const pack_args& a, int* tile_out) {
  // the largest tile (a whole number of 16-byte vectors, at most one per lane) whose input span -- with a head of less than 16
  // samples in front of tile 0 -- fits beside the table
  const int room = RS_LDS_FLOATS - RS_OUT_FLOATS - pp_round4(a.up * a.taps_per_phase);
  int tile = RS_TILE_BYTES / pcm_sample_bytes(a.fmt);
  while (tile >= 16 && pp_round4((int)pp_span_cap(tile + 16, a.up, a.down, a.taps_per_phase)) > room) tile /= 2;
  ST2_REQUIRE(tile >= 16, "%s: a table of %d x %d taps at ratio %d / %d does not fit the %d bytes of LDS", who, a.up,
              a.taps_per_phase, a.up, a.down, RS_LDS_FLOATS * 4);
  const int64_t m_cap = ((int64_t)a.samples_per_frame * a.T_cap * a.up + a.down - 1) / a.down;
  ST2_REQUIRE(st2_cdiv(m_cap, tile) <= 0x7fffffff / 2, "%s: a row of %lld output samples is too long", who, (long long)m_cap);
  *tile_out = tile;
  return 0;
}

int pack_resample_move(const char* who, const pack_args& a, int tile) {
  const int64_t m_cap = ((int64_t)a.samples_per_frame * a.T_cap * a.up + a.down - 1) / a.down;
  const int gx = st2_cdiv(m_cap, tile);
  pcm_dispatch(a.fmt, [&](auto f) {
    hipLaunchKernelGGL((wave_resample_pack_kernel<f()>), dim3(gx, a.B), dim3(RS_THREADS), 0, reinterpret_cast<hipStream_t>(a.stream),
                       a.wave, a.w_bs, a.frames, a.B, a.T_cap, a.samples_per_frame, a.trim, a.up, a.down, a.taps, a.taps_per_phase,
                       tile, reinterpret_cast<typename pcm_fmt<f()>::type*>(a.out), (long long)a.out_capacity,
                       reinterpret_cast<const long long*>(a.offsets), a.level);
  });
  ST2_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int st2_wave_resample_pack(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                      int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                                      int32_t taps_per_phase, int32_t fmt, void* out, int64_t out_capacity, int64_t* offsets,
                                      void* stream) {
  const char* who = "st2_wave_resample_pack";
  ST2_REQUIRE(taps, "%s: wave / frames / taps / out / offsets is NULL", who);  // to the plan, no taps would mean the plain move
  return pack_plan(who, pack_args{wave, w_bs, frames, B, T_cap, samples_per_frame, trim, up, down, taps, taps_per_phase, fmt, nullptr,
                                  0, out, out_capacity, offsets, stream});
}
