// st2_wave_resample_pack (st2.h, added under ABI 23): the packing step of the sync-free path with a
// rational polyphase resampler in it.  Every row's valid samples are read once at the model rate and written back to back at
// the rate and in the sample format a client asked for -- fp32, 16-bit PCM or G.711 mu-law / A-law -- with no host read and no
// allocation, so the call is legal under stream capture.
#include "st2_common.h"
#include "st2_pcm.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE_BYTES = RS_THREADS * 16;  // a tile of output: one 16-byte store per lane
// Static LDS, 63 KiB: [phase table U x K | the tile's input span | the tile's converted output + one vector of head room]
constexpr int RS_LDS_FLOATS = 16128;
constexpr int RS_OUT_FLOATS = (RS_TILE_BYTES + 16) / 4;

__host__ __device__ constexpr int rs_round4(int v) { return (v + 3) & ~3; }
// Upper bound of the input span (in floats, from its 4-sample-aligned start) of a tile of `tile` + head (< 16) output samples
__host__ __device__ constexpr long long rs_span_cap(long long tile, int U, int D, int K) { return (tile + 16) * D / U + K + 8; }

template <int FMT> struct rs_out { using type = float; };
template <> struct rs_out<ST2_PCM_S16> { using type = int16_t; };
template <> struct rs_out<ST2_PCM_ULAW> { using type = uint8_t; };
template <> struct rs_out<ST2_PCM_ALAW> { using type = uint8_t; };

template <int FMT>
__device__ __forceinline__ typename rs_out<FMT>::type rs_cvt(float y) {
  if constexpr (FMT == ST2_PCM_F32) return y;
  else if constexpr (FMT == ST2_PCM_S16) return pcm16(y);
  else if constexpr (FMT == ST2_PCM_ULAW) return g711_ulaw(pcm16(y));
  else return g711_alaw(pcm16(y));
}

// m_b = ceil(n_b U / D) output samples
__device__ __forceinline__ long long rs_row_samples(const int32_t* __restrict__ frames, int b, int T_cap, int spf, int trim,
                                                    int U, int D) {
  return (pack_row_samples(frames, b, T_cap, spf, trim) * U + D - 1) / D;
}

__global__ __launch_bounds__(64) void resample_offsets_kernel(const int32_t* __restrict__ frames, int B, int T_cap, int spf,
                                                              int trim, int U, int D, long long* __restrict__ offsets) {
  pack_scan_rows(B, offsets, [&](int b) { return rs_row_samples(frames, b, T_cap, spf, trim, U, D); });
}

// Workgroup (t, b) makes the output samples [j0, j1) of row b: tile 0 starts at the row's first sample and ends `tile` samples
// behind the first 16-byte boundary of the destination, every later tile starts and ends on such a boundary (`tile` samples
// are a whole number of 16-byte vectors).  Three phases with a barrier between them:
//   1. the phase table and the tile's input span [c(j0) - h, c(j1 - 1) - h + K) go to LDS with 16-byte loads; a sample in
//      front of the row or at / past n_b is a SELECTED zero -- nothing of `wave` at or past n_b is read;
//   2. lane l makes the samples j0 + l, j0 + l + 256, ...: y = sum_k taps[p][k] x[c - h + k] in fp32, fmaf, k ascending (the
//      same chain wherever the tile boundaries fall), converts and puts the sample where it lies in the destination's 16-byte
//      grid;
//   3. every 16-byte vector that lies wholly inside [j0, j1) leaves with one store per lane; the vector the row's start cuts
//      (tile 0) and the one its end cuts (the last tile) are peeled sample by sample.
// A workgroup whose tile lies behind the row's end -- or behind the write bound -- leaves before any barrier: the grid is sized
// by the capacity, the work by the frames.
template <int FMT>
__global__ __launch_bounds__(RS_THREADS) void wave_resample_pack_kernel(
    const float* __restrict__ wave, int64_t w_bs, const int32_t* __restrict__ frames, int B, int T_cap, int spf, int trim, int U,
    int D, const float* __restrict__ taps, int K, int tile, typename rs_out<FMT>::type* __restrict__ out, long long out_capacity,
    const long long* __restrict__ offsets) {
  using OUT = typename rs_out<FMT>::type;
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
  const int h = (K - 1) / 2;
  const long long c0 = j0 * D / U;
  const unsigned p0 = (unsigned)(j0 * D - c0 * U);
  const long long i_lo = c0 - h;
  const long long i_hi = c0 + ((long long)p0 + (long long)(len - 1) * D) / U - h + K - 1;  // the last input sample of the tile
  const long long a0 = i_lo & ~3LL;  // floor to a multiple of 4, also for a negative start
  const int n4 = (int)((i_hi - a0) / 4 + 1);

  float* __restrict__ tab = lds;
  float* __restrict__ xs = lds + rs_round4(U * K);
  unsigned char* __restrict__ ys = reinterpret_cast<unsigned char*>(lds + (RS_LDS_FLOATS - RS_OUT_FLOATS));
  // -- 1. stage
  const int nt = U * K;
  for (int q = threadIdx.x; 4 * q + 4 <= nt; q += RS_THREADS) {
    const f32x4_u a = *reinterpret_cast<const f32x4_u*>(taps + 4 * q);
    *reinterpret_cast<float4*>(tab + 4 * q) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  }
  if ((int)threadIdx.x < (nt & 3)) tab[(nt & ~3) + threadIdx.x] = taps[(nt & ~3) + threadIdx.x];
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  for (int q = threadIdx.x; q < n4; q += RS_THREADS) {
    const long long i = a0 + 4LL * q;
    float4 x;
    if (i >= 0 && i + 4 <= n) {
      const f32x4_u a = *reinterpret_cast<const f32x4_u*>(src + i);
      x = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    } else {  // an edge of the row: every sample on its own, loaded only where it is valid
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = 0.0f;
        if (i + r >= 0 && i + r < n) e[r] = src[i + r];
      }
      x = make_float4(e[0], e[1], e[2], e[3]);
    }
    *reinterpret_cast<float4*>(xs + 4 * q) = x;
  }
  __syncthreads();
  // -- 2. filter and convert
  const int mis0 = blockIdx.x == 0 ? mis : 0;  // where sample j0 lies in its 16-byte vector of the destination
  const float* __restrict__ x0 = xs + (int)(i_lo - a0);
  OUT* __restrict__ yo = reinterpret_cast<OUT*>(ys + mis0);
  for (int jj = threadIdx.x; jj < len; jj += RS_THREADS) {
    const unsigned t = p0 + (unsigned)jj * (unsigned)D;  // < 2^23: jj <= 4111, D <= 1024
    const unsigned c = t / (unsigned)U;
    const float* __restrict__ tp = tab + (t - c * (unsigned)U) * K;
    const float* __restrict__ xp = x0 + c;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) acc = fmaf(tp[k], xp[k], acc);
    yo[jj] = rs_cvt<FMT>(acc);
  }
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

template <int FMT>
void launch_resample(int gx, int B, hipStream_t s, const float* wave, int64_t w_bs, const int32_t* frames, int T_cap, int spf,
                     int trim, int U, int D, const float* taps, int K, int tile, void* out, long long cap, const long long* offs) {
  hipLaunchKernelGGL((wave_resample_pack_kernel<FMT>), dim3(gx, B), dim3(RS_THREADS), 0, s, wave, w_bs, frames, B, T_cap, spf,
                     trim, U, D, taps, K, tile, reinterpret_cast<typename rs_out<FMT>::type*>(out), cap, offs);
}

}  // namespace

extern "C" int st2_wave_resample_pack(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                      int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, const float* taps,
                                      int32_t taps_per_phase, int32_t fmt, void* out, int64_t out_capacity, int64_t* offsets,
                                      void* stream) {
  ST2_REQUIRE(wave && frames && out && offsets && taps, "st2_wave_resample_pack: wave / frames / taps / out / offsets is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0,
              "st2_wave_resample_pack: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)", B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0 && out_capacity >= 0, "st2_wave_resample_pack: trim=%d / out_capacity=%lld must not be negative", trim,
              (long long)out_capacity);
  ST2_REQUIRE(up >= 1 && up <= 1024 && down >= 1 && down <= 1024, "st2_wave_resample_pack: bad ratio %d / %d (each 1..1024)", up,
              down);
  ST2_REQUIRE(taps_per_phase >= 1 && taps_per_phase <= 512, "st2_wave_resample_pack: taps_per_phase=%d is outside 1..512",
              taps_per_phase);
  ST2_REQUIRE(fmt == ST2_PCM_F32 || fmt == ST2_PCM_S16 || fmt == ST2_PCM_ULAW || fmt == ST2_PCM_ALAW,
              "st2_wave_resample_pack: unknown format %d", fmt);
  const int size = fmt == ST2_PCM_F32 ? 4 : (fmt == ST2_PCM_S16 ? 2 : 1);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(out) % size == 0 && reinterpret_cast<uintptr_t>(wave) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(taps) % 4 == 0,
              "st2_wave_resample_pack: wave / taps / out is not aligned to its sample type");
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(B == 1 || w_bs >= row, "st2_wave_resample_pack: w_bs=%lld is less than the %lld samples of a row at capacity",
              (long long)w_bs, (long long)row);
  // the largest tile (a whole number of 16-byte vectors, at most one per lane) whose input span fits beside the table
  const int room = RS_LDS_FLOATS - RS_OUT_FLOATS - rs_round4(up * taps_per_phase);
  int tile = RS_TILE_BYTES / size;
  while (tile >= 16 && rs_round4((int)rs_span_cap(tile, up, down, taps_per_phase)) > room) tile /= 2;
  ST2_REQUIRE(tile >= 16, "st2_wave_resample_pack: a table of %d x %d taps at ratio %d / %d does not fit the %d bytes of LDS", up,
              taps_per_phase, up, down, RS_LDS_FLOATS * 4);
  const int64_t m_cap = (row * up + down - 1) / down;
  ST2_REQUIRE(st2_cdiv(m_cap, tile) <= 0x7fffffff / 2, "st2_wave_resample_pack: a row of %lld output samples is too long",
              (long long)m_cap);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  long long* offs = reinterpret_cast<long long*>(offsets);
  hipLaunchKernelGGL(resample_offsets_kernel, dim3(1), dim3(64), 0, s, frames, B, T_cap, samples_per_frame, trim, up, down, offs);
  ST2_CHECK_LAUNCH("st2_wave_resample_pack (offsets)");
  const int gx = st2_cdiv(m_cap, tile);
  auto go = fmt == ST2_PCM_F32 ? launch_resample<ST2_PCM_F32>
            : fmt == ST2_PCM_S16 ? launch_resample<ST2_PCM_S16>
            : fmt == ST2_PCM_ULAW ? launch_resample<ST2_PCM_ULAW> : launch_resample<ST2_PCM_ALAW>;
  go(gx, B, s, wave, w_bs, frames, T_cap, samples_per_frame, trim, up, down, taps, taps_per_phase, tile, out,
     (long long)out_capacity, offs);
  ST2_CHECK_LAUNCH("st2_wave_resample_pack");
  return 0;
}
