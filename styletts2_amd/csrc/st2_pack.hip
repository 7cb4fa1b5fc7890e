// Sync-free synthesis (st2.h, added under ABI 23): the frame counts of a batch from its durations, on the device, and the
// valid samples of a ragged batch of waveforms packed into one contiguous fp32 / 16-bit PCM buffer.  With these two the host
// never reads a predicted duration: it states a frame capacity, and frame counts travel as a device int32 [B] from the
// duration head to the samples a server copies out.
#include "st2_common.h"
#include "st2_pcm.h"

namespace {

// frames[b] = clamp(sum_{n < len[b]} dur[b][n], 1, T_cap); one wave per row (N <= 512: at most 8 durations per lane), 64-bit sum
// so that no caller-supplied duration can wrap it.
__global__ __launch_bounds__(64) void frames_from_durations_kernel(const long long* __restrict__ dur, int N,
                                                                   const int32_t* __restrict__ len, int T_cap,
                                                                   int32_t* __restrict__ frames, int* status) {
  const int b = blockIdx.x;
  const int n_b = len ? min(max(len[b], 0), N) : N;
  const long long* db = dur + (int64_t)b * N;
  long long acc = 0;
  for (int n = threadIdx.x; n < n_b; n += 64) acc += db[n];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) {
    if (acc > T_cap) st2_raise_status(status, ST2_STATUS_FRAME_CAPACITY);  // the row is synthesised truncated to T_cap frames
    frames[b] = (int32_t)min(max(acc, 1LL), (long long)T_cap);
  }
}

constexpr int PACK_THREADS = 256;
constexpr int PACK_ITERS = 4;  // 16-byte stores per lane and workgroup

// Workgroup (chunk, b) moves PACK_THREADS * PACK_ITERS 16-byte vectors of row b's ALIGNED body (V samples each: 8 x int16 or
// 4 x fp32); chunk 0 also moves the row's head (the samples in front of the first 16-byte boundary of the destination) and its
// tail (what is left behind the last whole vector), both shorter than one vector.  A workgroup whose chunk lies behind the
// row's end leaves at once: the grid is sized by the capacity, the work by the frames.
template <typename OUT, int V>
__global__ __launch_bounds__(PACK_THREADS) void wave_pack_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                 const int32_t* __restrict__ frames, int B, int T_cap, int spf,
                                                                 int trim, OUT* __restrict__ out, long long out_capacity,
                                                                 const long long* __restrict__ offsets,
                                                                 const float* __restrict__ level) {
  static_assert(V * sizeof(OUT) == 16, "one vector = one 16-byte store");
  const int b = blockIdx.y;
  const long long off = offsets[b];
  const long long limit = min(offsets[B], out_capacity);  // nothing at or past it is written
  const long long n = min(pack_row_samples(frames, b, T_cap, spf, trim), max(limit - off, 0LL));
  if (n <= 0) return;
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  OUT* __restrict__ dst = out + off;
  const row_gain gain = pack_row_gain(level, b);
  const long long head = min(n, (long long)((16 - (int)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / (long long)sizeof(OUT));
  const long long nvec = (n - head) / V;
  const long long v0 = (long long)blockIdx.x * (PACK_THREADS * PACK_ITERS);
  if (v0 >= nvec && blockIdx.x != 0) return;
#pragma unroll
  for (int it = 0; it < PACK_ITERS; ++it) {
    const long long v = v0 + it * PACK_THREADS + threadIdx.x;
    if (v >= nvec) break;
    const long long i = head + v * V;
    if constexpr (V == 4) {
      const float4 a = gain(load_f32x4(src + i));
      uint4 o;
      o.x = __float_as_uint(a.x); o.y = __float_as_uint(a.y); o.z = __float_as_uint(a.z); o.w = __float_as_uint(a.w);
      *reinterpret_cast<uint4*>(dst + i) = o;
    } else {
      const float4 a = gain(load_f32x4(src + i)), c = gain(load_f32x4(src + i + 4));
      auto two = [](float lo, float hi) { return (uint32_t)(uint16_t)pcm16(lo) | ((uint32_t)(uint16_t)pcm16(hi) << 16); };
      uint4 o;
      o.x = two(a.x, a.y); o.y = two(a.z, a.w); o.z = two(c.x, c.y); o.w = two(c.z, c.w);
      *reinterpret_cast<uint4*>(dst + i) = o;
    }
  }
  if (blockIdx.x == 0) {
    const long long t0 = head + nvec * V;  // head < V and n - t0 < V: one lane per sample
    long long i = -1;
    if ((long long)threadIdx.x < head) i = threadIdx.x;
    else if (threadIdx.x >= 64 && t0 + (threadIdx.x - 64) < n) i = t0 + (threadIdx.x - 64);
    if (i >= 0) {
      if constexpr (V == 4) dst[i] = gain(src[i]); else dst[i] = pcm16(gain(src[i]));
    }
  }
}

}  // namespace

extern "C" int st2_frames_from_durations(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, int32_t T_cap,
                                         int32_t* frames, void* stream) {
  ST2_REQUIRE(dur && frames, "st2_frames_from_durations: dur / frames is NULL");
  ST2_REQUIRE(B > 0 && N > 0 && T_cap > 0, "st2_frames_from_durations: bad geometry (B=%d, N=%d, T_cap=%d)", B, N, T_cap);
  ST2_REQUIRE(N <= 512, "st2_frames_from_durations: N=%d tokens exceed the 512 of PL-BERT's position table", N);
  hipLaunchKernelGGL(frames_from_durations_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(dur), N, len, T_cap, frames, st2_status_device_ptr());
  ST2_CHECK_LAUNCH("st2_frames_from_durations");
  return 0;
}

int pack_move(const char* who, const pack_args& a) {
  const int64_t row = (int64_t)a.samples_per_frame * a.T_cap;
  hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
  const long long* offs = reinterpret_cast<const long long*>(a.offsets);
  if (a.fmt == ST2_PCM_S16) {
    const int gx = st2_cdiv(st2_cdiv(row, 8), PACK_THREADS * PACK_ITERS);
    hipLaunchKernelGGL((wave_pack_kernel<int16_t, 8>), dim3(gx, a.B), dim3(PACK_THREADS), 0, s, a.wave, a.w_bs, a.frames, a.B,
                       a.T_cap, a.samples_per_frame, a.trim, reinterpret_cast<int16_t*>(a.out), (long long)a.out_capacity, offs,
                       a.level);
  } else {
    const int gx = st2_cdiv(st2_cdiv(row, 4), PACK_THREADS * PACK_ITERS);
    hipLaunchKernelGGL((wave_pack_kernel<float, 4>), dim3(gx, a.B), dim3(PACK_THREADS), 0, s, a.wave, a.w_bs, a.frames, a.B,
                       a.T_cap, a.samples_per_frame, a.trim, reinterpret_cast<float*>(a.out), (long long)a.out_capacity, offs,
                       a.level);
  }
  ST2_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int st2_wave_pack(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                             int32_t samples_per_frame, int32_t trim, int32_t fmt, void* out, int64_t out_capacity,
                             int64_t* offsets, void* stream) {
  return pack_plan("st2_wave_pack", pack_args{wave, w_bs, frames, B, T_cap, samples_per_frame, trim, 1, 1, nullptr, 0, fmt, nullptr,
                                              0, out, out_capacity, offsets, stream});
}
