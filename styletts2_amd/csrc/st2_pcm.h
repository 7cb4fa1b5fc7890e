// What the packing entry points and the clip ingest share (st2_pack.hip: st2_wave_pack; st2_resample.hip:
// st2_wave_resample_pack; st2_passage.hip: st2_wave_pack_gaps and the pack plan; st2_ingest.hip: st2_clip_ingest): a row's
// sample counts, the pack plan's arguments, the packed source vectors, the sample conversions, both ways, and the sample
// formats' types, size and dispatch.  The polyphase rule of the two
// resamplers is st2_polyphase.h.
#pragma once
#include <type_traits>
#include "st2_common.h"

// n_b = max(0, spf * clamp(frames[b], 0, T_cap) - trim): the row's valid samples at the model rate
__device__ __forceinline__ long long pack_row_samples(const int32_t* __restrict__ frames, int b, int T_cap, int spf, int trim) {
  const long long f = min(max(frames[b], 0), T_cap);  // clamped to the capacity: never a read past the row
  return max(0LL, f * spf - trim);
}

// m_b = (n_b U + D - 1) div D: the row's samples at the output rate U / D of the model's, in 64 bits (U = D = 1: n_b itself)
__device__ __forceinline__ long long pack_row_out_samples(const int32_t* __restrict__ frames, int b, int T_cap, int spf, int trim,
                                                          int U, int D) {
  return (pack_row_samples(frames, b, T_cap, spf, trim) * U + D - 1) / D;
}

// What the level measurement reads for a sample (st2_level.hip; st2_polyphase.h's cleaning option): a non-finite one counts as 0
__device__ __forceinline__ float finite_or_zero(float x) { return fabsf(x) <= 3.402823466e38f ? x : 0.0f; }  // NaN: false

// The per-row gain of st2_wave_pack_level (st2_level.hip): g_b = level[b][2], read once per workgroup and
// multiplied into every input sample as it is loaded, before anything else a move does.  level == NULL: no multiply at all --
// not one by 1.0f, which would quieten the NaN payloads the fp32 bit copy hands on -- and the move is the one it always was.
struct row_gain {
  bool on;
  float g;
  __device__ __forceinline__ float operator()(float x) const { return on ? x * g : x; }
  __device__ __forceinline__ float4 operator()(float4 x) const {
    return on ? make_float4(x.x * g, x.y * g, x.z * g, x.w * g) : x;
  }
};
__device__ __forceinline__ row_gain pack_row_gain(const float* __restrict__ level, int b) {
  return level ? row_gain{true, level[4 * b + 2]} : row_gain{false, 1.0f};
}

// The source of a row's aligned body starts wherever the destination's alignment puts it: 4-byte aligned only.
struct __attribute__((packed, aligned(4))) f32x4_u {
  float v[4];
};
// Four 16-bit / 8-bit samples of a client's clip: a row starts wherever its sample type may.
struct __attribute__((packed, aligned(2))) s16x4_u {
  int16_t v[4];
};
struct __attribute__((packed, aligned(1))) u8x4_u {
  uint8_t v[4];
};

__device__ __forceinline__ int16_t pcm16(float x) {
  // (int16) rint(clamp(x, -1, 1) * 32767): v_rndne = round-to-nearest-even as np.rint; NaN -> 0 (fminf / fmaxf would turn
  // it into a full-scale sample)
  const float c = fminf(fmaxf(x, -1.0f), 1.0f);
  return x != x ? (int16_t)0 : (int16_t)(int)rintf(c * 32767.0f);
}

// ITU-T G.711 of a 16-bit sample, by the segment rule of the standard's reference code (G.191): the magnitude of a negative
// sample is its one's complement; mu-law keeps 14 bits, adds the bias 33 and clips at 0x1FFF, A-law keeps 13 bits.
__device__ __forceinline__ uint8_t g711_ulaw(int s) {
  const int a = min(((s < 0 ? ~s : s) >> 2) + 33, 0x1FFF);  // 33..8191: the leading one sits at bit 5..12
  const int seg = 26 - __clz(a);
  const int code = ((seg << 4) | ((a >> (seg + 1)) & 15)) ^ 0x7F;
  return (uint8_t)(s < 0 ? code : code | 0x80);
}

__device__ __forceinline__ uint8_t g711_alaw(int s) {
  int ix = (s < 0 ? ~s : s) >> 4;  // 0..2047
  if (ix > 15) {
    const int e = 28 - __clz(ix);  // 1..7: the leading one at bit e + 3
    ix = (ix >> (e - 1)) - 16 + (e << 4);
  }
  return (uint8_t)((s < 0 ? ix : ix | 0x80) ^ 0x55);
}

// The way back, ITU-T G.711 expansion to the 16-bit value at the centre of the code's interval: mu-law takes the bias off again
// (the two zero codes 0xFF / 0x7F both give 0), A-law's smallest magnitudes are +-8.
__device__ __forceinline__ int g711_ulaw_decode(int code) {
  const int inv = ~code & 0xFF;
  const int lin = ((((inv & 15) << 3) + 0x84) << ((inv >> 4) & 7)) - 0x84;  // 0..32124
  return code < 0x80 ? -lin : lin;
}

__device__ __forceinline__ int g711_alaw_decode(int code) {
  const int ix = (code ^ 0x55) & 0x7F;
  const int e = ix >> 4;
  const int man = e > 0 ? (ix & 15) + 16 : (ix & 15);
  const int lin = ((man << 4) + 8) << (e > 0 ? e - 1 : 0);  // 8..32256
  return code > 127 ? lin : -lin;
}

// A sample format of st2.h as a type: what a sample is stored as, and four of them wherever a row of that type may start.
template <int FMT> struct pcm_fmt { using type = float; using vec = f32x4_u; };
template <> struct pcm_fmt<ST2_PCM_S16> { using type = int16_t; using vec = s16x4_u; };
template <> struct pcm_fmt<ST2_PCM_ULAW> { using type = uint8_t; using vec = u8x4_u; };
template <> struct pcm_fmt<ST2_PCM_ALAW> { using type = uint8_t; using vec = u8x4_u; };

template <int FMT>
__device__ __forceinline__ typename pcm_fmt<FMT>::type pcm_encode(float y) {
  if constexpr (FMT == ST2_PCM_F32) return y;
  else if constexpr (FMT == ST2_PCM_S16) return pcm16(y);
  else if constexpr (FMT == ST2_PCM_ULAW) return g711_ulaw(pcm16(y));
  else return g711_alaw(pcm16(y));
}

template <int FMT>
__device__ __forceinline__ float pcm_decode(typename pcm_fmt<FMT>::type v) {
  if constexpr (FMT == ST2_PCM_F32) return v;
  else if constexpr (FMT == ST2_PCM_S16) return (float)v * (1.0f / 32768.0f);  // exact
  else if constexpr (FMT == ST2_PCM_ULAW) return (float)g711_ulaw_decode(v) * (1.0f / 32768.0f);
  else return (float)g711_alaw_decode(v) * (1.0f / 32768.0f);
}

// Four samples at an address aligned to their type only, with one load, decoded
template <int FMT>
__device__ __forceinline__ float4 pcm_decode4(const typename pcm_fmt<FMT>::type* __restrict__ p) {
  const typename pcm_fmt<FMT>::vec a = *reinterpret_cast<const typename pcm_fmt<FMT>::vec*>(p);
  return make_float4(pcm_decode<FMT>(a.v[0]), pcm_decode<FMT>(a.v[1]), pcm_decode<FMT>(a.v[2]), pcm_decode<FMT>(a.v[3]));
}
__device__ __forceinline__ float4 load_f32x4(const float* __restrict__ p) { return pcm_decode4<ST2_PCM_F32>(p); }

// The pack plan (st2_passage.hip): what the three packing entries st2_wave_pack, st2_wave_resample_pack
// and st2_wave_pack_gaps receive, and the one function that serves them -- every refusal once (`who` names the entry in the
// message), then the row scan, the move, and the fill where there are gaps.  taps == NULL: the plain move (up = down = 1,
// fp32 / 16-bit PCM); gaps == NULL or gap_cap == 0: no fill; level == NULL (every entry but st2_wave_pack_level): no gain.
static_assert((int)ST2_PACK_F32 == (int)ST2_PCM_F32 && (int)ST2_PACK_S16 == (int)ST2_PCM_S16,
              "st2_wave_pack's format codes are the first two of st2_pcm_format: the code below tests ST2_PCM_* only");
struct pack_args {
  const float* wave;
  int64_t w_bs;
  const int32_t* frames;
  int32_t B, T_cap, samples_per_frame, trim, up, down;
  const float* taps;
  int32_t taps_per_phase, fmt;
  const int32_t* gaps;
  int32_t gap_cap;
  void* out;
  int64_t out_capacity;
  int64_t* offsets;
  void* stream;
  const float* level = nullptr;  // fp32 [B][4] of st2_wave_level: the moves multiply by level[b][2]
};
int pack_plan(const char* who, const pack_args& a);
// The move launch over offsets that the scan has written on the same stream, each beside its kernel (st2_pack.hip,
// st2_resample.hip), and the output tile the resampling move's LDS budget allows (a refusal when there is none).
int pack_move(const char* who, const pack_args& a);
int pack_resample_tile(const char* who, const pack_args& a, int* tile);
int pack_resample_move(const char* who, const pack_args& a, int tile);

inline int pcm_sample_bytes(int fmt) { return fmt == ST2_PCM_F32 ? 4 : (fmt == ST2_PCM_S16 ? 2 : 1); }

// f(std::integral_constant<int, FMT>) for a format code of st2.h (checked by the caller)
template <class F>
inline void pcm_dispatch(int fmt, F&& f) {
  switch (fmt) {
    case ST2_PCM_F32: return f(std::integral_constant<int, ST2_PCM_F32>{});
    case ST2_PCM_S16: return f(std::integral_constant<int, ST2_PCM_S16>{});
    case ST2_PCM_ULAW: return f(std::integral_constant<int, ST2_PCM_ULAW>{});
    default: return f(std::integral_constant<int, ST2_PCM_ALAW>{});
  }
}
