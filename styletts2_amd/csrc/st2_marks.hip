// Timing marks and per-token prosody controls (st2.h, added under ABI 23).  Both rest on one device
// primitive: row b's token boundaries in decoder frames, under exactly the rule expand_by_durations_kernel (st2_glue.hip)
// gathers by.  st2_token_marks turns the boundaries into sample positions of the packed stream; st2_prosody_controls_tok
// looks a frame's token up by them and applies that token's pitch scale / energy shift to the prosody predictor's curves.
// (The third token control, the duration head with a per-token rate, is an instantiation of duration_head_kernel in
// st2_glue.hip.)
#include "st2_common.h"
#include "st2_tokens.h"

namespace {

// One wave per row.  bound[n] = the first frame of token n (st2.h "the boundary rule"), marks[n] = the first output sample at
// or after that frame's time in the row's packed samples.  EDGES (st2_token_marks_edges): the row was cut to the `count` samples
// from `head` on (st2_wave_edges) before it was packed, and a boundary's sample is clamp(s - head, 0, count) of them.
template <bool EDGES>
__global__ __launch_bounds__(64) void token_marks_kernel(const long long* __restrict__ dur, int N, const int32_t* __restrict__ len,
                                                         const int32_t* __restrict__ frames, int T_cap, int shift, int spf, int trim,
                                                         int U, int D, int32_t* __restrict__ marks, int32_t* __restrict__ bound_out,
                                                         const int32_t* __restrict__ edges) {
  __shared__ int cum[512];
  const int b = blockIdx.x;
  const int n_b = len ? min(max(len[b], 0), N) : N;
  const int T_b = frames ? min(max(frames[b], 0), T_cap) : T_cap;
  scan_durations(dur + (int64_t)b * N, N, n_b, T_cap, cum);
  __syncthreads();
  const long long n_smp = max(0LL, (long long)spf * T_b - trim);
  for (int n = threadIdx.x; n <= N; n += 64) {
    int bound;
    if (n == 0) bound = 0;
    else if (n == N) bound = T_b;
    else {
      const int c = cum[n - 1];
      bound = min(T_b, c == 0 ? 0 : c + (shift ? 1 : 0));
    }
    long long s = min((long long)spf * bound, n_smp);
    if constexpr (EDGES) s = min(max(s - edges[2 * b], 0LL), (long long)max(edges[2 * b + 1], 0));
    marks[(int64_t)b * (N + 1) + n] = (int32_t)((s * U + D - 1) / D);
    if (bound_out) bound_out[(int64_t)b * (N + 1) + n] = bound;
  }
}

constexpr int TOK_THREADS = 256;
constexpr int TOK_COLS = 1024;  // columns of one workgroup: 512 frames, two per thread

// Workgroup (chunk, b) covers TOK_COLS columns of row b of BOTH curves, one FRAME (two adjacent columns) per thread and
// iteration: the frame's token is searched once.  One whose chunk lies at or past the row's end (2 T_b) leaves at once, before
// the scan.  One operation per element: a multiply for F0, an add for N (x itself where the shift is 0).
__global__ __launch_bounds__(TOK_THREADS) void prosody_controls_tok_kernel(float* __restrict__ f0, float* __restrict__ n, int64_t bs,
                                                                           int T, const long long* __restrict__ dur, int N,
                                                                           int shift, const float* __restrict__ tok_f0_scale,
                                                                           const float* __restrict__ tok_n_shift,
                                                                           const int32_t* __restrict__ frames) {
  __shared__ int cum[512];
  const int b = blockIdx.y;
  const int T_b = frames ? min(max(frames[b], 0), T) : T;
  const int t0 = blockIdx.x * (TOK_COLS / 2);
  if (t0 >= T_b) return;
  if (threadIdx.x < 64) scan_durations(dur + (int64_t)b * N, N, N, T, cum);
  __syncthreads();
  float* __restrict__ fr = f0 + (int64_t)b * bs;
  float* __restrict__ nr = n + (int64_t)b * bs;
  const float* __restrict__ scr = tok_f0_scale ? tok_f0_scale + (int64_t)b * N : nullptr;
  const float* __restrict__ shr = tok_n_shift ? tok_n_shift + (int64_t)b * N : nullptr;
#pragma unroll
  for (int it = 0; it < TOK_COLS / 2 / TOK_THREADS; ++it) {
    const int t = t0 + it * TOK_THREADS + (int)threadIdx.x;
    if (t >= T_b) break;
    const int idx = token_of_frame(cum, N, t, shift);
    const int l = 2 * t;
    if (scr) {
      const float v = scr[idx];
      const float sc = v != v ? 1.0f : fminf(fmaxf(v, 0.5f), 2.0f);
      fr[l] = fr[l] * sc;
      fr[l + 1] = fr[l + 1] * sc;
    }
    if (shr) {
      const float v = shr[idx];
      const float sh = v != v ? 0.0f : fminf(fmaxf(v, -2.0f), 2.0f);
      const float x0 = nr[l], x1 = nr[l + 1];
      nr[l] = sh == 0.0f ? x0 : x0 + sh;
      nr[l + 1] = sh == 0.0f ? x1 : x1 + sh;
    }
  }
}

}  // namespace

extern "C" int st2_sizeof_token_controls(void) { return (int)sizeof(st2_token_controls); }

// Both entries: every refusal under the entry's name `who`, then the one launch.  edges == NULL: st2_token_marks.
static int marks_plan(const char* who, const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* frames,
                      int32_t T_cap, int32_t shift, int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, int32_t* marks,
                      int32_t* bound_out, const int32_t* edges, void* stream) {
  ST2_REQUIRE(dur && marks, "%s: dur / marks is NULL", who);
  ST2_REQUIRE(B > 0 && N > 0 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, N=%d, T_cap=%d, samples_per_frame=%d)", who,
              B, N, T_cap, samples_per_frame);
  ST2_REQUIRE(N <= 512, "%s: N=%d tokens exceed the 512 of PL-BERT's position table", who, N);
  ST2_REQUIRE(up >= 1 && up <= 1024 && down >= 1 && down <= 1024, "%s: up=%d / down=%d must lie in 1..1024", who, up, down);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  // ceil(spf T_cap U / D) <= INT32_MAX  <=>  spf T_cap <= floor(INT32_MAX D / U)
  ST2_REQUIRE((int64_t)samples_per_frame * T_cap <= (int64_t)INT32_MAX * down / up,
              "%s: a row at capacity (%d frames of %d samples at %d / %d) does not fit the int32 marks", who, T_cap, samples_per_frame,
              up, down);
  auto kernel = edges ? token_marks_kernel<true> : token_marks_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(dur), N,
                     len, frames, T_cap, shift ? 1 : 0, samples_per_frame, trim, up, down, marks, bound_out, edges);
  ST2_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int st2_token_marks(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* frames, int32_t T_cap,
                               int32_t shift, int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down, int32_t* marks,
                               int32_t* bound_out, void* stream) {
  return marks_plan("st2_token_marks", dur, B, N, len, frames, T_cap, shift, samples_per_frame, trim, up, down, marks, bound_out,
                    nullptr, stream);
}

// st2_token_marks_edges (st2.h): the marks of rows that st2_wave_edges cut, relative to the cut row
extern "C" int st2_token_marks_edges(const int64_t* dur, int32_t B, int32_t N, const int32_t* len, const int32_t* frames,
                                     int32_t T_cap, int32_t shift, int32_t samples_per_frame, int32_t trim, int32_t up, int32_t down,
                                     int32_t* marks, int32_t* bound_out, const int32_t* edges, void* stream) {
  ST2_REQUIRE(edges && reinterpret_cast<uintptr_t>(edges) % 4 == 0, "st2_token_marks_edges: edges is NULL or not aligned to int32");
  return marks_plan("st2_token_marks_edges", dur, B, N, len, frames, T_cap, shift, samples_per_frame, trim, up, down, marks,
                    bound_out, edges, stream);
}

extern "C" int st2_prosody_controls_tok(float* f0, float* n, int64_t bs, int32_t B, int32_t L, const int64_t* dur, int32_t N,
                                        int32_t shift, const float* tok_f0_scale, const float* tok_n_shift, const int32_t* frames,
                                        void* stream) {
  ST2_REQUIRE(f0 && n && dur, "st2_prosody_controls_tok: f0 / n / dur is NULL");
  ST2_REQUIRE(B > 0 && B <= 65535 && L > 0 && L % 2 == 0 && N > 0 && (B == 1 || bs >= L),
              "st2_prosody_controls_tok: bad geometry (B=%d, L=%d, N=%d, bs=%lld)", B, L, N, (long long)bs);
  ST2_REQUIRE(N <= 512, "st2_prosody_controls_tok: N=%d tokens exceed the 512 of PL-BERT's position table", N);
  if (!tok_f0_scale && !tok_n_shift) return 0;  // nothing to apply: no launch
  hipLaunchKernelGGL(prosody_controls_tok_kernel, dim3(st2_cdiv(L, TOK_COLS), B), dim3(TOK_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), f0, n, bs, L / 2, reinterpret_cast<const long long*>(dur), N,
                     shift ? 1 : 0, tok_f0_scale, tok_n_shift, frames);
  ST2_CHECK_LAUNCH("st2_prosody_controls_tok");
  return 0;
}
