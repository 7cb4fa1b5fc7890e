// st2_wave_dynamics (st2.h, added under ABI 23): a speech compressor in the hand-over, behind the breaks
// and in front of the level measurement.  The decoder has made the whole row before the hand-over starts, so nothing here is a
// recurrence: the envelope with instant attack and a release that is linear in dB is a prefix maximum of c[m] + m rho, which is
// exactly associative, and the attack is a zero-phase hold-and-smooth look-ahead as the limiter's (st2_limit.hip).  Everything
// between the block sums and the gain runs on the 64-sample grid of st2_wave_breaks.  Three launches, no atomics, no allocation,
// no synchronisation, no host read: legal under stream capture.  Grids are sized by the capacity, the work by `frames`.
//
// Launch 1, one workgroup per (tile of BR_TILE samples, row): the block sums of st2_blocksums.h, the kernel st2_wave_breaks
//   launches: one read of the valid samples.
// Launch 2, one workgroup per row, fp64: K = ceil(n_b / 64) blocks are walked in chunks of DY_CHUNK with 2 A blocks of halo
//   each side in LDS.  Per chunk: the detector and the static curve, z = c + k rho; the prefix maximum by wave scans, 256
//   blocks at a time, with the carry of what lies in front (the carry of the NEXT chunk's span is kept on the way: the 4 A
//   blocks two spans share are made twice, and a maximum gives the same bits both times); g = P - k rho; the hold by doubling
//   -- pass s makes the maxima over 2 s blocks from those over s --; the smoother's chain, neighbouring lanes on neighbouring
//   LDS words, the window word at a wave-uniform address; the gain, rounded once.  The row's maximum and count are folded at
//   the end, by shuffles and four LDS words.
// Launch 3, one workgroup per (tile of DY_TILE samples, row): the 66 gains the tile can need go to LDS; a lane's 4-sample vector
//   lies in one half of one block, so it needs two of them, at addresses nearly every lane of a wave shares (a broadcast, no
//   bank conflict); 16-byte loads and stores wherever the row allows, sample by sample where a vector touches the row's end.
//   A row that is left alone is moved as 32-bit words.
#include <cfloat>
#include <cmath>
#include <initializer_list>

#include "st2_blocksums.h"

namespace {

constexpr int DY_THREADS = 256;
constexpr int DY_VEC = 4;                                // 4-sample vectors of a lane of launch 3, DY_THREADS apart
constexpr int DY_TILE = DY_THREADS * 4 * DY_VEC;         // samples of a workgroup of launch 3
constexpr int DY_GAINS = DY_TILE / BR_BLOCK + 2;         // the tile's blocks and one neighbour each side
constexpr int DY_CHUNK = 1024;                           // blocks of a chunk of launch 2
constexpr int DY_MAX_A = 64;
constexpr int DY_SPAN = DY_CHUNK + 4 * DY_MAX_A;         // a chunk and 2 A blocks each side, at most
static_assert(DY_CHUNK % DY_THREADS == 0 && DY_GAINS <= DY_THREADS, "whole passes; one gain per lane");

struct __attribute__((packed, aligned(4))) dy_u32x4 {
  uint32_t v[4];
};

// A row's four parameters as the kernels read them: clamped, in fp64; `alone` where the row is left as it is
struct dy_row {
  bool alone;
  double T, slope, knee, makeup;
};

__device__ __forceinline__ dy_row dy_params(const float* __restrict__ p) {
  const float T = p[0], sl = p[1], kn = p[2], mk = p[3];
  dy_row r;
  r.alone = !(fabsf(T) <= FLT_MAX) || sl != sl || kn != kn || mk != mk;  // a NaN anywhere, or a threshold that is not finite
  r.T = (double)T;
  r.slope = (double)fminf(fmaxf(sl, 0.0f), 1.0f);
  r.knee = (double)fminf(fmaxf(kn, 0.0f), 40.0f);
  r.makeup = (double)fminf(fmaxf(mk, -24.0f), 24.0f);
  return r;
}

// Rules 3 and 4 for block k of a row of K blocks: the level of the three block sums around it, through the static curve
__device__ __forceinline__ double dy_curve(const float* __restrict__ s, int k, int K, const dy_row& r) {
  const float sm = k > 0 ? fminf(s[k - 1], FLT_MAX) : 0.0f, s0 = fminf(s[k], FLT_MAX), sp = k + 1 < K ? fminf(s[k + 1], FLT_MAX) : 0.0f;
  const float E = fminf((sm + s0) + sp, FLT_MAX);
  if (!(E > 0.0f)) return 0.0;  // L = -inf lies under every threshold
  const double o = 10.0 * log10((double)E / 192.0) - r.T;
  if (2.0 * o <= -r.knee) return 0.0;
  if (fabs(2.0 * o) < r.knee) {
    const double u = o + r.knee / 2.0;
    return (r.slope * (u * u)) / (2.0 * r.knee);
  }
  return r.slope * o;
}

__device__ __forceinline__ double dy_wave_scan_max(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double u = __shfl_up(v, off, 64);
    if ((int)(threadIdx.x & 63) >= off) v = fmax(v, u);
  }
  return v;
}

__global__ __launch_bounds__(DY_THREADS) void dynamics_row_kernel(const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                  const float* __restrict__ params, const float* __restrict__ sums,
                                                                  float* __restrict__ lin, int kcap, const float* __restrict__ win,
                                                                  int A, double rho, float* __restrict__ dyn) {
  __shared__ double G[DY_SPAN];  // g over the span; block k0 - 2 A + i at [i], -inf outside the row
  __shared__ double X[DY_SPAN], Y[DY_SPAN];
  __shared__ double wtot[DY_THREADS / 64], keep, red_mx[DY_THREADS / 64];
  __shared__ int red_ct[DY_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const dy_row r = dy_params(params + 4 * (int64_t)b);
  if (r.alone || n == 0) {
    if (tid == 0) dyn[2 * b] = dyn[2 * b + 1] = 0.0f;
    return;
  }
  const int K = (int)((n + BR_BLOCK - 1) / BR_BLOCK);
  const int S = DY_CHUNK + 4 * A, w = 2 * A + 1;
  const float* __restrict__ s = sums + (int64_t)b * kcap;
  float* __restrict__ lo = lin + (int64_t)b * kcap;
  double carry = -INFINITY;  // P in front of the span
  double mx = 0.0;
  int cnt = 0;
  for (int k0 = 0; k0 < K; k0 += DY_CHUNK) {
    const int kstart = k0 - 2 * A;
    for (int i = tid; i < S; i += DY_THREADS) {  // rule 5's z: one multiply, one add
      const int k = kstart + i;
      X[i] = k >= 0 && k < K ? dy_curve(s, k, K, r) + (double)k * rho : -INFINITY;
    }
    __syncthreads();
    for (int seg = 0; seg < S; seg += DY_THREADS) {  // the prefix maximum, DY_THREADS blocks at a time
      const int i = seg + tid, k = kstart + i;
      double v = dy_wave_scan_max(i < S ? X[i] : -INFINITY);
      if (lane == 63) wtot[wave] = v;
      __syncthreads();
      double total = carry;
#pragma unroll
      for (int u = 0; u < DY_THREADS / 64; ++u) {
        if (u == wave) v = fmax(v, total);
        total = fmax(total, wtot[u]);
      }
      if (i < S) G[i] = k >= 0 && k < K ? v - (double)k * rho : -INFINITY;
      if (i == DY_CHUNK - 1) keep = v;  // P in front of the next chunk's span
      carry = total;
      __syncthreads();
    }
    carry = keep;
    // rule 6's hold: cur[i] = max G[i .. i + p) where that lies inside the span; an entry whose run leaves it is never read
    const double* cur = G;
    double* a = X;
    double* o = Y;
    int p = 1;
    for (; 2 * p <= w; p *= 2) {
      for (int i = tid; i < S; i += DY_THREADS) a[i] = i + p < S ? fmax(cur[i], cur[i + p]) : cur[i];
      __syncthreads();
      cur = a;
      double* t = a; a = o; o = t;
    }
    // the window of 2 A + 1 from two runs of p (p <= w < 2 p): M[i] = m[k0 - A + i], i in [0, DY_CHUNK + 2 A)
    double* M = a;
    for (int i = tid; i < DY_CHUNK + 2 * A; i += DY_THREADS) M[i] = fmax(cur[i], cur[i + w - p]);
    __syncthreads();
    for (int kk = tid; kk < DY_CHUNK && k0 + kk < K; kk += DY_THREADS) {
      const int k = k0 + kk;
      double d = M[kk];  // A = 0: the hold is g and there is no window
      if (A > 0) {
        d = 0.0;
        for (int j = 0; j < w; ++j) d = d + (double)win[j] * M[min(max(k - A + j, 0), K - 1) - k0 + A];
      }
      const double dp = fmax(d, G[kk + 2 * A]);
      lo[k] = (float)pow(10.0, (r.makeup - dp) / 20.0);
      mx = fmax(mx, dp);
      cnt += dp > 0.0 ? 1 : 0;
    }
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, off, 64));
    cnt += __shfl_xor(cnt, off, 64);
  }
  if (lane == 0) {
    red_mx[wave] = mx;
    red_ct[wave] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int u = 1; u < DY_THREADS / 64; ++u) {
      mx = fmax(mx, red_mx[u]);
      cnt += red_ct[u];
    }
    dyn[2 * b] = (float)mx;
    dyn[2 * b + 1] = (float)cnt;
  }
}

__global__ __launch_bounds__(DY_THREADS) void dynamics_apply_kernel(const float* __restrict__ wave, int64_t w_bs,
                                                                    const int32_t* __restrict__ frames, int T_cap, int spf, int trim,
                                                                    const float* __restrict__ params, const float* __restrict__ lin,
                                                                    int kcap, float* __restrict__ out, int64_t o_bs) {
  __shared__ float sl[DY_GAINS];  // sl[j] = lin[clamp(t0 / 64 - 1 + j, 0, K - 1)]
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long n = pack_row_samples(frames, b, T_cap, spf, trim);
  const long long t0 = (long long)blockIdx.x * DY_TILE;
  if (t0 >= n) return;  // behind the row's end: the grid is sized by the capacity
  const float* __restrict__ src = wave + (int64_t)b * w_bs;
  float* __restrict__ dst = out + (int64_t)b * o_bs;
  if (dy_params(params + 4 * (int64_t)b).alone) {  // left alone: the valid samples' bits, NaN payloads as they are
    const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int v = 0; v < DY_VEC; ++v) {
      const long long i = t0 + 4LL * (v * DY_THREADS + tid);
      if (i >= n) break;
      if (i + 4 <= n) {
        *reinterpret_cast<dy_u32x4*>(d32 + i) = *reinterpret_cast<const dy_u32x4*>(s32 + i);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < n) d32[i + e] = s32[i + e];
      }
    }
    return;
  }
  const int K = (int)((n + BR_BLOCK - 1) / BR_BLOCK);
  const int kf = (int)(t0 / BR_BLOCK) - 1;
  if (tid < DY_GAINS) sl[tid] = lin[(int64_t)b * kcap + min(max(kf + tid, 0), K - 1)];
  __syncthreads();
  float x[DY_VEC][4];
#pragma unroll
  for (int v = 0; v < DY_VEC; ++v) {
    const long long i = t0 + 4LL * (v * DY_THREADS + tid);
    if (i >= n) break;
    if (i + 4 <= n) {
      const float4 q = load_f32x4(src + i);
      x[v][0] = q.x; x[v][1] = q.y; x[v][2] = q.z; x[v][3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[v][e] = i + e < n ? src[i + e] : 0.0f;
    }
  }
#pragma unroll
  for (int v = 0; v < DY_VEC; ++v) {
    const long long i = t0 + 4LL * (v * DY_THREADS + tid);
    if (i >= n) break;
    // the four samples lie in one half of block i / 64: between the centres of blocks ka and ka + 1
    const int ka = (int)(i >> 6) - ((i & 63) < 32 ? 1 : 0);
    const float la = sl[ka - kf], dl = sl[ka + 1 - kf] - la;
    const int m = 2 * (int)(i - 64LL * ka) - 63;  // t = m / 128, exact: 1 <= m <= 127
    f32x4_u y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y.v[e] = x[v][e] * fmaf((float)(m + 2 * e) * 0.0078125f, dl, la);
    if (i + 4 <= n) {
      *reinterpret_cast<f32x4_u*>(dst + i) = y;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e < n) dst[i + e] = y.v[e];
    }
  }
}

// Blocks of a row at capacity
int64_t dynamics_blocks(int64_t row) { return (row + BR_BLOCK - 1) / BR_BLOCK; }

}  // namespace

extern "C" int32_t st2_wave_dynamics_tile(void) { return DY_TILE; }
extern "C" int32_t st2_wave_dynamics_chunk(void) { return DY_CHUNK; }

// lin fp32 [B][Kcap] | s fp32 [B][Kcap]
extern "C" int64_t st2_wave_dynamics_workspace_bytes(int32_t B, int32_t T_cap, int32_t samples_per_frame) {
  if (B <= 0 || T_cap <= 0 || samples_per_frame <= 0) return 0;
  return (2 * (int64_t)B * dynamics_blocks((int64_t)samples_per_frame * T_cap) * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int st2_wave_dynamics(const float* wave, int64_t w_bs, const int32_t* frames, int32_t B, int32_t T_cap,
                                 int32_t samples_per_frame, int32_t trim, const float* params, int32_t A, const float* win,
                                 double rho, float* out, int64_t o_bs, float* dyn, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const char* who = "st2_wave_dynamics";
  ST2_REQUIRE(wave && frames, "%s: wave / frames is NULL", who);
  ST2_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && samples_per_frame > 0, "%s: bad geometry (B=%d, T_cap=%d, samples_per_frame=%d)",
              who, B, T_cap, samples_per_frame);
  ST2_REQUIRE(trim >= 0, "%s: trim=%d must not be negative", who, trim);
  const int64_t row = (int64_t)samples_per_frame * T_cap;
  ST2_REQUIRE(row <= INT32_MAX - DY_TILE, "%s: a row of %lld samples is too long for the int32 counts", who, (long long)row);
  ST2_REQUIRE(B == 1 || w_bs >= row, "%s: w_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)w_bs,
              (long long)row);
  ST2_REQUIRE(B == 1 || o_bs >= row, "%s: o_bs=%lld is less than the %lld samples of a row at capacity", who, (long long)o_bs,
              (long long)row);
  ST2_REQUIRE(params && out && dyn && workspace, "%s: params / out / dyn / workspace is NULL", who);
  ST2_REQUIRE(A >= 0 && A <= DY_MAX_A, "%s: A=%d is outside 0..%d", who, A, DY_MAX_A);
  ST2_REQUIRE(A == 0 || win, "%s: win is NULL with A=%d", who, A);
  ST2_REQUIRE(std::isfinite(rho) && rho > 0.0, "%s: rho=%g must be finite and positive", who, rho);
  for (const void* p : {(const void*)wave, (const void*)params, (const void*)win, (const void*)out, (const void*)dyn,
                        (const void*)workspace})
    ST2_REQUIRE(reinterpret_cast<uintptr_t>(p) % 4 == 0, "%s: wave / params / win / out / dyn / workspace is not aligned to float", who);
  ST2_REQUIRE(reinterpret_cast<uintptr_t>(frames) % 4 == 0, "%s: frames is not aligned to int32", who);
  // floats from the first sample of row 0 to the last of row B - 1, of either buffer
  const int64_t w_extent = (int64_t)(B - 1) * w_bs + row, o_extent = (int64_t)(B - 1) * o_bs + row;
  ST2_REQUIRE(out + o_extent <= wave || wave + w_extent <= out, "%s: out aliases wave", who);
  const int64_t need = st2_wave_dynamics_workspace_bytes(B, T_cap, samples_per_frame);
  ST2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld are needed", who, (long long)workspace_bytes,
              (long long)need);

  const int kcap = (int)dynamics_blocks(row);
  float* lin = reinterpret_cast<float*>(workspace);
  float* sums = lin + (int64_t)B * kcap;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(breaks_sums_kernel, dim3(st2_cdiv(row, BR_TILE), B), dim3(BR_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, sums, kcap, kcap);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(dynamics_row_kernel, dim3(B), dim3(DY_THREADS), 0, s, frames, T_cap, samples_per_frame, trim, params, sums, lin,
                     kcap, A > 0 ? win : nullptr, A, rho, dyn);
  ST2_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(dynamics_apply_kernel, dim3(st2_cdiv(row, DY_TILE), B), dim3(DY_THREADS), 0, s, wave, w_bs, frames, T_cap,
                     samples_per_frame, trim, params, lin, kcap, out, o_bs);
  ST2_CHECK_LAUNCH(who);
  return 0;
}
