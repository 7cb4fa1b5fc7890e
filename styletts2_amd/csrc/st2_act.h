// Activation / split helpers of the conv epilogues and the ONE definition of the split-f16 prologue: st2_act_split
// (st2_actsplit.hip), the one-role fused conv (st2_conv1d_f16s_impl.h) and its warp-specialised build (st2_conv1d_f16s_ws.h) all
// call st2_prologue / st2_split_f16 below.  Device code, gfx950.
#pragma once
#include "st2_common.h"
#include <type_traits>

typedef _Float16 st2_h8 __attribute__((ext_vector_type(8)));

static __device__ __forceinline__ float leaky(float v, float slope) { return v >= 0.f ? v : v * slope; }

// Largest finite f16 magnitude; operands of the split-f16 convs are clamped to it before the hi cast.  One v_med3_f32 (the
// compare / select form costs four VALU instructions and two VCC wait states per element of a prologue that is VALU-bound:
// DESIGN.md section 3 iv); finite values map exactly as before, a NaN operand becomes -65504 -- like an overflow it differs
// from the clamped value, so the caller's `clamped != value` test reports it through ST2_STATUS_F16_RANGE.
static __device__ __forceinline__ float st2_clamp_f16(float u) { return __builtin_amdgcn_fmed3f(u, -65504.f, 65504.f); }

// ---- the split-f16 prologue, stated once (DESIGN.md "The split-f16 prologue, stated once") ---------------------------------------
// Every function below is a template over the value type T: float (one channel) or st2_f2 (two adjacent channels as packed-f32
// ops: the one-role fused conv's 32-row layout).  Same IEEE operations in the same order per component, so the instantiations are
// bitwise each other.  Plain encodings and low-half broadcasts only (tools/check_isa.py: an op_sel on a packed-f32 op would be
// the gfx950 hazard of DESIGN.md section 9).
typedef float st2_f2 __attribute__((ext_vector_type(2)));

template <class T>
static __device__ __forceinline__ T st2_splat(float c) {
  if constexpr (std::is_same_v<T, float>) return c;
  else return T{c, c};
}

// s = sin(r) for x = n * pi + r: n = rint(x/pi), r = x - n*pi (two-term, fma-exact), odd minimax polynomial of degree 9 on
// [-pi/2, pi/2] (max abs error 1.2e-7, fitted in tools/fit_sin.py); sin(x) = (-1)^n s
template <class T>
static __device__ __forceinline__ T st2_sin_reduced(T x, T& n) {
  n = __builtin_elementwise_rint(x * st2_splat<T>(0.3183098861837907f));
  T r = __builtin_elementwise_fma(n, st2_splat<T>(-3.1415927410125732f), x);
  r = __builtin_elementwise_fma(n, st2_splat<T>(8.742277657347586e-08f), r);
  const T r2 = r * r;
  T p = st2_splat<T>(2.6000539037340786e-06f);
  p = __builtin_elementwise_fma(p, r2, st2_splat<T>(-0.00019806614727713168f));
  p = __builtin_elementwise_fma(p, r2, st2_splat<T>(0.008333017118275166f));
  p = __builtin_elementwise_fma(p, r2, st2_splat<T>(-0.16666656732559204f));
  return __builtin_elementwise_fma(r2 * r, p, r);
}

// sin(x)^2 to ~2.4e-7 absolute
template <class T>
static __device__ __forceinline__ T sin_sq(T x) {
  T n;
  const T s = st2_sin_reduced(x, n);
  return s * s;
}

// sin(x) to 1.2e-7 absolute (sign restored from the parity of n)
static __device__ __forceinline__ float sin_acc(float x) {
  float n;
  const float s = st2_sin_reduced(x, n);
  return ((int)n & 1) ? -s : s;
}

template <class T>
static __device__ __forceinline__ T snake(T v, T alpha, T inv_alpha) {
  return v + inv_alpha * sin_sq(alpha * v);  // x + (1/a) * sin(a*x)^2, Modules/istftnet.py:69
}

// Per input channel (T = float: 32 B) or per pair of adjacent channels (T = st2_f2: 64 B, the same 32 B per channel); xs = x_scale,
// 0 for the channel tail of the last chunk.  ST2_CHAN_PAR_FILL is the entry of a channel past C_in.
template <class T>
struct st2_chan_par {
  T mean, rstd, g, beta, alpha, inv_alpha, xs, pad1;
};
#define ST2_CHAN_PAR_FILL {0.f, 1.f, 1.f, 0.f, 1.f, 1.f, 0.f, 0.f}

// Affine + activation of prologue PRO on v.  AdaIN: mean / rstd / g = 1 + gamma / beta per channel; COLNORM: g / beta per channel,
// statistics (cmean, crstd) per POSITION -- they stay scalar in the packed form: splatting crstd, the HIGH element of the (mean,
// rstd) pair its load returns, would be an op_sel'd packed op (tools/check_isa.py).  The operand scale, the zero padding AFTER the
// activation (as F.conv1d pads the activated tensor) and the split follow in the caller.
// Its two halves are callable on their own: st2_act_split, whose parameters are scalar loads, requests alpha between them.
template <int PRO, class T>
static __device__ __forceinline__ T st2_pro_affine(T v, const st2_chan_par<T>& par, float cmean, float crstd) {
  if constexpr (st2_pro_is_adain(PRO)) {
    const T u = (v - par.mean) * par.rstd;
    return par.g * u + par.beta;
  } else if constexpr (PRO == ST2_PRO_COLNORM) {
    T u;
    if constexpr (std::is_same_v<T, float>) u = (v - cmean) * crstd;
    else u = T{(v.x - cmean) * crstd, (v.y - cmean) * crstd};
    return u * par.g + par.beta;
  } else {
    return v;
  }
}
template <int PRO, class T>
static __device__ __forceinline__ T st2_pro_activation(T v, const st2_chan_par<T>& par, float slope) {
  if constexpr (st2_pro_has_snake(PRO)) {
    return snake(v, par.alpha, par.inv_alpha);
  } else if constexpr (!st2_pro_has_leaky(PRO)) {
    return v;
  } else if constexpr (std::is_same_v<T, float>) {
    return leaky(v, slope);
  } else {
    return T{leaky(v.x, slope), leaky(v.y, slope)};
  }
}
template <int PRO, class T>
static __device__ __forceinline__ T st2_prologue(T v, const st2_chan_par<T>& par, float slope, float cmean, float crstd) {
  return st2_pro_activation<PRO>(st2_pro_affine<PRO>(v, par, cmean, crstd), par, slope);
}

// Element e of a slot: w -> hi[e] + lo[e], saturated to the f16 range instead of overflowing to inf (hi) / NaN (lo = w - inf), so
// the conv stays finite.  `sat` collects whether any w was out of range (so is a NaN operand, which becomes -65504): the caller
// reports it as ST2_STATUS_F16_RANGE.  (It writes the elements and the flag in place, in the order the kernels always did: returning
// them moves the vector inserts and the flag's OR, and the compiler's packing of the surrounding f32 ops with them.)
static __device__ __forceinline__ void st2_split_f16(float w, st2_h8& hi, st2_h8& lo, int e, bool& sat) {
  const float vc = st2_clamp_f16(w);
  sat |= vc != w;
  const _Float16 h = (_Float16)vc;
  hi[e] = h;
  lo[e] = (_Float16)(vc - (float)h);
}

// Run-time prologue -> compile-time tag: f(std::integral_constant<int, PRO>{})
template <class F>
static __host__ __device__ __forceinline__ void st2_dispatch_pro(int pro, F&& f) {
  switch (pro) {
    case ST2_PRO_LEAKY: f(std::integral_constant<int, ST2_PRO_LEAKY>{}); break;
    case ST2_PRO_ADAIN_LEAKY: f(std::integral_constant<int, ST2_PRO_ADAIN_LEAKY>{}); break;
    case ST2_PRO_ADAIN_SNAKE: f(std::integral_constant<int, ST2_PRO_ADAIN_SNAKE>{}); break;
    case ST2_PRO_SNAKE: f(std::integral_constant<int, ST2_PRO_SNAKE>{}); break;
    case ST2_PRO_COLNORM: f(std::integral_constant<int, ST2_PRO_COLNORM>{}); break;
    default: f(std::integral_constant<int, ST2_PRO_NONE>{}); break;
  }
}

static __device__ __forceinline__ float gelu_erf(float v) {
  return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
}


// HF "gelu_new" (tanh approximation), the ALBERT FFN activation
static __device__ __forceinline__ float gelu_tanh(float v) {
  return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * (v * v * v))));
}
