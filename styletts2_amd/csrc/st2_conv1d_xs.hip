// C entry points of the xs conv family; the kernels live in st2_conv1d_xs_impl.h and are instantiated in
// st2_conv1d_xs_k{0..3}.hip.  Also here: the per-launch timing hook of bench.py's roofline leg and the start-up
// autotuner that picks, per shape class and device, the fastest of the bitwise-equivalent builds of a launch.
#include "st2_conv1d_xs_impl.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

extern template int st2xs::launch_by_cout<1, 32>(const st2_conv_desc&, hipStream_t, int);
extern template int st2xs::launch_by_cout<2, 32>(const st2_conv_desc&, hipStream_t, int);
extern template int st2xs::launch_by_cout<3, 32>(const st2_conv_desc&, hipStream_t, int);
extern template int st2xs::launch_by_cout<5, 16>(const st2_conv_desc&, hipStream_t, int);
extern template int st2xs::launch_by_cout<7, 16>(const st2_conv_desc&, hipStream_t, int);
extern template int st2xs::launch_by_cout<11, 16>(const st2_conv_desc&, hipStream_t, int);

namespace {

int launch_xs(const st2_conv_desc& d, hipStream_t s, int variant) {
  switch (d.ks) {
    case 1:
      return st2xs::launch_by_cout<1, 32>(d, s, variant);
    case 2:
      return st2xs::launch_by_cout<2, 32>(d, s, variant);
    case 3:
      return st2xs::launch_by_cout<3, 32>(d, s, variant);
    case 5:
      return st2xs::launch_by_cout<5, 16>(d, s, variant);
    case 7:
      return st2xs::launch_by_cout<7, 16>(d, s, variant);
    case 11:
      return st2xs::launch_by_cout<11, 16>(d, s, variant);
    default:
      st2_set_error("st2_conv1d_xs: unsupported kernel size %d (have 1,2,3,5,7,11)", d.ks);
      return 1;
  }
}

// ---- measurement hook (bench.py's roofline leg) ---------------------------------------------------------------------
// HIP events around every st2_conv1d_xs launch, on the launch stream, whoever issues it (the C++ plans of st2_engine.hip
// or the Python per-kernel plans).  Process-wide and single-threaded by contract (st2.h), not legal under stream capture:
// enabled around the bench's timed region only.
struct TimedLaunch {
  int ks, c_in, c_out, L, B;
  hipEvent_t e0, e1;
};
std::vector<TimedLaunch> g_timed;
bool g_timing = false;

// ---- start-up autotuner ----------------------------------------------------------------------------------------------
// Key = (device, ks, C_in, C_out, L_out, B); value = the variant (st2xs::XS_V_* bits) that won the measurement.  Every
// candidate issues the same products in the same order and the same epilogue, so the choice changes time, never results.
typedef std::tuple<int, int, int, int, int, int> TuneKey;
struct TuneEntry {
  int chosen = st2xs::XS_V_RULE;
  int n = 0;
  int variant[8] = {};
  float ms[8] = {};
};
std::mutex g_tune_mu;     // the table
std::mutex g_measure_mu;  // one measurement at a time (they share g_scratch); never held together with a launch of another thread
std::map<TuneKey, TuneEntry> g_tune;
std::atomic<int> g_tune_entries{0};
std::atomic<int> g_tune_mode{0};
void* g_scratch = nullptr;  // candidate launches write here, never into the caller's output (it may alias a residual)
size_t g_scratch_bytes = 0;
int g_scratch_dev = -1;

int current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}

using st2xs::rule_variant;  // the build an untuned process runs (st2_conv1d_xs_impl.h)

std::vector<int> candidates(const st2_conv_desc& d) {
  std::vector<int> c;
  const int rule = rule_variant(d);
  c.push_back(rule);
  if (d.C_out <= 64 || d.ks == 1) return c;  // narrow tiles / token GEMMs: one build each
  // only launches of ~100 us or more are measured -- below that two event pairs of two launches do not resolve a 2 %
  // difference (single-utterance launches of the long-form loop read 0.02-0.1 ms for the same build) -- the rest follow the rule
  if (2.0 * d.B * d.C_in * (double)d.C_out * d.ks * d.L_out < 2e10) return c;
  const int64_t wg128 = (int64_t)st2_cdiv(d.L_out, 128) * st2_cdiv(d.C_out, 128) * d.B;
  const int ny = st2_cdiv(d.C_out, 128);
  const bool swz = (ny == 2 || ny == 4 || ny == 8);
  auto add = [&](int v) {
    for (int x : c)
      if (x == v) return;
    if ((v & st2xs::XS_V_SWIZZLE) && !swz) return;
    if (c.size() < 8) c.push_back(v);
  };
  if (d.ks >= 7) {
    add(0);
    if (wg128 >= 512) add(st2xs::XS_V_WIDE);
    add(st2xs::XS_V_SWIZZLE);
    if (wg128 >= 512) add(st2xs::XS_V_WIDE | st2xs::XS_V_SWIZZLE);
  } else {
    add(0);
    if (d.ks == 3 && wg128 >= 512 && d.L_out >= 512) add(st2xs::XS_V_WIDE);  // short rows waste the second half-tile
    add(st2xs::XS_V_SWIZZLE);
  }
  return c;
}

bool ensure_scratch(size_t bytes) {
  const int dev = current_device();
  if (g_scratch && g_scratch_dev == dev && g_scratch_bytes >= bytes) return true;
  if (g_scratch) (void)hipFree(g_scratch);
  g_scratch = nullptr;
  g_scratch_bytes = 0;
  if (hipMalloc(&g_scratch, bytes) != hipSuccess) {
    (void)hipGetLastError();
    g_scratch = nullptr;
    return false;
  }
  g_scratch_bytes = bytes;
  g_scratch_dev = dev;
  return true;
}

// Times every candidate build of this launch on the caller's stream (synchronously: tuning mode is a start-up phase) and
// returns the winner; the caller's tensors are only READ (outputs go to a scratch tensor of the same strides).
int tune_launch(const st2_conv_desc& d, hipStream_t s, TuneEntry& e) {
  const std::vector<int> cands = candidates(d);
  e.n = (int)cands.size();
  for (int i = 0; i < e.n; ++i) e.variant[i] = cands[i];
  e.chosen = cands[0];
  if (e.n < 2) return e.chosen;
  const size_t bytes = ((size_t)(d.B - 1) * d.y_bs + (size_t)(d.C_out - 1) * d.y_cs + d.L_out + 64) * sizeof(float);
  if (!ensure_scratch(bytes)) return e.chosen;  // no memory to measure in: the rule stands
  st2_conv_desc t = d;
  t.y = reinterpret_cast<float*>(g_scratch);
  // the caller's alignment class decides which epilogue build runs: keep it (hipMalloc returns >= 256-byte alignment)
  t.y += (reinterpret_cast<uintptr_t>(d.y) & 255) / sizeof(float);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return e.chosen;
  // Round-robin over the candidates, best group per candidate: a clock / power excursion of a few milliseconds (seen once
  // in ~25 bench runs: both builds of the dominant class read 17-24 % high and the slower one won, profiles/r04/r04ak_bench.json)
  // then hits every candidate alike or is dropped by the minimum, instead of landing on whichever build was being timed.
  constexpr int GROUPS = 3, PER = 2;
  bool ok[8];
  float best[8];
  for (int i = 0; i < e.n; ++i) {
    best[i] = 1e30f;
    ok[i] = launch_xs(t, s, cands[i]) == 0;  // warm-up: code object, LDS attribute, clocks
  }
  for (int g = 0; g < GROUPS; ++g) {
    for (int i = 0; i < e.n; ++i) {
      if (!ok[i]) continue;
      (void)hipEventRecord(e0, s);
      for (int r = 0; ok[i] && r < PER; ++r) ok[i] = launch_xs(t, s, cands[i]) == 0;
      (void)hipEventRecord(e1, s);
      float ms = 0.f;
      ok[i] = ok[i] && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
      if (ok[i] && ms / PER < best[i]) best[i] = ms / PER;
    }
  }
  for (int i = 0; i < e.n; ++i) e.ms[i] = ok[i] && best[i] < 1e29f ? best[i] : -1.f;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  // the rule's build (candidate 0) keeps the launch unless another one is at least 2 % faster
  int win = 0;
  for (int i = 1; i < e.n; ++i)
    if (e.ms[i] > 0.f && e.ms[win] > 0.f && e.ms[i] < e.ms[win] * (win == 0 ? 0.98f : 1.0f)) win = i;
  e.chosen = e.ms[win] > 0.f ? cands[win] : cands[0];
  return e.chosen;
}

int pick_variant(const st2_conv_desc& d, hipStream_t s) {
  if (!g_tune_mode.load(std::memory_order_relaxed) && !g_tune_entries.load(std::memory_order_relaxed))
    return st2xs::XS_V_RULE;
  const TuneKey key(current_device(), d.ks, d.C_in, d.C_out, d.L_out, d.B);
  {
    std::lock_guard<std::mutex> lock(g_tune_mu);
    auto it = g_tune.find(key);
    if (it != g_tune.end()) return it->second.chosen;  // incl. a class another thread is measuring right now: the rule
    if (!g_tune_mode.load(std::memory_order_relaxed)) return st2xs::XS_V_RULE;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return st2xs::XS_V_RULE;  // a capture cannot be timed: the class stays untuned for now
    }
    TuneEntry placeholder;  // chosen = XS_V_RULE, n = 0: "being measured"
    g_tune[key] = placeholder;
    g_tune_entries.store((int)g_tune.size(), std::memory_order_relaxed);
  }
  // The measurement itself (hipMalloc, 1 + 3 x 2 launches per candidate, event synchronisation) runs OUTSIDE the table lock
  // (advisor, round 4): other threads / devices keep launching, on the rule's build for this class until the result lands.
  TuneEntry e;
  {
    std::lock_guard<std::mutex> measuring(g_measure_mu);
    tune_launch(d, s, e);
  }
  std::lock_guard<std::mutex> lock(g_tune_mu);
  g_tune[key] = e;
  return e.chosen;
}

}  // namespace

extern "C" int st2_conv_timing(int enable) {
  if (enable) {
    for (auto& t : g_timed) {
      (void)hipEventDestroy(t.e0);
      (void)hipEventDestroy(t.e1);
    }
    g_timed.clear();
  }
  g_timing = enable != 0;
  return 0;
}

extern "C" int st2_conv_timing_read(double* rows, int32_t cap_rows) {
  ST2_REQUIRE(!g_timing, "st2_conv_timing_read: stop the recording first (st2_conv_timing(0))");
  int n = 0;
  for (auto& t : g_timed) {
    float ms = 0.f;
    if (hipEventSynchronize(t.e1) != hipSuccess || hipEventElapsedTime(&ms, t.e0, t.e1) != hipSuccess) {
      st2_set_error("st2_conv_timing_read: %s", hipGetErrorString(hipGetLastError()));
      return -1;
    }
    if (rows && n < cap_rows) {
      double* r = rows + (int64_t)n * 6;
      r[0] = t.ks; r[1] = t.c_in; r[2] = t.c_out; r[3] = t.L; r[4] = t.B; r[5] = ms;
    }
    ++n;
  }
  return n;
}

extern "C" int st2_conv_tune(int mode) {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  if (mode < 0) {  // forget every measurement of the current device
    const int dev = current_device();
    for (auto it = g_tune.begin(); it != g_tune.end();) it = std::get<0>(it->first) == dev ? g_tune.erase(it) : std::next(it);
    g_tune_entries.store((int)g_tune.size(), std::memory_order_relaxed);
    mode = 0;
  }
  g_tune_mode.store(mode != 0, std::memory_order_relaxed);
  if (!mode && g_scratch) {
    (void)hipFree(g_scratch);
    g_scratch = nullptr;
    g_scratch_bytes = 0;
  }
  return 0;
}

extern "C" int st2_conv_tune_set(int32_t ks, int32_t C_in, int32_t C_out, int32_t L_out, int32_t B, int32_t variant) {
  ST2_REQUIRE(variant >= -1 && variant < 4, "st2_conv_tune_set: variant %d out of range", variant);
  const TuneKey key(current_device(), ks, C_in, C_out, L_out, B);
  std::lock_guard<std::mutex> lock(g_tune_mu);
  if (variant < 0) {
    g_tune.erase(key);
  } else {
    TuneEntry e;
    e.chosen = variant;
    e.n = 1;
    e.variant[0] = variant;
    e.ms[0] = 0.f;
    g_tune[key] = e;
  }
  g_tune_entries.store((int)g_tune.size(), std::memory_order_relaxed);
  return 0;
}

extern "C" int st2_conv_tune_read(double* rows, int32_t cap_rows) {
  std::lock_guard<std::mutex> lock(g_tune_mu);
  const int dev = current_device();
  int n = 0;
  for (auto& kv : g_tune) {
    if (std::get<0>(kv.first) != dev) continue;
    if (rows && n < cap_rows) {
      double* r = rows + (int64_t)n * 24;
      r[0] = std::get<1>(kv.first); r[1] = std::get<2>(kv.first); r[2] = std::get<3>(kv.first);
      r[3] = std::get<4>(kv.first); r[4] = std::get<5>(kv.first); r[5] = dev;
      r[6] = kv.second.chosen; r[7] = kv.second.n;
      for (int i = 0; i < 8; ++i) {
        r[8 + 2 * i] = i < kv.second.n ? kv.second.variant[i] : -1;
        r[9 + 2 * i] = i < kv.second.n ? kv.second.ms[i] : 0.0;
      }
    }
    ++n;
  }
  return n;
}

extern "C" int st2_conv1d_xs_part_cols(const st2_conv_desc* dp) {
  return dp ? st2xs::small_grid_cols(*dp) : 128;
}

// The conv launch rule (st2.h st2_conv_launch_plan): the ONE statement of how a split-f16 conv is routed,
// scaled and sized.  conv() of the C++ plans and ops.conv1d of the Python plans both ask here.
constexpr int XS_HALO = 32;         // zero columns in front of every xs row (>= the largest pad_left on the path: 25)
constexpr int XS_MIN_L = 256;       // shorter rows stay on the fused kernel: an xs row is >= 640 slots
constexpr int XS_MIN_C_PLAIN = 64;  // prologue-free convs take the xs pair from this many input channels on (the split pass is
                                    // then cheap next to the conv; measured 39 us vs 80 us per denoiser Linear at B*N = 3200)
// Layers whose xs pair is HBM-bound take the fused kernel (prologue arithmetic on the VALU beside the MFMAs, no activation pass:
// 12 instead of 20 bytes per element): the narrow HiFi-GAN stages (C <= 64) and the k = 3 resblock convs at C = 128.  Measured
// per layer at B = 32 (tools/probe_conv.py, profiles/archive/r02/r02y_probe_conv_b32.log): fused / pair = 0.80-0.96 at C = 64,
// 0.86-0.91 at C = 32, 0.89-0.92 at C = 128 k = 3; 1.04-1.19 everywhere else.
constexpr int FUSED_MAX_C = 64, FUSED_K3_MAX_C = 128;

extern "C" int st2_conv_launch_plan(const st2_conv_desc* dp, int32_t want_stats, int32_t gb_seg, int32_t force_fused,
                                    st2_conv_plan* p) {
  ST2_REQUIRE(dp && p, "st2_conv_launch_plan: null descriptor or plan");
  const st2_conv_desc& d = *dp;
  const bool norm = st2_pro_needs_stats(d.pro);
  const bool prefer_fused = d.pro != ST2_PRO_NONE && (d.C_in <= FUSED_MAX_C || (d.ks <= 3 && d.C_in <= FUSED_K3_MAX_C));
  const bool xs = !force_fused && d.pad_left <= XS_HALO && d.L_in >= XS_MIN_L &&
                  (d.pro != ST2_PRO_NONE || d.C_in >= XS_MIN_C_PLAIN) && !prefer_fused;
  *p = st2_conv_plan{};
  p->route = xs ? ST2_CONV_ROUTE_XS : ST2_CONV_ROUTE_FUSED;
  p->prefer_fused = prefer_fused;
  p->x_scale = norm ? 8.0f : 1.0f;
  p->xs_cg = (d.C_in + 31) / 32 * 32 / 8;
  p->xs_lp = XS_HALO + (std::max(d.L_in, 1) + 1 + 511) / 512 * 512 + 96;
  p->xs_halo = XS_HALO;
  p->xs_min_l = XS_MIN_L;
  p->xs_bytes = (int64_t)d.B * 2 * p->xs_cg * p->xs_lp * 16;
  ST2_REQUIRE(xs || gb_seg <= 0, "st2_conv_launch_plan: a per-segment affine (gb_seg) exists on the st2_act_split + st2_conv1d_xs "
              "route only; this layer takes the fused kernel");
  if (want_stats) {  // one slot per 128 columns, or per 64 / 32-column tile of a small xs grid (one utterance)
    p->part_cols = xs ? st2_conv1d_xs_part_cols(dp) : 128;
    p->part_nt = st2_cdiv(d.L_out, p->part_cols);
    p->part_floats = (int64_t)d.B * d.C_out * p->part_nt * 3;  // (sum, sum of squares) per slot, then the slots' shifts
  } else if (!xs) {
    p->splitk_bytes = st2_conv1d_f16s_splitk_bytes(dp);  // skinny layers run split-K (this thread's st2_conv1d_f16s_split_as holds)
  }
  return 0;
}

extern "C" int st2_conv1d_xs(const st2_conv_desc* dp, void* stream) {
  ST2_REQUIRE(dp != nullptr, "st2_conv1d_xs: null descriptor");
  const st2_conv_desc& d = *dp;
  ST2_REQUIRE(d.B > 0 && d.C_in > 0 && d.C_out > 0 && d.L_out > 0,
              "st2_conv1d_xs: empty geometry B=%d C_in=%d C_out=%d L_out=%d", d.B, d.C_in, d.C_out, d.L_out);
  ST2_REQUIRE(d.xs && d.wq && d.y, "st2_conv1d_xs: null tensor pointer");
  ST2_REQUIRE((reinterpret_cast<uintptr_t>(d.wq) & 15) == 0 && (reinterpret_cast<uintptr_t>(d.xs) & 15) == 0,
              "st2_conv1d_xs: wq and xs must be 16-byte aligned");
  ST2_REQUIRE(d.dil >= 1 && d.dil <= 8, "st2_conv1d_xs: dil=%d out of range", d.dil);
  ST2_REQUIRE(d.pad_left >= 0 && d.pad_left <= d.xs_halo, "st2_conv1d_xs: pad_left=%d exceeds the xs halo %d",
              d.pad_left, d.xs_halo);
  ST2_REQUIRE(d.res_shift >= 0 && d.res_shift <= 1, "st2_conv1d_xs: res_shift must be 0 or 1");
  ST2_REQUIRE(d.out_scale > 0.f, "st2_conv1d_xs: out_scale must be set");
  ST2_REQUIRE(d.B <= 65535, "st2_conv1d_xs: grid too large");
  ST2_REQUIRE((int64_t)d.C_out * d.y_cs < (1ll << 31) && (!d.res || (int64_t)d.C_out * d.res_cs < (1ll << 31)) &&
                  (!d.res2 || (int64_t)d.C_out * d.res2_cs < (1ll << 31)),
              "st2_conv1d_xs: a batch item of y / res / res2 must span < 2^31 elements");
  if (d.part) ST2_REQUIRE((reinterpret_cast<uintptr_t>(d.part) & 7) == 0, "st2_conv1d_xs: part must be 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int variant = pick_variant(d, s);
  if (g_timing && d.C_in >= 64 && d.L_out >= 256 && g_timed.size() < 65536) {
    TimedLaunch t{d.ks, d.C_in, d.C_out, d.L_out, d.B, nullptr, nullptr};
    if (hipEventCreate(&t.e0) == hipSuccess && hipEventCreate(&t.e1) == hipSuccess) {
      (void)hipEventRecord(t.e0, s);
      const int rc = launch_xs(d, s, variant);
      (void)hipEventRecord(t.e1, s);
      g_timed.push_back(t);
      return rc;
    }
  }
  return launch_xs(d, s, variant);
}
