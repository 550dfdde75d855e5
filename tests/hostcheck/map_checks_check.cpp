// map_checks_check -- the refusals of the map's window calls that make no HIP call (visual-odometry_amd/csrc/map_checks.h: the
// frame check, the round-parameter check, the capture-growth refusal) under the host sanitizers, without a GPU and without
// the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_checks_check.cpp -o map_checks_check && ./map_checks_check      (ends with "map_checks_check: all ok")
// Every row names the code and the whole message the call must leave.  They were read off refine_check as it stood in capi.hip
// before the checks moved here (one function of fifteen parameters then): same conditions, same order, same text.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "map_checks.h"

static char g_msg[512];
int vo_fail(int code, const char* fmt, ...) {          // the library's keeps the message per thread; here one buffer does
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return code;
}

static int g_bad = 0;
static void expect(const char* what, int code, int want_code, const char* want_msg) {
  const bool ok = code == want_code && (code == VO_OK || std::strcmp(g_msg, want_msg) == 0);
  std::printf("%-58s -> %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) { std::printf("    got %d \"%s\"\n    want %d \"%s\"\n", code, code == VO_OK ? "" : g_msg, want_code, want_msg); ++g_bad; }
}

int main() {
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[64];                      // stands for device arrays: never dereferenced on the host
  const float* uv = reinterpret_cast<const float*>(dev);
  const float* app = reinterpret_cast<const float*>(dev + 16);
  const void* stats = dev + 32;
  const float K[9] = {180, 0, 0, 0, 180, 0, 320, 240, 1};
  const float K0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Knan[9] = {180, 0, 0, 0, NAN, 0, 320, 240, 1}, Krank2[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
  const float damp = 1e-3f;
  const MapFrames ok{2, K, uv, 4, app, 4, 4, nullptr};                 // the smallest window: 2 frames of n_max 4
  const MapRounds rok{3, 65536, 3, 3, 1.5f, &damp};
  const char* fn = "f";

  // ---- the frame check ----
  struct FrameRow { const char* what; MapFrames f; const void* stats; const MapRounds* r; int code; const char* msg; };
  auto with = [&](auto edit) { MapFrames f = ok; edit(f); return f; };
  const MapRounds r_neg{-1, 65536, 3, 3, 1.5f, &damp};
  const size_t big = ((size_t)1 << 30) + 1;
  const FrameRow frames[] = {
      {"the smallest window", ok, stats, &rok, VO_OK, ""},
      {"no round parameters (culling)", ok, stats, nullptr, VO_OK, ""},
      {"n_frames 0", with([](MapFrames& f) { f.n_frames = 0; }), stats, &rok, E, "f: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames 1", with([](MapFrames& f) { f.n_frames = 1; }), stats, &rok, VO_OK, ""},
      {"n_frames 65535", with([](MapFrames& f) { f.n_frames = 65535; }), stats, &rok, VO_OK, ""},
      {"n_frames 65536", with([](MapFrames& f) { f.n_frames = 65536; }), stats, &rok, E, "f: n_frames 65536 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames -1", with([](MapFrames& f) { f.n_frames = -1; }), stats, &rok, E, "f: n_frames -1 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_max -1", with([](MapFrames& f) { f.n_max = -1; }), stats, &rok, E, "f: negative row count"},
      {"n_max 0, no arrays, strides 0", with([](MapFrames& f) { f.n_max = 0; f.d_uv = f.d_app = nullptr; f.uv_stride = f.app_stride = 0; }), stats, &rok, VO_OK, ""},
      {"null pixels", with([](MapFrames& f) { f.d_uv = nullptr; }), stats, &rok, E, "f: null argument"},
      {"null appearances", with([](MapFrames& f) { f.d_app = nullptr; }), stats, &rok, E, "f: null argument"},
      {"pixels 4 bytes off", with([&](MapFrames& f) { f.d_uv = uv + 1; }), stats, &rok, E, "f: device arrays must be 8-byte aligned"},
      {"appearances 4 bytes off", with([&](MapFrames& f) { f.d_app = app + 1; }), stats, &rok, E, "f: device arrays must be 8-byte aligned"},
      {"statistics 1 byte off", ok, dev + 33, &rok, E, "f: device arrays must be 8-byte aligned"},
      {"null statistics are the caller's to refuse", ok, nullptr, &rok, VO_OK, ""},
      {"uv_stride one below n_max", with([](MapFrames& f) { f.uv_stride = 3; }), stats, &rok, E, "f: a stride is smaller than n_max"},
      {"app_stride one below n_max", with([](MapFrames& f) { f.app_stride = 3; }), stats, &rok, E, "f: a stride is smaller than n_max"},
      {"a stride below n_max with one frame", with([](MapFrames& f) { f.n_frames = 1; f.app_stride = 3; }), stats, &rok, E, "f: a stride is smaller than n_max"},
      {"uv_stride 0x7ffffffe", with([](MapFrames& f) { f.uv_stride = 0x7ffffffe; }), stats, &rok, VO_OK, ""},
      {"uv_stride 0x7fffffff", with([](MapFrames& f) { f.uv_stride = 0x7fffffff; }), stats, &rok, E, "f: stride too large"},
      {"app_stride 0x7fffffff / 10 - 1", with([](MapFrames& f) { f.app_stride = 0x7fffffff / 10 - 1; }), stats, &rok, VO_OK, ""},
      {"app_stride 0x7fffffff / 10", with([](MapFrames& f) { f.app_stride = 0x7fffffff / 10; }), stats, &rok, E, "f: more than 2^30 rows in one call"},
      {"n_max * n_frames = 2^30", with([](MapFrames& f) { f.n_frames = 1024; f.n_max = 1 << 20; f.uv_stride = f.app_stride = (size_t)1 << 20; }), stats, &rok, VO_OK, ""},
      {"n_max * n_frames = 2^30 + 1024", with([](MapFrames& f) { f.n_frames = 1024; f.n_max = (1 << 20) + 1; f.uv_stride = f.app_stride = ((size_t)1 << 20) + 1; }), stats, &rok, E,
       "f: more than 2^30 rows in one call"},
      {"n_max * n_frames = 2^30 + 1", with([&](MapFrames& f) { f.n_frames = 1; f.n_max = (int)big; f.uv_stride = f.app_stride = big; }), stats, &rok, E, "f: more than 2^30 rows in one call"},
      {"n_max INT_MAX, 65535 frames (no overflow)", with([](MapFrames& f) { f.n_frames = 65535; f.n_max = 0x7fffffff; f.uv_stride = 0x7ffffffe; f.app_stride = 0x7fffffff; }), stats, &rok, E,
       "f: a stride is smaller than n_max"},
      {"K all zero", with([&](MapFrames& f) { f.K = K0; }), stats, &rok, E, "f: K is singular"},
      {"K of rank 2", with([&](MapFrames& f) { f.K = Krank2; }), stats, &rok, E, "f: K is singular"},
      {"K with a NaN", with([&](MapFrames& f) { f.K = Knan; }), stats, &rok, E, "f: K is singular"},
      // where two would fail, the first in the order written at map_frames_check
      {"n_frames 0 before n_max -1", with([](MapFrames& f) { f.n_frames = 0; f.n_max = -1; }), stats, &rok, E, "f: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_max -1 before null arrays", with([](MapFrames& f) { f.n_max = -1; f.d_uv = nullptr; }), stats, &rok, E, "f: negative row count"},
      {"null before unaligned", with([&](MapFrames& f) { f.d_uv = nullptr; f.d_app = app + 1; }), stats, &rok, E, "f: null argument"},
      {"unaligned before a small stride", with([&](MapFrames& f) { f.d_uv = uv + 1; f.uv_stride = 3; }), stats, &rok, E, "f: device arrays must be 8-byte aligned"},
      {"a small stride before a large one", with([](MapFrames& f) { f.app_stride = 3; f.uv_stride = 0x7fffffff; }), stats, &rok, E, "f: a stride is smaller than n_max"},
      {"a large stride before the rounds", with([](MapFrames& f) { f.uv_stride = 0x7fffffff; }), stats, &r_neg, E, "f: stride too large"},
      {"the rounds before a singular K", with([&](MapFrames& f) { f.K = K0; }), stats, &r_neg, E, "f: negative n_rounds"},
      {"a singular K before 2^30 rows", with([&](MapFrames& f) { f.K = K0; f.app_stride = 0x7fffffff / 10; }), stats, &rok, E, "f: K is singular"},
      {"bad rounds not looked at without them", with([&](MapFrames& f) { f.K = K0; }), stats, nullptr, E, "f: K is singular"},
  };
  for (const FrameRow& r : frames) expect(r.what, map_frames_check(fn, r.f, r.stats, r.r), r.code, r.msg);

  // ---- the round parameters ----
  const float inf = INFINITY, nan = NAN, neg = -1e-30f, zero = 0.f, most = FLT_MAX, negzero = -0.f;
  struct RoundRow { const char* what; MapRounds r; int code; const char* msg; };
  const RoundRow rounds[] = {
      {"three rounds", rok, VO_OK, ""},
      {"n_rounds 0", {0, 65536, 3, 3, 1.5f, &damp}, VO_OK, ""},
      {"n_rounds -1", {-1, 65536, 3, 3, 1.5f, &damp}, E, "f: negative n_rounds"},
      {"n_rounds at the most", {65536, 65536, 3, 3, 1.5f, &damp}, VO_OK, ""},
      {"n_rounds one above the most", {65537, 65536, 3, 3, 1.5f, &damp}, E, "f: more than 65536 rounds"},
      {"n_rounds INT_MAX where nothing bounds them", {0x7fffffff, 0x7fffffff, 2, 2, 1.5f, &damp}, VO_OK, ""},
      {"min_obs one below the least (3)", {3, 65536, 2, 3, 1.5f, &damp}, E, "f: min_obs must be at least 3"},
      {"min_obs one below the least (2)", {3, 65536, 1, 2, 1.5f, &damp}, E, "f: min_obs must be at least 2"},
      {"min_obs above the least", {3, 65536, 7, 2, 1.5f, &damp}, VO_OK, ""},
      {"huber_px 0 (no robust weight)", {3, 65536, 3, 3, 0.f, &damp}, VO_OK, ""},
      {"huber_px -0", {3, 65536, 3, 3, negzero, &damp}, VO_OK, ""},
      {"huber_px FLT_MAX", {3, 65536, 3, 3, most, &damp}, VO_OK, ""},
      {"huber_px negative", {3, 65536, 3, 3, neg, &damp}, E, "f: huber_px must be finite and not negative"},
      {"huber_px infinite", {3, 65536, 3, 3, inf, &damp}, E, "f: huber_px must be finite and not negative"},
      {"huber_px NaN", {3, 65536, 3, 3, nan, &damp}, E, "f: huber_px must be finite and not negative"},
      {"damping 0", {3, 65536, 3, 3, 1.5f, &zero}, VO_OK, ""},
      {"damping FLT_MAX", {3, 65536, 3, 3, 1.5f, &most}, VO_OK, ""},
      {"damping negative", {3, 65536, 3, 3, 1.5f, &neg}, E, "f: damping must be finite and not negative"},
      {"damping infinite", {3, 65536, 3, 3, 1.5f, &inf}, E, "f: damping must be finite and not negative"},
      {"damping NaN", {3, 65536, 3, 3, 1.5f, &nan}, E, "f: damping must be finite and not negative"},
      {"a call without damping (the bundle)", {3, 65536, 3, 3, 1.5f, nullptr}, VO_OK, ""},
      {"n_rounds before min_obs", {-1, 65536, 2, 3, nan, &nan}, E, "f: negative n_rounds"},
      {"min_obs before huber_px", {3, 65536, 2, 3, nan, &nan}, E, "f: min_obs must be at least 3"},
      {"huber_px before damping", {3, 65536, 3, 3, nan, &nan}, E, "f: huber_px must be finite and not negative"},
  };
  for (const RoundRow& r : rounds) expect(r.what, map_rounds_check(fn, r.r), r.code, r.msg);

  // ---- the capture-growth refusal ----
  const int N = VO_ERR_NOT_READY;
  expect("not capturing: a small workspace may grow", capture_growth_check(false, fn, {{0, 100}}, "%d frames", 2), VO_OK, "");
  expect("capturing, nothing to size", capture_growth_check(true, fn, {}, "these maps"), VO_OK, "");
  expect("capturing, the workspace is exactly enough", capture_growth_check(true, fn, {{100, 100}, {0, 0}}, "%d frames", 2), VO_OK, "");
  expect("capturing, one byte short", capture_growth_check(true, "vo_map_refine_batch_dev", {{99, 100}}, "%d frames of n_max %d on this map", 2, 4), N,
         "vo_map_refine_batch_dev: the workspace would have to grow inside a graph capture (make one call with 2 frames of n_max 4 on this map before capturing)");
  expect("capturing, the second buffer short", capture_growth_check(true, "voe_map_merge_dev", {{100, 100}, {7, 8}, {5, 5}}, "these maps"), N,
         "voe_map_merge_dev: the workspace would have to grow inside a graph capture (make one call with these maps before capturing)");
  expect("capturing, three numbers in the tail", capture_growth_check(true, "voe_map_covis_batch_dev", {{0, 1}}, "%d frames of n_max %d and %d words on this map", 4096, 1 << 30, 0x7fffffff), N,
         "voe_map_covis_batch_dev: the workspace would have to grow inside a graph capture (make one call with 4096 frames of n_max 1073741824 and 2147483647 words on this map before capturing)");
  {   // a tail longer than its buffer is cut, not overrun
    const std::string longtail(400, 'x');
    const int code = capture_growth_check(true, fn, {{0, 1}}, "%s", longtail.c_str());
    const bool ok = code == N && std::strlen(g_msg) < sizeof(g_msg) && std::strstr(g_msg, "xxxx before capturing)") != nullptr;
    std::printf("%-58s -> %s\n", "capturing, a tail of 400 characters", ok ? "ok" : "FAILED");
    g_bad += !ok;
  }

  // ---- invert_k against the product ----
  double Ki[9];
  bool inv_ok = invert_k(K, Ki);
  for (int r = 0; r < 3 && inv_ok; ++r)
    for (int c = 0; c < 3; ++c) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)K[r + 3 * k] * Ki[k + 3 * c];
      inv_ok = inv_ok && std::fabs(s - (r == c)) < 1e-12;
    }
  std::printf("%-58s -> %s\n", "K * K^-1 = I", inv_ok ? "ok" : "FAILED");
  g_bad += !inv_ok;

  if (g_bad) { std::printf("map_checks_check: %d FAILED\n", g_bad); return 1; }
  std::puts("map_checks_check: all ok");
  return 0;
}
