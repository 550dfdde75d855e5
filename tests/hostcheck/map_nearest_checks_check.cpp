// map_nearest_checks_check -- the refusals of voe_map_nearest* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// map_nearest_check) under the host sanitizers, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_nearest_checks_check.cpp -o map_nearest_checks_check && ./map_nearest_checks_check
//   (ends with "map_nearest_checks_check: all ok")
// Every row names the code and the whole message the call must leave; where two refusals would fire, the first listed in the
// header wins.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>

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
  static_assert(sizeof(voe_map_nearest_params) == 16 && sizeof(voe_map_nearest_stats) == 32, "the records of NEAREST in vo_hip.h");
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[1 << 16];                 // stands for the device's arrays: never dereferenced on the host
  const float* app = reinterpret_cast<const float*>(dev);
  char* far = dev + (1 << 15);                         // 4 frames x stride 12 x 40 bytes = 1920 bytes: far beyond the frames
  const voe_map_nearest_params ok{0.1f, 0.8f, 1, 0};
  const MapFrames frames{4, nullptr, nullptr, 0, app, 12, 10, nullptr};
  const MapNearestPtrs all{far, far + 4096, far + 8192, far + 12288, far + 16384};
  const MapNearestPtrs least{far, nullptr, nullptr, nullptr, nullptr};
  const char* fn = "g";
  auto with = [&](auto edit) { voe_map_nearest_params p = ok; edit(p); return p; };
  auto ptrs = [&](auto edit) { MapNearestPtrs d = all; edit(d); return d; };
  auto fr = [&](auto edit) { MapFrames f = frames; edit(f); return f; };
  using P = voe_map_nearest_params;
  using D = MapNearestPtrs;
  using F = MapFrames;
  const size_t span = 40 * (3 * 12 + 10);              // bytes the frames span
  struct Row { const char* what; MapFrames f; MapNearestPtrs d; voe_map_nearest_params p; int code; const char* msg; };
  const Row rows[] = {
      {"the defaults, every array", frames, all, ok, VO_OK, ""},
      {"the defaults, d_entry_out alone", frames, least, ok, VO_OK, ""},
      // the lookup's refusals for the frames
      {"n_frames 0", fr([](F& f) { f.n_frames = 0; }), all, ok, E, "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames INT_MIN", fr([](F& f) { f.n_frames = INT_MIN; }), all, ok, E, "g: n_frames -2147483648 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames 65535", fr([](F& f) { f.n_frames = 65535; f.n_max = 1; }), least, ok, VO_OK, ""},
      {"n_frames 65536", fr([](F& f) { f.n_frames = 65536; }), all, ok, E, "g: n_frames 65536 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_max -1", fr([](F& f) { f.n_max = -1; }), all, ok, E, "g: negative row count"},
      {"n_max 0, null rows", fr([](F& f) { f.n_max = 0; f.d_app = nullptr; }), all, ok, VO_OK, ""},
      {"null rows with n_max > 0", fr([](F& f) { f.d_app = nullptr; }), all, ok, E, "g: null argument"},
      {"rows 4 bytes off", fr([&](F& f) { f.d_app = app + 1; }), all, ok, E, "g: device appearance rows must be 8-byte aligned"},
      {"rows 8 bytes off", fr([&](F& f) { f.d_app = app + 2; }), all, ok, VO_OK, ""},
      {"app_stride below n_max", fr([](F& f) { f.app_stride = 9; }), all, ok, E, "g: app_stride 9 is smaller than n_max 10"},
      {"app_stride below n_max, one frame", fr([](F& f) { f.app_stride = 9; f.n_frames = 1; }), all, ok, VO_OK, ""},
      {"app_stride == n_max", fr([](F& f) { f.app_stride = 10; }), all, ok, VO_OK, ""},
      {"app_stride (2^31 - 1) / 10", fr([](F& f) { f.app_stride = 0x7fffffff / 10; f.n_frames = 1; }), least, ok, E, "g: more than 2^30 rows in one call"},
      {"2^30 rows", fr([](F& f) { f.n_frames = 1 << 15; f.n_max = 1 << 15; f.app_stride = 1 << 15; }), least, ok, VO_OK, ""},
      {"2^30 + 2^15 rows", fr([](F& f) { f.n_frames = (1 << 15) + 1; f.n_max = 1 << 15; f.app_stride = 1 << 15; }), least, ok, E, "g: more than 2^30 rows in one call"},
      // the call's own
      {"null d_entry_out", frames, ptrs([](D& d) { d.entry = nullptr; }), ok, E, "g: null params or d_entry_out"},
      {"radius 0", frames, all, with([](P& p) { p.radius = 0.f; }), E, "g: radius must be finite and positive"},
      {"radius -0", frames, all, with([](P& p) { p.radius = -0.f; }), E, "g: radius must be finite and positive"},
      {"radius -1", frames, all, with([](P& p) { p.radius = -1.f; }), E, "g: radius must be finite and positive"},
      {"radius NaN", frames, all, with([](P& p) { p.radius = NAN; }), E, "g: radius must be finite and positive"},
      {"radius inf", frames, all, with([](P& p) { p.radius = INFINITY; }), E, "g: radius must be finite and positive"},
      {"radius FLT_MAX", frames, all, with([](P& p) { p.radius = 3.402823466e38f; }), VO_OK, ""},
      {"radius 1e-30", frames, all, with([](P& p) { p.radius = 1e-30f; }), VO_OK, ""},
      {"ratio 0 (off)", frames, all, with([](P& p) { p.ratio = 0.f; }), VO_OK, ""},
      {"ratio -0 (off)", frames, all, with([](P& p) { p.ratio = -0.f; }), VO_OK, ""},
      {"ratio 1", frames, all, with([](P& p) { p.ratio = 1.f; }), VO_OK, ""},
      {"ratio 1e-30", frames, all, with([](P& p) { p.ratio = 1e-30f; }), VO_OK, ""},
      {"ratio above 1", frames, all, with([](P& p) { p.ratio = 1.0000001f; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"ratio -0.5", frames, all, with([](P& p) { p.ratio = -0.5f; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"ratio NaN", frames, all, with([](P& p) { p.ratio = NAN; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"ratio inf", frames, all, with([](P& p) { p.ratio = INFINITY; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"unique 0", frames, all, with([](P& p) { p.unique = 0; }), VO_OK, ""},
      {"unique 2", frames, all, with([](P& p) { p.unique = 2; }), E, "g: unique must be 0 or 1"},
      {"unique -1", frames, all, with([](P& p) { p.unique = -1; }), E, "g: unique must be 0 or 1"},
      {"reserved 1", frames, all, with([](P& p) { p.reserved = 1; }), E, "g: reserved must be 0"},
      {"d_entry_out 2 bytes off", frames, ptrs([&](D& d) { d.entry = far + 2; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_entry_out 4 bytes off", frames, ptrs([&](D& d) { d.entry = far + 4; }), ok, VO_OK, ""},
      {"d_status_out 1 byte off", frames, ptrs([&](D& d) { d.status = far + 4097; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_dist2_out 2 bytes off", frames, ptrs([&](D& d) { d.dist2 = far + 8194; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_stats 4 bytes off", frames, ptrs([&](D& d) { d.stats = far + 16388; }), ok, E, "g: d_app_out and d_stats must be 8-byte aligned"},
      {"d_app_out 4 bytes off", frames, ptrs([&](D& d) { d.app_out = far + 12292; }), ok, E, "g: d_app_out and d_stats must be 8-byte aligned"},
      {"d_app_out == d_app", frames, ptrs([&](D& d) { d.app_out = dev; }), ok, VO_OK, ""},
      {"d_app_out one row into d_app", frames, ptrs([&](D& d) { d.app_out = dev + 40; }), ok, E, "g: d_app_out overlaps d_app without being d_app"},
      {"d_app_out ending one row into d_app", fr([&](F& f) { f.d_app = app + 10 * 100; }), ptrs([&](D& d) { d.app_out = dev + 40 * 100 - span + 40; }), ok, E,
       "g: d_app_out overlaps d_app without being d_app"},
      {"d_app_out ending where d_app begins", fr([&](F& f) { f.d_app = app + 10 * 100; }), ptrs([&](D& d) { d.app_out = dev + 40 * 100 - span; }), ok, VO_OK, ""},
      {"d_app_out beginning where d_app ends", frames, ptrs([&](D& d) { d.app_out = dev + span; }), ok, VO_OK, ""},
      {"d_app_out 8 bytes before d_app's end", frames, ptrs([&](D& d) { d.app_out = dev + span - 8; }), ok, E, "g: d_app_out overlaps d_app without being d_app"},
      {"an overlap with n_max 0 is none", fr([](F& f) { f.n_max = 0; }), ptrs([&](D& d) { d.app_out = dev + 40; }), ok, VO_OK, ""},
      // the order
      {"n_frames before the null output", fr([](F& f) { f.n_frames = 0; }), ptrs([](D& d) { d.entry = nullptr; }), ok, E,
       "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"the stride before the radius", fr([](F& f) { f.app_stride = 9; }), all, with([](P& p) { p.radius = 0.f; }), E, "g: app_stride 9 is smaller than n_max 10"},
      {"the null output before the radius", frames, ptrs([](D& d) { d.entry = nullptr; }), with([](P& p) { p.radius = 0.f; }), E, "g: null params or d_entry_out"},
      {"the radius before the ratio", frames, all, with([](P& p) { p.radius = 0.f; p.ratio = 2.f; }), E, "g: radius must be finite and positive"},
      {"the ratio before unique", frames, all, with([](P& p) { p.ratio = 2.f; p.unique = 2; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"unique before reserved", frames, all, with([](P& p) { p.unique = 2; p.reserved = 1; }), E, "g: unique must be 0 or 1"},
      {"reserved before the alignment", frames, ptrs([&](D& d) { d.stats = far + 16388; }), with([](P& p) { p.reserved = 1; }), E, "g: reserved must be 0"},
      {"the alignment before the overlap", frames, ptrs([&](D& d) { d.app_out = dev + 40; d.stats = far + 16388; }), ok, E, "g: d_app_out and d_stats must be 8-byte aligned"},
  };
  for (const Row& r : rows) expect(r.what, map_nearest_check(fn, r.f, &r.p, r.d), r.code, r.msg);
  expect("null params", map_nearest_check(fn, frames, nullptr, all), E, "g: null params or d_entry_out");
  if (g_bad) { std::printf("map_nearest_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_nearest_checks_check: all ok\n");
  return 0;
}
