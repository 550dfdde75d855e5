// map_guided_checks_check -- the refusals of voe_map_guided* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// map_guided_check) under the host sanitizers, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_guided_checks_check.cpp -o map_guided_checks_check && ./map_guided_checks_check
//   (ends with "map_guided_checks_check: all ok")
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
  static_assert(sizeof(voe_map_guided_params) == 32 && sizeof(voe_map_guided_stats) == 48, "the records of GUIDED in vo_hip.h");
  static_assert(offsetof(voe_map_guided_params, z_near) == 16 && offsetof(voe_map_guided_params, reserved) == 24, "the parameters' layout");
  static_assert(offsetof(voe_map_guided_stats, n_nan) == 28 && offsetof(voe_map_guided_stats, n_in_view) == 32 && offsetof(voe_map_guided_stats, n_gated) == 40,
                "the eight counts of voe_map_nearest_stats, then two 8-byte ones");
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[1 << 16];                 // stands for the device's arrays: never dereferenced on the host
  const float* app = reinterpret_cast<const float*>(dev);
  const float* uv = reinterpret_cast<const float*>(dev + (1 << 14));
  char* far = dev + (1 << 15);                         // 4 frames x stride 12 x 40 bytes = 1920 bytes: far beyond the frames
  static const float K[9] = {500.f, 0.f, 0.f, 0.f, 500.f, 0.f, 320.f, 240.f, 1.f};
  const voe_map_guided_params ok{8.f, 0.1f, 0.8f, 1, 0, 10, {0, 0}};
  const MapFrames frames{4, K, uv, 12, app, 12, 10, nullptr};
  const MapGuidedPtrs all{far + 20480, far, far + 4096, far + 8192, far + 10240, far + 12288, far + 16384};
  const MapGuidedPtrs least{far + 20480, far, nullptr, nullptr, nullptr, nullptr, nullptr};
  const char* fn = "g";
  auto with = [&](auto edit) { voe_map_guided_params p = ok; edit(p); return p; };
  auto ptrs = [&](auto edit) { MapGuidedPtrs d = all; edit(d); return d; };
  auto fr = [&](auto edit) { MapFrames f = frames; edit(f); return f; };
  using P = voe_map_guided_params;
  using D = MapGuidedPtrs;
  using F = MapFrames;
  const size_t span = 40 * (3 * 12 + 10);              // bytes the frames span
  const char* nulls = "g: null params, d_entry_out, d_T16 or K";
  const char* four = "g: int32 and float32 arrays must be 4-byte aligned";
  const char* eight = "g: d_app_out and d_stats must be 8-byte aligned";
  struct Row { const char* what; MapFrames f; MapGuidedPtrs d; voe_map_guided_params p; int code; const char* msg; };
  const Row rows[] = {
      {"the defaults, every array", frames, all, ok, VO_OK, ""},
      {"the defaults, d_entry_out alone", frames, least, ok, VO_OK, ""},
      // the lookup's refusals for the frames
      {"n_frames 0", fr([](F& f) { f.n_frames = 0; }), all, ok, E, "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames INT_MIN", fr([](F& f) { f.n_frames = INT_MIN; }), all, ok, E, "g: n_frames -2147483648 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames 65535", fr([](F& f) { f.n_frames = 65535; f.n_max = 1; }), least, ok, VO_OK, ""},
      {"n_frames 65536", fr([](F& f) { f.n_frames = 65536; }), all, ok, E, "g: n_frames 65536 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_max -1", fr([](F& f) { f.n_max = -1; }), all, ok, E, "g: negative row count"},
      {"n_max 0, null rows and pixels", fr([](F& f) { f.n_max = 0; f.d_app = nullptr; f.d_uv = nullptr; f.app_stride = f.uv_stride = 0; }), all, ok, VO_OK, ""},
      {"null rows with n_max > 0", fr([](F& f) { f.d_app = nullptr; }), all, ok, E, "g: null argument"},
      {"null pixels with n_max > 0", fr([](F& f) { f.d_uv = nullptr; }), all, ok, E, "g: null argument"},
      {"rows 4 bytes off", fr([&](F& f) { f.d_app = app + 1; }), all, ok, E, "g: device appearance rows and pixels must be 8-byte aligned"},
      {"pixels 4 bytes off", fr([&](F& f) { f.d_uv = uv + 1; }), all, ok, E, "g: device appearance rows and pixels must be 8-byte aligned"},
      {"pixels 8 bytes off", fr([&](F& f) { f.d_uv = uv + 2; }), all, ok, VO_OK, ""},
      {"app_stride below n_max", fr([](F& f) { f.app_stride = 9; }), all, ok, E, "g: a stride is smaller than n_max 10"},
      {"uv_stride below n_max", fr([](F& f) { f.uv_stride = 9; }), all, ok, E, "g: a stride is smaller than n_max 10"},
      {"uv_stride below n_max, one frame", fr([](F& f) { f.uv_stride = 9; f.n_frames = 1; }), all, ok, E, "g: a stride is smaller than n_max 10"},
      {"strides == n_max", fr([](F& f) { f.app_stride = f.uv_stride = 10; }), all, ok, VO_OK, ""},
      {"app_stride (2^31 - 1) / 10", fr([](F& f) { f.app_stride = 0x7fffffff / 10; f.n_frames = 1; }), least, ok, E, "g: more than 2^30 rows in one call"},
      {"uv_stride 2^31 - 1", fr([](F& f) { f.uv_stride = 0x7fffffff; f.n_frames = 1; }), least, ok, E, "g: more than 2^30 rows in one call"},
      {"2^30 rows", fr([](F& f) { f.n_frames = 1 << 15; f.n_max = 1 << 15; f.app_stride = f.uv_stride = 1 << 15; }), least, ok, VO_OK, ""},
      {"2^30 + 2^15 rows", fr([](F& f) { f.n_frames = (1 << 15) + 1; f.n_max = 1 << 15; f.app_stride = f.uv_stride = 1 << 15; }), least, ok, E,
       "g: more than 2^30 rows in one call"},
      // the call's own
      {"null d_entry_out", frames, ptrs([](D& d) { d.entry = nullptr; }), ok, E, nulls},
      {"null d_T16", frames, ptrs([](D& d) { d.T16 = nullptr; }), ok, E, nulls},
      {"null K", fr([](F& f) { f.K = nullptr; }), all, ok, E, nulls},
      {"radius_px 0", frames, all, with([](P& p) { p.radius_px = 0.f; }), E, "g: radius_px must be finite and positive"},
      {"radius_px -1", frames, all, with([](P& p) { p.radius_px = -1.f; }), E, "g: radius_px must be finite and positive"},
      {"radius_px NaN", frames, all, with([](P& p) { p.radius_px = NAN; }), E, "g: radius_px must be finite and positive"},
      {"radius_px inf", frames, all, with([](P& p) { p.radius_px = INFINITY; }), E, "g: radius_px must be finite and positive"},
      {"radius_px FLT_MAX", frames, all, with([](P& p) { p.radius_px = 3.402823466e38f; }), VO_OK, ""},
      {"radius_px 1e-30", frames, all, with([](P& p) { p.radius_px = 1e-30f; }), VO_OK, ""},
      {"radius 0", frames, all, with([](P& p) { p.radius = 0.f; }), E, "g: radius must be finite and positive"},
      {"radius -0", frames, all, with([](P& p) { p.radius = -0.f; }), E, "g: radius must be finite and positive"},
      {"radius NaN", frames, all, with([](P& p) { p.radius = NAN; }), E, "g: radius must be finite and positive"},
      {"radius inf", frames, all, with([](P& p) { p.radius = INFINITY; }), E, "g: radius must be finite and positive"},
      {"radius FLT_MAX", frames, all, with([](P& p) { p.radius = 3.402823466e38f; }), VO_OK, ""},
      {"ratio 0 (off)", frames, all, with([](P& p) { p.ratio = 0.f; }), VO_OK, ""},
      {"ratio -0 (off)", frames, all, with([](P& p) { p.ratio = -0.f; }), VO_OK, ""},
      {"ratio 1", frames, all, with([](P& p) { p.ratio = 1.f; }), VO_OK, ""},
      {"ratio above 1", frames, all, with([](P& p) { p.ratio = 1.0000001f; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"ratio -0.5", frames, all, with([](P& p) { p.ratio = -0.5f; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"ratio NaN", frames, all, with([](P& p) { p.ratio = NAN; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"unique 0", frames, all, with([](P& p) { p.unique = 0; }), VO_OK, ""},
      {"unique 2", frames, all, with([](P& p) { p.unique = 2; }), E, "g: unique must be 0 or 1"},
      {"unique -1", frames, all, with([](P& p) { p.unique = -1; }), E, "g: unique must be 0 or 1"},
      {"z_far == z_near", frames, all, with([](P& p) { p.z_near = p.z_far = 3; }), VO_OK, ""},
      {"z_far below z_near", frames, all, with([](P& p) { p.z_near = 3; p.z_far = 2; }), E, "g: z_far is below z_near"},
      {"negative depths in order", frames, all, with([](P& p) { p.z_near = -5; p.z_far = -2; }), VO_OK, ""},
      {"reserved[0] 1", frames, all, with([](P& p) { p.reserved[0] = 1; }), E, "g: reserved must be 0"},
      {"reserved[1] -1", frames, all, with([](P& p) { p.reserved[1] = -1; }), E, "g: reserved must be 0"},
      {"d_entry_out 2 bytes off", frames, ptrs([&](D& d) { d.entry = far + 2; }), ok, E, four},
      {"d_entry_out 4 bytes off", frames, ptrs([&](D& d) { d.entry = far + 4; }), ok, VO_OK, ""},
      {"d_status_out 1 byte off", frames, ptrs([&](D& d) { d.status = far + 4097; }), ok, E, four},
      {"d_dist2_out 2 bytes off", frames, ptrs([&](D& d) { d.dist2 = far + 8194; }), ok, E, four},
      {"d_pix2_out 2 bytes off", frames, ptrs([&](D& d) { d.pix2 = far + 10242; }), ok, E, four},
      {"d_pix2_out 4 bytes off", frames, ptrs([&](D& d) { d.pix2 = far + 10244; }), ok, VO_OK, ""},
      {"d_T16 2 bytes off", frames, ptrs([&](D& d) { d.T16 = far + 20482; }), ok, E, four},
      {"d_T16 4 bytes off", frames, ptrs([&](D& d) { d.T16 = far + 20484; }), ok, VO_OK, ""},
      {"d_stats 4 bytes off", frames, ptrs([&](D& d) { d.stats = far + 16388; }), ok, E, eight},
      {"d_app_out 4 bytes off", frames, ptrs([&](D& d) { d.app_out = far + 12292; }), ok, E, eight},
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
      {"the stride before the radius", fr([](F& f) { f.uv_stride = 9; }), all, with([](P& p) { p.radius_px = 0.f; }), E, "g: a stride is smaller than n_max 10"},
      {"the null output before the radius", frames, ptrs([](D& d) { d.entry = nullptr; }), with([](P& p) { p.radius_px = 0.f; }), E, nulls},
      {"radius_px before radius", frames, all, with([](P& p) { p.radius_px = 0.f; p.radius = 0.f; }), E, "g: radius_px must be finite and positive"},
      {"the radius before the ratio", frames, all, with([](P& p) { p.radius = 0.f; p.ratio = 2.f; }), E, "g: radius must be finite and positive"},
      {"the ratio before unique", frames, all, with([](P& p) { p.ratio = 2.f; p.unique = 2; }), E, "g: ratio must be 0 (off) or in (0, 1]"},
      {"unique before the depths", frames, all, with([](P& p) { p.unique = 2; p.z_far = -1; }), E, "g: unique must be 0 or 1"},
      {"the depths before reserved", frames, all, with([](P& p) { p.z_far = -1; p.reserved[0] = 1; }), E, "g: z_far is below z_near"},
      {"reserved before the alignment", frames, ptrs([&](D& d) { d.stats = far + 16388; }), with([](P& p) { p.reserved[1] = 1; }), E, "g: reserved must be 0"},
      {"the alignment before the overlap", frames, ptrs([&](D& d) { d.app_out = dev + 40; d.stats = far + 16388; }), ok, E, eight},
  };
  for (const Row& r : rows) expect(r.what, map_guided_check(fn, r.f, &r.p, r.d), r.code, r.msg);
  expect("null params", map_guided_check(fn, frames, nullptr, all), E, nulls);
  if (g_bad) { std::printf("map_guided_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_guided_checks_check: all ok\n");
  return 0;
}
