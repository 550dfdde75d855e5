// map_fuse_checks_check -- the refusals of voe_map_fuse* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// map_fuse_check) under the host sanitizers, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_fuse_checks_check.cpp -o map_fuse_checks_check && ./map_fuse_checks_check
//   (ends with "map_fuse_checks_check: all ok")
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
  static_assert(sizeof(voe_map_fuse_params) == 32 && sizeof(voe_map_fuse_stats) == 56, "the records of FUSE in vo_hip.h");
  static_assert(offsetof(voe_map_fuse_params, radius) == 4 && offsetof(voe_map_fuse_params, position) == 8 &&
                offsetof(voe_map_fuse_params, veto_shared_frame) == 12 && offsetof(voe_map_fuse_params, dry_run) == 16 &&
                offsetof(voe_map_fuse_params, reserved) == 20, "voe_map_fuse_params");
  static_assert(offsetof(voe_map_fuse_stats, n_rows_rewritten) == 20 && offsetof(voe_map_fuse_stats, by_verdict) == 24 &&
                offsetof(voe_map_fuse_stats, n_gated) == 48, "voe_map_fuse_stats");
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[1 << 16];                 // stands for the device's arrays: never dereferenced on the host
  const float* app = reinterpret_cast<const float*>(dev);
  char* far = dev + (1 << 15);                         // 4 frames x stride 12 x 40 bytes = 1920 bytes: far beyond the frames
  const voe_map_fuse_params ok{0.04f, 0.1f, 1, 1, 0, {0, 0, 0}};
  const voe_map_fuse_params plain{0.04f, 0.1f, 0, 0, 0, {0, 0, 0}};      // what a call without frames may ask
  const MapFrames frames{4, nullptr, nullptr, 0, app, 12, 10, nullptr};
  const MapFrames none{0, nullptr, nullptr, 0, nullptr, 0, 0, nullptr};
  const MapFusePtrs all{far, far + 2048, far + 4096, far + 6144, far + 8192, far + 12288, far + 16384};
  const MapFusePtrs least{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, far + 16384};
  const char* fn = "g";
  auto with = [&](auto edit) { voe_map_fuse_params p = ok; edit(p); return p; };
  auto ptrs = [&](auto edit) { MapFusePtrs d = all; edit(d); return d; };
  auto fr = [&](auto edit) { MapFrames f = frames; edit(f); return f; };
  using P = voe_map_fuse_params;
  using D = MapFusePtrs;
  using F = MapFrames;
  const int* counts = reinterpret_cast<const int*>(far + 20000);
  const size_t span = 40 * (3 * 12 + 10);              // bytes the frames span
  struct Row { const char* what; MapFrames f; MapFusePtrs d; voe_map_fuse_params p; int code; const char* msg; };
  const Row rows[] = {
      {"the defaults, every array", frames, all, ok, VO_OK, ""},
      {"the defaults, d_stats alone", frames, least, ok, VO_OK, ""},
      {"no frames, d_stats alone", none, least, plain, VO_OK, ""},
      {"no frames, the per-entry arrays", none, ptrs([](D& d) { d.app_out = nullptr; }), plain, VO_OK, ""},
      {"no frames, n_max ignored", fr([](F& f) { f = MapFrames{0, nullptr, nullptr, 0, nullptr, 7, 5, nullptr}; }), least, plain, VO_OK, ""},
      // the lookup's refusals for the frames, when frames are given
      {"n_frames 0 with rows", fr([](F& f) { f.n_frames = 0; }), all, ok, E, "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames 0 with counts alone", fr([&](F& f) { f.n_frames = 0; f.d_app = nullptr; f.d_n = counts; }), least, plain, E,
       "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames INT_MIN", fr([](F& f) { f.n_frames = INT_MIN; }), all, ok, E, "g: n_frames -2147483648 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_frames 65535", fr([](F& f) { f.n_frames = 65535; f.n_max = 1; }), least, ok, VO_OK, ""},
      {"n_frames 65536", fr([](F& f) { f.n_frames = 65536; }), all, ok, E, "g: n_frames 65536 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"n_max -1", fr([](F& f) { f.n_max = -1; }), all, ok, E, "g: negative row count"},
      {"frames with n_max 0 and null rows", fr([](F& f) { f.n_max = 0; f.d_app = nullptr; }), all, ok, VO_OK, ""},
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
      {"null d_stats", frames, ptrs([](D& d) { d.stats = nullptr; }), ok, E, "g: null params or d_stats"},
      {"radius_xyz 0", frames, all, with([](P& p) { p.radius_xyz = 0.f; }), E, "g: radius_xyz must be finite and positive"},
      {"radius_xyz -0", frames, all, with([](P& p) { p.radius_xyz = -0.f; }), E, "g: radius_xyz must be finite and positive"},
      {"radius_xyz -1", frames, all, with([](P& p) { p.radius_xyz = -1.f; }), E, "g: radius_xyz must be finite and positive"},
      {"radius_xyz NaN", frames, all, with([](P& p) { p.radius_xyz = NAN; }), E, "g: radius_xyz must be finite and positive"},
      {"radius_xyz inf", frames, all, with([](P& p) { p.radius_xyz = INFINITY; }), E, "g: radius_xyz must be finite and positive"},
      {"radius_xyz FLT_MAX", frames, all, with([](P& p) { p.radius_xyz = 3.402823466e38f; }), VO_OK, ""},
      {"radius_xyz 1e-30", frames, all, with([](P& p) { p.radius_xyz = 1e-30f; }), VO_OK, ""},
      {"radius 0", frames, all, with([](P& p) { p.radius = 0.f; }), E, "g: radius must be finite and positive"},
      {"radius -1", frames, all, with([](P& p) { p.radius = -1.f; }), E, "g: radius must be finite and positive"},
      {"radius NaN", frames, all, with([](P& p) { p.radius = NAN; }), E, "g: radius must be finite and positive"},
      {"radius inf", frames, all, with([](P& p) { p.radius = INFINITY; }), E, "g: radius must be finite and positive"},
      {"radius FLT_MAX", frames, all, with([](P& p) { p.radius = 3.402823466e38f; }), VO_OK, ""},
      {"position 0", frames, all, with([](P& p) { p.position = 0; }), VO_OK, ""},
      {"position 2", frames, all, with([](P& p) { p.position = 2; }), E, "g: position must be 0 or 1"},
      {"position -1", frames, all, with([](P& p) { p.position = -1; }), E, "g: position must be 0 or 1"},
      {"veto_shared_frame 0", frames, all, with([](P& p) { p.veto_shared_frame = 0; }), VO_OK, ""},
      {"veto_shared_frame 2", frames, all, with([](P& p) { p.veto_shared_frame = 2; }), E, "g: veto_shared_frame must be 0 or 1"},
      {"veto_shared_frame -1", frames, all, with([](P& p) { p.veto_shared_frame = -1; }), E, "g: veto_shared_frame must be 0 or 1"},
      {"dry_run 1", frames, all, with([](P& p) { p.dry_run = 1; }), VO_OK, ""},
      {"dry_run 2", frames, all, with([](P& p) { p.dry_run = 2; }), E, "g: dry_run must be 0 or 1"},
      {"dry_run -1", frames, all, with([](P& p) { p.dry_run = -1; }), E, "g: dry_run must be 0 or 1"},
      {"reserved[0] 1", frames, all, with([](P& p) { p.reserved[0] = 1; }), E, "g: reserved must be 0"},
      {"reserved[1] 1", frames, all, with([](P& p) { p.reserved[1] = 1; }), E, "g: reserved must be 0"},
      {"reserved[2] -1", frames, all, with([](P& p) { p.reserved[2] = -1; }), E, "g: reserved must be 0"},
      {"the veto without frames", none, least, with([](P& p) { p.veto_shared_frame = 1; }), E, "g: veto_shared_frame without frames"},
      {"d_app_out without frames", none, ptrs([](D&) {}), plain, E, "g: d_app_out without frames"},
      {"d_partner_out 2 bytes off", frames, ptrs([&](D& d) { d.partner = far + 2; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_partner_out 4 bytes off", frames, ptrs([&](D& d) { d.partner = far + 4; }), ok, VO_OK, ""},
      {"d_dist2_out 1 byte off", frames, ptrs([&](D& d) { d.dist2 = far + 2049; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_gap2_out 2 bytes off", frames, ptrs([&](D& d) { d.gap2 = far + 4098; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_verdict_out 3 bytes off", frames, ptrs([&](D& d) { d.verdict = far + 6147; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
      {"d_remap_out 2 bytes off", frames, ptrs([&](D& d) { d.remap = far + 8194; }), ok, E, "g: int32 and float32 arrays must be 4-byte aligned"},
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
      {"n_frames before the null d_stats", fr([](F& f) { f.n_frames = 0; }), ptrs([](D& d) { d.stats = nullptr; }), ok, E,
       "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)"},
      {"the stride before radius_xyz", fr([](F& f) { f.app_stride = 9; }), all, with([](P& p) { p.radius_xyz = 0.f; }), E, "g: app_stride 9 is smaller than n_max 10"},
      {"the null d_stats before radius_xyz", frames, ptrs([](D& d) { d.stats = nullptr; }), with([](P& p) { p.radius_xyz = 0.f; }), E, "g: null params or d_stats"},
      {"radius_xyz before radius", frames, all, with([](P& p) { p.radius_xyz = 0.f; p.radius = 0.f; }), E, "g: radius_xyz must be finite and positive"},
      {"radius before position", frames, all, with([](P& p) { p.radius = 0.f; p.position = 2; }), E, "g: radius must be finite and positive"},
      {"position before the veto", frames, all, with([](P& p) { p.position = 2; p.veto_shared_frame = 2; }), E, "g: position must be 0 or 1"},
      {"the veto before dry_run", frames, all, with([](P& p) { p.veto_shared_frame = 2; p.dry_run = 2; }), E, "g: veto_shared_frame must be 0 or 1"},
      {"dry_run before reserved", frames, all, with([](P& p) { p.dry_run = 2; p.reserved[0] = 1; }), E, "g: dry_run must be 0 or 1"},
      {"reserved before the veto without frames", none, least, with([](P& p) { p.reserved[0] = 1; }), E, "g: reserved must be 0"},
      {"the veto without frames before d_app_out without", none, ptrs([](D&) {}), with([](P&) {}), E, "g: veto_shared_frame without frames"},
      {"d_app_out without frames before the alignment", none, ptrs([&](D& d) { d.stats = far + 16388; }), plain, E, "g: d_app_out without frames"},
      {"reserved before the alignment", frames, ptrs([&](D& d) { d.stats = far + 16388; }), with([](P& p) { p.reserved[2] = 1; }), E, "g: reserved must be 0"},
      {"the alignment before the overlap", frames, ptrs([&](D& d) { d.app_out = dev + 40; d.stats = far + 16388; }), ok, E, "g: d_app_out and d_stats must be 8-byte aligned"},
  };
  for (const Row& r : rows) expect(r.what, map_fuse_check(fn, r.f, &r.p, r.d), r.code, r.msg);
  expect("null params", map_fuse_check(fn, frames, nullptr, all), E, "g: null params or d_stats");
  expect("null params without frames", map_fuse_check(fn, none, nullptr, least), E, "g: null params or d_stats");
  if (g_bad) { std::printf("map_fuse_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_fuse_checks_check: all ok\n");
  return 0;
}
