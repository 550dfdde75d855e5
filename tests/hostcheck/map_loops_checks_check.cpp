// map_loops_checks_check -- the refusals of voe_map_loops* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// map_loops_check) under the host sanitizers, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_loops_checks_check.cpp -o map_loops_checks_check && ./map_loops_checks_check
//   (ends with "map_loops_checks_check: all ok")
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
  static_assert(sizeof(voe_map_loops_params) == 72 && sizeof(voe_map_loop_record) == 40 && sizeof(voe_map_loops_stats) == 32, "the records of vo_map_loops.h");
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[64];                      // stands for the device's arrays: never dereferenced on the host
  const voe_map_loops_params ok{50, 5, 12, 3, 8, 0, {64, 2.f, 0}, 10000.f, 50, 6, {1.f, 1.f, 1.f}, 0};
  const MapLoopsPtrs all{dev, dev, dev, dev, dev, dev, dev, dev};
  const MapLoopsPtrs least{dev, dev, dev, dev, dev, nullptr, nullptr, dev};
  const char* fn = "g";
  auto with = [&](auto edit) { voe_map_loops_params p = ok; edit(p); return p; };
  auto ptrs = [&](auto edit) { MapLoopsPtrs d = all; edit(d); return d; };
  using P = voe_map_loops_params;
  using D = MapLoopsPtrs;
  struct Row { const char* what; int n_frames; MapLoopsPtrs d; voe_map_loops_params p; int code; const char* msg; };
  const Row rows[] = {
      {"the defaults, every array", 121, all, ok, VO_OK, ""},
      {"the defaults, no optional array", 121, least, ok, VO_OK, ""},
      {"null d_S16", 121, ptrs([](D& d) { d.S16 = nullptr; }), ok, E, "g: null argument"},
      {"null d_edges_out", 121, ptrs([](D& d) { d.edges = nullptr; }), ok, E, "g: null argument"},
      {"null d_Z16_out", 121, ptrs([](D& d) { d.Z16 = nullptr; }), ok, E, "g: null argument"},
      {"null d_weights_out", 121, ptrs([](D& d) { d.weights = nullptr; }), ok, E, "g: null argument"},
      {"null d_loops_out", 121, ptrs([](D& d) { d.loops = nullptr; }), ok, E, "g: null argument"},
      {"null d_stats", 121, ptrs([](D& d) { d.stats = nullptr; }), ok, E, "g: null argument"},
      {"n_frames 0", 0, all, ok, E, "g: n_frames 0 outside 1 .. 4096"},
      {"n_frames INT_MIN", INT_MIN, all, ok, E, "g: n_frames -2147483648 outside 1 .. 4096"},
      {"n_frames 4096", 4096, all, ok, VO_OK, ""},
      {"n_frames 4097", 4097, all, ok, E, "g: n_frames 4097 outside 1 .. 4096"},
      {"d_loops_out 4 bytes off", 121, ptrs([](D& d) { d.loops = dev + 4; }), ok, E, "g: d_loops_out and d_stats must be 8-byte aligned"},
      {"d_stats 4 bytes off", 121, ptrs([](D& d) { d.stats = dev + 4; }), ok, E, "g: d_loops_out and d_stats must be 8-byte aligned"},
      {"d_S16 2 bytes off", 121, ptrs([](D& d) { d.S16 = dev + 2; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_S16 4 bytes off", 121, ptrs([](D& d) { d.S16 = dev + 4; }), ok, VO_OK, ""},
      {"d_edges_out 1 byte off", 121, ptrs([](D& d) { d.edges = dev + 1; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_Z16_out 2 bytes off", 121, ptrs([](D& d) { d.Z16 = dev + 2; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_weights_out 4 bytes off", 121, ptrs([](D& d) { d.weights = dev + 4; }), ok, VO_OK, ""},
      {"d_hist_out 2 bytes off", 121, ptrs([](D& d) { d.hist = dev + 2; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_ref_frame_out 3 bytes off", 121, ptrs([](D& d) { d.ref_frame = dev + 3; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"gap 0", 121, all, with([](P& p) { p.gap = 0; }), VO_OK, ""},
      {"gap -1", 121, all, with([](P& p) { p.gap = -1; }), E, "g: negative gap"},
      {"gap INT_MAX (no candidate, no overflow)", 121, all, with([](P& p) { p.gap = INT_MAX; }), VO_OK, ""},
      {"ref_window 0", 121, all, with([](P& p) { p.ref_window = 0; }), VO_OK, ""},
      {"ref_window -1", 121, all, with([](P& p) { p.ref_window = -1; }), E, "g: negative ref_window"},
      {"ref_window INT_MAX", 121, all, with([](P& p) { p.ref_window = INT_MAX; }), VO_OK, ""},
      {"min_shared 1", 121, all, with([](P& p) { p.min_shared = 1; }), VO_OK, ""},
      {"min_shared 0", 121, all, with([](P& p) { p.min_shared = 0; }), E, "g: min_shared must be at least 1"},
      {"separation 0", 121, all, with([](P& p) { p.separation = 0; }), VO_OK, ""},
      {"separation -1", 121, all, with([](P& p) { p.separation = -1; }), E, "g: negative separation"},
      {"separation INT_MAX", 121, all, with([](P& p) { p.separation = INT_MAX; }), VO_OK, ""},
      {"max_loops 1", 121, all, with([](P& p) { p.max_loops = 1; }), VO_OK, ""},
      {"max_loops 0", 121, all, with([](P& p) { p.max_loops = 0; }), E, "g: max_loops 0 outside 1 .. n_frames"},
      {"max_loops == n_frames", 121, all, with([](P& p) { p.max_loops = 121; }), VO_OK, ""},
      {"max_loops n_frames + 1", 121, all, with([](P& p) { p.max_loops = 122; }), E, "g: max_loops 122 outside 1 .. n_frames"},
      {"w_loop 0 0 1", 121, all, with([](P& p) { p.w_loop[0] = 0.f; p.w_loop[1] = 0.f; }), VO_OK, ""},
      {"w_loop -1 1 1", 121, all, with([](P& p) { p.w_loop[0] = -1.f; }), E, "g: w_loop must be finite and not negative"},
      {"w_loop 1 NaN 1", 121, all, with([](P& p) { p.w_loop[1] = NAN; }), E, "g: w_loop must be finite and not negative"},
      {"w_loop 1 1 inf", 121, all, with([](P& p) { p.w_loop[2] = INFINITY; }), E, "g: w_loop must be finite and not negative"},
      {"w_loop 0 0 0", 121, all, with([](P& p) { p.w_loop[0] = p.w_loop[1] = p.w_loop[2] = 0.f; }), E, "g: w_loop is all zero"},
      {"w_loop -0 -0 -0", 121, all, with([](P& p) { p.w_loop[0] = p.w_loop[1] = p.w_loop[2] = -0.f; }), E, "g: w_loop is all zero"},
      {"a null pointer before n_frames", 0, ptrs([](D& d) { d.S16 = nullptr; }), ok, E, "g: null argument"},
      {"n_frames before the alignment", 0, ptrs([](D& d) { d.stats = dev + 4; }), ok, E, "g: n_frames 0 outside 1 .. 4096"},
      {"the alignment before the parameters", 121, ptrs([](D& d) { d.stats = dev + 4; }), with([](P& p) { p.gap = -1; }), E,
       "g: d_loops_out and d_stats must be 8-byte aligned"},
      {"gap before min_shared", 121, all, with([](P& p) { p.gap = -1; p.min_shared = 0; }), E, "g: negative gap"},
      {"max_loops before w_loop", 121, all, with([](P& p) { p.max_loops = 0; p.w_loop[0] = -1.f; }), E, "g: max_loops 0 outside 1 .. n_frames"},
  };
  for (const Row& r : rows) expect(r.what, map_loops_check(fn, r.n_frames, r.d, &r.p), r.code, r.msg);
  expect("null params", map_loops_check(fn, 121, all, nullptr), E, "g: null argument");
  if (g_bad) { std::printf("map_loops_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_loops_checks_check: all ok\n");
  return 0;
}
