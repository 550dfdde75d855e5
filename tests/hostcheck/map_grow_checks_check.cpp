// map_grow_checks_check -- the refusals of voe_map_grow* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// map_grow_check and map_grow_room, behind the frame and round checks that tests/hostcheck/map_checks_check.cpp drives) under the
// host sanitizers, without a GPU and without the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/map_grow_checks_check.cpp -o map_grow_checks_check && ./map_grow_checks_check   (ends with "map_grow_checks_check: all ok")
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
  const int E = VO_ERR_INVALID_ARG;
  alignas(8) static char dev[64];                      // stands for the device's track array: never dereferenced on the host
  const voe_map_grow_params ok{5, 3, 3, 0.f, 0.f, 2.f, 0.f, 2.f, 0, 0};
  const char* fn = "g";
  struct Row { const char* what; voe_map_grow_params p; const void* tracks; int cap; int code; const char* msg; };
  auto with = [&](auto edit) { voe_map_grow_params p = ok; edit(p); return p; };
  const Row rows[] = {
      {"the defaults, no track array", ok, nullptr, 0, VO_OK, ""},
      {"the defaults, a track array", ok, dev, 4, VO_OK, ""},
      {"room without an array", ok, nullptr, 7, VO_OK, ""},
      {"min_frames 2", with([](voe_map_grow_params& p) { p.min_frames = 2; }), dev, 4, VO_OK, ""},
      {"min_frames 1", with([](voe_map_grow_params& p) { p.min_frames = 1; }), dev, 4, E, "g: min_frames must be at least 2"},
      {"min_frames INT_MIN", with([](voe_map_grow_params& p) { p.min_frames = INT_MIN; }), dev, 4, E, "g: min_frames must be at least 2"},
      {"max_rms_px 0 (off)", with([](voe_map_grow_params& p) { p.max_rms_px = 0.f; }), dev, 4, VO_OK, ""},
      {"max_rms_px -0.5", with([](voe_map_grow_params& p) { p.max_rms_px = -0.5f; }), dev, 4, E, "g: max_rms_px must be finite and not negative"},
      {"max_rms_px NaN", with([](voe_map_grow_params& p) { p.max_rms_px = NAN; }), dev, 4, E, "g: max_rms_px must be finite and not negative"},
      {"max_rms_px inf", with([](voe_map_grow_params& p) { p.max_rms_px = INFINITY; }), dev, 4, E, "g: max_rms_px must be finite and not negative"},
      {"max_err_px -1", with([](voe_map_grow_params& p) { p.max_err_px = -1.f; }), dev, 4, E, "g: max_err_px must be finite and not negative"},
      {"max_err_px NaN", with([](voe_map_grow_params& p) { p.max_err_px = NAN; }), dev, 4, E, "g: max_err_px must be finite and not negative"},
      {"min_parallax_deg 179.5", with([](voe_map_grow_params& p) { p.min_parallax_deg = 179.5f; }), dev, 4, VO_OK, ""},
      {"min_parallax_deg 180", with([](voe_map_grow_params& p) { p.min_parallax_deg = 180.f; }), dev, 4, E, "g: min_parallax_deg must be in [0, 180)"},
      {"min_parallax_deg -1", with([](voe_map_grow_params& p) { p.min_parallax_deg = -1.f; }), dev, 4, E, "g: min_parallax_deg must be in [0, 180)"},
      {"min_parallax_deg NaN", with([](voe_map_grow_params& p) { p.min_parallax_deg = NAN; }), dev, 4, E, "g: min_parallax_deg must be in [0, 180)"},
      {"max_added INT_MAX", with([](voe_map_grow_params& p) { p.max_added = INT_MAX; }), dev, 4, VO_OK, ""},
      {"max_added -1", with([](voe_map_grow_params& p) { p.max_added = -1; }), dev, 4, E, "g: negative max_added"},
      {"track_cap -1", ok, nullptr, -1, E, "g: negative track_cap"},
      {"a track array with track_cap 0", ok, dev, 0, E, "g: a track array with track_cap == 0"},
      {"the track array 4 bytes off", ok, dev + 4, 4, E, "g: d_track_out must be 8-byte aligned"},
      {"min_frames before the thresholds", with([](voe_map_grow_params& p) { p.min_frames = 0; p.max_rms_px = NAN; }), dev, 4, E, "g: min_frames must be at least 2"},
      {"the thresholds before max_added", with([](voe_map_grow_params& p) { p.max_err_px = -1.f; p.max_added = -1; }), dev, 4, E, "g: max_err_px must be finite and not negative"},
      {"max_added before track_cap", with([](voe_map_grow_params& p) { p.max_added = -2; }), dev + 4, -1, E, "g: negative max_added"},
  };
  for (const Row& r : rows) expect(r.what, map_grow_check(fn, &r.p, r.tracks, r.cap), r.code, r.msg);

  // ---- the room: max_added, or with 0 every row of the window, never below 1 and never past an int ----
  struct Room { const char* what; int max_added, n_frames, n_max, want; };
  const Room rooms[] = {
      {"max_added 7", 7, 3, 100, 7},
      {"max_added 0: the rows", 0, 3, 100, 300},
      {"max_added 0, no rows", 0, 3, 0, 1},
      {"max_added INT_MAX", INT_MAX, 3, 100, INT_MAX},
      {"max_added 0, 2^30 rows (no overflow of the product)", 0, 65535, 16384, 65535 * 16384},
  };
  for (const Room& r : rooms) {
    voe_map_grow_params p = ok;
    p.max_added = r.max_added;
    const int got = map_grow_room(&p, r.n_frames, r.n_max);
    const bool good = got == r.want;
    std::printf("%-58s -> %s\n", r.what, good ? "ok" : "FAILED");
    if (!good) { std::printf("    got %d want %d\n", got, r.want); ++g_bad; }
  }
  // ---- the rounds' own refusals, as the grow call asks them (least_obs 2, no limit of rounds) ----
  const float damp = 0.f, damp_bad = -1.f;
  expect("min_obs 2", map_rounds_check(fn, MapRounds{5, INT_MAX, 2, 2, 0.f, &damp}), VO_OK, "");
  expect("min_obs 1", map_rounds_check(fn, MapRounds{5, INT_MAX, 1, 2, 0.f, &damp}), E, "g: min_obs must be at least 2");
  expect("n_rounds 0 (the linear point alone)", map_rounds_check(fn, MapRounds{0, INT_MAX, 3, 2, 0.f, &damp}), VO_OK, "");
  expect("n_rounds -1", map_rounds_check(fn, MapRounds{-1, INT_MAX, 3, 2, 0.f, &damp}), E, "g: negative n_rounds");
  expect("damping -1", map_rounds_check(fn, MapRounds{5, INT_MAX, 3, 2, 0.f, &damp_bad}), E, "g: damping must be finite and not negative");
  if (g_bad) { std::printf("map_grow_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("map_grow_checks_check: all ok\n");
  return 0;
}
