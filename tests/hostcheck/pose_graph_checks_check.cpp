// pose_graph_checks_check -- the refusals of voe_pose_graph* that make no HIP call (visual-odometry_amd/csrc/map_checks.h:
// pose_graph_check and map_apply_check) under the host sanitizers, without a GPU and without the library: a stand-alone program over the header
// alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/pose_graph_checks_check.cpp -o pose_graph_checks_check && ./pose_graph_checks_check
//   (ends with "pose_graph_checks_check: all ok")
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
  alignas(8) static char dev[64];                      // stands for the device's arrays: never dereferenced on the host
  const voe_pose_graph_params ok{8, 8, 1e-6f, 1e-4f, 0.f, 1, VOE_POSE_GRAPH_CHAIN};
  const PoseGraphPtrs all{dev, dev, dev, dev, dev, dev, dev, dev};
  const PoseGraphPtrs least{dev, dev, dev, nullptr, nullptr, nullptr, nullptr, dev};
  const char* fn = "g";
  auto with = [&](auto edit) { voe_pose_graph_params p = ok; edit(p); return p; };
  auto ptrs = [&](auto edit) { PoseGraphPtrs d = all; edit(d); return d; };
  struct Row { const char* what; int n_frames, n_edges; PoseGraphPtrs d; voe_pose_graph_params p; int code; const char* msg; };
  const Row rows[] = {
      {"the defaults, every array", 5, 7, all, ok, VO_OK, ""},
      {"the defaults, no optional array", 5, 7, least, ok, VO_OK, ""},
      {"one frame, no edge, no edge arrays", 1, 0, ptrs([](PoseGraphPtrs& d) { d.edges = nullptr; d.Z16 = nullptr; }), ok, VO_OK, ""},
      {"null d_S16", 5, 7, ptrs([](PoseGraphPtrs& d) { d.S16 = nullptr; }), ok, E, "g: null argument"},
      {"null d_stats", 5, 7, ptrs([](PoseGraphPtrs& d) { d.stats = nullptr; }), ok, E, "g: null argument"},
      {"n_frames 0", 0, 7, all, ok, E, "g: n_frames must be at least 1"},
      {"n_frames INT_MIN", INT_MIN, 7, all, ok, E, "g: n_frames must be at least 1"},
      {"n_edges -1", 5, -1, all, ok, E, "g: negative n_edges"},
      {"n_frames 2^24 + 1", (1 << 24) + 1, 7, all, ok, E, "g: more than 2^24 frames or edges"},
      {"n_edges INT_MAX", 5, INT_MAX, all, ok, E, "g: more than 2^24 frames or edges"},
      {"null edges with edges", 5, 7, ptrs([](PoseGraphPtrs& d) { d.edges = nullptr; }), ok, E, "g: null edges or measurements"},
      {"null measurements with edges", 5, 7, ptrs([](PoseGraphPtrs& d) { d.Z16 = nullptr; }), ok, E, "g: null edges or measurements"},
      {"d_S16 2 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.S16 = dev + 2; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_S16 4 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.S16 = dev + 4; }), ok, VO_OK, ""},
      {"d_weights 1 byte off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.weights = dev + 1; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_edge_status_out 2 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.edge_status = dev + 2; }), ok, E, "g: float32 and int32 arrays must be 4-byte aligned"},
      {"d_edge_cost_out 4 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.edge_cost = dev + 4; }), ok, E, "g: d_edge_cost_out, d_rounds_out and d_stats must be 8-byte aligned"},
      {"d_rounds_out 4 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.rounds = dev + 4; }), ok, E, "g: d_edge_cost_out, d_rounds_out and d_stats must be 8-byte aligned"},
      {"d_stats 4 bytes off", 5, 7, ptrs([](PoseGraphPtrs& d) { d.stats = dev + 4; }), ok, E, "g: d_edge_cost_out, d_rounds_out and d_stats must be 8-byte aligned"},
      {"n_rounds 0 (evaluates)", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_rounds = 0; }), VO_OK, ""},
      {"n_rounds -1", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_rounds = -1; }), E, "g: negative n_rounds"},
      {"n_cg 1", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_cg = 1; }), VO_OK, ""},
      {"n_cg 0", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_cg = 0; }), E, "g: n_cg must be at least 1"},
      {"cg_tol 0", 5, 7, all, with([](voe_pose_graph_params& p) { p.cg_tol = 0.f; }), VO_OK, ""},
      {"cg_tol -1", 5, 7, all, with([](voe_pose_graph_params& p) { p.cg_tol = -1.f; }), E, "g: cg_tol must be finite and not negative"},
      {"cg_tol NaN", 5, 7, all, with([](voe_pose_graph_params& p) { p.cg_tol = NAN; }), E, "g: cg_tol must be finite and not negative"},
      {"lambda0 0", 5, 7, all, with([](voe_pose_graph_params& p) { p.lambda0 = 0.f; }), VO_OK, ""},
      {"lambda0 inf", 5, 7, all, with([](voe_pose_graph_params& p) { p.lambda0 = INFINITY; }), E, "g: lambda0 must be finite and not negative"},
      {"huber -0.5", 5, 7, all, with([](voe_pose_graph_params& p) { p.huber = -0.5f; }), E, "g: huber must be finite and not negative"},
      {"huber NaN", 5, 7, all, with([](voe_pose_graph_params& p) { p.huber = NAN; }), E, "g: huber must be finite and not negative"},
      {"65536 steps", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_rounds = 6553; p.n_cg = 8; }), VO_OK, ""},
      {"65540 steps", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_rounds = 6554; p.n_cg = 8; }), E,
       "g: n_rounds * (n_cg + 2) above 65536 (the launches of a call are a fixed sequence)"},
      {"INT_MAX rounds of INT_MAX iterations (no overflow)", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_rounds = INT_MAX; p.n_cg = INT_MAX; }), E,
       "g: n_rounds * (n_cg + 2) above 65536 (the launches of a call are a fixed sequence)"},
      {"JACOBI", 5, 7, all, with([](voe_pose_graph_params& p) { p.preconditioner = VOE_POSE_GRAPH_JACOBI; }), VO_OK, ""},
      {"preconditioner 2", 5, 7, all, with([](voe_pose_graph_params& p) { p.preconditioner = 2; }), E, "g: unknown preconditioner 2"},
      {"preconditioner -1", 5, 7, all, with([](voe_pose_graph_params& p) { p.preconditioner = -1; }), E, "g: unknown preconditioner -1"},
      {"a null pointer before n_frames", 0, 7, ptrs([](PoseGraphPtrs& d) { d.S16 = nullptr; }), ok, E, "g: null argument"},
      {"n_frames before the alignment", 0, 7, ptrs([](PoseGraphPtrs& d) { d.stats = dev + 4; }), ok, E, "g: n_frames must be at least 1"},
      {"the alignment before the parameters", 5, 7, ptrs([](PoseGraphPtrs& d) { d.stats = dev + 4; }), with([](voe_pose_graph_params& p) { p.n_cg = 0; }), E,
       "g: d_edge_cost_out, d_rounds_out and d_stats must be 8-byte aligned"},
      {"n_cg before the preconditioner", 5, 7, all, with([](voe_pose_graph_params& p) { p.n_cg = 0; p.preconditioner = 9; }), E, "g: n_cg must be at least 1"},
  };
  for (const Row& r : rows) expect(r.what, pose_graph_check(fn, r.n_frames, r.n_edges, r.d, &r.p), r.code, r.msg);
  expect("null params", pose_graph_check(fn, 5, 7, all, nullptr), E, "g: null argument");
  // ---- voe_map_apply_correction*: map_apply_check ----
  const float* app = reinterpret_cast<const float*>(dev);
  const float* S = reinterpret_cast<const float*>(dev + 8);
  expect("apply: the least", map_apply_check(fn, 3, app, 4, 4, S, S, nullptr, dev), VO_OK, "");
  expect("apply: no rows, no appearances", map_apply_check(fn, 3, nullptr, 0, 0, S, S, dev, dev), VO_OK, "");
  expect("apply: null S_old", map_apply_check(fn, 3, app, 4, 4, nullptr, S, nullptr, dev), E, "g: null argument");
  expect("apply: null d_stats", map_apply_check(fn, 3, app, 4, 4, S, S, nullptr, nullptr), E, "g: null argument");
  expect("apply: n_frames 0", map_apply_check(fn, 0, app, 4, 4, S, S, nullptr, dev), E, "g: n_frames 0 outside 1 .. 65535 (the frame is a grid dimension)");
  expect("apply: n_frames 65536", map_apply_check(fn, 65536, app, 4, 4, S, S, nullptr, dev), E, "g: n_frames 65536 outside 1 .. 65535 (the frame is a grid dimension)");
  expect("apply: n_max -1", map_apply_check(fn, 3, app, 4, -1, S, S, nullptr, dev), E, "g: negative row count");
  expect("apply: null appearances", map_apply_check(fn, 3, nullptr, 4, 4, S, S, nullptr, dev), E, "g: null appearances");
  expect("apply: d_app 4 bytes off", map_apply_check(fn, 3, reinterpret_cast<const float*>(dev + 4), 4, 4, S, S, nullptr, dev), E, "g: device arrays must be 8-byte aligned");
  expect("apply: d_stats 4 bytes off", map_apply_check(fn, 3, app, 4, 4, S, S, nullptr, dev + 4), E, "g: device arrays must be 8-byte aligned");
  expect("apply: a matrix array 2 bytes off", map_apply_check(fn, 3, app, 4, 4, reinterpret_cast<const float*>(dev + 2), S, nullptr, dev), E,
         "g: the matrices and d_ref_frame_out must be 4-byte aligned");
  expect("apply: d_ref_frame_out 4 bytes off (allowed)", map_apply_check(fn, 3, app, 4, 4, S, S, dev + 4, dev), VO_OK, "");
  expect("apply: a stride below n_max", map_apply_check(fn, 3, app, 3, 4, S, S, nullptr, dev), E, "g: a stride is smaller than n_max");
  expect("apply: 2^30 + rows", map_apply_check(fn, 65535, app, 20000, 20000, S, S, nullptr, dev), E, "g: more than 2^30 rows in one call");
  expect("apply: the null pointer before n_frames", map_apply_check(fn, 0, app, 4, 4, nullptr, S, nullptr, dev), E, "g: null argument");
  if (g_bad) { std::printf("pose_graph_checks_check: %d FAILED\n", g_bad); return 1; }
  std::printf("pose_graph_checks_check: all ok\n");
  return 0;
}
