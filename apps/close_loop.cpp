// close_loop -- a loop closed on a data directory: the ground-truth chain is drifted by a seeded generator (a scale drift of
// 0.3 % per step, 0.4 % noise, 2 mrad / 2 mm noise, chained into similarities S_f), loop edges are taken between the frame pairs
// that ONE voe_map_covis call ranks highest beyond a gap of 50 frames, each loop edge is measured by vo_map_localise of its two
// frames in the map of world.dat (Z = T_j T_i^-1), ONE voe_pose_graph call distributes them over the chain with frame 0 held,
// and ONE voe_map_apply_correction call carries the correction into the map that belongs to the drifted chain (every landmark
// where the drifted pose of the first frame that sees it puts it).
// With --from-map the loop edges come from ONE voe_map_loops call on that drifted map and the drifted chain instead: no
// localisation in world.dat and no ranking on the host -- what a running system, which has only its own map, can do.
//   usage: close_loop <data dir> [--seed=1] [--loops=4] [--gap=50] [--jacobi] [--from-map]
// Printed: the loop edges, the optimiser's rounds, the camera-centre error and the map's distance to world.dat before and after.
// Exit 0 iff every call's status is OK and the median camera-centre error falls below a fifth of what it was (the float64
// restatement of the same experiment, tests/test_pose_graph_cpu.py, gives 0.054 of it).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <random>

#include "known_common.hpp"

namespace {
using M4 = std::array<double, 16>;                            // row-major 4x4
M4 ident() { M4 m{}; m[0] = m[5] = m[10] = m[15] = 1.0; return m; }
M4 mul(const M4& a, const M4& b) {
  M4 c{};
  for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) for (int j = 0; j < 4; ++j) c[4 * r + k] += a[4 * r + j] * b[4 * j + k];
  return c;
}
// the inverse of [M | t]: adjugate over determinant
M4 inv(const M4& a) {
  const double m00 = a[0], m01 = a[1], m02 = a[2], m10 = a[4], m11 = a[5], m12 = a[6], m20 = a[8], m21 = a[9], m22 = a[10];
  const double det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
  M4 o = ident();
  o[0] = (m11 * m22 - m12 * m21) / det; o[1] = (m02 * m21 - m01 * m22) / det; o[2] = (m01 * m12 - m02 * m11) / det;
  o[4] = (m12 * m20 - m10 * m22) / det; o[5] = (m00 * m22 - m02 * m20) / det; o[6] = (m02 * m10 - m00 * m12) / det;
  o[8] = (m10 * m21 - m11 * m20) / det; o[9] = (m01 * m20 - m00 * m21) / det; o[10] = (m00 * m11 - m01 * m10) / det;
  for (int r = 0; r < 3; ++r) o[4 * r + 3] = -(o[4 * r] * a[3] + o[4 * r + 1] * a[7] + o[4 * r + 2] * a[11]);
  return o;
}
M4 from(const vo::Isometry3f& T) { M4 m = ident(); for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = T(r, c); return m; }
M4 from(const vo::Similarity3f& S) { M4 m = ident(); for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = S(r, c); return m; }
vo::Similarity3f sim(const M4& m) {
  vo::Similarity3f S = vo::Similarity3f::Identity();
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) S.m[r + 4 * c] = (float)m[4 * r + c];
  return S;
}
// [c Rx(w0) Ry(w1) Rz(w2) | t]
M4 small(double c, const double w[3], const double t[3]) {
  const double sx = std::sin(w[0]), cx = std::cos(w[0]), sy = std::sin(w[1]), cy = std::cos(w[1]), sz = std::sin(w[2]), cz = std::cos(w[2]);
  const double R[9] = {cy * cz, -cy * sz, sy, sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy, -cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy};
  M4 m = ident();
  for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) m[4 * r + k] = c * R[3 * r + k]; m[4 * r + 3] = t[r]; }
  return m;
}
std::array<double, 3> centre(const M4& S) { const M4 i = inv(S); return {i[3], i[7], i[11]}; }
std::array<double, 3> move_point(const M4& S, const double p[3]) {
  return {S[0] * p[0] + S[1] * p[1] + S[2] * p[2] + S[3], S[4] * p[0] + S[5] * p[1] + S[6] * p[2] + S[7], S[8] * p[0] + S[9] * p[1] + S[10] * p[2] + S[11]};
}
double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  int n_loops = 4, gap = 50;
  bool from_map = false, loops_given = false;
  vo::PoseGraphOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--loops=", 0) == 0) { n_loops = std::atoi(s.c_str() + 8); loops_given = true; }
    else if (s.rfind("--gap=", 0) == 0) gap = std::atoi(s.c_str() + 6);
    else if (s == "--jacobi") opt.preconditioner = VOE_POSE_GRAPH_JACOBI;
    else if (s == "--from-map") from_map = true;
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) { std::printf("usage: close_loop <data dir> [--seed=1] [--loops=4] [--gap=50] [--jacobi] [--from-map]\n"); return -1; }
  std::string path = pos[0];
  if (path.back() != '/') path.push_back('/');
  try {
    known::Dataset data;
    if (!known::load_dataset(path, data, false)) return -1;
    vo::Vector10fVector world_app;
    vo::Vector3fVector world_xyz;
    if (!vo::get_meas_content(path + "world.dat", world_app, world_xyz, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    const size_t F = data.meas_files.size();
    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> apps;
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      pixels.push_back(known::strip_id(meas_with_id));
      apps.push_back(appearances);
    }
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    if (gt.size() < F || F < 2) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }
    std::vector<M4> G;                                        // ground truth: p_cam = G p_world
    for (size_t f = 0; f < F; ++f) G.push_back(from((gt[f] * data.cameraInRobot).inverse()));

    // the drifted chain and its odometry edges
    std::mt19937 rng(seed);
    std::normal_distribution<double> normal(0.0, 1.0);
    vo::PoseGraph graph;
    std::vector<M4> S{G[0]};
    for (size_t k = 0; k + 1 < F; ++k) {
      const double c = std::exp(0.003 + 0.004 * normal(rng));
      double w[3], t[3];
      for (double& x : w) x = 0.002 * normal(rng);
      for (double& x : t) x = 0.002 * normal(rng);
      const M4 z = mul(small(c, w, t), mul(G[k + 1], inv(G[k])));
      S.push_back(mul(z, S.back()));
      graph.addEdge((int)k, (int)k + 1, sim(z));
    }

    // the loop edges: the pairs the covisibility ranks highest beyond the gap, measured by localising both frames in world.dat
    vo::DeviceMap world((int)world_app.size());
    world.update(world_xyz, world_app);
    std::vector<std::pair<int, std::pair<int, int>>> ranked;
    if (!from_map) {                                          // (--from-map neither ranks on the host nor localises in world.dat)
      const vo::Covisibility cov = world.covisibility(apps);
      for (size_t i = 0; i < F; ++i)
        for (size_t j = i + (size_t)gap + 1; j < F; ++j) ranked.push_back({-cov.shared(i, j), {(int)i, (int)j}});
      std::sort(ranked.begin(), ranked.end());
    }
    const vo::Camera cam = data.camera();
    int taken = 0;
    bool ok = true;
    for (const auto& r : ranked) {
      if (taken >= n_loops) break;
      const int i = r.second.first, j = r.second.second;
      vo_map_localise_stats si{}, sj{};
      const vo::Isometry3f Ti = world.localise(cam, pixels[(size_t)i], apps[(size_t)i], vo::LocaliseOptions(), &si);
      const vo::Isometry3f Tj = world.localise(cam, pixels[(size_t)j], apps[(size_t)j], vo::LocaliseOptions(), &sj);
      std::printf("loop %d - %d: %d shared landmarks, localised %s / %s\n", i, j, -r.first, vo::localise_status_name(si.status), vo::localise_status_name(sj.status));
      if (si.status != VO_MAP_LOCALISE_OK || sj.status != VO_MAP_LOCALISE_OK) continue;
      graph.addEdge(i, j, sim(mul(from(Tj), inv(from(Ti)))));
      ++taken;
    }
    if (!from_map && taken == 0) { std::printf("no loop edge could be measured\n"); return 1; }

    // the map that belongs to the drifted chain: every landmark where the drifted pose of the first frame that sees it puts it
    std::vector<int32_t> first(world_xyz.size(), -1);
    for (size_t f = 0; f < F; ++f) {
      std::vector<int32_t> ent;
      world.lookup(apps[f], nullptr, &ent);
      for (int32_t e : ent) if (e >= 0 && first[(size_t)e] < 0) first[(size_t)e] = (int32_t)f;
    }
    vo::Vector3fVector drifted = world_xyz;
    for (size_t e = 0; e < drifted.size(); ++e) {
      if (first[e] < 0) continue;
      const double p[3] = {world_xyz[e][0], world_xyz[e][1], world_xyz[e][2]};
      const auto q = move_point(mul(inv(S[(size_t)first[e]]), G[(size_t)first[e]]), p);
      for (int k = 0; k < 3; ++k) drifted[e][k] = (float)q[(size_t)k];
    }
    vo::DeviceMap map((int)world_app.size());
    map.update(drifted, world_app);
    std::vector<vo::Similarity3f> S_old, S_new;
    for (const M4& s : S) S_old.push_back(sim(s));

    // --from-map: the loop edges as the drifted map itself shows them, found and measured by one call
    if (from_map) {
      vo::LoopsOptions lo;
      lo.gap = gap;
      if (loops_given) lo.max_loops = n_loops;
      const vo::MapLoops found = map.loops(cam, pixels, apps, S_old, lo);
      std::printf("voe_map_loops: %d candidates, %d survivors, %d slots, %d measured\n", found.stats.n_candidates, found.stats.n_survivors, found.stats.n_slots,
                  found.stats.n_ok);
      for (const voe_map_loop_record& r : found.loops)
        if (r.status != VOE_MAP_LOOP_EMPTY)
          std::printf("loop %d - %d: %d landmarks in the band, %d pairs, %d RANSAC inliers, %d solver inliers, %s\n", r.i, r.j, r.c, r.n_pairs, r.ransac_inliers,
                      r.num_inliers, vo::loop_status_name(r.status));
      graph.addLoops(found);
      taken = found.stats.n_ok;
      if (taken == 0) { std::printf("no loop edge could be measured\n"); return 1; }
    }

    // optimise, then carry the correction into the map
    S_new = S_old;
    std::vector<uint8_t> fixed(F, 0);
    fixed[0] = 1;
    std::vector<voe_pose_graph_round> rounds;
    const voe_pose_graph_stats st = graph.optimise(S_new, fixed, opt, nullptr, nullptr, &rounds);
    for (size_t r = 0; r < rounds.size(); ++r)
      std::printf("round %zu: cost %.6g -> %.6g, lambda %.3g, %d PCG iterations, %s\n", r, rounds[r].cost, rounds[r].cost_candidate, rounds[r].lambda,
                  rounds[r].cg_iterations, rounds[r].accepted ? "accepted" : "rejected");
    std::printf("pose graph of %d frames, %d edges (%d loops): status %s, cost %.6g -> %.6g\n", st.n_frames, st.n_edges, taken, vo::pose_graph_status_name(st.status),
                st.cost_before, st.cost_after);
    ok = ok && st.status == VOE_POSE_GRAPH_OK;
    std::vector<int32_t> ref;
    const voe_map_apply_stats as = map.applyCorrection(apps, S_old, S_new, false, &ref);
    std::printf("correction applied: %d entries, %d seen, %d moved\n", as.n_entries, as.n_seen, as.n_moved);
    bool same_ref = ref.size() == first.size();
    for (size_t e = 0; same_ref && e < ref.size(); ++e) same_ref = ref[e] == first[e];
    ok = ok && same_ref && as.n_moved > 0;
    if (!same_ref) std::printf("the reference frames DISAGREE with the first frame that sees each landmark\n");

    // the errors: camera centres against the ground truth, the map's seen landmarks against world.dat
    std::vector<double> before, after;
    double max_b = 0.0, max_a = 0.0;
    for (size_t f = 0; f < F; ++f) {
      const auto g = centre(G[f]), b = centre(S[f]), a = centre(from(S_new[f]));
      const double db = std::sqrt((b[0] - g[0]) * (b[0] - g[0]) + (b[1] - g[1]) * (b[1] - g[1]) + (b[2] - g[2]) * (b[2] - g[2]));
      const double da = std::sqrt((a[0] - g[0]) * (a[0] - g[0]) + (a[1] - g[1]) * (a[1] - g[1]) + (a[2] - g[2]) * (a[2] - g[2]));
      before.push_back(db); after.push_back(da);
      max_b = std::max(max_b, db); max_a = std::max(max_a, da);
    }
    double rms_b = 0.0, rms_a = 0.0;
    int n_seen = 0;
    for (size_t f = 0; f < F; ++f) {                           // (read back through the lookup: the points of every hit)
      vo::Vector3fVector pts;
      std::vector<int32_t> ent;
      const vo::IntPairVector hits = map.lookup(apps[f], &pts, &ent);
      for (size_t k = 0; k < hits.size(); ++k) {
        const size_t e = (size_t)hits[k].second;
        if (first[e] != (int32_t)f) continue;                 // every seen landmark once, at its reference frame
        double sb = 0.0, sa = 0.0;
        for (int c = 0; c < 3; ++c) {
          sb += ((double)drifted[e][c] - world_xyz[e][c]) * ((double)drifted[e][c] - world_xyz[e][c]);
          sa += ((double)pts[k][c] - world_xyz[e][c]) * ((double)pts[k][c] - world_xyz[e][c]);
        }
        rms_b += sb; rms_a += sa; ++n_seen;
        first[e] = -2;
      }
    }
    const double mb = median(before), ma = median(after);
    std::printf("camera-centre error: max %.3f -> %.3f, median %.3f -> %.3f (%.3f of it)\n", max_b, max_a, mb, ma, mb > 0 ? ma / mb : 0.0);
    std::printf("map, %d seen landmarks against world.dat: rms %.4f -> %.4f\n", n_seen, std::sqrt(rms_b / std::max(n_seen, 1)), std::sqrt(rms_a / std::max(n_seen, 1)));
    const bool fell = ma < mb / 5.0;
    std::printf("%s\n", ok && fell ? "the loop is closed" : "the loop is NOT closed");
    return ok && fell ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "close_loop: %s\n", e.what());
    return 2;
  }
}
