// bundle_map -- joint bundle adjustment on a data directory whose answer is known, beside the alternation: the start is that of
// adjust_map (the same seeded generator and flags: world.dat pushed, the poses of trajectory.dat pushed, the first and the last
// frame held at their ground truth), ONE vox_map_bundle call runs n_rounds Levenberg-Marquardt rounds whose reduced camera
// system is solved by matrix-free PCG, and ONE vo_map_adjust call with its defaults (6 sweeps of 2 + 2 rounds) runs from the
// same start on a second map.
//   usage: bundle_map <data dir> [--rounds=3] [--cg=64] [--tol=1e-8] [--lambda=1e-4] [--push-points=0.02] [--push-t=0.01]
//                     [--push-angles=0.005] [--seed=1]
// Printed: the cost per round as the call records it, and the total cost over ALL rows that hit an entry, evaluated on the host
// in double, at the start, after the joint call and after the alternation.  Exit 0 iff the joint call's status is OK and its
// final cost is below the one the alternation reaches.
#include <algorithm>
#include <cstring>
#include <random>

#include "known_common.hpp"

namespace {
// inv(G C) in double
void camera_in_map_inverse(const vo::Isometry3f& G, const vo::Isometry3f& C, double T[12]) {
  double R[9], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r + 3 * c] = (double)G(r, 0) * C(0, c) + (double)G(r, 1) * C(1, c) + (double)G(r, 2) * C(2, c);
    t[r] = (double)G(r, 0) * C(0, 3) + (double)G(r, 1) * C(1, 3) + (double)G(r, 2) * C(2, 3) + (double)G(r, 3);
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r + 3 * c] = R[c + 3 * r];
    T[9 + r] = -(R[3 * r] * t[0] + R[1 + 3 * r] * t[1] + R[2 + 3 * r] * t[2]);
  }
}

// v2t(dx) T in double (translation dx[0:3], R = Rx Ry Rz), rounded once
vo::Isometry3f pushed(const double dx[6], const double T[12]) {
  const double sx = std::sin(dx[3]), cx = std::cos(dx[3]), sy = std::sin(dx[4]), cy = std::cos(dx[4]), sz = std::sin(dx[5]), cz = std::cos(dx[5]);
  const double dR[9] = {cy * cz, sx * sy * cz + cx * sz, -cx * sy * cz + sx * sz, -cy * sz, -sx * sy * sz + cx * cz, cx * sy * sz + sx * cz,
                        sy, -sx * cy, cx * cy};
  vo::Isometry3f out = vo::Isometry3f::Identity();
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 3; ++r)
      out(r, c) = (float)(dR[r] * T[3 * c] + dR[r + 3] * T[1 + 3 * c] + dR[r + 6] * T[2 + 3 * c] + (c == 3 ? dx[r] : 0.0));
  return out;
}

struct Hit { int frame, row, entry; };

double total_cost(const std::vector<Hit>& hits, const std::vector<vo::Vector2fVector>& pixels, const vo::IsometryVector& poses,
                  const vo::Vector3fVector& pts, const vo::Matrix3f& K) {
  double total = 0;
  for (const Hit& h : hits) {
    const vo::Isometry3f& T = poses[(size_t)h.frame];
    const auto& p = pts[(size_t)h.entry];
    double pc[3], q[3];
    for (int r = 0; r < 3; ++r) pc[r] = (double)T(r, 0) * p[0] + (double)T(r, 1) * p[1] + (double)T(r, 2) * p[2] + (double)T(r, 3);
    for (int r = 0; r < 3; ++r) q[r] = (double)K(r, 0) * pc[0] + (double)K(r, 1) * pc[1] + (double)K(r, 2) * pc[2];
    const auto& m = pixels[(size_t)h.frame][(size_t)h.row];
    const double e0 = q[0] / q[2] - (double)m[0], e1 = q[1] / q[2] - (double)m[1];
    total += e0 * e0 + e1 * e1;
  }
  return total;
}
}  // namespace

int main(int argc, char* argv[]) {
  double push_points = 0.02, push_t = 0.01, push_angles = 0.005;
  unsigned seed = 1;
  vo::BundleOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--rounds=", 0) == 0) opt.n_rounds = std::atoi(s.c_str() + 9);
    else if (s.rfind("--cg=", 0) == 0) opt.n_cg = std::atoi(s.c_str() + 5);
    else if (s.rfind("--tol=", 0) == 0) opt.cg_tol = (float)std::atof(s.c_str() + 6);
    else if (s.rfind("--lambda=", 0) == 0) opt.lambda0 = (float)std::atof(s.c_str() + 9);
    else if (s.rfind("--push-points=", 0) == 0) push_points = std::atof(s.c_str() + 14);
    else if (s.rfind("--push-t=", 0) == 0) push_t = std::atof(s.c_str() + 9);
    else if (s.rfind("--push-angles=", 0) == 0) push_angles = std::atof(s.c_str() + 14);
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) {
    std::printf("usage: bundle_map <data dir> [--rounds=3] [--cg=64] [--tol=1e-8] [--lambda=1e-4] [--push-points=0.02] [--push-t=0.01] "
                "[--push-angles=0.005] [--seed=1]\n");
    return -1;
  }
  std::string path = pos[0];
  if (path.back() != '/') path.push_back('/');
  try {
    known::Dataset data;
    if (!known::load_dataset(path, data, false)) return -1;
    vo::Vector10fVector world_app;
    vo::Vector3fVector world_xyz;
    if (!vo::get_meas_content(path + "world.dat", world_app, world_xyz, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    const size_t F = data.meas_files.size();
    if (F < 2 || gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames (at least 2 needed)\n", gt.size(), F); return -1; }

    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    vo::Vector3fVector start = world_xyz;
    for (auto& p : start)
      for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + push_points * unit(rng));
    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> apps;
    vo::IsometryVector truth, poses0;
    std::vector<uint8_t> fixed(F, 0);
    fixed[0] = fixed[F - 1] = 1;
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      pixels.push_back(known::strip_id(meas_with_id));
      apps.push_back(appearances);
      double T[12], dx[6];
      camera_in_map_inverse(gt[f], data.cameraInRobot, T);
      for (int k = 0; k < 6; ++k) dx[k] = (k < 3 ? push_t : push_angles) * unit(rng);
      truth.push_back(pushed(zero, T));
      poses0.push_back(fixed[f] ? truth.back() : pushed(dx, T));
    }

    vo::DeviceMap joint((int)world_app.size()), alternated((int)world_app.size());
    joint.update(start, world_app);
    alternated.update(start, world_app);
    std::vector<Hit> hits;
    for (size_t f = 0; f < F; ++f) {
      const vo::IntPairVector pairs = joint.lookup(apps[f]);
      for (const auto& pr : pairs) hits.push_back(Hit{(int)f, pr.first, pr.second});
    }
    const vo::Camera cam = data.camera();
    const vo::Matrix3f K = cam.cameraMatrix();
    std::printf("map of %d entries, %zu frames, %zu observations: points pushed by up to %g, poses by up to %g / %g rad (seed %u), frames 0 and %zu held\n",
                joint.size(), F, hits.size(), push_points, push_t, push_angles, seed, F - 1);

    static const char* const names[6] = {"OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE"};
    const double cost_start = total_cost(hits, pixels, poses0, start, K);

    // the joint call
    vo::IsometryVector bundled = poses0;
    std::vector<vox_map_bundle_round> rounds;
    const vox_map_bundle_stats st = joint.bundle(cam, pixels, apps, bundled, &fixed, opt, &rounds);
    vo::Vector3fVector pts;
    vo::Vector10fVector unused;
    joint.read(pts, unused);
    const double cost_joint = total_cost(hits, pixels, bundled, pts, K);
    for (size_t r = 0; r < rounds.size(); ++r)
      std::printf("round %zu: cost %.6g, candidate %.6g, lambda %.3g, %d PCG iterations to |r| / |r0| = %.3g, %s\n", r, rounds[r].cost,
                  rounds[r].cost_candidate, rounds[r].lambda, rounds[r].cg_iterations, rounds[r].residual, rounds[r].accepted ? "accepted" : "rejected");
    std::printf("joint call: status %s, %d free frames, %d free landmarks, %d of %d rounds accepted, cost %.6g -> %.6g\n",
                st.status >= 0 && st.status < 6 ? names[st.status] : "?", st.n_free_frames, st.n_free_points, st.n_accepted, opt.n_rounds,
                st.cost_before, st.cost_after);

    // the alternation with its defaults from the same start
    vo::IsometryVector adjusted = poses0;
    const vo::AdjustOptions alt;
    alternated.adjust(cam, pixels, apps, adjusted, &fixed, alt);
    alternated.read(pts, unused);
    const double cost_alt = total_cost(hits, pixels, adjusted, pts, K);
    const bool below = cost_joint < cost_alt;
    std::printf("total cost: start %.6g, joint (%d rounds) %.6g, alternation (%d sweeps of %d + %d rounds) %.6g: the joint call ends %s the alternation\n",
                cost_start, opt.n_rounds, cost_joint, alt.n_sweeps, alt.pose_rounds, alt.point_rounds, cost_alt, below ? "below" : "NOT BELOW");
    return st.status == VOX_MAP_BUNDLE_OK && below ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "bundle_map: %s\n", e.what());
    return 2;
  }
}
