// adjust_map -- block-coordinate bundle adjustment on a data directory whose answer is known: the map is world.dat with every
// point pushed off by a seeded amount, the poses are those of trajectory.dat pushed off by v2t(seeded translation and angles),
// the first and the last frame are held at their ground truth (the gauge), and ONE vo_map_adjust call alternates the pose half
// and the point half n_sweeps times.
//   usage: adjust_map <data dir> [--sweeps=6] [--rounds=2] [--push-points=0.02] [--push-t=0.01] [--push-angles=0.005] [--seed=1]
// Self-check: next to the composed call, the explicit loop of DeviceMap::refinePoses and DeviceMap::refine runs on a second map
// from the same start, and the total cost over ALL rows that hit an entry is evaluated on the host, in double, after every
// half-sweep.  Printed: that cost, the statuses of the last sweep, the median pose error (largest entry of T - T_gt) and the
// median point error (distance to world.dat over the OK landmarks) at the start and at the end.  Exit 0 iff the total cost
// never rose, both medians fell below the start's, and the composed call left the same bytes as the explicit loop.
// Alternation is a descent, not a fast one: expect the cost to fall by orders of magnitude and the errors by a factor of 5 to 10
// in six sweeps, not to the data's floor.
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

double median(std::vector<double> v) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
}  // namespace

int main(int argc, char* argv[]) {
  double push_points = 0.02, push_t = 0.01, push_angles = 0.005;
  unsigned seed = 1;
  vo::AdjustOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--sweeps=", 0) == 0) opt.n_sweeps = std::atoi(s.c_str() + 9);
    else if (s.rfind("--rounds=", 0) == 0) opt.pose_rounds = opt.point_rounds = std::atoi(s.c_str() + 9);
    else if (s.rfind("--push-points=", 0) == 0) push_points = std::atof(s.c_str() + 14);
    else if (s.rfind("--push-t=", 0) == 0) push_t = std::atof(s.c_str() + 9);
    else if (s.rfind("--push-angles=", 0) == 0) push_angles = std::atof(s.c_str() + 14);
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) {
    std::printf("usage: adjust_map <data dir> [--sweeps=6] [--rounds=2] [--push-points=0.02] [--push-t=0.01] [--push-angles=0.005] [--seed=1]\n");
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

    vo::DeviceMap composed((int)world_app.size()), looped((int)world_app.size());
    composed.update(start, world_app);
    looped.update(start, world_app);
    std::vector<Hit> hits;
    for (size_t f = 0; f < F; ++f) {
      const vo::IntPairVector pairs = composed.lookup(apps[f]);
      for (const auto& pr : pairs) hits.push_back(Hit{(int)f, pr.first, pr.second});
    }
    const vo::Camera cam = data.camera();
    const vo::Matrix3f K = cam.cameraMatrix();
    std::printf("map of %d entries, %zu frames, %zu observations: points pushed by up to %g, poses by up to %g / %g rad (seed %u), frames 0 and %zu held\n",
                composed.size(), F, hits.size(), push_points, push_t, push_angles, seed, F - 1);

    // the explicit loop, with the total cost after every half-sweep
    vo::IsometryVector poses = poses0;
    vo::Vector3fVector pts = start;
    vo::Vector10fVector unused;
    vo::PoseRefineOptions po; po.n_rounds = opt.pose_rounds; po.min_obs = opt.min_obs_pose; po.huber_px = opt.huber_px; po.damping = opt.damping;
    vo::RefineOptions ro; ro.n_rounds = opt.point_rounds; ro.min_obs = opt.min_obs_point; ro.huber_px = opt.huber_px; ro.damping = opt.damping;
    double cost = total_cost(hits, pixels, poses, pts, K);
    const double cost_start = cost;
    bool never_rose = true;
    std::printf("total cost: %.6g", cost);
    for (int s = 0; s < opt.n_sweeps; ++s) {
      looped.refinePoses(cam, pixels, apps, poses, &fixed, po);
      double c = total_cost(hits, pixels, poses, pts, K);
      never_rose = never_rose && c <= cost; cost = c;
      std::printf(" -> %.6g", cost);
      looped.refine(cam, pixels, apps, poses, ro);
      looped.read(pts, unused);
      c = total_cost(hits, pixels, poses, pts, K);
      never_rose = never_rose && c <= cost; cost = c;
      std::printf(" -> %.6g", cost);
    }
    std::printf("\n");

    // the composed call from the same start
    vo::IsometryVector adjusted = poses0;
    std::vector<vo_map_adjust_stats> sweeps;
    std::vector<int32_t> pose_status, point_status;
    composed.adjust(cam, pixels, apps, adjusted, &fixed, opt, &sweeps, &pose_status, &point_status);
    vo::Vector3fVector adjusted_pts;
    composed.read(adjusted_pts, unused);
    bool same = adjusted_pts.size() == pts.size();
    for (size_t e = 0; same && e < pts.size(); ++e) same = std::memcmp(&adjusted_pts[e], &pts[e], 12) == 0;
    for (size_t f = 0; same && f < F; ++f) same = std::memcmp(adjusted[f].data(), poses[f].data(), 64) == 0;

    const vo_map_adjust_stats& last = sweeps.back();
    std::printf("last sweep, poses:");
    for (int k = 0; k < 6; ++k) std::printf(" %s %d", vo::pose_refine_status_name(k), last.poses.by_status[k]);
    std::printf("; points:");
    for (int k = 0; k < 6; ++k) std::printf(" %s %d", vo::refine_status_name(k), last.points.by_status[k]);
    std::vector<double> pe0, pe1, qe0, qe1;
    for (size_t f = 0; f < F; ++f) {
      double a = 0, b = 0;
      for (int k = 0; k < 16; ++k) {
        a = std::fmax(a, std::fabs((double)poses0[f].data()[k] - (double)truth[f].data()[k]));
        b = std::fmax(b, std::fabs((double)adjusted[f].data()[k] - (double)truth[f].data()[k]));
      }
      pe0.push_back(a); pe1.push_back(b);
    }
    for (size_t e = 0; e < adjusted_pts.size() && e < world_xyz.size(); ++e) {
      if (point_status[e] != VO_MAP_REFINE_OK) continue;
      double a = 0, b = 0;
      for (int k = 0; k < 3; ++k) {
        a += std::pow((double)start[e][k] - (double)world_xyz[e][k], 2); b += std::pow((double)adjusted_pts[e][k] - (double)world_xyz[e][k], 2);
      }
      qe0.push_back(std::sqrt(a)); qe1.push_back(std::sqrt(b));
    }
    const bool better = median(pe1) < median(pe0) && median(qe1) < median(qe0);
    std::printf("\nmedian pose error %.4g -> %.4g, median point error %.4g -> %.4g over %zu OK landmarks\n", median(pe0), median(pe1), median(qe0),
                median(qe1), qe0.size());
    std::printf("total cost %.6g -> %.6g: it %s; the composed call %s the explicit loop bit for bit\n", cost_start, cost,
                never_rose ? "never rose" : "ROSE", same ? "equals" : "DIFFERS FROM");
    return never_rose && better && same ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "adjust_map: %s\n", e.what());
    return 2;
  }
}
