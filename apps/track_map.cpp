// track_map -- the frames of a data directory TRACKED against the map of its world.dat: the tracker voe_map_guided exists for.
// Every appearance of every frame is pushed by seeded Gaussian noise, so bit equality -- the association the map calls had --
// finds nothing.  Per frame:
//   1. the prior is predicted from the last two solved poses at constant velocity, T-1 T-2^-1 T-1 (p_cam = T p_map), its
//      rotation re-orthonormalised; with one solved pose it is that pose;
//   2. ONE voe_map_guided associates the frame with the map inside a pixel window around the prior's projections and returns the
//      rows canonicalised;
//   3. vo_map_localise with n_hypotheses == 0 and T0 = the prior solves the pose on the canonical rows (tracking against the map);
//   4. when that status is not OK -- the first frame, which has no prior, and the trajectory's turns, where constant velocity is
//      off by up to 250 px -- the frame is relocalised GLOBALLY: voe_map_nearest over the whole map, then vo_map_localise with
//      RANSAC.  These frames are counted.
//   usage: track_map <data dir> [--px=8] [--sigma=0.005] [--radius=0.1] [--ratio=0.8] [--seed=1]
// Exit 0 iff every frame ends OK and within 1e-4 of trajectory.dat (largest absolute entry difference of the robot pose
// inv(T) inv(C), the bound of apps/localise).
#include <cstring>
#include <random>

#include "known_common.hpp"

namespace {
// inv(T) inv(C) in double against the ground-truth pose: largest absolute entry difference of the 3 x 4 (apps/localise.cpp)
double robot_pose_error(const vo::Isometry3f& T, const vo::Isometry3f& C, const vo::Isometry3f& gt) {
  auto inv = [](const vo::Isometry3f& X, double R[9], double t[3]) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r + 3 * c] = X(c, r);
    for (int r = 0; r < 3; ++r) t[r] = -(R[r] * X(0, 3) + R[r + 3] * X(1, 3) + R[r + 6] * X(2, 3));
  };
  double Ra[9], ta[3], Rb[9], tb[3], err = 0;
  inv(T, Ra, ta);
  inv(C, Rb, tb);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      err = std::fmax(err, std::fabs(Ra[r] * Rb[3 * c] + Ra[r + 3] * Rb[1 + 3 * c] + Ra[r + 6] * Rb[2 + 3 * c] - (double)gt(r, c)));
    err = std::fmax(err, std::fabs(Ra[r] * tb[0] + Ra[r + 3] * tb[1] + Ra[r + 6] * tb[2] + ta[r] - (double)gt(r, 3)));
  }
  return err;
}

// The constant-velocity prediction A B^-1 A in double, its rotation brought back onto SO(3) (Gram-Schmidt on the columns).  A PICP
// round multiplies the pose by a rigid update, so whatever the rotation block lacks of being orthonormal survives every solve; the
// product (with the transpose for the inverse) would hand on twice the last pose's defect plus the one before, frame after frame.
vo::Isometry3f predict(const vo::Isometry3f& A, const vo::Isometry3f& B) {
  double a[16], bi[16], m[16], p[16];
  for (int k = 0; k < 16; ++k) { a[k] = A.data()[k]; bi[k] = 0; }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) bi[r + 4 * c] = B(c, r);
  for (int r = 0; r < 3; ++r) bi[r + 12] = -(bi[r] * B(0, 3) + bi[r + 4] * B(1, 3) + bi[r + 8] * B(2, 3));
  bi[15] = 1;
  auto mul = [](const double* x, const double* y, double* z) {
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 4; ++r) z[r + 4 * c] = x[r] * y[4 * c] + x[r + 4] * y[1 + 4 * c] + x[r + 8] * y[2 + 4 * c] + x[r + 12] * y[3 + 4 * c];
  };
  mul(a, bi, m);
  mul(m, a, p);
  for (int c = 0; c < 3; ++c) {
    for (int k = 0; k < c; ++k) {
      const double d = p[4 * c] * p[4 * k] + p[1 + 4 * c] * p[1 + 4 * k] + p[2 + 4 * c] * p[2 + 4 * k];
      for (int r = 0; r < 3; ++r) p[r + 4 * c] -= d * p[r + 4 * k];
    }
    const double n = std::sqrt(p[4 * c] * p[4 * c] + p[1 + 4 * c] * p[1 + 4 * c] + p[2 + 4 * c] * p[2 + 4 * c]);
    for (int r = 0; r < 3; ++r) p[r + 4 * c] /= n;
  }
  vo::Isometry3f out = vo::Isometry3f::Identity();
  for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) out(r, c) = (float)p[r + 4 * c];
  return out;
}
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  double sigma = 0.005;
  vo::GuidedOptions guided;
  guided.radius_px = 8.f;
  guided.radius = 0.1f;
  guided.ratio = 0.8f;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--sigma=", 0) == 0) sigma = std::atof(s.c_str() + 8);
    else if (s.rfind("--px=", 0) == 0) guided.radius_px = (float)std::atof(s.c_str() + 5);
    else if (s.rfind("--radius=", 0) == 0) guided.radius = (float)std::atof(s.c_str() + 9);
    else if (s.rfind("--ratio=", 0) == 0) guided.ratio = (float)std::atof(s.c_str() + 8);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || !(sigma >= 0)) { std::printf("usage: track_map <data dir> [--px=8] [--sigma=0.005] [--radius=0.1] [--ratio=0.8] [--seed=1]\n"); return -1; }
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
    if (F < 1 || gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }
    const vo::Camera cam = data.camera();
    vo::DeviceMap map((int)world_app.size());
    map.update(world_xyz, world_app);
    std::printf("map of %d entries; every appearance pushed by N(0, %g) (seed %u); window %g px, radius %g, ratio %g\n", map.size(), sigma, seed,
                guided.radius_px, guided.radius, guided.ratio);

    vo::NearestOptions global;
    global.radius = guided.radius;
    global.ratio = guided.ratio;
    vo::LocaliseOptions from_prior;                         // no RANSAC: every hit is handed on, the start is T0
    from_prior.ransac.n_hypotheses = 0;
    const vo::LocaliseOptions from_scratch;

    std::mt19937 rng(seed);
    std::normal_distribution<float> noise(0.f, (float)sigma);
    vo::IsometryVector solved;
    size_t n_fallback = 0, n_bad = 0;
    long long n_gated = 0, n_rows = 0;
    double worst = 0;
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      const vo::Vector2fVector pixels = known::strip_id(meas_with_id);
      if (sigma > 0)
        for (auto& a : appearances) for (int k = 0; k < 10; ++k) a[k] += noise(rng);

      vo_map_localise_stats st{};
      st.status = VO_MAP_LOCALISE_FEW_MATCHES;
      vo::Isometry3f T = vo::Isometry3f::Identity();
      int n_matched = 0;
      double prior_err = -1;
      if (!solved.empty()) {
        const vo::Isometry3f& T1 = solved.back();
        const vo::Isometry3f prior = predict(T1, solved.size() >= 2 ? solved[solved.size() - 2] : T1);
        prior_err = robot_pose_error(prior, data.cameraInRobot, gt[f]);
        const vo::MapGuided g = map.guided(cam, {pixels}, {appearances}, {prior}, guided);
        n_matched = g.stats.n_matched;
        n_gated += g.stats.n_gated;
        n_rows += g.stats.n_live;
        T = map.localise(cam, pixels, g.canonical[0], from_prior, &st, &prior);
      }
      const bool fallback = st.status != VO_MAP_LOCALISE_OK;
      if (fallback) {
        ++n_fallback;
        const vo::MapNearest r = map.nearest({appearances}, global);
        n_matched = r.stats.n_matched;
        T = map.localise(cam, pixels, r.canonical[0], from_scratch, &st);
      }
      const double err = robot_pose_error(T, data.cameraInRobot, gt[f]);
      worst = std::fmax(worst, err);
      const bool ok = st.status == VO_MAP_LOCALISE_OK && err < 1e-4;
      n_bad += !ok;
      std::printf("%s: %zu rows, prior diff %.3g, %d matched %s, %d inliers, %s, diff %.3g\n", data.meas_files[f].c_str(), pixels.size(), prior_err,
                  n_matched, fallback ? "GLOBALLY" : "in the window", st.num_inliers, vo::localise_status_name(st.status), err);
      solved.push_back(T);
    }
    std::printf("%zu frames, %zu took the fallback (the first has no prior); %.2f entries tested per tracked row; %zu not OK or beyond 1e-4; "
                "largest pose difference to trajectory.dat: %.3g\n", F, n_fallback, n_rows ? (double)n_gated / (double)n_rows : 0.0, n_bad, worst);
    return n_bad == 0 ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "track_map: %s\n", e.what());
    return 2;
  }
}
