// associate_map -- frames whose appearances are NOT copies of the map's: every row of every frame of a data directory is pushed
// by seeded Gaussian noise, associated with the map by voe_map_nearest (the nearest entry within a radius) and handed on as the
// canonical rows that call returns; the map calls behind it then have to give what they give on the clean files.
//   usage: associate_map <data dir> [--tracks] [--sigma=0.005] [--radius=0.1] [--ratio=0.8] [--seed=1]
// Default: the map is world.dat; all frames are canonicalised in ONE call and localised in one vo_map_localise_batch_dev.  Exit 0
//   iff every frame's canonical rows equal the clean file's bytes and every pose lies within 1e-4 of trajectory.dat.
// --tracks: no map positions are used.  A DICTIONARY map is filled frame by frame -- voe_map_nearest of the frame against the
//   dictionary, then an update with the canonical rows (the points are dummies) --, a second pass canonicalises all frames against
//   the finished dictionary, and voe_map_grow from an EMPTY map on the canonical frames has to add the landmarks it adds on the
//   clean frames (grow_map --from-empty), points byte for byte: grouping and order are the same, and positions do not depend on
//   descriptor values.
#include <cmath>
#include <cstring>
#include <random>

#include "known_common.hpp"

namespace {
// inv(T) inv(C) in double against the ground-truth pose: largest absolute entry difference of the 3 x 4 (as apps/localise.cpp)
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
// inv(G C) in double (as apps/grow_map.cpp)
vo::Isometry3f camera_in_map_inverse(const vo::Isometry3f& G, const vo::Isometry3f& C) {
  double R[9], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r + 3 * c] = (double)G(r, 0) * C(0, c) + (double)G(r, 1) * C(1, c) + (double)G(r, 2) * C(2, c);
    t[r] = (double)G(r, 0) * C(0, 3) + (double)G(r, 1) * C(1, 3) + (double)G(r, 2) * C(2, 3) + (double)G(r, 3);
  }
  vo::Isometry3f T = vo::Isometry3f::Identity();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T(r, c) = (float)R[c + 3 * r];
    T(r, 3) = (float)-(R[3 * r] * t[0] + R[1 + 3 * r] * t[1] + R[2 + 3 * r] * t[2]);
  }
  return T;
}
bool same_bytes(const vo::Vector10fVector& a, const vo::Vector10fVector& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (std::memcmp(a[i].data(), b[i].data(), 40) != 0) return false;
  return true;
}
void census(const vo::MapNearest& r) {
  const voe_map_nearest_stats& s = r.stats;
  std::printf("%d live rows against %d entries: %d MATCHED, %d NO_ENTRY, %d AMBIGUOUS, %d DISPLACED, %d NAN_ROW\n", s.n_live, s.n_entries, s.n_matched,
              s.n_no_entry, s.n_ambiguous, s.n_displaced, s.n_nan);
}
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  double sigma = 0.005;
  bool tracks = false;
  vo::NearestOptions near;
  near.radius = 0.1f;
  near.ratio = 0.8f;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s == "--tracks") tracks = true;
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--sigma=", 0) == 0) sigma = std::atof(s.c_str() + 8);
    else if (s.rfind("--radius=", 0) == 0) near.radius = (float)std::atof(s.c_str() + 9);
    else if (s.rfind("--ratio=", 0) == 0) near.ratio = (float)std::atof(s.c_str() + 8);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || !(sigma >= 0)) { std::printf("usage: associate_map <data dir> [--tracks] [--sigma=0.005] [--radius=0.1] [--ratio=0.8] [--seed=1]\n"); return -1; }
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

    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> clean, pushed;
    std::mt19937 rng(seed);
    std::normal_distribution<float> noise(0.f, (float)sigma);
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      pixels.push_back(known::strip_id(meas_with_id));
      clean.push_back(appearances);
      if (sigma > 0)
        for (auto& a : appearances) for (int k = 0; k < 10; ++k) a[k] += noise(rng);
      pushed.push_back(appearances);
    }
    std::printf("%zu frames, every appearance pushed by N(0, %g) (seed %u); radius %g, ratio %g\n", F, sigma, seed, near.radius, near.ratio);

    if (!tracks) {
      vo::DeviceMap map((int)world_app.size());
      map.update(world_xyz, world_app);
      size_t exact = 0;
      for (size_t f = 0; f < F; ++f) exact += map.lookup(pushed[f]).size();
      std::printf("map of %d entries; the exact lookup of the pushed rows hits %zu\n", map.size(), exact);
      const vo::MapNearest r = map.nearest(pushed, near);
      census(r);
      size_t frames_equal = 0;
      for (size_t f = 0; f < F; ++f) frames_equal += same_bytes(r.canonical[f], clean[f]);
      std::vector<vo_map_localise_stats> stats;
      const vo::IsometryVector poses = map.localise_batch(cam, pixels, r.canonical, vo::LocaliseOptions(), &stats);
      double worst = 0;
      bool status_ok = true;
      for (size_t f = 0; f < F; ++f) {
        worst = std::fmax(worst, robot_pose_error(poses[f], data.cameraInRobot, gt[f]));
        status_ok = status_ok && stats[f].status == VO_MAP_LOCALISE_OK;
      }
      std::printf("canonical rows equal the clean files' bytes in %zu of %zu frames; statuses %s; largest pose difference to trajectory.dat: %.3g\n",
                  frames_equal, F, status_ok ? "all OK" : "NOT all OK", worst);
      return frames_equal == F && status_ok && worst < 1e-4 ? 0 : 1;
    }

    // --tracks: the dictionary, frame by frame
    vo::DeviceMap dict(4096);
    for (size_t f = 0; f < F; ++f) {
      const vo::MapNearest r = dict.nearest({pushed[f]}, near);
      dict.update(vo::Vector3fVector(pushed[f].size(), vo::Vector3f::Zero()), r.canonical[0]);
    }
    const vo::MapNearest all = dict.nearest(pushed, near);
    std::printf("dictionary of %d classes; second pass: ", dict.size());
    census(all);

    vo::IsometryVector poses;
    for (size_t f = 0; f < F; ++f) poses.push_back(camera_in_map_inverse(gt[f], data.cameraInRobot));
    vo::GrowOptions opt;
    vo::DeviceMap grown_clean((int)world_app.size()), grown_canon((int)world_app.size());
    const voe_map_grow_stats sc = grown_clean.grow(cam, pixels, clean, poses, opt);
    const voe_map_grow_stats sn = grown_canon.grow(cam, pixels, all.canonical, poses, opt);
    vo::Vector3fVector xc, xn;
    vo::Vector10fVector ac, an;
    grown_clean.read(xc, ac);
    grown_canon.read(xn, an);
    bool same = xc.size() == xn.size();
    for (size_t e = 0; same && e < xc.size(); ++e) same = std::memcmp(xc[e].data(), xn[e].data(), 12) == 0;
    std::printf("grow from an empty map: %d landmarks on the clean frames, %d on the canonical frames; points %s\n", sc.n_added, sn.n_added,
                same ? "equal byte for byte" : "DIFFER");
    return same && sc.n_added > 0 && sc.n_added == sn.n_added && all.stats.n_ambiguous == 0 ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "associate_map: %s\n", e.what());
    return 2;
  }
}
