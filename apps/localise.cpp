// localise -- every frame of a data directory localised in the map of its world.dat, each one from scratch (no prior, no
// predecessor): the second pass over a mapped route.  The map is built on the device with ONE vo_map_update of world.dat; a
// frame is looked up in it by appearance (vo_map_lookup), a P3P RANSAC over the hits gives the start and the inliers, PICP
// rounds finish (vo_map_localise) -- or all frames go through one vo_map_localise_batch_dev call with --batch.
//   usage: localise <data dir> [out dir] [--batch] [--hyp=N] [--px=P] [--rounds=R]        (defaults 64, 2, 50)
// The data knows the answer: a measurement's appearance row is its landmark's row bit for bit and names it by id, and
// trajectory.dat holds every robot pose.  With T_i the pose found for frame i (p_cam = T_i p_map) and C the cam_transform of
// camera.dat, the robot pose is inv(T_i) inv(C).  Exit 0 iff every frame's lookup equals the ids of its file, every status is
// OK and every pose lies within 1e-4 of trajectory.dat (largest absolute entry difference, printed).
// Written: trajectory_est.txt (x y z of the robot per frame), trajectory_gt.txt, poses_raw.txt (T_i, as vo_complete).
#include <cstring>

#include "known_common.hpp"

namespace {
// inv(T) inv(C) in double against the ground-truth pose: largest absolute entry difference of the 3 x 4
double robot_pose_error(const vo::Isometry3f& T, const vo::Isometry3f& C, const vo::Isometry3f& gt, double robot[12]) {
  auto inv = [](const vo::Isometry3f& X, double R[9], double t[3]) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r + 3 * c] = X(c, r);
    for (int r = 0; r < 3; ++r) t[r] = -(R[r] * X(0, 3) + R[r + 3] * X(1, 3) + R[r + 6] * X(2, 3));
  };
  double Ra[9], ta[3], Rb[9], tb[3];
  inv(T, Ra, ta);
  inv(C, Rb, tb);
  double err = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) robot[r + 3 * c] = Ra[r] * Rb[3 * c] + Ra[r + 3] * Rb[1 + 3 * c] + Ra[r + 6] * Rb[2 + 3 * c];
    robot[9 + r] = Ra[r] * tb[0] + Ra[r + 3] * tb[1] + Ra[r + 6] * tb[2] + ta[r];
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) err = std::fmax(err, std::fabs(robot[r + 3 * c] - (double)gt(r, c)));
    err = std::fmax(err, std::fabs(robot[9 + r] - (double)gt(r, 3)));
  }
  return err;
}
}  // namespace

int main(int argc, char* argv[]) {
  std::string path, out = "./";
  bool batch = false;
  vo::LocaliseOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s == "--batch") batch = true;
    else if (s.rfind("--hyp=", 0) == 0) opt.ransac.n_hypotheses = std::atoi(s.c_str() + 6);
    else if (s.rfind("--px=", 0) == 0) opt.ransac.threshold_px = (float)std::atof(s.c_str() + 5);
    else if (s.rfind("--rounds=", 0) == 0) opt.n_iters = std::atoi(s.c_str() + 9);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) { std::printf("usage: localise <data dir> [out dir] [--batch] [--hyp=N] [--px=P] [--rounds=R]\n"); return -1; }
  path = pos[0];
  if (path.back() != '/') path.push_back('/');
  if (pos.size() > 1) out = pos[1];
  if (out.back() != '/') out.push_back('/');
  if (opt.ransac.n_hypotheses < 1) { std::printf("--hyp must be positive: every frame is localised without a prior\n"); return -1; }
  try {
    known::Dataset data;
    if (!known::load_dataset(path, data, false)) return -1;
    vo::Vector10fVector world_app;
    vo::Vector3fVector world_xyz;                                    // world.dat: every landmark's position and appearance
    if (!vo::get_meas_content(path + "world.dat", world_app, world_xyz, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    vo::save_gt_trajectory(path + "trajectory.dat", out + "trajectory_gt.txt");
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    vo::DeviceMap map((int)world_app.size());
    map.update(world_xyz, world_app);
    std::printf("map of %d entries from %zu landmarks\n", map.size(), world_app.size());
    const vo::Camera cam = data.camera();

    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> apps;
    bool lookup_ok = true;
    for (const std::string& name : data.meas_files) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + name, appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + name).c_str()); return -1; }
      std::vector<int32_t> entries;
      const vo::IntPairVector hits = map.lookup(appearances, nullptr, &entries);
      bool same = hits.size() == meas_with_id.size();
      for (size_t i = 0; i < meas_with_id.size(); ++i) same = same && entries[i] == (int)meas_with_id[i].x();
      if (!same) { std::printf("%s: the lookup differs from the ids of the file (%zu hits of %zu rows)\n", name.c_str(), hits.size(), meas_with_id.size()); lookup_ok = false; }
      pixels.push_back(known::strip_id(meas_with_id));
      apps.push_back(appearances);
    }

    vo::IsometryVector poses;
    std::vector<vo_map_localise_stats> stats(pixels.size());
    if (batch) {
      poses = map.localise_batch(cam, pixels, apps, opt, &stats);
    } else {
      for (size_t f = 0; f < pixels.size(); ++f) poses.push_back(map.localise(cam, pixels[f], apps[f], opt, &stats[f]));
    }

    std::FILE* est = std::fopen((out + "trajectory_est.txt").c_str(), "w");
    double worst = 0;
    bool status_ok = true;
    for (size_t f = 0; f < poses.size(); ++f) {
      const vo_map_localise_stats& s = stats[f];
      double robot[12], err = -1;
      if (f < gt.size()) { err = robot_pose_error(poses[f], data.cameraInRobot, gt[f], robot); worst = std::fmax(worst, err); }
      if (est && f < gt.size()) std::fprintf(est, "%.9g %.9g %.9g\n", robot[9], robot[10], robot[11]);
      if (s.status != VO_MAP_LOCALISE_OK) status_ok = false;
      std::printf("%s: %d rows, %d hits, %d handed on, %d inliers, %s, diff %.3g\n", data.meas_files[f].c_str(), s.n_rows, s.n_hits,
                  s.ransac_inliers, s.num_inliers, vo::localise_status_name(s.status), err);
    }
    if (est) std::fclose(est);
    known::write_poses_raw(out + "poses_raw.txt", poses);
    const bool enough_gt = gt.size() >= poses.size();
    if (!enough_gt) std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), poses.size());
    std::printf("%s: %zu frames, lookup %s, statuses %s, largest pose difference to trajectory.dat: %.3g\n", batch ? "one batched call" : "single calls",
                poses.size(), lookup_ok ? "equal to the ids" : "DIFFERENT", status_ok ? "all OK" : "NOT all OK", worst);
    return lookup_ok && status_ok && enough_gt && worst < 1e-4 ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "localise: %s\n", e.what());
    return 2;
  }
}
