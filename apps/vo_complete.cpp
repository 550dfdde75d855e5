// vo_complete -- counterpart of the reference's src/apps/vo_complete.cpp:68-187
// on the GPU path: monocular VO on a data directory with unknown data
// association.  Same call sequence, same output files (written into the
// current directory or into argv[2]): world.txt, trajectory_gt.txt, map.txt,
// map_appearances.txt, trajectory_est_complete.txt, trajectory_est_data.txt.
//   usage: vo_complete <data dir> [output dir] [rounds=100] [--resident [--match-up-front]] [--exact] [--ransac[=px]]
//          [--track-ransac[=px]] [--refine-init[=huber_px]]
// --resident: the same sequence through vo::DeviceSequence -- all measurement files are read and uploaded first, the
// whole frame chain runs on the GPU without a host round trip per frame, the map upkeep included (vo_map_*: the
// reference's upsert as a hash table of first occurrences in device memory).  Same outputs.
// --exact: the solver in reference-order arithmetic (PICPSolver::setExact): every pose of the chain is then
// bit-identical to the reference's float32 arithmetic given the same first relative pose.
// --ransac[=px]: the first relative pose from the inliers of a RANSAC over the first pair's matches (2048 hypotheses,
// Sampson threshold px, default 1, seed 0: vo::estimate_transform_ransac / DeviceSequence::setInitRansac) instead of from
// all of them.  The frame-by-frame form refits the inliers with the same estimate_transform it uses without the flag;
// with no mismatched pair every output file is the same as without the flag.
// --track-ransac[=px]: every frame t >= 2 is tracked from the best of 2048 P3P hypotheses over its joined pairs (reprojection
// threshold px, default 1, seed 0: vo::estimate_pose_ransac / DeviceSequence::setTrackRansac) -- the solver starts from the
// winner's pose and runs its rounds on the winner's inliers.  A frame the host form refuses (fewer than 4 pairs, no valid
// hypothesis, fewer than 6 inliers) runs as without the flag, which is what the device form does on its own.
// --refine-init[=huber_px]: the first relative pose, from either initialisation, is refined by 10 Gauss-Newton rounds on the
// Sampson error of the first pair's matches (Huber weight at huber_px pixels, default 1, 0: none: vo::refine_transform /
// DeviceSequence::setInitRefine) before anything uses it; behind --ransac only the winner's inliers take part, marked at
// their positions among the matches, so that both forms sum the same pairs in the same order and write the same files.
// Also written: poses_raw.txt, one camera pose per line (row-major 4x4, %.9g = exact float32 round trip), and map_raw.txt,
// one map entry per line (x y z a0..a9, %.9g).
#include <cmath>
#include <cstdio>
#include <iostream>

#include "vo/vo.hpp"

using namespace vo;

static void write_poses_raw(const std::string& file, const IsometryVector& trajectory) {
  std::FILE* f = std::fopen(file.c_str(), "w");
  if (!f) return;
  for (const auto& X : trajectory) {
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::fprintf(f, "%.9g ", X(r, c));
    std::fprintf(f, "\n");
  }
  std::fclose(f);
}

static void write_map_raw(const std::string& file, const PointCloudVector<3>& map) {
  std::FILE* f = std::fopen(file.c_str(), "w");
  if (!f) return;
  for (size_t i = 0; i < map.size(); ++i) {
    for (int k = 0; k < 3; ++k) std::fprintf(f, "%.9g ", map.points()[i][k]);
    for (int k = 0; k < 10; ++k) std::fprintf(f, "%.9g ", map.appearances()[i].v[k]);
    std::fprintf(f, "\n");
  }
  std::fclose(f);
}

// the device-resident form of the loop below: same call sequence, the frame chain inside vo::DeviceSequence
static int run_resident(const std::string& path, const std::string& out, int rounds, bool exact, bool up_front, float ransac_px,
                        float track_px, float refine_px, const std::string& first_file,
                        const std::string& second_file, const std::set<std::string>& files) {
  std::vector<PointCloudVector<2>> frames;
  std::vector<std::string> names{first_file, second_file};
  names.insert(names.end(), files.begin(), files.end());
  for (const auto& f : names) {
    PointCloudVector<2> pc;
    if (!get_meas_content(path + f, pc)) { std::cout << "Unable to open file " << path + f << std::endl; return -1; }
    frames.push_back(std::move(pc));
  }
  Vector3fVector world_points;
  Vector10fVector world_points_appearances;
  if (!get_meas_content(path + "world.dat", world_points_appearances, world_points, true)) { std::cout << "Unable to open world file\n"; return -1; }
  write_eigen_vectors_to_file(out + "world.txt", world_points);
  std::vector<int> int_params;
  Matrix3f k;
  Isometry3f H;
  if (!get_camera_params(path + "camera.dat", int_params, k, H)) { std::cout << "Unable to get camera parameters\n"; return -1; }
  Camera cam(int_params[3], int_params[2], int_params[0], int_params[1], k);
  DeviceSequence seq(cam, frames, rounds);
  seq.setExact(exact);
  seq.setMatchUpFront(up_front);              // all consecutive pairs in one batched matcher call before the chain
  if (ransac_px > 0.f) seq.setInitRansac(ransac_params(ransac_px));
  if (track_px > 0.f) seq.setTrackRansac(track_ransac_params(track_px));
  if (refine_px >= 0.f) seq.setInitRefine(10, refine_px);
  seq.setKeepMap(true);                       // map.update / history inside the chain, on the device (vo_complete.cpp:145-147,175-176)
  seq.run();
  const IsometryVector trajectory = seq.trajectory();          // waits for the chain
  if (refine_px >= 0.f) {
    const vo_epi_refine_stats rs = seq.initRefineStats();
    std::printf("refine-init: status %d, %d rounds, %d pairs, cost %.6g -> %.6g\n", rs.status, rs.rounds, rs.n_used, rs.cost_before,
                rs.cost_after);
  }
  for (int t = 2; t < seq.frames(); ++t) {
    int n_match, n_join, n_tri;
    seq.counts(t, n_match, n_join, n_tri);
    const Isometry3f& X = trajectory[(size_t)t];
    std::printf("%s: %d matches, %d model correspondences, t = % .5f % .5f % .5f\n", names[(size_t)t].c_str(), n_match, n_join,
                X(0, 3), X(1, 3), X(2, 3));
  }
  const PointCloudVector<3> map = seq.map(&H);                 // map = H * map (vo_complete.cpp:183)
  write_map_raw(out + "map_raw.txt", map);
  write_eigen_vectors_to_file(out + "map.txt", map.points());
  write_eigen_vectors_to_file(out + "map_appearances.txt", map.appearances());
  save_trajectory(out + "trajectory_est_complete.txt", trajectory, H);
  save_trajectory(out + "trajectory_est_data.txt", trajectory, H, true);
  write_poses_raw(out + "poses_raw.txt", trajectory);
  return 0;
}

int main(int argc, char* argv[]) {
  // flags first, wherever they stand; what is left are the positional arguments
  bool resident = false, exact = false, up_front = false;
  float ransac_px = 0.f;                      // 0: no RANSAC
  float track_px = 0.f;                       // 0: no tracking RANSAC
  float refine_px = -1.f;                     // < 0: no refit of the first pose; otherwise its Huber width (0: no weight)
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string a(argv[i]);
    if (a == "--resident") resident = true;
    else if (a == "--exact") exact = true;
    else if (a == "--match-up-front") up_front = true;
    else if (a == "--ransac") ransac_px = 1.f;
    else if (a.rfind("--ransac=", 0) == 0) {
      ransac_px = std::strtof(a.c_str() + 9, nullptr);
      if (!(ransac_px > 0.f)) { std::cout << "--ransac=px needs a positive threshold" << std::endl; return -1; }
    }
    else if (a == "--track-ransac") track_px = 1.f;
    else if (a.rfind("--track-ransac=", 0) == 0) {
      track_px = std::strtof(a.c_str() + 15, nullptr);
      if (!(track_px > 0.f)) { std::cout << "--track-ransac=px needs a positive threshold" << std::endl; return -1; }
    }
    else if (a == "--refine-init") refine_px = 1.f;
    else if (a.rfind("--refine-init=", 0) == 0) {
      char* end = nullptr;
      refine_px = std::strtof(a.c_str() + 14, &end);
      if (end == a.c_str() + 14 || !(refine_px >= 0.f) || !std::isfinite(refine_px)) {
        std::cout << "--refine-init=huber_px needs a width >= 0" << std::endl; return -1;
      }
    }
    else if (a.rfind("--", 0) == 0) { std::cout << "unknown option " << a << std::endl; return -1; }
    else pos.push_back(a);
  }
  if (pos.empty()) { std::cout << "Error: need path parameter to read data" << std::endl; return -1; }
  std::string path(pos[0]);
  if (path.back() != '/') path.push_back('/');
  std::string out = pos.size() > 1 ? pos[1] : ".";
  if (out.back() != '/') out.push_back('/');
  const int rounds = pos.size() > 2 ? std::atoi(pos[2].c_str()) : 100;
  try {
    save_gt_trajectory(path + "trajectory.dat", out + "trajectory_gt.txt");
    const std::regex pattern("^meas-\\d.*\\.dat$");
    std::set<std::string> files;
    if (!get_file_names(path, files, pattern)) { std::cout << "unable to open directory\n"; return -1; }
    if (files.size() < 2) { std::cout << "need at least two measurement files\n"; return -1; }
    const auto first_file = *(files.begin());
    const auto second_file = *(files.erase(files.begin()));
    files.erase(files.begin());

    if (resident) return run_resident(path, out, rounds, exact, up_front, ransac_px, track_px, refine_px, first_file, second_file, files);
    PointCloudVector<2> reference_pc, current_pc;
    if (!get_meas_content(path + first_file, reference_pc)) { std::cout << "Unable to open file measurement file 0\n"; return -1; }
    if (!get_meas_content(path + second_file, current_pc)) { std::cout << "Unable to open file measurement file 1\n"; return -1; }
    Vector3fVector world_points;
    Vector10fVector world_points_appearances;
    if (!get_meas_content(path + "world.dat", world_points_appearances, world_points, true)) { std::cout << "Unable to open world file\n"; return -1; }
    write_eigen_vectors_to_file(out + "world.txt", world_points);
    // the pairs are (ref_idx,curr_idx)
    IntPairVector correspondences_imgs = compute_correspondences_images(reference_pc.appearances(), current_pc.appearances());
    std::vector<int> int_params;   // z_near,z_far,cols,rows
    Matrix3f k;
    Isometry3f H;
    if (!get_camera_params(path + "camera.dat", int_params, k, H)) { std::cout << "Unable to get camera parameters\n"; return -1; }
    Camera cam(int_params[3], int_params[2], int_params[0], int_params[1], k);

    IntPairVector init_pairs;                  // --ransac: the inliers of the first pair's matches
    std::vector<uint8_t> inlier;
    if (ransac_px > 0.f) {
      estimate_transform_ransac(cam.cameraMatrix(), correspondences_imgs, reference_pc.points(), current_pc.points(),
                                ransac_params(ransac_px), &inlier);
      for (size_t i = 0; i < correspondences_imgs.size(); ++i) if (inlier[i]) init_pairs.push_back(correspondences_imgs[i]);
    }
    Isometry3f X = estimate_transform(cam.cameraMatrix(), ransac_px > 0.f ? init_pairs : correspondences_imgs,
                                      reference_pc.points(), current_pc.points());
    if (refine_px >= 0.f) {                    // --refine-init: the matches where they lie, the inliers marked
      vo_epi_refine_stats rs;
      X = refine_transform(cam.cameraMatrix(), correspondences_imgs, reference_pc.points(), current_pc.points(), X,
                           refine_params(10, refine_px), ransac_px > 0.f ? &inlier : nullptr, &rs);
      std::printf("refine-init: status %d, %d rounds, %d pairs, cost %.6g -> %.6g\n", rs.status, rs.rounds, rs.n_used, rs.cost_before,
                  rs.cost_after);
    }

    PointCloudVector<3> triangulated_pc;
    IntPairVector correspondences_world;
    triangulate_points(k, X, correspondences_imgs, reference_pc, current_pc, triangulated_pc, correspondences_world);   // (curr_idx,world_idx)

    IsometryVector trajectory;
    trajectory.reserve(files.size() + 2);
    trajectory.push_back(Isometry3f::Identity());
    trajectory.push_back(X);
    PICPSolver solver;
    solver.setKernelThreshold(10000);
    solver.setExact(exact);

    reference_pc = current_pc;   // correspondences_world now reads (ref_idx,world_idx)
    PointCloudVector<3> triangulated_transformed, map;
    map.update(triangulated_pc);
    Isometry3f history = X.inverse();
    Isometry3f X_curr = X;

    for (const auto& file : files) {
      if (!get_meas_content(path + file, current_pc)) { std::cout << "Unable to open file " << path + file << std::endl; return -1; }
      correspondences_imgs = compute_correspondences_images(reference_pc.appearances(), current_pc.appearances());
      correspondences_world = extract_correspondences_world(correspondences_imgs, correspondences_world);
      triangulated_transformed = X_curr * triangulated_pc;
      cam.setWorldInCameraPose(Isometry3f::Identity());
      const IntPairVector* round_pairs = &correspondences_world;
      IntPairVector track_pairs;              // --track-ransac: the winner's inliers, the solve starting from its pose
      if (track_px > 0.f) {
        try {
          std::vector<uint8_t> inlier;
          const Isometry3f T = estimate_pose_ransac(cam, triangulated_transformed.points(), current_pc.points(), correspondences_world,
                                                    track_ransac_params(track_px), &inlier);
          for (size_t i = 0; i < correspondences_world.size(); ++i) if (inlier[i]) track_pairs.push_back(correspondences_world[i]);
          cam.setWorldInCameraPose(T);
          round_pairs = &track_pairs;
        } catch (const vo::Error&) {}         // refused: the plain frame, as the device form falls back
      }
      solver.init(cam, triangulated_transformed.points(), current_pc.points());
      for (int i = 0; i < rounds; i++) solver.oneRound(*round_pairs, false);
      cam = solver.camera();
      trajectory.push_back(cam.worldInCameraPose());
      X_curr = cam.worldInCameraPose();
      std::printf("%s: %zu matches, %zu model correspondences, %d inliers, t = % .5f % .5f % .5f\n", file.c_str(),
                  correspondences_imgs.size(), correspondences_world.size(), solver.numInliers(), X_curr(0, 3), X_curr(1, 3), X_curr(2, 3));
      triangulate_points(k, cam.worldInCameraPose(), correspondences_imgs, reference_pc, current_pc, triangulated_pc, correspondences_world);
      map.update(history * triangulated_pc);
      history = history * cam.worldInCameraPose().inverse();
      reference_pc = current_pc;
    }
    map = H * map;
    write_map_raw(out + "map_raw.txt", map);
    write_eigen_vectors_to_file(out + "map.txt", map.points());
    write_eigen_vectors_to_file(out + "map_appearances.txt", map.appearances());
    save_trajectory(out + "trajectory_est_complete.txt", trajectory, H);
    save_trajectory(out + "trajectory_est_data.txt", trajectory, H, true);
    write_poses_raw(out + "poses_raw.txt", trajectory);
    return 0;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "vo_complete: %s\n", e.what());
    return 2;
  }
}
