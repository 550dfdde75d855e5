// align_map -- the map vo_complete estimated, aligned to the world it was estimated from: reads what evaluate reads (map.txt,
// map_appearances.txt and trajectory_est_data.txt in <out dir>, world.dat and trajectory.dat in <data dir>), puts both maps
// on the device and runs ONE voe_map_align call, world = dst, estimate = src: the similarity S = [c R | t] with
// p_world ~ S p_estimate, by 3-point RANSAC on the landmarks of equal appearance and Umeyama refits over the inliers.
//   usage: align_map <data dir> <out dir> [--threshold=0.5] [--hypotheses=256] [--seed=1] [--refits=1] [--no-scale] [--merge]
// Printed: S, its scale beside evaluate's median_ratio_inv (the one scalar evaluate relates the two frames by), the matches,
// the inliers and their rms beside evaluate's rmse_map.  --merge: the estimate's landmarks that the world does not hold are
// appended to the world map, moved by S (VOE_MAP_MERGE_KEEP_DST), and the counts printed.
// Exit 0 iff the alignment's status is OK.
#include <cstdio>
#include <cstdlib>

#include "vo/evaluation.hpp"
#include "vo/localise.hpp"

int main(int argc, char* argv[]) {
  vo::AlignOptions opt;
  opt.threshold = 0.5f; opt.n_hypotheses = 256;
  bool merge = false;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--threshold=", 0) == 0) opt.threshold = (float)std::atof(s.c_str() + 12);
    else if (s.rfind("--hypotheses=", 0) == 0) opt.n_hypotheses = std::atoi(s.c_str() + 13);
    else if (s.rfind("--seed=", 0) == 0) opt.seed = std::strtoull(s.c_str() + 7, nullptr, 10);
    else if (s.rfind("--refits=", 0) == 0) opt.n_refits = std::atoi(s.c_str() + 9);
    else if (s == "--no-scale") opt.with_scale = false;
    else if (s == "--merge") merge = true;
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.size() < 2) {
    std::printf("usage: align_map <data dir> <out dir> [--threshold=0.5] [--hypotheses=256] [--seed=1] [--refits=1] [--no-scale] [--merge]\n");
    return -1;
  }
  std::string path = pos[0], out = pos[1];
  if (path.back() != '/') path.push_back('/');
  if (out.back() != '/') out.push_back('/');
  try {
    const vo::Vector3fVector map_est = vo::read_eigen_vectors<3>(out + "map.txt");
    const vo::Vector10fVector map_app = vo::read_eigen_vectors<10>(out + "map_appearances.txt");
    vo::Vector3fVector world;
    vo::Vector10fVector world_app;
    if (!vo::get_meas_content(path + "world.dat", world_app, world, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    if (map_est.empty() || map_est.size() != map_app.size()) { std::printf("map.txt and map_appearances.txt hold %zu and %zu rows\n", map_est.size(), map_app.size()); return -1; }

    vo::DeviceMap dst((int)world.size()), src((int)map_est.size());
    dst.update(world, world_app);
    src.update(map_est, map_app);
    std::printf("world of %d landmarks, estimate of %d\n", dst.size(), src.size());

    voe_map_align_stats st{};
    const vo::Similarity3f S = dst.align(src, opt, &st);
    std::printf("status %s: %d matches, %d inliers (winner: hypothesis %d with %d, %d of %d hypotheses valid), refit %s\n", vo::align_status_name(st.status),
                st.n_matches, st.n_inliers, st.best_hypothesis, st.best_count, st.n_valid, opt.n_hypotheses, st.refit_kept ? "kept" : "not kept");
    std::printf("S =\n");
    for (int r = 0; r < 4; ++r) std::printf("  %12.6f %12.6f %12.6f %12.6f\n", S(r, 0), S(r, 1), S(r, 2), S(r, 3));
    std::printf("scale %.9g, rms %.9g over the inliers (threshold %g)\n", st.scale, st.rms, opt.threshold);

    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    const vo::IsometryVector est = vo::get_est_data(out + "trajectory_est_data.txt");
    if (!gt.empty() && !est.empty()) {
      const vo::EvalResult ev = vo::evaluate(gt, est, map_est, map_app, world, world_app);
      std::printf("evaluate: median_ratio_inv %.9g, rmse_map %.9g over %d points\n", ev.median_ratio_inv, ev.rmse_map, ev.matched_map_points);
    }
    if (merge && st.status == VOE_MAP_ALIGN_OK) {
      const voe_map_merge_stats ms = dst.merge(src, &S, VOE_MAP_MERGE_KEEP_DST);
      std::printf("merged: %d of the estimate's %d landmarks were in the world already, %d appended, the world map holds %d\n", ms.n_shared, ms.n_src,
                  ms.n_appended, ms.n_dst_after);
    }
    return st.status == VOE_MAP_ALIGN_OK ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "align_map: %s\n", e.what());
    return 2;
  }
}
