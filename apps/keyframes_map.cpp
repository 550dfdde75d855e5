// keyframes_map -- which frames of a data directory to keep: the map is world.dat, the frames are ALL the measurement files, ONE
// voe_map_covis call gives the bit rows and ONE voe_map_keyframes call, with the first and the last frame protected, drops the
// frames whose landmarks enough other frames see.
//   usage: keyframes_map <data dir> [--observers=3] [--share=1000] [--min-seen=1] [--max-gap=0] [--max-dropped=1024] [--seed=1]
// Printed: the dropped frames in drop order with seen and red at their step, the census of the verdicts and the observations
// before and after.  Then the points are pushed with bundle_map's seeded generator (up to 0.1 per coordinate), the poses are the
// ground truth, and vo_map_refine runs twice from the same pushed map: over all frames, and over ALL frames with the call's row
// counts -- a dropped frame has no live row; both sets of figures are printed (landmarks OK, observations, cost, the median and
// the largest error to world.dat).  Exit 0 iff the same landmarks come out OK and at least half the frames were dropped.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <random>

#include "known_common.hpp"

static void errors(const vo::Vector3fVector& got, const vo::Vector3fVector& world, const std::vector<int32_t>& status, double* median, double* worst) {
  std::vector<double> e;
  for (size_t i = 0; i < got.size(); ++i)
    if (status[i] == VO_MAP_REFINE_OK) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += ((double)got[i][k] - (double)world[i][k]) * ((double)got[i][k] - (double)world[i][k]);
      e.push_back(std::sqrt(s));
    }
  std::sort(e.begin(), e.end());
  *median = e.empty() ? 0.0 : e[e.size() / 2];
  *worst = e.empty() ? 0.0 : e.back();
}

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  vo::KeyframesOptions opt;
  opt.share_permille = 1000;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--observers=", 0) == 0) opt.min_observers = std::atoi(s.c_str() + 12);
    else if (s.rfind("--share=", 0) == 0) opt.share_permille = std::atoi(s.c_str() + 8);
    else if (s.rfind("--min-seen=", 0) == 0) opt.min_seen = std::atoi(s.c_str() + 11);
    else if (s.rfind("--max-gap=", 0) == 0) opt.max_gap = std::atoi(s.c_str() + 10);
    else if (s.rfind("--max-dropped=", 0) == 0) opt.max_dropped = std::atoi(s.c_str() + 14);
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) {
    std::printf("usage: keyframes_map <data dir> [--observers=3] [--share=1000] [--min-seen=1] [--max-gap=0] [--max-dropped=1024] [--seed=1]\n");
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
    const size_t F = data.meas_files.size();
    if (F < 1) { std::printf("no measurement files in %s\n", path.c_str()); return -1; }
    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> apps;
    std::vector<int> live;
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      pixels.push_back(known::strip_id(meas_with_id));
      apps.push_back(appearances);
      live.push_back((int)appearances.size());
    }
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    if (gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }
    vo::IsometryVector poses;
    for (size_t f = 0; f < F; ++f) poses.push_back((gt[f] * data.cameraInRobot).inverse());

    vo::Vector3fVector pushed = world_xyz;                    // bundle_map's generator
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    for (auto& p : pushed)
      for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + 0.1 * unit(rng));

    vo::DeviceMap map((int)world_app.size());
    map.update(pushed, world_app);
    const vo::Covisibility cov = map.covisibility(apps, false);
    std::printf("map of %d entries, %zu frames: %d hits, %d entries seen by some frame, %zu words per row\n", cov.stats.n_entries, F, cov.stats.n_hits,
                cov.stats.n_entries_seen, cov.n_words);
    std::vector<uint8_t> flags(F, VOE_MAP_KEYFRAMES_FREE);
    flags[0] = flags[F - 1] = VOE_MAP_KEYFRAMES_PROTECTED;
    const vo::MapKeyframes kf = map.keyframes(cov, opt, &flags, &live);
    const voe_map_keyframes_stats& ks = kf.stats;
    std::printf("keyframes (min_observers %d, share %d per mille, min_seen %d, max_gap %d, max_dropped %d), frames 0 and %zu protected\n", opt.min_observers,
                opt.share_permille, opt.min_seen, opt.max_gap, opt.max_dropped, F - 1);
    std::printf("order:");
    for (int j = 0; j < ks.n_dropped; ++j) std::printf(" %d", kf.order[(size_t)j]);
    std::printf("\n");
    for (int j = 0; j < ks.n_dropped; ++j) {
      const size_t f = (size_t)kf.order[(size_t)j];
      std::printf("  step %d: frame %zu, %d of the %d entries it sees have %d other observers\n", j, f, kf.red[f], kf.seen[f], opt.min_observers);
    }
    long long obs_all = 0, obs_kept = 0;
    for (size_t f = 0; f < F; ++f) { obs_all += kf.seen[f]; obs_kept += kf.keep[f] ? kf.seen[f] : 0; }
    std::printf("dropped %d kept %d of %d frames (gone %d protected %d needed %d blocked %d empty %d); entries seen, summed over the frames: %lld -> %lld\n",
                ks.n_dropped, ks.n_kept, ks.n_frames, ks.n_gone, ks.n_protected, ks.n_needed, ks.n_blocked, ks.n_empty, obs_all, obs_kept);

    // the refinement from the same pushed map: over all frames, then over ALL frames with the call's row counts
    vo::RefineOptions ro;
    ro.n_rounds = 5;
    ro.min_obs = 3;
    vo_map_refine_stats st_all{}, st_kept{};
    std::vector<int32_t> status_all, status_kept;
    vo::Vector3fVector pts_all, pts_kept;
    vo::Vector10fVector unused;
    map.refine(data.camera(), pixels, apps, poses, ro, &st_all, &status_all);
    map.read(pts_all, unused);
    map.clear();
    map.update(pushed, world_app);
    for (size_t f = 0; f < F; ++f) { pixels[f].resize((size_t)kf.n_rows[f]); apps[f].resize((size_t)kf.n_rows[f]); }
    map.refine(data.camera(), pixels, apps, poses, ro, &st_kept, &status_kept);
    map.read(pts_kept, unused);
    double med_all, max_all, med_kept, max_kept;
    errors(pts_all, world_xyz, status_all, &med_all, &max_all);
    errors(pts_kept, world_xyz, status_all, &med_kept, &max_kept);      // (over the same landmarks: those OK from all frames)
    std::printf("refine over all %zu frames:  %d landmarks OK, %d observations, cost %.6g -> %.6g, error to world.dat median %.3g max %.3g\n", F,
                st_all.by_status[0], st_all.n_obs, st_all.cost_before, st_all.cost_after, med_all, max_all);
    std::printf("refine over the %d kept:      %d landmarks OK, %d observations, cost %.6g -> %.6g, error to world.dat median %.3g max %.3g\n", ks.n_kept,
                st_kept.by_status[0], st_kept.n_obs, st_kept.cost_before, st_kept.cost_after, med_kept, max_kept);
    bool same = status_all.size() == status_kept.size();
    for (size_t i = 0; same && i < status_all.size(); ++i) same = (status_all[i] == VO_MAP_REFINE_OK) == (status_kept[i] == VO_MAP_REFINE_OK);
    const bool half = 2 * ks.n_dropped >= ks.n_frames;
    std::printf("%s; %s\n", same ? "the kept frames refine the same landmarks" : "the kept frames refine OTHER landmarks",
                half ? "at least half the frames were dropped" : "fewer than half the frames were dropped");
    return same && half ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "keyframes_map: %s\n", e.what());
    return 2;
  }
}
