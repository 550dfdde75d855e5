// window_map -- the local window of a frame on a data directory: the map is world.dat, the frames are ALL the measurement files,
// ONE voe_map_covis call counts the landmarks every two frames share and ONE voe_map_window call chooses the frames to free, the
// frames to hold and the landmarks between them.
//   usage: window_map <data dir> [--query=0] [--free=8] [--fixed=8] [--min-shared=15] [--bundle] [--seed=1]
// Printed: the window (the free frames in rank order, the query first, then the fixed frames) and its statistics.  With --bundle
// the points are pushed with bundle_map's seeded generator (up to 0.02 per coordinate), the poses are the ground truth, and ONE
// vox_map_bundle call runs over ALL frames with the window's row counts and mask -- a frame outside the window has no live row
// and is held; the cost before and after is printed.  Exit 0 iff the window was chosen and, with --bundle, the bundle's status
// is OK and its counts agree with the window's: as many free frames, and as many observations as the window's frames have hits.
#include <cstring>
#include <random>

#include "known_common.hpp"

int main(int argc, char* argv[]) {
  int query = 0;
  bool bundle = false;
  unsigned seed = 1;
  vo::WindowOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--query=", 0) == 0) query = std::atoi(s.c_str() + 8);
    else if (s.rfind("--free=", 0) == 0) opt.k_free = std::atoi(s.c_str() + 7);
    else if (s.rfind("--fixed=", 0) == 0) opt.k_fixed = std::atoi(s.c_str() + 8);
    else if (s.rfind("--min-shared=", 0) == 0) opt.min_shared = std::atoi(s.c_str() + 13);
    else if (s == "--bundle") bundle = true;
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty()) {
    std::printf("usage: window_map <data dir> [--query=0] [--free=8] [--fixed=8] [--min-shared=15] [--bundle] [--seed=1]\n");
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

    vo::Vector3fVector start = world_xyz;
    if (bundle) {                                             // bundle_map's generator
      std::mt19937 rng(seed);
      std::uniform_real_distribution<double> unit(-1.0, 1.0);
      for (auto& p : start)
        for (int k = 0; k < 3; ++k) p[k] = (float)((double)p[k] + 0.02 * unit(rng));
    }
    vo::DeviceMap map((int)world_app.size());
    map.update(start, world_app);

    const vo::Covisibility cov = map.covisibility(apps);
    std::printf("map of %d entries, %zu frames: %d hits, %d entries seen by some frame, %zu words per row\n", cov.stats.n_entries, F, cov.stats.n_hits,
                cov.stats.n_entries_seen, cov.n_words);
    const vo::MapWindow w = map.window(cov, query, opt, &live);
    const voe_map_window_stats& ws = w.stats;
    std::printf("window of frame %d (k_free %d, k_fixed %d, min_shared %d): status %s\n", query, opt.k_free, opt.k_fixed, opt.min_shared,
                vo::window_status_name(ws.status));
    std::printf("order:");
    for (int j = 0; j < ws.n_free + ws.n_fixed; ++j) std::printf(" %d", w.order[(size_t)j]);
    std::printf("\n");
    for (int j = 0; j < ws.n_free + ws.n_fixed; ++j) {
      const size_t f = (size_t)w.order[(size_t)j];
      std::printf("  frame %zu %s: shares %d with the query, sees %d\n", f, w.role[f] == VOE_MAP_WINDOW_FREE ? "FREE " : "FIXED", cov.shared((size_t)query, f),
                  cov.shared(f, f));
    }
    std::printf("free %d fixed %d candidates %d fixed candidates %d landmarks %d, the query sees %d\n", ws.n_free, ws.n_fixed, ws.n_candidates,
                ws.n_fixed_candidates, ws.n_points, ws.query_seen);
    if (ws.status == VOE_MAP_WINDOW_QUERY_UNSEEN) return 1;
    if (!bundle) return 0;

    if (ws.status != VOE_MAP_WINDOW_OK) { std::printf("no frame is held: a bundle on this window has a free gauge\n"); return 1; }
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    if (gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }
    // ALL frames, with the window's row counts: a frame outside the window has no live row (and is held)
    vo::IsometryVector poses;
    long long window_hits = 0;
    for (size_t f = 0; f < F; ++f) {
      poses.push_back((gt[f] * data.cameraInRobot).inverse());
      pixels[f].resize((size_t)w.n_rows[f]);
      apps[f].resize((size_t)w.n_rows[f]);
      if (w.role[f] != VOE_MAP_WINDOW_OUTSIDE) window_hits += cov.shared(f, f);
    }
    if (cov.stats.n_hits != cov.stats.n_seen) std::printf("(some frame hits an entry twice: the observations exceed the entries seen)\n");
    static const char* const names[6] = {"OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE"};
    const vox_map_bundle_stats st = map.bundle(data.camera(), pixels, apps, poses, &w.fixed);
    std::printf("bundle over all %zu frames: status %s, %d free frames, %d free landmarks, %d observations, cost %.6g -> %.6g\n", F,
                st.status >= 0 && st.status < 6 ? names[st.status] : "?", st.n_free_frames, st.n_free_points, st.n_obs, st.cost_before, st.cost_after);
    const bool agree = st.n_free_frames == ws.n_free && (long long)st.n_obs == window_hits && cov.stats.n_hits == cov.stats.n_seen;
    std::printf("%s: %d free frames for %d, %d observations for %lld hits of the window's frames\n", agree ? "window and bundle agree" : "window and bundle DISAGREE",
                st.n_free_frames, ws.n_free, st.n_obs, window_hits);
    return st.status == VOX_MAP_BUNDLE_OK && agree ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "window_map: %s\n", e.what());
    return 2;
  }
}
