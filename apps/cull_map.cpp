// cull_map -- landmarks taken out of the map on a data directory whose answer is known: the map is world.dat, the poses are
// those of trajectory.dat (obtained as refine_map obtains them), `outliers` landmarks that at least three rows see are pushed
// off by +-0.2 ... 0.4 per coordinate with a seeded generator, and ONE voe_map_cull call (min_obs = 1, min_frames = 1,
// max_rms_px = px) has to take exactly those out.
//   usage: cull_map <data dir> [--seed=1] [--outliers=40] [--px=1]
// Printed: the counts by verdict, the largest RMS error among the landmarks kept and the smallest among those pushed.
// Exit 0 iff exactly the pushed landmarks were dropped and a lookup of every frame afterwards returns, for every row,
// remap[the entry it returned before].
// (On the example data the seeds 1 to 5 exit 0.  A seed that pushes a landmark behind one of its cameras still exits 0: its
// verdict is BEHIND instead of HIGH_ERROR, and it is dropped all the same.)
#include <algorithm>
#include <cmath>
#include <random>

#include "known_common.hpp"

namespace {
// inv(G C) in double
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
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  int outliers = 40;
  double px = 1.0;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--outliers=", 0) == 0) outliers = std::atoi(s.c_str() + 11);
    else if (s.rfind("--px=", 0) == 0) px = std::atof(s.c_str() + 5);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || outliers < 0) { std::printf("usage: cull_map <data dir> [--seed=1] [--outliers=40] [--px=1]\n"); return -1; }
  std::string path = pos[0];
  if (path.back() != '/') path.push_back('/');
  try {
    known::Dataset data;
    if (!known::load_dataset(path, data, false)) return -1;
    vo::Vector10fVector world_app;
    vo::Vector3fVector world_xyz;
    if (!vo::get_meas_content(path + "world.dat", world_app, world_xyz, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    const vo::IsometryVector gt = vo::get_gt_data(path + "trajectory.dat");
    const size_t F = data.meas_files.size(), M = world_app.size();
    if (F < 1 || gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }

    std::vector<vo::Vector2fVector> pixels;
    std::vector<vo::Vector10fVector> apps;
    vo::IsometryVector poses;
    for (size_t f = 0; f < F; ++f) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector appearances;
      if (!vo::get_meas_content(path + data.meas_files[f], appearances, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      pixels.push_back(known::strip_id(meas_with_id));
      apps.push_back(appearances);
      poses.push_back(camera_in_map_inverse(gt[f], data.cameraInRobot));
    }

    // the entries every frame's rows find BEFORE the cull, and how often each landmark is seen
    vo::DeviceMap map((int)M);
    map.update(world_xyz, world_app);
    std::vector<std::vector<int32_t>> before(F);
    std::vector<int> seen(M, 0);
    for (size_t f = 0; f < F; ++f) {
      map.lookup(apps[f], nullptr, &before[f]);
      for (int32_t e : before[f]) if (e >= 0) ++seen[(size_t)e];
    }
    std::vector<int> candidates;
    for (size_t e = 0; e < M; ++e) if (seen[e] >= 3) candidates.push_back((int)e);
    if ((size_t)outliers > candidates.size()) { std::printf("only %zu landmarks have three observations\n", candidates.size()); return -1; }

    // the pushed landmarks: a partial Fisher-Yates draw, then a step of 0.2 ... 0.4 with a drawn sign per coordinate
    std::mt19937 rng(seed);
    for (int k = 0; k < outliers; ++k) std::swap(candidates[(size_t)k], candidates[(size_t)k + rng() % (candidates.size() - (size_t)k)]);
    std::vector<uint8_t> pushed(M, 0);
    vo::Vector3fVector start = world_xyz;
    std::uniform_real_distribution<double> step(0.2, 0.4);
    for (int k = 0; k < outliers; ++k) {
      const size_t e = (size_t)candidates[(size_t)k];
      pushed[e] = 1;
      for (int a = 0; a < 3; ++a) { const double s = step(rng); start[e][a] = (float)((double)start[e][a] + ((rng() & 1u) ? s : -s)); }
    }
    map.clear();
    map.update(start, world_app);
    std::printf("map of %d entries, %zu frames: %d of the %zu landmarks with >= 3 observations pushed by 0.2 ... 0.4 per coordinate (seed %u)\n",
                map.size(), F, outliers, candidates.size(), seed);

    vo::CullOptions opt;
    opt.min_obs = 1; opt.min_frames = 1; opt.max_rms_px = (float)px;
    std::vector<int32_t> verdict, remap;
    std::vector<voe_map_cull_entry> entries;
    const voe_map_cull_stats st = map.cull(data.camera(), pixels, apps, poses, opt, &verdict, &remap, &entries);
    std::printf("%d observations;", st.n_obs);
    for (int k = 0; k < 8; ++k) std::printf(" %s %d", vo::cull_verdict_name(k), st.by_verdict[k]);
    std::printf("\nkept %d of %d (%s)\n", st.n_kept, st.n_before, st.status == VOE_MAP_CULL_OK ? "OK" : "NOTHING_DROPPED");

    bool exact = true;
    double worst_kept = 0, best_pushed = 1e300;
    for (size_t e = 0; e < M; ++e) {
      const bool dropped = remap[e] < 0;
      if (dropped != (pushed[e] != 0)) exact = false;
      if (entries[e].n_obs > 0) {
        const double rms = std::sqrt(entries[e].mean_sq_px);
        if (pushed[e]) best_pushed = std::fmin(best_pushed, rms); else worst_kept = std::fmax(worst_kept, rms);
      }
    }
    std::printf("largest RMS error of a landmark that was not pushed %.4g px, smallest of a pushed one %.4g px (threshold %g px)\n", worst_kept,
                outliers ? best_pushed : 0.0, px);

    bool lookups = map.size() == st.n_kept;
    for (size_t f = 0; f < F && lookups; ++f) {
      std::vector<int32_t> after;
      map.lookup(apps[f], nullptr, &after);
      for (size_t i = 0; i < after.size(); ++i)
        if (after[i] != (before[f][i] >= 0 ? remap[(size_t)before[f][i]] : -1)) lookups = false;
    }
    std::printf("%s; every lookup afterwards %s\n", exact ? "exactly the pushed landmarks were dropped" : "the dropped landmarks are NOT the pushed ones",
                lookups ? "returns remap[the entry it returned before]" : "does NOT return remap[the entry it returned before]");
    return exact && lookups ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "cull_map: %s\n", e.what());
    return 2;
  }
}
