// grow_map -- landmarks the map gains from the frames, on a data directory whose answer is known: the map is world.dat (or
// nothing, with --from-empty), optionally with `drop` landmarks that at least three rows see taken out by a seeded generator; the
// poses are those of trajectory.dat (obtained as refine_map obtains them), and ONE voe_map_grow call over all frames has to put
// landmarks (back) where world.dat has them.
//   usage: grow_map <data dir> [--from-empty | --drop=N --seed=S] [--min-frames=3] [--parallax=2] [--rms=2] [--bound=B]
// Printed: the census of rows and verdicts, and the distances of the added points to world.dat, matched by appearance.
// Exit 0 iff something was added and the largest distance stays under the bound.  Its default is twice the largest distance the
// float64 restatement measures on the example data from an empty map with two views allowed (profiles/map_grow_budget.json,
// example_from_empty_two_views: 1.822e-3); the margin is for the float32 rounding of the stored point, which that figure lacks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <random>

#include "known_common.hpp"

namespace {
constexpr double DEFAULT_BOUND = 3.644e-3;

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
std::string bits_of(const vo::Vector10f& a) { return std::string(reinterpret_cast<const char*>(a.data()), 40); }
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  int drop = 0;
  bool from_empty = false;
  double bound = DEFAULT_BOUND;
  vo::GrowOptions opt;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s == "--from-empty") from_empty = true;
    else if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--drop=", 0) == 0) drop = std::atoi(s.c_str() + 7);
    else if (s.rfind("--min-frames=", 0) == 0) opt.min_frames = opt.min_obs = std::atoi(s.c_str() + 13);
    else if (s.rfind("--parallax=", 0) == 0) opt.min_parallax_deg = (float)std::atof(s.c_str() + 11);
    else if (s.rfind("--rms=", 0) == 0) opt.max_rms_px = (float)std::atof(s.c_str() + 6);
    else if (s.rfind("--bound=", 0) == 0) bound = std::atof(s.c_str() + 8);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || drop < 0 || (from_empty && drop > 0)) {
    std::printf("usage: grow_map <data dir> [--from-empty | --drop=N --seed=S] [--min-frames=3] [--parallax=2] [--rms=2] [--bound=%g]\n", DEFAULT_BOUND);
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

    // the map to start from: world.dat, without the dropped landmarks, or nothing
    std::vector<uint8_t> keep(M, from_empty ? 0 : 1);
    vo::DeviceMap map((int)M);
    if (drop > 0) {
      map.update(world_xyz, world_app);
      std::vector<int> seen(M, 0);
      for (size_t f = 0; f < F; ++f) {
        std::vector<int32_t> ent;
        map.lookup(apps[f], nullptr, &ent);
        for (int32_t e : ent) if (e >= 0) ++seen[(size_t)e];
      }
      std::vector<int> candidates;
      for (size_t e = 0; e < M; ++e) if (seen[e] >= 3) candidates.push_back((int)e);
      if ((size_t)drop > candidates.size()) { std::printf("only %zu landmarks have three observations\n", candidates.size()); return -1; }
      std::mt19937 rng(seed);
      for (int k = 0; k < drop; ++k) {
        std::swap(candidates[(size_t)k], candidates[(size_t)k + rng() % (candidates.size() - (size_t)k)]);
        keep[(size_t)candidates[(size_t)k]] = 0;
      }
      map.clear();
    }
    vo::Vector3fVector start_xyz;
    vo::Vector10fVector start_app;
    for (size_t e = 0; e < M; ++e) if (keep[e]) { start_xyz.push_back(world_xyz[e]); start_app.push_back(world_app[e]); }
    if (!start_xyz.empty()) map.update(start_xyz, start_app);
    std::printf("map of %d entries (world.dat holds %zu), %zu frames", map.size(), M, F);
    if (drop > 0) std::printf(": %d landmarks with >= 3 observations taken out (seed %u)", drop, seed);
    std::printf("\n");

    std::vector<int32_t> rows;
    std::vector<voe_map_grow_track> tracks;
    const voe_map_grow_stats st = map.grow(data.camera(), pixels, apps, poses, opt, &rows, &tracks);
    std::printf("%d live rows: %d hit the map, %d hold a NaN, %d open in %d tracks;", st.n_live, st.n_hits, st.n_nan, st.n_open, st.n_tracks);
    for (int k = 0; k < 9; ++k) std::printf(" %s %d", vo::grow_verdict_name(k), st.by_verdict[k]);
    std::printf("\nadded %d to %d (%s)\n", st.n_added, st.n_before, st.status == VOE_MAP_GROW_OK ? "OK" : st.status == VOE_MAP_GROW_NO_OPEN_ROWS ? "NO_OPEN_ROWS" : "NOTHING_ADDED");

    // the distances of the added points to world.dat, matched by appearance
    std::map<std::string, size_t> by_app;
    for (size_t e = 0; e < M; ++e) by_app.emplace(bits_of(world_app[e]), e);
    vo::Vector3fVector now_xyz;
    vo::Vector10fVector now_app;
    map.read(now_xyz, now_app);
    std::vector<double> dist;
    int strangers = 0, refined = 0;
    for (const voe_map_grow_track& t : tracks) refined += t.verdict == VOE_MAP_GROW_ADDED && t.refined;
    bool in_place = (int)now_xyz.size() == st.n_after && st.n_after == st.n_before + st.n_added;
    for (size_t e = (size_t)st.n_before; e < now_xyz.size(); ++e) {
      const auto it = by_app.find(bits_of(now_app[e]));
      if (it == by_app.end()) { ++strangers; continue; }
      double d2 = 0;
      for (int a = 0; a < 3; ++a) { const double d = (double)now_xyz[e][a] - (double)world_xyz[it->second][a]; d2 += d * d; }
      dist.push_back(std::sqrt(d2));
    }
    std::sort(dist.begin(), dist.end());
    const double largest = dist.empty() ? 0.0 : dist.back(), median = dist.empty() ? 0.0 : dist[dist.size() / 2];
    std::printf("%zu added points matched to world.dat (%d of no landmark), %d refined: distance median %.4g, largest %.4g (bound %.4g)\n", dist.size(),
                strangers, refined, median, largest, bound);
    const bool ok = st.n_added > 0 && in_place && strangers == 0 && largest < bound;
    std::printf("%s\n", ok ? "the added landmarks lie where world.dat has them" : "the added landmarks do NOT lie where world.dat has them");
    return ok ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "grow_map: %s\n", e.what());
    return 2;
  }
}
