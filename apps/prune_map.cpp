// prune_map -- single observations taken back on a data directory whose answer is known: the map is world.dat, the poses are
// those of trajectory.dat (obtained as refine_map obtains them), and a seeded generator plants three kinds of fault:
//   `pushed` landmarks that at least `min-obs` rows see (and that lie at least 1 in front of their cameras) are moved by
//   +-0.2 ... 0.4 per coordinate; the poses of frames F/4, F/2 and 3F/4 are moved by 0.05 in every coordinate of t; `wrong` rows of
//   such landmarks, outside those frames, are given the appearance of a random OTHER such landmark that is not pushed (a wrong
//   association: the row now observes that landmark, at the wrong pixel).
// ONE voe_map_prune call (max_err_px = px, unique, the landmark guard at 500 and the frame guard at 300 per mille) has to prune
// exactly the wrong rows that sit on no named landmark or frame, and to name exactly the pushed landmarks and the pushed frames.
//   usage: prune_map <data dir> [--seed=1] [--wrong=100] [--pushed=20] [--px=1] [--min-obs=5]
// Printed: what a dry-run voe_map_cull(max_err_px = px) would drop; what the call prunes and names; the cost per observation that
// two rounds of vox_map_bundle end at on the pruned rows against the unpruned ones, each after vo_map_refine and
// vo_map_refine_poses of what was named.  Exit 0 iff the three conditions above hold.
// (The draw takes landmarks with >= 5 observations: a wrong row on a landmark seen twice is half of its observations, and the
// landmark guard at 500 per mille would -- rightly -- refuse to tell which of the two is wrong.)
#include <algorithm>
#include <cmath>
#include <random>
#include <set>

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

const char* bundle_status_name(int s) {
  static const char* names[] = {"OK", "NOT_FINITE", "BEHIND", "NOTHING_FREE", "NO_STEP", "COST_ROSE"};
  return s >= 0 && s < 6 ? names[s] : "?";
}
}  // namespace

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  int wrong = 100, pushed_n = 20, min_obs = 5;
  double px = 1.0;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--wrong=", 0) == 0) wrong = std::atoi(s.c_str() + 8);
    else if (s.rfind("--pushed=", 0) == 0) pushed_n = std::atoi(s.c_str() + 9);
    else if (s.rfind("--px=", 0) == 0) px = std::atof(s.c_str() + 5);
    else if (s.rfind("--min-obs=", 0) == 0) min_obs = std::atoi(s.c_str() + 10);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || wrong < 0 || pushed_n < 0 || min_obs < 3) {
    std::printf("usage: prune_map <data dir> [--seed=1] [--wrong=100] [--pushed=20] [--px=1] [--min-obs=5]\n");
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
    if (F < 4 || gt.size() < F) { std::printf("trajectory.dat holds %zu poses for %zu frames\n", gt.size(), F); return -1; }

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

    // the entries every frame's rows find on the clean data, and how often each landmark is seen
    vo::DeviceMap map((int)M);
    map.update(world_xyz, world_app);
    std::vector<std::vector<int32_t>> before(F);
    std::vector<int> seen(M, 0);
    for (size_t f = 0; f < F; ++f) {
      map.lookup(apps[f], nullptr, &before[f]);
      for (int32_t e : before[f]) if (e >= 0) ++seen[(size_t)e];
    }
    std::vector<int> candidates;
    std::vector<std::pair<int, int>> rows;                    // the rows of the candidates
    for (size_t e = 0; e < M; ++e) if (seen[e] >= min_obs) candidates.push_back((int)e);
    for (size_t f = 0; f < F; ++f)
      for (size_t i = 0; i < before[f].size(); ++i)
        if (before[f][i] >= 0 && seen[(size_t)before[f][i]] >= min_obs) rows.push_back({(int)f, (int)i});
    if ((size_t)pushed_n > candidates.size() || candidates.size() < 2) {
      std::printf("only %zu landmarks have %d observations\n", candidates.size(), min_obs);
      return -1;
    }

    // 1. pushed landmarks: a partial Fisher-Yates draw among the candidates at least 1 in front of every camera that sees them (a
    //    push of up to 0.4 per coordinate must not put an innocent row behind its camera), then a step of 0.2 ... 0.4 with a drawn
    //    sign per coordinate
    std::mt19937 rng(seed);
    std::vector<double> z_min(M, 1e300);
    for (size_t f = 0; f < F; ++f)
      for (size_t i = 0; i < before[f].size(); ++i)
        if (before[f][i] >= 0) {
          const size_t e = (size_t)before[f][i];
          const vo::Isometry3f& T = poses[f];
          z_min[e] = std::fmin(z_min[e], (double)T(2, 0) * world_xyz[e][0] + (double)T(2, 1) * world_xyz[e][1] + (double)T(2, 2) * world_xyz[e][2] + (double)T(2, 3));
        }
    std::vector<int> deep;
    for (int e : candidates) if (z_min[(size_t)e] > 1.0) deep.push_back(e);
    if ((size_t)pushed_n > deep.size()) { std::printf("only %zu candidates lie 1 in front of their cameras\n", deep.size()); return -1; }
    for (int k = 0; k < pushed_n; ++k) std::swap(deep[(size_t)k], deep[(size_t)k + rng() % (deep.size() - (size_t)k)]);
    std::vector<uint8_t> pushed(M, 0);
    vo::Vector3fVector start = world_xyz;
    std::uniform_real_distribution<double> step(0.2, 0.4);
    for (int k = 0; k < pushed_n; ++k) {
      const size_t e = (size_t)deep[(size_t)k];
      pushed[e] = 1;
      for (int a = 0; a < 3; ++a) { const double s = step(rng); start[e][a] = (float)((double)start[e][a] + ((rng() & 1u) ? s : -s)); }
    }
    // 2. pushed poses
    std::vector<uint8_t> pushed_frame(F, 0);
    for (size_t f : {F / 4, F / 2, 3 * F / 4}) {
      pushed_frame[f] = 1;
      for (int a = 0; a < 3; ++a) poses[f](a, 3) += 0.05f;
    }
    // 3. wrong associations: a partial Fisher-Yates draw of rows outside the pushed frames, each given the appearance of another
    //    candidate that is not pushed.  (The hard tests need no context: a wrong row that lands behind its camera is pruned also on
    //    a named landmark or in a named frame, so the draw keeps the two apart.)
    std::vector<std::pair<int, int>> free_rows;
    for (const auto& fi : rows) if (!pushed_frame[(size_t)fi.first]) free_rows.push_back(fi);
    std::vector<int> targets;
    for (int e : candidates) if (!pushed[(size_t)e]) targets.push_back(e);
    if ((size_t)wrong > free_rows.size() || targets.size() < 2) { std::printf("too few rows or targets for %d wrong associations\n", wrong); return -1; }
    std::set<std::pair<int, int>> planted;
    std::vector<int32_t> planted_on;                          // the landmark a planted row now observes, in the order of `order`
    std::vector<std::pair<int, int>> order;
    for (int k = 0; k < wrong; ++k) {
      std::swap(free_rows[(size_t)k], free_rows[(size_t)k + rng() % (free_rows.size() - (size_t)k)]);
      const int f = free_rows[(size_t)k].first, i = free_rows[(size_t)k].second;
      int other;
      do other = targets[rng() % targets.size()]; while (other == before[(size_t)f][(size_t)i]);
      apps[(size_t)f][(size_t)i] = world_app[(size_t)other];
      planted.insert({f, i}); order.push_back({f, i}); planted_on.push_back(other);
    }
    map.clear();
    map.update(start, world_app);
    std::printf("map of %d entries, %zu frames, %zu landmarks with >= %d observations (seed %u): %d rows re-pointed to another such landmark, %d such "
                "landmarks pushed by 0.2 ... 0.4, frames %zu, %zu and %zu pushed by 0.05 in t\n",
                map.size(), F, candidates.size(), min_obs, seed, wrong, pushed_n, F / 4, F / 2, 3 * F / 4);

    // what the only remover would do
    vo::CullOptions copt;
    copt.min_obs = 1; copt.min_frames = 1; copt.max_rms_px = 0.f; copt.max_err_px = (float)px; copt.dry_run = true;
    const voe_map_cull_stats cst = map.cull(data.camera(), pixels, apps, poses, copt);
    std::printf("a dry-run voe_map_cull(max_err_px = %g) would drop %d of %d landmarks\n", px, cst.n_before - cst.n_kept, cst.n_before);

    // ONE call
    vo::PruneOptions opt;
    opt.max_err_px = (float)px; opt.unique = true; opt.max_share_landmark = 500; opt.max_share_frame = 300;
    const vo::MapPrune r = map.prune(data.camera(), pixels, apps, poses, opt);
    std::printf("%d observations; pruned %d:", r.stats.n_obs, r.stats.n_pruned);
    for (int k = VOE_MAP_PRUNE_NOT_FINITE; k <= VOE_MAP_PRUNE_FRAME_AT_FAULT; ++k) std::printf(" %s %d", vo::prune_status_name(k), r.stats.by_status[k]);
    std::printf("\nnamed %d landmarks and %d frames\n", r.stats.n_landmarks_at_fault, r.stats.n_frames_at_fault);

    bool landmarks_exact = true, frames_exact = true, rows_exact = true;
    for (size_t e = 0; e < M; ++e) if ((r.landmarks[e].at_fault != 0) != (pushed[e] != 0)) landmarks_exact = false;
    for (size_t f = 0; f < F; ++f) if ((r.frames[f].at_fault != 0) != (pushed_frame[f] != 0)) frames_exact = false;
    std::set<std::pair<int, int>> expected;
    int on_named = 0;
    for (size_t k = 0; k < order.size(); ++k) {
      const bool named = r.landmarks[(size_t)planted_on[k]].at_fault != 0 || r.frames[(size_t)order[k].first].at_fault != 0;
      if (named) ++on_named; else expected.insert(order[k]);
    }
    int innocent = 0, missed = 0;
    for (size_t f = 0; f < F; ++f)
      for (size_t i = 0; i < r.n_max; ++i) {
        const int s = r.status[f * r.n_max + i];
        const bool cut = s >= VOE_MAP_PRUNE_NOT_FINITE && s <= VOE_MAP_PRUNE_RELATIVE, want = expected.count({(int)f, (int)i}) != 0;
        if (cut && !want) ++innocent;
        if (!cut && want) ++missed;
      }
    rows_exact = innocent == 0 && missed == 0;
    std::printf("%d of the %d planted rows sit on a named landmark or frame and stay; of the others %d were missed, %d innocent rows were pruned\n",
                on_named, wrong, missed, innocent);
    std::printf("the pruned rows are %s; the named landmarks are %s; the named frames are %s\n", rows_exact ? "exactly those" : "NOT those",
                landmarks_exact ? "exactly the pushed ones" : "NOT the pushed ones", frames_exact ? "exactly the pushed ones" : "NOT the pushed ones");

    // downstream: refine what was named, then two bundle rounds -- on the pruned rows, and the same on the unpruned ones
    std::vector<uint8_t> hold(F, 1), gauge(F, 0);
    for (size_t f = 0; f < F; ++f) if (r.frames[f].at_fault) hold[f] = 0;
    gauge[0] = gauge[F - 1] = 1;
    vo::BundleOptions bopt;
    bopt.n_rounds = 2;
    double cost[2] = {0, 0};
    for (int run = 0; run < 2; ++run) {
      const std::vector<vo::Vector10fVector>& rows_in = run == 0 ? r.appearances : apps;
      vo::IsometryVector T = poses;
      map.clear();
      map.update(start, world_app);
      map.refine(data.camera(), pixels, rows_in, T);
      map.refinePoses(data.camera(), pixels, rows_in, T, &hold);
      const vox_map_bundle_stats b = map.bundle(data.camera(), pixels, rows_in, T, &gauge, bopt);
      cost[run] = b.n_obs > 0 ? b.cost_after / b.n_obs : 0.0;
      std::printf("vox_map_bundle on the %s rows: %s, %d observations, cost per observation %.6g -> %.6g px^2\n", run == 0 ? "pruned" : "unpruned",
                  bundle_status_name(b.status), b.n_obs, b.n_obs > 0 ? b.cost_before / b.n_obs : 0.0, cost[run]);
    }
    return rows_exact && landmarks_exact && frames_exact ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "prune_map: %s\n", e.what());
    return 2;
  }
}
