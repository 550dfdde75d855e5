// fuse_map -- duplicate landmarks in a map whose appearances REPEAT: the landmarks of world.dat get appearances folded into 50
// classes of 20 near-copies (class centre + N(0, 0.002)), 300 of them are entered a second time -- the point pushed by
// U(-0.015, 0.015), the appearance by N(0, 0.005), as a revisit under a drifted prior leaves them --, and a window of frames sees
// every landmark through either copy.  ONE voe_map_fuse call (radius 0.1, radius_xyz 0.04: world.dat's closest two landmarks are
// 0.051 apart; the veto on) has to fuse exactly the planted pairs and hand back rows that the exact lookup finds at
// remap[the entry it found before].
//   usage: fuse_map <data dir> [--seed=1] [--radius=0.1] [--radius-xyz=0.04] [--every=6]
// Exit 0 iff exactly the planted pairs were fused and every rewritten row obeys rule 7 of FUSE (include/vo_hip.h).
#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>
#include <set>

#include "known_common.hpp"

int main(int argc, char* argv[]) {
  unsigned seed = 1;
  int every = 6;
  vo::FuseOptions opt;
  opt.radius = 0.1f;
  opt.radius_xyz = 0.04f;
  opt.midpoint = false;
  opt.veto_shared_frame = true;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    const std::string s(argv[i]);
    if (s.rfind("--seed=", 0) == 0) seed = (unsigned)std::atoi(s.c_str() + 7);
    else if (s.rfind("--radius=", 0) == 0) opt.radius = (float)std::atof(s.c_str() + 9);
    else if (s.rfind("--radius-xyz=", 0) == 0) opt.radius_xyz = (float)std::atof(s.c_str() + 13);
    else if (s.rfind("--every=", 0) == 0) every = std::atoi(s.c_str() + 8);
    else if (s.rfind("--", 0) == 0) { std::printf("unknown option %s\n", s.c_str()); return -1; }
    else pos.push_back(s);
  }
  if (pos.empty() || every < 1) { std::printf("usage: fuse_map <data dir> [--seed=1] [--radius=0.1] [--radius-xyz=0.04] [--every=6]\n"); return -1; }
  std::string path = pos[0];
  if (path.back() != '/') path.push_back('/');
  try {
    known::Dataset data;
    if (!known::load_dataset(path, data, false)) return -1;
    vo::Vector10fVector world_app;
    vo::Vector3fVector world_xyz;
    if (!vo::get_meas_content(path + "world.dat", world_app, world_xyz, true)) { std::printf("unable to read %sworld.dat\n", path.c_str()); return -1; }
    const size_t L = world_xyz.size(), n_classes = 50, n_dup = std::min<size_t>(300, L);

    // the folded appearances, then the planted duplicates
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> centre(-1.f, 1.f), push(-0.015f, 0.015f);
    std::normal_distribution<float> within(0.f, 0.002f), noise(0.f, 0.005f);
    std::vector<std::array<float, 10>> classes(n_classes);
    for (auto& c : classes) for (int k = 0; k < 10; ++k) c[k] = centre(rng);
    vo::Vector10fVector app(L);
    for (size_t j = 0; j < L; ++j) for (int k = 0; k < 10; ++k) app[j][k] = classes[j % n_classes][k] + within(rng);
    std::vector<int> order(L);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<int> chosen(order.begin(), order.begin() + n_dup), copy_of(L, -1);
    std::sort(chosen.begin(), chosen.end());
    vo::Vector3fVector xyz = world_xyz;
    std::set<std::pair<int, int>> planted;
    for (size_t d = 0; d < n_dup; ++d) {
      const int j = chosen[d];
      vo::Vector3f p = world_xyz[j];
      vo::Vector10f a = app[j];
      for (int k = 0; k < 3; ++k) p[k] += push(rng);
      for (int k = 0; k < 10; ++k) a[k] += noise(rng);
      copy_of[j] = (int)xyz.size();
      planted.insert({j, (int)xyz.size()});
      xyz.push_back(p);
      app.push_back(a);
    }
    vo::DeviceMap map((int)xyz.size());
    map.update(xyz, app);

    // the window: every row goes to one of its landmark's copies
    std::vector<vo::Vector10fVector> frames;
    std::vector<std::vector<int>> before;
    std::bernoulli_distribution coin(0.5);
    size_t rows = 0, on_copies = 0;
    for (size_t f = 0; f < data.meas_files.size(); f += (size_t)every) {
      vo::Vector3fVector meas_with_id;
      vo::Vector10fVector unused;
      if (!vo::get_meas_content(path + data.meas_files[f], unused, meas_with_id)) { std::printf("unable to read %s\n", (path + data.meas_files[f]).c_str()); return -1; }
      vo::Vector10fVector a;
      std::vector<int> ent;
      for (const auto& m : meas_with_id) {
        const int id = (int)m.x();
        const int e = copy_of[id] >= 0 && coin(rng) ? copy_of[id] : id;
        a.push_back(app[e]);
        ent.push_back(e);
        on_copies += e != id;
      }
      rows += a.size();
      frames.push_back(a);
      before.push_back(ent);
    }
    bool lookup_ok = true;
    for (size_t f = 0; f < frames.size(); ++f) {
      const vo::IntPairVector hits = map.lookup(frames[f]);
      lookup_ok = lookup_ok && hits.size() == frames[f].size();
      for (size_t i = 0; lookup_ok && i < hits.size(); ++i) lookup_ok = hits[i].first == (int)i && hits[i].second == before[f][i];
    }
    std::printf("map of %d entries: %zu landmarks in %zu appearance classes, %zu entered twice; %zu frames, %zu rows, %zu on the second copies; the exact "
                "lookup before the fuse %s\n", map.size(), L, n_classes, n_dup, frames.size(), rows, on_copies, lookup_ok ? "finds every row" : "MISSES rows");

    const vo::MapFuse r = map.fuse(opt, frames);
    const voe_map_fuse_stats& s = r.stats;
    std::printf("voe_map_fuse (radius %g, radius_xyz %g): status %s, %d -> %d entries, %d pairs fused, %d vetoed, %d rows rewritten, %lld pairs passed the "
                "spatial gate\n", opt.radius, opt.radius_xyz, s.status == VOE_MAP_FUSE_OK ? "OK" : "NOTHING_FUSED", s.n_before, s.n_after, s.n_pairs,
                s.n_conflicts, s.n_rows_rewritten, (long long)s.n_gated);
    for (int v = 0; v < 6; ++v) std::printf("  %s %d\n", vo::fuse_verdict_name(v), s.by_verdict[v]);
    std::set<std::pair<int, int>> fused;
    for (size_t e = 0; e < r.verdict.size(); ++e)
      if (r.verdict[e] == VOE_MAP_FUSE_SURVIVOR) fused.insert({(int)e, r.partner[e]});
    const bool pairs_ok = fused == planted && s.n_after == (int)L && map.size() == (int)L;
    bool rows_ok = (size_t)s.n_rows_rewritten == on_copies;
    for (size_t f = 0; f < frames.size(); ++f) {
      const vo::IntPairVector hits = map.lookup(r.rows[f]);
      rows_ok = rows_ok && hits.size() == frames[f].size();
      for (size_t i = 0; rows_ok && i < hits.size(); ++i) rows_ok = hits[i].first == (int)i && hits[i].second == r.remap[before[f][i]];
    }
    std::printf("%s; the exact lookup of the rewritten rows %s\n", pairs_ok ? "exactly the planted pairs were fused" : "the fused pairs are NOT the planted ones",
                rows_ok ? "returns remap[the entry before] at every position" : "does NOT obey rule 7");
    return lookup_ok && pairs_ok && rows_ok ? 0 : 1;
  } catch (const vo::Error& e) {
    std::fprintf(stderr, "fuse_map: %s\n", e.what());
    return 2;
  }
}
