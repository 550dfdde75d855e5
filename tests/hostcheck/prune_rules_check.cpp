// prune_rules_check.cpp -- the inline rules of visual-odometry_amd/csrc/prune_rules.h, compiled for the host with the sanitizers
// (tests/test_map_prune_cpu.py builds it with -fsanitize=address,undefined and runs it as a program) and held against brute force
// on a few thousand random small inputs: the guards against 128-bit products, also near 2^31 * 1000; the rank of the lower median
// and the order (sq, position) against a stable sort; the winner of a run of duplicates against the rule told per observation, as
// the kernels tell it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "prune_rules.h"

using namespace vo;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

int main() {
  std::mt19937_64 rng(20261021);
  // ---- the statuses ----
  int n_el = 0, n_soft = 0, n_pruned = 0;
  for (int s = 0; s < PS_COUNT; ++s) { n_el += prune_eligible(s); n_soft += prune_soft(s); n_pruned += prune_pruned(s); }
  CHECK(n_el == 5 && n_soft == 2 && n_pruned == 5);
  CHECK(prune_eligible(PS_KEPT) && prune_eligible(PS_LANDMARK_AT_FAULT) && prune_eligible(PS_FRAME_AT_FAULT) && !prune_eligible(PS_DUPLICATE));
  CHECK(!prune_pruned(PS_KEPT) && !prune_pruned(PS_MISS) && !prune_pruned(PS_NOT_LIVE) && !prune_pruned(PS_LANDMARK_AT_FAULT) && !prune_pruned(PS_FRAME_AT_FAULT));
  // ---- the guards: n_soft * 1000 > share * n_el, exactly ----
  const auto brute_guard = [](int64_t s, int64_t n, int64_t share) { return (__int128)s * 1000 > (__int128)share * n; };
  for (int t = 0; t < 4000; ++t) {
    const int n = (int)(rng() % 40), s = n ? (int)(rng() % (uint64_t)(n + 1)) : 0, share = (int)(rng() % 1001);
    CHECK(prune_guard_fires(s, n, share) == brute_guard(s, n, share));
  }
  for (int t = 0; t < 4000; ++t) {                                     // counts near 2^31: the products pass 2^31 * 1000
    const int n = INT32_MAX - (int)(rng() % 1000), s = n - (int)(rng() % 3000000), share = 997 + (int)(rng() % 4);
    CHECK(prune_guard_fires(s, n, share) == brute_guard(s, n, share));
  }
  CHECK(!prune_guard_fires(INT32_MAX, INT32_MAX, 1000) && prune_guard_fires(INT32_MAX, INT32_MAX, 999) && prune_guard_fires(1, INT32_MAX, 0));
  CHECK(!prune_guard_fires(1, 2, 500) && !prune_guard_fires(2, 4, 500) && prune_guard_fires(3, 4, 500) && prune_guard_fires(2, 2, 500));
  CHECK(!prune_guard_fires(0, 0, 0) && !prune_guard_fires(0, 5, 0) && prune_guard_fires(1, 5, 0));
  for (int n = 0; n <= 64; ++n)
    for (int s = 0; s <= n; ++s) CHECK(!prune_guard_fires(s, n, 1000));
  // ---- the lower median by rank count, as the kernels count: values from a small set, so that ties are common ----
  for (int t = 0; t < 3000; ++t) {
    const int n = 1 + (int)(rng() % 50);
    std::vector<double> sq(n);
    for (double& x : sq) x = (double)(rng() % 7) * 0.25;
    std::vector<int> order(n);
    for (int k = 0; k < n; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sq[a] < sq[b]; });
    const int target = prune_median_rank(n);
    CHECK(target == (n - 1) / 2 && target >= 0 && target < n);
    int holders = 0;
    for (int a = 0; a < n; ++a) {
      int rank = 0;
      for (int b = 0; b < n; ++b) rank += prune_before(sq[b], b, sq[a], a);
      CHECK(order[rank] == a);                                         // ranks are distinct and are the stable sort's places
      if (rank == target) { ++holders; CHECK(sq[a] == sq[order[target]]); }
    }
    CHECK(holders == 1);
    std::vector<double> sorted = sq;
    std::sort(sorted.begin(), sorted.end());
    CHECK(sorted[target] == sq[order[target]]);
    CHECK(n % 2 == 1 ? target == n / 2 : target == n / 2 - 1);
  }
  // ---- the winner of a run, against the rule told per observation ----
  for (int t = 0; t < 3000; ++t) {
    const int n = 1 + (int)(rng() % 9);
    std::vector<double> sq(n);
    std::vector<unsigned char> ok(n);
    for (int k = 0; k < n; ++k) { sq[k] = (double)(rng() % 5) * 0.5; ok[k] = rng() % 4 != 0; }
    const int w = prune_run_winner(sq.data(), ok.data(), n);
    int stays = 0;
    for (int a = 0; a < n; ++a) {
      if (!ok[a]) continue;
      bool dup = false;
      for (int b = 0; b < n; ++b) dup |= b != a && ok[b] && prune_before(sq[b], b, sq[a], a);
      if (!dup) { ++stays; CHECK(a == w); }
    }
    const bool any = std::any_of(ok.begin(), ok.end(), [](unsigned char x) { return x != 0; });
    CHECK(stays == (any ? 1 : 0) && (any || w == -1));
    if (any)
      for (int k = 0; k < n; ++k) CHECK(!ok[k] || sq[w] < sq[k] || (sq[w] == sq[k] && w <= k));
  }
  if (fails) { std::printf("prune_rules_check: %d failures\n", fails); return 1; }
  std::printf("prune_rules_check: ok\n");
  return 0;
}
