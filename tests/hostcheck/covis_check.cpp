// covis_check -- a host check of the inline rules of visual-odometry_amd/csrc/covis_rules.h, the text the kernels of
// map_covis.hip compile: the tile numbering of the upper triangle, the word / bit addressing and the rank key, each against a
// naive loop, on host arrays.  A stand-alone program; tests/test_map_covis_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it.  Exit 0 iff every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "covis_rules.h"

using namespace vo;

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

// every frame pair f <= g lies in exactly one launched tile, taken the way covis_count_kernel takes it: tile (ti, tj), rows
// ti * TILE + 0 .. TILE - 1 against tj * TILE + 0 .. TILE - 1, stored at (f, g) and -- off the diagonal -- mirrored at (g, f)
static void check_tiles(int F) {
  const int T = covis_tiles_edge(F), n = covis_tiles(F);
  std::vector<int> hit((size_t)F * F, 0);
  int prev_i = 0, prev_j = -1;
  for (int t = 0; t < n; ++t) {
    int ti = -1, tj = -1;
    covis_tile(t, T, &ti, &tj);
    CHECK(0 <= ti && ti <= tj && tj < T, "F %d tile %d -> (%d, %d) of %d", F, t, ti, tj, T);
    CHECK((ti == prev_i && tj == prev_j + 1) || (ti == prev_i + 1 && tj == ti && prev_j == T - 1), "F %d tile %d: not row by row", F, t);
    prev_i = ti; prev_j = tj;
    for (int r = 0; r < COVIS_TILE; ++r)
      for (int c = 0; c < COVIS_TILE; ++c) {
        const int f = ti * COVIS_TILE + r, g = tj * COVIS_TILE + c;
        if (f >= F || g >= F) continue;
        ++hit[(size_t)f * F + g];
        if (ti != tj) ++hit[(size_t)g * F + f];
      }
  }
  for (int f = 0; f < F; ++f)
    for (int g = 0; g < F; ++g) CHECK(hit[(size_t)f * F + g] == 1, "F %d: pair (%d, %d) written %d times", F, f, g, hit[(size_t)f * F + g]);
  CHECK(n == T * (T + 1) / 2 && T * COVIS_TILE >= F && (T - 1) * COVIS_TILE < F, "F %d: %d tiles along an edge, %d launched", F, T, n);
}

// setting bits through the helpers equals a naive array of booleans, for sizes at the word edges; rows of an odd word count
static void check_bits(int size, int n_frames) {
  const int W = covis_words_for(size) + (size % 3 == 0 ? 1 : 0);     // sometimes a word more than needed
  std::vector<uint32_t> bits((size_t)n_frames * W, 0u);
  std::vector<char> naive((size_t)n_frames * size, 0);
  unsigned s = 12345u + (unsigned)size;
  for (int k = 0; k < 4 * size + 8; ++k) {
    s = s * 1664525u + 1013904223u;
    const int f = (int)((s >> 8) % (unsigned)n_frames), e = (int)((s >> 12) % (unsigned)size);
    CHECK(covis_word(e) < W && covis_word(e) == e / 32 && covis_bit(e) == (1u << (e % 32)), "entry %d", e);
    bits[covis_row(f, W) + (size_t)covis_word(e)] |= covis_bit(e);
    naive[(size_t)f * size + e] = 1;
  }
  for (int e : {0, size - 1}) { bits[covis_row(n_frames - 1, W) + (size_t)covis_word(e)] |= covis_bit(e); naive[(size_t)(n_frames - 1) * size + e] = 1; }
  for (int f = 0; f < n_frames; ++f)
    for (int b = 0; b < 32 * W; ++b) {
      const bool set = (bits[(size_t)f * W + b / 32] >> (b % 32)) & 1u;
      CHECK(set == (b < size && naive[(size_t)f * size + b]), "size %d frame %d bit %d", size, f, b);
    }
  CHECK(covis_words_for(size) == (size + 31) / 32 && 32 * covis_words_for(size) >= size && 32 * (covis_words_for(size) - 1) < size, "size %d", size);
}

// ascending keys are (count descending, frame ascending), ties included
static void check_rank(int F) {
  std::vector<int> count((size_t)F);
  unsigned s = 99u + (unsigned)F;
  for (int g = 0; g < F; ++g) { s = s * 1664525u + 1013904223u; count[(size_t)g] = (int)((s >> 16) % 7u) * (g % 5 == 0 ? 100000 : 1); }
  if (F > 2) count[(size_t)F - 1] = count[0];                // a tie between the first and the last frame
  std::vector<int> naive((size_t)F), by_key((size_t)F);
  for (int g = 0; g < F; ++g) naive[(size_t)g] = by_key[(size_t)g] = g;
  std::stable_sort(naive.begin(), naive.end(), [&](int a, int b) { return count[(size_t)a] != count[(size_t)b] ? count[(size_t)a] > count[(size_t)b] : a < b; });
  std::sort(by_key.begin(), by_key.end(), [&](int a, int b) { return covis_rank_key(count[(size_t)a], a) < covis_rank_key(count[(size_t)b], b); });
  CHECK(naive == by_key, "F %d: the key's order is not (count descending, frame ascending)", F);
  for (int g = 0; g < F; ++g) {                              // the counting rank the kernels use
    int r = 0;
    for (int h = 0; h < F; ++h) r += covis_rank_key(count[(size_t)h], h) < covis_rank_key(count[(size_t)g], g);
    CHECK(naive[(size_t)r] == g, "F %d: frame %d has counting rank %d", F, g, r);
  }
  CHECK(covis_rank_key(0x7fffffff, 0) < covis_rank_key(0, 0) && covis_rank_key(0, 4095) < ~0ull, "the key's range");
}

int main() {
  const int frames[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257};
  for (int F : frames) check_tiles(F);
  for (int F : frames) check_rank(F);
  const int sizes[] = {1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049};
  for (int size : sizes) check_bits(size, 3);
  std::printf(failures ? "covis_check: %d FAILED\n" : "covis_check: ok (%d)\n", failures);
  return failures ? 1 : 0;
}
