// keyframes_check -- a host check of the inline rules of visual-odometry_amd/csrc/keyframes_rules.h, the text the kernels of
// map_keyframes.hip compile: the bit-sliced counters (add a row, take a row out, "count >= t" as a mask) against plain integer
// counters per bit, on random words and on the carry edges; the share test, the order of two candidates and the gap rule against
// naive forms.  A stand-alone program; tests/test_map_keyframes_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it.  Exit 0 iff every check holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "keyframes_rules.h"

using namespace vo;

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

static unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (s >> 4) ^ (s << 9); }

// counter e of the planes, read back bit by bit
static int counter(const uint32_t* c, int P, int e) {
  int v = 0;
  for (int p = 0; p < P; ++p) v |= (int)((c[p] >> e) & 1u) << p;
  return v;
}

static void compare(const uint32_t* c, int P, const int* naive, const char* what, int k) {
  for (int e = 0; e < 32; ++e) CHECK(counter(c, P, e) == naive[e], "%s %d: counter %d is %d, not %d (P %d)", what, k, e, counter(c, P, e), naive[e], P);
  for (int p = P; p < KEYFRAMES_MAX_PLANES; ++p) CHECK(c[p] == 0xDEADBEEFu, "%s %d: plane %d beyond P %d written", what, k, p, P);
  // the mask of every threshold that can occur, and of some that cannot
  for (uint32_t t = 0; t <= (1u << P) + 2u; ++t) {
    uint32_t want = 0u;
    for (int e = 0; e < 32; ++e) want |= (uint32_t)((uint32_t)naive[e] >= t) << e;
    CHECK(keyframes_ge(c, P, t) == want, "%s %d: count >= %u gives %08x, not %08x (P %d)", what, k, t, keyframes_ge(c, P, t), want, P);
  }
  CHECK(keyframes_ge(c, P, (1u << KEYFRAMES_MAX_PLANES) - 1u) == 0u || P == KEYFRAMES_MAX_PLANES, "%s %d: the cut threshold", what, k);
}

// n_frames rows go in, in an order, and come out in another: after every operation the planes equal the naive counters
static void check_planes(int n_frames, unsigned seed, int density) {
  const int P = keyframes_planes(n_frames);
  CHECK((1 << P) >= n_frames + 1 && (P == 1 || (1 << (P - 1)) < n_frames + 1) && P <= KEYFRAMES_MAX_PLANES, "planes for %d frames: %d", n_frames, P);
  uint32_t c[KEYFRAMES_MAX_PLANES];
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) c[p] = p < P ? 0u : 0xDEADBEEFu;
  int naive[32] = {0};
  std::vector<uint32_t> rows((size_t)n_frames);
  unsigned s = seed;
  for (int f = 0; f < n_frames; ++f) {
    uint32_t x = 0u;
    for (int e = 0; e < 32; ++e) x |= (uint32_t)((int)(rnd(s) % 100u) < density) << e;
    if (density >= 100) x = ~0u;
    x |= 1u | 1u << 31;                                     // bits 0 and 31 count every frame: the carries run the whole way
    rows[(size_t)f] = x;
  }
  const int stride = n_frames < 300 ? 1 : n_frames / 150;   // (the threshold sweep is the cost: not after every row of 4096)
  for (int f = 0; f < n_frames; ++f) {
    keyframes_add(c, P, rows[(size_t)f]);
    for (int e = 0; e < 32; ++e) naive[e] += (int)((rows[(size_t)f] >> e) & 1u);
    if (f % stride == 0 || f >= n_frames - 3) compare(c, P, naive, "add", f);
  }
  CHECK(naive[0] == n_frames && naive[31] == n_frames, "every frame counted");
  // out again, odd frames first and from the top, then the even ones
  int k = 0;
  for (int pass = 1; pass >= 0; --pass)
    for (int f = n_frames - 1; f >= 0; --f) {
      if ((f & 1) != pass) continue;
      keyframes_sub(c, P, rows[(size_t)f]);
      for (int e = 0; e < 32; ++e) naive[e] -= (int)((rows[(size_t)f] >> e) & 1u);
      if (k % stride == 0 || k >= n_frames - 3) compare(c, P, naive, "sub", k);
      ++k;
    }
  for (int p = 0; p < P; ++p) CHECK(c[p] == 0u, "plane %d is not empty after every row left", p);
}

static void check_threshold() {
  CHECK(keyframes_threshold(1) == 2u && keyframes_threshold(3) == 4u && keyframes_threshold(4095) == 4096u, "min_observers + 1");
  CHECK(keyframes_threshold(8190) == 8191u && keyframes_threshold(8191) == 8191u && keyframes_threshold(0x7fffffff) == 8191u, "the cut");
  uint32_t c[KEYFRAMES_MAX_PLANES];
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) c[p] = (4096u >> p) & 1u ? ~0u : 0u;       // every counter at 4096
  CHECK(keyframes_ge(c, KEYFRAMES_MAX_PLANES, 4096u) == ~0u && keyframes_ge(c, KEYFRAMES_MAX_PLANES, 4097u) == 0u, "4096 frames");
  CHECK(keyframes_ge(c, KEYFRAMES_MAX_PLANES, keyframes_threshold(0x7fffffff)) == 0u, "no count reaches the cut threshold");
}

static void check_candidates() {
  // the share test at its edge, and where int32 products would overflow
  CHECK(keyframes_share_ok(9, 10, 900) && !keyframes_share_ok(899, 1000, 900) && keyframes_share_ok(899, 1000, 899), "900 per mille");
  CHECK(keyframes_share_ok(0, 5, 0) && !keyframes_share_ok(0, 5, 1) && keyframes_share_ok(5, 5, 1000) && !keyframes_share_ok(4, 5, 1000), "the ends");
  CHECK(keyframes_share_ok(0x7fffffff, 0x7fffffff, 1000) && !keyframes_share_ok(0x7ffffffe, 0x7fffffff, 1000), "int64");
  // the order: against exact fractions in long long, ties to the lower frame, a frame below 0 is no candidate
  unsigned s = 99u;
  for (int k = 0; k < 20000; ++k) {
    const int sa = 1 + (int)(rnd(s) % 40u), sb = 1 + (int)(rnd(s) % 40u);
    const int ra = (int)(rnd(s) % (unsigned)(sa + 1)), rb = (int)(rnd(s) % (unsigned)(sb + 1));
    const int fa = (int)(rnd(s) % 50u), fb = (fa + 1 + (int)(rnd(s) % 49u)) % 50;
    const long long l = (long long)ra * sb, r = (long long)rb * sa;
    const bool want = l > r || (l == r && fa < fb);
    CHECK(keyframes_before(ra, sa, fa, rb, sb, fb) == want, "%d/%d frame %d against %d/%d frame %d", ra, sa, fa, rb, sb, fb);
    CHECK(keyframes_before(ra, sa, fa, rb, sb, fb) != keyframes_before(rb, sb, fb, ra, sa, fa), "one of two goes first");
  }
  CHECK(keyframes_before(9, 10, 3, 18, 20, 5) && !keyframes_before(18, 20, 5, 9, 10, 3), "equal shares in other terms: the lower frame");
  CHECK(keyframes_before(12000, 12001, 1, 11999, 12000, 0), "a difference float32 does not see");
  CHECK(keyframes_before(0x7fffffff, 0x7fffffff, 1, 0x7ffffffe, 0x7fffffff, 0), "products beyond int32");
  CHECK(!keyframes_before(1, 1, -1, 0, 1, 4) && keyframes_before(0, 1, 4, 1, 1, -1) && !keyframes_before(0, 1, -1, 0, 1, -1), "no candidate");
}

static void check_gap() {
  unsigned s = 7u;
  for (int k = 0; k < 4000; ++k) {
    const int F = 1 + (int)(rnd(s) % 14u);
    std::vector<uint8_t> live((size_t)F);                   // (exactly F bytes: a step outside is the sanitizer's to see)
    for (int f = 0; f < F; ++f) live[(size_t)f] = rnd(s) % 3u != 0u;
    for (int f = 0; f < F; ++f)
      for (int g = 1; g <= 5; ++g) {
        int a = f - 1, b = f + 1;
        while (a >= 0 && !live[(size_t)a]) --a;
        while (b < F && !live[(size_t)b]) ++b;
        CHECK(keyframes_gap_ok(live.data(), F, f, g) == (b - a - 1 <= g), "F %d frame %d max_gap %d", F, f, g);
      }
  }
}

int main() {
  for (int F : {1, 2, 3, 4, 7, 8, 9, 15, 16, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256, 1023, 1024, 4095, 4096}) {
    check_planes(F, 17u + (unsigned)F, 50);
    check_planes(F, 29u + (unsigned)F, 100);                // every counter at every count up to F
    check_planes(F, 43u + (unsigned)F, 3);
  }
  check_threshold();
  check_candidates();
  check_gap();
  if (failures) { std::printf("keyframes_check: %d FAILED\n", failures); return 1; }
  std::printf("keyframes_check: ok\n");
  return 0;
}
