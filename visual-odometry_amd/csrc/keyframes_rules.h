// keyframes_rules.h -- the small integer rules of map_keyframes.hip (include/vo_hip.h: KEYFRAMES), as inline functions that the
// kernels and a host check (tests/hostcheck/keyframes_check.cpp) compile from this one text: the bit-sliced counters of how many
// frames see an entry (32 entries per word operation), the tests a candidate passes and the order of two candidates.  Nothing
// here forms a floating point number: every operation on the planes is an and, an xor or an or.
#ifndef VO_KEYFRAMES_RULES_H
#define VO_KEYFRAMES_RULES_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KEYFRAMES_HD __host__ __device__ inline
#else
#define KEYFRAMES_HD inline
#endif

namespace vo {

constexpr int KEYFRAMES_CHUNK = 256;          // 32-bit words of a row one workgroup takes at a time: one word per lane
constexpr int KEYFRAMES_MAX_PLANES = 13;      // 2^13 > VOE_MAP_COVIS_MAX_FRAMES = 4096: a count of frames fits 13 bits

// PLANES.  c[p] holds bit p of the counters of the 32 entries of one word: counter(e) = sum over p of ((c[p] >> e) & 1) << p.
// The planes a count of up to n_frames needs: the smallest P with 2^P >= n_frames + 1
KEYFRAMES_HD int keyframes_planes(int n_frames) {
  int P = 1;
  while (P < KEYFRAMES_MAX_PLANES && (1 << P) < n_frames + 1) ++P;
  return P;
}

// every counter whose bit of x is set goes up by one: a ripple carry.  (A counter at 2^P - 1 would wrap: keyframes_planes
// leaves room for every frame.)
KEYFRAMES_HD void keyframes_add(uint32_t* c, int P, uint32_t x) {
  uint32_t carry = x;
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) {
    if (p < P) {
      const uint32_t t = c[p] & carry;
      c[p] ^= carry;
      carry = t;
    }
  }
}

// every counter whose bit of x is set goes down by one: a ripple borrow.  (A counter at 0 would wrap: only rows that were
// added are taken out.)
KEYFRAMES_HD void keyframes_sub(uint32_t* c, int P, uint32_t x) {
  uint32_t borrow = x;
  for (int p = 0; p < KEYFRAMES_MAX_PLANES; ++p) {
    if (p < P) {
      const uint32_t t = ~c[p] & borrow;
      c[p] ^= borrow;
      borrow = t;
    }
  }
}

// the threshold of "cnt - 1 >= min_observers" as a count: min_observers + 1, cut to what 13 planes can tell apart (no counter
// reaches 2^13 - 1, as a count is at most 4096)
KEYFRAMES_HD uint32_t keyframes_threshold(int min_observers) {
  const long long t = (long long)min_observers + 1;
  const long long top = (1ll << KEYFRAMES_MAX_PLANES) - 1;
  return (uint32_t)(t < 0 ? 0 : t > top ? top : t);
}

// bit e of the result: counter(e) >= t, from the top plane down.  t at or above 2^P: no P-bit counter reaches it.
KEYFRAMES_HD uint32_t keyframes_ge(const uint32_t* c, int P, uint32_t t) {
  if (P < 32 && (t >> P) != 0u) return 0u;
  uint32_t gt = 0u, eq = ~0u;
  for (int p = KEYFRAMES_MAX_PLANES - 1; p >= 0; --p) {
    if (p < P) {
      if ((t >> p) & 1u) eq &= c[p];
      else { gt |= eq & c[p]; eq &= ~c[p]; }
    }
  }
  return gt | eq;
}

// CANDIDATES.  The share test: 1000 red >= share_permille seen, in int64
KEYFRAMES_HD bool keyframes_share_ok(int red, int seen, int share_permille) {
  return 1000ll * (long long)red >= (long long)share_permille * (long long)seen;
}

// candidate a = (red_a, seen_a, frame_a) goes before b: the higher share red / seen, compared by cross-multiplication in
// int64 (both seen >= 1); equal shares: the lower frame.  A frame below 0 is no candidate.
KEYFRAMES_HD bool keyframes_before(int red_a, int seen_a, int frame_a, int red_b, int seen_b, int frame_b) {
  if (frame_a < 0) return false;
  if (frame_b < 0) return true;
  const long long l = (long long)red_a * (long long)seen_b, r = (long long)red_b * (long long)seen_a;
  return l != r ? l > r : frame_a < frame_b;
}

// The gap rule for frame f, live[g] != 0 for the frames that are neither GONE nor dropped: with a the nearest live frame
// below f (-1 if none) and b the nearest above (n_frames if none), b - a - 1 <= max_gap.  The walk ends as soon as the run is
// too long, so it costs at most max_gap + 2 reads.
KEYFRAMES_HD bool keyframes_gap_ok(const uint8_t* live, int n_frames, int f, int max_gap) {
  int run = 1;                                 // f itself would be missing
  for (int a = f - 1; a >= 0 && !live[a]; --a)
    if (++run > max_gap) return false;
  for (int b = f + 1; b < n_frames && !live[b]; ++b)
    if (++run > max_gap) return false;
  return run <= max_gap;
}

}  // namespace vo
#endif
