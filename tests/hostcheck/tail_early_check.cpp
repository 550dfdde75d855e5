// How the early form of the tail launch picks the first repeat and what it then stores (csrc/vo_internal.h,
// picp_tail_first_repeat, picp_cycle_skips, picp_cycle_skip -- the functions the kernel calls), against a brute-force
// restatement of the launch-per-round solve: a trajectory of pose ids whose first repeat is pose k = pose j, the detector of
// every launch looking 63 rounds back, the most recent match winning.  All (k, j, N) with k <= 70.  Host code only: no device
// is touched.  Prints "ok <cases>" or the first mismatch.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vo_internal.h"

namespace {
constexpr int WINDOW = vo::PICP_HIST - 1;

struct Ref {
  int detected_at = 0, period = 0, skipped = 0, target = 0, skip_from = vo::PICP_CYCLE_RUN;
};

// the launches 1 .. last of the launch-per-round solve: launch `it` looks at the pose after round it - 1
Ref reference(const std::vector<int>& id, int last) {
  Ref r;
  for (int it = 1; it <= last; ++it) {
    const int p = it - 1;
    for (int l = 0; l < WINDOW; ++l) {
      const int e = p - 1 - l;
      if (e < 0 || id[e] != id[p]) continue;
      r.detected_at = it;
      r.period = l + 1;
      if (it + 1 < last) {
        const int j = p - r.period;
        r.skipped = last - 1 - it;
        r.target = j + (last - j) % r.period;
        r.skip_from = it + 1;
      }
      return r;
    }
  }
  return r;
}

int fail(const char* what, int k, int j, int n, int it) {
  printf("MISMATCH %s at k %d j %d N %d round %d\n", what, k, j, n, it);
  return 1;
}
}  // namespace

int main() {
  long cases = 0;
  for (int k = 1; k <= 70; ++k)
    for (int j = 0; j < k; ++j)
      for (int n = 3; n <= k + (k - j) + 6; ++n) {
        // (every N up to those that put the target on each residue of the period, and two beyond)
        const int last = n - 1, period = k - j;
        std::vector<int> id(n + 1);
        for (int r = 0; r <= n; ++r) id[r] = r < k ? r : id[r - period];
        const Ref want = reference(id, last);
        // a tail launch whose first in-launch round is it0, in state RUN: the rounds it runs until one of them finds a repeat
        const int stop = want.detected_at ? want.detected_at : last;
        // (from round 2, and from each of the four rounds up to the one whose launch finds the repeat: M = k - 3 .. k)
        for (int it0 = 2; it0 <= stop; it0 = it0 < stop - 3 ? stop - 3 : it0 + 1) {
          for (int it = it0; it <= last; ++it) {
            unsigned long long hn = 0, ho = 0;
            for (int l = 0; l < WINDOW; ++l) {
              if (it - 1 - l >= 0 && id[it - 1 - l] == id[it]) hn |= 1ull << l;
              if (it - 2 - l >= 0 && id[it - 2 - l] == id[it - 1]) ho |= 1ull << l;
            }
            int kf = -1, jf = -1;
            if (!vo::picp_tail_first_repeat(hn, ho, it, &kf, &jf)) continue;
            // the first round that sees a repeat sees the reference's, whichever of the two poses it is
            if (want.detected_at == 0) {
              // (the reference's launches end before the repeat shows: only the pose of round `last` itself may repeat)
              if (kf != last) return fail("a repeat the reference never sees", k, j, n, it);
              if (vo::picp_cycle_skips(kf, last)) return fail("skips beyond the last round", k, j, n, it);
              break;
            }
            if (kf + 1 != want.detected_at || kf - jf != want.period) return fail("first repeat", k, j, n, it);
            if (vo::picp_cycle_skips(kf, last) != (want.skipped > 0 || want.skip_from != vo::PICP_CYCLE_RUN))
              return fail("skips", k, j, n, it);
            if (vo::picp_cycle_skips(kf, last)) {
              const vo::PicpSkip s = vo::picp_cycle_skip(kf, jf, last);
              if (s.detected_at != want.detected_at || s.period != want.period || s.skipped != want.skipped ||
                  s.target != want.target || s.skip_from != want.skip_from)
                return fail("control block", k, j, n, it);
              if (id[s.target] != id[last]) return fail("target pose", k, j, n, it);
              if (s.target > kf - 1 || s.target < jf) return fail("target range", k, j, n, it);
            }
            ++cases;
            break;
          }
        }
      }
  printf("ok %ld\n", cases);
  return 0;
}
