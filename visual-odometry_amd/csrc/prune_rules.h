// prune_rules.h -- the small decisions of map_prune.hip (include/vo_hip.h: PRUNE) that are made on whole numbers or on an order,
// as inline functions that the kernels and a host check (tests/hostcheck/prune_rules_check.cpp) compile from this one text: the
// two guards' comparison in int64, the rank of the lower median, the order (sq, key) of two observations and the winner of a
// run of duplicates.  No function here adds, multiplies or rounds a floating point number: doubles are only compared.
#ifndef VO_PRUNE_RULES_H
#define VO_PRUNE_RULES_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PRUNE_HD __host__ __device__ inline
#else
#define PRUNE_HD inline
#endif

namespace vo {

// the statuses of rule 9, as the kernels write them
enum {
  PS_KEPT = 0, PS_NOT_LIVE = 1, PS_MISS = 2, PS_NOT_FINITE = 3, PS_BEHIND = 4, PS_DUPLICATE = 5, PS_HIGH_ERROR = 6, PS_RELATIVE = 7,
  PS_LANDMARK_AT_FAULT = 8, PS_FRAME_AT_FAULT = 9, PS_COUNT = 10
};

// rule 5: the observation passed rules 3 and 4 (whatever the soft tests and the guards made of it afterwards)
PRUNE_HD bool prune_eligible(int status) { return status == PS_KEPT || (status >= PS_HIGH_ERROR && status <= PS_FRAME_AT_FAULT); }
// rule 6: still HIGH_ERROR or RELATIVE
PRUNE_HD bool prune_soft(int status) { return status == PS_HIGH_ERROR || status == PS_RELATIVE; }
// rule 9: the row is taken out of its frame
PRUNE_HD bool prune_pruned(int status) { return status >= PS_NOT_FINITE && status <= PS_RELATIVE; }

// rules 7 and 8: more than `share` per mille of the n_el eligible observations are soft.  n_soft <= n_el < 2^31 and
// share <= 1000, so both products stay below 2^41.  1000 can never fire (n_soft <= n_el), 0 fires on the first soft one.
PRUNE_HD bool prune_guard_fires(int n_soft, int n_el, int share) { return (int64_t)n_soft * 1000 > (int64_t)share * (int64_t)n_el; }

// rule 6: the rank of the lower median among n_el >= 1 values in ascending order
PRUNE_HD int prune_median_rank(int n_el) { return (n_el - 1) / 2; }

// the order of two observations of one landmark: (sq, key), and the keys of a list are distinct, so it is total on finite sq.
// a and b are list positions or keys -- a list is in ascending key, either gives the same answer.
PRUNE_HD bool prune_before(double sq_a, int a, double sq_b, int b) { return sq_a < sq_b || (sq_a == sq_b && a < b); }

// rule 4: the member of a run of n observations of one (entry, frame) that stays: the first in the order (sq, position) among
// those with ok[k] != 0 (they passed rule 3), or -1 when none passed.  The kernels decide "is some other member before me" per
// observation with prune_before; this is the same decision told from the run's side, and what the host check compares.
PRUNE_HD int prune_run_winner(const double* sq, const unsigned char* ok, int n) {
  int w = -1;
  for (int k = 0; k < n; ++k)
    if (ok[k] && (w < 0 || prune_before(sq[k], k, sq[w], w))) w = k;
  return w;
}

}  // namespace vo

#endif
