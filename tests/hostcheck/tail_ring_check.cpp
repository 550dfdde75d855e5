// The predicate by which the closing tail launch decides that the partial rows of launch `target` still lie in the ring
// (csrc/vo_internal.h, picp_tail_ring_holds), evaluated on the host: one line "skip_from target 0|1" per query read from the
// arguments (pairs of integers), after a first line with PICP_SLOTS.  Host code only: no device is touched.
#include <stdio.h>
#include <stdlib.h>

#include "vo_internal.h"

int main(int argc, char** argv) {
  printf("%d\n", vo::PICP_SLOTS);
  for (int k = 1; k + 1 < argc; k += 2) {
    const int skip_from = atoi(argv[k]), target = atoi(argv[k + 1]);
    printf("%d %d %d\n", skip_from, target, vo::picp_tail_ring_holds(skip_from, target) ? 1 : 0);
  }
  return 0;
}
