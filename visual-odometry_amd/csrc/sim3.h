// sim3.h -- the 3x3 algebra of a similarity S = [M | t] that the pose graph (pose_graph.hip) and the loop edges (map_loops.hip)
// share, so that "M^-1 is the adjugate over the determinant" (include/vo_pose_graph.h) is one text.  Column-major, double.
#pragma once

#include <hip/hip_runtime.h>

namespace vo {

__device__ __forceinline__ double pg_det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[7] * M[5]) - M[3] * (M[1] * M[8] - M[7] * M[2]) + M[6] * (M[1] * M[5] - M[4] * M[2]);
}
__device__ __forceinline__ void pg_inv3(const double* M, double* I) {
  const double d = pg_det3(M);
  I[0] = (M[4] * M[8] - M[7] * M[5]) / d; I[3] = (M[6] * M[5] - M[3] * M[8]) / d; I[6] = (M[3] * M[7] - M[6] * M[4]) / d;
  I[1] = (M[7] * M[2] - M[1] * M[8]) / d; I[4] = (M[0] * M[8] - M[6] * M[2]) / d; I[7] = (M[6] * M[1] - M[0] * M[7]) / d;
  I[2] = (M[1] * M[5] - M[4] * M[2]) / d; I[5] = (M[3] * M[2] - M[0] * M[5]) / d; I[8] = (M[0] * M[4] - M[3] * M[1]) / d;
}
__device__ __forceinline__ void pg_mv(const double* M, const double* x, double* y) {
#pragma unroll
  for (int r = 0; r < 3; ++r) y[r] = M[r] * x[0] + M[r + 3] * x[1] + M[r + 6] * x[2];
}

}  // namespace vo
