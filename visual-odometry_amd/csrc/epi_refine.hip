// epi_refine.hip -- Gauss-Newton refit of a relative pose on the Sampson error of 2D-2D pairs (vo_refine_transform[_dev]:
// include/vo_hip.h has the definition; DESIGN.md section 4.11 the measurements).  A round is two launches:
//   epi_refine_acc_kernel    one workgroup per 256 POSITIONS of the pair array: residual, analytic Jacobian and Huber weight
//                            of every live, marked pair in double, the 15 + 5 + 1 sums and three counts reduced over the
//                            workgroup in a fixed order (lanes by butterfly, waves in wave order) into the workgroup's row;
//   epi_refine_step_kernel   one workgroup: the rows (staged through LDS) summed in workgroup order, the 5 x 5 solve (LDL^T),
//                            the pose update in device memory -- and, behind the last accumulation, the accept rule, the pose
//                            and the statistics.
// No atomics and no dependence on scheduling: a row is a function of its 256 positions, the sum a function of the rows up to
// the live count (a workgroup past it holds +0.0 and is not read), so the result does not depend on n_max.  Nothing is read
// back between rounds; a refit that has failed (status != 0 in the state) turns the launches behind it into no-ops.
#include "vo_internal.h"
#include "../../include/vo_hip.h"

namespace vo {

constexpr int RB = 256;
constexpr int STEP_ROWS = 128;     // rows the step kernel stages in LDS at a time (24 KB)
static_assert(sizeof(vo_epi_refine_stats) == 40, "the statistics are written as 6 ints and 2 doubles");

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// b1 = normalise(th x e_k), k the axis of the smallest |th_k| (the lowest on ties), b2 = th x b1
__device__ __forceinline__ void refine_basis(const double th[3], double b1[3], double b2[3]) {
  int k = 0;
  if (fabs(th[1]) < fabs(th[k])) k = 1;
  if (fabs(th[2]) < fabs(th[k])) k = 2;
  const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
  cross3(th, e, b1);
  const double n = sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
  b1[0] /= n; b1[1] /= n; b1[2] /= n;
  cross3(th, b1, b2);
}

// the pose a refit starts from: R row-major, th = t / |t|, tn = |t| in double of the float X (column-major 4x4)
__device__ __forceinline__ void refine_input_pose(const RefineArgs& a, double R[9], double th[3], double& tn) {
  float X[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) X[k] = a.d_X_in ? a.d_X_in[k] : a.X_in[k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)X[r + 4 * c];
  const double t[3] = {(double)X[12], (double)X[13], (double)X[14]};
  tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  th[0] = t[0] / tn; th[1] = t[1] / tn; th[2] = t[2] / tn;
}

// matrix p of a round, row-major: p = 0 the fundamental F = K^-T E^T K^-1 of E = [th]x R; p = 1 .. 3 its derivative along
// rotation component p - 1 (E -> [th]x [e_k]x R); p = 4, 5 along b1, b2 (E -> [b]x R)
__device__ __forceinline__ void refine_matrix(const double Kinv[9], const double R[9], const double th[3], int p, double M[9]) {
  double v[3] = {th[0], th[1], th[2]};
  if (p >= 4) {                                 // only the two translation directions need the tangent basis
    double b1[3], b2[3];
    refine_basis(th, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = p == 4 ? b1[k] : b2[k];
  }
  double E[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double col[3] = {R[c], R[3 + c], R[6 + c]};
    if (p >= 1 && p <= 3) {
      const double e[3] = {p == 1 ? 1.0 : 0.0, p == 2 ? 1.0 : 0.0, p == 3 ? 1.0 : 0.0};
      double w[3];
      cross3(e, col, w);
      col[0] = w[0]; col[1] = w[1]; col[2] = w[2];
    }
    double o[3];
    cross3(v, col, o);
    E[c] = o[0]; E[3 + c] = o[1]; E[6 + c] = o[2];
  }
  double T[9];                                  // E^T K^-1
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T[3 * r + c] = E[r] * Kinv[c] + E[3 + r] * Kinv[3 + c] + E[6 + r] * Kinv[6 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[3 * r + c] = Kinv[r] * T[c] + Kinv[3 + r] * T[3 + c] + Kinv[6 + r] * T[6 + c];
}

__global__ __launch_bounds__(RB) void epi_refine_acc_kernel(RefineArgs a, int it) {
  __shared__ double s_M[6][9];
  __shared__ double s_red[RB / 64][REFINE_ROW];
  if (it > 0 && a.st->status != 0) return;
  if (threadIdx.x < 6) {
    double R[9], th[3], tn;
    if (it == 0) {
      refine_input_pose(a, R, th, tn);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = a.st->R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) th[k] = a.st->th[k];
    }
    double M[9];
    refine_matrix(a.Kinv, R, th, (int)threadIdx.x, M);
#pragma unroll
    for (int k = 0; k < 9; ++k) s_M[threadIdx.x][k] = M[k];
  }
  __syncthreads();
  const int n = live_rows(a.d_n, a.n_max);
  double acc[REFINE_ROW];
#pragma unroll
  for (int k = 0; k < REFINE_ROW; ++k) acc[k] = 0.0;
  const int i = blockIdx.x * RB + threadIdx.x;
  if (i < n) {
    if (a.mask && !a.mask[i]) {
      acc[22] = 1.0;                                        // live but unmarked: takes no part, counted with the skipped
    } else {
      const int2 pr = reinterpret_cast<const int2*>(a.pairs)[i];
      if (pr.x < 0 || pr.x >= a.n1 || pr.y < 0 || pr.y >= a.n2) {
        acc[23] = 1.0;                                      // checked before any load, as epi_ata_kernel does
      } else {
        const float2 q1 = reinterpret_cast<const float2*>(a.p1)[pr.x];
        const float2 q2 = reinterpret_cast<const float2*>(a.p2)[pr.y];
        const double u1 = q1.x, v1 = q1.y, u2 = q2.x, v2 = q2.y;
        double fa[2], fb[2], r = 0.0, s = 1.0, J[5];
        bool ok = true;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const double* M = s_M[p];
          const double a0 = M[0] * u2 + M[1] * v2 + M[2], a1 = M[3] * u2 + M[4] * v2 + M[5], a2 = M[6] * u2 + M[7] * v2 + M[8];
          const double b0 = M[0] * u1 + M[3] * v1 + M[6], b1 = M[1] * u1 + M[4] * v1 + M[7];
          const double e = u1 * a0 + v1 * a1 + a2;
          if (p == 0) {
            const double s2 = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
            s = sqrt(s2);
            r = e / s;
            ok = s2 > 0.0 && isfinite(r);
            fa[0] = a0; fa[1] = a1; fb[0] = b0; fb[1] = b1;
          } else {
            const double ds = (fa[0] * a0 + fa[1] * a1 + fb[0] * b0 + fb[1] * b1) / s;
            J[p - 1] = (e - r * ds) / s;
          }
        }
        if (ok) {
          const double ar = fabs(r);
          const double w = (a.huber > 0.0 && ar > a.huber) ? a.huber / ar : 1.0;
          int k = 0;
#pragma unroll
          for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int q = p; q < 5; ++q) acc[k++] = w * J[p] * J[q];
#pragma unroll
          for (int p = 0; p < 5; ++p) acc[15 + p] = w * J[p] * r;
          acc[20] = w * r * r;
          acc[21] = 1.0;
        } else {
          acc[22] = 1.0;                                    // zero denominator or NaN
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < REFINE_ROW; ++k) {
    double v = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < REFINE_ROW) {
    double v = 0.0;
    for (int w = 0; w < RB / 64; ++w) v += s_red[w][threadIdx.x];
    a.partials[(size_t)blockIdx.x * REFINE_ROW + threadIdx.x] = v;
  }
}

// exp([w]x) R -> R (row-major): I + A W + B W^2, A = sin(t)/t, B = 2 sin^2(t/2)/t^2 (their series below t^2 = 1e-16)
__device__ __forceinline__ void refine_rotate(const double w[3], double R[9]) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (t2 < 1e-16) {
    A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0;
  } else {
    const double t = sqrt(t2), sh = sin(0.5 * t);
    A = sin(t) / t; B = 2.0 * sh * sh / t2;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double col[3] = {R[c], R[3 + c], R[6 + c]};
    double w1[3], w2[3];
    cross3(w, col, w1);
    cross3(w, w1, w2);
#pragma unroll
    for (int r = 0; r < 3; ++r) R[3 * r + c] = col[r] + A * w1[r] + B * w2[r];
  }
}

// H d = -g, H the 5 x 5 upper triangle row-major (15 entries), by LDL^T without pivoting; false when a pivot is not above
// 1e-12 x the largest diagonal entry of H
__device__ __forceinline__ bool refine_solve(const double h[15], const double g[5], double d[5]) {
  double H[5][5];
  int k = 0;
#pragma unroll
  for (int p = 0; p < 5; ++p)
#pragma unroll
    for (int q = p; q < 5; ++q) { H[p][q] = h[k]; H[q][p] = h[k]; ++k; }
  double big = H[0][0];
#pragma unroll
  for (int p = 1; p < 5; ++p) big = H[p][p] > big ? H[p][p] : big;
  const double lim = 1e-12 * big;
  double L[5][5], D[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double v = H[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) v -= L[j][q] * L[j][q] * D[q];
    if (!(v > lim)) return false;
    D[j] = v;
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double u = H[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) u -= L[i][q] * L[j][q] * D[q];
      L[i][j] = u / v;
    }
  }
  double y[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double v = -g[i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
    y[i] = v;
  }
#pragma unroll
  for (int i = 4; i >= 0; --i) {
    double v = y[i] / D[i];
#pragma unroll
    for (int q = i + 1; q < 5; ++q) v -= L[q][i] * d[q];
    d[i] = v;
  }
  return true;
}

__global__ __launch_bounds__(RB) void epi_refine_step_kernel(RefineArgs a, int it) {
  __shared__ double s_rows[STEP_ROWS * REFINE_ROW];
  __shared__ double s_sum[REFINE_ROW];
  RefineState* st = a.st;
  const bool last = it == a.n_rounds;
  const bool dead = it > 0 && st->status != 0;
  if (!dead) {
    // the rows in workgroup order: staged through LDS by the whole workgroup (coalesced, every load in flight at once), added
    // sequentially by one thread per column -- the order of the additions is that of the plain loop over the rows
    const int n = live_rows(a.d_n, a.n_max);
    int nb = (n + RB - 1) / RB;
    if (nb > a.grid) nb = a.grid;
    double v = 0.0;
    for (int b0 = 0; b0 < nb; b0 += STEP_ROWS) {
      const int cnt = (nb - b0 < STEP_ROWS ? nb - b0 : STEP_ROWS) * REFINE_ROW;
      const double* src = a.partials + (size_t)b0 * REFINE_ROW;
      for (int k = threadIdx.x; k < cnt; k += RB) s_rows[k] = src[k];
      __syncthreads();
      if (threadIdx.x < REFINE_ROW)
        for (int k = threadIdx.x; k < cnt; k += REFINE_ROW) v += s_rows[k];
      __syncthreads();
    }
    if (threadIdx.x < REFINE_ROW) s_sum[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!dead) {
    const double cost = s_sum[20];
    const int used = (int)s_sum[21], skipped = (int)s_sum[22], bad = (int)s_sum[23];
    double R[9], th[3], tn;
    if (it == 0) {
      refine_input_pose(a, R, th, tn);
#pragma unroll
      for (int k = 0; k < 16; ++k) st->X_in[k] = a.d_X_in ? a.d_X_in[k] : a.X_in[k];
      st->tn = tn; st->cost0 = cost; st->cost1 = cost;
      st->used0 = used; st->skipped0 = skipped; st->bad0 = bad; st->rounds = 0;
      int s = VO_EPI_REFINE_OK;
      if (bad > 0) s = VO_EPI_REFINE_BAD_INDEX;
      else if (!(tn > 0.0) || !isfinite(tn)) s = VO_EPI_REFINE_BAD_INPUT;
      else if (used < 8) s = VO_EPI_REFINE_FEW_PAIRS;
      st->status = s;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = st->R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) th[k] = st->th[k];
    }
    if (st->status == 0 && !last) {
      double h[15], g[5], d[5];
#pragma unroll
      for (int k = 0; k < 15; ++k) h[k] = s_sum[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) g[k] = s_sum[15 + k];
      if (!refine_solve(h, g, d)) {
        st->status = VO_EPI_REFINE_SINGULAR;
      } else {
        double b1[3], b2[3], t[3];
        refine_basis(th, b1, b2);
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = th[k] + d[3] * b1[k] + d[4] * b2[k];
        const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) th[k] = t[k] / n;
        refine_rotate(d, R);
        st->rounds = it + 1;
      }
    }
    if (st->status == 0 && last) {
      if (used != st->used0 || !(cost <= st->cost0)) st->status = VO_EPI_REFINE_COST_ROSE;
      else st->cost1 = cost;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) st->R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) st->th[k] = th[k];
  }
  if (!last) return;
  if (st->status == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.X_out[r + 4 * c] = (float)st->R[3 * r + c];
      a.X_out[12 + r] = (float)(st->tn * st->th[r]);
      a.X_out[3 + 4 * r] = 0.f;
    }
    a.X_out[15] = 1.f;
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) a.X_out[k] = st->X_in[k];
  }
  int* so = reinterpret_cast<int*>(a.stats);
  so[0] = st->status; so[1] = st->rounds; so[2] = st->used0; so[3] = st->skipped0; so[4] = st->bad0; so[5] = 0;
  double* sd = reinterpret_cast<double*>(so + 6);
  sd[0] = st->cost0; sd[1] = st->cost1;
}

size_t epi_refine_workspace_bytes(int n_max) {
  const size_t grid = ((size_t)(n_max > 0 ? n_max : 1) + RB - 1) / RB;
  return 512 + sizeof(double) * REFINE_ROW * grid;
}

// a.st / a.partials / a.grid are set here from ws; n_rounds + 1 accumulations, each followed by its step
hipError_t launch_epi_refine(hipStream_t st, RefineArgs a, void* ws) {
  static_assert(sizeof(RefineState) <= 512, "the state's slot of the workspace");
  a.st = static_cast<RefineState*>(ws);
  a.partials = reinterpret_cast<double*>(static_cast<char*>(ws) + 512);
  a.grid = (int)(((size_t)(a.n_max > 0 ? a.n_max : 1) + RB - 1) / RB);
  for (int it = 0; it <= a.n_rounds; ++it) {
    hipLaunchKernelGGL(epi_refine_acc_kernel, dim3(a.grid), dim3(RB), 0, st, a, it);
    hipLaunchKernelGGL(epi_refine_step_kernel, dim3(1), dim3(RB), 0, st, a, it);
  }
  return hipGetLastError();
}

}  // namespace vo
