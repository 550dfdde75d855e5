// ransac.hip -- RANSAC in front of the epipolar initialisation (vo_estimate_transform_ransac[_dev]):
//   ransac_gather_kernel  checks the live pairs' indices (as epi_ata_kernel) and writes one float4 (u1, v1, u2, v2) per pair
//                         in pixels -- 16 B a pair, which the scoring pass re-reads from L2 once per hypothesis block;
//   ransac_hyp_kernel     one thread per hypothesis: the sample (splitmix64 draws, vo_hip.h), the 8 x 9 system of the
//                         normalised points formed in float as epi_ata_kernel forms its rows, its null vector by Gaussian
//                         elimination with full pivoting in double, the rank-2 projection (linalg::svd3, as
//                         fundamental_from_normal_matrix), F = T1^T F T2 scaled to unit Frobenius norm, 9 floats;
//   ransac_score_kernel   the hot path, ransac_common.h's scoring tile on EpiModel (below): every thread holds RANSAC_PTS
//                         correspondences in registers, the workgroup walks a block of 64 hypotheses whose F is wave-uniform;
//   ransac_select_kernel  one workgroup: invalid hypotheses get -1, the winner is the maximum of (count << 32) | ~h (the
//                         most inliers, ties to the lowest h);
//   ransac_mask_kernel / ransac_scatter_kernel
//                         the winner's inlier mask (the same per-pair predicate) and the inlier pairs compacted in their
//                         original order: count / scan (geom.hip's launch_scan) / scatter; the mask tail and the scatter
//                         are ransac_common.h's.
// Counts are integers: nothing here depends on scheduling.  The refit of the winner's inliers is vo_estimate_transform_dev
// itself (capi.hip).
#include "vo_internal.h"
#include "ransac_common.h"
#include "../../include/vo/linalg.hpp"

namespace vo {

constexpr int RB = 256;            // threads per workgroup (gather, scoring, mask)
constexpr int RANSAC_PTS = 4;      // correspondences per thread of the scoring pass
constexpr int RANSAC_FS = 12;      // floats per hypothesis: F row-major in [0, 9), [9] = 1 valid / 0 invalid

// Sampson distance below the threshold: e^2 < thr^2 * den, e = x1^T F x2, den = (F x2)_0^2 + (F x2)_1^2 + (F^T x1)_0^2 +
// (F^T x1)_1^2 -- d^2 = e^2 / den < thr^2 without the division; den = 0 or a NaN anywhere never passes
__device__ __forceinline__ bool sampson_inlier(const float* f, const float4 p, float thr2) {
  const float a0 = f[0] * p.z + f[1] * p.w + f[2];     // F x2
  const float a1 = f[3] * p.z + f[4] * p.w + f[5];
  const float a2 = f[6] * p.z + f[7] * p.w + f[8];
  const float b0 = f[0] * p.x + f[3] * p.y + f[6];     // F^T x1
  const float b1 = f[1] * p.x + f[4] * p.y + f[7];
  const float e = p.x * a0 + p.y * a1 + a2;
  const float den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
  return e * e < thr2 * den;
}

__global__ __launch_bounds__(RB) void ransac_gather_kernel(RansacArgs a) {
  const int n = live_rows(a.d_n, a.n_max);
  const float qnan = __int_as_float(0x7fc00000);
  int bad = 0;
  for (int i = blockIdx.x * RB + threadIdx.x; i < n; i += gridDim.x * RB) {
    const int2 pr = reinterpret_cast<const int2*>(a.pairs)[i];
    float4 o = make_float4(qnan, qnan, qnan, qnan);            // a bad pair is never an inlier (and the call is refused)
    if (pr.x < 0 || pr.x >= a.n1 || pr.y < 0 || pr.y >= a.n2) ++bad;
    else {
      const float2 q1 = reinterpret_cast<const float2*>(a.p1)[pr.x];
      const float2 q2 = reinterpret_cast<const float2*>(a.p2)[pr.y];
      o = make_float4(q1.x, q1.y, q2.x, q2.y);
    }
    a.pts[i] = o;
  }
  if (bad) atomicAdd(&a.info[1], bad);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.info[0] = n;
}

__global__ __launch_bounds__(64) void ransac_hyp_kernel(RansacArgs a) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= a.n_hyp) return;
  const int n = live_rows(a.d_n, a.n_max);
  float* out = a.F + (size_t)h * RANSAC_FS;
  int idx[8];
  int k = 0;
  if (n >= 8)
    for (unsigned j = 0; j < 64 && k < 8; ++j) {
      const int v = ransac_draw(a.seed, h, j, n);
      bool fresh = true;
      for (int q = 0; q < k; ++q) fresh &= idx[q] != v;
      if (fresh) idx[k++] = v;
    }
  bool ok = k == 8;
  double A[8][9];
  // normalize(): x / (max_x / 2.f) - 1.f in float, then double -- as epi_ata_kernel forms its rows
  const float hx1 = __uint_as_float(a.maxima[0]) / 2.f, hy1 = __uint_as_float(a.maxima[1]) / 2.f;
  const float hx2 = __uint_as_float(a.maxima[2]) / 2.f, hy2 = __uint_as_float(a.maxima[3]) / 2.f;
  double amax = 0.0;
  if (ok)
    for (int r = 0; r < 8; ++r) {
      const float4 p = a.pts[idx[r]];
      const double d1[3] = {(double)(p.x / hx1 - 1.f), (double)(p.y / hy1 - 1.f), 1.0};
      const double d2[3] = {(double)(p.z / hx2 - 1.f), (double)(p.w / hy2 - 1.f), 1.0};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          A[r][3 * i + j] = d1[i] * d2[j];
          amax = fmax(amax, fabs(A[r][3 * i + j]));
        }
    }
  // null vector: elimination with full pivoting; a relative pivot below 1e-12 (or a NaN) leaves the hypothesis invalid
  int col[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
  for (int r = 0; r < 8 && ok; ++r) {
    int pr = r, pc = r;
    double best = -1.0;
    for (int i = r; i < 8; ++i)
      for (int c = r; c < 9; ++c)
        if (fabs(A[i][c]) > best) { best = fabs(A[i][c]); pr = i; pc = c; }
    if (!(best > 1e-12 * amax)) { ok = false; break; }
    for (int c = 0; c < 9; ++c) { const double t = A[r][c]; A[r][c] = A[pr][c]; A[pr][c] = t; }
    for (int i = 0; i < 8; ++i) { const double t = A[i][r]; A[i][r] = A[i][pc]; A[i][pc] = t; }
    { const int t = col[r]; col[r] = col[pc]; col[pc] = t; }
    for (int i = r + 1; i < 8; ++i) {
      const double m = A[i][r] / A[r][r];
      for (int c = r; c < 9; ++c) A[i][c] -= m * A[r][c];
    }
  }
  float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    double x[9];
    x[8] = 1.0;
    for (int r = 7; r >= 0; --r) {
      double s = A[r][8] * x[8];
      for (int c = r + 1; c < 8; ++c) s += A[r][c] * x[c];
      x[r] = -s / A[r][r];
    }
    linalg::Mat3d Fa;
    for (int c = 0; c < 9; ++c) Fa.m[col[c] / 3][col[c] % 3] = x[c];
    linalg::Mat3d U, V;
    double s[3];
    linalg::svd3(Fa, U, s, V);
    linalg::Mat3d D = linalg::Mat3d::zero();
    D.m[0][0] = s[0]; D.m[1][1] = s[1];                                  // rank 2, as fundamental_from_normal_matrix
    const linalg::Mat3d R2 = U * D * V.transpose();
    // conditioning_matrix() in float, then F = T1^T F T2 in double
    linalg::Mat3d t1 = linalg::Mat3d::identity(), t2 = linalg::Mat3d::identity();
    t1.m[0][0] = 1.f / hx1; t1.m[0][2] = -1.f; t1.m[1][1] = 1.f / hy1; t1.m[1][2] = -1.f;
    t2.m[0][0] = 1.f / hx2; t2.m[0][2] = -1.f; t2.m[1][1] = 1.f / hy2; t2.m[1][2] = -1.f;
    const linalg::Mat3d Fd = t1.transpose() * R2 * t2;
    double nrm = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) nrm += Fd.m[i][j] * Fd.m[i][j];
    nrm = sqrt(nrm);
    ok = nrm > 0.0 && isfinite(nrm);
    if (ok)
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) F[3 * i + j] = (float)(Fd.m[i][j] / nrm);
  }
  for (int c = 0; c < 9; ++c) out[c] = F[c];
  out[9] = ok ? 1.f : 0.f;
}

// the epipolar front end as a model of ransac_common.h: a pair is (u1, v1, u2, v2), a hypothesis F with its valid flag
struct EpiModel {
  static constexpr int NT = RB, PTS = RANSAC_PTS;
  using Pair = float4;
  struct Hyp { float f[9]; };
  const RansacArgs& a;
  __device__ __forceinline__ Pair load_pair(int i) const { return a.pts[i]; }
  static __device__ __forceinline__ Pair zero_pair() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ bool valid(int h) const { return !(a.F[(size_t)h * RANSAC_FS + 9] == 0.f); }
  __device__ __forceinline__ Hyp load(int h) const {
    const float* g = a.F + (size_t)h * RANSAC_FS;
    Hyp hyp;
#pragma unroll
    for (int c = 0; c < 9; ++c) hyp.f[c] = g[c];
    return hyp;
  }
  __device__ __forceinline__ bool inlier(const Hyp& hyp, const Pair& p) const { return sampson_inlier(hyp.f, p, a.thr2); }
};

__global__ __launch_bounds__(RB) void ransac_score_kernel(RansacArgs a) {
  ransac_score_body(EpiModel{a}, blockIdx.x, blockIdx.y, live_rows(a.d_n, a.n_max), a.n_hyp, a.counts);
}

__global__ __launch_bounds__(1024) void ransac_select_kernel(RansacArgs a) {
  const unsigned long long best = ransac_select_best(a.n_hyp, a.F + 9, RANSAC_FS, a.counts);
  if (threadIdx.x == 0) {
    a.info[2] = best ? (int)(0xFFFFFFFFull - (best & 0xFFFFFFFFull)) : -1;
    a.info[3] = best ? (int)(best >> 32) : 0;
  }
}

__global__ __launch_bounds__(RB) void ransac_mask_kernel(RansacArgs a) {
  const int n = live_rows(a.d_n, a.n_max);
  const int win = a.info[2];
  const int i = blockIdx.x * RB + threadIdx.x;
  bool in = false;
  if (win >= 0 && i < n) {
    const float* g = a.F + (size_t)win * RANSAC_FS;
    float f[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) f[c] = g[c];
    in = sampson_inlier(f, a.pts[i], a.thr2);
  }
  ransac_mask_tail<RB>(in, blockIdx.x, a.n_max, a.mask, a.blk);
}

__global__ __launch_bounds__(RB) void ransac_scatter_kernel(RansacArgs a) {
  ransac_scatter_body<RB>(blockIdx.x, a.n_max, a.mask, a.blk, a.pairs, a.out_pairs);
}

static int ransac_nb(int n_max) { return (n_max + RB - 1) / RB; }

// The workspace, block by block (each 256-aligned), in this order; ws may be null (the walk then only measures)
RansacArgs ransac_layout(void* ws, int n_max, int n_hyp, size_t* bytes) {
  RansacArgs a{};
  WsCarver w(ws);
  a.info = w.take<int>(256);                                   // [0, 32) info, [32, 48) maxima
  a.maxima = WsCarver::within<unsigned>(a.info, 32);
  a.pts = w.take<float4>(16 * (size_t)n_max);
  a.F = w.take<float>(4 * RANSAC_FS * (size_t)n_hyp);
  a.counts = w.take<int>(4 * (size_t)n_hyp);
  a.mask = w.take<uint8_t>((size_t)n_max);
  a.blk = w.take<int>(4 * (size_t)ransac_nb(n_max));           // per-workgroup counts
  a.out_pairs = w.take<int32_t>(8 * (size_t)n_max);            // compacted pairs
  a.n_max = n_max; a.n_hyp = n_hyp;
  if (bytes) *bytes = w.bytes;
  return a;
}

size_t ransac_workspace_bytes(int n_max, int n_hyp) {
  size_t bytes;
  return ransac_layout(nullptr, n_max, n_hyp, &bytes), bytes;
}

hipError_t launch_ransac(hipStream_t st, const RansacArgs& a) {
  hipError_t e = hipMemsetAsync(a.info, 0, 64, st);                   // info and maxima
  if (e == hipSuccess) e = hipMemsetAsync(a.counts, 0, sizeof(int) * (size_t)a.n_hyp, st);
  if (e != hipSuccess) return e;
  e = launch_epi_maxima(st, a.p1, a.n1, a.p2, a.n2, a.maxima);
  if (e != hipSuccess) return e;
  const int nb = ransac_nb(a.n_max);
  hipLaunchKernelGGL(ransac_gather_kernel, dim3(nb < 1024 ? nb : 1024), dim3(RB), 0, st, a);
  hipLaunchKernelGGL(ransac_hyp_kernel, dim3((a.n_hyp + 63) / 64), dim3(64), 0, st, a);
  const int nsb = (a.n_max + RB * RANSAC_PTS - 1) / (RB * RANSAC_PTS);
  hipLaunchKernelGGL(ransac_score_kernel, dim3(nsb, (a.n_hyp + RANSAC_HB - 1) / RANSAC_HB), dim3(RB), 0, st, a);
  hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(ransac_mask_kernel, dim3(nb), dim3(RB), 0, st, a);
  e = launch_scan(st, a.blk, nb, &a.info[4]);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ransac_scatter_kernel, dim3(nb), dim3(RB), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
