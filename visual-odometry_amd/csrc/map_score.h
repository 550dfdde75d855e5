// map_score.h -- a landmark judged from its ordered observation list: the statistics and the four tests of include/vo_map_cull.h,
// as ONE device function for map_cull.hip (cull_score_kernel) and map_grow.hip (grow_track_kernel).  The rules are the header's;
// the operations and their order are what cull_score_kernel has always done, so that a point scored by both gives the same bytes
// (-ffp-contract=off: nothing here is fused or re-associated by the compiler).  The poses come through `load_pose(f, Rt)`: the
// cull reads them through L2 (MapView::load_pose), the grow kernel from the copy its workgroup staged in LDS -- the same floats.
#pragma once
#include "vo_internal.h"

namespace vo {

enum { CV_KEPT = 0, CV_UNSEEN = 1, CV_FEW_OBS = 2, CV_FEW_FRAMES = 3, CV_NOT_FINITE = 4, CV_BEHIND = 5, CV_HIGH_ERROR = 6, CV_LOW_PARALLAX = 7 };

__device__ __forceinline__ int score_ror1(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x121, 0xf, 0xf, false); }

// One observation of the landmark p by map_obs (no Huber weight: rho is |e|^2): |e|^2, camera z, and the unit ray u = d / |d|,
// d = R^T p_cam.
template <class PoseLoad>
__device__ __forceinline__ void score_obs(const MapView& v, PoseLoad load_pose, const double K[9], const double p[3], int key, double& sq, double& z,
                                          double u[3]) {
  float2 m;
  const int f = v.decode(key, m);
  float Rt[12];
  load_pose(f, Rt);
  MapObs o;
  map_obs(K, Rt, p, (double)m.x, (double)m.y, 0.0, o);
  sq = o.rho;
  z = o.pc[2];
  double d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = __builtin_fma((double)Rt[2 + 3 * c], o.pc[2], __builtin_fma((double)Rt[1 + 3 * c], o.pc[1], (double)Rt[3 * c] * o.pc[0]));
  const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  u[0] = d[0] / nrm; u[1] = d[1] / nrm; u[2] = d[2] / nrm;                 // (|d| == 0: NaN, which pass 1 reports)
}

struct MapScore {
  double sum, mx, mz, cmin;             // the sum of |e|^2, its maximum, the smallest camera z, the smallest u_k . u_l (2 with no pair visited)
  int n_fr;                             // the changes of key / n_max along the list
  bool any_bad;                         // a term is not finite
};

// The list keys[0 .. n) of the landmark at p, by the 16 lanes of one DPP row (lg: this lane's place in it).  Called by whole rows
// with n, p and `parallax` the same in the 16 lanes; every lane returns the same bits.  Pass 1 strides the list over the lanes
// (observation k in lane k mod 16): the sum by the fixed tree of refine_row_sum, the extrema and the frame changes by the same
// four row steps.  Pass 2 (only with the parallax test on) visits the pairs in tiles of 16 x 16: tile B's rays and their list
// positions go round the row (row_ror:1, 16 steps), every lane keeps the minimum of its dot products.
template <class PoseLoad>
__device__ __forceinline__ MapScore score_list(const MapView& v, PoseLoad load_pose, const double K[9], const double p[3], const int* keys, int n,
                                               bool parallax, int lg) {
  constexpr int CG = MAP_ROW;
  const int n_max = v.n_max;
  // ---- pass 1: the sums, the extrema, the frame changes ----
  double sum = 0.0, mx = 0.0, mz = 1.7976931348623157e308, changes = 0.0;
  bool bad = false;
  for (int j = lg; j < n; j += CG) {
    const int key = keys[j];
    const int prev = j > 0 ? keys[j - 1] / n_max : -1;
    double sq, z, u[3];
    score_obs(v, load_pose, K, p, key, sq, z, u);
    sum += sq;
    mx = fmax(mx, sq);
    mz = fmin(mz, z);
    changes += (key / n_max != prev) ? 1.0 : 0.0;
    bad |= !(refine_finite(sq) && refine_finite(z) && refine_finite(u[0]) && refine_finite(u[1]) && refine_finite(u[2]));
  }
  MapScore s;
  s.sum = refine_row_sum(sum);
  s.mx = refine_row_max(mx);
  s.mz = refine_row_min(mz);
  s.n_fr = (int)refine_row_sum(changes);                     // (whole numbers below 2^31: exact)
  s.any_bad = refine_row_any(bad);
  // ---- pass 2: the smallest u_k . u_l over the pairs ----
  double cmin = 2.0;
  if (parallax && n >= 2) {                                  // (the same in the 16 lanes of a row: the row's DPP moves see all of them)
    const int tiles = (n + CG - 1) / CG;
    for (int ta = 0; ta < tiles; ++ta) {
      const int ka = ta * CG + lg;
      double ua[3] = {0.0, 0.0, 0.0}, sq, z;
      if (ka < n) score_obs(v, load_pose, K, p, keys[ka], sq, z, ua);
      for (int tb = ta; tb < tiles; ++tb) {
        const int kb = tb * CG + lg;
        double ub[3] = {ua[0], ua[1], ua[2]};
        if (tb != ta && kb < n) score_obs(v, load_pose, K, p, keys[kb], sq, z, ub);
        int ib = kb < n ? kb : -1;                           // the list position that travels with the ray
#pragma unroll
        for (int t = 0; t < CG; ++t) {
          if (ka < n && ib >= 0 && ib != ka) cmin = fmin(cmin, ua[0] * ub[0] + ua[1] * ub[1] + ua[2] * ub[2]);
          ub[0] = refine_dpp<0x121>(ub[0]); ub[1] = refine_dpp<0x121>(ub[1]); ub[2] = refine_dpp<0x121>(ub[2]);
          ib = score_ror1(ib);
        }
      }
    }
  }
  s.cmin = refine_row_min(cmin);
  return s;
}

// the thresholds of the four tests as the kernels carry them: squares (0: off), the cosine, whether the parallax test is on
struct MapScoreThr { double max_mean_sq, max_sq, cos_thr; int parallax; };

// the statistics as recorded (n >= 1) and the first of NOT_FINITE, BEHIND, HIGH_ERROR, LOW_PARALLAX that matches, or CV_KEPT
__device__ __forceinline__ int score_judge(const MapScore& s, int n, const MapScoreThr& t, double& mean, double& cosp) {
  cosp = (t.parallax && n >= 2) ? s.cmin : 1.0;
  mean = n > 0 ? s.sum / (double)n : 0.0;
  if (s.any_bad) return CV_NOT_FINITE;
  if (!(s.mz > 0.0)) return CV_BEHIND;
  if ((t.max_mean_sq > 0.0 && mean > t.max_mean_sq) || (t.max_sq > 0.0 && s.mx > t.max_sq)) return CV_HIGH_ERROR;
  if (t.parallax && cosp > t.cos_thr) return CV_LOW_PARALLAX;
  return CV_KEPT;
}

}  // namespace vo
