// pose_ransac.hip -- P3P RANSAC in front of the tracking solve (vo_estimate_pose_ransac[_dev]):
//   pose_gather_kernel    checks the live pairs' indices and writes one float4 (world x, y, z, measured u) + one float
//                         (measured v) per pair;
//   pose_hyp_kernel       one thread per hypothesis, in double, register-resident: the sample (the splitmix64 draws of
//                         vo_hip.h, first 4 distinct), Grunert's P3P on the first three (one quartic, closed form + two
//                         Newton steps), every real solution with positive depths turned into R, t (triads of the two
//                         congruent triangles), the one that reprojects the 4th sample closest kept, rounded to float;
//   pose_score_kernel     the hot path, ransac_common.h's scoring tile on PoseModel (below): POSE_PTS pairs per thread in
//                         registers, a block of 64 wave-uniform poses per workgroup, Camera::projectPoint's gates and the
//                         squared reprojection error in float;
//   pose_select_kernel    one workgroup: the winner (ransac_common.h), the status code, and the pose handed on (the
//                         winner's, or the identity on a fallback);
//   pose_mask_kernel / pose_scatter_kernel
//                         the pairs handed on (the winner's inliers, or every live pair on a fallback) as a mask and
//                         compacted in their original order: count / scan (geom.hip's launch_scan) / scatter; the mask
//                         tail and the scatter are ransac_common.h's.
// The batched form (vo_estimate_pose_ransac_batch_dev) runs the same bodies with the problem as a grid dimension, every
// problem on its own info words, hypotheses, counts and per-workgroup counts: its results are the single form's bit for bit.
// No host synchronisation anywhere: the call can be captured into a graph, and the solve that follows reads the pose and
// the pair count where these kernels leave them.  Counts are integers: nothing here depends on scheduling.
#include "vo_internal.h"
#include "ransac_common.h"
#include "../../include/vo_hip.h"

namespace vo {

namespace {

constexpr int PB = 256;            // threads per workgroup (gather, scoring, mask)
constexpr int POSE_PTS = 4;        // pairs per thread of the scoring pass
constexpr int POSE_FS = 16;        // floats per hypothesis: R column-major [0, 9), t [9, 12), [12] = 1 valid / 0 invalid

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 d3(double x, double y, double z) { return D3{x, y, z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return d3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ D3 unit(D3 a) { return (1.0 / sqrt(dot(a, a))) * a; }

// the largest real root of m^3 + a m^2 + b m + c (Cardano with one real root, the trigonometric form with three)
__device__ __forceinline__ double cubic_largest_root(double a, double b, double c) {
  const double p = b - a * a / 3.0, q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c;
  const double D = q * q / 4.0 + p * p * p / 27.0;
  double y;
  if (D > 0.0) {
    const double s = sqrt(D);
    y = cbrt(-q / 2.0 + s) + cbrt(-q / 2.0 - s);
  } else {
    const double r = sqrt(-p / 3.0);
    const double c3 = r > 0.0 ? fmin(1.0, fmax(-1.0, -q / (2.0 * r * r * r))) : 0.0;
    y = 2.0 * r * cos(acos(c3) / 3.0);
  }
  return y - a / 3.0;
}

// the P3P hypothesis of one sample; every array is indexed by constants only (the solution loop is unrolled)
struct P3P {
  // inputs: world points P1..P4, unit bearings j1..j3, the 4th measurement, K in double
  D3 P1, P2, P3, P4, j1, j2, j3;
  double u4, v4;
  double K[9];
  // Grunert's quantities
  double a2, b2, c2, ca, cb, cg, amc;
  // the best solution so far
  bool have = false;
  double best_v = 0.0, best_err = 0.0;
  double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};

  // one root v of the quartic: the distances, R and t, the 4th point's reprojection; kept when closer (ties: smaller v)
  __device__ __forceinline__ void consider(double v, bool real) {
    if (!real) return;
    const double u = ((amc - 1.0) * v * v - 2.0 * amc * cb * v + 1.0 + amc) / (2.0 * (cg - v * ca));
    const double s1sq = b2 / (1.0 + v * v - 2.0 * v * cb);
    if (!(v > 0.0 && u > 0.0 && s1sq > 0.0) || !isfinite(u) || !isfinite(s1sq)) return;
    const double s1 = sqrt(s1sq);
    const D3 Q1 = s1 * j1, Q2 = (u * s1) * j2, Q3 = (v * s1) * j3;
    // R maps the world triad of (P1, P2, P3) onto the camera triad of (Q1, Q2, Q3): R = Bq Bp^T; t from the centroids
    const D3 px = unit(P2 - P1), pz = unit(cross(P2 - P1, P3 - P1)), py = cross(pz, px);
    const D3 qx = unit(Q2 - Q1), qz = unit(cross(Q2 - Q1, Q3 - Q1)), qy = cross(qz, qx);
    double Rn[9];
    Rn[0] = qx.x * px.x + qy.x * py.x + qz.x * pz.x;  Rn[3] = qx.x * px.y + qy.x * py.y + qz.x * pz.y;  Rn[6] = qx.x * px.z + qy.x * py.z + qz.x * pz.z;
    Rn[1] = qx.y * px.x + qy.y * py.x + qz.y * pz.x;  Rn[4] = qx.y * px.y + qy.y * py.y + qz.y * pz.y;  Rn[7] = qx.y * px.z + qy.y * py.z + qz.y * pz.z;
    Rn[2] = qx.z * px.x + qy.z * py.x + qz.z * pz.x;  Rn[5] = qx.z * px.y + qy.z * py.y + qz.z * pz.y;  Rn[8] = qx.z * px.z + qy.z * py.z + qz.z * pz.z;
    const D3 cp = (1.0 / 3.0) * (P1 + P2 + P3), cq = (1.0 / 3.0) * (Q1 + Q2 + Q3);
    const double tn[3] = {cq.x - (Rn[0] * cp.x + Rn[3] * cp.y + Rn[6] * cp.z), cq.y - (Rn[1] * cp.x + Rn[4] * cp.y + Rn[7] * cp.z),
                          cq.z - (Rn[2] * cp.x + Rn[5] * cp.y + Rn[8] * cp.z)};
    // the 4th sample: depth > 0 and its squared pixel error, +inf otherwise (a NaN counts as +inf)
    const double x4 = Rn[0] * P4.x + Rn[3] * P4.y + Rn[6] * P4.z + tn[0];
    const double y4 = Rn[1] * P4.x + Rn[4] * P4.y + Rn[7] * P4.z + tn[1];
    const double z4 = Rn[2] * P4.x + Rn[5] * P4.y + Rn[8] * P4.z + tn[2];
    const double hx = K[0] * x4 + K[3] * y4 + K[6] * z4, hy = K[1] * x4 + K[4] * y4 + K[7] * z4, hz = K[2] * x4 + K[5] * y4 + K[8] * z4;
    const double ex = hx / hz - u4, ey = hy / hz - v4;
    double err = ex * ex + ey * ey;
    if (!(z4 > 0.0) || !(err == err)) err = __builtin_inf();
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 9; ++c) finite &= isfinite(Rn[c]);
    finite &= isfinite(tn[0]) && isfinite(tn[1]) && isfinite(tn[2]);
    if (!finite) return;
    if (have && !(err < best_err || (err == best_err && v < best_v))) return;
    have = true; best_v = v; best_err = err;
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = Rn[c];
    t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
  }
};

__device__ __forceinline__ double quartic(double A4, double A3, double A2, double A1, double A0, double v) {
  return (((A4 * v + A3) * v + A2) * v + A1) * v + A0;
}
__device__ __forceinline__ double newton2(double A4, double A3, double A2, double A1, double A0, double v) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double d = ((4.0 * A4 * v + 3.0 * A3) * v + 2.0 * A2) * v + A1;
    if (d != 0.0) v -= quartic(A4, A3, A2, A1, A0, v) / d;
  }
  return v;
}

__device__ __forceinline__ bool pose_inlier(const CamK& cam, const Pose& T, float4 p, float pv, float thr2) {
  float u, v, pc[3], ph[3], inv;
  const bool inside = project_point(cam, T, p.x, p.y, p.z, u, v, pc, ph, inv);
  const float du = u - p.w, dv = v - pv;
  return inside && du * du + dv * dv < thr2;        // strict; a NaN never passes
}

__device__ __forceinline__ Pose load_pose(const float* g) {
  Pose T;
#pragma unroll
  for (int c = 0; c < 9; ++c) T.R[c] = g[c];
  T.t[0] = g[9]; T.t[1] = g[10]; T.t[2] = g[11];
  return T;
}

// ---- the per-problem bodies: one problem's arrays in `a`, the workgroup's place in that problem's grid in bx / by.  The
// single form calls them with its own block indices, the batched form (below) with the problem taken off the grid first.
__device__ __forceinline__ void pose_gather_body(const PoseRansacArgs& a, unsigned bx, unsigned gx) {
  const int n = live_rows(a.d_n, a.n_max);
  const float qnan = __int_as_float(0x7fc00000);
  int bad = 0;
  for (int i = bx * PB + threadIdx.x; i < n; i += gx * PB) {
    const int2 pr = reinterpret_cast<const int2*>(a.pairs)[i];
    float4 o = make_float4(qnan, qnan, qnan, qnan);            // a bad pair is never an inlier
    float ov = qnan;
    if (pr.x < 0 || pr.x >= a.n_meas || pr.y < 0 || pr.y >= a.n_world) ++bad;
    else {
      const float* w = a.world + 3 * (size_t)pr.y;
      const float2 m = reinterpret_cast<const float2*>(a.meas)[pr.x];
      o = make_float4(w[0], w[1], w[2], m.x);
      ov = m.y;
    }
    a.pts[i] = o;
    a.pv[i] = ov;
  }
  if (bad) atomicAdd(&a.info[1], bad);
  if (bx == 0 && threadIdx.x == 0) a.info[0] = n;
}

__device__ __forceinline__ void pose_hyp_body(const PoseRansacArgs a, const int h) {
  if (h >= a.n_hyp) return;
  const int n = live_rows(a.d_n, a.n_max);
  // the first 4 distinct draws, held in four registers (no array: the selects below replace the indexed stores)
  int i0 = 0, i1 = 0, i2 = 0, i3 = 0, k = 0;
  if (n >= 4)
    for (unsigned j = 0; j < 64 && k < 4; ++j) {
      const int v = ransac_draw(a.seed, h, j, n);
      if ((k < 1 || v != i0) && (k < 2 || v != i1) && (k < 3 || v != i2)) {
        i0 = k == 0 ? v : i0; i1 = k == 1 ? v : i1; i2 = k == 2 ? v : i2; i3 = k == 3 ? v : i3;
        ++k;
      }
    }
  bool ok = k == 4;
  float out[POSE_FS];
#pragma unroll
  for (int c = 0; c < POSE_FS; ++c) out[c] = 0.f;
  if (ok) {
    P3P s;
    const float4 r0 = a.pts[i0], r1 = a.pts[i1], r2 = a.pts[i2], r3 = a.pts[i3];
    const float w0 = a.pv[i0], w1 = a.pv[i1], w2 = a.pv[i2], w3 = a.pv[i3];
    s.P1 = d3(r0.x, r0.y, r0.z); s.P2 = d3(r1.x, r1.y, r1.z); s.P3 = d3(r2.x, r2.y, r2.z); s.P4 = d3(r3.x, r3.y, r3.z);
    s.u4 = r3.w; s.v4 = w3;
#pragma unroll
    for (int c = 0; c < 9; ++c) s.K[c] = a.cam.K[c];
    const double* Ki = a.Kinv;
    auto bearing = [&](double u, double v) {
      return unit(d3(Ki[0] * u + Ki[3] * v + Ki[6], Ki[1] * u + Ki[4] * v + Ki[7], Ki[2] * u + Ki[5] * v + Ki[8]));
    };
    s.j1 = bearing(r0.w, w0); s.j2 = bearing(r1.w, w1); s.j3 = bearing(r2.w, w2);
    // degenerate world triangle (collinear or repeated points): invalid
    const D3 e12 = s.P2 - s.P1, e13 = s.P3 - s.P1;
    const D3 cr = cross(e12, e13);
    ok = sqrt(dot(cr, cr)) > 1e-9 * sqrt(dot(e12, e12)) * sqrt(dot(e13, e13));
    // Grunert (Haralick et al. 1994): a, b, c the sides opposite P1, P2, P3; alpha, beta, gamma the angles between the
    // bearings (2,3), (1,3), (1,2); s2 = u s1, s3 = v s1 and one quartic in v
    s.a2 = dot(s.P2 - s.P3, s.P2 - s.P3); s.b2 = dot(e13, e13); s.c2 = dot(e12, e12);
    s.ca = dot(s.j2, s.j3); s.cb = dot(s.j1, s.j3); s.cg = dot(s.j1, s.j2);
    const double a2 = s.a2, b2 = s.b2, c2 = s.c2, ca = s.ca, cb = s.cb, cg = s.cg;
    const double amc = (a2 - c2) / b2, apc = (a2 + c2) / b2;
    s.amc = amc;
    const double A4 = (amc - 1.0) * (amc - 1.0) - 4.0 * c2 / b2 * ca * ca;
    const double A3 = 4.0 * (amc * (1.0 - amc) * cb - (1.0 - apc) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb);
    const double A2 = 2.0 * (amc * amc - 1.0 + 2.0 * amc * amc * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca -
                             4.0 * apc * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg);
    const double A1 = 4.0 * (-amc * (1.0 + amc) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - apc) * ca * cg);
    const double A0 = (1.0 + amc) * (1.0 + amc) - 4.0 * a2 / b2 * cg * cg;
    ok = ok && A4 != 0.0 && isfinite(A4) && isfinite(A3) && isfinite(A2) && isfinite(A1) && isfinite(A0);
    if (ok) {
      // Ferrari: monic, depressed (x = y - B/4), the resolvent cubic's largest root m, then two quadratics
      const double B = A3 / A4, C = A2 / A4, D = A1 / A4, E = A0 / A4;
      const double p = C - 3.0 * B * B / 8.0;
      const double q = D - B * C / 2.0 + B * B * B / 8.0;
      const double r = E - B * D / 4.0 + B * B * C / 16.0 - 3.0 * B * B * B * B / 256.0;
      const double m = cubic_largest_root(p, p * p / 4.0 - r, -q * q / 8.0);
      double y[4];
      bool real[4];
      if (m > 0.0) {
        const double sm = sqrt(2.0 * m);
#pragma unroll
        for (int s1 = 0; s1 < 2; ++s1) {
          const double sg = s1 ? -1.0 : 1.0;
          const double rad = -(2.0 * p + 2.0 * m + sg * 2.0 * q / sm);
          const double sr = sqrt(fmax(rad, 0.0));
          y[2 * s1] = (sg * sm + sr) / 2.0; y[2 * s1 + 1] = (sg * sm - sr) / 2.0;
          real[2 * s1] = real[2 * s1 + 1] = rad >= 0.0;
        }
      } else {                                           // q = 0: biquadratic, y^2 = (-p +- sqrt(p^2 - 4r)) / 2
        const double disc = p * p - 4.0 * r;
        const double sd = sqrt(fmax(disc, 0.0));
#pragma unroll
        for (int s1 = 0; s1 < 2; ++s1) {
          const double w = (-p + (s1 ? -sd : sd)) / 2.0;
          const double sw = sqrt(fmax(w, 0.0));
          y[2 * s1] = sw; y[2 * s1 + 1] = -sw;
          real[2 * s1] = real[2 * s1 + 1] = disc >= 0.0 && w >= 0.0;
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) s.consider(newton2(A4, A3, A2, A1, A0, y[c] - B / 4.0), real[c]);
      ok = s.have;
    }
    if (ok) {
#pragma unroll
      for (int c = 0; c < 9; ++c) out[c] = (float)s.R[c];
      out[9] = (float)s.t[0]; out[10] = (float)s.t[1]; out[11] = (float)s.t[2];
      out[12] = 1.f;
    }
  }
  float4* dst = reinterpret_cast<float4*>(a.poses + (size_t)h * POSE_FS);
  dst[0] = make_float4(out[0], out[1], out[2], out[3]);
  dst[1] = make_float4(out[4], out[5], out[6], out[7]);
  dst[2] = make_float4(out[8], out[9], out[10], out[11]);
  dst[3] = make_float4(out[12], out[13], out[14], out[15]);
}

// the P3P front end as a model of ransac_common.h: a pair is (world x, y, z, measured u) + measured v, a hypothesis a pose
// behind its valid flag
struct PoseModel {
  static constexpr int NT = PB, PTS = POSE_PTS;
  struct Pair { float4 p; float v; };
  using Hyp = Pose;
  const PoseRansacArgs& a;
  __device__ __forceinline__ Pair load_pair(int i) const { return Pair{a.pts[i], a.pv[i]}; }
  static __device__ __forceinline__ Pair zero_pair() { return Pair{make_float4(0.f, 0.f, 0.f, 0.f), 0.f}; }
  __device__ __forceinline__ bool valid(int h) const { return !(a.poses[(size_t)h * POSE_FS + 12] == 0.f); }
  __device__ __forceinline__ Hyp load(int h) const { return load_pose(a.poses + (size_t)h * POSE_FS); }
  __device__ __forceinline__ bool inlier(const Hyp& T, const Pair& p) const { return pose_inlier(a.cam, T, p.p, p.v, a.thr2); }
};

__device__ __forceinline__ void pose_score_body(const PoseRansacArgs& a, unsigned bx, unsigned by) {
  ransac_score_body(PoseModel{a}, bx, by, live_rows(a.d_n, a.n_max), a.n_hyp, a.counts);
}

__device__ __forceinline__ void pose_select_body(const PoseRansacArgs a) {
  const unsigned long long best = ransac_select_best(a.n_hyp, a.poses + 12, POSE_FS, a.counts);
  if (threadIdx.x == 0) {
    const int win = best ? (int)(0xFFFFFFFFull - (best & 0xFFFFFFFFull)) : -1;
    const int cnt = best ? (int)(best >> 32) : 0;
    const int n = live_rows(a.d_n, a.n_max);
    const int st = a.info[1] > 0 ? VO_POSE_RANSAC_BAD_INDEX : n < 4 ? VO_POSE_RANSAC_FEW_PAIRS
                 : win < 0 ? VO_POSE_RANSAC_NO_HYPOTHESIS : cnt < 6 ? VO_POSE_RANSAC_FEW_INLIERS : VO_POSE_RANSAC_OK;
    a.info[2] = win; a.info[3] = cnt; a.info[4] = st;
    if (a.status) *a.status = st;
    Pose T;
#pragma unroll
    for (int c = 0; c < 9; ++c) T.R[c] = (c % 4 == 0) ? 1.f : 0.f;
    T.t[0] = T.t[1] = T.t[2] = 0.f;
    if (st == VO_POSE_RANSAC_OK) T = load_pose(a.poses + (size_t)win * POSE_FS);
    float T16[16];
    pose_to_T16(T, T16);
#pragma unroll
    for (int c = 0; c < 16; ++c) a.T_out[c] = T16[c];         // 4-byte stores: any float-aligned d_T16_out
  }
}

__device__ __forceinline__ void pose_mask_body(const PoseRansacArgs& a, unsigned bx) {
  const int n = live_rows(a.d_n, a.n_max);
  const int st = a.info[4], win = a.info[2];
  const int i = bx * PB + threadIdx.x;
  bool in = false;
  if (i < n) {
    if (st != VO_POSE_RANSAC_OK) in = true;                      // fallback: every live pair, as the plain frame
    else in = pose_inlier(a.cam, load_pose(a.poses + (size_t)win * POSE_FS), a.pts[i], a.pv[i], a.thr2);
  }
  ransac_mask_tail<PB>(in, bx, a.n_max, a.mask, a.blk);
}

__device__ __forceinline__ void pose_scatter_body(const PoseRansacArgs& a, unsigned bx) {
  ransac_scatter_body<PB>(bx, a.n_max, a.mask, a.blk, a.pairs, a.out_pairs);
}

// problem p of a batched call: problem 0's arrays moved on by p strides (elements, as vo_picp_solve_batch_dev counts them)
__device__ __forceinline__ PoseRansacArgs pose_problem(const PoseRansacBatchArgs& b, int p) {
  PoseRansacArgs a = b.a;
  const size_t n = (size_t)a.n_max, H = (size_t)a.n_hyp;
  a.pairs += 2 * p * b.pairs_stride;
  if (a.d_n) a.d_n += p;
  a.world += 3 * p * b.world_stride;
  a.meas += 2 * p * b.meas_stride;
  a.info += 8 * p;
  a.pts += p * n;
  a.pv += p * n;
  a.poses += p * H * POSE_FS;
  a.counts += p * H;
  a.mask += p * n;
  a.blk += p * (size_t)b.nb;
  a.out_pairs += 2 * p * b.pairs_stride;
  a.n_out += p;
  a.T_out += 16 * p;
  a.status += p;
  return a;
}

}  // namespace

// ---- the single form -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void pose_gather_kernel(PoseRansacArgs a) {
  pose_gather_body(a, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64) void pose_hyp_kernel(PoseRansacArgs a) { pose_hyp_body(a, blockIdx.x * 64 + threadIdx.x); }

__global__ __launch_bounds__(PB) void pose_score_kernel(PoseRansacArgs a) {
  pose_score_body(a, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(1024) void pose_select_kernel(PoseRansacArgs a) { pose_select_body(a); }

__global__ __launch_bounds__(PB) void pose_mask_kernel(PoseRansacArgs a) {
  pose_mask_body(a, blockIdx.x);
}

__global__ __launch_bounds__(PB) void pose_scatter_kernel(PoseRansacArgs a) { pose_scatter_body(a, blockIdx.x); }

// ---- the batched form: the problem is the last grid dimension, every kernel runs the single form's body on that problem's
// arrays.  A workgroup of the scoring, mask and scatter grids that lies wholly beyond its problem's live pairs returns at
// once (the grids are sized by the capacity): it would add nothing to a count, and the mask bytes and the per-workgroup
// count it leaves alone were zeroed by the launch.
__global__ __launch_bounds__(PB) void pose_gather_batch_kernel(PoseRansacBatchArgs b) {
  const PoseRansacArgs a = pose_problem(b, blockIdx.y);
  pose_gather_body(a, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64) void pose_hyp_batch_kernel(PoseRansacBatchArgs b) {
  pose_hyp_body(pose_problem(b, blockIdx.y), blockIdx.x * 64 + threadIdx.x);
}

__global__ __launch_bounds__(PB) void pose_score_batch_kernel(PoseRansacBatchArgs b) {
  const PoseRansacArgs a = pose_problem(b, blockIdx.z);
  if ((int)blockIdx.x * (PB * POSE_PTS) >= live_rows(a.d_n, a.n_max)) return;
  pose_score_body(a, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(1024) void pose_select_batch_kernel(PoseRansacBatchArgs b) { pose_select_body(pose_problem(b, blockIdx.x)); }

__global__ __launch_bounds__(PB) void pose_mask_batch_kernel(PoseRansacBatchArgs b) {
  const PoseRansacArgs a = pose_problem(b, blockIdx.y);
  if ((int)blockIdx.x * PB >= live_rows(a.d_n, a.n_max)) return;
  pose_mask_body(a, blockIdx.x);
}

__global__ __launch_bounds__(PB) void pose_scatter_batch_kernel(PoseRansacBatchArgs b) {
  const PoseRansacArgs a = pose_problem(b, blockIdx.y);
  if ((int)blockIdx.x * PB >= live_rows(a.d_n, a.n_max)) return;
  pose_scatter_body(a, blockIdx.x);
}

static int pose_nb(int n_max) { return (n_max + PB - 1) / PB; }

// The workspace, block by block (each 256-aligned), in this order; ws may be null (the walk then only measures)
PoseRansacArgs pose_ransac_layout(void* ws, int n_max, int n_hyp, size_t* bytes) {
  PoseRansacArgs a{};
  WsCarver w(ws);
  a.info = w.take<int>(256);                                   // ints [0, 8) info, int [8] default pair count,
  a.n_out = WsCarver::within<int>(a.info, 32);                 // floats [16, 32) default pose
  a.T_out = WsCarver::within<float>(a.info, 64);
  a.pts = w.take<float4>(16 * (size_t)n_max);
  a.pv = w.take<float>(4 * (size_t)n_max);
  a.poses = w.take<float>(4 * POSE_FS * (size_t)n_hyp);
  a.counts = w.take<int>(4 * (size_t)n_hyp);
  a.mask = w.take<uint8_t>((size_t)n_max);
  a.blk = w.take<int>(4 * (size_t)pose_nb(n_max));             // per-workgroup counts
  a.out_pairs = w.take<int32_t>(8 * (size_t)n_max);            // default compacted pairs
  a.n_max = n_max; a.n_hyp = n_hyp;
  if (bytes) *bytes = w.bytes;
  return a;
}

size_t pose_ransac_workspace_bytes(int n_max, int n_hyp) {
  size_t bytes;
  return pose_ransac_layout(nullptr, n_max, n_hyp, &bytes), bytes;
}

hipError_t launch_pose_ransac(hipStream_t st, const PoseRansacArgs& a) {
  hipError_t e = hipMemsetAsync(a.info, 0, 32, st);
  if (e == hipSuccess) e = hipMemsetAsync(a.counts, 0, sizeof(int) * (size_t)a.n_hyp, st);
  if (e != hipSuccess) return e;
  const int nb = pose_nb(a.n_max);
  hipLaunchKernelGGL(pose_gather_kernel, dim3(nb < 1024 ? nb : 1024), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(pose_hyp_kernel, dim3((a.n_hyp + 63) / 64), dim3(64), 0, st, a);
  const int nsb = (a.n_max + PB * POSE_PTS - 1) / (PB * POSE_PTS);
  hipLaunchKernelGGL(pose_score_kernel, dim3(nsb, (a.n_hyp + RANSAC_HB - 1) / RANSAC_HB), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(pose_select_kernel, dim3(1), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(pose_mask_kernel, dim3(nb), dim3(PB), 0, st, a);
  e = launch_scan(st, a.blk, nb, a.n_out);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pose_scatter_kernel, dim3(nb), dim3(PB), 0, st, a);
  return hipGetLastError();
}

// The batched form's workspace (P problems of capacity n_max, H hypotheses, nb = ceil(n_max / 256)): the single form's blocks
// times P, without its default outputs (those go to the caller's arrays).  The first three blocks are zeroed by every call, as
// one range.
PoseRansacBatchArgs pose_ransac_batch_layout(void* ws, int n_problems, int n_max, int n_hyp, size_t* bytes) {
  PoseRansacBatchArgs b{};
  const size_t P = (size_t)n_problems, n = (size_t)n_max, H = (size_t)n_hyp;
  WsCarver w(ws);
  b.a.info = w.take<int>(32 * P);                              // [P][8]
  b.a.blk = w.take<int>(4 * P * (size_t)pose_nb(n_max));       // [P][nb]
  b.a.counts = w.take<int>(4 * P * H);                         // [P][H]
  b.a.pts = w.take<float4>(16 * P * n);
  b.a.pv = w.take<float>(4 * P * n);
  b.a.poses = w.take<float>(4 * POSE_FS * P * H);
  b.a.mask = w.take<uint8_t>(P * n);
  b.a.n_max = n_max; b.a.n_hyp = n_hyp;
  b.nb = pose_nb(n_max); b.n_problems = n_problems;
  if (bytes) *bytes = w.bytes;
  return b;
}

size_t pose_ransac_batch_workspace_bytes(int n_problems, int n_max, int n_hyp) {
  size_t bytes;
  return pose_ransac_batch_layout(nullptr, n_problems, n_max, n_hyp, &bytes), bytes;
}

// 3 memsets at the most and 7 launches, whatever the number of problems
hipError_t launch_pose_ransac_batch(hipStream_t st, const PoseRansacBatchArgs& b) {
  const PoseRansacArgs& a = b.a;
  const size_t P = (size_t)b.n_problems, H = (size_t)a.n_hyp;
  // info and the per-workgroup counts, and the hypothesis counts with them while they are the workspace's own: the layout
  // walked again from its first block says where those lie
  const char* own = reinterpret_cast<const char*>(pose_ransac_batch_layout(a.info, b.n_problems, a.n_max, a.n_hyp).a.counts);
  const bool own_counts = reinterpret_cast<const char*>(a.counts) == own;
  const char* zero_end = own + (own_counts ? 4 * P * H : 0);
  hipError_t e = hipMemsetAsync(a.info, 0, (size_t)(zero_end - reinterpret_cast<const char*>(a.info)), st);
  if (e == hipSuccess && !own_counts) e = hipMemsetAsync(a.counts, 0, 4 * P * H, st);
  if (e == hipSuccess) e = hipMemsetAsync(a.mask, 0, P * (size_t)a.n_max, st);
  if (e != hipSuccess) return e;
  const unsigned np = (unsigned)b.n_problems;
  hipLaunchKernelGGL(pose_gather_batch_kernel, dim3(b.nb < 1024 ? b.nb : 1024, np), dim3(PB), 0, st, b);
  hipLaunchKernelGGL(pose_hyp_batch_kernel, dim3((a.n_hyp + 63) / 64, np), dim3(64), 0, st, b);
  const int nsb = (a.n_max + PB * POSE_PTS - 1) / (PB * POSE_PTS);
  hipLaunchKernelGGL(pose_score_batch_kernel, dim3(nsb, (a.n_hyp + RANSAC_HB - 1) / RANSAC_HB, np), dim3(PB), 0, st, b);
  hipLaunchKernelGGL(pose_select_batch_kernel, dim3(np), dim3(1024), 0, st, b);
  hipLaunchKernelGGL(pose_mask_batch_kernel, dim3(b.nb, np), dim3(PB), 0, st, b);
  e = launch_scan(st, a.blk, b.nb, a.n_out, nullptr, b.n_problems, (size_t)b.nb);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pose_scatter_batch_kernel, dim3(b.nb, np), dim3(PB), 0, st, b);
  return hipGetLastError();
}

}  // namespace vo
