// map_bundle.hip -- joint adjustment of a window's poses and the map's points (vox_map_bundle*): Levenberg-Marquardt rounds
// whose reduced camera system S = U - W V^-1 W^T is never formed; S p is one pass over the landmarks' ordered observation
// lists (map_refine.hip builds them) and one pass over the frames' rows, and preconditioned conjugate gradients runs on those
// two passes.  The rules are those of include/vo_map_bundle.h.  Everything is double, every sum has a fixed order, nothing is
// read back, and no launch waits for another workgroup: a round is a fixed sequence of 3 (n_cg + 2) launches,
//   bundle_point_kernel<LIN>    16 lanes per landmark: V_j, g_j, the damped V_j^-1
//   bundle_frame_lin_kernel     one workgroup per frame: U_f, g_f, then D_f and r_f (which need V^-1)
//   bundle_cg_init_kernel       one workgroup: x = 0, z = D^-1 r, p = z, r.z, |r_0|^2
//   n_cg times  bundle_point_kernel<PASS_A>  t_j = V_j^-1 sum W^T p_f
//               bundle_frame_sp_kernel       (S p)_f = U_f p_f - sum W t_j and p_f . (S p)_f
//               bundle_cg_update_kernel      one workgroup: alpha, x, r, z, beta, p, the stop flag
//   bundle_point_kernel<BACK>   the candidate points
//   bundle_cost_kernel<CAND>    one workgroup per frame: the candidate pose, its cost and z flag
//   bundle_decide_kernel        one workgroup: the accept rule, lambda, the round's record, the copy
// The three one-workgroup launches and the end's verdict run lm_pcg.h's driver, which pose_graph.hip shares: the control block,
// the ordered sums over the frames, PCG's vector side, the accept rule and lambda.  A PCG that has stopped leaves `stop` set in
// the control block; its remaining launches read it and return at once.
// The frame-side reduction is map_pose_refine.hip's (frame_reduce, vo_internal.h): DPP inside every row of 16 lanes, the 16 row
// sums through LDS, one thread per term adds them in row order.  A single frame runs on one compute unit.  An observation is
// vo_math.h's map_obs with the Jacobian tail a kernel needs (map_obs_pose_jac: Jc, 2 x 6; map_obs_point_jac: Jp, 2 x 3) and the
// normal-equation sums of accum_normal<3> / accum_normal<6> -- the one model of the four adjustment files.
#include "vo_internal.h"
#include "../../include/vo_map_bundle.h"

namespace vo {

constexpr int BB = 256;                   // threads per workgroup
constexpr int BROWS = BB / 16;            // DPP rows per workgroup
constexpr int BG = 16;                    // lanes per landmark
static_assert(BB == MAP_WG && BG == MAP_ROW, "the shared helpers of vo_internal.h count on both sizes");
constexpr int BLPB = BB / BG;             // landmarks per workgroup and trip
constexpr int BDEC = 1024;                // threads of the deciding workgroups (the first 256 take part in the sums)
constexpr int BTERMS = 27;                // most sums a frame reduces at once

enum { BS_OK = 0, BS_FIXED = 1, BS_UNSEEN = 1, BS_FEW_OBS = 2 };
enum { B_LIN = 0, B_PASS_A = 1, B_BACK = 2 };
enum { B_START = 0, B_CAND = 1, B_FINAL = 2 };

static_assert(sizeof(vox_map_bundle_params) == 28 && sizeof(vox_map_bundle_round) == 40 && sizeof(vox_map_bundle_stats) == 48,
              "the deciding kernels write these records field by field");

__device__ __forceinline__ bool bundle_free_point(const MapBundleArgs& a, int e, int M) { return e >= 0 && e < M && a.l.cur[e] >= a.min_obs_point; }

template <int N>
__device__ __forceinline__ void bundle_load(const double* src, double (&dst)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) dst[k] = src[k];
}

// y = A x for the symmetric 3x3 A given by its upper triangle ((0,0),(0,1),(0,2),(1,1),(1,2),(2,2))
__device__ __forceinline__ void sym3_mul(const double A[6], const double x[3], double y[3]) {
  y[0] = A[0] * x[0] + A[1] * x[1] + A[2] * x[2];
  y[1] = A[1] * x[0] + A[3] * x[1] + A[4] * x[2];
  y[2] = A[2] * x[0] + A[4] * x[1] + A[5] * x[2];
}
// index of (r, c), r <= c, in the upper triangle of a 6x6 stored row by row
__device__ __forceinline__ constexpr int tri6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// ---- the start: statuses, the state in double, the census ------------------------------------------------------------
__global__ __launch_bounds__(BB) void bundle_init_frames_kernel(MapBundleArgs a) {
  __shared__ int s_n;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = a.v.size();
  const int32_t* ent = a.l.ent + (size_t)f * a.v.n_max;
  if (tid == 0) s_n = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < a.v.n_max; i += BB) { const int e = ent[i]; mine += e >= 0 && e < M; }
  if (mine) atomicAdd(&s_n, mine);                           // (an integer count does not depend on the order)
  __syncthreads();
  if (tid < 12) {
    const double v = (double)a.v.pose_at(f, tid);
    a.w.T[12 * (size_t)f + tid] = v;
    a.w.Tc[12 * (size_t)f + tid] = v;
  }
  if (tid < 6) a.w.x[6 * (size_t)f + tid] = 0.0;
  if (tid == 0) {
    const int n = s_n;
    a.w.n_obs[f] = n;
    a.w.pose_status[f] = (a.fixed && a.fixed[f] != 0) ? BS_FIXED : n < a.min_obs_pose ? BS_FEW_OBS : BS_OK;
  }
}

__global__ __launch_bounds__(BB) void bundle_init_points_kernel(MapBundleArgs a) {
  const int M = a.v.size();
  const int e = blockIdx.x * BB + threadIdx.x;
  if (e >= M) return;
  const int n = a.l.cur[e];
  a.w.point_status[e] = n == 0 ? BS_UNSEEN : n < a.min_obs_point ? BS_FEW_OBS : BS_OK;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = (double)a.v.pts[3 * (size_t)e + k];
    a.w.P[3 * (size_t)e + k] = v;
    a.w.Pc[3 * (size_t)e + k] = v;
  }
}

__global__ __launch_bounds__(BB) void bundle_census_kernel(MapBundleArgs a) {
  __shared__ int s_n[3];
  const int M = a.v.size();
  if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
  __syncthreads();
  int ff = 0, fp = 0, no = 0;
  for (int f = threadIdx.x; f < a.v.n_frames; f += BB) { ff += a.w.pose_status[f] == BS_OK; no += a.w.n_obs[f]; }
  for (int e = threadIdx.x; e < M; e += BB) fp += a.w.point_status[e] == BS_OK;
  if (ff) atomicAdd(&s_n[0], ff);
  if (fp) atomicAdd(&s_n[1], fp);
  if (no) atomicAdd(&s_n[2], no);
  __syncthreads();
  if (threadIdx.x == 0) {
    MapBundleCtl c{};
    c.lambda = a.lambda0;
    c.n_free_frames = s_n[0]; c.n_free_points = s_n[1]; c.n_obs = s_n[2];
    *a.w.ctl = c;
  }
}

// ---- the total cost: one workgroup per frame ---------------------------------------------------------------------------
// START: at the state.  CAND: the candidate pose v2t(x_f) T_f is formed first (every thread the same bits, thread 0 stores it),
// the points are the candidate's.  FINAL: at the rounded state, which the rounding launch left in the candidate arrays.
template <int MODE>
__global__ __launch_bounds__(BB) void bundle_cost_kernel(MapBundleArgs a) {
  __shared__ double s_row[BROWS][BTERMS], s_tot[BTERMS];
  const MapBundleCtl& c = *a.w.ctl;
  if (MODE != B_START && c.dead) return;
  if (MODE == B_CAND && (c.bad || c.nostep)) return;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = a.v.size();
  double T[12], K[9];
  bundle_load((MODE == B_FINAL ? a.w.Tc : a.w.T) + 12 * (size_t)f, T);
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  if (MODE == B_CAND) {
    if (a.w.pose_status[f] == BS_OK) {
      double x[6];
      bundle_load(a.w.x + 6 * (size_t)f, x);
      pose_apply_v2t(x, T);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) if (tid == k) a.w.Tc[12 * (size_t)f + k] = T[k];
  }
  const double* P = MODE == B_START ? a.w.P : a.w.Pc;
  const int32_t* ent = a.l.ent + (size_t)f * a.v.n_max;
  const float2* uv = reinterpret_cast<const float2*>(a.v.uv) + (size_t)f * a.v.uv_stride;
  double acc[2] = {0.0, 0.0};                                // the cost; the count of rows whose camera z is not > 0
  for (int i = tid; i < a.v.n_max; i += BB) {
    const int e = ent[i];
    if (e < 0 || e >= M) continue;
    double p[3];
    bundle_load(P + 3 * (size_t)e, p);
    const float2 m = uv[i];
    MapObs o;
    map_obs(K, T, p, (double)m.x, (double)m.y, a.huber, o);
    acc[0] += o.rho;
    acc[1] += o.front() ? 0.0 : 1.0;
  }
  frame_reduce(acc, s_row, s_tot);
  if (tid == 0) { a.w.fcost[f] = acc[0]; a.w.fflag[f] = acc[1] != 0.0; }
}

// the start's verdict: the total cost of the start in the fixed order, NOT_FINITE / BEHIND / NOTHING_FREE
__global__ __launch_bounds__(BB) void bundle_start_kernel(MapBundleArgs a) {
  __shared__ double s_sum[256];
  __shared__ int s_flag;
  if (threadIdx.x == 0) s_flag = 0;
  __syncthreads();
  double mine = 0.0;
  int fl = 0;
  for (int f = threadIdx.x; f < a.v.n_frames; f += BB) { mine += a.w.fcost[f]; fl |= a.w.fflag[f]; }
  if (fl) atomicOr(&s_flag, 1);
  const double total = block_tree_sum(mine, s_sum);
  if (threadIdx.x == 0) {
    MapBundleCtl& c = *a.w.ctl;
    c.cost_start = total; c.cost_cur = total;
    int st = VOX_MAP_BUNDLE_OK;
    if (!refine_finite(total)) st = VOX_MAP_BUNDLE_NOT_FINITE;
    else if (s_flag) st = VOX_MAP_BUNDLE_BEHIND;
    else if (c.n_free_frames == 0 && c.n_free_points == 0) st = VOX_MAP_BUNDLE_NOTHING_FREE;
    c.status = st; c.dead = st != VOX_MAP_BUNDLE_OK;
  }
}

// ---- the landmark side: 16 lanes per landmark over its ordered list ------------------------------------------------
//   LIN     V_j = sum w Jp^T Jp, g_j = sum w Jp^T e over ALL its observations; V_j += lambda diag V_j; V_j^-1 by three solves
//   PASS_A  t_j = V_j^-1 sum over the observations in free frames of W^T p_f,  W^T v = w Jp^T (Jc v)
//   BACK    the candidate point p_j - V_j^-1 (g_j + sum over the observations in free frames of W^T x_f)
template <int MODE>
__global__ __launch_bounds__(BB) void bundle_point_kernel(MapBundleArgs a) {
  const MapBundleCtl& c = *a.w.ctl;
  if (c.dead) return;
  if (MODE == B_PASS_A && (c.bad || c.stop)) return;
  if (MODE == B_BACK && (c.bad || c.nostep)) return;
  const int M = a.v.size();
  const int lg = threadIdx.x & (BG - 1), grp = threadIdx.x / BG;
  const double lambda = c.lambda;
  const double* vec = MODE == B_PASS_A ? a.w.p : a.w.x;
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const int n_batches = (a.v.bound + BLPB - 1) / BLPB;
  for (int batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {      // (uniform in the workgroup: the DPP sums see whole rows)
    const int e = batch * BLPB + grp;
    const bool run = bundle_free_point(a, e, M);
    const int n = run ? a.l.cur[e] : 0;
    const int off = run ? a.l.offset(e) : 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (run) bundle_load(a.w.P + 3 * (size_t)e, p);
    constexpr int NT = MODE == B_LIN ? 9 : 3;
    double acc[9];                                           // (PASS_A and BACK use the first three)
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = 0.0;
    for (int j = lg; j < n; j += BG) {
      float2 m;
      const int f = a.v.decode(a.l.keys[off + j], m);
      if (MODE != B_LIN && a.w.pose_status[f] != BS_OK) continue;
      double T[12], P0[3], P1[3];
      bundle_load(a.w.T + 12 * (size_t)f, T);
      MapObs o;
      map_obs(K, T, p, (double)m.x, (double)m.y, a.huber, o);
      map_obs_point_jac(o, T, P0, P1);
      if constexpr (MODE == B_LIN) {
        accum_normal<3, false>(o, P0, P1, acc);
      } else {
        double v[6], C0[6], C1[6];
        bundle_load(vec + 6 * (size_t)f, v);
        map_obs_pose_jac(o, C0, C1);
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { s0 += C0[k] * v[k]; s1 += C1[k] * v[k]; }
        s0 *= o.w; s1 *= o.w;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += __builtin_fma(P1[k], s1, P0[k] * s0);
      }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = refine_row_sum(acc[k]);
    if (!run) {
      if (MODE == B_BACK && e < M && lg < 3) a.w.Pc[3 * (size_t)e + lg] = a.w.P[3 * (size_t)e + lg];
      continue;
    }
    if constexpr (MODE == B_LIN) {
      const double H[6] = {acc[0] + lambda * acc[0], acc[1], acc[2], acc[3] + lambda * acc[3], acc[4], acc[5] + lambda * acc[5]};
      double c0[3], c1[3], c2[3];
      const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
      const bool ok = ldlt3_solve(H, e0, c0) && ldlt3_solve(H, e1, c1) && ldlt3_solve(H, e2, c2) && refine_finite(acc[6]) &&
                      refine_finite(acc[7]) && refine_finite(acc[8]);
      if (lg == 0) {
        if (!ok) {
          a.w.ctl->bad = 1;                                   // (whoever meets one stores the same 1)
        } else {
          double* V = a.w.Vinv + 6 * (size_t)e;
          V[0] = c0[0]; V[1] = c1[0]; V[2] = c2[0]; V[3] = c1[1]; V[4] = c2[1]; V[5] = c2[2];
          double* g = a.w.gj + 3 * (size_t)e;
          g[0] = acc[6]; g[1] = acc[7]; g[2] = acc[8];
        }
      }
    } else {
      double Vi[6], y[3];
      bundle_load(a.w.Vinv + 6 * (size_t)e, Vi);
      if (MODE == B_PASS_A) {
        sym3_mul(Vi, acc, y);
        if (lg < 3) a.w.tj[3 * (size_t)e + lg] = lg == 0 ? y[0] : lg == 1 ? y[1] : y[2];
      } else {
        double g[3];
        bundle_load(a.w.gj + 3 * (size_t)e, g);
        const double s[3] = {g[0] + acc[0], g[1] + acc[1], g[2] + acc[2]};
        sym3_mul(Vi, s, y);
        if (lg < 3) a.w.Pc[3 * (size_t)e + lg] = p[lg == 0 ? 0 : lg == 1 ? 1 : 2] - (lg == 0 ? y[0] : lg == 1 ? y[1] : y[2]);
      }
    }
  }
}

// ---- the frame side: one workgroup per free frame over its rows ------------------------------------------------------
// U_f = sum w Jc^T Jc and g_f = sum w Jc^T e over ALL its rows; then, over the rows of free landmarks, sum W V^-1 W^T and
// sum W V^-1 g_j; stored: the damped U_f, D_f = U_f - the first sum, r_f = -g_f + the second
__global__ __launch_bounds__(BB) void bundle_frame_lin_kernel(MapBundleArgs a) {
  __shared__ double s_row[BROWS][BTERMS], s_tot[BTERMS];
  const MapBundleCtl& c = *a.w.ctl;
  const int f = blockIdx.x, tid = threadIdx.x;
  if (c.dead || a.w.pose_status[f] != BS_OK) return;
  const int M = a.v.size();
  const double lambda = c.lambda;
  double T[12], K[9];
  bundle_load(a.w.T + 12 * (size_t)f, T);
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const int32_t* ent = a.l.ent + (size_t)f * a.v.n_max;
  const float2* uv = reinterpret_cast<const float2*>(a.v.uv) + (size_t)f * a.v.uv_stride;
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0;
  for (int i = tid; i < a.v.n_max; i += BB) {
    const int e = ent[i];
    if (e < 0 || e >= M) continue;
    double p[3];
    bundle_load(a.w.P + 3 * (size_t)e, p);
    const float2 m = uv[i];
    MapObs o;
    double C0[6], C1[6];
    map_obs(K, T, p, (double)m.x, (double)m.y, a.huber, o);
    map_obs_pose_jac(o, C0, C1);
    accum_normal<6, false>(o, C0, C1, acc);
  }
  frame_reduce(acc, s_row, s_tot);
  double keep = 0.0;                                          // thread k < 27 keeps term k: the damped U (k < 21) or g (k >= 21)
  {
    const int diag[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[diag[k]] += lambda * acc[diag[k]];
#pragma unroll
    for (int k = 0; k < 27; ++k) if (tid == k) keep = acc[k];
  }
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0;
  for (int i = tid; i < a.v.n_max; i += BB) {
    const int e = ent[i];
    if (!bundle_free_point(a, e, M)) continue;
    double p[3], Vi[6], g[3];
    bundle_load(a.w.P + 3 * (size_t)e, p);
    bundle_load(a.w.Vinv + 6 * (size_t)e, Vi);
    bundle_load(a.w.gj + 3 * (size_t)e, g);
    const float2 m = uv[i];
    MapObs o;
    double C0[6], C1[6], P0[3], P1[3];
    map_obs(K, T, p, (double)m.x, (double)m.y, a.huber, o);
    map_obs_pose_jac(o, C0, C1);
    map_obs_point_jac(o, T, P0, P1);
    double W[6][3], Y[6][3];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double w0 = o.w * C0[r], w1 = o.w * C1[r];
#pragma unroll
      for (int k = 0; k < 3; ++k) W[r][k] = __builtin_fma(w1, P1[k], w0 * P0[k]);
      sym3_mul(Vi, W[r], Y[r]);
    }
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int b = r; b < 6; ++b) acc[k++] += Y[r][0] * W[b][0] + Y[r][1] * W[b][1] + Y[r][2] * W[b][2];
      acc[21 + r] += Y[r][0] * g[0] + Y[r][1] * g[1] + Y[r][2] * g[2];
    }
  }
  frame_reduce(acc, s_row, s_tot);
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    if (tid == k) {
      if (k < 21) { a.w.U[21 * (size_t)f + k] = keep; a.w.D[21 * (size_t)f + k] = keep - acc[k]; }
      else a.w.r[6 * (size_t)f + (k - 21)] = -keep + acc[k];
    }
  }
}

// (S p)_f = U_f p_f - sum over the rows of free landmarks of W t_j,  W v = w Jc^T (Jp v);  and p_f . (S p)_f
__global__ __launch_bounds__(BB) void bundle_frame_sp_kernel(MapBundleArgs a) {
  __shared__ double s_row[BROWS][BTERMS], s_tot[BTERMS];
  const MapBundleCtl& c = *a.w.ctl;
  const int f = blockIdx.x, tid = threadIdx.x;
  if (c.dead || c.bad || c.stop || a.w.pose_status[f] != BS_OK) return;
  const int M = a.v.size();
  double T[12], K[9];
  bundle_load(a.w.T + 12 * (size_t)f, T);
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = a.v.K[k];
  const int32_t* ent = a.l.ent + (size_t)f * a.v.n_max;
  const float2* uv = reinterpret_cast<const float2*>(a.v.uv) + (size_t)f * a.v.uv_stride;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < a.v.n_max; i += BB) {
    const int e = ent[i];
    if (!bundle_free_point(a, e, M)) continue;
    double p[3], t[3];
    bundle_load(a.w.P + 3 * (size_t)e, p);
    bundle_load(a.w.tj + 3 * (size_t)e, t);
    const float2 m = uv[i];
    MapObs o;
    double C0[6], C1[6], P0[3], P1[3];
    map_obs(K, T, p, (double)m.x, (double)m.y, a.huber, o);
    map_obs_pose_jac(o, C0, C1);
    map_obs_point_jac(o, T, P0, P1);
    const double s0 = o.w * (P0[0] * t[0] + P0[1] * t[1] + P0[2] * t[2]);
    const double s1 = o.w * (P1[0] * t[0] + P1[1] * t[1] + P1[2] * t[2]);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += __builtin_fma(C1[k], s1, C0[k] * s0);
  }
  frame_reduce(acc, s_row, s_tot);
  if (tid == 0) {
    double U[21], pv[6], pq = 0.0;
    bundle_load(a.w.U + 21 * (size_t)f, U);
    bundle_load(a.w.p + 6 * (size_t)f, pv);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < 6; ++b) s += U[r <= b ? tri6(r, b) : tri6(b, r)] * pv[b];
      const double q = s - acc[r];
      a.w.q[6 * (size_t)f + r] = q;
      pq += pv[r] * q;
    }
    a.w.pq[f] = pq;
  }
}

// ---- the vector side of PCG: one workgroup running lm_pcg.h's driver on the frames of status OK ------------------------------
// z_f = D_f^-1 r_f at the round's start: a frame whose D_f has a pivot that is not > 0 keeps its z and makes the round bad, as a
// landmark's V_j has before
__device__ __forceinline__ bool bundle_precondition(const MapBundleArgs& a, int* s_bad) {
  if (a.w.ctl->bad) return true;                              // (uniform; thread 0 writes it behind the sums' barriers)
  if (threadIdx.x == 0) *s_bad = 0;
  __syncthreads();
  for (int f = threadIdx.x; f < a.v.n_frames; f += BB) {
    if (a.w.pose_status[f] != BS_OK) continue;
    double D[21], r[6], z[6];
    bundle_load(a.w.D + 21 * (size_t)f, D);
    bundle_load(a.w.r + 6 * (size_t)f, r);
    if (!ldlt6d_solve(D, r, z)) { atomicOr(s_bad, 1); continue; }
#pragma unroll
    for (int k = 0; k < 6; ++k) a.w.z[6 * (size_t)f + k] = z[k];
  }
  __syncthreads();
  return *s_bad != 0;
}

// lm_cg_sweep fused in one loop -- D_f solves frame by frame, so nothing waits for another thread: x, r, z_f = D_f^-1 r_f and
// the thread's share of r.z and |r|^2 (with the two barriers and the trip through memory an iteration measured 5 % slower)
__device__ __forceinline__ void bundle_cg_sweep(const MapBundleArgs& a, double alpha, double& rz, double& rr) {
  for (int f = threadIdx.x; f < a.v.n_frames; f += BB) {
    if (a.w.pose_status[f] != BS_OK) continue;
    double D[21], r[6], z[6];
    bundle_load(a.w.D + 21 * (size_t)f, D);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      a.w.x[6 * (size_t)f + k] += alpha * a.w.p[6 * (size_t)f + k];
      r[k] = a.w.r[6 * (size_t)f + k] - alpha * a.w.q[6 * (size_t)f + k];
      a.w.r[6 * (size_t)f + k] = r[k];
    }
    if (!ldlt6d_solve(D, r, z))                               // (D factorised at the round's start: only a non-finite r ends here)
#pragma unroll
      for (int k = 0; k < 6; ++k) z[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { a.w.z[6 * (size_t)f + k] = z[k]; rz += r[k] * z[k]; rr += r[k] * r[k]; }
  }
}

__global__ __launch_bounds__(BB) void bundle_cg_init_kernel(MapBundleArgs a) {
  __shared__ double s_sum[256];
  __shared__ int s_bad;
  MapBundleCtl& c = *a.w.ctl;
  if (c.dead) return;
  lm_cg_begin<6, false>(c, a.v.n_frames, c.n_free_frames == 0, a.w.r, a.w.z, a.w.x, a.w.p, [&](int f) { return a.w.pose_status[f] == BS_OK; },
                        [&] { return bundle_precondition(a, &s_bad); }, s_sum);
}

__global__ __launch_bounds__(BB) void bundle_cg_update_kernel(MapBundleArgs a) {
  __shared__ double s_sum[256];
  lm_cg_step<6, false>(*a.w.ctl, a.v.n_frames, a.cg_tol, a.w.pq, a.w.z, a.w.p, [&](int f) { return a.w.pose_status[f] == BS_OK; },
                       [&](double alpha, double& rz, double& rr) { bundle_cg_sweep(a, alpha, rz, rr); }, s_sum);
}

// ---- the round's verdict: one workgroup ----------------------------------------------------------------------------------
__global__ __launch_bounds__(BDEC) void bundle_decide_kernel(MapBundleArgs a, int round) {
  __shared__ double s_sum[256];
  __shared__ int s_flag;
  MapBundleCtl& c = *a.w.ctl;
  vox_map_bundle_round* rec = a.rounds_out ? static_cast<vox_map_bundle_round*>(a.rounds_out) + round : nullptr;
  if (c.dead) { lm_round_skipped(rec); return; }
  const int M = a.v.size();
  const bool formed = lm_formed(c);
  if (threadIdx.x == 0) s_flag = 0;
  __syncthreads();
  double mine = 0.0;
  int fl = 0;
  if (formed && threadIdx.x < 256)
    for (int f = threadIdx.x; f < a.v.n_frames; f += 256) { mine += a.w.fcost[f]; fl |= a.w.fflag[f]; }
  if (fl) atomicOr(&s_flag, 1);
  const double cand = block_tree_sum(mine, s_sum);             // (its barriers publish s_flag too)
  if (lm_decide(c, rec, cand, s_flag != 0, c.n_free_frames > 0)) {
    for (size_t k = threadIdx.x; k < 12 * (size_t)a.v.n_frames; k += BDEC)
      if (a.w.pose_status[k / 12] == BS_OK) a.w.T[k] = a.w.Tc[k];
    for (size_t k = threadIdx.x; k < 3 * (size_t)M; k += BDEC) a.w.P[k] = a.w.Pc[k];
  }
}

// ---- the end: the state rounded to float32 into the candidate arrays, its cost (bundle_cost_kernel<FINAL>), the verdict ---------
__global__ __launch_bounds__(BB) void bundle_round_kernel(MapBundleArgs a) {
  if (a.w.ctl->dead) return;
  const int M = a.v.size();
  const size_t k = (size_t)blockIdx.x * BB + threadIdx.x;
  if (k < 12 * (size_t)a.v.n_frames) a.w.Tc[k] = (double)(float)a.w.T[k];
  if (k < 3 * (size_t)M) a.w.Pc[k] = (double)(float)a.w.P[k];
}

__global__ __launch_bounds__(BDEC) void bundle_finish_kernel(MapBundleArgs a) {
  __shared__ double s_sum[256];
  const MapBundleCtl& c = *a.w.ctl;
  const int M = a.v.size();
  double mine = 0.0;
  if (!c.dead && threadIdx.x < 256)
    for (int f = threadIdx.x; f < a.v.n_frames; f += 256) mine += a.w.fcost[f];
  const double total = block_tree_sum(mine, s_sum);
  const int status = lm_final_status(c, a.n_rounds, total, VOX_MAP_BUNDLE_NO_STEP, VOX_MAP_BUNDLE_COST_ROSE);
  const bool write = status == VOX_MAP_BUNDLE_OK && c.n_accepted > 0;
  for (int f = threadIdx.x; f < a.v.n_frames; f += BDEC) {
    const int ps = a.w.pose_status[f];
    if (a.pose_status_out) a.pose_status_out[f] = ps;
    if (write && ps == BS_OK) store_pose12(a.w.Tc + 12 * (size_t)f, a.T_out + 16 * (size_t)f);
  }
  for (int e = threadIdx.x; e < M; e += BDEC) {
    const int ps = a.w.point_status[e];
    if (a.point_status_out) a.point_status_out[e] = ps;
    if (write && ps == BS_OK)
      for (int k = 0; k < 3; ++k) a.v.pts[3 * (size_t)e + k] = (float)a.w.Pc[3 * (size_t)e + k];
  }
  if (threadIdx.x == 0) {
    vox_map_bundle_stats* s = static_cast<vox_map_bundle_stats*>(a.stats);
    s->status = status; s->n_frames = a.v.n_frames; s->n_entries = M; s->n_obs = c.n_obs; s->n_free_frames = c.n_free_frames;
    s->n_free_points = c.n_free_points; s->n_accepted = c.n_accepted; s->reserved = 0;
    s->cost_before = c.cost_start; s->cost_after = c.dead ? c.cost_start : total;
  }
}

MapBundleWs map_bundle_layout(void* base, int n_frames, int bound) {
  MapBundleWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames, B = (size_t)(bound > 0 ? bound : 1), d = sizeof(double);
  w.T = c.take<double>(12 * d * F); w.Tc = c.take<double>(12 * d * F);
  w.P = c.take<double>(3 * d * B); w.Pc = c.take<double>(3 * d * B);
  w.Vinv = c.take<double>(6 * d * B); w.gj = c.take<double>(3 * d * B); w.tj = c.take<double>(3 * d * B);
  w.U = c.take<double>(21 * d * F); w.D = c.take<double>(21 * d * F);
  w.r = c.take<double>(6 * d * F); w.x = c.take<double>(6 * d * F); w.z = c.take<double>(6 * d * F);
  w.p = c.take<double>(6 * d * F); w.q = c.take<double>(6 * d * F);
  w.pq = c.take<double>(d * F); w.fcost = c.take<double>(d * F);
  w.fflag = c.take<int>(4 * F); w.n_obs = c.take<int>(4 * F);
  w.pose_status = c.take<int32_t>(4 * F); w.point_status = c.take<int32_t>(4 * B);
  w.ctl = c.take<MapBundleCtl>(sizeof(MapBundleCtl));
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_map_bundle(hipStream_t st, const MapBundleArgs& a, int n_cu) {
  hipError_t e = launch_map_refine_lists(st, a.l, a.v.n_frames, a.v.n_max, a.v.bound);
  if (e != hipSuccess) return e;
  const dim3 frames(a.v.n_frames), wg(BB), one(1);
  const int B = a.v.bound > 0 ? a.v.bound : 1;
  const dim3 points(landmark_grid(a.v.bound, n_cu));
  hipLaunchKernelGGL(bundle_init_frames_kernel, frames, wg, 0, st, a);
  hipLaunchKernelGGL(bundle_init_points_kernel, dim3((B + BB - 1) / BB), wg, 0, st, a);
  hipLaunchKernelGGL(bundle_census_kernel, one, wg, 0, st, a);
  hipLaunchKernelGGL(bundle_cost_kernel<B_START>, frames, wg, 0, st, a);
  hipLaunchKernelGGL(bundle_start_kernel, one, wg, 0, st, a);
  for (int r = 0; r < a.n_rounds; ++r) {
    hipLaunchKernelGGL(bundle_point_kernel<B_LIN>, points, wg, 0, st, a);
    hipLaunchKernelGGL(bundle_frame_lin_kernel, frames, wg, 0, st, a);
    hipLaunchKernelGGL(bundle_cg_init_kernel, one, wg, 0, st, a);
    for (int k = 0; k < a.n_cg; ++k) {
      hipLaunchKernelGGL(bundle_point_kernel<B_PASS_A>, points, wg, 0, st, a);
      hipLaunchKernelGGL(bundle_frame_sp_kernel, frames, wg, 0, st, a);
      hipLaunchKernelGGL(bundle_cg_update_kernel, one, wg, 0, st, a);
    }
    hipLaunchKernelGGL(bundle_point_kernel<B_BACK>, points, wg, 0, st, a);
    hipLaunchKernelGGL(bundle_cost_kernel<B_CAND>, frames, wg, 0, st, a);
    hipLaunchKernelGGL(bundle_decide_kernel, one, dim3(BDEC), 0, st, a, r);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const size_t most = 12 * (size_t)a.v.n_frames > 3 * (size_t)B ? 12 * (size_t)a.v.n_frames : 3 * (size_t)B;
  hipLaunchKernelGGL(bundle_round_kernel, dim3((unsigned)((most + BB - 1) / BB)), wg, 0, st, a);
  hipLaunchKernelGGL(bundle_cost_kernel<B_FINAL>, frames, wg, 0, st, a);
  hipLaunchKernelGGL(bundle_finish_kernel, one, dim3(BDEC), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
