// pose_graph.hip -- a pose graph over similarities (voe_pose_graph*): Levenberg-Marquardt rounds on relative-pose edges, the
// damped system solved matrix-free by preconditioned conjugate gradients.  The rules are those of include/vo_pose_graph.h.
// Everything is double, every sum has a fixed order, nothing is read back and no launch waits for another workgroup: a round
// is a fixed sequence of 3 (n_cg + 2) launches,
//   pg_edge_kernel<LIN>       one thread per edge: A, E, the residual, the IRLS weights (the edge's record), its cost
//   pg_frame_lin_kernel       16 lanes per frame over its incidence list: g_f, H_ff, the chain weights W_f, r_f = -g_f
//   pg_cg_init_kernel         one workgroup: x = 0, z = M^-1 r, p = z, r.z, |r_0|^2
//   n_cg times  pg_edge_y_kernel      y_e = w o (J_i p_i + J_j p_j)
//               pg_frame_hp_kernel    q_f = sum J_f^T y_e + lambda diag(H_ff) o p_f and p_f . q_f
//               pg_cg_update_kernel   one workgroup: alpha, x, r, z = M^-1 r, beta, p, the stop flag
//   pg_candidate_kernel       the update of every active frame
//   pg_edge_kernel<CAND>      the candidate's cost per edge
//   pg_decide_kernel          one workgroup: the accept rule, lambda, the round's record, the copy
// M^-1 is the frames' diagonal blocks (JACOBI) or the exact inverse of the odometry chain's matrix (CHAIN): two segmented
// sums over the frames, run by the one workgroup of the PCG launches block after block with a running total.  Those launches,
// the verdict and the end run lm_pcg.h's driver, which map_bundle.hip shares.  A PCG that has stopped leaves `stop` set in the
// control block; its remaining launches read it and return at once.  The incidence lists
// are built like map_refine.hip's observation lists: count, block offsets, scan, scatter, order by rank.
#include "vo_internal.h"
#include "sim3.h"
#include "../../include/vo_pose_graph.h"

namespace vo {

constexpr int PB = 256;                   // threads per workgroup
constexpr int PG = 16;                    // lanes per frame
constexpr int PFPB = PB / PG;             // frames per workgroup of the 16-lane kernels
constexpr int PDEC = 1024;                // threads of the deciding workgroups (the first 256 take part in the sums)
static_assert(PB == MAP_WG && PG == MAP_ROW, "the shared helpers of vo_internal.h count on both sizes");

enum { PF_ACTIVE = 0, PF_HELD = 1, PF_ISOLATED = 2 };
enum { PE_START = 0, PE_LIN = 1, PE_CAND = 2 };
// an edge's record: M_A (9, column-major), t_A (3), c_A, t_E (3), the seven weights, the seven residuals
constexpr int REC_MA = 0, REC_TA = 9, REC_CA = 12, REC_TE = 13, REC_W = 16, REC_R = 23;
static_assert(REC_R + 7 == POSE_GRAPH_REC, "the record's length as the layout takes it");

static_assert(sizeof(voe_pose_graph_params) == 28 && sizeof(voe_pose_graph_round) == 40 && sizeof(voe_pose_graph_stats) == 48,
              "the deciding kernels write these records field by field");

// ---- 3x3 and similarity algebra, column-major, in the order the header's restatement uses ------------------------------------
// (pg_det3, pg_inv3, pg_mv: sim3.h)
__device__ __forceinline__ void pg_mtv(const double* M, const double* x, double* y) {
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = M[3 * c] * x[0] + M[3 * c + 1] * x[1] + M[3 * c + 2] * x[2];
}
__device__ __forceinline__ void pg_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double pg_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// S^-1 and A B for S = [M | t] as 12 doubles
__device__ __forceinline__ void pg_sim_inv(const double* S, double* O) {
  pg_inv3(S, O);
  double y[3];
  pg_mv(O, S + 9, y);
  O[9] = -y[0]; O[10] = -y[1]; O[11] = -y[2];
}
__device__ __forceinline__ void pg_sim_mul(const double* A, const double* B, double* O) {
#pragma unroll
  for (int c = 0; c < 3; ++c) pg_mv(A, B + 3 * c, O + 3 * c);
  double y[3];
  pg_mv(A, B + 9, y);
  O[9] = y[0] + A[9]; O[10] = y[1] + A[10]; O[11] = y[2] + A[11];
}
// the rotation's logarithm by the header's formula
__device__ __forceinline__ void pg_log_so3(const double* R, double* w) {
  const double v[3] = {(R[5] - R[7]) / 2.0, (R[6] - R[2]) / 2.0, (R[1] - R[3]) / 2.0};
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double theta = atan2(n, (R[0] + R[4] + R[8] - 1.0) / 2.0);
  const double k = theta < 1e-4 ? 1.0 + theta * theta / 6.0 : theta / n;
  w[0] = v[0] * k; w[1] = v[1] * k; w[2] = v[2] * k;
}
// what the adjoint of [c R | t] needs: M = c R, R, c, t
struct PgAd { double M[9], R[9], t[3], c; };
__device__ __forceinline__ void pg_ad_from(const double* S, PgAd& A) {
  A.c = cbrt(pg_det3(S));
#pragma unroll
  for (int k = 0; k < 9; ++k) { A.M[k] = S[k]; A.R[k] = S[k] / A.c; }
  A.t[0] = S[9]; A.t[1] = S[10]; A.t[2] = S[11];
}
// Ad u, Ad^T y, Ad^-1 u, Ad^-T y (the inverse written with R^T for R^-1)
__device__ __forceinline__ void pg_ad(const PgAd& A, const double* u, double* o) {
  double Rw[3], Mt[3], x[3];
  pg_mv(A.R, u + 3, Rw); pg_mv(A.M, u, Mt); pg_cross(A.t, Rw, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[k] = Mt[k] + x[k] - u[6] * A.t[k]; o[3 + k] = Rw[k]; }
  o[6] = u[6];
}
__device__ __forceinline__ void pg_ad_t(const PgAd& A, const double* y, double* o) {
  double x[3], d[3];
  pg_mtv(A.M, y, o);
  pg_cross(A.t, y, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = y[3 + k] - x[k];
  pg_mtv(A.R, d, o + 3);
  o[6] = y[6] - pg_dot(A.t, y);
}
__device__ __forceinline__ void pg_ad_inv(const PgAd& A, const double* u, double* o) {
  double x[3], d[3];
  pg_cross(A.t, u + 3, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = u[k] - x[k] + u[6] * A.t[k];
  pg_mtv(A.R, d, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] /= A.c;
  pg_mtv(A.R, u + 3, o + 3);
  o[6] = u[6];
}
__device__ __forceinline__ void pg_ad_inv_t(const PgAd& A, const double* y, double* o) {
  double x[3], Rb[3];
  pg_mv(A.R, y, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] /= A.c;
  pg_cross(A.t, o, x);
  pg_mv(A.R, y + 3, Rb);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[3 + k] = x[k] + Rb[k];
  o[6] = pg_dot(A.t, o) + y[6];
}
// G u and G^T y for G = [[I, -[t_E]x, t_E], [0, I, 0], [0, 0, 1]]
__device__ __forceinline__ void pg_g(const double* tE, const double* u, double* o) {
  double x[3];
  pg_cross(u + 3, tE, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[k] = u[k] + x[k] + u[6] * tE[k]; o[3 + k] = u[3 + k]; }
  o[6] = u[6];
}
__device__ __forceinline__ void pg_g_t(const double* tE, const double* y, double* o) {
  double x[3];
  pg_cross(tE, y, x);
#pragma unroll
  for (int k = 0; k < 3; ++k) { o[k] = y[k]; o[3 + k] = x[k] + y[3 + k]; }
  o[6] = pg_dot(tE, y) + y[6];
}
__device__ __forceinline__ void pg_rec_ad(const double* rec, PgAd& A) {
  A.c = rec[REC_CA];
#pragma unroll
  for (int k = 0; k < 9; ++k) { A.M[k] = rec[REC_MA + k]; A.R[k] = rec[REC_MA + k] / A.c; }
#pragma unroll
  for (int k = 0; k < 3; ++k) A.t[k] = rec[REC_TA + k];
}
// J u for the frame on `side` of the edge (0: it is i, J = -G Ad(A); 1: it is j, J = G), and J^T y
__device__ __forceinline__ void pg_j(const double* rec, const PgAd& A, int side, const double* u, double* o) {
  if (side) { pg_g(rec + REC_TE, u, o); return; }
  double v[7];
  pg_ad(A, u, v);
  pg_g(rec + REC_TE, v, o);
#pragma unroll
  for (int k = 0; k < 7; ++k) o[k] = -o[k];
}
__device__ __forceinline__ void pg_j_t(const double* rec, const PgAd& A, int side, const double* y, double* o) {
  if (side) { pg_g_t(rec + REC_TE, y, o); return; }
  double v[7];
  pg_g_t(rec + REC_TE, y, v);
  pg_ad_t(A, v, o);
#pragma unroll
  for (int k = 0; k < 7; ++k) o[k] = -o[k];
}
__device__ __forceinline__ constexpr int tri7(int r, int c) { return r * 7 - r * (r - 1) / 2 + (c - r); }

__device__ __forceinline__ int pg_offset(const PoseGraphWs& w, int f) { return w.cnt[f] + w.blk[f / PB]; }

// ---- the start: the state in double, the edges' statuses, the incidence lists ---------------------------------------------------
__global__ __launch_bounds__(PB) void pg_init_frames_kernel(PoseGraphArgs a) {
  const size_t k = (size_t)blockIdx.x * PB + threadIdx.x;
  if (k >= 12 * (size_t)a.n_frames) return;
  const size_t f = k / 12, e = k % 12;
  const double v = (double)a.S16[16 * f + (e % 3) + 4 * (e / 3)];
  a.w.T[k] = v; a.w.Tc[k] = v;
}

__device__ __forceinline__ bool pg_edge_live(const PoseGraphArgs& a, int e, int& i, int& j, double (&w3)[3]) {
  i = a.edges[2 * (size_t)e]; j = a.edges[2 * (size_t)e + 1];
  bool ok = i >= 0 && i < a.n_frames && j >= 0 && j < a.n_frames && i != j;
  bool some = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w3[k] = a.weights ? (double)a.weights[3 * (size_t)e + k] : 1.0;
    ok = ok && w3[k] >= 0.0 && refine_finite(w3[k]);
    some = some || w3[k] > 0.0;
  }
  return ok && some;
}

__global__ __launch_bounds__(PB) void pg_init_edges_kernel(PoseGraphArgs a) {
  const int e = blockIdx.x * PB + threadIdx.x;
  if (e >= a.n_edges) return;
  int i, j;
  double w3[3];
  const bool live = pg_edge_live(a, e, i, j, w3);
  a.w.estatus[e] = live ? VOE_POSE_GRAPH_EDGE_OK : VOE_POSE_GRAPH_EDGE_SKIPPED;
  if (live) { atomicAdd(&a.w.cnt[i], 1); atomicAdd(&a.w.cnt[j], 1); }      // (integer counts do not depend on the order)
}

__global__ __launch_bounds__(PB) void pg_offsets_kernel(PoseGraphArgs a) {
  __shared__ int s_wave[PB / 64];
  const int f = blockIdx.x * PB + threadIdx.x;
  int tot;
  const int x = block_exclusive_scan<PB>(f < a.n_frames ? a.w.cnt[f] : 0, s_wave, tot);
  if (f < a.n_frames) a.w.cnt[f] = x;
  if (threadIdx.x == 0) a.w.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PB) void pg_scatter_kernel(PoseGraphArgs a) {
  const int e = blockIdx.x * PB + threadIdx.x;
  if (e >= a.n_edges || a.w.estatus[e] != VOE_POSE_GRAPH_EDGE_OK) return;
  const size_t slots = 2 * (size_t)a.n_edges;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int f = a.edges[2 * (size_t)e + side];
    const int at = atomicAdd(&a.w.cur[f], 1);
    const size_t o = (size_t)pg_offset(a.w, f) + at;
    if (o < slots) a.w.lst_tmp[o] = 2 * e + side;             // (always: the segments partition the incidences)
  }
}

__global__ __launch_bounds__(PB) void pg_order_kernel(PoseGraphArgs a) {
  const size_t slots = 2 * (size_t)a.n_edges;
  const size_t s = (size_t)blockIdx.x * PB + threadIdx.x;
  if (s >= slots || s >= (size_t)*a.w.total) return;
  const int key = a.w.lst_tmp[s];
  if (key < 0 || (size_t)key >= slots) return;
  const int f = a.edges[key];                                 // (edges[2 e + side])
  if (f < 0 || f >= a.n_frames) return;
  const int off = pg_offset(a.w, f), n = a.w.cur[f];
  int rank = 0;
  for (int k = 0; k < n; ++k) rank += a.w.lst_tmp[off + k] < key;
  if ((size_t)off + rank < slots) a.w.keys[off + rank] = key;
}

// ---- an edge at a state: A, E, the residual, the weights, the cost -----------------------------------------------------------
// START and LIN read the state and write the record; CAND reads the candidate arrays (the candidate, or the rounded state at the
// end) and writes its cost alone.
template <int MODE>
__global__ __launch_bounds__(PB) void pg_edge_kernel(PoseGraphArgs a) {
  const PoseGraphCtl& c = *a.w.ctl;
  if (MODE == PE_LIN && c.dead) return;
  if (MODE == PE_CAND && (c.dead || c.bad || c.nostep)) return;
  const int e = blockIdx.x * PB + threadIdx.x;
  if (e >= a.n_edges) return;
  double* cost = (MODE == PE_CAND ? a.w.ecost_c : a.w.ecost) + 2 * (size_t)e;
  if (a.w.estatus[e] != VOE_POSE_GRAPH_EDGE_OK) {
    cost[0] = 0.0; cost[1] = 0.0;
    if (MODE == PE_START) a.w.es2_start[e] = 0.0;
    return;
  }
  int i, j;
  double w3[3];
  (void)pg_edge_live(a, e, i, j, w3);
  const double* T = MODE == PE_CAND ? a.w.Tc : a.w.T;
  double Si[12], Sj[12], Z[12], Ii[12], A[12], Iz[12], E[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    Si[k] = T[12 * (size_t)i + k]; Sj[k] = T[12 * (size_t)j + k];
    Z[k] = (double)a.Z16[16 * (size_t)e + (k % 3) + 4 * (k / 3)];
  }
  pg_sim_inv(Si, Ii); pg_sim_mul(Sj, Ii, A);
  pg_sim_inv(Z, Iz); pg_sim_mul(A, Iz, E);
  const double cE = cbrt(pg_det3(E));
  double R[9], r[7];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = E[k] / cE;
  r[0] = E[9]; r[1] = E[10]; r[2] = E[11];
  pg_log_so3(R, r + 3);
  r[6] = log(cE);
  const double s2 = w3[0] * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + w3[1] * (r[3] * r[3] + r[4] * r[4] + r[5] * r[5]) + w3[2] * (r[6] * r[6]);
  const double s = sqrt(s2);
  double rho = 1.0, val = s2;
  if (a.huber > 0.0 && s > a.huber) { rho = a.huber / s; val = a.huber * (2.0 * s - a.huber); }
  cost[0] = s2; cost[1] = val;
  if (MODE == PE_START) a.w.es2_start[e] = s2;
  if (MODE != PE_CAND) {
    double* rec = a.w.rec + POSE_GRAPH_REC * (size_t)e;
#pragma unroll
    for (int k = 0; k < 12; ++k) rec[REC_MA + k] = A[k];      // (M_A, then t_A)
    rec[REC_CA] = cbrt(pg_det3(A));
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[REC_TE + k] = E[9 + k];
#pragma unroll
    for (int k = 0; k < 7; ++k) { rec[REC_W + k] = rho * w3[k < 3 ? 0 : k < 6 ? 1 : 2]; rec[REC_R + k] = r[k]; }
  }
}

// one workgroup: the frames' kinds, the census, the cost of the start, what the call can be
__global__ __launch_bounds__(PB) void pg_start_kernel(PoseGraphArgs a) {
  __shared__ double s_sum[256];
  __shared__ int s_n[3];
  if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
  __syncthreads();
  int n_free = 0, n_active = 0, n_live = 0;
  for (int f = threadIdx.x; f < a.n_frames; f += PB) {
    const bool held = a.fixed && a.fixed[f] != 0;
    const int kind = held ? PF_HELD : a.w.cur[f] == 0 ? PF_ISOLATED : PF_ACTIVE;
    a.w.fstat[f] = kind;
    n_free += !held; n_active += kind == PF_ACTIVE;
  }
  double mine = 0.0;
  for (int e = threadIdx.x; e < a.n_edges; e += PB) {
    n_live += a.w.estatus[e] == VOE_POSE_GRAPH_EDGE_OK;
    mine += a.w.ecost[2 * (size_t)e + 1];
  }
  if (n_free) atomicAdd(&s_n[0], n_free);
  if (n_active) atomicAdd(&s_n[1], n_active);
  if (n_live) atomicAdd(&s_n[2], n_live);
  const double total = block_tree_sum(mine, s_sum);              // (its barriers publish s_n too)
  if (threadIdx.x == 0) {
    PoseGraphCtl c{};
    c.lambda = a.lambda0; c.cost_cur = total; c.cost_start = total;
    c.n_free = s_n[0]; c.n_active = s_n[1]; c.n_live = s_n[2];
    c.status = !refine_finite(total) ? VOE_POSE_GRAPH_NOT_FINITE
               : c.n_free == 0       ? VOE_POSE_GRAPH_NOTHING_FREE
               : c.n_live == 0       ? VOE_POSE_GRAPH_NO_EDGES
               : c.n_active == 0     ? VOE_POSE_GRAPH_NOTHING_FREE : VOE_POSE_GRAPH_OK;
    c.dead = c.status != VOE_POSE_GRAPH_OK;
    *a.w.ctl = c;
  }
}

// ---- linearisation of the frames: 16 lanes per frame over its incidence list ------------------------------------------------
__global__ __launch_bounds__(PB) void pg_frame_lin_kernel(PoseGraphArgs a) {
  const PoseGraphCtl& c = *a.w.ctl;
  if (c.dead) return;
  const int lane = threadIdx.x & (PG - 1), f = blockIdx.x * PFPB + (int)threadIdx.x / PG;
  const bool valid = f < a.n_frames && a.w.fstat[f] == PF_ACTIVE;
  double g[7] = {}, H[28] = {}, wl[3] = {}, wa[3] = {};
  if (valid) {
    const int off = pg_offset(a.w, f), n = a.w.cur[f];
    for (int k = lane; k < n; k += PG) {
      const int key = a.w.keys[off + k], e = key >> 1, side = key & 1;
      const double* rec = a.w.rec + POSE_GRAPH_REC * (size_t)e;
      PgAd A;
      pg_rec_ad(rec, A);
      double J[7][7];                                         // J[c]: column c
#pragma unroll
      for (int col = 0; col < 7; ++col) {
        double u[7] = {};
        u[col] = 1.0;
        pg_j(rec, A, side, u, J[col]);
      }
#pragma unroll
      for (int c1 = 0; c1 < 7; ++c1) {
        double s = 0.0;
#pragma unroll
        for (int k7 = 0; k7 < 7; ++k7) s += J[c1][k7] * (rec[REC_W + k7] * rec[REC_R + k7]);
        g[c1] += s;
#pragma unroll
        for (int c2 = c1; c2 < 7; ++c2) {
          double h = 0.0;
#pragma unroll
          for (int k7 = 0; k7 < 7; ++k7) h += J[c1][k7] * rec[REC_W + k7] * J[c2][k7];
          H[tri7(c1, c2)] += h;
        }
      }
      const int other = a.edges[2 * (size_t)e + (side ? 0 : 1)];
#pragma unroll
      for (int k3 = 0; k3 < 3; ++k3) {
        const double w = rec[REC_W + 3 * k3];
        wa[k3] += w;
        if (other == f - 1) wl[k3] += w;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = refine_row_sum(g[k]);
#pragma unroll
  for (int k = 0; k < 28; ++k) H[k] = refine_row_sum(H[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) { wl[k] = refine_row_sum(wl[k]); wa[k] = refine_row_sum(wa[k]); }
  if (f >= a.n_frames || lane != 0) return;
#pragma unroll
  for (int k = 0; k < 7; ++k) a.w.r[7 * (size_t)f + k] = (valid && (k < 6 || a.with_scale)) ? -g[k] : 0.0;
#pragma unroll
  for (int k = 0; k < 28; ++k) a.w.H[28 * (size_t)f + k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.w.W[3 * (size_t)f + k] = wl[k] > 0.0 ? wl[k] : wa[k] > 0.0 ? wa[k] : 1.0;
}

// ---- H p: the edges, then the frames ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void pg_edge_y_kernel(PoseGraphArgs a) {
  const PoseGraphCtl& c = *a.w.ctl;
  if (c.dead || c.bad || c.stop) return;
  const int e = blockIdx.x * PB + threadIdx.x;
  if (e >= a.n_edges || a.w.estatus[e] != VOE_POSE_GRAPH_EDGE_OK) return;
  const int i = a.edges[2 * (size_t)e], j = a.edges[2 * (size_t)e + 1];
  const double* rec = a.w.rec + POSE_GRAPH_REC * (size_t)e;
  PgAd A;
  pg_rec_ad(rec, A);
  double pi[7], pj[7], yi[7], yj[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { pi[k] = a.w.p[7 * (size_t)i + k]; pj[k] = a.w.p[7 * (size_t)j + k]; }
  pg_j(rec, A, 0, pi, yi);
  pg_j(rec, A, 1, pj, yj);
#pragma unroll
  for (int k = 0; k < 7; ++k) a.w.y[7 * (size_t)e + k] = rec[REC_W + k] * (yi[k] + yj[k]);
}

__global__ __launch_bounds__(PB) void pg_frame_hp_kernel(PoseGraphArgs a) {
  const PoseGraphCtl& c = *a.w.ctl;
  if (c.dead || c.bad || c.stop) return;
  const double lambda = c.lambda;
  const int lane = threadIdx.x & (PG - 1), f = blockIdx.x * PFPB + (int)threadIdx.x / PG;
  const bool valid = f < a.n_frames && a.w.fstat[f] == PF_ACTIVE;
  double q[7] = {};
  if (valid) {
    const int off = pg_offset(a.w, f), n = a.w.cur[f];
    for (int k = lane; k < n; k += PG) {
      const int key = a.w.keys[off + k], e = key >> 1, side = key & 1;
      const double* rec = a.w.rec + POSE_GRAPH_REC * (size_t)e;
      PgAd A;
      pg_rec_ad(rec, A);
      double y[7], o[7];
#pragma unroll
      for (int k7 = 0; k7 < 7; ++k7) y[k7] = a.w.y[7 * (size_t)e + k7];
      pg_j_t(rec, A, side, y, o);
#pragma unroll
      for (int k7 = 0; k7 < 7; ++k7) q[k7] += o[k7];
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) q[k] = refine_row_sum(q[k]);
  if (!valid || lane != 0) return;
  double pq = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double p = a.w.p[7 * (size_t)f + k];
    const double v = (k < 6 || a.with_scale) ? q[k] + lambda * a.w.H[28 * (size_t)f + tri7(k, k)] * p : 0.0;
    a.w.q[7 * (size_t)f + k] = v;
    pq += p * v;
  }
  a.w.pq[f] = pq;
}

// ---- M^-1 r, by the one workgroup (PB threads) of the PCG launches -----------------------------------------------------------------
struct PgScanLds { double v[2][PB][7]; int stop[2][PB]; double carry[7]; };

// the segmented inclusive sum of the header over one block of 256 positions: eight doubling steps, then the running total
__device__ __forceinline__ void pg_block_scan(double (&v)[7], bool stopped, PgScanLds& s) {
  const int i = threadIdx.x;
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    const int d = 1 << step, b = step & 1;
#pragma unroll
    for (int k = 0; k < 7; ++k) s.v[b][i][k] = v[k];
    s.stop[b][i] = stopped;
    __syncthreads();
    if (i >= d && !stopped) {
#pragma unroll
      for (int k = 0; k < 7; ++k) v[k] += s.v[b][i - d][k];
      stopped = s.stop[b][i - d] != 0;
    }
  }
  if (!stopped) {
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] += s.carry[k];
  }
  __syncthreads();
  if (i == PB - 1) {
#pragma unroll
    for (int k = 0; k < 7; ++k) s.carry[k] = v[k];
  }
  __syncthreads();
}

// z = M^-1 r over all frames; returns (to every thread) whether a pivot of JACOBI was not > 0
__device__ __forceinline__ bool pg_precondition(const PoseGraphArgs& a, double lambda, PgScanLds& s, int* s_bad) {
  const int tid = threadIdx.x, F = a.n_frames;
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  if (a.precond == VOE_POSE_GRAPH_JACOBI) {
    for (int f = tid; f < F; f += PB) {
      double z[7] = {};
      if (a.w.fstat[f] == PF_ACTIVE) {
        double D[28], r[7];
#pragma unroll
        for (int k = 0; k < 28; ++k) D[k] = a.w.H[28 * (size_t)f + k];
#pragma unroll
        for (int k = 0; k < 7; ++k) { D[tri7(k, k)] += lambda * D[tri7(k, k)]; r[k] = a.w.r[7 * (size_t)f + k]; }
        const bool ok = a.with_scale ? ldlt_solve<7, 7>(D, r, z) : ldlt_solve<6, 7>(D, r, z);     // (6: the leading block)
        if (!ok) {
          atomicOr(s_bad, 1);
#pragma unroll
          for (int k = 0; k < 7; ++k) z[k] = 0.0;
        }
        if (!a.with_scale) z[6] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < 7; ++k) a.w.z[7 * (size_t)f + k] = z[k];
    }
    __syncthreads();
    return *s_bad != 0;
  }
  const int nb = (F + PB - 1) / PB;
  if (tid < 7) s.carry[tid] = 0.0;
  __syncthreads();
  for (int b = nb - 1; b >= 0; --b) {                         // the suffix sum: position tid is frame b * 256 + 255 - tid
    const int f = b * PB + (PB - 1 - tid);
    const bool in = f < F, active = in && a.w.fstat[f] == PF_ACTIVE;
    double v[7] = {};
    PgAd A;
    if (active) {
      double r[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) r[k] = a.w.r[7 * (size_t)f + k];
      pg_ad_from(a.w.T + 12 * (size_t)f, A);
      pg_ad_t(A, r, v);
    }
    pg_block_scan(v, in && !active, s);
    if (active) {
      double cc[7], e[7];
      pg_ad_inv_t(A, v, cc);
#pragma unroll
      for (int k = 0; k < 7; ++k) cc[k] /= (1.0 + lambda) * a.w.W[3 * (size_t)f + (k < 3 ? 0 : k < 6 ? 1 : 2)];
      pg_ad_inv(A, cc, e);
#pragma unroll
      for (int k = 0; k < 7; ++k) a.w.tmp[7 * (size_t)f + k] = e[k];
    }
  }
  __syncthreads();
  if (tid < 7) s.carry[tid] = 0.0;
  __syncthreads();
  for (int b = 0; b < nb; ++b) {                              // the prefix sum: position tid is frame b * 256 + tid
    const int f = b * PB + tid;
    const bool in = f < F, active = in && a.w.fstat[f] == PF_ACTIVE;
    double v[7] = {};
    if (active) {
#pragma unroll
      for (int k = 0; k < 7; ++k) v[k] = a.w.tmp[7 * (size_t)f + k];
    }
    pg_block_scan(v, in && !active, s);
    if (in) {
      double z[7] = {};
      if (active) {
        PgAd A;
        pg_ad_from(a.w.T + 12 * (size_t)f, A);
        pg_ad(A, v, z);
        if (!a.with_scale) z[6] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < 7; ++k) a.w.z[7 * (size_t)f + k] = z[k];
    }
  }
  __syncthreads();
  return false;
}

// the two PCG launches: lm_pcg.h's driver on the ACTIVE frames (DENSE: the others keep r = z = p = 0)
__global__ __launch_bounds__(PB) void pg_cg_init_kernel(PoseGraphArgs a) {
  __shared__ PgScanLds s_scan;
  __shared__ double s_sum[256];
  __shared__ int s_bad;
  PoseGraphCtl& c = *a.w.ctl;
  if (c.dead) return;
  const double lambda = c.lambda;
  lm_cg_begin<7, true>(c, a.n_frames, false, a.w.r, a.w.z, a.w.x, a.w.p, [&](int f) { return a.w.fstat[f] == PF_ACTIVE; },
                       [&] { return pg_precondition(a, lambda, s_scan, &s_bad); }, s_sum);
}

__global__ __launch_bounds__(PB) void pg_cg_update_kernel(PoseGraphArgs a) {
  __shared__ PgScanLds s_scan;
  __shared__ double s_sum[256];
  __shared__ int s_bad;
  PoseGraphCtl& c = *a.w.ctl;
  const double lambda = c.lambda;
  const auto active = [&](int f) { return a.w.fstat[f] == PF_ACTIVE; };
  // (the blocks were factorised at the round's start: only a residual that is not finite fails here, and then z = 0 for every frame)
  const auto precond = [&] {
    const bool bad = pg_precondition(a, lambda, s_scan, &s_bad);
    if (bad)
      for (size_t k = threadIdx.x; k < 7 * (size_t)a.n_frames; k += PB) a.w.z[k] = 0.0;
    return bad;
  };
  lm_cg_step<7, true>(c, a.n_frames, a.cg_tol, a.w.pq, a.w.z, a.w.p, active, [&](double alpha, double& rz, double& rr) {
    lm_cg_sweep<7, true>(a.n_frames, alpha, a.w.q, a.w.r, a.w.z, a.w.x, a.w.p, active, precond, rz, rr);
  }, s_sum);
}

// ---- the candidate and the round's verdict --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void pg_candidate_kernel(PoseGraphArgs a) {
  const PoseGraphCtl& c = *a.w.ctl;
  if (c.dead || c.bad || c.nostep) return;
  const int f = blockIdx.x * PB + threadIdx.x;
  if (f >= a.n_frames) return;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = a.w.T[12 * (size_t)f + k];
  if (a.w.fstat[f] == PF_ACTIVE) {
    double x[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) x[k] = a.w.x[7 * (size_t)f + k];
    const double sx = sin(x[3]), cx = cos(x[3]), sy = sin(x[4]), cy = cos(x[4]), sz = sin(x[5]), cz = cos(x[5]);
    const double a10 = sx * sy, a12 = -sx * cy, a20 = -cx * sy, a22 = cx * cy;
    const double dR[9] = {cy * cz, a10 * cz + cx * sz, a20 * cz + sx * sz, cy * (-sz), a10 * (-sz) + cx * cz, a20 * (-sz) + sx * cz,
                          sy, a12, a22};                      // Rx Ry Rz, column-major
    const double es = a.with_scale ? exp(x[6]) : 1.0;
    double N[12];
#pragma unroll
    for (int col = 0; col < 4; ++col)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        N[r + 3 * col] = es * (dR[r] * T[3 * col] + dR[r + 3] * T[1 + 3 * col] + dR[r + 6] * T[2 + 3 * col]) + (col == 3 ? x[r] : 0.0);
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = N[k];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) a.w.Tc[12 * (size_t)f + k] = T[k];
}

__global__ __launch_bounds__(PDEC) void pg_decide_kernel(PoseGraphArgs a, int round) {
  __shared__ double s_sum[256];
  PoseGraphCtl& c = *a.w.ctl;
  voe_pose_graph_round* rec = a.rounds_out ? static_cast<voe_pose_graph_round*>(a.rounds_out) + round : nullptr;
  if (c.dead) { lm_round_skipped(rec); return; }
  double mine = 0.0;
  if (lm_formed(c) && threadIdx.x < 256)
    for (int e = threadIdx.x; e < a.n_edges; e += 256) mine += a.w.ecost_c[2 * (size_t)e + 1];
  const double cand = block_tree_sum(mine, s_sum);
  if (lm_decide(c, rec, cand, false, true))
    for (size_t k = threadIdx.x; k < 12 * (size_t)a.n_frames; k += PDEC) a.w.T[k] = a.w.Tc[k];
}

// ---- the end: the state rounded to float32 into the candidate arrays, its cost (pg_edge_kernel<CAND>), the verdict -------------
__global__ __launch_bounds__(PB) void pg_round_kernel(PoseGraphArgs a) {
  if (a.w.ctl->dead) return;
  const size_t k = (size_t)blockIdx.x * PB + threadIdx.x;
  if (k < 12 * (size_t)a.n_frames) a.w.Tc[k] = (double)(float)a.w.T[k];
}

__global__ __launch_bounds__(PDEC) void pg_finish_kernel(PoseGraphArgs a) {
  __shared__ double s_sum[256];
  const PoseGraphCtl& c = *a.w.ctl;
  double mine = 0.0;
  if (!c.dead && threadIdx.x < 256)
    for (int e = threadIdx.x; e < a.n_edges; e += 256) mine += a.w.ecost_c[2 * (size_t)e + 1];
  const double total = block_tree_sum(mine, s_sum);
  const int status = lm_final_status(c, a.n_rounds, total, VOE_POSE_GRAPH_NO_STEP, VOE_POSE_GRAPH_COST_ROSE);
  const bool write = status == VOE_POSE_GRAPH_OK && c.n_accepted > 0;
  if (write)
    for (int f = threadIdx.x; f < a.n_frames; f += PDEC)
      if (a.w.fstat[f] == PF_ACTIVE) store_pose12(a.w.Tc + 12 * (size_t)f, a.S16 + 16 * (size_t)f);
  for (int e = threadIdx.x; e < a.n_edges; e += PDEC) {
    if (a.edge_status_out) a.edge_status_out[e] = a.w.estatus[e];
    if (a.edge_cost_out) a.edge_cost_out[e] = write ? a.w.ecost_c[2 * (size_t)e] : a.w.es2_start[e];
  }
  if (threadIdx.x == 0) {
    voe_pose_graph_stats* s = static_cast<voe_pose_graph_stats*>(a.stats);
    s->status = status; s->n_frames = a.n_frames; s->n_edges = a.n_edges; s->n_live_edges = c.n_live; s->n_free_frames = c.n_free;
    s->n_active_frames = c.n_active; s->n_accepted = c.n_accepted; s->reserved = 0;
    s->cost_before = c.cost_start; s->cost_after = c.dead ? c.cost_start : total;
  }
}

PoseGraphWs pose_graph_layout(void* base, int n_frames, int n_edges) {
  PoseGraphWs w{};
  WsCarver c(base);
  const size_t F = (size_t)n_frames, E = (size_t)(n_edges > 0 ? n_edges : 1), d = sizeof(double);
  w.cnt = c.take<int>(4 * 2 * F); w.cur = w.cnt ? w.cnt + F : nullptr;      // (one memset clears both)
  w.T = c.take<double>(12 * d * F); w.Tc = c.take<double>(12 * d * F);
  w.rec = c.take<double>(POSE_GRAPH_REC * d * E);
  w.ecost = c.take<double>(2 * d * E); w.ecost_c = c.take<double>(2 * d * E); w.es2_start = c.take<double>(d * E);
  w.y = c.take<double>(7 * d * E);
  w.r = c.take<double>(7 * d * F); w.x = c.take<double>(7 * d * F); w.z = c.take<double>(7 * d * F);
  w.p = c.take<double>(7 * d * F); w.q = c.take<double>(7 * d * F); w.tmp = c.take<double>(7 * d * F);
  w.pq = c.take<double>(d * F); w.H = c.take<double>(28 * d * F); w.W = c.take<double>(3 * d * F);
  w.blk = c.take<int>(4 * ((F + PB - 1) / PB)); w.total = c.take<int>(4);
  w.lst_tmp = c.take<int>(4 * 2 * E); w.keys = c.take<int>(4 * 2 * E);
  w.estatus = c.take<int32_t>(4 * E); w.fstat = c.take<int32_t>(4 * F);
  w.ctl = c.take<PoseGraphCtl>(sizeof(PoseGraphCtl));
  w.bytes = c.bytes;
  return w;
}

hipError_t launch_pose_graph(hipStream_t st, const PoseGraphArgs& a) {
  const int F = a.n_frames, E = a.n_edges;
  const dim3 wg(PB), one(1), edges((unsigned)((E > 0 ? E : 1) + PB - 1) / PB), frame_blocks((unsigned)(F + PB - 1) / PB),
      rows((unsigned)(F + PFPB - 1) / PFPB), slots((unsigned)((2 * (size_t)(E > 0 ? E : 1) + PB - 1) / PB)),
      state((unsigned)((12 * (size_t)F + PB - 1) / PB));
  hipError_t e = hipMemsetAsync(a.w.cnt, 0, sizeof(int) * 2 * (size_t)F, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pg_init_frames_kernel, state, wg, 0, st, a);
  hipLaunchKernelGGL(pg_init_edges_kernel, edges, wg, 0, st, a);
  hipLaunchKernelGGL(pg_offsets_kernel, frame_blocks, wg, 0, st, a);
  e = launch_scan(st, a.w.blk, (int)frame_blocks.x, a.w.total);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pg_scatter_kernel, edges, wg, 0, st, a);
  hipLaunchKernelGGL(pg_order_kernel, slots, wg, 0, st, a);
  hipLaunchKernelGGL(pg_edge_kernel<PE_START>, edges, wg, 0, st, a);
  hipLaunchKernelGGL(pg_start_kernel, one, wg, 0, st, a);
  for (int r = 0; r < a.n_rounds; ++r) {
    hipLaunchKernelGGL(pg_edge_kernel<PE_LIN>, edges, wg, 0, st, a);
    hipLaunchKernelGGL(pg_frame_lin_kernel, rows, wg, 0, st, a);
    hipLaunchKernelGGL(pg_cg_init_kernel, one, wg, 0, st, a);
    for (int k = 0; k < a.n_cg; ++k) {
      hipLaunchKernelGGL(pg_edge_y_kernel, edges, wg, 0, st, a);
      hipLaunchKernelGGL(pg_frame_hp_kernel, rows, wg, 0, st, a);
      hipLaunchKernelGGL(pg_cg_update_kernel, one, wg, 0, st, a);
    }
    hipLaunchKernelGGL(pg_candidate_kernel, frame_blocks, wg, 0, st, a);
    hipLaunchKernelGGL(pg_edge_kernel<PE_CAND>, edges, wg, 0, st, a);
    hipLaunchKernelGGL(pg_decide_kernel, one, dim3(PDEC), 0, st, a, r);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pg_round_kernel, state, wg, 0, st, a);
  hipLaunchKernelGGL(pg_edge_kernel<PE_CAND>, edges, wg, 0, st, a);
  hipLaunchKernelGGL(pg_finish_kernel, one, dim3(PDEC), 0, st, a);
  return hipGetLastError();
}


// ---- the correction carried into the map (voe_map_apply_correction*) -----------------------------------------------------------
// An entry's reference frame is the frame of its first observation in ascending key f * n_max + i: an integer atomicMin over the
// lookup's hits, exact like the covisibility's atomicOr.  The entry moves by S_new[f]^-1 S_old[f], in double, rounded once.
__global__ __launch_bounds__(PB) void apply_key_kernel(MapApplyArgs a) {
  const size_t k = (size_t)blockIdx.x * PB + threadIdx.x;
  if (k >= (size_t)a.n_frames * (size_t)a.n_max) return;
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  const int e = a.ent[k];
  if (e >= 0 && e < M) atomicMin(&a.key[e], (int)k);
}

__global__ __launch_bounds__(PB) void apply_move_kernel(MapApplyArgs a) {
  __shared__ int s_n[2];
  if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
  __syncthreads();
  int M = a.hdr[0];
  M = M < a.cap ? M : a.cap;
  M = M < a.bound ? M : a.bound;
  const int e = blockIdx.x * PB + threadIdx.x;
  if (e < M) {
    const int key = a.key[e];
    const bool seen = key != MAP_APPLY_NO_KEY;
    const int f = seen ? key / a.n_max : -1;
    if (a.ref_frame_out) a.ref_frame_out[e] = f;
    if (seen) {
      atomicAdd(&s_n[0], 1);
      const float *so = a.S_old + 16 * (size_t)f, *sn = a.S_new + 16 * (size_t)f;
      bool same = true;
#pragma unroll
      for (int k = 0; k < 16; ++k) same = same && __float_as_uint(so[k]) == __float_as_uint(sn[k]);
      if (!same) {
        double O[12], N[12], I[12], p[3], q[3], d[3], o[3];
#pragma unroll
        for (int k = 0; k < 12; ++k) { O[k] = (double)so[(k % 3) + 4 * (k / 3)]; N[k] = (double)sn[(k % 3) + 4 * (k / 3)]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (double)a.pts[3 * (size_t)e + k];
        pg_mv(O, p, q);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = (q[k] + O[9 + k]) - N[9 + k];
        pg_inv3(N, I);
        pg_mv(I, d, o);
        const bool finite = refine_finite(o[0]) && refine_finite(o[1]) && refine_finite(o[2]);
        if (finite) {
          atomicAdd(&s_n[1], 1);
          if (!a.dry_run) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.pts[3 * (size_t)e + k] = (float)o[k];
          }
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) { a.stats[0] = M; a.stats[3] = 0; }
    if (s_n[0]) atomicAdd(&a.stats[1], s_n[0]);
    if (s_n[1]) atomicAdd(&a.stats[2], s_n[1]);
  }
}

hipError_t launch_map_apply_correction(hipStream_t st, const MapApplyArgs& a) {
  const size_t rows = (size_t)a.n_frames * (size_t)a.n_max, B = (size_t)(a.bound > 0 ? a.bound : 1);
  hipError_t e = hipMemsetAsync(a.key, 0x7f, sizeof(int) * B, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.stats, 0, 4 * sizeof(int), st);
  if (e != hipSuccess) return e;
  if (rows) hipLaunchKernelGGL(apply_key_kernel, dim3((unsigned)((rows + PB - 1) / PB)), dim3(PB), 0, st, a);
  hipLaunchKernelGGL(apply_move_kernel, dim3((unsigned)((B + PB - 1) / PB)), dim3(PB), 0, st, a);
  return hipGetLastError();
}

}  // namespace vo
