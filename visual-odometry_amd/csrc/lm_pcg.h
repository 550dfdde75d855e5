// lm_pcg.h -- the driver that map_bundle.hip and pose_graph.hip share ("the driver"): Levenberg-Marquardt rounds
// around preconditioned conjugate gradients, run by one-workgroup launches on a control block in device memory.  A caller
// brings its vectors ([n_frames][W] doubles), which frames take part, its preconditioner and its launches; the order of every
// sum, the stop rules, the verdict and the lambda schedule are here, once.  Everything is double; nothing is read back.
#pragma once

#include "vo_math.h"

namespace vo {

// The control block of a call: written by the one-workgroup launches (and `bad` by whoever meets a pivot that is not > 0).
// Packed to its 76 bytes: a caller's block derives from it and puts its own counts behind n_accepted, where a base of natural
// alignment would pad; every block is carved at a multiple of 256 bytes, so the doubles lie at multiples of 8 all the same.
struct __attribute__((packed, aligned(4))) LmCtl {
  double lambda, cost_cur, cost_start, rz, rr0, rr;
  int status;                           // the call status decided at the start, 0 while alive
  int dead;                             // the start has decided the call: no round runs
  int bad;                              // this round: a pivot is not > 0
  int stop;                             // this round: PCG has stopped, its remaining launches return at once
  int nostep;                           // this round: PCG could not take one iteration
  int iters;                            // this round: PCG iterations taken
  int n_accepted;
};
static_assert(sizeof(LmCtl) == 76, "the callers' blocks keep their 88 bytes");

// v[k] <- the sum of v[k] over the workgroup in the order of the public headers: thread t < 256 brings its partial sums, then a
// binary tree over the thread index (t with t + 128, + 64, ... + 1); every thread of the workgroup (256 or more) calls it and
// gets the totals.  s: K * 256 doubles of LDS, free again behind the next barrier.
template <int K>
__device__ __forceinline__ void block_tree_sum(double (&v)[K], double* s) {
  const int t = threadIdx.x;
  __syncthreads();                                            // (s may still be read from the sum before)
  if (t < 256) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k * 256 + t] = v[k];
  }
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k * 256 + t] += s[k * 256 + t + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = s[k * 256];
}
__device__ __forceinline__ double block_tree_sum(double mine, double* s /* [256] */) {
  double v[1] = {mine};
  block_tree_sum<1>(v, s);
  return v[0];
}

// ---- the vector side of PCG, by ONE workgroup of 256 threads ---------------------------------------------------------------
// Thread t takes the frames t, t + 256, ... in that order and a frame's W entries in ascending order, in every loop: frame f
// goes into partial sum f mod 256 in frame order.  active(f): whether frame f takes part.  DENSE: the frames that take no part
// hold r = z = p = 0, so the loops that only read those need not ask (a caller without that promise leaves them unwritten).
// precond(): z = M^-1 r for every active frame, called by all threads, ending behind a barrier; returns, to every thread, whether
// a pivot was not > 0.  What it does with a frame it cannot solve is the caller's rule.

// The start of a round's PCG: x = 0, p = z = M^-1 r (p = 0 where nothing can be solved), r.z and |r_0|^2.  none_free: there is
// no active frame, PCG stops before it starts.
template <int W, bool DENSE, class Active, class Precond>
__device__ __forceinline__ void lm_cg_begin(LmCtl& c, int n_frames, bool none_free, const double* r, const double* z, double* x,
                                            double* p, Active active, Precond precond, double* s_sum /* [256] */) {
  const bool bad = precond();
  double rz = 0.0, rr = 0.0;
  for (int f = threadIdx.x; f < n_frames; f += 256) {
    const bool on = DENSE || active(f);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double zk = on && !bad ? z[W * (size_t)f + k] : 0.0;
      x[W * (size_t)f + k] = 0.0;
      p[W * (size_t)f + k] = zk;
      if (on) { const double rk = r[W * (size_t)f + k]; rz += rk * zk; rr += rk * rk; }
    }
  }
  const double t_rz = block_tree_sum(rz, s_sum);
  const double t_rr = block_tree_sum(rr, s_sum);
  if (threadIdx.x == 0) {
    c.bad = bad; c.iters = 0; c.nostep = 0;
    c.stop = bad || none_free;
    c.rz = t_rz; c.rr0 = t_rr; c.rr = t_rr;
  }
}

// The middle of an iteration in its plain shape: x += alpha p and r -= alpha q, a barrier, z = M^-1 r, a barrier, then this
// thread's share of r.z and |r|^2.  (A caller whose preconditioner works frame by frame may fuse the three in one loop of its
// own, as map_bundle.hip does: the sums receive the same operands in the same order.)
template <int W, bool DENSE, class Active, class Precond>
__device__ __forceinline__ void lm_cg_sweep(int n_frames, double alpha, const double* q, double* r, const double* z, double* x,
                                            const double* p, Active active, Precond precond, double& rz, double& rr) {
  for (int f = threadIdx.x; f < n_frames; f += 256) {
    if (!active(f)) continue;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      x[W * (size_t)f + k] += alpha * p[W * (size_t)f + k];
      r[W * (size_t)f + k] -= alpha * q[W * (size_t)f + k];
    }
  }
  __syncthreads();
  (void)precond();                    // (the blocks were factorised at the round's start: only a residual that is not finite fails here)
  __syncthreads();
  for (int f = threadIdx.x; f < n_frames; f += 256) {
    if (!DENSE && !active(f)) continue;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double rk = r[W * (size_t)f + k];
      rz += rk * z[W * (size_t)f + k]; rr += rk * rk;
    }
  }
}

// One iteration behind q = A p and pq[f] = p_f . q_f: p.q, alpha, then sweep(alpha, rz, rr) -- x, r, z = M^-1 r and the thread's
// share of r.z and |r|^2, lm_cg_sweep or a caller's fused form of it --, beta, p, the stop flag
template <int W, bool DENSE, class Active, class Sweep>
__device__ __forceinline__ void lm_cg_step(LmCtl& c, int n_frames, double cg_tol, const double* pq, const double* z, double* p,
                                           Active active, Sweep sweep, double* s_sum /* [256] */) {
  if (c.dead || c.bad || c.stop) return;
  const double rz_old = c.rz, rr0 = c.rr0;
  const int iters = c.iters;
  double mine = 0.0;
  for (int f = threadIdx.x; f < n_frames; f += 256)
    if (active(f)) mine += pq[f];
  const double pAp = block_tree_sum(mine, s_sum);
  if (!(pAp > 0.0) || !refine_finite(pAp)) {                   // (uniform: every thread holds the same total)
    if (threadIdx.x == 0) { c.stop = 1; c.nostep = iters == 0; }
    return;
  }
  double rz = 0.0, rr = 0.0;
  sweep(rz_old / pAp, rz, rr);
  const double t_rz = block_tree_sum(rz, s_sum);
  const double t_rr = block_tree_sum(rr, s_sum);
  const double beta = t_rz / rz_old;
  for (int f = threadIdx.x; f < n_frames; f += 256) {
    if (!DENSE && !active(f)) continue;
#pragma unroll
    for (int k = 0; k < W; ++k) p[W * (size_t)f + k] = z[W * (size_t)f + k] + beta * p[W * (size_t)f + k];
  }
  if (threadIdx.x == 0) {
    c.rz = t_rz; c.rr = t_rr; c.iters = iters + 1;
    if (!(sqrt(t_rr) > cg_tol * sqrt(rr0))) c.stop = 1;        // (a residual that is not finite stops as well)
  }
}

// ---- the round's verdict ------------------------------------------------------------------------------------------------------
// Rec: vox_map_bundle_round / voe_pose_graph_round (cost, cost_candidate, lambda, residual, cg_iterations, accepted).
// the record of a round that a dead call does not run
template <class Rec>
__device__ __forceinline__ void lm_round_skipped(Rec* rec) {
  if (threadIdx.x == 0 && rec) { rec->cost = 0.0; rec->cost_candidate = 0.0; rec->lambda = 0.0; rec->residual = 0.0; rec->cg_iterations = 0; rec->accepted = 0; }
}
// whether this round's PCG has left a step of which a candidate was formed
__device__ __forceinline__ bool lm_formed(const LmCtl& c) { return !c.bad && !c.nostep; }

// Called by every thread of the deciding workgroup with the candidate's total cost (anything when none was formed): the accept
// rule (veto: the caller's own reason against this candidate), the round's record, lambda / 10 floored at 1e-12 or x 10 floored
// at 1e-6, the reset of the round's flags.  solved: PCG had something to solve (the record's residual is 0 otherwise).  Returns
// whether the candidate is accepted; copying it into the state is the caller's.
template <class Rec>
__device__ __forceinline__ bool lm_decide(LmCtl& c, Rec* rec, double cand, bool veto, bool solved) {
  const bool formed = lm_formed(c);
  const double cur = c.cost_cur, lambda = c.lambda, rr0 = c.rr0, rr = c.rr;
  const int iters = c.iters, bad = c.bad;
  const bool accept = formed && refine_finite(cand) && !veto && cand <= cur;
  __syncthreads();                                            // (every thread has read the block that thread 0 now writes)
  if (threadIdx.x == 0) {
    if (rec) {
      rec->cost = cur; rec->cost_candidate = formed ? cand : 0.0; rec->lambda = lambda;
      rec->residual = (solved && !bad) ? (rr0 > 0.0 ? sqrt(rr / rr0) : 0.0) : 0.0;
      rec->cg_iterations = iters; rec->accepted = accept;
    }
    if (accept) {
      c.cost_cur = cand; c.n_accepted += 1;
      if (lambda > 0.0) { const double l = lambda / 10.0; c.lambda = l > 1e-12 ? l : 1e-12; }
    } else {
      const double l = 10.0 * lambda;
      c.lambda = l > 1e-6 ? l : 1e-6;
    }
    c.bad = 0; c.stop = 0; c.nostep = 0; c.iters = 0;
  }
  return accept;
}

// ---- the end ------------------------------------------------------------------------------------------------------------------------
// the call's status from the total cost of the rounded state: the start's when it decided the call, else NO_STEP / COST_ROSE
__device__ __forceinline__ int lm_final_status(const LmCtl& c, int n_rounds, double total, int no_step, int cost_rose) {
  if (c.dead) return c.status;
  if (n_rounds > 0 && c.n_accepted == 0) return no_step;
  if (!(total <= c.cost_start)) return cost_rose;              // (a cost that is not finite has risen)
  return c.status;
}

// 12 doubles (M column-major, then t) -> the 16 floats of a column-major 4 x 4
__device__ __forceinline__ void store_pose12(const double* T, float* o) {
  for (int col = 0; col < 4; ++col) {
    o[4 * col] = (float)T[3 * col]; o[4 * col + 1] = (float)T[3 * col + 1]; o[4 * col + 2] = (float)T[3 * col + 2];
    o[4 * col + 3] = col == 3 ? 1.f : 0.f;
  }
}

}  // namespace vo
