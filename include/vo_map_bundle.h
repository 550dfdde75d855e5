/* vo_map_bundle.h -- a second extension of the map's interface (vo_hip.h, which includes this file): the poses of a window and
 * the map's points adjusted JOINTLY, by Levenberg-Marquardt rounds whose reduced camera system is solved matrix-free by
 * preconditioned conjugate gradients (vox_map_bundle*).  Conventions, error codes, vo_map and vo_last_error are those of
 * vo_hip.h; the cost, the observations and both Jacobians are those of vo_map_adjust.h.
 *
 * A SECOND NAMESPACE.  The vo_ namespace is closed: vo_hip.h declares a pinned number of functions and vo_map_adjust.h exactly
 * its four, which alone carry a version node.  Entry points added from here on are spelled vox_ (vo, extension), are declared in
 * extension headers like this one, are exported unversioned, return the VO_* codes and set vo_last_error like every other call.
 * vo_abi_version() stays 1: nothing that existed has changed. */
#ifndef VO_MAP_BUNDLE_H
#define VO_MAP_BUNDLE_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* JOINT ADJUSTMENT.  Frames, pixels, appearances, d_n_rows, strides, K, d_T16 (in place) and d_fixed mean what they mean in
 * vo_map_adjust_batch_dev.  Enqueued on the context's stream; nothing is read back.  RULES:
 *   observation  exactly that of vo_map_refine / vo_map_refine_poses: a live row (frame f, position i) whose lookup returns an
 *                entry; key f * n_max + i.  A landmark consumes its observations in ascending key, a frame its rows in ascending
 *                i; two rows of one frame that hit one entry are two observations.
 *   cost         sum of rho(e), e = proj(K, T p) - uv, the full K, no gate, Huber by IRLS weight w = min(1, huber_px / |e|) --
 *                the cost of vo_map_adjust, term for term.
 *   unknowns     a frame is FREE when it is not held and has >= min_obs_pose observations; a landmark is FREE when it has
 *                >= min_obs_point observations, those from held frames included.  Everything else is a constant: its
 *                observations still count in the cost and in the blocks of the free side.
 *   gauge        the caller pins it with d_fixed.  With no frame held the gauge is free: the solution drifts in its seven
 *                free parameters (a rigid motion and the scale), as in vo_map_adjust; the damping keeps every round solvable.
 *   state        poses (12 entries: R column-major, t) and points live in DOUBLE in the workspace for the whole call, start at
 *                the float32 inputs widened, and are rounded to float32 once, at the end.
 *   round        one round is one attempt at the damping lambda (lambda0 in the first round):
 *                1. linearise at the state: per free landmark V_j = sum w Jp^T Jp, g_j = sum w Jp^T e; per free frame
 *                   U_f = sum w Jc^T Jc, g_f = sum w Jc^T e; Jc = j [I, -[p_cam]x] (the left perturbation of
 *                   vo_map_refine_poses), Jp = j R, j = d e / d p_cam.  W = w Jc^T Jp of an observation is recomputed wherever
 *                   it is needed and never stored.
 *                2. V_j += lambda diag V_j, U_f += lambda diag U_f (Marquardt).
 *                3. V_j^-1 by the 3x3 LDL^T of vo_map_refine.
 *                4. r_f = -g_f + sum over the frame's rows of free landmarks of W V_j^-1 g_j.
 *                5. D_f = U_f - sum over the same rows of W V_j^-1 W^T (the Schur-Jacobi preconditioner), solved by the 6x6
 *                   LDL^T of vo_map_refine_poses.
 *                6. PCG on S x = r, S = U - W V^-1 W^T (never formed), from x = 0: z = D^-1 r, p = z; per iteration
 *                   t_j = V_j^-1 sum over the landmark's observations in free frames of W^T p_f, then
 *                   (S p)_f = U_f p_f - sum over the frame's rows of free landmarks of W t_j, alpha = r.z / p.Sp, x += alpha p,
 *                   r -= alpha Sp, z = D^-1 r, beta = r.z / (the last r.z), p = z + beta p.  At most n_cg iterations; it stops
 *                   after an iteration with |r| <= cg_tol |r_0|, and before one whose p.Sp is not > 0 or not finite.  With no
 *                   free frame there is nothing to solve: no iteration, and that is no failure.
 *                7. dp_j = -V_j^-1 (g_j + sum over the observations in free frames of W^T x_f); the candidate is
 *                   v2t(x_f) T_f (the v2t of vo_map_refine_poses) and p_j + dp_j.
 *                8. the total cost of the candidate over ALL observations.
 *                9. ACCEPT iff that cost is finite, every observation of the candidate has camera z > 0 and the cost is <= the
 *                   current one: the candidate becomes the state, lambda <- max(lambda / 10, 1e-12) (a lambda of 0 stays 0).
 *               10. REJECT otherwise, and when a pivot of some V_j or D_f is not > 0, or when free frames exist and PCG could
 *                   not take one iteration: the state is unchanged, lambda <- max(10 lambda, 1e-6).
 *   sums         every sum is double and taken in an order that is a function of the data alone: a landmark's terms lane by
 *                lane (observation k of its list in lane k mod 16) and the 16 lanes by a fixed tree; a frame's terms thread by
 *                thread (row i in thread i mod 256), 16 lanes by the same tree, the 16 rows of lanes in order; a sum over
 *                frames into partial sum f mod 256 in frame order, the 256 partial sums by a binary tree.  No float atomics
 *                anywhere: three calls give the same bytes.
 *   end          the state is rounded to float32 (a pose: 12 entries, the bottom row written as 0, 0, 0, 1) and the total cost
 *                of the rounded state is evaluated.
 *   call status  in d_stats, in this order of precedence:
 *                NOT_FINITE    the total cost of the start is not finite
 *                BEHIND        some observation has camera z that is not > 0 at the start
 *                NOTHING_FREE  no free frame and no free landmark
 *                NO_STEP       n_rounds > 0 and no round was accepted
 *                COST_ROSE     the cost of the rounded final state exceeds the cost of the start
 *                OK            otherwise
 *   written      only OK writes, and only when a round was accepted: the 64 bytes of every free frame and the 12 bytes of every
 *                free landmark are replaced.  Every other byte of d_T16 and of the map, and everything under any other status,
 *                is left bit for bit.  n_rounds == 0 evaluates: it writes nothing but statuses and statistics, its status is
 *                OK, NOT_FINITE, BEHIND or NOTHING_FREE.
 * d_pose_status_out [n_frames] (or NULL): OK (free) / FIXED / FEW_OBS; d_point_status_out [map size] (or NULL): OK (free) /
 * UNSEEN / FEW_OBS -- the values of VO_MAP_POSE_* and VO_MAP_REFINE_* with the same names.  d_rounds_out [n_rounds] (or NULL,
 * 8-byte aligned): per round the current cost, the candidate's cost, the lambda used, the PCG iterations taken, the final
 * |r| / |r_0| and whether it was accepted; a round that formed no candidate (a pivot, no PCG step) records a candidate cost of
 * 0; under NOT_FINITE, BEHIND and NOTHING_FREE no round runs and the records are zero.  *d_stats (8-byte aligned).
 * The launches of a call are a fixed sequence -- 3 (n_cg + 2) per round, whatever the data: a round whose PCG has stopped
 * passes through its remaining launches, which return at once.  No launch waits for another workgroup.  A single frame is
 * traversed by ONE workgroup, as in vo_map_refine_poses: the call is meant for windows of many frames.
 * Capturable once a call of the same shape (n_frames, n_max) has sized the workspaces; a capture that would have to grow them
 * is refused (VO_ERR_NOT_READY) before anything is enqueued.  A captured call is launched for the map's CAPACITY, not for the
 * host's bound of the moment (vo_hip.h, A CALL CAPTURED ON A MAP), so that it reaches what an update behind it in the graph adds.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_adjust_batch_dev (n_rounds < 0, min_obs_pose < 3, min_obs_point < 2,
 * huber_px negative or not finite, and those of the frames), n_cg < 1, cg_tol or lambda0 negative or not finite, and
 * n_rounds * (n_cg + 2) > VOX_MAP_BUNDLE_MAX_STEPS. */
#define VOX_MAP_BUNDLE_MAX_STEPS 65536   /* most n_rounds * (n_cg + 2): 3 launches each */
#define VOX_MAP_BUNDLE_OK            0   /* a round was accepted (or n_rounds == 0) and the rounded state costs no more than the start */
#define VOX_MAP_BUNDLE_NOT_FINITE    1   /* the total cost of the start is not finite */
#define VOX_MAP_BUNDLE_BEHIND        2   /* at the start an observation has camera z that is not > 0 */
#define VOX_MAP_BUNDLE_NOTHING_FREE  3   /* no free frame and no free landmark */
#define VOX_MAP_BUNDLE_NO_STEP       4   /* no round was accepted */
#define VOX_MAP_BUNDLE_COST_ROSE     5   /* the rounded final state costs more than the start */
typedef struct vox_map_bundle_params {
  int32_t n_rounds, n_cg; float cg_tol, lambda0; int32_t min_obs_pose, min_obs_point; float huber_px;
} vox_map_bundle_params;
typedef struct vox_map_bundle_round {
  double cost, cost_candidate, lambda, residual; int32_t cg_iterations, accepted;
} vox_map_bundle_round;
typedef struct vox_map_bundle_stats {
  int32_t status, n_frames, n_entries, n_obs, n_free_frames, n_free_points, n_accepted, reserved; double cost_before, cost_after;
} vox_map_bundle_stats;
int vox_map_bundle_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                             size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                             float *d_T16 /* [n_frames][16], in place */, const uint8_t *d_fixed /* [n_frames] or NULL */,
                             const vox_map_bundle_params *params, int32_t *d_pose_status_out /* [n_frames] or NULL */,
                             int32_t *d_point_status_out /* [map size] or NULL */,
                             vox_map_bundle_round *d_rounds_out /* [n_rounds] or NULL */, vox_map_bundle_stats *d_stats);
/* host arrays as in vo_map_adjust; T16 in place, point_status_out [vo_map_size] (or NULL), rounds_out [n_rounds] (or NULL).
 * Uploads, the device call, one read-back; the same results bit for bit. */
int vox_map_bundle(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows, int n_max,
                   float *T16, const uint8_t *fixed, const vox_map_bundle_params *params, int32_t *pose_status_out,
                   int32_t *point_status_out, vox_map_bundle_round *rounds_out, vox_map_bundle_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_BUNDLE_H */
