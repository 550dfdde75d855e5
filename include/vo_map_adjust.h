/* vo_map_adjust.h -- an extension of the map's interface (vo_hip.h, which includes this file): the poses of a window refined
 * on the cost vo_map_refine minimises (vo_map_refine_poses*), and the alternation of the two halves (vo_map_adjust*).
 * Conventions, error codes, vo_map and vo_map_refine_stats are those of vo_hip.h. */
#ifndef VO_MAP_ADJUST_H
#define VO_MAP_ADJUST_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* POSE REFINEMENT (motion-only adjustment: the points are fixed, the poses move) -- the other half of the same cost.  Every
 * frame's pose is re-estimated from ALL its rows that hit an entry of the map, by Gauss-Newton on the reprojection error.
 * Frame f: pixels, appearances, d_n_rows, strides and K exactly as vo_map_refine_batch_dev takes them; start pose d_T16_in +
 * 16 f (column-major 4x4, p_cam = T p_map), result d_T16_out + 16 f (the two may be the same array).  Enqueued on the
 * context's stream: vo_map_lookup_batch_dev with the entry of every query position, ONE launch with one workgroup per frame
 * that runs all rounds (the pose never leaves the workgroup), one launch for the statistics.  A single frame therefore runs
 * on ONE compute unit, whatever its size: the call is meant for windows of frames and fills the device from about 256 frames
 * on.  RULES (those of REFINEMENT in vo_hip.h wherever they overlap):
 *   observation  a live row (frame f, position i) whose lookup returns an entry; a frame consumes its observations in
 *                ascending i; the point is the entry's float32 point widened to double; two rows that hit one entry are two
 *                observations.
 *   cost         sum of rho(e), e = proj(K, T p) - uv, the full K, no image or depth gate; huber_px as in REFINEMENT (IRLS,
 *                w = min(1, huber_px / |e|)).  It is the cost vo_map_refine minimises, term for term.
 *   round        dx = (t, alpha) with d p_cam / d dx = [I, -[p_cam]x]; H = sum w J^T J + damping I, b = sum w J^T e,
 *                dx = -H^-1 b by a 6x6 LDL^T in natural order; T <- v2t(dx) T with the solver's v2t (translation dx[0:3],
 *                R = Rx(dx3) Ry(dx4) Rz(dx5)).  Sums, solve, sin / cos and T are double; T is rounded to float32 once, after
 *                the last round, its bottom row written as 0, 0, 0, 1; no re-orthonormalisation.  n_rounds == 0 evaluates
 *                cost and status and changes no pose.
 *   status       per frame, in this order of precedence:
 *                FIXED       d_fixed[f] != 0
 *                FEW_OBS     fewer than min_obs observations
 *                NOT_FINITE  a sum of some evaluation, the step or the pose is not finite, or a pivot is not > 0 (the frame
 *                            stops there)
 *                BEHIND      at the start, in some round or at the end an observation has camera z that is not > 0 (sticky:
 *                            the rounds go on)
 *                COST_ROSE   the cost of the float32-rounded final pose is larger than the cost at the start
 *                OK          otherwise: the 64 bytes of the pose are replaced.  Every other status hands on the input pose
 *                            bit for bit.
 * d_status_out [n_frames] (or NULL) receives the statuses; d_H_out [n_frames][36] doubles (or NULL) the damped H of the last
 * solved round, column-major -- the pose's information matrix in pixels^-2, for callers that want a covariance -- written
 * only for frames that solved at least once; *d_stats (8-byte aligned) the census: n_obs counts the observations of all
 * frames, cost_before / cost_after are sums over the OK frames in double, taken in a fixed order (frames f, f + 1024, ... in
 * frame order into partial sum f mod 1024, the partial sums in order).  No float atomics: every output is a function of the
 * data alone, three calls give the same bytes.
 * Capturable once a call of the same shape (n_frames, n_max) has sized the workspace; a capture that would have to grow it is
 * refused (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_refine_batch_dev (d_T16_in and d_T16_out in the place of d_T16),
 * min_obs < 3, and n_rounds > VO_MAP_ADJUST_MAX_ROUNDS (all rounds run in one launch: the bound keeps a launch finite). */
#define VO_MAP_ADJUST_MAX_ROUNDS 65536   /* most rounds of a half, most sweeps of the alternation */
#define VO_MAP_POSE_OK          0   /* the pose was replaced */
#define VO_MAP_POSE_FIXED       1   /* held by d_fixed */
#define VO_MAP_POSE_FEW_OBS     2   /* fewer than min_obs observations */
#define VO_MAP_POSE_BEHIND      3   /* at the start, in some round or at the end, an observation has camera z that is not > 0 */
#define VO_MAP_POSE_NOT_FINITE  4   /* a non-finite sum, a pivot that is not > 0, a non-finite step or pose */
#define VO_MAP_POSE_COST_ROSE   5   /* final cost > initial cost */
typedef struct vo_map_pose_refine_params { int32_t n_rounds; int32_t min_obs; float huber_px; float damping; } vo_map_pose_refine_params;
typedef struct vo_map_pose_refine_stats  { int32_t n_frames, n_obs; int32_t by_status[6]; double cost_before, cost_after; } vo_map_pose_refine_stats;
int vo_map_refine_poses_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride,
                                  const float *d_app, size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                                  const float *d_T16_in /* [n_frames][16] */, const uint8_t *d_fixed /* [n_frames] or NULL: none */,
                                  const vo_map_pose_refine_params *params, float *d_T16_out /* [n_frames][16], may be d_T16_in */,
                                  int32_t *d_status_out /* [n_frames] or NULL */, double *d_H_out /* [n_frames][36] or NULL */,
                                  vo_map_pose_refine_stats *d_stats);
/* host arrays: uv [n_frames][n_max][2], app [n_frames][n_max][10], n_rows [n_frames] (or NULL), T16 [n_frames][16] IN PLACE,
 * fixed [n_frames] (or NULL); status_out [n_frames] (or NULL), H_out [n_frames][36] (or NULL: frames that never solved keep
 * what the array held).  Uploads, the device call, one read-back; the same results bit for bit. */
int vo_map_refine_poses(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows,
                        int n_max, float *T16, const uint8_t *fixed, const vo_map_pose_refine_params *params,
                        int32_t *status_out, double *H_out, vo_map_pose_refine_stats *stats_out);

/* ADJUSTMENT (block-coordinate bundle adjustment): n_sweeps sweeps, each the pose half -- vo_map_refine_poses_batch_dev in
 * place on d_T16 with pose_rounds / min_obs_pose -- and then the point half -- vo_map_refine_batch_dev in place on the map
 * with point_rounds / min_obs_point from the poses just written --, huber_px and damping shared.  Nothing is read back between
 * them.  Every half-sweep minimises the same total cost over its own block with the other block fixed and keeps only what
 * does not raise its cost, so the total over all observations cannot rise from one half-sweep to the next.  Alternation is a
 * descent, not a fast one: it is linear where a joint solver is quadratic (DESIGN.md section 4.14 has figures).
 * GAUGE.  The caller pins it with d_fixed.  With no frame held the solution drifts in its seven free parameters (a rigid
 * motion and the scale); hold two frames, or one frame and accept the scale of the start.
 * Outputs: d_pose_status_out [n_frames] (or NULL) and d_point_status_out [map size] (or NULL) are those of the last sweep;
 * d_stats [n_sweeps] (8-byte aligned) one pair of statistics per sweep.
 * CONTRACT.  The call adds no arithmetic: poses, the map's bytes, statuses and every per-sweep statistic equal BIT FOR BIT
 * the explicit loop of the two public calls.  (The lookup depends on neither poses nor points: it runs once per call.)
 * Capturable once a call of the same shape has sized the workspaces.  Refused (VO_ERR_INVALID_ARG): n_sweeps outside
 * 1 .. VO_MAP_ADJUST_MAX_ROUNDS, pose_rounds or point_rounds above it, and the refusals of the two halves. */
typedef struct vo_map_adjust_params {
  int32_t n_sweeps, pose_rounds, point_rounds, min_obs_pose, min_obs_point; float huber_px, damping;
} vo_map_adjust_params;
typedef struct vo_map_adjust_stats { vo_map_pose_refine_stats poses; vo_map_refine_stats points; } vo_map_adjust_stats;
int vo_map_adjust_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                            size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                            float *d_T16 /* [n_frames][16], in place */, const uint8_t *d_fixed /* [n_frames] or NULL */,
                            const vo_map_adjust_params *params, int32_t *d_pose_status_out /* [n_frames] or NULL */,
                            int32_t *d_point_status_out /* [map size] or NULL */, vo_map_adjust_stats *d_stats /* [n_sweeps] */);
/* host arrays as in vo_map_refine_poses and vo_map_refine; T16 in place, point_status_out [vo_map_size] (or NULL),
 * stats_out [n_sweeps].  Uploads, the device call, one read-back; the same results bit for bit. */
int vo_map_adjust(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows, int n_max,
                  float *T16, const uint8_t *fixed, const vo_map_adjust_params *params, int32_t *pose_status_out,
                  int32_t *point_status_out, vo_map_adjust_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_ADJUST_H */
