/* vo_map_loops.h -- an eighth extension header (vo_hip.h includes this file): LOOP EDGES found and measured in the map
 * (voe_map_loops*).  voe_map_covis says which frames share landmarks, voe_pose_graph distributes relative-pose edges over a
 * trajectory and voe_map_apply_correction carries the result into the map; this call produces what the second one takes: for a
 * window of frames with their drifted similarities, the edges (i, j, Z_ij, weights) of the loops the map itself shows.
 * Conventions, error codes, vo_map and vo_last_error are those of vo_hip.h; the namespace is the voe_ of vo_map_cull.h, whose
 * rule holds these symbols by itself: every exported voe_ function is declared in a header under include/ that vo_hip.h
 * includes, every declared one is exported, all unversioned.  vo_abi_version() stays 1. */
#ifndef VO_MAP_LOOPS_H
#define VO_MAP_LOOPS_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames, pixels, appearances, d_n_rows, the strides, n_max, the camera (rows, cols, z_near, z_far, K) mean what they mean in
 * vo_map_localise_batch_dev.  d_S16 [n_frames][16]: float32, column-major 4x4, S = [M | t] with M = c R, p_cam = S p_map: the
 * trajectory as it has drifted (the layout of voe_pose_graph; a rigid T16 is a valid input); read only.  A drifted map holds
 * every entry where its REFERENCE FRAME put it, so the landmarks an old frame sees lie in several mutually drifted coordinate
 * systems; a loop (i, j) is therefore measured against the BAND of i alone -- the entries whose reference frame lies in
 * [i - ref_window, i], which sit in the coordinate system of S_i up to ref_window steps of drift.  Enqueued on the context's
 * stream; nothing is read back; the map is NEVER written.  RULES:
 *   1 hits         the public vo_map_lookup_batch_dev with its entry output, bit for bit: e(f, row), -1 where the row has no
 *                  entry, is not live or holds a NaN.
 *   2 reference    ref(e): the rule of voe_map_apply_correction (vo_pose_graph.h) and its launches -- the frame of the first
 *                  observation in ascending key f * n_max + row, by an integer atomicMin; -1 for an entry no row sees.
 *                  d_ref_frame_out [map size] (or NULL) equals byte for byte what a dry_run voe_map_apply_correction on the
 *                  same frames writes.
 *   3 histogram    hist[j][r] is the number of entries e with sees(j, e) -- the sees() of vo_map_covis.h: two rows of one frame
 *                  on one entry count ONCE -- and ref(e) == r.  Integers, exact.  d_hist_out [n_frames][n_frames] (or NULL).
 *   4 candidate    c(i, j) = the sum of hist[j][r] over max(i - ref_window, 0) <= r <= i.  The candidate of frame j is the i
 *                  with 0 <= i < j - gap and c(i, j) >= min_shared that is best by (c descending, i ascending).  A frame may
 *                  have none.
 *   5 choice       frame j KEEPS its candidate iff no j' with 0 < |j' - j| <= separation has a candidate with a larger c, or
 *                  with an equal c and j' < j.  The survivors are ranked by (c descending, j ascending); the first max_loops
 *                  of them fill the slots 0, 1, ... in that order.  All integers, a function of the data alone.
 *   6 pairs        of slot l = (i, j): the live rows of frame j in ascending row whose entry e has
 *                  max(i - ref_window, 0) <= ref(e) <= i.  Two rows on one entry are TWO pairs, as in vo_map_localise.  Pair k
 *                  of the slot is (row, k); world point k is the entry's point as the map holds it; the slot's pixels are
 *                  frame j's n_max pixels, copied.  The slots are problems of the public batched calls at constant strides of
 *                  n_max elements (voe_map_loops_problems_dev).
 *   7 measurement  vo_estimate_pose_ransac_batch_dev (params->ransac) over the max_loops problems, then
 *                  vo_picp_solve_batch_dev (kernel_threshold, keep_outliers 0, n_iters) from the winners on their inliers.
 *                  CONTRACT: poses, inlier sets and solver statistics equal bit for bit the explicit sequence of those two
 *                  public calls on the gathered arrays; the call adds no arithmetic of its own.
 *   8 finish       STATUS of a slot, in this order of precedence (the names and numbers 0-4 of vo_map_localise):
 *                    EMPTY         no survivor filled it
 *                    FEW_MATCHES   fewer than 6 pairs
 *                    NO_CONSENSUS  the RANSAC fell back (its codes 1-3)
 *                    NOT_FINITE    the solved pose, or the Z formed from it, holds a NaN or an infinity
 *                    FEW_INLIERS   the solver's final inlier count is below min_inliers
 *                    OK            otherwise
 *                  EDGE of an OK slot, in double from the float32 inputs widened: c_i = cbrt(det M_i);
 *                  S'_j = [c_i R | c_i t] of the solved rigid pose [R | t]; Z = S'_j S_i^-1 with M^-1 the adjugate over the
 *                  determinant and S^-1 = [M^-1 | -M^-1 t] (the rule of vo_pose_graph.h); rounded to float32 once, the bottom
 *                  row written as 0 0 0 1.
 *                  WRITTEN  OK: edge (i, j), Z, the weights w_loop.  Every other candidate: edge (i, j), the identity, weights
 *                  0 0 0.  EMPTY: edge (-1, -1), the identity, weights 0 0 0.  By voe_pose_graph's live-edge rule every slot
 *                  that is not OK is SKIPPED there: the three arrays go into voe_pose_graph_dev behind the odometry edges with
 *                  no host step and no compaction.
 *                  RECORD   d_loops_out[l]: i, j (-1, -1 when EMPTY), c, the pairs, the RANSAC's status and inliers (the
 *                  pairs handed to the solver), the solver's inliers, the status, the solver's two chi^2 sums.
 *                  STATISTICS  n_frames; n_entries: the size the device holds; n_candidates: frames with a candidate;
 *                  n_survivors; n_slots: min(n_survivors, max_loops); n_ok; two reserved words, written as 0.
 * The launches of a call are a fixed sequence that depends on (n_frames, n_max, the map's size bound, max_loops,
 * n_hypotheses, n_iters) alone: the lookup's 3; the 2 memsets and 2 launches of the reference frames; a memset and a launch for
 * the bit rows; ONE launch for histogram, prefix sum and candidate (a workgroup per frame); one for the choice (one workgroup);
 * one for the pairs (a workgroup per slot); the two public calls; one for the finish.  No launch waits for another workgroup.
 * Capturable under the workspace rule of the other window calls: once a call of the same shape (n_frames, n_max, max_loops,
 * n_hypotheses) on this map has sized the workspaces, which the map handle owns (the two public calls keep theirs in the
 * context, by their own rule); a capture that would have to grow them is refused (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_lookup_batch_dev and of vo_map_localise_batch_dev for the frames, the
 * camera and (ransac, n_iters, min_inliers) -- n_hypotheses == 0 included: there is no prior; n_frames outside
 * 1 .. VOE_MAP_COVIS_MAX_FRAMES; gap < 0, ref_window < 0, min_shared < 1, separation < 0, max_loops < 1 or > n_frames; a w_loop
 * that is negative, not finite or all zero; a null d_S16, params, d_edges_out, d_Z16_out, d_weights_out, d_loops_out or d_stats;
 * d_loops_out or d_stats off an 8-byte boundary, any other array off a 4-byte one. */
#define VOE_MAP_LOOP_OK            0
#define VOE_MAP_LOOP_FEW_MATCHES   1
#define VOE_MAP_LOOP_NO_CONSENSUS  2
#define VOE_MAP_LOOP_FEW_INLIERS   3
#define VOE_MAP_LOOP_NOT_FINITE    4
#define VOE_MAP_LOOP_EMPTY         5
typedef struct voe_map_loops_params {
  int32_t gap, ref_window, min_shared, separation, max_loops, reserved0;
  vo_ransac_params ransac;
  float kernel_threshold; int32_t n_iters, min_inliers;
  float w_loop[3];          /* (w_t, w_r, w_s) of every OK edge */
  int32_t reserved1;
} voe_map_loops_params;
typedef struct voe_map_loop_record {
  int32_t i, j, c, n_pairs, ransac_status, ransac_inliers, num_inliers, status;
  float chi_inliers, chi_outliers;
} voe_map_loop_record;
typedef struct voe_map_loops_stats {
  int32_t n_frames, n_entries, n_candidates, n_survivors, n_slots, n_ok, reserved[2];
} voe_map_loops_stats;
int voe_map_loops_batch_dev(vo_map *m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9],
                            const float *d_uv, size_t uv_stride, const float *d_app, size_t app_stride, int n_max,
                            const int *d_n_rows /* [n_frames] or NULL */, const float *d_S16 /* [n_frames][16], read only */,
                            const voe_map_loops_params *params, int32_t *d_edges_out /* [max_loops][2] */,
                            float *d_Z16_out /* [max_loops][16] */, float *d_weights_out /* [max_loops][3] */,
                            voe_map_loop_record *d_loops_out /* [max_loops], 8-byte aligned */,
                            int32_t *d_hist_out /* [n_frames][n_frames] or NULL */, int32_t *d_ref_frame_out /* [map size] or NULL */,
                            voe_map_loops_stats *d_stats /* 8-byte aligned */);
/* host arrays: uv [n_frames][n_max][2], app [n_frames][n_max][10], n_rows [n_frames] (or NULL), S16 [n_frames][16]; hist_out and
 * ref_frame_out [vo_map_size] may be NULL.  Reads the size first, as voe_map_covis does.  Uploads, the device call, one
 * read-back; the same bytes. */
int voe_map_loops(vo_map *m, int n_frames, int rows, int cols, int z_near, int z_far, const float K[9], const float *uv,
                  const float *app, const int *n_rows, int n_max, const float *S16, const voe_map_loops_params *params,
                  int32_t *edges_out, float *Z16_out, float *weights_out, voe_map_loop_record *loops_out, int32_t *hist_out,
                  int32_t *ref_frame_out, voe_map_loops_stats *stats_out);
/* What the LAST voe_map_loops*_dev call on this map left in the map's workspace, for a caller that wants to weigh or to repeat
 * a measurement.  The problems of rule 6: world points [max_loops][n_max][3], pixels [max_loops][n_max][2], pairs
 * [max_loops][n_max][2] int32 (row, k), counts [max_loops]; the candidates of rule 4 [n_frames][2] int32 (i, c; i == -1: none);
 * the measurement of rule 7: the RANSAC's inlier pairs [max_loops][n_max][2] and their counts [max_loops], the solved poses
 * [max_loops][16] and the solver's statistics [max_loops][4] as vo_picp_solve_batch_dev writes them.  Device pointers, valid until
 * the next call on this map that sizes its workspaces; any output pointer may be NULL.  VO_ERR_NOT_READY before the first call. */
typedef struct voe_map_loops_problems {
  const float *d_world_xyz, *d_uv; const int32_t *d_pairs; const int *d_n_pairs; const int32_t *d_candidates;
  const int32_t *d_inlier_pairs; const int *d_n_inliers; const float *d_T16, *d_solver_stats;
} voe_map_loops_problems;
int voe_map_loops_problems_dev(vo_map *m, voe_map_loops_problems *out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_LOOPS_H */
