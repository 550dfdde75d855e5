/* vo_pose_graph.h -- a seventh extension header (vo_hip.h includes this file): a POSE GRAPH over similarities, optimised under
 * relative-pose edges (voe_pose_graph*).  It distributes measured constraints -- odometry steps and loop closures -- over a
 * trajectory in its seven parameters per frame, the scale included.  The call needs a context and no map.  Conventions, error
 * codes and vo_last_error are those of vo_hip.h; the namespace is the voe_ of vo_map_cull.h, whose rule holds these symbols by
 * itself: every exported voe_ function is declared in a header under include/ that vo_hip.h includes, every declared one is
 * exported, all unversioned.  vo_abi_version() stays 1. */
#ifndef VO_POSE_GRAPH_H
#define VO_POSE_GRAPH_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE OPTIMISER.  d_S16 [n_frames][16]: float32, column-major 4x4, S = [M | t] with M = c R (the layout of voe_map_align's
 * S16; a rigid T16 is a valid input), last row 0 0 0 1; updated in place.  d_edges [n_edges][2]: int32 (i, j).  d_Z16
 * [n_edges][16]: the measured Z_ij ~ S_j S_i^-1, which takes camera-i coordinates to camera-j.  d_weights [n_edges][3] (or
 * NULL: all ones): (w_t, w_r, w_s) on the translation, rotation and log-scale parts.  d_fixed [n_frames] (or NULL): != 0
 * holds the frame.  Enqueued on the context's stream; nothing is read back.  RULES:
 *   state        S of every frame as 12 doubles (M column-major, then t) in the context's workspace for the whole call,
 *                started at the float32 inputs widened, rounded to float32 once, at the end.  For any 3x3 M:
 *                c = cbrt(det M), R = M / c; M^-1 is the adjugate over the determinant; S^-1 = [M^-1 | -M^-1 t].
 *   live edge    0 <= i, j < n_frames, i != j, its three weights finite, >= 0 and not all zero.  Every other edge is
 *                SKIPPED (d_edge_status_out): it has no part in anything and is never a refusal.
 *   residual     of a live edge: A = S_j S_i^-1, E = A Z^-1, r = (t_E, log(R_E), ln c_E): seven numbers.  log(R), for
 *                v = (R32 - R23, R13 - R31, R21 - R12) / 2 (one-based row, column), n = |v|, theta = atan2(n, (tr R - 1) / 2):
 *                v (1 + theta^2 / 6) where theta < 1e-4, v theta / n otherwise.  A rotation residual near pi is out of
 *                scope: the formula's value stands.
 *   cost         s^2 = w_t |r_t|^2 + w_r |r_r|^2 + w_s r_s^2 per live edge; huber == 0: the cost is the sum of s^2;
 *                huber > 0: s^2 up to huber, huber (2 s - huber) beyond, by IRLS weight rho = min(1, huber / s) on all
 *                seven parts, as vo_map_refine words it.  The total is summed edge e into partial sum e mod 256 in edge
 *                order, the 256 partial sums by a binary tree.
 *   frames       HELD (d_fixed), ISOLATED (not held, no live edge touches it) or ACTIVE.  Only ACTIVE frames are unknowns;
 *                with with_scale == 0 their seventh parameter is held at 0 and every frame keeps its c: the rigid graph.
 *   update       a left perturbation d = (tau, omega, sigma): S <- [e^sigma Rx(omega_1) Ry(omega_2) Rz(omega_3) | tau] S,
 *                the v2t of vo_map_refine_poses with a scale.
 *   Jacobians    J_j = G, J_i = -G Ad(A), G = [[I, -[t_E]x, t_E], [0, I, 0], [0, 0, 1]].  For A = [c R | t], Ad(A) maps
 *                (tau, omega, sigma) to (c R tau + t x (R omega) - sigma t, R omega, sigma).  The inverse left Jacobian of
 *                the rotation part is taken as I; the accept rule keeps that from raising the cost.
 *   round        one attempt at the damping lambda (lambda0 in the first round):
 *                1. linearise at the state: per edge w = rho (w_t x 3, w_r x 3, w_s); per ACTIVE frame g_f = sum J_f^T (w r)
 *                   and H_ff = sum J_f^T diag(w) J_f over the frame's incident live edges in ascending 2 e + side (side 0:
 *                   the frame is i; 1: it is j): term k of that list in lane k mod 16 of the frame's 16 lanes, a lane's
 *                   terms in ascending k, the 16 lanes by the fixed tree of vo_map_refine (neighbour, other pair of the
 *                   quad, mirrored half row, mirrored row).  The lists are built on the device by count, scan and scatter and
 *                   ordered by rank, which costs deg^2 comparisons for a frame of deg incident edges (as vo_map_refine's
 *                   lists do per landmark): meant for hubs of hundreds of edges, not of 10^4.  No float atomics anywhere.
 *                2. PCG on (H + lambda diag H) x = -g from x = 0: z = M^-1 r, p = z; per iteration q = (H + lambda diag H) p,
 *                   alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M^-1 r, beta = r.z / (the last r.z), p = z + beta p.  At
 *                   most n_cg iterations; it stops after an iteration with |r| <= cg_tol |r_0| and before one whose p.q is not
 *                   > 0 or not finite.  H p is never formed: one pass over the edges, y_e = w o (J_i p_i + J_j p_j), then
 *                   one pass over the frames, q_f = sum J_f^T y_e in the order of step 1, plus lambda diag(H_ff) o p_f.
 *                   Sums over frames: frame f into partial sum f mod 256 in frame order, the 256 partial sums by a binary tree.
 *                3. the candidate: the update with x_f on every ACTIVE frame; its total cost.
 *                4. ACCEPT iff that cost is finite and <= the current one: the candidate becomes the state,
 *                   lambda <- max(lambda / 10, 1e-12) (a lambda of 0 stays 0).  REJECT otherwise, and when the
 *                   preconditioner met a pivot that is not > 0 at the round's start or PCG could not take one iteration: the state
 *                   is unchanged, lambda <- max(10 lambda, 1e-6).  (A solve that fails LATER in the round -- the blocks are
 *                   the same, so only a residual that is not finite can do it -- gives z = 0 for EVERY frame: r.z = 0, and
 *                   the next iteration stops on p.q or on the residual that is not finite.)
 *   M^-1         JACOBI: z_f = (H_ff + lambda diag H_ff)^-1 r_f by an LDL^T in natural order (7x7; 6x6 with with_scale == 0).
 *                CHAIN (the default): the exact inverse of the Gauss-Newton matrix of the odometry chain f - 1 -> f at zero
 *                residual, M^-1 = P W^-1 P^T with P = diag(Ad(S_f)) . prefix sum . diag(Ad(S_f)^-1), P^T the same with a suffix
 *                sum and the transposes:  a_f = Ad(S_f)^T r_f;  b_f = a_f + a_f+1 + ...;  d_f = Ad(S_f)^-1 W_f^-1 Ad(S_f)^-T b_f;
 *                h_f = ... + d_f-1 + d_f;  z_f = Ad(S_f) h_f.  Ad(S)^-1 is written with R^T for R^-1 and R^T / c for M^-1.
 *                Both sums restart at zero behind every frame that is not ACTIVE (whose a, d and z are zero).  W_f is
 *                (1 + lambda) x, for each of the three parts by itself, the summed rho w of the live edges joining f - 1 and f
 *                in either direction; where that is zero the summed rho w of all the frame's live edges; 1 where that is zero
 *                too.  With with_scale == 0 the seventh component of z is zeroed after the apply.  The sums are doubles in an
 *                order that is a function of n_frames alone: blocks of 256 consecutive frames, inside a block eight doubling
 *                steps (distance 1, 2, ... 128: v_k <- v_k + v_(k - distance), a restart stops a lane for good), the blocks in
 *                sequence with the running total added to every lane no restart has stopped.  Its iteration count follows the
 *                number of loop edges, JACOBI's the length of the chain.
 *   end          the state is rounded to float32 (bottom row written as 0 0 0 1) and its cost evaluated.
 *   call status  in d_stats, in this order of precedence:
 *                NOT_FINITE    the total cost of the start is not finite
 *                NOTHING_FREE  every frame is held
 *                NO_EDGES      no edge is live
 *                NOTHING_FREE  (again, behind NO_EDGES) no frame is ACTIVE: the live edges join held frames only
 *                NO_STEP       n_rounds > 0 and no round was accepted
 *                COST_ROSE     the cost of the rounded final state exceeds the cost of the start
 *                OK            otherwise
 *   written      only OK writes, and only when a round was accepted: the 64 bytes of every ACTIVE frame.  Every other byte of
 *                d_S16, and everything under any other status, is left bit for bit.  n_rounds == 0 evaluates.
 * OUTPUTS.  d_edge_status_out [n_edges] (or NULL).  d_edge_cost_out [n_edges] (or NULL, 8-byte aligned): s^2 (without the
 * Huber function) of every live edge at the state d_S16 holds after the call, 0 for a skipped one: a false loop stands out.
 * d_rounds_out [n_rounds] (or NULL, 8-byte aligned): the record of vox_map_bundle_round; zero where no round ran.  *d_stats
 * (8-byte aligned).
 * The launches are a fixed sequence that depends on (n_frames, n_edges, n_rounds, n_cg) alone -- 3 (n_cg + 2) per round; a PCG
 * that has stopped passes through its remaining launches, which return at once.  No launch waits for another workgroup.  The
 * PCG's vector updates and the sums of CHAIN run in ONE workgroup, block after block.  Capturable once a call with at least
 * these n_frames and n_edges has sized the workspace, which the context owns; a capture that would have to grow it is refused
 * (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): n_frames < 1, n_edges < 0, more than 2^24 frames or edges, a null d_S16, params or d_stats, null d_edges or d_Z16 with
 * n_edges > 0, a misaligned pointer (4 bytes for float32 / int32 arrays, 8 for the doubles and the records), n_rounds < 0,
 * n_cg < 1, cg_tol, lambda0 or huber negative or not finite, n_rounds * (n_cg + 2) > VOE_POSE_GRAPH_MAX_STEPS, an unknown
 * preconditioner. */
#define VOE_POSE_GRAPH_MAX_STEPS 65536   /* most n_rounds * (n_cg + 2): 3 launches each */
#define VOE_POSE_GRAPH_CHAIN         0   /* preconditioner: the odometry chain's exact inverse (two prefix sums) */
#define VOE_POSE_GRAPH_JACOBI        1   /* preconditioner: the frames' diagonal blocks */
#define VOE_POSE_GRAPH_EDGE_OK       0
#define VOE_POSE_GRAPH_EDGE_SKIPPED  1
#define VOE_POSE_GRAPH_OK            0
#define VOE_POSE_GRAPH_NOT_FINITE    1
#define VOE_POSE_GRAPH_NOTHING_FREE  2
#define VOE_POSE_GRAPH_NO_EDGES      3
#define VOE_POSE_GRAPH_NO_STEP       4
#define VOE_POSE_GRAPH_COST_ROSE     5
typedef struct voe_pose_graph_params {
  int32_t n_rounds, n_cg; float cg_tol, lambda0, huber; int32_t with_scale, preconditioner;
} voe_pose_graph_params;
typedef struct voe_pose_graph_round {
  double cost, cost_candidate, lambda, residual; int32_t cg_iterations, accepted;
} voe_pose_graph_round;
typedef struct voe_pose_graph_stats {
  int32_t status, n_frames, n_edges, n_live_edges, n_free_frames /* not held */, n_active_frames, n_accepted, reserved;
  double cost_before, cost_after;
} voe_pose_graph_stats;
int voe_pose_graph_dev(vo_ctx *ctx, int n_frames, float *d_S16 /* [n_frames][16], in place */, int n_edges,
                       const int32_t *d_edges /* [n_edges][2] */, const float *d_Z16 /* [n_edges][16] */,
                       const float *d_weights /* [n_edges][3] or NULL */, const uint8_t *d_fixed /* [n_frames] or NULL */,
                       const voe_pose_graph_params *params, int32_t *d_edge_status_out /* [n_edges] or NULL */,
                       double *d_edge_cost_out /* [n_edges] or NULL */, voe_pose_graph_round *d_rounds_out /* [n_rounds] or NULL */,
                       voe_pose_graph_stats *d_stats);
/* host arrays; S16 in place.  Uploads, the device call, one read-back; the same results bit for bit. */
int voe_pose_graph(vo_ctx *ctx, int n_frames, float *S16, int n_edges, const int32_t *edges, const float *Z16, const float *weights,
                   const uint8_t *fixed, const voe_pose_graph_params *params, int32_t *edge_status_out, double *edge_cost_out,
                   voe_pose_graph_round *rounds_out, voe_pose_graph_stats *stats_out);

/* CARRYING THE CORRECTION INTO THE MAP.  The frames' appearances, d_n_rows, the stride and n_max mean what they mean in every
 * window call (vo_map_refine_batch_dev); d_uv and uv_stride are taken for the sake of the common shape and not read (d_uv may be
 * NULL).  d_S16_old, d_S16_new [n_frames][16]: the frames' similarities before and after voe_pose_graph (p_cam = S p_map).  RULES:
 *   reference frame  of an entry: the frame f of its first observation in ascending key f * n_max + i over the hits of
 *                    vo_map_lookup_batch_dev on these frames -- an integer atomicMin on the key, exact.
 *   move             p' = S_new[f]^-1 (S_old[f] p) in double from the float32 widened (M^-1: the adjugate over the
 *                    determinant), rounded to float32 once: the entry keeps its place in its reference frame's camera.
 *   keeps every byte an entry no row of these frames sees (d_ref_frame_out -1); an entry whose reference frame's two
 *                    matrices are bit-equal (all 16 floats), so that a call with new == old leaves the map bit for bit; an
 *                    entry whose moved point is not finite; every entry under dry_run != 0 (the outputs are written as they
 *                    would be).  The hash table, the appearances and the header are never touched.
 *   afterwards       the rigid pose of frame f is [R | t / c] of its S_new (vo::rigid_pose, rigid_pose): every projection in
 *                    an entry's reference frame is what it was.
 * d_ref_frame_out [map size] (or NULL).  *d_stats (8-byte aligned): n_entries, n_seen, n_moved (under dry_run: that would
 * move).  The lookup's 3 launches, 2 memsets and 2 launches, whatever the data; nothing is read back; capturable under the
 * workspace rule of vo_map_refine_batch_dev.  Refused (VO_ERR_INVALID_ARG): n_frames outside 1 .. 65535, negative n_max, null
 * appearances with n_max > 0, a null d_S16_old, d_S16_new or d_stats, d_app or d_stats off an 8-byte boundary, a matrix array
 * off a 4-byte one, app_stride < n_max, more than 2^30 rows. */
typedef struct voe_map_apply_stats { int32_t n_entries, n_seen, n_moved, reserved; } voe_map_apply_stats;
int voe_map_apply_correction_batch_dev(vo_map *m, int n_frames, const float *d_uv /* not read */, size_t uv_stride, const float *d_app,
                                       size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                                       const float *d_S16_old, const float *d_S16_new, int dry_run,
                                       int32_t *d_ref_frame_out /* [map size] or NULL */, voe_map_apply_stats *d_stats);
/* host arrays (app [n_frames][n_max][10]; uv not read, may be NULL); ref_frame_out [vo_map_size] (or NULL).  Uploads, the device
 * call, one read-back; the same results bit for bit. */
int voe_map_apply_correction(vo_map *m, int n_frames, const float *uv, const float *app, const int *n_rows, int n_max,
                             const float *S16_old, const float *S16_new, int dry_run, int32_t *ref_frame_out,
                             voe_map_apply_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_POSE_GRAPH_H */
