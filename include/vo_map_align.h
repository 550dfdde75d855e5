/* vo_map_align.h -- a fourth extension of the map's interface (vo_hip.h, which includes this file): TWO maps.  How two maps of
 * one scene relate (voe_map_align*: a similarity found by 3-point RANSAC on the landmarks they share) and one map put into
 * the other (voe_map_merge*).  Conventions, error codes, vo_map and vo_last_error are those of vo_hip.h; the namespace is the
 * voe_ of vo_map_cull.h, whose rule holds these symbols by itself: every exported voe_ function is declared in a header under
 * include/ that vo_hip.h includes, every declared one is exported, all unversioned.  vo_abi_version() stays 1. */
#ifndef VO_MAP_ALIGN_H
#define VO_MAP_ALIGN_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The host's bound of the map's size: what sizes the launches of every call on the map where the host must not wait (the size
 * the host last learnt plus the rows of every update since; the capacity once an update has been captured).  Never below the
 * size the device holds.  No device work. */
int voe_map_size_bound(vo_map *m, int *n_max_out);

/* ALIGNMENT.  Finds the similarity S = [c R | t] with p_dst ~ c R p_src + t.  Both maps on one context; neither is written.
 * Enqueued on the context's stream; nothing is read back.  n_max below is voe_map_size_bound(src) at the time of the call.
 * RULES:
 *   matches      vo_map_lookup_dev on dst with src's appearance array, n_max as above, d_n_rows = src's device size.  Match k
 *                is (src entry, dst entry), in ascending src entry: the pairs are bit for bit those of the public lookup.
 *                n = the number of matches.  Pair k is the six float32 a = src's point of the src entry, b = dst's point of
 *                the dst entry.
 *   sampling     draw(h, j) of vo_estimate_transform_ransac (vo_hip.h) with n = the matches.  The sample of hypothesis h is the
 *                first 3 DISTINCT values of draw(h, 0), draw(h, 1), ... within j < 64.
 *   solve        Umeyama 1991 on m pairs (m = 3 for a hypothesis), in DOUBLE from the float32 points widened:
 *                  ca, cb = the means of a, b;  da = a - ca, db = b - cb
 *                  Sigma = (1/m) sum db da^T;  var_a = (1/m) sum |da|^2
 *                  svd3(Sigma) = U diag(s) V^T (s descending)
 *                  D = diag(1, 1, d), d = -1 when det U * det V < 0 and +1 otherwise;  R = U D V^T
 *                  c = (s0 + s1 + d s2) / var_a, and c = 1 when with_scale == 0
 *                  t = cb - c R ca
 *                invalid on any of: (a hypothesis) fewer than 3 distinct draws; var_a not > 0 or not finite; s1 <= 1e-9 s0 (a
 *                degenerate triangle: rank < 2); c not > 0; any of the 12 numbers c R, t not finite.
 *                The 12 numbers M = c R (column-major 3x3) and t are then rounded to float32: that is the model.
 *   scoring      in float32, fused multiply-adds in exactly this order (fma(x, y, z) = x y + z rounded once):
 *                  r_i = fma(M[i], a0, fma(M[i+3], a1, fma(M[i+6], a2, t_i))) - b_i          i = 0, 1, 2
 *                  d2  = fma(r_0, r_0, fma(r_1, r_1, r_2 * r_2))
 *                pair k is an inlier iff d2 < threshold * threshold (the product in float32; strict; a NaN is an outlier).
 *                An invalid hypothesis has count -1.  The winner: most inliers, ties to the lowest h.
 *   refit        n_refits rounds (0 .. VOE_MAP_ALIGN_MAX_REFITS).  Each takes the inliers of the current model (the winner's at
 *                first, the previous refit's afterwards) and runs the solve over all of them.  Two passes: the sums of a and
 *                of b first, then the centred moments.  Every sum is taken in a fixed order -- inlier pairs k in blocks of 256,
 *                a block's terms by a binary tree over k mod 256 (k with k + 128, then + 64, ... + 1), the blocks' sums by the
 *                same tree over block index mod 256 after each of the 256 has added its blocks in ascending order -- with no
 *                floating-point atomics: three calls give the same bytes.  The model is rounded to float32.  A round with
 *                fewer than 3 inliers or an invalid solve ends the refits (the launches still run, and return at once).
 *                The result is the last valid refit if its inlier count is >= the winner's; otherwise the winner's minimal
 *                model and mask.  stats.refit_kept says which (1: the refit).  Decided on the device.
 *   status       the first that holds: FEW_MATCHES (n < 3), NO_HYPOTHESIS (every hypothesis invalid), FEW_INLIERS (the final
 *                count < max(min_inliers, 3)), OK.  Not OK: d_S16_out is the identity, the mask all 0, n_inliers 0, refit_kept 0,
 *                scale 1 and rms 0.  The call still returns VO_OK: a failed alignment is a status, as in vo_map_localise.
 *   outputs      d_S16_out        column-major 4x4: M, t, last row 0 0 0 1
 *                d_pairs_out      [n_max][2], *d_n_matches: the lookup's (8-byte aligned)
 *                d_inlier_mask    [n_max] bytes, or NULL: 1 for the final model's inliers, 0 elsewhere (all n_max are written)
 *                d_hypothesis_counts  [n_hypotheses], or NULL
 *                *d_stats         (8-byte aligned) status, n_matches, n_inliers, best_hypothesis (-1: none), best_count (the
 *                                 winner's), n_valid (hypotheses), refit_kept; scale: the returned model's c in double, before
 *                                 the rounding; rms: sqrt(mean d2) over the final inliers, in DOUBLE from the float32 model
 *                                 and points widened, r_i = ((M[i] a0 + M[i+3] a1) + M[i+6] a2 + t_i) - b_i left to right,
 *                                 d2 = (r_0 r_0 + r_1 r_1) + r_2 r_2, summed in the order of the refit's sums.
 * The launches are a fixed sequence whatever the data (they depend on n_max, n_hypotheses and n_refits alone), and no launch
 * waits for another workgroup.  Capturable once a call of the same shape has sized the workspaces, which dst's handle owns;
 * otherwise VO_ERR_NOT_READY before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): a null map, src == dst, maps of different contexts, n_hypotheses outside 1 .. 65536, n_refits
 * outside 0 .. VOE_MAP_ALIGN_MAX_REFITS, min_inliers < 0, a threshold not positive or not finite, a null or misaligned output. */
#define VOE_MAP_ALIGN_OK             0
#define VOE_MAP_ALIGN_FEW_MATCHES    1
#define VOE_MAP_ALIGN_NO_HYPOTHESIS  2
#define VOE_MAP_ALIGN_FEW_INLIERS    3
#define VOE_MAP_ALIGN_MAX_REFITS     16
typedef struct voe_map_align_params {
  uint64_t seed; int32_t n_hypotheses, with_scale, n_refits, min_inliers; float threshold /* in dst's units */; int32_t reserved;
} voe_map_align_params;                                       /* 32 bytes */
typedef struct voe_map_align_stats {
  int32_t status, n_matches, n_inliers, best_hypothesis, best_count, n_valid, refit_kept, reserved; double scale, rms;
} voe_map_align_stats;                                        /* 48 bytes */
int voe_map_align_dev(vo_map *dst, vo_map *src, const voe_map_align_params *params, float *d_S16_out,
                      int32_t *d_pairs_out /* [n_max][2] */, int *d_n_matches, uint8_t *d_inlier_mask /* [n_max] or NULL */,
                      int32_t *d_hypothesis_counts /* [n_hypotheses] or NULL */, voe_map_align_stats *d_stats);
/* host arrays: pairs_out [vo_map_size(src)][2], mask_out [vo_map_size(src)], counts_out [n_hypotheses], each or NULL.  The
 * device call and one read-back; the same results bit for bit. */
int voe_map_align(vo_map *dst, vo_map *src, const voe_map_align_params *params, float S16_out[16], int32_t *pairs_out,
                  int *n_matches_out, uint8_t *mask_out, int32_t *counts_out, voe_map_align_stats *stats_out);

/* MERGING.  src's entries into dst, moved by d_S16 (device, column-major 4x4, or NULL: as they are).  vo_map_update's transform
 * applies the 3x3 block exactly as given (p' = t + M p, no re-orthonormalisation), so a scaled rotation is applied as one: no
 * staging of transformed points is needed.  src keeps every byte.  n_max = voe_map_size_bound(src).
 *   VOE_MAP_MERGE_TAKE_SRC  the map afterwards is bit for bit what vo_map_update_dev(dst, src's points, src's appearances,
 *                           n_max, src's device size, d_S16) builds: a shared landmark takes src's (moved) point.
 *   VOE_MAP_MERGE_KEEP_DST  dst's existing entries keep every byte.  Only the src entries whose lookup in dst misses are
 *                           appended, in src order, moved (an entry whose appearance holds a NaN always misses, as in update):
 *                           the lookup with its entry output, a stable compaction of the misses (count / scan / scatter) into
 *                           a staging area, then vo_map_update_dev of those rows -- the result equals, bit for bit,
 *                           vo_map_update of those rows into dst.
 *   d_remap_out  [n_max] or NULL: the dst entry that src entry i is found at by a lookup AFTER the merge, or -1 (also beyond
 *                src's size).
 *   *d_stats     n_src, n_shared (src entries the lookup BEFORE the merge finds in dst), n_appended (the growth of dst),
 *                n_dst_after.
 * Growth and capture are those of vo_map_update_dev (dst grows on the host before anything is enqueued; a capture that would
 * have to grow dst or the workspaces is refused with VO_ERR_NOT_READY).  Refused (VO_ERR_INVALID_ARG): a null map, src == dst,
 * maps of different contexts, a policy other than the two, a null d_stats. */
#define VOE_MAP_MERGE_TAKE_SRC  0
#define VOE_MAP_MERGE_KEEP_DST  1
typedef struct voe_map_merge_stats { int32_t n_src, n_shared, n_appended, n_dst_after; } voe_map_merge_stats;      /* 16 bytes */
int voe_map_merge_dev(vo_map *dst, vo_map *src, const float *d_S16 /* or NULL */, int policy, int32_t *d_remap_out /* [n_max] or NULL */,
                      voe_map_merge_stats *d_stats);
/* S16: host, column-major, or NULL; remap_out [vo_map_size(src)] or NULL.  The device call and one read-back. */
int voe_map_merge(vo_map *dst, vo_map *src, const float S16[16], int policy, int32_t *remap_out, voe_map_merge_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_ALIGN_H */
