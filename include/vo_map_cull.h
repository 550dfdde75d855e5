/* vo_map_cull.h -- a third extension of the map's interface (vo_hip.h, which includes this file): landmarks taken OUT of the
 * map, judged from all their observations in a window of frames with known poses (voe_map_cull*).  Conventions, error codes,
 * vo_map and vo_last_error are those of vo_hip.h; the observations are those of vo_map_refine.
 *
 * A THIRD NAMESPACE, OPENED BY RULE.  vo_ is closed (vo_hip.h, vo_map_adjust.h) and so is vox_ (vo_map_bundle.h: exactly its
 * two calls).  Entry points added from here on are spelled voe_ (vo, extension).  The rule that holds them, whatever their
 * number: every exported voe_ function is declared in a header under include/ that vo_hip.h includes, every declared one is
 * exported, and all are exported unversioned.  They return the VO_* codes and set vo_last_error like every other call.
 * vo_abi_version() stays 1: nothing that existed has changed. */
#ifndef VO_MAP_CULL_H
#define VO_MAP_CULL_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CULLING.  Frames, pixels, appearances, d_n_rows, strides, K and d_T16 mean what they mean in vo_map_refine_batch_dev.
 * Enqueued on the context's stream; nothing is read back.  RULES:
 *   observation  exactly that of vo_map_refine: a live row (frame f, position i) whose lookup returns an entry; key
 *                f * n_max + i.  A landmark consumes its observations in ascending key; two rows of one frame that hit one
 *                entry are two observations.
 *   statistics   per landmark, all in DOUBLE from the float32 inputs widened:
 *                n_obs         the number of observations
 *                n_frames      the distinct frames: the changes of key / n_max along the ordered list
 *                mean_sq_px    the sum of |e|^2, e = proj(K, T p) - uv (p_cam = R p + t, q = K p_cam with the full K,
 *                              e = (q0 / q2, q1 / q2) - uv; no Huber, no gate), divided by n_obs.  The sum is taken as
 *                              vo_map_refine takes its sums: observation k of the list in lane k mod 16, a lane's terms in
 *                              ascending k, the 16 lanes by the fixed tree (neighbour, other pair of the quad, mirrored half
 *                              row, mirrored row).
 *                max_sq_px     the largest |e|^2
 *                min_z         the smallest camera z (p_cam's third entry)
 *                cos_parallax  the minimum over all pairs k < l of u_k . u_l, where u_k = d_k / |d_k| and d_k = R^T p_cam,k is
 *                              the ray in the map's frame, taken from the p_cam already computed -- not through a camera
 *                              centre, so that a pose that is not exactly orthonormal has one meaning.  |d_k| is the square
 *                              root of d.d summed x, y, z; the dot product is summed x, y, z.  With fewer than two
 *                              observations it is 1.  The pairs are visited only when the parallax test is on
 *                              (min_parallax_deg > 0); with the test off cos_parallax is 1 as well.
 *                Maxima and minima are exact in any order: mean_sq_px alone has an order.  A NaN in any term makes the
 *                landmark NOT_FINITE (below), whatever the order in which a maximum would have met it.
 *   verdict      per entry, the first that matches:
 *                UNSEEN        n_obs == 0 (every entry whose appearance holds a NaN is one: no lookup finds it)
 *                FEW_OBS       n_obs < min_obs
 *                FEW_FRAMES    n_frames < min_frames
 *                NOT_FINITE    a term of any statistic is not finite, or some |d_k| is 0
 *                BEHIND        min_z is not > 0
 *                HIGH_ERROR    max_rms_px > 0 and mean_sq_px > max_rms_px^2, or max_err_px > 0 and max_sq_px > max_err_px^2
 *                              (squares are compared: the thresholds, widened to double, are squared; no square root is taken)
 *                LOW_PARALLAX  min_parallax_deg > 0 and cos_parallax > cos_thr, cos_thr = cos(min_parallax_deg * pi / 180)
 *                              computed once on the host, in double
 *                KEPT          otherwise
 *                An UNSEEN entry stays unless drop_unseen != 0; every other verdict but KEPT drops.  A threshold of 0 switches
 *                its test off.  The statistics of an entry that is UNSEEN, FEW_OBS or FEW_FRAMES are recorded as computed (with no
 *                observation: 0, 0, 0 and 1); of a NOT_FINITE entry only n_obs and n_frames mean anything.
 *   effect       the survivors keep their relative order and their 12 + 40 bytes, bit for bit.  hdr[0] (the size) becomes the
 *                number kept; the base of the last update becomes the number kept and its row count 0 (there is no last
 *                update).  The count of rows dropped for lack of room and the history isometry are untouched.  The table is
 *                rebuilt from the survivors, which also clears the overflow markers, as growth does.  d_remap_out[j] is the
 *                new index of old entry j, or -1.  The map afterwards is a valid map for every call: it is the map that
 *                vo_map_update of the survivors, in order, into a cleared map would have built.
 *   dry_run      != 0: everything is computed and every output written, d_remap_out included, as it would be; the map, its
 *                table and its header keep every byte.
 *   call status  in d_stats: OK -- something was dropped (or would be, under dry_run); NOTHING_DROPPED -- every byte of the
 *                map, its table and its header is left as read.  The launches of a call are a fixed sequence whatever the
 *                data: under NOTHING_DROPPED and dry_run the staging copy, the copy back, the header update and the table's
 *                rebuild still run and return at once, guarded by a flag the scan wrote on the device (the rebuild is NOT
 *                idempotent -- which of two colliding classes takes which slot depends on scheduling -- so it is skipped,
 *                not repeated).  No launch waits for another workgroup.
 *   statistics   n_before, n_kept, n_obs (observations in all) and by_verdict[8] (entries per verdict).
 * d_verdict_out [old size] (or NULL), d_remap_out [old size] (or NULL), d_entry_out [old size] (or NULL, 8-byte aligned),
 * *d_stats (8-byte aligned).  "Old size" is the size the device holds when the call runs.
 * Nothing is read back, so the host's bound of the size stays what it was: it remains an upper bound.  The host form lowers
 * it to the number kept when no update of the map has been captured; it reads the size first and so fails with
 * VO_ERR_BAD_INDEX on a map that has dropped rows for lack of room, exactly as vo_map_refine does, while the _dev form works
 * on the entries such a map kept.
 * Capturable once a call of the same shape (n_frames, n_max) has sized the workspaces; a capture that would have to grow them
 * is refused (VO_ERR_NOT_READY) before anything is enqueued.  A captured cull is launched for the map's CAPACITY, not for the
 * host's bound of the moment (vo_hip.h, A CALL CAPTURED ON A MAP): in a graph { cull ; vo_map_update_dev } every replay judges
 * every entry the map holds when it runs, and the per-entry arrays need room for that size.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_refine_batch_dev for the frames, min_obs < 1, min_frames < 1, a
 * threshold negative or not finite, min_parallax_deg >= 180, a misaligned d_entry_out or d_stats. */
#define VOE_MAP_CULL_KEPT          0
#define VOE_MAP_CULL_UNSEEN        1
#define VOE_MAP_CULL_FEW_OBS       2
#define VOE_MAP_CULL_FEW_FRAMES    3
#define VOE_MAP_CULL_NOT_FINITE    4
#define VOE_MAP_CULL_BEHIND        5
#define VOE_MAP_CULL_HIGH_ERROR    6
#define VOE_MAP_CULL_LOW_PARALLAX  7
#define VOE_MAP_CULL_OK               0   /* something was dropped (or would be, under dry_run) */
#define VOE_MAP_CULL_NOTHING_DROPPED  1   /* every byte of the map, its table and its header is left as read */
typedef struct voe_map_cull_params {
  int32_t min_obs, min_frames; float max_rms_px, max_err_px, min_parallax_deg; int32_t drop_unseen, dry_run;
} voe_map_cull_params;
typedef struct voe_map_cull_entry {
  int32_t verdict, n_obs, n_frames, reserved; double mean_sq_px, max_sq_px, min_z, cos_parallax;
} voe_map_cull_entry;
typedef struct voe_map_cull_stats {
  int32_t status, n_before, n_kept, n_obs, by_verdict[8];
} voe_map_cull_stats;
int voe_map_cull_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                           size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                           const float *d_T16 /* [n_frames][16], p_cam = T p_map */, const voe_map_cull_params *params,
                           int32_t *d_verdict_out /* [old size] or NULL */, int32_t *d_remap_out /* [old size] or NULL */,
                           voe_map_cull_entry *d_entry_out /* [old size] or NULL */, voe_map_cull_stats *d_stats);
/* host arrays as in vo_map_refine; verdict_out, remap_out, entry_out [vo_map_size before the call] (or NULL).  Uploads, the
 * device call, one read-back; the same results bit for bit. */
int voe_map_cull(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows, int n_max,
                 const float *T16, const voe_map_cull_params *params, int32_t *verdict_out, int32_t *remap_out,
                 voe_map_cull_entry *entry_out, voe_map_cull_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_CULL_H */
