/* vo_map_grow.h -- a sixth extension of the map's interface (vo_hip.h, which includes this file): landmarks the map GAINS from
 * the frames it is asked to work on (voe_map_grow*).  The rows of a window of frames that find no entry are grouped into tracks
 * by equal appearance, every track is triangulated from all its rows at the given poses, and the tracks that pass the cull's
 * tests are appended.  Conventions, error codes, vo_map and vo_last_error are those of vo_hip.h; the namespace is the voe_ of
 * vo_map_cull.h, whose rule holds these symbols by itself: every exported voe_ function is declared in a header under include/
 * that vo_hip.h includes, every declared one is exported, all unversioned.  vo_abi_version() stays 1. */
#ifndef VO_MAP_GROW_H
#define VO_MAP_GROW_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GROWING.  Frames, pixels, appearances, d_n_rows, strides, K and d_T16 mean what they mean in vo_map_refine_batch_dev.
 * Enqueued on the context's stream; nothing is read back; no launch waits for another workgroup; the launches are a fixed
 * sequence that depends on n_frames, n_max and the parameters alone.  RULES:
 *   open row     a live row (frame f, position i) whose appearance holds no NaN and whose lookup in the map misses -- the
 *                lookup is vo_map_lookup_batch_dev with its entry output, bit for bit.  Its key is f * n_max + i.  Rows that
 *                hit the map, rows with a NaN appearance and rows behind the live rows are not open.
 *   track        a class of open rows whose ten appearance floats compare equal under operator== (-0 equals +0).  Tracks are
 *                numbered by ascending smallest key: the numbering a vo_map_update of all open rows, in key order, into an empty
 *                map would give its entries (and that is how it is made: a private table owned by the handle, filled by the
 *                update's own launches from a stable compaction of the open rows).  A track keeps the appearance bits of its
 *                first row.  Its observations are its rows in ascending key; two rows of one frame in one track are two
 *                observations.  n_obs is their number, n_frames the number of changes of key / n_max along the list, as in the
 *                cull.
 *   linear point for a track with n_obs >= min_obs and n_frames >= min_frames.  All sums in DOUBLE from the float32 inputs
 *                widened.  Per observation d = R^T K^-1 (u, v, 1) (K^-1: the adjugate over the determinant, in double, on the
 *                host; R, t as given), u = d / |d|, c = -R^T t; A = sum (I - u u^T), b = sum (I - u u^T) c: nine sums, taken as
 *                vo_map_refine takes its sums (observation k of the list in lane k mod 16, a lane's terms in ascending k, the 16
 *                lanes by the fixed tree: neighbour, other pair of the quad, mirrored half row, mirrored row).  p_lin = A^-1 b by
 *                refine's 3x3 LDL^T in natural order.
 *   refinement   n_rounds rounds of exactly vo_map_refine's per-landmark round (huber_px, damping), started at p_lin in double,
 *                not rounded first; as there, the last step is rounded to float32 and the cost that decides is that point's.
 *                The refined point is taken iff refine's own status for that landmark would be OK: every sum finite, camera
 *                z > 0 in every round, cost not risen; `refined` says so.  Otherwise, and with n_rounds == 0, p_lin stands.  The
 *                chosen point is rounded to float32 once.
 *   score        the float32 point widened again, under the cull's statistics with the cull's definitions and orders
 *                (vo_map_cull.h: n_obs, n_frames, mean_sq_px, max_sq_px, min_z, cos_parallax; the pairs visited only when
 *                min_parallax_deg > 0) -- computed by the device function that voe_map_cull runs, so that a dry-run cull of the
 *                grown map over the same frames reports the same bytes for every appended entry.
 *   verdict      per track, the first that matches:
 *                FEW_OBS       n_obs < min_obs
 *                FEW_FRAMES    n_frames < min_frames
 *                DEGENERATE    a sum of the linear system is not finite, some |d| is 0, or a pivot of A is not > 0
 *                NOT_FINITE, BEHIND, HIGH_ERROR, LOW_PARALLAX    exactly the cull's tests on the score, with max_rms_px,
 *                              max_err_px and min_parallax_deg (a threshold of 0 switches its test off)
 *                NO_ROOM       the track would be added, but max_added tracks before it, in track order, already are
 *                ADDED         otherwise
 *                Rays that are parallel only to within rounding give a tiny POSITIVE pivot and a far point, not DEGENERATE:
 *                it is the tests behind DEGENERATE that catch that case (LOW_PARALLAX when the parallax test is on, BEHIND or
 *                HIGH_ERROR when the far point lands wrongly); a caller who switches all three off gets such points added.
 *                The point and the four statistics of a FEW_OBS, FEW_FRAMES or DEGENERATE track are recorded as 0, 0, 0, 0
 *                and 1, `refined` as 0; of a NOT_FINITE track only n_obs and n_frames mean anything.
 *   effect       the ADDED tracks are compacted stably into a staging area -- float32 point and first-row appearance, in track
 *                order -- and appended by the launches of vo_map_update_dev.  The map afterwards is, bit for bit, the map that
 *                vo_map_update of those rows into the map before the call builds: the r-th ADDED track is entry
 *                n_before + r.  Existing entries, the history isometry and the count of rows dropped for lack of room keep
 *                every byte.
 *   dry_run      != 0: every output is written as it would be, the entries tracks WOULD get and n_after included; the map, its
 *                table and its header keep every byte.
 *   call status  in d_stats, the first that matches: NO_OPEN_ROWS; NOTHING_ADDED -- every byte of the map, its table and its
 *                header is left as read (the append's launches still run and return at once behind a flag on the device, as in
 *                the cull); OK -- something was added (or would be, under dry_run).
 *   room         max_added >= 0 is a host value; 0 means n_frames * n_max.  The map is grown on the host for max_added more
 *                entries before anything is enqueued (not under dry_run).  Under a graph capture the rule of vo_map_update_dev
 *                holds: the call is refused with VO_ERR_NOT_READY, before anything is enqueued, if the map or a workspace would
 *                have to grow; otherwise replays add entries the host never counts.  The host's bound of the size rises by
 *                max_added unless dry_run; the host form sets it to the true size after its read-back when no update of the map
 *                has been captured.  The call itself reads the map through the lookup alone and appends at the size the device
 *                holds, so no bound of the host clips it; a captured grow that adds makes the capacity the bound of every
 *                later call outside a capture, and a window call captured in the same graph is launched for the capacity
 *                wherever it stands (vo_hip.h, A CALL CAPTURED ON A MAP).
 *   determinism  no float atomics: calls from the same start give the same bytes in the map and in every output.
 * OUTPUTS.  d_row_out [n_frames][n_max] (or NULL): the entry the row is found at AFTER the call -- its hit, or its track's new
 * entry; -1 for a row that is not live or has a NaN appearance; -2 - t for an open row whose track t was not added.
 * d_track_out [track_cap] (or NULL, 8-byte aligned): the record of every track t < track_cap (first_key: its smallest key;
 * entry: the entry it got, or would get under dry_run, or -1).  *d_stats (8-byte aligned): whole numbers only -- n_live
 * rows, of which n_hits hit the map, n_nan hold a NaN and n_open are open; n_tracks; n_added; n_before and n_after, the map's
 * size before and (as it would be, under dry_run) after; by_verdict[12], tracks per verdict; reserved words written as 0.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_refine_batch_dev for the frames and the rounds, min_obs < 2,
 * min_frames < 2, a threshold negative or not finite, min_parallax_deg >= 180, negative max_added or track_cap, a non-null
 * d_track_out with track_cap == 0, a misaligned d_track_out or d_stats, a null d_stats or params. */
#define VOE_MAP_GROW_ADDED         0
#define VOE_MAP_GROW_FEW_OBS       1
#define VOE_MAP_GROW_FEW_FRAMES    2
#define VOE_MAP_GROW_DEGENERATE    3
#define VOE_MAP_GROW_NOT_FINITE    4
#define VOE_MAP_GROW_BEHIND        5
#define VOE_MAP_GROW_HIGH_ERROR    6
#define VOE_MAP_GROW_LOW_PARALLAX  7
#define VOE_MAP_GROW_NO_ROOM       8
#define VOE_MAP_GROW_OK             0   /* something was added (or would be, under dry_run) */
#define VOE_MAP_GROW_NO_OPEN_ROWS   1   /* every live row hits the map or holds a NaN */
#define VOE_MAP_GROW_NOTHING_ADDED  2   /* every byte of the map, its table and its header is left as read */
typedef struct voe_map_grow_params {
  int32_t n_rounds, min_obs, min_frames; float huber_px, damping, max_rms_px, max_err_px, min_parallax_deg; int32_t max_added, dry_run;
} voe_map_grow_params;
typedef struct voe_map_grow_track {
  int32_t verdict, n_obs, n_frames, entry, first_key, refined, reserved[2]; float xyz[3]; int32_t reserved2;
  double mean_sq_px, max_sq_px, min_z, cos_parallax;
} voe_map_grow_track;
typedef struct voe_map_grow_stats {
  int32_t status, n_live, n_hits, n_nan, n_open, n_tracks, n_added, n_before, n_after, by_verdict[12], reserved[3];
} voe_map_grow_stats;
int voe_map_grow_batch_dev(vo_map *m, int n_frames, const float K[9], const float *d_uv, size_t uv_stride, const float *d_app,
                           size_t app_stride, int n_max, const int *d_n_rows /* [n_frames] or NULL */,
                           const float *d_T16 /* [n_frames][16], p_cam = T p_map */, const voe_map_grow_params *params,
                           int32_t *d_row_out /* [n_frames][n_max] or NULL */, voe_map_grow_track *d_track_out /* [track_cap] or NULL */,
                           int track_cap, voe_map_grow_stats *d_stats);
/* host arrays as in vo_map_refine; row_out [n_frames][n_max] (or NULL), track_out [track_cap] (or NULL).  Uploads, the device
 * call, one read-back; the same results bit for bit. */
int voe_map_grow(vo_map *m, int n_frames, const float K[9], const float *uv, const float *app, const int *n_rows, int n_max,
                 const float *T16, const voe_map_grow_params *params, int32_t *row_out, voe_map_grow_track *track_out, int track_cap,
                 voe_map_grow_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_GROW_H */
