/* vo_map_covis.h -- a fifth extension of the map's interface (vo_hip.h, which includes this file): which frames belong
 * together.  How many map entries two frames both see (voe_map_covis*: the covisibility of frames) and, from it, the local
 * window of a frame -- the frames to free, the frames to hold, the landmarks between them (voe_map_window*).  Conventions, error
 * codes, vo_map and vo_last_error are those of vo_hip.h; the namespace is the voe_ of vo_map_cull.h, whose rule holds these
 * symbols by itself: every exported voe_ function is declared in a header under include/ that vo_hip.h includes, every declared
 * one is exported, all unversioned.  vo_abi_version() stays 1.  Every output of this header is an integer and EXACT: nothing here
 * has an order of summation, and no floating point number is formed. */
#ifndef VO_MAP_COVIS_H
#define VO_MAP_COVIS_H

#include "vo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* COVISIBILITY.  Frames, appearances, d_n_rows, app_stride and n_max mean what they mean in vo_map_lookup_batch_dev.
 * Enqueued on the context's stream; nothing is read back; the map is not written.  RULES:
 *   sees(f, e)   frame f has at least one live row whose lookup returns entry e.  The lookup is the public
 *                vo_map_lookup_batch_dev with its entry output: the hits are the lookup's, bit for bit.  Two rows of one frame
 *                that hit one entry see it ONCE -- this is not the observation of vo_map_refine, where they are two.  A row with
 *                a NaN appearance sees nothing; -0 equals +0; the rows behind the live rows see nothing.
 *   bits         d_bits_out [n_frames][n_words] uint32: bit (e & 31) of word (e >> 5) of row f is sees(f, e).  ALL n_words words
 *                of every row are written; every bit at or beyond the size the device holds is 0.  Rows are 4-byte aligned.
 *   counts       d_counts_out [n_frames][n_frames] int32 (or NULL): counts[f][g] is the number of entries e with sees(f, e) and
 *                sees(g, e).  The full matrix is written, both triangles; the diagonal is the number of entries frame f sees.
 *   statistics   n_frames; n_entries: the size the device holds; n_hits: the live rows that hit (two rows on one entry are two
 *                hits); n_seen: the sum of the diagonal; n_entries_seen: the entries seen by any frame; three reserved words,
 *                written as 0.  All are the same whether or not d_counts_out is given.
 * The launches of a call are a fixed sequence: they depend on n_frames, n_max, n_words and on whether counts are wanted, and on
 * nothing else.  No launch waits for another workgroup.
 * Capturable once a call of the same shape (n_frames, n_max, n_words) has sized the workspaces, which the map handle owns; a
 * capture that would have to grow them is refused (VO_ERR_NOT_READY) before anything is enqueued.
 * Refused (VO_ERR_INVALID_ARG): the refusals of vo_map_lookup_batch_dev for the frames; n_frames outside
 * 1 .. VOE_MAP_COVIS_MAX_FRAMES (the matrix is 64 MB there); n_words < 1; 32 * n_words < voe_map_size_bound(m); a null
 * d_bits_out or d_stats; a d_stats that is not 8-byte aligned. */
#define VOE_MAP_COVIS_MAX_FRAMES 4096
typedef struct voe_map_covis_stats {
  int32_t n_frames, n_entries, n_hits, n_seen, n_entries_seen, reserved[3];
} voe_map_covis_stats;
int voe_map_covis_batch_dev(vo_map *m, int n_frames, const float *d_app, size_t app_stride, int n_max,
                            const int *d_n_rows /* [n_frames] or NULL */, int n_words,
                            uint32_t *d_bits_out /* [n_frames][n_words] */, int32_t *d_counts_out /* [n_frames][n_frames] or NULL */,
                            voe_map_covis_stats *d_stats /* 8-byte aligned */);
/* host arrays: app [n_frames][n_max][10], n_rows [n_frames] (or NULL), bits_out [n_frames][n_words], counts_out (or NULL).  Reads
 * the size first and so fails with VO_ERR_BAD_INDEX on a map that has dropped rows for lack of room, exactly as vo_map_refine
 * does, while the _dev form works on the entries such a map kept.  Uploads, the device call, one read-back; the same bytes. */
int voe_map_covis(vo_map *m, int n_frames, const float *app, const int *n_rows, int n_max, int n_words, uint32_t *bits_out,
                  int32_t *counts_out, voe_map_covis_stats *stats_out);

/* WINDOW.  Reads the bit rows ALONE (those of voe_map_covis*, or any other): the map is there for the stream and for the
 * workspaces.  The row of the covisibility matrix it needs, it counts itself.  With c(g) the number of common bits of rows
 * `query` and g, RULES:
 *   candidates   the frames g != query with c(g) >= min_shared
 *   free         query, then the first k_free - 1 candidates in the order (c descending, g ascending)
 *   union        U, the OR of the free frames' rows: the landmarks of the window.  d_union_out [n_words] (or NULL) receives it.
 *   fixed        s(h) is the number of common bits of row h and U.  The fixed candidates are the frames h that are not free and
 *                have s(h) >= min_shared; the fixed frames are the first k_fixed of them in the order (s descending, h ascending).
 *   roles        d_role_out [n_frames]: VOE_MAP_WINDOW_OUTSIDE, _FREE or _FIXED
 *   n_rows_out   d_n_rows_out [n_frames]: the frame's live rows (d_n_rows[f], or n_max) for FREE and FIXED frames, 0 for OUTSIDE
 *   fixed_out    d_fixed_out [n_frames] bytes: 0 for FREE and 1 otherwise
 *   order        d_order_out [n_frames] (or NULL): the free frames in rank order with query first, then the fixed frames in rank
 *                order, then -1
 *   status       the first that holds: QUERY_UNSEEN -- row query is empty: every frame is OUTSIDE and n_free is 0; NO_FIXED --
 *                n_fixed == 0: a bundle on this window has a free gauge, the roles are as computed; OK.  The call returns VO_OK
 *                in all three cases.
 *   statistics   status, n_free, n_fixed, n_candidates, n_fixed_candidates; n_points: the population count of U; query_seen:
 *                that of row query; one reserved word, written as 0.
 * d_n_rows_out and d_fixed_out plug straight into vox_map_bundle_batch_dev, vo_map_adjust_batch_dev and voe_map_cull_batch_dev
 * over the SAME frame arrays, with no gather: a frame with 0 live rows has no observation, and a held frame is a constant.
 * Mind two things.  A FIXED frame brings in ALL of its own hits, not only those in U, so landmarks outside U can be free points
 * of such a bundle.  And `query` (like the rest of params) is a host value, read when the call is made: a captured call keeps it.
 * The launches are a fixed sequence that depends on n_frames and n_words alone; no launch waits for another workgroup; nothing
 * is read back.  Capturable once a call of the same shape (n_frames, n_words) on this map has sized the workspace.
 * Refused (VO_ERR_INVALID_ARG): query outside the frames; k_free outside 1 .. n_frames; k_fixed outside 0 .. n_frames;
 * min_shared < 1; n_frames outside 1 .. VOE_MAP_COVIS_MAX_FRAMES; n_words < 1; n_max < 0; a null d_bits, params, d_role_out,
 * d_n_rows_out, d_fixed_out or d_stats; a d_stats that is not 8-byte aligned. */
#define VOE_MAP_WINDOW_OUTSIDE       0
#define VOE_MAP_WINDOW_FREE          1
#define VOE_MAP_WINDOW_FIXED         2
#define VOE_MAP_WINDOW_OK            0
#define VOE_MAP_WINDOW_NO_FIXED      1   /* no frame is held: a bundle on this window has a free gauge */
#define VOE_MAP_WINDOW_QUERY_UNSEEN  2   /* row query is empty: every frame is OUTSIDE */
typedef struct voe_map_window_params { int32_t query, k_free, k_fixed, min_shared; } voe_map_window_params;
typedef struct voe_map_window_stats {
  int32_t status, n_free, n_fixed, n_candidates, n_fixed_candidates, n_points, query_seen, reserved;
} voe_map_window_stats;
int voe_map_window_dev(vo_map *m, int n_frames, int n_words, const uint32_t *d_bits, const int *d_n_rows /* [n_frames] or NULL */,
                       int n_max, const voe_map_window_params *params, int32_t *d_role_out /* [n_frames] */,
                       int *d_n_rows_out /* [n_frames] */, uint8_t *d_fixed_out /* [n_frames] */,
                       int32_t *d_order_out /* [n_frames] or NULL */, uint32_t *d_union_out /* [n_words] or NULL */,
                       voe_map_window_stats *d_stats /* 8-byte aligned */);
/* host arrays (order_out and union_out may be NULL).  Uploads, the device call, one read-back; the same bytes. */
int voe_map_window(vo_map *m, int n_frames, int n_words, const uint32_t *bits, const int *n_rows, int n_max,
                   const voe_map_window_params *params, int32_t *role_out, int *n_rows_out, uint8_t *fixed_out, int32_t *order_out,
                   uint32_t *union_out, voe_map_window_stats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* VO_MAP_COVIS_H */
