// map_checks.h -- refusals of the host path that make no HIP call and touch neither context nor map: plain C++, so that
// tests/hostcheck/map_checks_check.cpp compiles them with the host sanitizers and nothing else of the library.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <initializer_list>

#include "../../include/vo_hip.h"

int vo_fail(int code, const char* fmt, ...);   // vo_internal.h

// device arrays move as 8-byte pieces (vo_hip.h, Conventions): true when every pointer given is null or on such a boundary
template <typename... P>
static bool aligned8(const P*... p) { return ((... | reinterpret_cast<uintptr_t>(p)) & 7u) == 0; }

// K^-1 in double of the float K (column-major in, column-major out): adjugate / determinant; false when K is singular
static inline bool invert_k(const float K[9], double Kinv[9]) {
  double k[9];
  for (int i = 0; i < 9; ++i) k[i] = K[i];
#define VO_K(r, c) k[(r) + 3 * (c)]
  const double c00 = VO_K(1, 1) * VO_K(2, 2) - VO_K(1, 2) * VO_K(2, 1), c01 = VO_K(1, 2) * VO_K(2, 0) - VO_K(1, 0) * VO_K(2, 2),
               c02 = VO_K(1, 0) * VO_K(2, 1) - VO_K(1, 1) * VO_K(2, 0);
  const double det = VO_K(0, 0) * c00 + VO_K(0, 1) * c01 + VO_K(0, 2) * c02;
  if (!(det != 0.0) || !std::isfinite(det)) return false;
  // inverse = adjugate / det, column-major: Kinv(r, c) = cofactor(c, r) / det
  Kinv[0 + 3 * 0] = c00 / det;
  Kinv[1 + 3 * 0] = c01 / det;
  Kinv[2 + 3 * 0] = c02 / det;
  Kinv[0 + 3 * 1] = (VO_K(0, 2) * VO_K(2, 1) - VO_K(0, 1) * VO_K(2, 2)) / det;
  Kinv[1 + 3 * 1] = (VO_K(0, 0) * VO_K(2, 2) - VO_K(0, 2) * VO_K(2, 0)) / det;
  Kinv[2 + 3 * 1] = (VO_K(0, 1) * VO_K(2, 0) - VO_K(0, 0) * VO_K(2, 1)) / det;
  Kinv[0 + 3 * 2] = (VO_K(0, 1) * VO_K(1, 2) - VO_K(0, 2) * VO_K(1, 1)) / det;
  Kinv[1 + 3 * 2] = (VO_K(0, 2) * VO_K(1, 0) - VO_K(0, 0) * VO_K(1, 2)) / det;
  Kinv[2 + 3 * 2] = (VO_K(0, 0) * VO_K(1, 1) - VO_K(0, 1) * VO_K(1, 0)) / det;
#undef VO_K
  return true;
}

// a window of frames as every *_batch_dev call of the map takes it (vo_hip.h, vo_map_refine_batch_dev): frame g's pixels
// start at d_uv + 2 * g * uv_stride, its appearances at d_app + 10 * g * app_stride; d_n (or null) holds the live rows
struct MapFrames {
  int n_frames;
  const float* K;             // [9] column-major; null where the call has no camera (the covisibility)
  const float* d_uv; size_t uv_stride; const float* d_app; size_t app_stride;
  int n_max; const int* d_n;
};

// what a call that iterates is asked to do, and the limits of that call
struct MapRounds {
  int n_rounds, most_rounds, min_obs, least_obs;
  float huber_px; const float* damping;       // (null: the call has no damping)
};

static inline int map_rounds_check(const char* fn, const MapRounds& r) {
  if (r.n_rounds < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative n_rounds", fn);
  if (r.n_rounds > r.most_rounds) return vo_fail(VO_ERR_INVALID_ARG, "%s: more than %d rounds", fn, r.most_rounds);
  if (r.min_obs < r.least_obs) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_obs must be at least %d", fn, r.least_obs);
  if (!(r.huber_px >= 0.f && r.huber_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: huber_px must be finite and not negative", fn);
  if (r.damping && !(*r.damping >= 0.f && *r.damping <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: damping must be finite and not negative", fn);
  return VO_OK;
}

// The refusals the window calls share (refinement, pose refinement, adjustment, bundle, culling), in the order they fire:
//   1. n_frames outside 1 .. 65535      2. negative n_max          3. null pixels or appearances with n_max > 0
//   4. d_uv, d_app or d_stats not on an 8-byte boundary            5. a stride below n_max     6. uv_stride >= 2^31 - 1
//   7. the round parameters of the call (map_rounds_check), where it has any
//   8. a singular K                     9. app_stride >= (2^31 - 1) / 10 or more than 2^30 rows (the lookup's own limit, met
//                                          before anything is sized)
// Where two would fail, the first is the one reported.
static inline int map_frames_check(const char* fn, const MapFrames& f, const void* d_stats, const MapRounds* rounds = nullptr) {
  if (f.n_frames < 1 || f.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, f.n_frames);
  if (f.n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (f.n_max > 0 && !(f.d_uv && f.d_app)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(f.d_uv, f.d_app, d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  if (f.uv_stride < (size_t)f.n_max || f.app_stride < (size_t)f.n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: a stride is smaller than n_max", fn);
  if (f.uv_stride >= 0x7fffffff) return vo_fail(VO_ERR_INVALID_ARG, "%s: stride too large", fn);
  if (rounds)
    if (int r = map_rounds_check(fn, *rounds)) return r;
  double Kinv[9];
  if (!invert_k(f.K, Kinv)) return vo_fail(VO_ERR_INVALID_ARG, "%s: K is singular", fn);
  if (f.app_stride >= 0x7fffffff / 10 || (long long)f.n_max * f.n_frames > (1ll << 30))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  return VO_OK;
}

// voe_map_grow*: what the call refuses beyond the frames and the rounds (include/vo_map_grow.h), in the order they fire:
//   1. min_frames < 2 (min_obs < 2 is the rounds' refusal)          2. a threshold negative or not finite, min_parallax_deg >= 180
//   3. negative max_added or track_cap        4. a track array with track_cap == 0        5. a track array off an 8-byte boundary
static inline int map_grow_check(const char* fn, const voe_map_grow_params* p, const void* d_track_out, int track_cap) {
  if (p->min_frames < 2) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_frames must be at least 2", fn);
  if (!(p->max_rms_px >= 0.f && p->max_rms_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_rms_px must be finite and not negative", fn);
  if (!(p->max_err_px >= 0.f && p->max_err_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_err_px must be finite and not negative", fn);
  if (!(p->min_parallax_deg >= 0.f && p->min_parallax_deg < 180.f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_parallax_deg must be in [0, 180)", fn);
  if (p->max_added < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative max_added", fn);
  if (track_cap < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative track_cap", fn);
  if (d_track_out && track_cap == 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: a track array with track_cap == 0", fn);
  if (!aligned8(d_track_out)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_track_out must be 8-byte aligned", fn);
  return VO_OK;
}
// the tracks the call may add: max_added, or with 0 every row of the window (at least 1: it sizes arrays)
static inline int map_grow_room(const voe_map_grow_params* p, int n_frames, int n_max) {
  const long long rows = (long long)n_frames * n_max;
  const long long a = p->max_added > 0 ? p->max_added : rows;
  return (int)(a > 0 ? a : 1);
}

// voe_pose_graph*: what the call refuses (include/vo_pose_graph.h), in the order they fire:
//   1. a null d_S16, params or d_stats      2. n_frames < 1 or negative n_edges      3. null edges or measurements with n_edges > 0
//   4. a float32 / int32 array off a 4-byte boundary, the edge costs, the rounds' records or d_stats off an 8-byte one
//   5. negative n_rounds, n_cg < 1      6. cg_tol, lambda0 or huber negative or not finite      7. too many steps
//   8. an unknown preconditioner
struct PoseGraphPtrs {
  const void *S16, *edges, *Z16, *weights, *edge_status, *edge_cost, *rounds, *stats;
};
static inline int pose_graph_check(const char* fn, int n_frames, int n_edges, const PoseGraphPtrs& d, const voe_pose_graph_params* p) {
  if (!(d.S16 && p && d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_frames < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames must be at least 1", fn);
  if (n_edges < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative n_edges", fn);
  if (n_frames > (1 << 24) || n_edges > (1 << 24)) return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^24 frames or edges", fn);
  if (n_edges > 0 && !(d.edges && d.Z16)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null edges or measurements", fn);
  const uintptr_t four = reinterpret_cast<uintptr_t>(d.S16) | reinterpret_cast<uintptr_t>(d.edges) | reinterpret_cast<uintptr_t>(d.Z16) |
                         reinterpret_cast<uintptr_t>(d.weights) | reinterpret_cast<uintptr_t>(d.edge_status);
  if (four & 3u) return vo_fail(VO_ERR_INVALID_ARG, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
  if (!aligned8(d.edge_cost, d.rounds, d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_edge_cost_out, d_rounds_out and d_stats must be 8-byte aligned", fn);
  if (p->n_rounds < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative n_rounds", fn);
  if (p->n_cg < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_cg must be at least 1", fn);
  if (!(p->cg_tol >= 0.f && p->cg_tol <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: cg_tol must be finite and not negative", fn);
  if (!(p->lambda0 >= 0.f && p->lambda0 <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: lambda0 must be finite and not negative", fn);
  if (!(p->huber >= 0.f && p->huber <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: huber must be finite and not negative", fn);
  if ((long long)p->n_rounds * ((long long)p->n_cg + 2) > VOE_POSE_GRAPH_MAX_STEPS)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_rounds * (n_cg + 2) above %d (the launches of a call are a fixed sequence)", fn, VOE_POSE_GRAPH_MAX_STEPS);
  if (p->preconditioner != VOE_POSE_GRAPH_CHAIN && p->preconditioner != VOE_POSE_GRAPH_JACOBI)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: unknown preconditioner %d", fn, p->preconditioner);
  return VO_OK;
}

// voe_map_apply_correction*: what the call refuses (include/vo_pose_graph.h), in the order they fire:
//   1. a null matrix array or d_stats      2. n_frames outside 1 .. 65535, negative n_max      3. null appearances with n_max > 0
//   4. d_app or d_stats off an 8-byte boundary, a matrix array or d_ref_frame_out off a 4-byte one      5. app_stride < n_max
//   6. app_stride >= (2^31 - 1) / 10 or more than 2^30 rows
static inline int map_apply_check(const char* fn, int n_frames, const float* d_app, size_t app_stride, int n_max, const float* d_S16_old,
                                  const float* d_S16_new, const void* d_ref_frame_out, const void* d_stats) {
  if (!(d_S16_old && d_S16_new && d_stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_frames < 1 || n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, n_frames);
  if (n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (n_max > 0 && !d_app) return vo_fail(VO_ERR_INVALID_ARG, "%s: null appearances", fn);
  if (!aligned8(d_app) || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device arrays must be 8-byte aligned", fn);
  if ((reinterpret_cast<uintptr_t>(d_S16_old) | reinterpret_cast<uintptr_t>(d_S16_new) | reinterpret_cast<uintptr_t>(d_ref_frame_out)) & 3u)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: the matrices and d_ref_frame_out must be 4-byte aligned", fn);
  if (app_stride < (size_t)n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: a stride is smaller than n_max", fn);
  if (app_stride >= 0x7fffffff / 10 || (long long)n_max * n_frames > (1ll << 30))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  return VO_OK;
}

// voe_map_loops*: what the call refuses beyond the lookup's, the localisation's and the covisibility's own refusals
// (include/vo_map_loops.h), in the order they fire:
//   1. a null d_S16, params or output      2. n_frames outside 1 .. VOE_MAP_COVIS_MAX_FRAMES
//   3. d_loops_out or d_stats off an 8-byte boundary, any other array off a 4-byte one
//   4. gap < 0      5. ref_window < 0      6. min_shared < 1      7. separation < 0      8. max_loops outside 1 .. n_frames
//   9. a w_loop that is negative or not finite      10. w_loop all zero
struct MapLoopsPtrs {
  const void *S16, *edges, *Z16, *weights, *loops, *hist, *ref_frame, *stats;
};
static inline int map_loops_check(const char* fn, int n_frames, const MapLoopsPtrs& d, const voe_map_loops_params* p) {
  if (!(d.S16 && p && d.edges && d.Z16 && d.weights && d.loops && d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_frames < 1 || n_frames > VOE_MAP_COVIS_MAX_FRAMES)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. %d", fn, n_frames, VOE_MAP_COVIS_MAX_FRAMES);
  if (!aligned8(d.loops, d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_loops_out and d_stats must be 8-byte aligned", fn);
  const uintptr_t four = reinterpret_cast<uintptr_t>(d.S16) | reinterpret_cast<uintptr_t>(d.edges) | reinterpret_cast<uintptr_t>(d.Z16) |
                         reinterpret_cast<uintptr_t>(d.weights) | reinterpret_cast<uintptr_t>(d.hist) | reinterpret_cast<uintptr_t>(d.ref_frame);
  if (four & 3u) return vo_fail(VO_ERR_INVALID_ARG, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
  if (p->gap < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative gap", fn);
  if (p->ref_window < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative ref_window", fn);
  if (p->min_shared < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_shared must be at least 1", fn);
  if (p->separation < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative separation", fn);
  if (p->max_loops < 1 || p->max_loops > n_frames) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_loops %d outside 1 .. n_frames", fn, p->max_loops);
  bool any = false;
  for (int k = 0; k < 3; ++k) {
    if (!(p->w_loop[k] >= 0.f && p->w_loop[k] <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: w_loop must be finite and not negative", fn);
    any = any || p->w_loop[k] > 0.f;
  }
  if (!any) return vo_fail(VO_ERR_INVALID_ARG, "%s: w_loop is all zero", fn);
  return VO_OK;
}

// voe_map_nearest*: what the call refuses (include/vo_hip.h, NEAREST), in the order they fire.  1 - 6 are the lookup's refusals
// for the frames, word for word:
//   1. n_frames outside 1 .. 65535      2. negative n_max      3. null appearances with n_max > 0
//   4. appearance rows off an 8-byte boundary      5. app_stride < n_max (more than one frame)
//   6. app_stride >= (2^31 - 1) / 10 or more than 2^30 rows
//   7. a null params or d_entry_out     8. a radius that is not finite or <= 0      9. a ratio that is not finite or outside {0} u (0, 1]
//   10. unique outside 0 / 1            11. reserved != 0
//   12. an int32 / float32 output off a 4-byte boundary, d_app_out or d_stats off an 8-byte one
//   13. d_app_out overlapping d_app without being d_app (the frames span 10 * ((n_frames - 1) * app_stride + n_max) floats)
struct MapNearestPtrs {
  const void *entry, *status, *dist2, *app_out, *stats;
};
static inline int map_nearest_check(const char* fn, const MapFrames& f, const voe_map_nearest_params* p, const MapNearestPtrs& d) {
  if (f.n_frames < 1 || f.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, f.n_frames);
  if (f.n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (f.n_max > 0 && !f.d_app) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(f.d_app)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device appearance rows must be 8-byte aligned", fn);
  if (f.n_frames > 1 && f.app_stride < (size_t)f.n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: app_stride %zu is smaller than n_max %d", fn, f.app_stride, f.n_max);
  if (f.app_stride >= 0x7fffffff / 10 || (long long)f.n_max * f.n_frames > (1ll << 30))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  if (!p || !d.entry) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or d_entry_out", fn);
  if (!(p->radius > 0.f && p->radius <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: radius must be finite and positive", fn);
  if (!(p->ratio >= 0.f && p->ratio <= 1.f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: ratio must be 0 (off) or in (0, 1]", fn);
  if (p->unique != 0 && p->unique != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: unique must be 0 or 1", fn);
  if (p->reserved != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: reserved must be 0", fn);
  if ((reinterpret_cast<uintptr_t>(d.entry) | reinterpret_cast<uintptr_t>(d.status) | reinterpret_cast<uintptr_t>(d.dist2)) & 3u)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: int32 and float32 arrays must be 4-byte aligned", fn);
  if (!aligned8(d.app_out, d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out and d_stats must be 8-byte aligned", fn);
  if (d.app_out && d.app_out != (const void*)f.d_app && f.n_max > 0) {
    const uintptr_t span = sizeof(float) * 10 * ((uintptr_t)(f.n_frames - 1) * f.app_stride + (uintptr_t)f.n_max);
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.d_app), b = reinterpret_cast<uintptr_t>(d.app_out);
    if (a < b + span && b < a + span) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out overlaps d_app without being d_app", fn);
  }
  return VO_OK;
}

// voe_map_guided*: what the call refuses (include/vo_hip.h, GUIDED), in the order they fire.  1 - 6 are the lookup's refusals for
// the frames as map_nearest_check states them (3 and 4 now also for the pixels); `f` carries K, d_uv and both strides:
//   1. n_frames outside 1 .. 65535      2. negative n_max      3. null appearances or pixels with n_max > 0
//   4. appearance rows or pixels off an 8-byte boundary      5. app_stride or uv_stride < n_max
//   6. app_stride >= (2^31 - 1) / 10, uv_stride >= 2^31 - 1 or more than 2^30 rows
//   7. a null params, d_entry_out, d_T16 or K      8. radius_px, then radius, not finite or <= 0
//   9. a ratio that is not finite or outside {0} u (0, 1]      10. unique outside 0 / 1      11. z_far < z_near
//   12. reserved != 0      13. an int32 / float32 array (the poses among them) off a 4-byte boundary, d_app_out or d_stats off an
//   8-byte one      14. d_app_out overlapping d_app without being d_app
struct MapGuidedPtrs {
  const void *T16, *entry, *status, *dist2, *pix2, *app_out, *stats;
};
static inline int map_guided_check(const char* fn, const MapFrames& f, const voe_map_guided_params* p, const MapGuidedPtrs& d) {
  if (f.n_frames < 1 || f.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, f.n_frames);
  if (f.n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (f.n_max > 0 && !(f.d_app && f.d_uv)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (!aligned8(f.d_app, f.d_uv)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device appearance rows and pixels must be 8-byte aligned", fn);
  if (f.app_stride < (size_t)f.n_max || f.uv_stride < (size_t)f.n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: a stride is smaller than n_max %d", fn, f.n_max);
  if (f.app_stride >= 0x7fffffff / 10 || f.uv_stride >= 0x7fffffff || (long long)f.n_max * f.n_frames > (1ll << 30))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  if (!p || !d.entry || !d.T16 || !f.K) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params, d_entry_out, d_T16 or K", fn);
  if (!(p->radius_px > 0.f && p->radius_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: radius_px must be finite and positive", fn);
  if (!(p->radius > 0.f && p->radius <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: radius must be finite and positive", fn);
  if (!(p->ratio >= 0.f && p->ratio <= 1.f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: ratio must be 0 (off) or in (0, 1]", fn);
  if (p->unique != 0 && p->unique != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: unique must be 0 or 1", fn);
  if (p->z_far < p->z_near) return vo_fail(VO_ERR_INVALID_ARG, "%s: z_far is below z_near", fn);
  if (p->reserved[0] != 0 || p->reserved[1] != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: reserved must be 0", fn);
  if ((reinterpret_cast<uintptr_t>(d.T16) | reinterpret_cast<uintptr_t>(d.entry) | reinterpret_cast<uintptr_t>(d.status) |
       reinterpret_cast<uintptr_t>(d.dist2) | reinterpret_cast<uintptr_t>(d.pix2)) & 3u)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: int32 and float32 arrays must be 4-byte aligned", fn);
  if (!aligned8(d.app_out, d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out and d_stats must be 8-byte aligned", fn);
  if (d.app_out && d.app_out != (const void*)f.d_app && f.n_max > 0) {
    const uintptr_t span = sizeof(float) * 10 * ((uintptr_t)(f.n_frames - 1) * f.app_stride + (uintptr_t)f.n_max);
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.d_app), b = reinterpret_cast<uintptr_t>(d.app_out);
    if (a < b + span && b < a + span) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out overlaps d_app without being d_app", fn);
  }
  return VO_OK;
}

// voe_map_fuse*: what the call refuses (include/vo_hip.h, FUSE), in the order they fire.  Frames are GIVEN when n_frames != 0 or
// d_app or d_n is not null; 1 - 6 are then the lookup's refusals for them as map_nearest_check states them:
//   1. n_frames outside 1 .. 65535      2. negative n_max      3. null appearances with n_max > 0
//   4. appearance rows off an 8-byte boundary      5. app_stride < n_max (more than one frame)
//   6. app_stride >= (2^31 - 1) / 10 or more than 2^30 rows
//   7. a null params or d_stats      8. radius_xyz, then radius, not finite or <= 0
//   9. position, then veto_shared_frame, then dry_run outside 0 / 1      10. reserved != 0
//   11. veto_shared_frame, then d_app_out, without frames
//   12. an int32 / float32 output off a 4-byte boundary, d_app_out or d_stats off an 8-byte one
//   13. d_app_out overlapping d_app without being d_app
struct MapFusePtrs {
  const void *partner, *dist2, *gap2, *verdict, *remap, *app_out, *stats;
};
static inline bool map_fuse_has_frames(const MapFrames& f) { return f.n_frames != 0 || f.d_app || f.d_n; }
static inline int map_fuse_check(const char* fn, const MapFrames& f, const voe_map_fuse_params* p, const MapFusePtrs& d) {
  const bool frames = map_fuse_has_frames(f);
  if (frames) {
    if (f.n_frames < 1 || f.n_frames > 65535) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. 65535 (the frame is a grid dimension)", fn, f.n_frames);
    if (f.n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
    if (f.n_max > 0 && !f.d_app) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
    if (!aligned8(f.d_app)) return vo_fail(VO_ERR_INVALID_ARG, "%s: device appearance rows must be 8-byte aligned", fn);
    if (f.n_frames > 1 && f.app_stride < (size_t)f.n_max) return vo_fail(VO_ERR_INVALID_ARG, "%s: app_stride %zu is smaller than n_max %d", fn, f.app_stride, f.n_max);
    if (f.app_stride >= 0x7fffffff / 10 || (long long)f.n_max * f.n_frames > (1ll << 30))
      return vo_fail(VO_ERR_INVALID_ARG, "%s: more than 2^30 rows in one call", fn);
  }
  if (!p || !d.stats) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or d_stats", fn);
  if (!(p->radius_xyz > 0.f && p->radius_xyz <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: radius_xyz must be finite and positive", fn);
  if (!(p->radius > 0.f && p->radius <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: radius must be finite and positive", fn);
  if (p->position != 0 && p->position != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: position must be 0 or 1", fn);
  if (p->veto_shared_frame != 0 && p->veto_shared_frame != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: veto_shared_frame must be 0 or 1", fn);
  if (p->dry_run != 0 && p->dry_run != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: dry_run must be 0 or 1", fn);
  if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: reserved must be 0", fn);
  if (!frames && p->veto_shared_frame != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: veto_shared_frame without frames", fn);
  if (!frames && d.app_out) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out without frames", fn);
  if ((reinterpret_cast<uintptr_t>(d.partner) | reinterpret_cast<uintptr_t>(d.dist2) | reinterpret_cast<uintptr_t>(d.gap2) |
       reinterpret_cast<uintptr_t>(d.verdict) | reinterpret_cast<uintptr_t>(d.remap)) & 3u)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: int32 and float32 arrays must be 4-byte aligned", fn);
  if (!aligned8(d.app_out, d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out and d_stats must be 8-byte aligned", fn);
  if (d.app_out && d.app_out != (const void*)f.d_app && f.n_max > 0) {
    const uintptr_t span = sizeof(float) * 10 * ((uintptr_t)(f.n_frames - 1) * f.app_stride + (uintptr_t)f.n_max);
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.d_app), b = reinterpret_cast<uintptr_t>(d.app_out);
    if (a < b + span && b < a + span) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out overlaps d_app without being d_app", fn);
  }
  return VO_OK;
}

// voe_map_keyframes*: what the call refuses (include/vo_hip.h, KEYFRAMES), in the order they fire.  1 - 5 are the window's
// refusals for the shape and the pointers, word for word:
//   1. n_frames outside 1 .. VOE_MAP_COVIS_MAX_FRAMES      2. n_words < 1      3. a null d_bits or d_stats
//   4. (device pointers) d_stats off an 8-byte boundary      5. a null params or required output, negative n_max
//   6. n_words above 2^26      7. min_observers < 1      8. share_permille outside 0 .. 1000      9. min_seen < 1
//   10. max_gap < 0      11. max_dropped outside 0 .. VOE_MAP_KEYFRAMES_MAX_STEPS      12. reserved != 0
//   13. (device pointers) an int32 array off a 4-byte boundary      14. (host arrays) a flag byte above 2
struct MapKeyframesPtrs {
  const void *bits, *verdict, *n_rows, *keep, *step, *order, *seen, *red, *stats;
};
static inline int map_keyframes_check(const char* fn, int n_frames, int n_words, int n_max, const uint8_t* host_flags,
                                      const voe_map_keyframes_params* p, const MapKeyframesPtrs& d, bool dev) {
  if (n_frames < 1 || n_frames > VOE_MAP_COVIS_MAX_FRAMES)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: n_frames %d outside 1 .. %d", fn, n_frames, VOE_MAP_COVIS_MAX_FRAMES);
  if (n_words < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_words must be at least 1", fn);
  if (!d.bits || !d.stats) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (dev && !aligned8(d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_stats must be 8-byte aligned", fn);
  if (!(p && d.verdict && d.n_rows && d.keep && d.step && d.seen && d.red)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (n_max < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative row count", fn);
  if (n_words > (1 << 26)) return vo_fail(VO_ERR_INVALID_ARG, "%s: n_words %d above 2^26", fn, n_words);
  if (p->min_observers < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_observers must be at least 1", fn);
  if (p->share_permille < 0 || p->share_permille > 1000) return vo_fail(VO_ERR_INVALID_ARG, "%s: share_permille %d outside 0 .. 1000", fn, p->share_permille);
  if (p->min_seen < 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: min_seen must be at least 1", fn);
  if (p->max_gap < 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: negative max_gap", fn);
  if (p->max_dropped < 0 || p->max_dropped > VOE_MAP_KEYFRAMES_MAX_STEPS)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: max_dropped %d outside 0 .. %d", fn, p->max_dropped, VOE_MAP_KEYFRAMES_MAX_STEPS);
  if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: reserved must be 0", fn);
  if (dev && ((reinterpret_cast<uintptr_t>(d.bits) | reinterpret_cast<uintptr_t>(d.verdict) | reinterpret_cast<uintptr_t>(d.n_rows) |
               reinterpret_cast<uintptr_t>(d.step) | reinterpret_cast<uintptr_t>(d.order) | reinterpret_cast<uintptr_t>(d.seen) |
               reinterpret_cast<uintptr_t>(d.red)) & 3u))
    return vo_fail(VO_ERR_INVALID_ARG, "%s: int32 arrays must be 4-byte aligned", fn);
  if (host_flags)
    for (int f = 0; f < n_frames; ++f)
      if (host_flags[f] > VOE_MAP_KEYFRAMES_GONE) return vo_fail(VO_ERR_INVALID_ARG, "%s: flag %d of frame %d is none of FREE, PROTECTED, GONE", fn, host_flags[f], f);
  return VO_OK;
}

// voe_map_prune*: what the call refuses (include/vo_hip.h, PRUNE), in the order they fire.  1 and 2 are the cull's refusals:
//   1. a null K, d_T16 or d_stats      2. the frames' (map_frames_check)      3. a null params or d_entry_out
//   4. max_err_px, then rel_factor, then rel_floor_px negative or not finite      5. rel_min_obs < 3
//   6. max_share_landmark, then max_share_frame, outside 0 .. 1000      7. unique outside 0 / 1      8. reserved != 0
//   9. an int32 output off a 4-byte boundary; d_sq_out, d_app_out, d_landmark_out or d_frame_out off an 8-byte one
//   10. d_app_out overlapping d_app without being d_app
// All tests off (max_err_px == 0, rel_factor == 0, unique == 0) is NOT refused: rule 3 still runs.
struct MapPrunePtrs {
  const void *T16, *entry, *status, *sq, *app_out, *landmark, *frame, *stats;
};
static inline int map_prune_check(const char* fn, const MapFrames& f, const voe_map_prune_params* p, const MapPrunePtrs& d) {
  if (!(f.K && d.T16 && d.stats)) return vo_fail(VO_ERR_INVALID_ARG, "%s: null argument", fn);
  if (int r = map_frames_check(fn, f, d.stats)) return r;
  if (!p || !d.entry) return vo_fail(VO_ERR_INVALID_ARG, "%s: null params or d_entry_out", fn);
  if (!(p->max_err_px >= 0.f && p->max_err_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_err_px must be finite and not negative", fn);
  if (!(p->rel_factor >= 0.f && p->rel_factor <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: rel_factor must be finite and not negative", fn);
  if (!(p->rel_floor_px >= 0.f && p->rel_floor_px <= 3.402823466e38f)) return vo_fail(VO_ERR_INVALID_ARG, "%s: rel_floor_px must be finite and not negative", fn);
  if (p->rel_min_obs < 3) return vo_fail(VO_ERR_INVALID_ARG, "%s: rel_min_obs must be at least 3", fn);
  if (p->max_share_landmark < 0 || p->max_share_landmark > 1000) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_share_landmark %d outside 0 .. 1000", fn, p->max_share_landmark);
  if (p->max_share_frame < 0 || p->max_share_frame > 1000) return vo_fail(VO_ERR_INVALID_ARG, "%s: max_share_frame %d outside 0 .. 1000", fn, p->max_share_frame);
  if (p->unique != 0 && p->unique != 1) return vo_fail(VO_ERR_INVALID_ARG, "%s: unique must be 0 or 1", fn);
  if (p->reserved != 0) return vo_fail(VO_ERR_INVALID_ARG, "%s: reserved must be 0", fn);
  if ((reinterpret_cast<uintptr_t>(d.entry) | reinterpret_cast<uintptr_t>(d.status)) & 3u)
    return vo_fail(VO_ERR_INVALID_ARG, "%s: int32 arrays must be 4-byte aligned", fn);
  if (!aligned8(d.sq, d.app_out, d.landmark, d.frame)) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_sq_out, d_app_out, d_landmark_out and d_frame_out must be 8-byte aligned", fn);
  if (d.app_out && d.app_out != (const void*)f.d_app && f.n_max > 0) {
    const uintptr_t span = sizeof(float) * 10 * ((uintptr_t)(f.n_frames - 1) * f.app_stride + (uintptr_t)f.n_max);
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.d_app), b = reinterpret_cast<uintptr_t>(d.app_out);
    if (a < b + span && b < a + span) return vo_fail(VO_ERR_INVALID_ARG, "%s: d_app_out overlaps d_app without being d_app", fn);
  }
  return VO_OK;
}

// A workspace that would have to grow inside a graph capture: growing frees, allocates and waits.  `ws` lists the buffers the
// call sizes, each with its capacity and what the call needs; `tail` (printf form) names the call that sizes them outside a
// capture.  The callers ask BEFORE they enqueue anything: a HIP call refused later would invalidate the capture.
struct WsNeed { size_t cap, need; };
static inline int capture_growth_check(bool capturing, const char* fn, std::initializer_list<WsNeed> ws, const char* tail, ...) {
  bool fits = true;
  for (const WsNeed& w : ws) fits = fits && w.cap >= w.need;
  if (!capturing || fits) return VO_OK;
  char with[160];
  va_list ap;
  va_start(ap, tail);
  vsnprintf(with, sizeof(with), tail, ap);
  va_end(ap);
  return vo_fail(VO_ERR_NOT_READY, "%s: the workspace would have to grow inside a graph capture (make one call with %s before capturing)", fn, with);
}

// ---- the host's bound of a map's size --------------------------------------------------------------------------------------
// Every call that must not wait for the device sizes its launches and workspaces by a number the host keeps; the kernels read the
// true size from the map's header and clamp it by that number (MapView::size()), so an entry at or above the number is skipped
// without a word.  THE RULE: bound() >= the size the device holds whenever a call is enqueued, and launch_bound() >= the size the
// device holds whenever that call RUNS.  The two differ for a call enqueued inside a graph capture: the graph may hold an update
// BEHIND the call (the per-frame shape { window call ; update }), whose replays add entries before the call's next replay runs.
// One transition per event that changes what the host knows; capi_map.hip makes no assignment of its own, and
// tests/hostcheck/map_bound_check.cpp drives the transitions next to a brute-force model of the true size.
struct MapBound {
  long long size_ub = 0;        // upper bound of the size known without asking the device, as long as !replayable
  bool replayable = false;      // an update (or a grow that adds) of this map has been captured: replays add entries the host never counts
  int cap = 0;                  // the arrays' capacity: no size passes it (what does not fit is dropped and counted)

  // what bounds the size where the host must not wait: size_ub, or the capacity once replays may have outrun it
  int bound() const { return (int)(replayable || size_ub > cap ? cap : size_ub); }
  // what sizes the launches of a call enqueued now on the map's own entries (refinement, pose refinement, adjustment, bundle,
  // cull, transform): inside a capture the capacity, because the call runs again after whatever the rest of the graph appends
  int launch_bound(bool capturing) const { return capturing ? cap : bound(); }
  // what sizes the ALLOCATION of a workspace indexed by entry: always the capacity, so that the call can be captured later
  // without growing the workspace ("one eager call, then capture") whatever bound the capture then bakes in
  int alloc_bound() const { return cap; }
  // room for n more entries without asking the device?  (a map whose update has been captured asks every time outside a capture;
  // inside one nobody can ask, and the bound decides)
  bool room_known(bool capturing, int n) const { return (capturing || !replayable) && size_ub + n <= cap; }

  void on_clear() { size_ub = 0; }                                                // (a captured update stays captured)
  void on_arrays(int new_cap) { cap = new_cap; }                                  // created, or grown on the host
  void on_size_read(int size) { size_ub = size; }                                 // the host has read the header, the stream idle
  void on_update(int n, bool capturing) { size_ub += n; if (capturing) replayable = true; }      // n rows enqueued: at most n new entries
  void on_grow(int room, bool capturing, bool dry) { if (!dry) on_update(room, capturing); }     // at most `room` tracks appended
  // the host forms that have waited for their statistics: the size they report IS the size, unless replays may run unseen
  void on_host_cull(int n_kept, bool dry) { if (!replayable && !dry) size_ub = n_kept; }
  void on_host_grow(int n_after, bool dry) { if (!replayable && !dry) size_ub = n_after; }
  void on_host_merge(int n_dst_after) { if (!replayable) size_ub = n_dst_after; }
};
